"""Every entry that takes a workspace, run with exactly the bytes its *_workspace_bytes asks for at a
base that is not 256-aligned, between guard bytes: the results equal those of the ordinary call (which
allocates its own, aligned workspace) and no guard byte changes.

The guarded call is the `_ops` wrapper itself with its allocation replaced: the library is handed
base + 64 and workspace_bytes = need, nothing more.  The guards are allocated bytes of the same tensor,
so a layout that overran its size would show here without faulting."""

import numpy as np
import pytest
import torch

import pyrpatch_cases as PC

pytestmark = pytest.mark.gpu

FRONT, BACK, FILL = 64, 4096, 0xA5


class Guarded:
    """stands in for _ops._workspace: FRONT guard bytes, the workspace, BACK guard bytes"""

    def __init__(self):
        self.bufs = []

    def __call__(self, nbytes, device):
        need = int(nbytes)
        assert need > 0
        buf = torch.full((FRONT + need + BACK,), FILL, dtype=torch.uint8, device=device)
        assert buf.data_ptr() % 256 == 0 and (buf.data_ptr() + FRONT) % 256 != 0
        self.bufs.append((buf, need))
        return buf[FRONT:FRONT + need]

    def check(self):
        assert self.bufs, "the entry asked for no workspace"
        for buf, need in self.bufs:
            assert bool((buf[:FRONT] == FILL).all()) and bool((buf[FRONT + need:] == FILL).all()), need


def both(monkeypatch, fn):
    """fn() with the ordinary workspace, then between guards; the outputs must be equal"""
    from cirtorch import _ops
    ref = fn()
    g = Guarded()
    monkeypatch.setattr(_ops, "_workspace", g)
    got = fn()
    torch.cuda.synchronize()
    g.check()
    flat = lambda r: [r] if torch.is_tensor(r) else [t for x in r for t in flat(x)] if isinstance(r, (tuple, list)) else []
    a, b = flat(ref), flat(got)
    assert len(a) == len(b) > 0
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def rand(cuda, seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).random(shape, dtype=np.float32)).to(cuda)


def rows(cuda, seed, n, d):
    x = torch.from_numpy(np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32))
    return (x / x.norm(dim=1, keepdim=True)).to(cuda)


def ss_image(cuda):
    return (rand(cuda, 11, 2, 3, 40, 56) * 255).to(torch.uint8)     # octaves 40 x 56 and 20 x 28


def test_detect_keypoints(cuda, monkeypatch):
    from cirtorch import _ops
    x = rand(cuda, 1, 2, 1, 33, 47)
    both(monkeypatch, lambda: _ops.detect_keypoints(x, 64, kind="harris", ks=5))


@pytest.mark.parametrize("kind", ["hessian", "dog"])
def test_detect_scale_space(cuda, monkeypatch, kind):
    from cirtorch import _ops
    x = ss_image(cuda)

    # the pyramid too: it is read back from the 256-aligned start of the workspace
    both(monkeypatch, lambda: _ops.detect_scale_space(x, 64, kind=kind, levels=3, min_size=15, return_pyramid=True))


def test_scale_pyramid(cuda, monkeypatch):
    from cirtorch import _ops
    x = ss_image(cuda)
    both(monkeypatch, lambda: _ops.scale_pyramid(x, levels=3, min_size=15)[0])


def test_describe_keypoints_pyramid(cuda, monkeypatch):
    from cirtorch import _ops
    x = torch.from_numpy(PC.coarse_images(PC.MAIN, PC.SEED)).to(cuda)           # 2 x 1 x 97 x 131
    lafs = torch.from_numpy(PC.frames(PC.MAIN, PC.NPTS, PC.SEED)).to(cuda)      # scales over levels 0 .. 2 and past
    both(monkeypatch, lambda: _ops.describe_keypoints(x, lafs=lafs, orient=True, ps=16, return_lafs=True, pyramid=True))


def test_laf_affine_shape(cuda, monkeypatch):
    from cirtorch import _ops
    x = torch.from_numpy(PC.coarse_images(PC.MAIN, PC.SEED)).to(cuda)
    lafs = torch.from_numpy(PC.frames(PC.MAIN, PC.NPTS, PC.SEED)).to(cuda)
    both(monkeypatch, lambda: _ops.laf_affine_shape(x, lafs, ps=16))


@pytest.mark.parametrize("mode", ["nn", "smnn"])
def test_match_pairs(cuda, monkeypatch, mode):
    from cirtorch import _ops
    a, b = rows(cuda, 3, 10, 8), rows(cuda, 4, 12, 8)
    a_off = torch.tensor([0, 3, 4, 10], dtype=torch.int64, device=cuda)          # ragged: 3, 1 and 6 rows
    b_off = torch.tensor([0, 5, 7, 12], dtype=torch.int64, device=cuda)
    both(monkeypatch, lambda: _ops.match_pairs(a, a_off, b, b_off, mode, th=0.95))


def test_verify_pairs(cuda, monkeypatch):
    from cirtorch import _ops
    kp1 = rand(cuda, 5, 12, 2) * 100
    kp2 = kp1 * 1.1 + 3 + rand(cuda, 6, 12, 2)
    off = torch.tensor([0, 5, 6, 12], dtype=torch.int64, device=cuda)
    match = torch.cat([torch.arange(5), torch.tensor([-1]), torch.arange(6)]).to(cuda)   # indices within each pair
    both(monkeypatch, lambda: _ops.verify_pairs(kp1, off, kp2, off, match, iters=300, seed=9))   # two chunks


def test_knn_topk_checked(cuda, monkeypatch):
    from cirtorch import _ops
    db, q = rows(cuda, 7, 5000, 64), rows(cuda, 8, 4, 64)
    both(monkeypatch, lambda: _ops.knn_topk(db, db, q, q, 10, db_norm_max=1.0))


def test_rank_full(cuda, monkeypatch):
    from cirtorch import _ops
    db, q = rows(cuda, 9, 5000, 256), rows(cuda, 10, 3, 256)
    both(monkeypatch, lambda: _ops.rank_full(db, q))


def test_local_head(cuda, monkeypatch):
    from cirtorch import _ops
    x = rand(cuda, 12, 1, 16, 8, 8)          # NCHW view of the 1 x 8 x 8 x 16 map
    kpts = rand(cuda, 13, 1, 5, 2) * 2 - 1
    wt, bias = rand(cuda, 14, 8, 16) - 0.5, rand(cuda, 15, 8)
    both(monkeypatch, lambda: _ops.local_head(x, kpts, wt, bias))
