"""CPU checks of the workspace convention of every entry that takes one: a workspace one byte short of
what *_workspace_bytes asks for, and a null one, are refused with RR_ENOSPACE before anything is
enqueued (the calls pass made-up device addresses and run without a GPU), and the size asked for
never shrinks when a size argument grows."""

import ctypes
import itertools
import os

import pytest

from conftest import PKG

LIB = os.path.join(PKG, "librr.so")
P = ctypes.c_void_p(0x1000)   # "non-null, aligned"; never dereferenced
NULL = ctypes.c_void_p(0)
SS = (3, 1.6, 15)             # levels, sigma, min_size: 40 x 56 gives the octaves 40 x 56 and 20 x 28


def _lib():
    if not os.path.exists(LIB):
        pytest.skip("librr.so not built (run __graft_entry__.build())")
    from cirtorch import _engine
    return _engine.lib()


def _pyramid_bytes(lib, n, c=3, h=40, w=56):
    ob, wb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.rr_scale_pyramid_bytes(n, c, h, w, *SS, ctypes.byref(ob), ctypes.byref(wb)) == 0
    return ob.value, wb.value


# name -> (need(lib, **sizes), call(lib, ws, wsb, **sizes), the family's test shape, the grid of the monotonicity check)
CASES = {
    "rr_knn_topk": (
        lambda lib, n_db, nq, d, k: lib.rr_knn_workspace_bytes(n_db, nq, d, k, 0, 0),
        lambda lib, ws, wsb, n_db, nq, d, k: lib.rr_knn_topk(P, P, n_db, P, P, nq, d, k, 0, 0, P, P, ws, wsb, 0, NULL),
        dict(n_db=5000, nq=4, d=64, k=10), dict(n_db=(1, 5000, 16384, 16385, 100000), nq=(1, 4, 128), d=(64,), k=(1, 10, 100))),
    "rr_knn_topk_checked": (
        lambda lib, n_db, nq, d, k: lib.rr_knn_workspace_bytes(n_db, nq, d, k, 0, 1),
        lambda lib, ws, wsb, n_db, nq, d, k: lib.rr_knn_topk_checked(P, P, n_db, P, P, nq, d, k, 0, 0, P, P, ws, wsb, 1, 1.0,
                                                                    P, NULL),
        dict(n_db=5000, nq=4, d=64, k=10), dict(n_db=(1, 5000, 1000000), nq=(1, 4, 1024), d=(64,), k=(10, 100))),
    "rr_rank_full": (
        lambda lib, n, nq: lib.rr_rank_workspace_bytes(n, nq),
        lambda lib, ws, wsb, n, nq: lib.rr_rank_full(P, n, P, nq, 256, P, ws, wsb, NULL),
        dict(n=5000, nq=3), dict(n=(1, 4096, 5000, 100000), nq=(1, 3, 70))),
    "rr_local_head": (
        lambda lib, n, npts, c, e: lib.rr_local_head_workspace_bytes(n * npts, c, e),
        lambda lib, ws, wsb, n, npts, c, e: lib.rr_local_head(P, n, 8, 8, c, 0, P, npts, P, P, e, P, ws, wsb, NULL),
        dict(n=1, npts=5, c=16, e=8), dict(n=(1, 2, 8), npts=(1, 5, 2048), c=(16, 1024), e=(8, 128))),
    "rr_match_top2": (
        lambda lib, rows1, rows2: lib.rr_match_workspace_bytes(rows1, rows2, 0),
        lambda lib, ws, wsb, rows1, rows2: lib.rr_match_top2(P, P, rows1, P, P, rows2, 3, 8, 1, 1, P, P, P, P, ws, wsb, NULL),
        dict(rows1=10, rows2=12), dict(rows1=(1, 10, 33, 4096), rows2=(1, 12, 4096))),
    "rr_match_pairs": (
        lambda lib, rows1, rows2: lib.rr_match_workspace_bytes(rows1, rows2, 1),
        lambda lib, ws, wsb, rows1, rows2: lib.rr_match_pairs(P, P, rows1, P, P, rows2, 3, 8, 1, 1, 3, 0.8, P, P, ws, wsb,
                                                              NULL),
        dict(rows1=10, rows2=12), dict(rows1=(1, 10, 33, 4096), rows2=(1, 12, 4096))),
    "rr_verify_pairs": (
        lambda lib, rows1, npairs, iters: lib.rr_verify_workspace_bytes(rows1, npairs, iters),
        lambda lib, ws, wsb, rows1, npairs, iters: lib.rr_verify_pairs(P, P, rows1, P, P, rows1, P, npairs, 1, 3.0, iters, 1,
                                                                       7, P, P, P, ws, wsb, NULL),
        dict(rows1=12, npairs=3, iters=300), dict(rows1=(1, 12, 4096), npairs=(1, 3, 100), iters=(1, 256, 257, 300, 65536))),
    "rr_select_keypoints": (
        lambda lib, n, h, w: lib.rr_detect_workspace_bytes(n, h, w, 64),
        lambda lib, ws, wsb, n, h, w: lib.rr_select_keypoints(P, n, h, w, 5, 64, 0.0, 0, P, P, P, ws, wsb, NULL),
        dict(n=2, h=33, w=47), dict(n=(0, 1, 2, 128), h=(16, 33, 768), w=(16, 47, 1024))),
    "rr_detect_keypoints": (
        lambda lib, n, h, w: lib.rr_detect_workspace_bytes(n, h, w, 64),
        lambda lib, ws, wsb, n, h, w: lib.rr_detect_keypoints(P, n, 1, h, w, 0, 0, 0.04, NULL, 5, 64, 0.0, 0, P, P, P, NULL,
                                                              ws, wsb, NULL),
        dict(n=2, h=33, w=47), dict(n=(0, 1, 2), h=(16, 33), w=(16, 47))),
    "rr_scale_pyramid": (
        lambda lib, n, h, w: _pyramid_bytes(lib, n, 3, h, w)[1],
        lambda lib, ws, wsb, n, h, w: lib.rr_scale_pyramid(P, n, 3, h, w, 1, *SS, P, _pyramid_bytes(lib, n, 3, h, w)[0], ws,
                                                           wsb, NULL),
        dict(n=2, h=40, w=56), dict(n=(0, 1, 2, 128), h=(40, 97, 768), w=(56, 131, 1024))),
    "rr_detect_scale_space": (
        lambda lib, n, h, w: lib.rr_detect_scale_space_workspace_bytes(n, 3, h, w, *SS),
        lambda lib, ws, wsb, n, h, w: lib.rr_detect_scale_space(P, n, 3, h, w, 1, *SS, 2, 0.04, 0, 6.0, 64, P, P, P, ws, wsb,
                                                                NULL),
        dict(n=2, h=40, w=56), dict(n=(0, 1, 2, 128), h=(40, 97, 768), w=(56, 131, 1024))),
    "rr_describe_keypoints": (
        lambda lib, n, npts: lib.rr_describe_workspace_bytes(n, npts, 16, 8, 4),
        lambda lib, ws, wsb, n, npts: lib.rr_describe_keypoints(P, n, 1, 97, 131, 0, P, NULL, npts, 6.0, NULL, 1, 36, 16, 8, 4,
                                                                1, 0.2, P, NULL, NULL, ws, wsb, NULL),
        dict(n=2, npts=24), dict(n=(0, 1, 2, 128), npts=(0, 24, 2048))),
    "rr_describe_keypoints_pyramid": (
        lambda lib, n, h, w: lib.rr_describe_pyramid_workspace_bytes(n, 1, h, w, 24, 16, 8, 4),
        lambda lib, ws, wsb, n, h, w: lib.rr_describe_keypoints_pyramid(P, n, 1, h, w, 0, P, NULL, 24, 6.0, NULL, 1, 36, 16, 8,
                                                                        4, 1, 0.2, P, NULL, NULL, ws, wsb, NULL),
        dict(n=2, h=97, w=131), dict(n=(0, 1, 2, 128), h=(16, 31, 32, 97, 768), w=(16, 33, 131, 1024))),
    "rr_laf_affine_shape": (
        lambda lib, n, h, w: lib.rr_laf_affine_shape_workspace_bytes(n, 1, h, w, 24, 16),
        lambda lib, ws, wsb, n, h, w: lib.rr_laf_affine_shape(P, n, 1, h, w, 0, P, NULL, 24, 16, 1e-6, P, ws, wsb, NULL),
        dict(n=2, h=97, w=131), dict(n=(0, 1, 2, 128), h=(16, 31, 32, 97, 768), w=(16, 33, 131, 1024))),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_short_and_null_workspace_are_refused(name):
    lib = _lib()
    need_of, call, shape, _ = CASES[name]
    need = need_of(lib, **shape)
    assert need >= 256 and need % 256 == 0, need
    for ws, wsb in ((P, need - 1), (NULL, need), (P, 0)):
        assert call(lib, ws, wsb, **shape) == -3, (name, wsb)                       # RR_ENOSPACE
        msg = lib.rr_last_error().decode()
        assert msg.startswith(name.replace("_checked", "")) and "workspace" in msg, msg


def test_scale_space_select_short_and_null_workspace():
    """rr_scale_space_select takes any workspace of rr_detect_scale_space_workspace_bytes and exports no
    size of its own: for an empty batch its layout is the base slack alone (256 bytes, exactly), and for
    n images the candidate keys alone (8 bytes each, rr.h's bound per octave) are more than wsb below"""
    lib = _lib()

    def sel(n, ws, wsb):
        return lib.rr_scale_space_select(P, n, 40, 56, *SS, 0, 6.0, 64, P, P, P, ws, wsb, NULL)

    keys = 2 * 8 * (2 * 3 * 20 * 28 + 2 * 3 * 10 * 14)   # n = 2, D = 5: 2 ceil(D / 2) ceil(h / 2) ceil(w / 2) per octave
    assert keys < lib.rr_detect_scale_space_workspace_bytes(2, 1, 40, 56, *SS)
    for n, ws, wsb in ((0, P, 255), (0, NULL, 256), (2, P, keys), (2, NULL, 1 << 30), (2, P, 0)):
        assert sel(n, ws, wsb) == -3, (n, wsb)
        msg = lib.rr_last_error().decode()
        assert msg.startswith("rr_scale_space_select") and "workspace" in msg, msg
    assert sel(0, P, 256) == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_need_is_monotone_in_every_size(name):
    lib = _lib()
    need_of, _, _, grid = CASES[name]
    keys = sorted(grid)
    need = {pt: need_of(lib, **dict(zip(keys, pt))) for pt in itertools.product(*(grid[k] for k in keys))}
    for pt, b in need.items():
        assert b % 256 == 0 and b < 1 << 48, (name, pt, b)
        for i, k in enumerate(keys):
            j = grid[k].index(pt[i])
            if j + 1 < len(grid[k]):
                up = pt[:i] + (grid[k][j + 1],) + pt[i + 1:]
                assert need[up] >= b, (name, keys, pt, up)
