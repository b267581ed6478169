"""CPU checks of calibrated verification's host side: the three new C entries (in the header, exported,
bound), the workspace convention and the argument checks of rr_verify_pairs_essential /
rr_essential_5pt (they return before anything is enqueued, so they run without a GPU), the Python
surface's refusals, fundamental_from_essential against the reference's formula, the essential.npz
fixture against the numpy restatement of tests/essential_cases.py, and the two minimal solvers of that
restatement against each other."""

import ctypes
import functools
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import epipolar_cases as EC
import essential_cases as SC
from conftest import PKG, REPO, golden

HEADER = os.path.join(REPO, "include", "rr.h")
LIB = os.path.join(PKG, "librr.so")
NEW = ("rr_verify_essential_workspace_bytes", "rr_verify_pairs_essential", "rr_essential_5pt")
P = ctypes.c_void_p(0x1000)   # "non-null, aligned"; never dereferenced
NULL = ctypes.c_void_p(0)


def _lib():
    from cirtorch import _engine
    return _engine.lib()


# ---------------------------------------------------------------- the ABI
def test_new_symbols_in_header_exported_and_bound():
    from cirtorch import _engine, _ops
    import cirtorch.geometry.epipolar as E
    text = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(rr_\w+)\b", out))
    for name in NEW:
        assert re.search(r"^\s*(?:size_t|int)\s+%s\s*\(" % name, text, flags=re.M), name
        assert name in exported and name in _engine._SIGS, name
        assert getattr(_engine.lib(), name) is not None
    assert _ops.VERIFY_MODELS["essential"] == ("rr_verify_essential_workspace_bytes", "rr_verify_pairs_essential")
    assert set(_ops.VERIFY_MODELS) == {"homography", "fundamental", "essential"}
    assert callable(_ops.essential_5pt) and callable(E.run_5point) and callable(E.fundamental_from_essential)


# ---------------------------------------------------------------- workspace convention
def _need(lib, rows1, npairs, iters):
    return lib.rr_verify_essential_workspace_bytes(rows1, npairs, iters)


def _call(lib, ws, wsb, rows1, npairs, iters):
    return lib.rr_verify_pairs_essential(P, P, rows1, P, P, rows1, P, npairs, 1, P, P, 1.5, iters, 1, 7, P, P, P, ws, wsb, NULL)


def test_short_and_null_workspace_are_refused():
    lib = _lib()
    shape = dict(rows1=12, npairs=3, iters=300)
    need = _need(lib, **shape)
    assert need >= 256 and need % 256 == 0, need
    assert need >= 12 * 32 + 3 * 4 + 3 * 2 * 8     # records, counts, one key per (pair, chunk of 256)
    assert need == lib.rr_verify_epipolar_workspace_bytes(12, 3, 300)   # the one layout function
    for ws, wsb in ((P, need - 1), (NULL, need), (P, 0)):
        assert _call(lib, ws, wsb, **shape) == -3, wsb                                # RR_ENOSPACE
        msg = lib.rr_last_error().decode()
        assert msg.startswith("rr_verify_pairs_essential") and "workspace" in msg, msg
    assert _call(lib, P, need, rows1=12, npairs=0, iters=300) == 0                    # nothing to launch


def test_need_is_monotone_in_every_size():
    lib = _lib()
    grid = dict(rows1=(1, 12, 4096), npairs=(1, 3, 100), iters=(1, 256, 257, 300, 65536))
    keys = sorted(grid)
    need = {pt: _need(lib, **dict(zip(keys, pt))) for pt in itertools.product(*(grid[k] for k in keys))}
    for pt, b in need.items():
        assert b % 256 == 0 and b < 1 << 48, (pt, b)
        for i, k in enumerate(keys):
            j = grid[k].index(pt[i])
            if j + 1 < len(grid[k]):
                assert need[pt[:i] + (grid[k][j + 1],) + pt[i + 1:]] >= b, (keys, pt)


# ---------------------------------------------------------------- argument refusals
def test_argument_checks():
    """every refusal happens on the host: made-up device addresses, nothing is launched"""
    lib = _lib()
    need = _need(lib, 10, 2, 512)

    def verify(kp1=P, off1=P, kp2=P, off2=P, match=P, rows1=10, npairs=2, max_n1=10, K1=P, K2=P, th=1.5, iters=512, refine=2,
               inl=P, E=P, mask=P, ws=P, wsb=need):
        return lib.rr_verify_pairs_essential(kp1, off1, rows1, kp2, off2, 12, match, npairs, max_n1, K1, K2, th, iters, refine,
                                             7, inl, E, mask, ws, wsb, NULL)

    bad = [dict(kp1=NULL), dict(kp2=NULL), dict(off1=NULL), dict(off2=NULL), dict(match=NULL), dict(inl=NULL),
           dict(E=NULL), dict(mask=NULL), dict(ws=NULL), dict(iters=0), dict(iters=-5), dict(iters=(1 << 24) + 1),
           dict(refine=-1), dict(th=0.0), dict(th=-1.0), dict(th=float("inf")), dict(th=float("nan")),
           dict(wsb=need - 257), dict(wsb=0), dict(max_n1=11), dict(max_n1=-1), dict(rows1=-1), dict(npairs=-1),
           dict(kp1=ctypes.c_void_p(0x1004)), dict(K1=NULL), dict(K2=NULL), dict(K1=ctypes.c_void_p(0x1008)),
           dict(K2=ctypes.c_void_p(0x1008))]
    for kw in bad:
        assert verify(**kw) in (-1, -3), kw     # RR_EINVAL / RR_ENOSPACE, never RR_EHIP: no launch was attempted
        assert lib.rr_last_error().decode().startswith("rr_verify_pairs_essential"), kw
    for kw in (dict(K1=NULL), dict(K2=ctypes.c_void_p(0x1008))):
        assert verify(**kw) == -1 and " K" in lib.rr_last_error().decode(), kw        # RR_EINVAL
    # a null output is refused by its own check (RR_EINVAL, "null output"), not by a launch that fails for want
    # of a GPU: nothing is enqueued.  The same check serves the two other models.
    for kw in (dict(inl=NULL), dict(E=NULL), dict(mask=NULL)):
        assert verify(**kw) == -1 and lib.rr_last_error().decode() == "rr_verify_pairs_essential: null output", kw
    for name, fn in (("rr_verify_pairs", lib.rr_verify_pairs), ("rr_verify_pairs_epipolar", lib.rr_verify_pairs_epipolar)):
        for inl, M, mask in ((NULL, P, P), (P, NULL, P), (P, P, NULL)):
            assert fn(P, P, 10, P, P, 12, P, 2, 10, 1.5, 512, 2, 7, inl, M, mask, P, need, NULL) == -1, name
            assert lib.rr_last_error().decode() == name + ": null output"
    assert verify(npairs=0) == 0
    assert lib.rr_verify_pairs_essential(NULL, P, 0, NULL, P, 0, NULL, 0, 0, NULL, NULL, 1.5, 1, 0, 0, NULL, NULL, NULL, P, 256,
                                         NULL) == 0

    def five(x1=P, x2=P, n=3, E=P, nroots=P):
        return lib.rr_essential_5pt(x1, x2, n, E, nroots, NULL)

    for kw in [dict(x1=NULL), dict(x2=NULL), dict(E=NULL), dict(nroots=NULL), dict(n=-1), dict(x1=ctypes.c_void_p(0x1008)),
               dict(x2=ctypes.c_void_p(0x1008))]:
        assert five(**kw) == -1, kw                                                   # RR_EINVAL: refused, not launched
        assert lib.rr_last_error().decode().startswith("rr_essential_5pt"), kw
    assert five(n=0) == 0 and five(n=0, x1=NULL, x2=NULL, E=NULL, nroots=NULL) == 0


def test_python_refusals():
    from cirtorch.geometry.epipolar import run_5point
    from cirtorch.search import verify_pairs
    k1, k2, m = torch.zeros(2, 9, 2), torch.zeros(2, 10, 2), torch.zeros(2, 9, dtype=torch.int64)
    K = torch.eye(3, dtype=torch.float64)
    with pytest.raises(ValueError, match="model"):
        verify_pairs(k1, k2, m, model="nope")
    with pytest.raises(ValueError, match="K1"):                      # missing K
        verify_pairs(k1, k2, m, model="essential")
    with pytest.raises(ValueError, match="K1"):
        verify_pairs(k1, k2, m, model="essential", K1=K)
    for model in ("homography", "fundamental"):                      # K with another model
        with pytest.raises(ValueError, match="essential"):
            verify_pairs(k1, k2, m, model=model, K1=K, K2=K)
    for bad in (torch.eye(4, dtype=torch.float64), torch.zeros(3, 3, 3, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="K1"):                  # wrong K shape (P = 2)
            verify_pairs(k1, k2, m, model="essential", K1=bad, K2=K)
    for kw in (dict(iters=0), dict(refine=-1), dict(th=0.0), dict(max_n1=5), dict(offsets1=torch.tensor([0, 9, 18]))):
        with pytest.raises(ValueError):
            verify_pairs(k1, k2, m, model="essential", K1=K, K2=K, **kw)
    # the kernel-backed functions raise on CPU tensors, like the rest of the package
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        verify_pairs(k1, k2, m, model="essential", K1=K, K2=K)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        verify_pairs(k1.view(18, 2), k2.view(20, 2), m.view(18), offsets1=torch.tensor([0, 9, 18]),
                     offsets2=torch.tensor([0, 10, 20]), model="essential", K1=K, K2=torch.stack([K, K]))
    x = torch.zeros(4, 5, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        run_5point(x, x)
    for a, b in ((x[:, :4], x[:, :4]), (x, x[:3]), (x, x.float()), (x.long(), x.long()), (x[0], x[0])):
        with pytest.raises(ValueError):
            run_5point(a, b)


def test_fundamental_from_essential_is_the_reference_formula():
    """F = K2^-T E K1^-1 (fundamental.py:111-122 of the reference), the inverse of essential_from_fundamental"""
    from cirtorch.geometry.epipolar import essential_from_fundamental, fundamental_from_essential
    r = np.random.default_rng(3)
    E = r.standard_normal((4, 3, 3))
    K1 = np.stack([SC.K, SC.K2B, SC.K + r.uniform(-1, 1, (3, 3)), SC.K2B])
    K2 = np.stack([SC.K2B, SC.K, SC.K, SC.K2B + r.uniform(-1, 1, (3, 3))])
    F = fundamental_from_essential(torch.from_numpy(E), torch.from_numpy(K1), torch.from_numpy(K2))
    want = np.stack([np.linalg.inv(K2[i]).T @ E[i] @ np.linalg.inv(K1[i]) for i in range(4)])
    assert F.dtype == torch.float64
    np.testing.assert_allclose(F.numpy(), want, rtol=1e-12, atol=1e-18)
    back = essential_from_fundamental(F, torch.from_numpy(K1), torch.from_numpy(K2)).numpy()
    np.testing.assert_allclose(back, E, rtol=0, atol=1e-9)
    one = fundamental_from_essential(torch.from_numpy(E[0]), torch.from_numpy(K1[0]), torch.from_numpy(K2[0]))
    np.testing.assert_allclose(one.numpy(), want[0], rtol=1e-12, atol=1e-18)
    for args in ((torch.zeros(3, 4), torch.eye(3), torch.eye(3)), (torch.zeros(2, 3, 3), torch.eye(3), torch.eye(3))):
        with pytest.raises(ValueError):
            fundamental_from_essential(*args)


# ---------------------------------------------------------------- the fixture against the restatement
@functools.lru_cache(maxsize=None)
def ecase(k):
    g = golden("essential.npz")
    case = SC.ALL_CASES[k]
    kp1, off1, kp2, off2, match, planted, K1, K2, parts = SC.build_case(case, int(g["c_seeds"][k]))
    np.testing.assert_allclose(SC.checksum(kp1, kp2, match), g["c_chk"][k], rtol=0, atol=1e-6)
    return case, (kp1, off1, kp2, off2, match, planted, K1, K2), SC.essential_batch(
        kp1, off1, kp2, off2, match, K1, K2, SC.TH, case["iters"], case["refine"], SC.RUN_SEED)


def test_cases_cover_what_the_kernels_branch_on():
    ms = [[q[2] for q in c["pairs"]] for c in SC.ESS_CASES]
    for m in ([0], [4], [5], [8], [40], [257], [SC.STAGE + 1]):
        assert m in ms, m
    assert {c["iters"] for c in SC.ESS_CASES} >= {1, 257} and max(c["iters"] for c in SC.ESS_CASES) <= 512
    assert {c["refine"] for c in SC.ESS_CASES if c["pairs"][0][2] == 257} == {0, 2}
    kinds = {q[5] for c in SC.ESS_CASES for q in c["pairs"]}
    assert SC.TH == 1.5 and kinds == {"general", "planar", "twocam", "singular"}
    by = {c["name"]: c for c in SC.ESS_CASES}
    assert [q[2] for q in by["ragged4"]["pairs"]] == [0, 3, 60, 50] and by["outliers"]["pairs"][0][3] == 0.0
    assert by["planar"]["pairs"][0][2] == 60 and by["twocam"]["pairs"][0][2] == 60
    assert [q[5] for q in by["singularK"]["pairs"]].count("singular") == 1 and len(by["singularK"]["pairs"]) == 4


@pytest.mark.parametrize("k", range(len(SC.ALL_CASES)))
def test_restatement_equals_fixture(k):
    g = golden("essential.npz")
    case, (kp1, off1, kp2, off2, match, planted, K1, K2), (inl, Es, mask, infos) = ecase(k)
    assert kp1.dtype == np.float32 and kp2.dtype == np.float32 and match.dtype == np.int64
    np.testing.assert_array_equal(inl, g["c%d_inl" % k])
    np.testing.assert_array_equal(mask, g["c%d_mask" % k])
    np.testing.assert_array_equal([o["t"] for o in infos], g["c%d_t" % k])
    np.testing.assert_array_equal([o["root"] for o in infos], g["c%d_root" % k])
    for p, o in enumerate(infos):
        assert o["m"] == case["pairs"][p][2]
        assert int(mask[off1[p]:off1[p + 1]].sum()) == inl[p]
        if inl[p]:
            assert o["margin"] >= 1e-7
            sv = np.linalg.svd(Es[p], compute_uv=False)
            assert abs(np.sqrt((Es[p] ** 2).sum()) - 1) < 1e-14 and Es[p].reshape(-1)[np.argmax(np.abs(Es[p]))] > 0
            assert abs(sv[0] - sv[1]) < 1e-14 and sv[2] < 1e-14
            assert EC.f_err(Es[p], g["c%d_E" % k][p]) <= g["c%d_tol" % k][p]
        else:
            assert not Es[p].any() and not g["c%d_E" % k][p].any() and o["t"] == -1
    if case["name"] == "singularK":
        assert inl[1] == 0 and min(inl[0], inl[2], inl[3]) >= 18
    if case["name"] == "planar":
        assert g["planar_false"][0] == int((mask & ~planted).sum()) <= g["planar_false"][1]


def test_minimal_solvers_agree_and_fit_their_samples():
    """solvers A and B give the same solutions in the same order, every solution passes through its five
    points and is an essential matrix; the fixture's bounds come from them"""
    g = golden("essential.npz")
    x1, x2, E, nroots, drop, diffs, resid = SC.solver_samples(int(g["s_seed"]))
    np.testing.assert_allclose(SC.checksum(x1, x2), g["s_chk"], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(nroots, g["s_nroots"])
    assert drop == g["s_drop"] <= 0.02 and len(x1) > 256
    np.testing.assert_allclose(np.maximum(100 * diffs, 1e-12), g["s_tol"], rtol=1e-6, atol=0)
    assert 100 * resid == pytest.approx(float(g["s_resid"]), rel=1e-6) and resid < 1e-14
    assert set(nroots.tolist()) <= {0, 2, 4, 6, 8, 10} and nroots.min() >= 2
    for t in range(0, len(x1), 8):
        for k in range(nroots[t]):
            sv = np.linalg.svd(E[t, k], compute_uv=False)
            assert abs(sv[0] - sv[1]) < 1e-6 * max(1.0, 1e8 * diffs[t]) and sv[2] < 1e-6 * max(1.0, 1e8 * diffs[t])
        assert not E[t, nroots[t]:].any()


def test_draw5_is_a_prefix_rule():
    """five distinct in-range indices whose first four are the homography's"""
    import verify_cases as VC
    for m in (5, 8, 40, 257, 1025):
        s5 = EC.draw_n(99, 3, np.arange(200), m, 5)
        np.testing.assert_array_equal(s5[:, :4], VC.draw4(99, 3, np.arange(200), m))
        assert s5.min() >= 0 and s5.max() < m and all(len(set(r)) == 5 for r in s5.tolist())
