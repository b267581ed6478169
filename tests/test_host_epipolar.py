"""CPU checks of epipolar verification's host side: the cirtorch.geometry.epipolar package and its
names, the three new C entries (in the header, exported, bound), the workspace convention and the
argument checks of rr_verify_pairs_epipolar / rr_fundamental_dlt / rr_epipolar_distance (they return
before anything is enqueued, so they run without a GPU), the Python surface's refusals, the
epipolar.npz fixture against the numpy restatement of tests/epipolar_cases.py, and the seven-index
draw against draw4."""

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
import verify_cases as VC
from conftest import PKG, REPO, golden

HEADER = os.path.join(REPO, "include", "rr.h")
LIB = os.path.join(PKG, "librr.so")
NEW = ("rr_verify_epipolar_workspace_bytes", "rr_verify_pairs_epipolar", "rr_fundamental_dlt", "rr_epipolar_distance")
P = ctypes.c_void_p(0x1000)   # "non-null, aligned"; never dereferenced
NULL = ctypes.c_void_p(0)


def _lib():
    from cirtorch import _engine
    return _engine.lib()


# ---------------------------------------------------------------- the package and the ABI
def test_package_and_names():
    import cirtorch.geometry.epipolar as E
    from cirtorch.geometry.epipolar import fundamental, metrics
    for name in ("normalize_points", "normalize_transformation", "find_fundamental", "compute_correspond_epilines"):
        assert callable(getattr(fundamental, name)) and getattr(E, name) is getattr(fundamental, name)
    for name in ("sampson_epipolar_distance", "symmetrical_epipolar_distance"):
        assert callable(getattr(metrics, name)) and getattr(E, name) is getattr(metrics, name)


def test_new_symbols_in_header_exported_and_bound():
    from cirtorch import _engine
    text = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(rr_\w+)\b", out))
    for name in NEW:
        assert re.search(r"^\s*(?:size_t|int)\s+%s\s*\(" % name, text, flags=re.M), name
        assert name in exported and name in _engine._SIGS, name
        assert getattr(_engine.lib(), name) is not None
    assert "enum rr_epi_kind { RR_EPI_SAMPSON = 0, RR_EPI_SYMMETRICAL = 1 }" in text
    assert (_engine.RR_EPI_SAMPSON, _engine.RR_EPI_SYMMETRICAL) == (0, 1)


# ---------------------------------------------------------------- workspace convention
def _need(lib, rows1, npairs, iters):
    return lib.rr_verify_epipolar_workspace_bytes(rows1, npairs, iters)


def _call(lib, ws, wsb, rows1, npairs, iters):
    return lib.rr_verify_pairs_epipolar(P, P, rows1, P, P, rows1, P, npairs, 1, 1.5, iters, 1, 7, P, P, P, ws, wsb, NULL)


def test_short_and_null_workspace_are_refused():
    lib = _lib()
    shape = dict(rows1=12, npairs=3, iters=300)
    need = _need(lib, **shape)
    assert need >= 256 and need % 256 == 0, need
    assert need >= 12 * 32 + 3 * 4 + 3 * 2 * 8     # records, counts, one key per (pair, chunk of 256)
    for ws, wsb in ((P, need - 1), (NULL, need), (P, 0)):
        assert _call(lib, ws, wsb, **shape) == -3, wsb                                # RR_ENOSPACE
        msg = lib.rr_last_error().decode()
        assert msg.startswith("rr_verify_pairs_epipolar") and "workspace" in msg, msg
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

    def verify(kp1=P, off1=P, kp2=P, off2=P, match=P, rows1=10, npairs=2, max_n1=10, th=1.5, iters=512, refine=2, inl=P,
               F=P, mask=P, ws=P, wsb=need):
        return lib.rr_verify_pairs_epipolar(kp1, off1, rows1, kp2, off2, 12, match, npairs, max_n1, th, iters, refine, 7,
                                            inl, F, mask, ws, wsb, NULL)

    bad = [dict(kp1=NULL), dict(kp2=NULL), dict(off1=NULL), dict(off2=NULL), dict(match=NULL), dict(inl=NULL),
           dict(F=NULL), dict(mask=NULL), dict(ws=NULL), dict(iters=0), dict(iters=-5), dict(iters=(1 << 24) + 1),
           dict(refine=-1), dict(th=0.0), dict(th=-1.0), dict(th=float("inf")), dict(th=float("nan")),
           dict(wsb=need - 257), dict(wsb=0), dict(max_n1=11), dict(max_n1=-1), dict(rows1=-1), dict(npairs=-1),
           dict(kp1=ctypes.c_void_p(0x1004))]
    for kw in bad:
        assert verify(**kw) != 0, kw
        assert lib.rr_last_error().decode().startswith("rr_verify_pairs_epipolar"), kw
    assert verify(npairs=0) == 0
    assert lib.rr_verify_pairs_epipolar(NULL, P, 0, NULL, P, 0, NULL, 0, 0, 1.5, 1, 0, 0, NULL, NULL, NULL, P, 256, NULL) == 0

    def fund(p1=P, p2=P, w=NULL, off=P, rows=10, npairs=2, F=P):
        return lib.rr_fundamental_dlt(p1, p2, w, off, rows, npairs, F, NULL, 0, NULL)

    for kw in [dict(p1=NULL), dict(p2=NULL), dict(off=NULL), dict(F=NULL), dict(rows=-1), dict(npairs=-1),
               dict(p1=ctypes.c_void_p(0x1008))]:
        assert fund(**kw) != 0, kw
        assert lib.rr_last_error().decode().startswith("rr_fundamental_dlt"), kw
    assert fund(npairs=0) == 0 and fund(npairs=0, F=NULL, w=P) == 0

    def dist(p1=P, p2=P, F=P, off=P, rows=10, npairs=2, kind=0, squared=1, eps=1e-8, out=P):
        return lib.rr_epipolar_distance(p1, p2, F, off, rows, npairs, kind, squared, eps, out, NULL)

    for kw in [dict(p1=NULL), dict(p2=NULL), dict(F=NULL), dict(off=NULL), dict(out=NULL), dict(rows=-1), dict(npairs=-1),
               dict(kind=2), dict(kind=-1), dict(squared=2), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")),
               dict(p2=ctypes.c_void_p(0x1008))]:
        assert dist(**kw) != 0, kw
        assert lib.rr_last_error().decode().startswith("rr_epipolar_distance"), kw
    assert dist(npairs=0) == 0 and dist(npairs=0, F=NULL) == 0


def test_python_refusals():
    from cirtorch.geometry.epipolar import (find_fundamental, sampson_epipolar_distance, symmetrical_epipolar_distance)
    from cirtorch.search import verify_pairs
    k1, k2, m = torch.zeros(2, 9, 2), torch.zeros(2, 10, 2), torch.zeros(2, 9, dtype=torch.int64)
    with pytest.raises(ValueError, match="model"):
        verify_pairs(k1, k2, m, model="nope")
    for kw in (dict(iters=0), dict(refine=-1), dict(th=0.0), dict(max_n1=5), dict(offsets1=torch.tensor([0, 9, 18]))):
        with pytest.raises(ValueError):
            verify_pairs(k1, k2, m, model="fundamental", **kw)
    # the kernel-backed functions raise on CPU tensors, like the rest of the package
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        verify_pairs(k1, k2, m, model="fundamental")
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        verify_pairs(k1.view(18, 2), k2.view(20, 2), m.view(18), offsets1=torch.tensor([0, 9, 18]),
                     offsets2=torch.tensor([0, 10, 20]), model="fundamental")
    w, F = torch.ones(2, 9), torch.zeros(2, 3, 3)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        find_fundamental(k1, k1 + 1, w)
    for fn in (sampson_epipolar_distance, symmetrical_epipolar_distance):
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            fn(k1, k1 + 1, F)
        with pytest.raises(ValueError):
            fn(k1, k1, torch.zeros(3, 3))
    for args in [(k1, k2, w), (k1[:, :7], k1[:, :7], w[:, :7]), (k1[0], k1[0], w), (k1, k1.double(), w),
                 (k1, k1, torch.ones(2, 5)), (k1.long(), k1.long(), w)]:
        with pytest.raises(ValueError):
            find_fundamental(*args)


def test_plain_torch_helpers_equal_numpy():
    """normalize_points, normalize_transformation and compute_correspond_epilines run on any device"""
    from cirtorch.geometry.epipolar import compute_correspond_epilines, normalize_points, normalize_transformation
    p1, p2, _ = EC.fund_points(2, 9, False, 5)
    q, T = normalize_points(torch.from_numpy(p1))
    for i in range(2):
        qn, Tn = EC.normalize_points(p1[i])
        np.testing.assert_allclose(q[i].numpy(), qn, rtol=0, atol=1e-12)
        np.testing.assert_allclose(T[i].numpy(), Tn, rtol=1e-13, atol=0)
    M = torch.tensor([[[2.0, 4.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 2.0]], [[2.0, 4.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]]],
                     dtype=torch.float64)
    N = normalize_transformation(M)
    assert torch.equal(N[1], M[1]) and torch.allclose(N[0], M[0] / (2.0 + 1e-8), rtol=1e-15, atol=0)
    F = torch.from_numpy(np.stack([EC.fundamental(p1[i], p2[i]) for i in range(2)]))
    lines = compute_correspond_epilines(torch.from_numpy(p1), F).numpy()
    for i in range(2):
        l = np.concatenate([p1[i], np.ones((9, 1))], 1) @ F[i].numpy().T
        np.testing.assert_allclose(lines[i], l / np.sqrt(l[:, :1] ** 2 + l[:, 1:2] ** 2), rtol=1e-12, atol=1e-15)
        # a correspondence lies on its epipolar line up to the noise
        assert np.abs((np.concatenate([p2[i], np.ones((9, 1))], 1) * lines[i]).sum(1)).max() < 3.0


# ---------------------------------------------------------------- the fixture against the restatement
@functools.lru_cache(maxsize=None)
def ecase(k):
    g = golden("epipolar.npz")
    case = EC.EPI_CASES[k]
    kp1, off1, kp2, off2, match, planted = EC.build_case(case, int(g["e_seeds"][k]))
    np.testing.assert_allclose(EC.checksum(kp1, kp2, match), g["e_chk"][k], rtol=0, atol=1e-6)
    return case, (kp1, off1, kp2, off2, match, planted), EC.epipolar_batch(kp1, off1, kp2, off2, match, EC.TH, case["iters"],
                                                                           case["refine"], EC.RUN_SEED)


def test_cases_cover_what_the_kernels_branch_on():
    ms = [[q[2] for q in c["pairs"]] for c in EC.EPI_CASES]
    for m in ([0], [6], [7], [8], [40], [257], [EC.STAGE + 1]):
        assert m in ms, m
    assert {c["iters"] for c in EC.EPI_CASES} >= {1, 257} and max(c["iters"] for c in EC.EPI_CASES) <= 512
    assert {c["refine"] for c in EC.EPI_CASES if c["pairs"][0][2] == 257} == {0, 2}
    assert EC.TH == 1.5 and [q[2] for q in EC.EPI_CASES[-1]["pairs"]] == [0, 3, 60, 50]


@pytest.mark.parametrize("k", range(len(EC.EPI_CASES)))
def test_restatement_equals_fixture(k):
    g = golden("epipolar.npz")
    case, (kp1, off1, kp2, off2, match, planted), (inl, Fs, mask, infos) = ecase(k)
    assert kp1.dtype == np.float32 and kp2.dtype == np.float32 and match.dtype == np.int64
    assert kp1.size == 0 or (kp1.min() >= 0 and kp1[:, 0].max() < EC.W and kp1[:, 1].max() < EC.H_IMG)
    np.testing.assert_array_equal(inl, g["e%d_inl" % k])
    np.testing.assert_array_equal(mask, g["e%d_mask" % k])
    np.testing.assert_array_equal([o["t"] for o in infos], g["e%d_t" % k])
    np.testing.assert_array_equal([o["root"] for o in infos], g["e%d_root" % k])
    for p, o in enumerate(infos):
        assert o["m"] == case["pairs"][p][2] and o["margin"] >= 1e-7
        assert int(mask[off1[p]:off1[p + 1]].sum()) == inl[p]
        if inl[p]:
            assert abs(np.sqrt((Fs[p] ** 2).sum()) - 1) < 1e-14 and Fs[p].reshape(-1)[np.argmax(np.abs(Fs[p]))] > 0
            assert EC.f_err(Fs[p], g["e%d_F" % k][p]) <= g["e%d_tol" % k][p]
        else:
            assert not Fs[p].any() and not g["e%d_F" % k][p].any() and o["t"] == -1
    if case["name"] == "ragged4":   # the noise-free pair: exact in float32, every match an inlier
        assert inl.tolist()[:2] == [0, 0] and inl[3] == 50
        a, b = slice(off1[3], off1[4]), slice(off2[3], off2[4])
        rec = np.concatenate([kp1[a], kp2[b][match[a]]], 1).astype(np.float64)[match[a] >= 0]
        assert EC.sampson(Fs[3], rec)[1].max() < 1e-6


@pytest.mark.parametrize("k", range(len(EC.FUND_CASES)))
def test_fit_and_distance_restatements_equal_reference(k):
    """np.linalg.eigh restatement == the reference's float64 torch.svd run; the distances likewise"""
    g = golden("epipolar.npz")
    b, n, weighted = EC.FUND_CASES[k]
    p1, p2, w = EC.fund_points(b, n, weighted, int(g["fund_seeds"][k]))
    np.testing.assert_allclose(EC.checksum(p1, p2, w), g["fund_chk"][k], rtol=0, atol=1e-6)
    assert g["fund_tol"][k] >= 1e-12 and g["fund_tol_d"][k] >= 1e-12
    assert weighted == bool((w != 1).any()) and (not weighted or n < 9 or (w == 0).any())
    for i in range(b):
        Fr = g["fund%d_F" % k][i]
        assert EC.f_err(EC.fundamental(p1[i], p2[i], w[i]), Fr) <= g["fund_tol"][k]
        for key, kind, squared in (("sam", "sampson", True), ("sam_rt", "sampson", False), ("sym", "symmetrical", True),
                                   ("sym_rt", "symmetrical", False)):
            want = g["fund%d_%s" % (k, key)][i]
            got = EC.distance(p1[i], p2[i], Fr, kind, squared)
            assert np.abs(got - want).max() / np.abs(want).max() <= g["fund_tol_d"][k]


def test_seven_point_solvers_agree_and_fit_their_samples():
    """both null-space routes give the same F per root, and every root's F passes through its seven records"""
    kp1, kp2, match, _, _ = EC.planted_pair(60, 60, 40, 0.6, 0.3, 11)
    rows = np.nonzero(match >= 0)[0]
    rec = np.concatenate([kp1[rows], kp2[match[rows]]], 1).astype(np.float64)
    smp = EC.draw_n(3, 0, np.arange(64), len(rec), 7)
    Fa, na = EC.seven_point(rec[smp])
    Fb, nb = EC.seven_point(rec[smp], EC.null_gj)
    np.testing.assert_array_equal(na, nb)
    assert set(na.tolist()) <= {1, 3} and (na == 3).any() and (na == 1).any()
    for t in range(64):
        for r in range(na[t]):
            assert EC.f_err(Fa[t, r], Fb[t, r]) < 1e-7
            assert EC.sampson(Fa[t, r], rec[smp[t]])[1].max() < 1e-6
            assert abs(np.linalg.det(Fa[t, r] / np.abs(Fa[t, r]).max())) < 1e-9
        assert not Fa[t, na[t]:].any()


def test_draw7_extends_draw4():
    """seven distinct in-range indices whose first four are draw4's"""
    for m in (7, 8, 40, 257, 1025):
        s7 = EC.draw_n(99, 3, np.arange(200), m, 7)
        np.testing.assert_array_equal(s7[:, :4], VC.draw4(99, 3, np.arange(200), m))
        assert s7.min() >= 0 and s7.max() < m and all(len(set(r)) == 7 for r in s7.tolist())
    assert sorted(EC.draw_n(5, 1, [0], 7, 7)[0].tolist()) == list(range(7))
