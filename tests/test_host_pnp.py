"""CPU checks of localization's host side: the three new C entries (in the header, exported, bound), the
workspace convention and the argument checks of rr_localize_pairs / rr_p3p (they return before anything
is enqueued, so they run without a GPU), the Python surface's refusals, the pnp.npz fixture against the
numpy restatement of tests/pnp_cases.py and its two routes against each other, project_points /
unproject_points against values of the reference's functions, and the minimal solver's header run on
the CPU under AddressSanitizer and UBSan by a stand-alone program (tests/asan/p3p_host.cpp)."""

import ctypes
import functools
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import pnp_cases as PN
from conftest import PKG, REPO, golden

HEADER = os.path.join(REPO, "include", "rr.h")
LIB = os.path.join(PKG, "librr.so")
NEW = ("rr_localize_workspace_bytes", "rr_localize_pairs", "rr_p3p")
P = ctypes.c_void_p(0x1000)   # "non-null, aligned"; never dereferenced
NULL = ctypes.c_void_p(0)


def _lib():
    from cirtorch import _engine
    return _engine.lib()


# ---------------------------------------------------------------- the ABI
def test_new_symbols_in_header_exported_and_bound():
    from cirtorch import _engine, _ops
    from cirtorch.geometry.camera.perspective import project_points, unproject_points
    from cirtorch.geometry.pnp import solve_p3p
    from cirtorch.search import localize_pairs
    text = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(rr_\w+)\b", out))
    for name in NEW:
        assert re.search(r"^\s*(?:size_t|int)\s+%s\s*\(" % name, text, flags=re.M), name
        assert name in exported and name in _engine._SIGS, name
        assert getattr(_engine.lib(), name) is not None
    assert "#define RR_PNP_GN_STEPS 3" in text and PN.GN_STEPS == 3
    assert float(re.search(r"#define RR_PNP_SMALL_ANGLE2 (\S+)", text).group(1)) == PN.SMALL2
    assert all(callable(f) for f in (_ops.localize_pairs, _ops.p3p, solve_p3p, localize_pairs, project_points, unproject_points))


# ---------------------------------------------------------------- workspace convention
def _need(lib, rows1, npairs, iters):
    return lib.rr_localize_workspace_bytes(rows1, npairs, iters)


def _call(lib, ws, wsb, rows1, npairs, iters):
    return lib.rr_localize_pairs(P, P, rows1, P, NULL, P, rows1, P, npairs, 1, P, 3.0, iters, 1, 7, P, P, P, P, ws, wsb, NULL)


def test_short_and_null_workspace_are_refused():
    lib = _lib()
    shape = dict(rows1=12, npairs=3, iters=300)
    need = _need(lib, **shape)
    assert need >= 256 and need % 256 == 0, need
    assert need >= 12 * 40 + 3 * 4 + 3 * 2 * 8     # records of five doubles, counts, one key per (pair, chunk of 256)
    for ws, wsb in ((P, need - 1), (NULL, need), (P, 0)):
        assert _call(lib, ws, wsb, **shape) == -3, wsb                                # RR_ENOSPACE
        msg = lib.rr_last_error().decode()
        assert msg.startswith("rr_localize_pairs") and "workspace" in msg, msg
    assert _call(lib, P, need, rows1=12, npairs=0, iters=300) == 0                    # nothing to launch


def test_need_is_monotone_in_every_size():
    lib = _lib()
    grid = dict(rows1=(0, 1, 12, 4096), npairs=(0, 1, 3, 100), iters=(1, 256, 257, 300, 65536))
    keys = sorted(grid)
    need = {pt: _need(lib, **dict(zip(keys, pt))) for pt in itertools.product(*(grid[k] for k in keys))}
    for pt, b in need.items():
        assert b % 256 == 0 and b < 1 << 48, (pt, b)
        for i, k in enumerate(keys):
            j = grid[k].index(pt[i])
            if j + 1 < len(grid[k]):
                assert need[pt[:i] + (grid[k][j + 1],) + pt[i + 1:]] >= b, (keys, pt)
    assert need[(65536, 100, 4096)] > need[(300, 100, 4096)] > need[(300, 3, 4096)] > need[(300, 3, 12)]


# ---------------------------------------------------------------- argument refusals
def test_argument_checks():
    """every refusal happens on the host: made-up device addresses, nothing is launched"""
    lib = _lib()
    need = _need(lib, 10, 2, 512)

    def loc(kp1=P, off1=P, X=P, valid=NULL, off2=P, match=P, rows1=10, rows2=12, npairs=2, max_n1=10, K=P, th=3.0, iters=512,
            refine=2, inl=P, R=P, t=P, mask=P, ws=P, wsb=need):
        return lib.rr_localize_pairs(kp1, off1, rows1, X, valid, off2, rows2, match, npairs, max_n1, K, th, iters, refine, 7,
                                     inl, R, t, mask, ws, wsb, NULL)

    bad = [dict(kp1=NULL), dict(X=NULL), dict(off1=NULL), dict(off2=NULL), dict(match=NULL), dict(inl=NULL), dict(R=NULL),
           dict(t=NULL), dict(mask=NULL), dict(ws=NULL), dict(iters=0), dict(iters=-5), dict(iters=(1 << 24) + 1),
           dict(refine=-1), dict(th=0.0), dict(th=-1.0), dict(th=float("inf")), dict(th=float("nan")), dict(wsb=need - 257),
           dict(wsb=0), dict(max_n1=11), dict(max_n1=-1), dict(rows1=-1), dict(rows2=-1), dict(npairs=-1),
           dict(kp1=ctypes.c_void_p(0x1004)), dict(X=ctypes.c_void_p(0x1004)), dict(K=NULL), dict(K=ctypes.c_void_p(0x1008))]
    for kw in bad:
        assert loc(**kw) in (-1, -3), kw     # RR_EINVAL / RR_ENOSPACE, never RR_EHIP: no launch was attempted
        assert lib.rr_last_error().decode().startswith("rr_localize_pairs"), kw
    for kw in (dict(K=NULL), dict(K=ctypes.c_void_p(0x1008))):
        assert loc(**kw) == -1 and " K" in lib.rr_last_error().decode(), kw           # RR_EINVAL
    for kw in (dict(inl=NULL), dict(R=NULL), dict(t=NULL), dict(mask=NULL)):
        assert loc(**kw) == -1 and lib.rr_last_error().decode() == "rr_localize_pairs: null output", kw
    for kw in (dict(rows1=-1), dict(rows2=-1), dict(npairs=-1), dict(max_n1=-1)):
        assert loc(**kw) == -1 and "negative" in lib.rr_last_error().decode(), kw
    assert loc(npairs=0) == 0 and loc(npairs=0, valid=P) == 0
    assert lib.rr_localize_pairs(NULL, P, 0, NULL, NULL, P, 0, NULL, 0, 0, NULL, 3.0, 1, 0, 0, NULL, NULL, NULL, NULL, P, 256,
                                 NULL) == 0

    def p3(x=P, X=P, n=3, R=P, t=P, nsol=P):
        return lib.rr_p3p(x, X, n, R, t, nsol, NULL)

    for kw in [dict(x=NULL), dict(X=NULL), dict(R=NULL), dict(t=NULL), dict(nsol=NULL), dict(n=-1), dict(x=ctypes.c_void_p(0x1004)),
               dict(X=ctypes.c_void_p(0x1004))]:
        assert p3(**kw) == -1, kw                                                     # RR_EINVAL: refused, not launched
        assert lib.rr_last_error().decode().startswith("rr_p3p"), kw
    assert p3(n=0) == 0 and p3(n=0, x=NULL, X=NULL, R=NULL, t=NULL, nsol=NULL) == 0


def test_python_refusals():
    from cirtorch.geometry.pnp import solve_p3p
    from cirtorch.search import localize_pairs
    kp, X, m = torch.zeros(2, 9, 2), torch.zeros(2, 10, 3, dtype=torch.float64), torch.zeros(2, 9, dtype=torch.int64)
    K = torch.eye(3, dtype=torch.float64)
    for bad in (torch.eye(4, dtype=torch.float64), torch.zeros(3, 3, 3, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="K"):                   # wrong K shape (P = 2)
            localize_pairs(kp, X, m, bad)
    for kw in (dict(iters=0), dict(refine=-1), dict(th=0.0), dict(max_n1=5), dict(offsets1=torch.tensor([0, 9, 18])),
               dict(valid=torch.ones(2, 9, dtype=torch.bool)), dict(valid=torch.ones(2, 10))):
        with pytest.raises(ValueError):
            localize_pairs(kp, X, m, K, **kw)
    for args in ((kp, X[..., :2], m), (kp[..., :1], X, m), (kp, X, m.int()), (kp, X.long(), m), (kp, X[0], m), (kp, X, m[:, :8])):
        with pytest.raises(ValueError):
            localize_pairs(*args, K)
    # the kernel-backed functions raise on CPU tensors, like the rest of the package
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        localize_pairs(kp, X, m, K)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        localize_pairs(kp, X.float(), m, torch.stack([K, K]), valid=torch.ones(2, 10, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        localize_pairs(kp.view(18, 2), X.view(20, 3), m.view(18), K, offsets1=torch.tensor([0, 9, 18]),
                       offsets2=torch.tensor([0, 10, 20]))
    x, Xw = torch.zeros(4, 3, 2, dtype=torch.float64), torch.zeros(4, 3, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        solve_p3p(x, Xw)
    for a, b in ((x[:, :2], Xw), (x, Xw[:3]), (x, Xw[..., :2]), (x.long(), Xw), (x[0], Xw[0])):
        with pytest.raises(ValueError):
            solve_p3p(a, b)


# ---------------------------------------------------------------- the camera functions
def test_project_and_unproject_points_against_the_reference_values():
    from cirtorch.geometry.camera import project_points, unproject_points
    g = golden("pnp.npz")
    pts, Ks, uv, depth = (torch.from_numpy(a) for a in PN.cam_inputs(int(g["cam_seed"])))
    np.testing.assert_allclose(project_points(pts, Ks).numpy(), g["cam_uv"], rtol=1e-14, atol=1e-12)
    np.testing.assert_allclose(unproject_points(uv, depth, Ks).numpy(), g["cam_xyz"], rtol=1e-14, atol=1e-12)
    np.testing.assert_allclose(unproject_points(uv, depth, Ks, normalize=True).numpy(), g["cam_ray"], rtol=1e-14, atol=1e-12)
    assert pts[0, 5, 2] == 0.0 and np.isfinite(g["cam_uv"]).all()    # the point at Z = 0 is not divided
    # round trip: pixels -> camera frame at a depth -> pixels
    back = project_points(unproject_points(uv, depth, Ks), Ks)
    np.testing.assert_allclose(back.numpy(), uv.numpy(), rtol=0, atol=1e-10)
    ray = unproject_points(uv, depth, Ks, normalize=True)
    np.testing.assert_allclose(ray.norm(dim=-1, keepdim=True).numpy(), depth.numpy(), rtol=1e-14)
    assert project_points(pts.float(), Ks.float()).dtype == torch.float32
    for args in ((pts[..., :2], Ks), (pts, Ks[..., :2])):
        with pytest.raises(ValueError):
            project_points(*args)
    for args in ((uv, depth[..., 0], Ks), (pts, depth, Ks), (uv, depth, Ks[..., :2, :])):
        with pytest.raises(ValueError):
            unproject_points(*args)


# ---------------------------------------------------------------- the fixture against the restatement
@functools.lru_cache(maxsize=None)
def pcase(k, route="A"):
    g = golden("pnp.npz")
    case = PN.ALL_CASES[k]
    kp, off1, X, valid, off2, match, planted, Ks, parts = PN.build_case(case, int(g["c_seeds"][k]))
    np.testing.assert_allclose(PN.case_checksum(kp, X, match), g["c_chk"][k], rtol=0, atol=1e-6)
    return case, (kp, off1, X, valid, off2, match, planted, Ks, parts), PN.pnp_batch(
        kp, off1, X, valid, off2, match, Ks, PN.TH, case["iters"], case["refine"], PN.RUN_SEED, route)


def test_cases_cover_what_the_kernels_branch_on():
    g = golden("pnp.npz")
    by = {c["name"]: c for c in PN.PNP_CASES}
    ms = [[q[2] for q in c["pairs"]] for c in PN.PNP_CASES]
    for m in ([0], [2], [3], [4], [40], [257], [PN.STAGE + 1]):
        assert m in ms, m
    assert PN.STAGE == 1024 and by["m1025"]["pairs"][0][2] > PN.STAGE and by["m257_r2"]["pairs"][0][2] > 256
    assert {c["iters"] for c in PN.PNP_CASES} >= {1, 257} and by["iters257"]["iters"] > 256
    assert {c["refine"] for c in PN.PNP_CASES if c["pairs"][0][2] == 257} == {0, 2}
    kinds = {q[5] for c in PN.PNP_CASES for q in c["pairs"]}
    assert PN.TH == 3.0 and PN.NOISE == 0.3 and kinds == {"general", "valid", "nan", "behind", "coplanar", "singular", "othercam"}
    assert [q[2] for q in by["ragged4"]["pairs"]] == [0, 2, 60, 50] and by["outliers"]["pairs"][0][3] == 0.0
    assert [q[5] for q in by["singularK"]["pairs"]].count("singular") == 1 and len(by["singularK"]["pairs"]) == 4
    # the records each case really has, and what its scene claims
    for k, case in enumerate(PN.ALL_CASES):
        _, (kp, off1, X, valid, off2, match, planted, Ks, parts), (inl, Rs, ts, mask, infos) = pcase(k)
        for p, o in enumerate(infos):
            n, kind = case["pairs"][p][2], case["pairs"][p][5]
            if kind == "valid":
                assert valid is not None and o["m"] == n - n // 3
            elif kind == "nan":
                assert o["m"] == n - 1 and np.isnan(parts[p]["X"]).sum() == 1
            elif kind == "chain":
                assert valid is not None and 8 <= o["m"] <= n
            else:
                assert o["m"] == n, (case["name"], p)
            if kind == "behind":
                Xc = parts[p]["X"] @ parts[p]["R"].T + parts[p]["t"]
                back = (Xc[:, 2] < 0) & np.isin(np.arange(len(Xc)), parts[p]["match"])
                assert back.sum() == 18 and not mask[off1[p]:off1[p + 1]][np.isin(parts[p]["match"], np.nonzero(back)[0])].any()
            if kind == "coplanar":
                Xc = parts[p]["X"] @ parts[p]["R"].T + parts[p]["t"]
                assert np.abs(Xc @ np.array([0.2, -0.1, 1.0]) - 8.0).max() < 1e-9
    assert len(g["c_seeds"]) == len(PN.ALL_CASES)


@pytest.mark.parametrize("k", range(len(PN.ALL_CASES)))
def test_restatement_equals_fixture_and_routes_agree(k):
    g = golden("pnp.npz")
    case, (kp, off1, X, valid, off2, match, planted, Ks, parts), (inl, Rs, ts, mask, infos) = pcase(k)
    _, _, (inl_b, Rb, tb, mask_b, infos_b) = pcase(k, "B")
    assert kp.dtype == np.float32 and X.dtype == np.float64 and match.dtype == np.int64
    np.testing.assert_array_equal(inl, g["c%d_inl" % k])
    np.testing.assert_array_equal(mask, g["c%d_mask" % k])
    np.testing.assert_array_equal([o["t_win"] for o in infos], g["c%d_tw" % k])
    np.testing.assert_array_equal([o["sol"] for o in infos], g["c%d_sol" % k])
    np.testing.assert_array_equal(inl_b, inl)
    np.testing.assert_array_equal(mask_b, mask)
    assert [(o["t_win"], o["sol"]) for o in infos_b] == [(o["t_win"], o["sol"]) for o in infos]
    for p, o in enumerate(infos):
        tol = g["c%d_tol" % k][p]
        assert int(mask[off1[p]:off1[p + 1]].sum()) == inl[p]
        if inl[p]:
            assert o["margin"] >= 1e-7 and infos_b[p]["margin"] >= 1e-7
            assert np.abs(Rs[p] @ Rs[p].T - np.eye(3)).max() < 1e-12 and np.linalg.det(Rs[p]) > 0
            assert PN.pose_err(Rs[p], ts[p], g["c%d_R" % k][p], g["c%d_t" % k][p]) <= tol
            assert 100 * PN.pose_err(Rb[p], tb[p], Rs[p], ts[p]) <= tol * (1 + 1e-6)
        else:
            assert not Rs[p].any() and not ts[p].any() and not g["c%d_R" % k][p].any() and o["t_win"] == -1
    if case["name"] == "singularK":
        assert inl[1] == 0 and min(inl[0], inl[2], inl[3]) >= 18
    if case["name"] == "exact":
        assert inl[0] == 50 and PN.pose_err(Rs[0], ts[0], parts[0]["R"], parts[0]["t"]) <= g["x_tol"]
    if case["name"] == "chain":
        import pose_cases as PC
        deg = (PC.rot_angle_deg(Rs[0], parts[0]["R"]), PC.dir_angle_deg(ts[0], parts[0]["t"]))
        np.testing.assert_allclose(deg, g["chain_deg"], rtol=0, atol=1e-6)
        assert max(deg) < 1.0           # half of the GPU chain's bound


def test_minimal_solver_routes_agree_and_fit_their_samples():
    g = golden("pnp.npz")
    x, X, R, t, nsol, drop, diffs, resid = PN.solver_samples(int(g["s_seed"]))
    np.testing.assert_allclose(PN.checksum(x, X), g["s_chk"], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(nsol, g["s_nsol"])
    assert drop == g["s_drop"] <= 0.02 and len(x) > 256
    np.testing.assert_allclose(np.maximum(100 * diffs, 1e-12), g["s_tol"], rtol=1e-3, atol=0)
    assert 100 * resid == pytest.approx(float(g["s_resid"]), rel=1e-3) and resid < 1e-6
    assert set(nsol.tolist()) >= {1, 2, 4} and nsol.max() <= 4
    for i in range(len(x)):
        assert not R[i, nsol[i]:].any() and not t[i, nsol[i]:].any()
        for k in range(nsol[i]):
            assert np.abs(R[i, k] @ R[i, k].T - np.eye(3)).max() < 1e-9 and np.linalg.det(R[i, k]) > 0
            assert ((X[i] @ R[i, k].T + t[i, k])[:, 2] > 0).all()


def test_draw3_is_a_prefix_rule():
    """three distinct in-range indices: the first three of the homography's four"""
    import epipolar_cases as EC
    import verify_cases as VC
    for m in (3, 4, 40, 257, 1025):
        s3 = EC.draw_n(99, 3, np.arange(200), m, 3)
        if m >= 4:
            np.testing.assert_array_equal(s3, VC.draw4(99, 3, np.arange(200), m)[:, :3])
        assert s3.min() >= 0 and s3.max() < m and all(len(set(r)) == 3 for r in s3.tolist())


# ---------------------------------------------------------------- the solver's header on the CPU, sanitised
def test_p3p_header_on_the_host_under_asan_and_ubsan(tmp_path):
    """tests/asan/p3p_host.cpp includes csrc/rr_p3p.h, runs the same statements the kernels run over
    seeded samples and checks every solution; built with -fsanitize=address,undefined, a program of
    its own: nothing is preloaded, nothing runs on a GPU"""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++"))
                if c and os.path.exists(c)), None)
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "p3p_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"),
                            os.path.join(REPO, "tests", "asan", "p3p_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe, "4000", "9500"], capture_output=True, text=True, timeout=120)
    print(run.stdout[-2000:])
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    m = re.search(r"samples (\d+) solutions (\d+) histogram (\d+) (\d+) (\d+) (\d+) (\d+) planted_found (\d+) worst_residual (\S+)", run.stdout)
    assert m, run.stdout
    n, nsol, h0, h1, h2, h3, h4, found = (int(v) for v in m.groups()[:8])
    assert n == 4000 and h0 + h1 + h2 + h3 + h4 == n and min(h1, h2, h4) > 0
    assert found >= 0.99 * n and float(m.group(9)) < 1e-3
