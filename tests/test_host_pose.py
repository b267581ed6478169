"""CPU checks of relative pose's host side: the new names of cirtorch.geometry.epipolar,
cirtorch.geometry.linalg and cirtorch.search, the three new C entries (in the header, exported,
bound), their argument checks (they return before anything is enqueued, so they run without a GPU),
the Python surface's refusals, the pose.npz fixture against the numpy restatement of
tests/pose_cases.py, the plain-torch helpers against closed forms and the recorded kernel resources."""

import ctypes
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import epipolar_cases as EC
import pose_cases as PC
from conftest import PKG, REPO, golden

HEADER = os.path.join(REPO, "include", "rr.h")
LIB = os.path.join(PKG, "librr.so")
NEW = ("rr_recover_pose", "rr_triangulate_points", "rr_essential_decompose")
P = ctypes.c_void_p(0x1000)   # "non-null, aligned"; never dereferenced
NULL = ctypes.c_void_p(0)


def _lib():
    from cirtorch import _engine
    return _engine.lib()


# ---------------------------------------------------------------- the package and the ABI
def test_package_and_names():
    import cirtorch.geometry.epipolar as E
    import cirtorch.geometry.linalg as L
    import cirtorch.search as S
    from cirtorch.geometry.epipolar import essential, projection, triangulation
    for mod, names in ((essential, ("essential_from_fundamental", "decompose_essential_matrix", "essential_from_Rt",
                                    "motion_from_essential", "motion_from_essential_choose_solution", "relative_camera_motion")),
                       (triangulation, ("triangulate_points",)),
                       (projection, ("intrinsics_like", "scale_intrinsics", "projection_from_KRt", "KRt_from_projection", "depth",
                                     "projections_from_fundamental"))):
        for name in names:
            assert callable(getattr(mod, name)) and getattr(E, name) is getattr(mod, name), name
    for name in ("cross_product_matrix", "eye_like", "vec_like"):
        assert callable(getattr(L, name))
    assert callable(S.recover_pose)
    # what was there stays
    for name in ("find_fundamental", "normalize_points", "sampson_epipolar_distance"):
        assert callable(getattr(E, name))


def test_new_symbols_in_header_exported_and_bound():
    from cirtorch import _engine
    text = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(rr_\w+)\b", out))
    for name in NEW:
        assert re.search(r"^\s*int\s+%s\s*\(" % name, text, flags=re.M), name
        assert name in exported and name in _engine._SIGS, name
        assert getattr(_engine.lib(), name) is not None
    assert re.search(r"^#define RR_POSE_SWEEPS \d+$", text, flags=re.M)
    # the header cites the reference lines it restates and states the deviation
    for cite in ("essential.py:8-18", "essential.py:33-40", "essential.py:149-151", "triangulation.py:27-31", "conversions.py:77-83"):
        assert cite in text, cite


# ---------------------------------------------------------------- argument refusals
def test_argument_checks():
    """every refusal happens on the host: made-up device addresses, nothing is launched"""
    lib = _lib()

    def pose(kp1=P, off1=P, kp2=P, off2=P, match=P, mask=P, F=P, K1=P, K2=P, rows1=10, rows2=12, npairs=2, max_n1=10, R=P,
             t=P, E=P, front=P, pts=P, fmask=P):
        return lib.rr_recover_pose(kp1, off1, rows1, kp2, off2, rows2, match, mask, F, K1, K2, npairs, max_n1, R, t, E, front,
                                   pts, fmask, NULL, 0, NULL)

    bad = [dict(kp1=NULL), dict(kp2=NULL), dict(off1=NULL), dict(off2=NULL), dict(match=NULL), dict(F=NULL), dict(K1=NULL),
           dict(K2=NULL), dict(R=NULL), dict(t=NULL), dict(E=NULL), dict(front=NULL), dict(pts=NULL), dict(fmask=NULL),
           dict(max_n1=11), dict(max_n1=-1), dict(rows1=-1), dict(rows2=-1), dict(npairs=-1), dict(rows1=1 << 31, max_n1=0),
           dict(kp1=ctypes.c_void_p(0x1004)), dict(kp2=ctypes.c_void_p(0x1004))]
    for kw in bad:
        assert pose(**kw) != 0, kw
        assert lib.rr_last_error().decode().startswith("rr_recover_pose"), kw
    assert pose(npairs=0) == 0 and pose(mask=NULL, npairs=0) == 0
    assert lib.rr_recover_pose(NULL, P, 0, NULL, P, 0, NULL, NULL, NULL, NULL, NULL, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL,
                               NULL, 0, NULL) == 0

    def tri(p1=P, p2=P, P1=P, P2=P, off=P, rows=10, npairs=2, X=P):
        return lib.rr_triangulate_points(p1, p2, P1, P2, off, rows, npairs, X, NULL)

    for kw in [dict(p1=NULL), dict(p2=NULL), dict(P1=NULL), dict(P2=NULL), dict(off=NULL), dict(X=NULL), dict(rows=-1),
               dict(npairs=-1), dict(p1=ctypes.c_void_p(0x1008)), dict(p2=ctypes.c_void_p(0x1008)), dict(rows=1 << 31)]:
        assert tri(**kw) != 0, kw
        assert lib.rr_last_error().decode().startswith("rr_triangulate_points"), kw
    assert tri(npairs=0) == 0 and tri(npairs=0, P1=NULL, P2=NULL) == 0

    def dec(E=P, n=3, R1=P, R2=P, t=P):
        return lib.rr_essential_decompose(E, n, R1, R2, t, NULL)

    for kw in [dict(E=NULL), dict(R1=NULL), dict(R2=NULL), dict(t=NULL), dict(n=-1)]:
        assert dec(**kw) != 0, kw
        assert lib.rr_last_error().decode().startswith("rr_essential_decompose"), kw
    assert dec(n=0) == 0 and dec(n=0, E=NULL, R1=NULL, R2=NULL, t=NULL) == 0


def test_python_refusals():
    from cirtorch.geometry.epipolar import (decompose_essential_matrix, motion_from_essential,
                                            motion_from_essential_choose_solution, triangulate_points)
    from cirtorch.search import recover_pose
    k1, k2, m = torch.zeros(2, 9, 2), torch.zeros(2, 10, 2), torch.zeros(2, 9, dtype=torch.int64)
    F, K = torch.zeros(2, 3, 3, dtype=torch.float64), torch.eye(3, dtype=torch.float64)
    for kw in (dict(K1=torch.eye(4)), dict(K2=torch.zeros(3, 3, 3)), dict(F=torch.zeros(3, 3, 3)), dict(mask=torch.ones(2, 8, dtype=torch.bool)),
               dict(mask=torch.ones(2, 9)), dict(match=m.int()), dict(max_n1=5), dict(offsets1=torch.tensor([0, 9, 18])),
               dict(kpts1=torch.zeros(2, 9, 3))):
        args = dict(kpts1=k1, kpts2=k2, match=m, F=F, K1=K, K2=K)
        args.update(kw)
        with pytest.raises(ValueError):
            recover_pose(**args)
    # the kernel-backed functions raise on CPU tensors, like the rest of the package
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        recover_pose(k1, k2, m, F, K, K)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        recover_pose(k1, k2, m, F, K, K.expand(2, 3, 3), mask=torch.ones(2, 9, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        recover_pose(k1.view(18, 2), k2.view(20, 2), m.view(18), F, K, K, offsets1=torch.tensor([0, 9, 18]),
                     offsets2=torch.tensor([0, 10, 20]))
    Pm = torch.zeros(2, 3, 4)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        triangulate_points(Pm, Pm, k1, k1)
    for args in [(Pm[0], Pm[0], k1, k1), (Pm, Pm, k1, k2), (Pm, Pm, k1[0], k1[0]), (Pm.double(), Pm, k1, k1), (Pm[:1], Pm[:1], k1, k1),
                 (Pm.long(), Pm.long(), k1.long(), k1.long())]:
        with pytest.raises(ValueError):
            triangulate_points(*args)
    for fn in (decompose_essential_matrix, motion_from_essential):
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            fn(torch.zeros(2, 3, 3))
        with pytest.raises(ValueError):
            fn(torch.zeros(2, 3, 4))
    E3, K3 = torch.zeros(2, 3, 3), torch.eye(3).expand(2, 3, 3)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        motion_from_essential_choose_solution(E3, K3, K3, k1, k1)
    for args in [(E3, K3[0], K3, k1, k1), (E3, K3, K3, k1, k2), (E3[:1], K3, K3, k1, k1)]:
        with pytest.raises(ValueError):
            motion_from_essential_choose_solution(*args)
    with pytest.raises(ValueError):
        motion_from_essential_choose_solution(E3, K3, K3, k1, k1, mask=torch.ones(2, 8, dtype=torch.bool))


# ---------------------------------------------------------------- the fixture against the restatement
def check_pair(o, R, t, X, front, fmask, tol, scale, what):
    assert o["front"] == front and np.array_equal(o["front_mask"], fmask), what
    if o["slot"] < 0:
        assert not R.any() and not t.any() and not X.any() and front == 0, what
        return
    eR, et, eX = np.abs(o["R"] - R).max(), np.abs(o["t"] - t).max(), np.abs(o["points3d"] - X).max() / scale
    print(what, "counts", o["counts"], "R err %.3g t err %.3g X err %.3g" % (eR, et, eX), "tol", tol)
    assert (tol >= 1e-12).all() and eR <= tol[0] and et <= tol[1] and eX <= tol[2], what
    c = np.sort(o["counts"])[::-1]
    assert c[0] > c[1] and o["depth"] >= 1e-6 * scale and o["wgap"] >= 1e-6, what     # the generator's conditions
    assert abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.norm(t) - 1) < 1e-14


@functools.lru_cache(maxsize=None)
def pcase(k):
    g = golden("pose.npz")
    s, F, mask = PC.build_case(PC.CASES[k], int(g["p_seeds"][k]))
    np.testing.assert_allclose(PC.checksum(s["kp1"], s["kp2"], s["match"], F, np.zeros(0) if mask is None else mask), g["p_chk"][k],
                               rtol=0, atol=1e-6)
    return s, F, mask


def test_cases_cover_what_the_kernel_branches_on():
    assert [c["m"] for c in PC.CASES if c["kind"] == "true"][:8] == [0, 1, 7, 63, 64, 65, 257, EC.STAGE + 1]
    assert {c["m"] for c in PC.CASES if c["kind"] == "ver"} == {63, 64, 65, 257, EC.STAGE + 1}
    assert {"nomask", "k2"} <= {c["kind"] for c in PC.CASES} and PC.N_MOTIONS >= 16
    assert [n for n, _ in PC.RAGGED] == ["empty", "zeroF", "three", "noisy", "exact"]
    assert not np.array_equal(PC.K2_OTHER, PC.K1) and PC.K2_OTHER[0, 0] != PC.K2_OTHER[1, 1]
    # the motions: both signs of every translation component, and the restatement's four slots all win somewhere
    g = golden("pose.npz")
    first = [c["name"] for c in PC.CASES].index("motion0")
    ts = np.array([pcase(first + i)[0]["t"] for i in range(PC.N_MOTIONS)])
    assert ((ts > 0).any(0) & (ts < 0).any(0)).all(), ts
    slots = [PC.pose_pair(*(pcase(first + i)[0][key] for key in ("kp1", "kp2", "match")), None, pcase(first + i)[1], PC.K1, PC.K1)["slot"]
             for i in range(PC.N_MOTIONS)]
    print("winning slots of the restatement:", slots)
    assert len(set(slots)) >= 3 and g["p_seeds"].shape == (len(PC.CASES),)


@pytest.mark.parametrize("k", range(len(PC.CASES)))
def test_restatement_equals_fixture(k):
    g = golden("pose.npz")
    s, F, mask = pcase(k)
    o = PC.pose_pair(s["kp1"], s["kp2"], s["match"], mask, F, s["K1"], s["K2"])
    used = len(o["rows"])
    assert used == (PC.CASES[k]["m"] if mask is None else int(mask.sum()))
    check_pair(o, g["p%d_R" % k], g["p%d_t" % k], g["p%d_X" % k], int(g["p%d_front" % k]), g["p%d_fmask" % k], g["p%d_tol" % k],
               PC.median_depth(s["X"][o["rows"]]), PC.CASES[k]["name"])
    if PC.CASES[k]["kind"] == "true" and used:    # the true F: the planted motion itself, every match in front
        assert o["front"] == used and np.abs(o["R"] - s["R"]).max() < 1e-12
        assert np.abs(o["t"] - s["t"] / np.linalg.norm(s["t"])).max() < 1e-12
    if PC.CASES[k]["kind"] == "k2":
        assert not np.array_equal(s["K1"], s["K2"])


def test_ragged_and_end_to_end_restatements_equal_fixture():
    g = golden("pose.npz")
    scenes, Fs, mask = PC.build_ragged(int(g["r_seed"]))
    kp1, off1, kp2, off2, match = PC.ragged_arrays(scenes)
    np.testing.assert_allclose(PC.checksum(kp1, kp2, match, Fs, mask), g["r_chk"], rtol=0, atol=1e-6)
    infos = PC.pose_batch(kp1, off1, kp2, off2, match, mask, Fs, PC.K1, PC.K1)[6]
    for p, (o, s) in enumerate(zip(infos, scenes)):
        a = slice(off1[p], off1[p + 1])
        check_pair(o, g["r_R"][p], g["r_t"][p], g["r_X"][a], int(g["r_front"][p]), g["r_fmask"][a], g["r_tol"][p],
                   PC.median_depth(s["X"][o["rows"]]), PC.RAGGED[p][0])
    assert g["r_front"].tolist()[:3] == [0, 0, 3] and g["r_front"][4] == 50
    # the noise-free pair: the truth
    ex, se = infos[4], scenes[4]
    assert np.abs(ex["R"] - np.eye(3)).max() < 1e-9 and np.abs(ex["t"] - PC.T_EXACT).max() < 1e-9
    assert np.abs(ex["points3d"][ex["rows"]] - se["X"][ex["rows"]]).max() / PC.median_depth(se["X"]) < 1e-7
    # end to end: the numpy chain is what the fixture stores; it recovers the planted motion
    scenes = [PC.scene(*spec, int(g["e_seed"]) + 17 * k) for k, spec in enumerate(PC.E2E)]
    for p, s in enumerate(scenes):
        a = EC.epipolar_pair(s["kp1"], s["kp2"], s["match"], p, **PC.VER)
        o = PC.pose_pair(s["kp1"], s["kp2"], s["match"], a["mask"], a["F"], s["K1"], s["K2"])
        assert a["inliers"] == g["e_inl"][p] and o["front"] == g["e_front"][p]
        assert np.array_equal(o["R"], g["e_R"][p]) or np.abs(o["R"] - g["e_R"][p]).max() <= g["e_tol"][p][0]
        assert PC.rot_angle_deg(o["R"], s["R"]) < 1.0 and PC.dir_angle_deg(o["t"], s["t"]) < 1.0


# ---------------------------------------------------------------- plain-torch helpers against closed forms
def test_plain_torch_helpers():
    from cirtorch.geometry.epipolar import (KRt_from_projection, depth, essential_from_fundamental, essential_from_Rt,
                                            intrinsics_like, projection_from_KRt, projections_from_fundamental,
                                            relative_camera_motion, scale_intrinsics)
    from cirtorch.geometry.linalg import cross_product_matrix, eye_like, vec_like
    s = PC.scene(40, 40, 40, 1.0, 0.0, 5)      # the noise-free scene: exact correspondences
    s2 = PC.scene(40, 40, 40, 1.0, 0.3, 6)     # a rotated view (0.3 px noise on side 2: use the true points)
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    # essential_from_Rt of the planted motion annihilates the planted correspondences in normalised coordinates
    for sc in (s, s2):
        R, t, X = t64(sc["R"])[None], t64(sc["t"]).view(1, 3, 1), sc["X"]
        E = essential_from_Rt(torch.eye(3, dtype=torch.float64)[None], torch.zeros(1, 3, 1, dtype=torch.float64), R, t)[0].numpy()
        x1 = X / X[:, 2:]
        X2 = X @ sc["R"].T + sc["t"]
        x2 = X2 / X2[:, 2:]
        r = np.einsum("ni,ij,nj->n", x2, E, x1)
        assert np.abs(r).max() < 1e-14, np.abs(r).max()
        # and K^-T E K^-1 is the scene's F; essential_from_fundamental inverts it
        Ki = np.linalg.inv(EC.K)
        assert EC.f_err(Ki.T @ E @ Ki, sc["F"]) < 1e-13
        E2 = essential_from_fundamental(t64(sc["F"])[None], t64(EC.K)[None], t64(EC.K)[None])[0].numpy()
        assert EC.f_err(E2, E) < 1e-12
        # depth: the z of the moved points
        d = depth(R, t, t64(X)[None])[0].numpy()
        np.testing.assert_allclose(d, X2[:, 2], rtol=1e-14, atol=0)
    # a relative motion between two moved cameras: T2 T1^-1
    Ra, Rb = t64(EC.rot(0.1, -0.2, 0.05))[None], t64(EC.rot(-0.15, 0.1, 0.2))[None]
    ta, tb = t64([[0.3], [-0.1], [0.2]])[None], t64([[-0.5], [0.4], [0.1]])[None]
    R, t = relative_camera_motion(Ra, ta, Rb, tb)
    Xw = np.array([0.4, -0.3, 5.0])
    xa = Ra[0].numpy() @ Xw + ta[0, :, 0].numpy()
    np.testing.assert_allclose(R[0].numpy() @ xa + t[0, :, 0].numpy(), Rb[0].numpy() @ Xw + tb[0, :, 0].numpy(), rtol=0, atol=1e-14)   # a dozen roundings at magnitude 5
    # projection_from_KRt o KRt_from_projection round-trips
    K = t64(np.stack([PC.K1, PC.K2_OTHER]))
    Rs, ts = torch.cat([Ra, Rb]), torch.cat([ta, tb])
    Pm = projection_from_KRt(K, Rs, ts)
    assert tuple(Pm.shape) == (2, 3, 4)
    np.testing.assert_allclose(Pm[1].numpy(), PC.K2_OTHER @ np.concatenate([Rb[0].numpy(), tb[0].numpy()], 1), rtol=0, atol=1e-12)
    K_, R_, t_ = KRt_from_projection(Pm)
    np.testing.assert_allclose(K_.numpy(), K.numpy(), rtol=0, atol=1e-9)
    np.testing.assert_allclose(R_.numpy(), Rs.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(t_.numpy(), ts.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(projection_from_KRt(K_, R_, t_).numpy(), Pm.numpy(), rtol=0, atol=1e-9)
    # intrinsics
    img = torch.zeros(2, 3, 480, 640)
    Ki_ = intrinsics_like(500.0, img)
    assert tuple(Ki_.shape) == (2, 3, 3) and Ki_[1].tolist() == [[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]]
    Ks = scale_intrinsics(Ki_, 0.5)
    assert Ks[0].tolist() == [[250.0, 0.0, 160.0], [0.0, 250.0, 120.0], [0.0, 0.0, 1.0]] and Ki_[0, 0, 0] == 500.0
    # linalg
    v = t64([[1.0, 2.0, 3.0], [-0.5, 0.25, 4.0]])
    w = np.array([0.3, -0.7, 0.2])
    for i in range(2):
        np.testing.assert_allclose(cross_product_matrix(v)[i].numpy() @ w, np.cross(v[i].numpy(), w), rtol=0, atol=1e-15)
    assert torch.equal(eye_like(3, img), torch.eye(3).expand(2, 3, 3)) and torch.equal(vec_like(3, img), torch.zeros(2, 3, 1))
    assert eye_like(4, v).dtype == torch.float64
    # projections_from_fundamental: F is the fundamental matrix of the returned pair, [e2]_x P2 P1^+ ~ F
    F = t64(s2["F"])[None]
    PP = projections_from_fundamental(F)
    assert tuple(PP.shape) == (1, 3, 4, 2) and torch.equal(PP[0, :, :, 0], torch.eye(3, 4, dtype=torch.float64))
    P2 = PP[0, :, :, 1].numpy()
    e2 = P2[:, 3]
    Fb = np.array([[0, -e2[2], e2[1]], [e2[2], 0, -e2[0]], [-e2[1], e2[0], 0]]) @ P2[:, :3]
    assert EC.f_err(Fb, s2["F"]) < 1e-9


def test_recorded_kernel_resources():
    """profiles/pose_kernel_resources.json: what the compiler reported for the three kernels; no scratch"""
    rec = json.load(open(os.path.join(REPO, "profiles", "pose_kernel_resources.json")))
    assert set(rec["kernels"]) == {"k_recover_pose", "k_triangulate", "k_essential_decompose"}
    for name, r in rec["kernels"].items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs"] <= 256 and r["Occupancy [waves/SIMD]"] >= 1, name
