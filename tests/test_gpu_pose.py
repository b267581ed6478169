"""Relative pose on the GPU (rr_recover_pose / rr_triangulate_points / rr_essential_decompose,
cirtorch.search.recover_pose, cirtorch.geometry.epipolar) against what the reference's essential.py /
triangulation.py / projection.py produced in float64, one pair per call (tests/golden/pose.npz), and
the float64 numpy restatement of tests/pose_cases.py.

Tolerances.  `front` and `front_mask` are exact: the fixture's generator asserts that under each of
the four candidates no depth of a used record lies within 1e-6 x the median scene depth of zero, no
|w| within 1e-6 relative of 1e-8, and that the winner's count exceeds the runner-up's.  R, t (largest
absolute entry difference) and points3d (largest absolute coordinate difference relative to the
median depth of the pair's true points) are compared against the fixture's per-pair tolerance: 100 x
the difference between the reference's torch.svd path and the numpy restatement on the same inputs,
floor 1e-12 (make_golden_pose.py).  The candidate order is the entry's own (rr.h): which slot wins
is printed, never compared."""

import functools

import numpy as np
import pytest
import torch

import epipolar_cases as EC
import pose_cases as PC
from conftest import golden

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in PC.CASES]


def dev(x, cuda):
    return torch.from_numpy(np.array(x)).to(cuda)   # a copy: the cached cases are read-only


def bits(t):
    return t.cpu().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def pcase(k):
    """case k: the scene, F, mask (built once, never modified)"""
    g = golden("pose.npz")
    s, F, mask = PC.build_case(PC.CASES[k], int(g["p_seeds"][k]))
    np.testing.assert_allclose(PC.checksum(s["kp1"], s["kp2"], s["match"], F, np.zeros(0) if mask is None else mask), g["p_chk"][k],
                               rtol=0, atol=1e-6)
    for a in list(s.values()) + [F] + ([] if mask is None else [mask]):
        a.setflags(write=False)
    return s, F, mask


@functools.lru_cache(maxsize=None)
def ragged():
    g = golden("pose.npz")
    scenes, Fs, mask = PC.build_ragged(int(g["r_seed"]))
    arrays = PC.ragged_arrays(scenes)
    np.testing.assert_allclose(PC.checksum(arrays[0], arrays[2], arrays[4], Fs, mask), g["r_chk"], rtol=0, atol=1e-6)
    for a in arrays + (Fs, mask):
        a.setflags(write=False)
    return scenes, arrays, Fs, mask


def run_ops(cuda, kp1, off1, kp2, off2, match, mask, F, Ka, Kb, **kw):
    """the entry itself: (R, t [P, 3], E, front, points3d, front_mask uint8)"""
    from cirtorch import _ops
    p = len(off1) - 1
    full = lambda K: dev(np.ascontiguousarray(np.broadcast_to(K, (p, 3, 3))), cuda)  # noqa: E731
    return _ops.recover_pose(dev(kp1, cuda), dev(off1, cuda), dev(kp2, cuda), dev(off2, cuda), dev(match, cuda),
                             None if mask is None else dev(mask, cuda), dev(F.reshape(p, 3, 3), cuda), full(Ka), full(Kb), **kw)


def run_single(cuda, s, F, mask):
    off1, off2 = np.array([0, len(s["kp1"])], dtype=np.int64), np.array([0, len(s["kp2"])], dtype=np.int64)
    return run_ops(cuda, s["kp1"], off1, s["kp2"], off2, s["match"], mask, F, s["K1"], s["K2"])


def check_pair(got, want, tol, scale, what):
    """got: (R [3, 3], t [3], E [3, 3], front, X [n1, 3], fmask [n1]) numpy; want: (R, t, X, front, fmask)"""
    R, t, E, front, X, fmask = got
    wR, wt, wX, wfront, wfmask = want
    assert front == wfront, what
    np.testing.assert_array_equal(fmask.astype(bool), wfmask, err_msg=what)
    assert np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(X).all() and np.isfinite(E).all()
    if not wR.any():
        assert not R.any() and not t.any() and not E.any() and not X.any() and front == 0, what
        return
    eR, et, eX = np.abs(R - wR).max(), np.abs(t - wt).max(), np.abs(X - wX).max() / scale
    print(what, "front", front, "R err %.3g t err %.3g X err %.3g" % (eR, et, eX), "tol", tol)
    assert eR <= tol[0] and et <= tol[1] and eX <= tol[2], (what, eR, et, eX, tol)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12, what
    assert abs(np.linalg.norm(t) - 1) < 1e-14, what
    sv = np.linalg.svd(E)[1]
    assert np.abs(sv - [1.0, 1.0, 0.0]).max() < 1e-12, (what, sv)
    # E is the essential matrix of the returned motion: [t]_x R up to sign
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    assert min(np.abs(E - tx @ R).max(), np.abs(E + tx @ R).max()) < 1e-12, what
    assert not X[~wX.any(1)].any(), what      # rows that are not used: zeros


def slot_of(cuda, s, F, R, t):
    """the candidate slot of rr.h that (R, t) is, from rr_essential_decompose on E0"""
    from cirtorch.geometry.epipolar import motion_from_essential
    Rs, Ts = motion_from_essential(dev((s["K2"].T @ F @ s["K1"])[None], cuda))
    d = [max(np.abs(Rs[0, c].cpu().numpy() - R).max(), np.abs(Ts[0, c, :, 0].cpu().numpy() - t).max()) for c in range(4)]
    assert min(d) < 1e-9 and sorted(d)[1] > 1e-3, d
    return int(np.argmin(d))


# ---------------------------------------------------------------- against the fixture
@pytest.mark.parametrize("k", range(len(PC.CASES)))
def test_pose_vs_fixture(cuda, k):
    g = golden("pose.npz")
    s, F, mask = pcase(k)
    R, t, E, front, X, fmask = run_single(cuda, s, F, mask)
    assert R.dtype == torch.float64 and t.dtype == torch.float64 and X.dtype == torch.float64 and front.dtype == torch.int32
    assert tuple(R.shape) == (1, 3, 3) and tuple(t.shape) == (1, 3) and tuple(X.shape) == (len(s["kp1"]), 3)
    rows = PC.records(s, mask)[0]
    got = (R[0].cpu().numpy(), t[0].cpu().numpy(), E[0].cpu().numpy(), front.item(), X.cpu().numpy(), fmask.cpu().numpy())
    check_pair(got, (g["p%d_R" % k], g["p%d_t" % k], g["p%d_X" % k], int(g["p%d_front" % k]), g["p%d_fmask" % k]),
               g["p%d_tol" % k], PC.median_depth(s["X"][rows]), NAMES[k])
    if PC.CASES[k]["kind"] == "true" and len(rows):
        assert front.item() == len(rows)      # under the true F every match is in front


def test_four_slots_win(cuda):
    """the seeded motions: which candidate slot wins is the entry's own business, but with both signs of
    every translation component and rotations about every axis at least three of the four occur"""
    slots = []
    for i in range(PC.N_MOTIONS):
        s, F, mask = pcase(NAMES.index("motion%d" % i))
        R, t = run_single(cuda, s, F, mask)[:2]
        slots.append(slot_of(cuda, s, F, R[0].cpu().numpy(), t[0].cpu().numpy()))
    print("winning slots:", slots)
    assert len(set(slots)) >= 3, slots


def test_ragged_batch_vs_fixture(cuda):
    """an empty pair, a pair whose F is all zeros, a pair with 3 matches, a noisy pair and the noise-free pair"""
    from cirtorch.search import recover_pose
    g = golden("pose.npz")
    scenes, (kp1, off1, kp2, off2, match), Fs, mask = ragged()
    R, t, E, front, X, fmask = (o.cpu().numpy() for o in run_ops(cuda, kp1, off1, kp2, off2, match, mask, Fs, PC.K1, PC.K1))
    for p, s in enumerate(scenes):
        a = slice(off1[p], off1[p + 1])
        rows = PC.records(s, mask[a])[0]
        check_pair((R[p], t[p], E[p], front[p], X[a], fmask[a]), (g["r_R"][p], g["r_t"][p], g["r_X"][a], g["r_front"][p], g["r_fmask"][a]),
                   g["r_tol"][p], PC.median_depth(s["X"][rows]), PC.RAGGED[p][0])
    assert front.tolist()[:3] == [0, 0, 3] and not R[:2].any() and not E[:2].any() and not t[:2].any()
    # the noise-free pair (exact in float32): the truth itself
    s, a = scenes[4], slice(off1[4], off1[5])
    pl = s["planted"]
    eR, et = np.abs(R[4] - np.eye(3)).max(), np.abs(t[4] - PC.T_EXACT).max()
    eX = (np.abs(X[a][pl] - s["X"][pl]).max(1) / np.linalg.norm(s["X"][pl], axis=1)).max()
    print("noise-free pair: R err %.3g t err %.3g points rel err %.3g" % (eR, et, eX))
    assert eR < 1e-9 and et < 1e-9 and eX < 1e-7          # |t_true| = 1: no scale enters
    assert front[4] == pl.sum() == 50 and fmask[a][pl].all()
    # x2^T K2^-T E K1^-1 x1 vanishes on it
    Ki = np.linalg.inv(PC.K1)
    x1 = np.concatenate([s["kp1"][pl], np.ones((50, 1))], 1).astype(np.float64) @ Ki.T
    x2 = np.concatenate([s["kp2"][s["match"][pl]], np.ones((50, 1))], 1).astype(np.float64) @ Ki.T
    res = np.abs(np.einsum("ni,ij,nj->n", x2, E[4], x1)).max()
    print("noise-free pair: largest |x2^T E x1| %.3g" % res)
    assert res < 1e-12
    # the Python surface on the same batch: the same bits, its own shapes
    out = recover_pose(dev(kp1, cuda), dev(kp2, cuda), dev(match, cuda), dev(Fs, cuda), dev(PC.K1, cuda), dev(PC.K1, cuda),
                       mask=dev(mask, cuda), offsets1=dev(off1, cuda), offsets2=dev(off2, cuda))
    assert tuple(out[1].shape) == (5, 3, 1) and out[3].dtype == torch.bool and out[4].dtype == torch.int32
    assert bits(out[0]) == R.tobytes() and bits(out[1]) == t.tobytes() and bits(out[2]) == X.tobytes()
    assert np.array_equal(out[3].cpu().numpy(), fmask.astype(bool)) and np.array_equal(out[4].cpu().numpy(), front)


def test_intrinsics_forms_and_k1_ne_k2(cuda):
    """[3, 3] intrinsics == [P, 3, 3] intrinsics bit for bit, with K1 != K2"""
    from cirtorch.search import recover_pose
    s, F, mask = pcase(NAMES.index("k2_40"))
    assert not np.array_equal(s["K1"], s["K2"])
    k1 = dev(np.stack([s["kp1"]] * 3), cuda)
    k2 = dev(np.stack([s["kp2"]] * 3), cuda)
    m, mk, Fm = dev(np.stack([s["match"]] * 3), cuda), dev(np.stack([mask] * 3), cuda), dev(np.stack([F] * 3), cuda)
    a = recover_pose(k1, k2, m, Fm, dev(s["K1"], cuda), dev(s["K2"], cuda), mask=mk)
    b = recover_pose(k1, k2, m, Fm, dev(np.stack([s["K1"]] * 3), cuda), dev(np.stack([s["K2"]] * 3), cuda), mask=mk)
    assert all(bits(x) == bits(y) for x, y in zip(a, b))
    assert a[4].tolist() == [int(golden("pose.npz")["p%d_front" % NAMES.index("k2_40")])] * 3
    assert bits(a[0][0]) == bits(a[0][2]) and bits(a[2][0]) == bits(a[2][1])
    # with the wrong second camera the same data gives another answer
    c = recover_pose(k1, k2, m, Fm, dev(s["K1"], cuda), dev(s["K1"], cuda), mask=mk)
    assert bits(c[0]) != bits(a[0])


# ---------------------------------------------------------------- end to end
def test_verify_then_recover_pose(cuda):
    """verify_pairs(model="fundamental") -> recover_pose on planted pairs, 60 % inliers, 0.3 px noise"""
    from cirtorch.search import recover_pose, verify_pairs
    g = golden("pose.npz")
    scenes = [PC.scene(*spec, int(g["e_seed"]) + 17 * k) for k, spec in enumerate(PC.E2E)]
    kp1, off1, kp2, off2, match = PC.ragged_arrays(scenes)
    np.testing.assert_allclose(PC.checksum(kp1, kp2, match), g["e_chk"], rtol=0, atol=1e-6)
    args = (dev(kp1, cuda), dev(kp2, cuda), dev(match, cuda))
    offs = dict(offsets1=dev(off1, cuda), offsets2=dev(off2, cuda))
    inl, F, mask = verify_pairs(*args, th=PC.VER["th"], iters=PC.VER["iters"], refine=PC.VER["refine"], seed=PC.VER["seed"],
                                model="fundamental", **offs)
    np.testing.assert_array_equal(inl.cpu().numpy(), g["e_inl"])
    K = dev(PC.K1, cuda)
    R, t, X, fmask, front = (o.cpu().numpy() for o in recover_pose(*args, F, K, K, mask=mask, **offs))
    np.testing.assert_array_equal(front, g["e_front"])
    np.testing.assert_array_equal(fmask, g["e_fmask"])
    for p, s in enumerate(scenes):
        a = slice(off1[p], off1[p + 1])
        rows = np.nonzero(g["e_X"][a].any(1))[0]
        eR, et = np.abs(R[p] - g["e_R"][p]).max(), np.abs(t[p, :, 0] - g["e_t"][p]).max()
        eX = np.abs(X[a] - g["e_X"][a]).max() / PC.median_depth(s["X"][rows])
        rot, direc = PC.rot_angle_deg(R[p], s["R"]), PC.dir_angle_deg(t[p, :, 0], s["t"])
        print("end to end pair", p, "inliers", inl[p].item(), "front", front[p], "vs numpy chain: R %.3g t %.3g X %.3g" % (eR, et, eX),
              "tol", g["e_tol"][p], "vs planted: rotation %.4f deg, direction %.4f deg" % (rot, direc))
        assert eR <= g["e_tol"][p][0] and et <= g["e_tol"][p][1] and eX <= g["e_tol"][p][2]
        assert rot < 2.0 and direc < 2.0


# ---------------------------------------------------------------- structure
def test_fused_equals_chain(cuda):
    """rr_recover_pose == rr_essential_decompose + rr_triangulate_points under each candidate + a torch count, bit
    for bit.  With K1 = K2 = I the products inside the fused entry (E0, P1, P2) are exact, so the chain can be
    formed outside: the keypoints are the scene's in normalised coordinates (float32), F its essential matrix."""
    from cirtorch import _ops
    s = PC.scene(300, 310, 257, 1.0, 0.3, 4242)
    Ki, I3 = np.linalg.inv(EC.K), np.eye(3)
    nrm = lambda kp: ((np.concatenate([kp, np.ones((len(kp), 1))], 1).astype(np.float64) @ Ki.T)[:, :2]).astype(np.float32)  # noqa: E731
    kp1, kp2, match = nrm(s["kp1"]), nrm(s["kp2"]), s["match"]
    E0 = EC.K.T @ s["F"] @ EC.K
    E0 = E0 / np.linalg.norm(E0)
    off1, off2 = np.array([0, len(kp1)], dtype=np.int64), np.array([0, len(kp2)], dtype=np.int64)
    R, t, E, front, X, fmask = run_ops(cuda, kp1, off1, kp2, off2, match, None, E0, I3, I3)
    assert front.item() == 257
    R1, R2, tt = _ops.essential_decompose(dev(E0[None], cuda))
    rows = np.nonzero(match >= 0)[0]
    p1, p2 = dev(kp1[rows].astype(np.float64), cuda), dev(kp2[match[rows]].astype(np.float64), cuda)
    off = dev(np.array([0, len(rows)], dtype=np.int64), cuda)
    P1 = torch.cat([torch.eye(3, dtype=torch.float64, device=cuda), torch.zeros(3, 1, dtype=torch.float64, device=cuda)], 1)[None]
    best = None
    for c, (Rc, tc) in enumerate(((R1, tt), (R1, -tt), (R2, tt), (R2, -tt))):
        Xc = _ops.triangulate_points(p1, p2, P1, torch.cat([Rc, tc.unsqueeze(-1)], 2).contiguous(), off)
        inf = (Xc[:, 2] > 0) & ((Xc @ Rc[0].T)[:, 2] + tc[0, 2] > 0)
        n = int(inf.sum().item())
        if best is None or n > best[0]:
            best = (n, c, Rc, tc, Xc, inf)
    n, c, Rc, tc, Xc, inf = best
    print("chain: candidate", c, "front", n)
    assert n == front.item() and bits(Rc) == bits(R) and bits(tc) == bits(t)
    assert bits(Xc) == bits(X[dev(rows, cuda)]) and np.array_equal(inf.cpu().numpy(), fmask.cpu().numpy()[rows].astype(bool))
    assert not X.cpu().numpy()[match < 0].any()


def test_dense_equals_ragged_equals_single(cuda):
    from cirtorch.search import recover_pose
    parts = [PC.scene(70, 64, 40, 1.0, 0.3, 900 + i) for i in range(3)]
    k1, k2, m = (np.stack([q[key] for q in parts]) for key in ("kp1", "kp2", "match"))
    Fs = np.stack([EC.unit(q["F"]) for q in parts])
    K = dev(PC.K1, cuda)
    dense = recover_pose(dev(k1, cuda), dev(k2, cuda), dev(m, cuda), dev(Fs, cuda), K, K)
    off1, off2 = np.arange(4, dtype=np.int64) * 70, np.arange(4, dtype=np.int64) * 64
    rag = recover_pose(dev(k1.reshape(-1, 2), cuda), dev(k2.reshape(-1, 2), cuda), dev(m.reshape(-1), cuda), dev(Fs, cuda), K, K,
                       offsets1=dev(off1, cuda), offsets2=dev(off2, cuda), max_n1=70)
    assert tuple(dense[2].shape) == (3, 70, 3) and tuple(dense[3].shape) == (3, 70) and tuple(rag[2].shape) == (210, 3)
    assert bits(dense[0]) == bits(rag[0]) and bits(dense[1]) == bits(rag[1]) and bits(dense[2]) == bits(rag[2])
    assert torch.equal(dense[3].reshape(-1), rag[3]) and torch.equal(dense[4], rag[4])
    assert dense[4].tolist() == [40, 40, 40] and dense[3].sum(1).tolist() == [40, 40, 40]
    one = recover_pose(dev(k1[1], cuda), dev(k2[1], cuda), dev(m[1], cuda), dev(Fs[1], cuda), K, K)   # one pair, [N, 2] keypoints
    assert tuple(one[0].shape) == (1, 3, 3) and tuple(one[1].shape) == (1, 3, 1) and tuple(one[2].shape) == (70, 3)
    assert bits(one[0][0]) == bits(dense[0][1]) and bits(one[1][0]) == bits(dense[1][1]) and bits(one[2]) == bits(dense[2][1])
    assert torch.equal(one[3], dense[3][1]) and one[4].item() == 40


def test_pair_in_another_batch_and_reruns(cuda):
    """a pair keeps its bits as pair 1 of two pairs and as pair 7 of 44 at another row offset; two runs of one
    call are bit-identical"""
    s, F, mask = pcase(NAMES.index("ver257"))
    fa, fb = PC.scene(30, 28, 20, 1.0, 0.3, 77), PC.scene(55, 50, 35, 1.0, 0.3, 78)

    def batch(front, at, total):
        scenes = [front] * at + [s] + [fa] * (total - at - 1)
        arrays = PC.ragged_arrays(scenes)
        Fs = np.stack([F if q is s else EC.unit(q["F"]) for q in scenes])
        mk = np.concatenate([mask if q is s else np.ones(len(q["kp1"]), dtype=bool) for q in scenes])
        return arrays, Fs, mk, int(arrays[1][at])

    (a1, F1, m1, s0), (a2, F2, m2, b0) = batch(fa, 1, 2), batch(fb, 7, 44)
    x = run_ops(cuda, *a1, m1, F1, PC.K1, PC.K1)
    x2 = run_ops(cuda, *a1, m1, F1, PC.K1, PC.K1)
    assert all(bits(u) == bits(v) for u, v in zip(x, x2))
    y = run_ops(cuda, *a2, m2, F2, PC.K1, PC.K1)
    n1 = len(s["kp1"])
    assert s0 != b0 and x[3][1].item() == int(mask.sum())
    for i in range(4):
        assert bits(x[i][1]) == bits(y[i][7]), i
    assert bits(x[4][s0:s0 + n1]) == bits(y[4][b0:b0 + n1]) and bits(x[5][s0:s0 + n1]) == bits(y[5][b0:b0 + n1])
    # and equals the pair alone
    z = run_single(cuda, s, F, mask)
    assert bits(z[0][0]) == bits(x[0][1]) and bits(z[4]) == bits(x[4][s0:s0 + n1])


def test_graph_capture_replay_equals_eager(cuda):
    """one stream, no parallel branches: the kernel of the call in a torch.cuda.graph"""
    from cirtorch.search import recover_pose
    from cirtorch.utils.graph import GraphedForward
    parts = [PC.scene(70, 64, 40, 1.0, 0.3, 300 + i) for i in range(4)]
    K = dev(PC.K1, cuda)
    # one input tensor per replay: keypoints of both sides, the match list (indices < 2^24: exact in float32) and F
    x = []
    for i in (0, 2):
        q = parts[i:i + 2]
        x.append(torch.cat([dev(np.stack([p["kp1"] for p in q]).reshape(2, -1), cuda), dev(np.stack([p["kp2"] for p in q]).reshape(2, -1), cuda),
                            dev(np.stack([p["match"] for p in q]), cuda).float(),
                            dev(np.stack([EC.unit(p["F"]).astype(np.float32).reshape(-1) for p in q]), cuda)], 1))

    def fn(t):
        a = t[:, :140].reshape(2, 70, 2).contiguous()
        b = t[:, 140:268].reshape(2, 64, 2).contiguous()
        mm = t[:, 268:338].long()
        F = t[:, 338:].reshape(2, 3, 3).double()
        return recover_pose(a, b, mm, F, K, K)

    g = GraphedForward(fn, x[0])
    for t in (x[1], x[0]):
        got = [o.clone() for o in g(t)]
        want = fn(t)
        assert all(bits(u) == bits(v) for u, v in zip(got, want))
        assert want[4].tolist() == [40, 40]


# ---------------------------------------------------------------- the reference-named functions
def test_reference_named_functions(cuda):
    from cirtorch.geometry.epipolar import (decompose_essential_matrix, essential_from_fundamental,
                                            motion_from_essential_choose_solution, projection_from_KRt, triangulate_points)
    g = golden("pose.npz")
    ks = [NAMES.index(n) for n in ("true65", "k2_40", "true257")]
    for k in ks:
        s, F, mask = pcase(k)
        rows, rec = PC.records(s, mask)
        wR, wt, wX, tol = g["p%d_R" % k], g["p%d_t" % k], g["p%d_X" % k][rows], g["p%d_tol" % k]
        scale = PC.median_depth(s["X"][rows])
        K1, K2 = dev(s["K1"][None], cuda), dev(s["K2"][None], cuda)
        x1, x2 = dev(rec[None, :, :2], cuda), dev(rec[None, :, 2:], cuda)
        # triangulate_points under the fixture's motion
        P1 = projection_from_KRt(K1, torch.eye(3, dtype=torch.float64, device=cuda)[None], torch.zeros(1, 3, 1, dtype=torch.float64, device=cuda))
        P2 = projection_from_KRt(K2, dev(wR[None], cuda), dev(wt.reshape(1, 3, 1), cuda))
        X = triangulate_points(P1, P2, x1, x2)
        assert X.dtype == torch.float64 and tuple(X.shape) == (1, len(rows), 3)
        eX = np.abs(X[0].cpu().numpy() - wX).max() / scale
        # decompose_essential_matrix: the fixture's motion is one of the four
        E = essential_from_fundamental(dev(F[None], cuda), K1, K2)
        R1, R2, t = decompose_essential_matrix(E)
        assert tuple(R1.shape) == (1, 3, 3) and tuple(t.shape) == (1, 3, 1)
        eR = min(np.abs(R1[0].cpu().numpy() - wR).max(), np.abs(R2[0].cpu().numpy() - wR).max())
        et = min(np.abs(t[0, :, 0].cpu().numpy() - wt).max(), np.abs(t[0, :, 0].cpu().numpy() + wt).max())
        for Rc in (R1, R2):
            assert abs(torch.det(Rc[0]).item() - 1) < 1e-12
        # motion_from_essential_choose_solution
        R, tt, Xc = motion_from_essential_choose_solution(E, K1, K2, x1, x2)
        e3 = (np.abs(R[0].cpu().numpy() - wR).max(), np.abs(tt[0, :, 0].cpu().numpy() - wt).max(), np.abs(Xc[0].cpu().numpy() - wX).max() / scale)
        print(NAMES[k], "triangulate_points %.3g, decompose R %.3g t %.3g, choose_solution R %.3g t %.3g X %.3g" % ((eX, eR, et) + e3), "tol", tol)
        assert eX <= tol[2] and eR <= tol[0] and et <= tol[1] and e3[0] <= tol[0] and e3[1] <= tol[1] and e3[2] <= tol[2]
        # with a mask: the masked points come back as zeros, the others keep their bits
        half = torch.arange(len(rows), device=cuda)[None] % 2 == 0
        Rm, tm, Xm = motion_from_essential_choose_solution(E, K1, K2, x1, x2, mask=half)
        assert not Xm[0][~half[0]].any() and bits(Xm[0][half[0]]) == bits(Xc[0][half[0]]) and bits(Rm) == bits(R)
        # float32 inputs: float64 arithmetic on the same values, rounded once
        f = lambda a: a.float()  # noqa: E731
        X32 = triangulate_points(f(P1), f(P2), f(x1), f(x2))
        assert X32.dtype == torch.float32 and torch.equal(X32, triangulate_points(f(P1).double(), f(P2).double(), f(x1).double(), f(x2).double()).float())
        d32, d64 = decompose_essential_matrix(f(E)), decompose_essential_matrix(f(E).double())
        assert all(a.dtype == torch.float32 and torch.equal(a, b.float()) for a, b in zip(d32, d64))
        c32 = motion_from_essential_choose_solution(f(E), f(K1), f(K2), f(x1), f(x2))
        c64 = motion_from_essential_choose_solution(f(E).double(), f(K1).double(), f(K2).double(), f(x1).double(), f(x2).double())
        assert all(a.dtype == torch.float32 and torch.equal(a, b.float()) for a, b in zip(c32, c64))
    # a batch: every element chooses its own motion (the reference applies element 0's choice to all)
    Es, Ks, xs1, xs2, want = [], [], [], [], []
    for i in range(4):
        k = NAMES.index("motion%d" % i)
        s, F, _ = pcase(k)
        rows, rec = PC.records(s, None)
        Es.append(s["K2"].T @ F @ s["K1"])
        xs1.append(rec[:, :2])
        xs2.append(rec[:, 2:])
        want.append((g["p%d_R" % k], g["p%d_t" % k], g["p%d_tol" % k]))
    Kb = dev(np.stack([PC.K1] * 4), cuda)
    R, t, X = motion_from_essential_choose_solution(dev(np.stack(Es), cuda), Kb, Kb, dev(np.stack(xs1), cuda), dev(np.stack(xs2), cuda))
    for i, (wR, wt, tol) in enumerate(want):
        assert np.abs(R[i].cpu().numpy() - wR).max() <= tol[0] and np.abs(t[i, :, 0].cpu().numpy() - wt).max() <= tol[1]
