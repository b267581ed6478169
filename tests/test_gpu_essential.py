"""Calibrated verification on the GPU (rr_verify_pairs_essential / rr_essential_5pt, csrc/rr_epipolar.hip
and csrc/rr_fivepoint.h) against the float64 numpy restatement of tests/essential_cases.py and the
essential.npz fixture: the minimal solver on 257 samples, every RANSAC case (counts and masks exact,
E within the fixture's tolerance, singular values (s, s, 0)), the call forms, a pair's independence of
its batch, graph capture, the noise-free pair, the planar pair through recover_pose and the chain
verify_pairs(model="essential") -> fundamental_from_essential -> recover_pose."""

import functools

import numpy as np
import pytest
import torch

import epipolar_cases as EC
import essential_cases as SC
import pose_cases as PC
from conftest import golden

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in SC.ALL_CASES]


def dev(x, cuda):
    return torch.from_numpy(np.array(x)).to(cuda)   # a copy: the cached cases are read-only


def bits(t):
    return t.cpu().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def ecase(k):
    """case k: inputs, the oracle's outputs (computed once, never modified) and the tolerances"""
    g = golden("essential.npz")
    case = SC.ALL_CASES[k]
    kp1, off1, kp2, off2, match, planted, K1, K2, parts = SC.build_case(case, int(g["c_seeds"][k]))
    np.testing.assert_allclose(SC.checksum(kp1, kp2, match), g["c_chk"][k], rtol=0, atol=1e-6)
    inl, Es, mask, infos = SC.essential_batch(kp1, off1, kp2, off2, match, K1, K2, SC.TH, case["iters"], case["refine"], SC.RUN_SEED)
    np.testing.assert_array_equal(inl, g["c%d_inl" % k])
    np.testing.assert_array_equal(mask, g["c%d_mask" % k])
    for a in (kp1, off1, kp2, off2, match, planted, K1, K2, inl, Es, mask):
        a.setflags(write=False)
    return case, (kp1, off1, kp2, off2, match, K1, K2), (inl, Es, mask, infos), g["c%d_tol" % k], planted, parts


def case_named(name):
    return ecase(NAMES.index(name))


def run_ragged(cuda, inputs, case, seed=SC.RUN_SEED, **kw):
    from cirtorch.search import verify_pairs
    kp1, off1, kp2, off2, match, K1, K2 = inputs
    return verify_pairs(dev(kp1, cuda), dev(kp2, cuda), dev(match, cuda), th=SC.TH, iters=case["iters"], refine=case["refine"],
                        seed=seed, offsets1=dev(off1, cuda), offsets2=dev(off2, cuda), model="essential", K1=dev(K1, cuda),
                        K2=dev(K2, cuda), **kw)


def check_outputs(got, want, tol, what=""):
    inl, E, mask = got
    winl, wE, wmask = want[:3]
    assert inl.dtype == torch.int32 and E.dtype == torch.float64 and mask.dtype == torch.bool
    assert tuple(E.shape) == (len(winl), 3, 3)
    np.testing.assert_array_equal(inl.cpu().numpy(), winl, err_msg=what)
    np.testing.assert_array_equal(mask.cpu().numpy(), wmask, err_msg=what)
    En = E.cpu().numpy()
    assert np.isfinite(En).all()
    for p in range(len(winl)):
        if winl[p] == 0:
            assert not En[p].any(), what
        else:
            e = EC.f_err(En[p], wE[p])
            sv = np.linalg.svd(En[p], compute_uv=False)
            print(what, "pair", p, "inliers", winl[p], "E err", e, "tol", tol[p], "singular values", sv)
            assert e <= tol[p], (what, p, e, tol[p])
            # rr.h step e: unit Frobenius norm, the largest entry positive, singular values (s, s, 0)
            assert abs(np.sqrt((En[p] ** 2).sum()) - 1) < 1e-14 and En[p].reshape(-1)[np.argmax(np.abs(En[p]))] > 0
            assert abs(sv[0] - sv[1]) <= 1e-12 * sv[0] and sv[2] <= 1e-12 * sv[0], sv


# ---------------------------------------------------------------- 1. the minimal solver against the oracle
@functools.lru_cache(maxsize=None)
def solver_set():
    g = golden("essential.npz")
    x1, x2, E, nroots, drop, diffs, resid = SC.solver_samples(int(g["s_seed"]))
    np.testing.assert_allclose(SC.checksum(x1, x2), g["s_chk"], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(nroots, g["s_nroots"])
    assert drop <= 0.02 and len(x1) >= 256 + 1 - 5
    return x1, x2, E, nroots, g["s_tol"], float(g["s_resid"])


def test_five_point_vs_oracle(cuda):
    from cirtorch.geometry.epipolar import run_5point
    x1, x2, E, nroots, tol, bound = solver_set()
    Eg, ng = run_5point(dev(x1, cuda), dev(x2, cuda))
    assert tuple(Eg.shape) == (len(x1), 10, 3, 3) and Eg.dtype == torch.float64 and ng.dtype == torch.int32
    Eg, ng = Eg.cpu().numpy(), ng.cpu().numpy()
    np.testing.assert_array_equal(ng, nroots)
    assert set(nroots.tolist()) >= {2, 4, 6}
    h1 = np.concatenate([x1, np.ones(x1.shape[:2] + (1,))], -1)
    h2 = np.concatenate([x2, np.ones(x2.shape[:2] + (1,))], -1)
    worst, res = 0.0, 0.0
    for t in range(len(x1)):
        assert not Eg[t, nroots[t]:].any()
        for k in range(nroots[t]):
            e = EC.f_err(Eg[t, k], E[t, k])
            worst = max(worst, e / tol[t])
            assert e <= tol[t], (t, k, e, tol[t])
            assert abs(np.sqrt((Eg[t, k] ** 2).sum()) - 1) < 1e-14
            res = max(res, float(np.abs(np.einsum("ja,ab,jb->j", h2[t], Eg[t, k], h1[t])).max()))
    print("five-point: %d samples, %d solutions, largest E error / tolerance %.3g, largest |h2^T E h1| %.3g (bound %.3g)"
          % (len(x1), nroots.sum(), worst, res, bound))
    assert res <= bound, (res, bound)


# ---------------------------------------------------------------- 2. every RANSAC case against the oracle
@pytest.mark.parametrize("k", range(len(SC.ESS_CASES)))
def test_essential_pairs_vs_oracle(cuda, k):
    case, inputs, want, tol, _, _ = ecase(k)
    got = run_ragged(cuda, inputs, case)
    check_outputs(got, want, tol, case["name"])
    if case["name"] == "singularK":   # the failed pair gives zeros and its neighbours the oracle's values
        assert got[0].tolist()[1] == 0 and not got[1][1].any() and min(got[0].tolist()[0], got[0].tolist()[2]) >= 18


# ---------------------------------------------------------------- 3. call forms and runs
def test_dense_equals_ragged(cuda):
    """a dense [P, N, 2] batch == the same pairs through the ragged form, bit for bit; [3, 3] intrinsics ==
    [P, 3, 3] intrinsics"""
    from cirtorch.search import verify_pairs
    parts = [EC.planted_pair(70, 64, 40, 0.6, 0.3, 900 + s) for s in range(3)]
    k1, k2, m = (np.stack([q[i] for q in parts]) for i in range(3))
    K = dev(SC.K, cuda)
    kw = dict(th=SC.TH, iters=300, seed=5, model="essential")
    dense = verify_pairs(dev(k1, cuda), dev(k2, cuda), dev(m, cuda), K1=K, K2=K, **kw)
    off1, off2 = np.arange(4, dtype=np.int64) * 70, np.arange(4, dtype=np.int64) * 64
    K3 = dev(np.stack([SC.K] * 3), cuda)
    rag = verify_pairs(dev(k1.reshape(-1, 2), cuda), dev(k2.reshape(-1, 2), cuda), dev(m.reshape(-1), cuda),
                       offsets1=dev(off1, cuda), offsets2=dev(off2, cuda), max_n1=70, K1=K3, K2=K3, **kw)
    assert tuple(dense[2].shape) == (3, 70) and tuple(rag[2].shape) == (210,)
    assert torch.equal(dense[0], rag[0]) and torch.equal(dense[2].reshape(-1), rag[2]) and bits(dense[1]) == bits(rag[1])
    assert dense[0].min().item() >= 18 and dense[2].sum(1).tolist() == dense[0].tolist()
    one = verify_pairs(dev(k1[1], cuda), dev(k2[1], cuda), dev(m[1], cuda), K1=K, K2=K, **kw)   # one pair, [N, 2] keypoints
    assert tuple(one[0].shape) == (1,) and tuple(one[1].shape) == (1, 3, 3) and tuple(one[2].shape) == (70,)


def test_pair_in_another_batch_and_reruns(cuda):
    """a pair keeps its bits (inliers, mask, E) when the batch around it changes: as pair 1 of two pairs,
    and as pair 1 of 44 at another row offset (the hash takes the pair's index p, so p is held equal);
    two runs of one call are bit-identical"""
    case, inputs, want, tol, _, _ = case_named("m40")
    kp1, off1, kp2, off2, match, K1, K2 = inputs
    n1 = len(kp1)
    fa = EC.planted_pair(30, 28, 20, 0.6, 0.3, 77)
    fb = EC.planted_pair(55, 50, 35, 0.6, 0.3, 78)

    def batch(front, extra):
        parts = [front, (kp1, kp2, match)] + [fa] * extra
        o1 = np.cumsum([0] + [len(q[0]) for q in parts]).astype(np.int64)
        o2 = np.cumsum([0] + [len(q[1]) for q in parts]).astype(np.int64)
        Ks = np.stack([SC.K] * len(parts))
        return (np.concatenate([q[0] for q in parts]), o1, np.concatenate([q[1] for q in parts]), o2,
                np.concatenate([q[2] for q in parts]), Ks, Ks), int(o1[1])

    small, s0 = batch(fa, 0)
    big, b0 = batch(fb, 42)
    a = run_ragged(cuda, small, case)
    a2 = run_ragged(cuda, small, case)
    assert all(bits(x) == bits(y) for x, y in zip(a, a2))
    d = run_ragged(cuda, big, case)
    assert s0 != b0 and a[0][1].item() >= 18
    assert bits(a[0][1:2]) == bits(d[0][1:2]) and bits(a[1][1:2]) == bits(d[1][1:2])
    assert bits(a[2][s0:s0 + n1]) == bits(d[2][b0:b0 + n1])
    # the pair alone is p = 0: another sample stream, checked against the oracle at p = 0 (the fixture) and p = 1
    alone = run_ragged(cuda, inputs, case)
    b = run_ragged(cuda, inputs, case)
    assert all(bits(x) == bits(y) for x, y in zip(alone, b))
    check_outputs(alone, want, tol, "m40 alone")
    o = SC.essential_pair(kp1, kp2, match, K1[0], K2[0], 1, SC.TH, case["iters"], case["refine"], SC.RUN_SEED)
    assert o["margin"] >= 1e-7 and a[0][1].item() == o["inliers"]
    np.testing.assert_array_equal(a[2][s0:s0 + n1].cpu().numpy(), o["mask"])


def test_seed_changes_the_winner(cuda):
    """the all-outlier case: nothing but the samples decides, so another seed has another winner t in
    the oracle, and the engine returns each seed's own count, mask and E"""
    case, inputs, want, tol, _, _ = case_named("outliers")
    kp1, off1, kp2, off2, match, K1, K2 = inputs
    ts, Es = [want[3][0]["t"]], [bits(run_ragged(cuda, inputs, case)[1])]
    for seed in (1, 2):
        o = SC.essential_pair(kp1, kp2, match, K1[0], K2[0], 0, SC.TH, case["iters"], case["refine"], seed)
        got = run_ragged(cuda, inputs, case, seed=seed)
        print("seed", seed, "winner", o["t"], o["root"], "inliers", o["inliers"], "margin", o["margin"])
        assert o["margin"] >= 1e-7 and got[0].item() == o["inliers"]
        np.testing.assert_array_equal(got[2].cpu().numpy(), o["mask"])
        ts.append(o["t"])
        Es.append(bits(got[1]))
    assert len(set(ts)) == 3 and len(set(Es)) == 3, ts


def test_graph_capture_replay_equals_eager(cuda):
    """one stream, no parallel branches: the three kernels of the call in a torch.cuda.graph"""
    from cirtorch.search import verify_pairs
    from cirtorch.utils.graph import GraphedForward
    parts = [EC.planted_pair(70, 64, 40, 0.6, 0.3, 300 + s) for s in range(4)]
    k1 = [dev(np.stack([q[0] for q in parts[i:i + 2]]), cuda) for i in (0, 2)]
    k2 = [dev(np.stack([q[1] for q in parts[i:i + 2]]), cuda) for i in (0, 2)]
    m = [dev(np.stack([q[2] for q in parts[i:i + 2]]), cuda) for i in (0, 2)]
    K = dev(np.stack([SC.K] * 2), cuda)
    # one input tensor per replay: keypoints of both sides and the match list (indices < 2^24: exact in float32)
    x = [torch.cat([k1[i].reshape(2, -1), k2[i].reshape(2, -1), m[i].float()], 1) for i in (0, 1)]

    def fn(t):
        a = t[:, :140].reshape(2, 70, 2).contiguous()
        b = t[:, 140:268].reshape(2, 64, 2).contiguous()
        mm = t[:, 268:].long()
        return verify_pairs(a, b, mm, th=SC.TH, iters=300, refine=2, seed=9, model="essential", K1=K, K2=K)

    g = GraphedForward(fn, x[0])
    for t in (x[1], x[0]):
        gi, gE, gm = [o.clone() for o in g(t)]
        ei, eE, em = fn(t)
        assert torch.equal(gi, ei) and torch.equal(gm, em) and bits(gE) == bits(eE)
        assert ei.min().item() >= 18


# ---------------------------------------------------------------- 4. the noise-free pair
def test_noise_free_pair(cuda):
    """the `exact` construction of planted_pair (noise-free in float32): every planted match is an inlier
    and fundamental_from_essential(E, K, K) is the true F up to scale"""
    from cirtorch.geometry.epipolar import fundamental_from_essential
    case, inputs, want, tol, planted, parts = case_named("exact")
    got = run_ragged(cuda, inputs, case)
    check_outputs(got, want, tol, "exact")
    assert planted.sum() == 50 and got[0].item() == 50 and got[2].cpu().numpy()[planted].all()
    K = dev(SC.K, cuda)
    F = fundamental_from_essential(got[1][0], K, K).cpu().numpy()
    e = EC.f_err(F, parts[0]["F"])
    print("noise-free pair: F from E against the true F", e, "tol", tol[0])
    assert e <= tol[0]


# ---------------------------------------------------------------- 5. the planar pair
def test_planar_pair_through_recover_pose(cuda):
    """counts and mask exact on a plane (test 2 checks them too); recover_pose on the result puts points
    in front, and its motion is one of the two a plane admits: every triangulated point reprojects
    within th into both views.  The true motion is not compared: the twisted twin may win."""
    from cirtorch.geometry.epipolar import fundamental_from_essential
    from cirtorch.search import recover_pose
    g = golden("essential.npz")
    case, inputs, want, tol, planted, parts = case_named("planar")
    kp1, off1, kp2, off2, match, K1, K2 = inputs
    inl, E, mask = run_ragged(cuda, inputs, case)
    check_outputs((inl, E, mask), want, tol, "planar")
    false_e = int((mask.cpu().numpy() & ~planted).sum())
    print("planar pair: false inliers essential %d (fixture %d), fundamental %d" % (false_e, g["planar_false"][0], g["planar_false"][1]))
    assert false_e == g["planar_false"][0] <= g["planar_false"][1]
    Ka, Kb = dev(K1[0], cuda), dev(K2[0], cuda)
    F = fundamental_from_essential(E, Ka[None], Kb[None])
    R, t, X, fmask, front = recover_pose(dev(kp1, cuda), dev(kp2, cuda), dev(match, cuda), F[0], Ka, Kb, mask=mask[None][0])
    R, t, X, fmask = R[0].cpu().numpy(), t[0].cpu().numpy(), X.cpu().numpy().reshape(-1, 3), fmask.cpu().numpy().reshape(-1)
    assert front.item() > 0 and fmask.sum() == front.item()
    rows = np.nonzero(fmask)[0]
    p1 = X[rows] @ K1[0].T
    p2 = (X[rows] @ R.T + t[:, 0]) @ K2[0].T
    e1 = np.linalg.norm(p1[:, :2] / p1[:, 2:] - kp1[rows], axis=1).max()
    e2 = np.linalg.norm(p2[:, :2] / p2[:, 2:] - kp2[match[rows]], axis=1).max()
    print("planar pair: front %d of %d inliers, largest reprojection error px %.3g / %.3g" % (front.item(), inl.item(), e1, e2))
    assert e1 <= SC.TH and e2 <= SC.TH


# ---------------------------------------------------------------- 6. the chain
def test_chain_recovers_the_planted_motion(cuda):
    """verify_pairs(model="essential") -> fundamental_from_essential -> recover_pose with K2 != K1"""
    from cirtorch.geometry.epipolar import fundamental_from_essential
    from cirtorch.search import recover_pose
    case, inputs, want, tol, planted, parts = case_named("chain")
    kp1, off1, kp2, off2, match, K1, K2 = inputs
    assert not np.array_equal(K1[0], K2[0])
    inl, E, mask = run_ragged(cuda, inputs, case)
    check_outputs((inl, E, mask), want, tol, "chain")
    Ka, Kb = dev(K1[0], cuda), dev(K2[0], cuda)
    F = fundamental_from_essential(E[0], Ka, Kb)
    R, t, X, fmask, front = recover_pose(dev(kp1, cuda), dev(kp2, cuda), dev(match, cuda), F, Ka, Kb, mask=mask)
    s = parts[0]
    rot, direc = PC.rot_angle_deg(R[0].cpu().numpy(), s["R"]), PC.dir_angle_deg(t[0, :, 0].cpu().numpy(), s["t"])
    print("chain: inliers %d front %d, against the planted motion: rotation %.4f deg, direction %.4f deg" % (
        inl.item(), front.item(), rot, direc))
    assert front.item() >= 0.9 * inl.item()
    assert rot < 2.0 and direc < 2.0
