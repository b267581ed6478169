"""Localization on the GPU (rr_localize_pairs / rr_p3p, csrc/rr_pnp.hip and csrc/rr_p3p.h) against the float64
numpy restatement of tests/pnp_cases.py and the pnp.npz fixture: the minimal solver on 257 samples, every
RANSAC case (counts and masks exact, the pose within the fixture's tolerance), the call forms, a pair's
independence of its batch, graph capture, the noise-free pair and the chain
verify_pairs(model="fundamental") -> recover_pose -> localize_pairs of a third planted view."""

import functools

import numpy as np
import pytest
import torch

import epipolar_cases as EC
import pnp_cases as PN
import pose_cases as PC
from conftest import golden

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in PN.ALL_CASES]


def dev(x, cuda):
    return None if x is None else torch.from_numpy(np.array(x)).to(cuda)   # a copy: the cached cases are read-only


def bits(t):
    return t.cpu().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def pcase(k):
    """case k: inputs, the oracle's outputs (computed once, never modified) and the tolerances"""
    g = golden("pnp.npz")
    case = PN.ALL_CASES[k]
    kp, off1, X, valid, off2, match, planted, Ks, parts = PN.build_case(case, int(g["c_seeds"][k]))
    np.testing.assert_allclose(PN.case_checksum(kp, X, match), g["c_chk"][k], rtol=0, atol=1e-6)
    inl, Rs, ts, mask, infos = PN.pnp_batch(kp, off1, X, valid, off2, match, Ks, PN.TH, case["iters"], case["refine"], PN.RUN_SEED)
    np.testing.assert_array_equal(inl, g["c%d_inl" % k])
    np.testing.assert_array_equal(mask, g["c%d_mask" % k])
    for a in (kp, off1, X, off2, match, planted, Ks, inl, Rs, ts, mask) + (() if valid is None else (valid,)):
        a.setflags(write=False)
    return case, (kp, off1, X, valid, off2, match, Ks), (inl, Rs, ts, mask, infos), g["c%d_tol" % k], planted, parts


def case_named(name):
    return pcase(NAMES.index(name))


def run_ragged(cuda, inputs, case, seed=PN.RUN_SEED, **kw):
    from cirtorch.search import localize_pairs
    kp, off1, X, valid, off2, match, Ks = inputs
    return localize_pairs(dev(kp, cuda), dev(X, cuda), dev(match, cuda), dev(Ks, cuda), th=PN.TH, iters=case["iters"],
                          refine=case["refine"], seed=seed, valid=dev(valid, cuda), offsets1=dev(off1, cuda),
                          offsets2=dev(off2, cuda), **kw)


def check_outputs(got, want, tol, what=""):
    inl, R, t, mask = got
    winl, wR, wt, wmask = want[:4]
    assert inl.dtype == torch.int32 and R.dtype == torch.float64 and t.dtype == torch.float64 and mask.dtype == torch.bool
    assert tuple(R.shape) == (len(winl), 3, 3) and tuple(t.shape) == (len(winl), 3, 1)
    np.testing.assert_array_equal(inl.cpu().numpy(), winl, err_msg=what)
    np.testing.assert_array_equal(mask.cpu().numpy(), wmask, err_msg=what)
    Rn, tn = R.cpu().numpy(), t.cpu().numpy()[:, :, 0]
    assert np.isfinite(Rn).all() and np.isfinite(tn).all()
    for p in range(len(winl)):
        if winl[p] == 0:
            assert not Rn[p].any() and not tn[p].any(), what
        else:
            e = PN.pose_err(Rn[p], tn[p], wR[p], wt[p])
            print(what, "pair", p, "inliers", winl[p], "pose err", e, "tol", tol[p])
            assert e <= tol[p], (what, p, e, tol[p])
            assert np.abs(Rn[p] @ Rn[p].T - np.eye(3)).max() < 1e-12 and np.linalg.det(Rn[p]) > 0


# ---------------------------------------------------------------- 1. the minimal solver against the oracle
@functools.lru_cache(maxsize=None)
def solver_set():
    g = golden("pnp.npz")
    x, X, R, t, nsol, drop, diffs, resid = PN.solver_samples(int(g["s_seed"]))
    np.testing.assert_allclose(PN.checksum(x, X), g["s_chk"], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(nsol, g["s_nsol"])
    assert drop <= 0.02 and len(x) >= 256 + 1 - 5
    return x, X, R, t, nsol, g["s_tol"], float(g["s_resid"])


def test_p3p_vs_oracle(cuda):
    from cirtorch.geometry.pnp import solve_p3p
    x, X, R, t, nsol, tol, bound = solver_set()
    Rg, tg, ng = solve_p3p(dev(x, cuda), dev(X, cuda))
    assert tuple(Rg.shape) == (len(x), 4, 3, 3) and tuple(tg.shape) == (len(x), 4, 3)
    assert Rg.dtype == torch.float64 and tg.dtype == torch.float64 and ng.dtype == torch.int32
    Rg, tg, ng = Rg.cpu().numpy(), tg.cpu().numpy(), ng.cpu().numpy()
    np.testing.assert_array_equal(ng, nsol)
    assert set(nsol.tolist()) >= {1, 2, 4}
    worst, res = 0.0, 0.0
    for i in range(len(x)):
        assert not Rg[i, nsol[i]:].any() and not tg[i, nsol[i]:].any()
        for k in range(nsol[i]):
            e = PN.pose_err(Rg[i, k], tg[i, k], R[i, k], t[i, k])
            worst = max(worst, e / tol[i])
            assert e <= tol[i], (i, k, e, tol[i])
            Y = X[i] @ Rg[i, k].T + tg[i, k]
            assert (Y[:, 2] > 0).all()
            res = max(res, float(np.abs(Y[:, :2] / Y[:, 2:] - x[i]).max()))
    print("p3p: %d samples, %d solutions, largest pose error / tolerance %.3g, largest reprojection residual %.3g (bound %.3g)"
          % (len(x), nsol.sum(), worst, res, bound))
    assert res <= bound, (res, bound)


# ---------------------------------------------------------------- 2. every RANSAC case against the oracle
@pytest.mark.parametrize("k", range(len(PN.ALL_CASES)))
def test_localize_pairs_vs_oracle(cuda, k):
    case, inputs, want, tol, _, _ = pcase(k)
    got = run_ragged(cuda, inputs, case)
    check_outputs(got, want, tol, case["name"])
    if case["name"] == "singularK":   # the failed pair gives zeros and its neighbours the oracle's values
        assert got[0].tolist()[1] == 0 and not got[1][1].any() and min(got[0].tolist()[0], got[0].tolist()[2]) >= 18


# ---------------------------------------------------------------- 3. call forms and runs
def dense_parts(seed0, n):
    return [PN.scene(70, 64, 40, 0.6, PN.NOISE, "valid" if s == 1 else "general", seed0 + s) for s in range(n)]


def test_dense_equals_ragged_equals_single(cuda):
    """a dense [P, N, .] batch == the same pairs through the ragged form == each pair alone (as pair p of a batch
    whose other pairs are empty: the hash takes the pair's index), bit for bit; [3, 3] intrinsics == [P, 3, 3];
    float32 points3d are converted once"""
    from cirtorch.search import localize_pairs
    parts = dense_parts(900, 3)
    kp, X, m = (np.stack([q[k] for q in parts]) for k in ("kp", "X", "match"))
    valid = np.stack([np.ones(64, dtype=bool) if q["valid"] is None else q["valid"] for q in parts])
    K = dev(PN.K, cuda)
    kw = dict(th=PN.TH, iters=300, seed=5)
    dense = localize_pairs(dev(kp, cuda), dev(X, cuda), dev(m, cuda), K, valid=dev(valid, cuda), **kw)
    off1, off2 = np.arange(4, dtype=np.int64) * 70, np.arange(4, dtype=np.int64) * 64
    K3 = dev(np.stack([PN.K] * 3), cuda)
    rag = localize_pairs(dev(kp.reshape(-1, 2), cuda), dev(X.reshape(-1, 3), cuda), dev(m.reshape(-1), cuda), K3,
                         valid=dev(valid.reshape(-1), cuda), offsets1=dev(off1, cuda), offsets2=dev(off2, cuda), max_n1=70, **kw)
    assert tuple(dense[3].shape) == (3, 70) and tuple(rag[3].shape) == (210,) and tuple(dense[2].shape) == (3, 3, 1)
    assert torch.equal(dense[0], rag[0]) and torch.equal(dense[3].reshape(-1), rag[3])
    assert bits(dense[1]) == bits(rag[1]) and bits(dense[2]) == bits(rag[2])
    assert dense[0].min().item() >= 12 and dense[3].sum(1).tolist() == dense[0].tolist()
    # pair 0 alone, in the one-pair form ([N1, 2], [N2, 3], [N1], [N2]): the same p = 0, the same bits
    one = localize_pairs(dev(kp[0], cuda), dev(X[0], cuda), dev(m[0], cuda), K, valid=dev(valid[0], cuda), **kw)
    assert tuple(one[0].shape) == (1,) and tuple(one[1].shape) == (1, 3, 3) and tuple(one[2].shape) == (1, 3, 1)
    assert tuple(one[3].shape) == (70,)
    assert one[0][0] == dense[0][0] and bits(one[1][0]) == bits(dense[1][0]) and bits(one[2][0]) == bits(dense[2][0])
    assert torch.equal(one[3], dense[3][0])
    x32 = torch.from_numpy(X.astype(np.float32)).to(cuda)
    a = localize_pairs(dev(kp, cuda), x32, dev(m, cuda), K, **kw)
    b = localize_pairs(dev(kp, cuda), x32.double(), dev(m, cuda), K, **kw)
    assert all(bits(u) == bits(v) for u, v in zip(a, b))


def test_pair_in_another_batch_and_reruns(cuda):
    """a pair keeps its bits (inliers, mask, pose) when the batch around it changes: as pair 1 of two pairs, and
    as pair 1 of 44 at another row offset (the hash takes the pair's index p, so p is held equal); two runs
    of one call are bit-identical"""
    case, inputs, want, tol, _, _ = case_named("m40")
    kp, off1, X, valid, off2, match, Ks = inputs
    n1 = len(kp)
    fa = PN.scene(30, 28, 20, 0.6, PN.NOISE, "general", 77)
    fb = PN.scene(55, 50, 35, 0.6, PN.NOISE, "general", 78)
    me = dict(kp=kp, X=X, match=match)

    def batch(front, extra):
        parts = [front, me] + [fa] * extra
        o1 = np.cumsum([0] + [len(q["kp"]) for q in parts]).astype(np.int64)
        o2 = np.cumsum([0] + [len(q["X"]) for q in parts]).astype(np.int64)
        return (np.concatenate([q["kp"] for q in parts]), o1, np.concatenate([q["X"] for q in parts]), None, o2,
                np.concatenate([q["match"] for q in parts]), np.stack([PN.K] * len(parts))), int(o1[1])

    small, s0 = batch(fa, 0)
    big, b0 = batch(fb, 42)
    a = run_ragged(cuda, small, case)
    a2 = run_ragged(cuda, small, case)
    assert all(bits(x) == bits(y) for x, y in zip(a, a2))
    d = run_ragged(cuda, big, case)
    assert s0 != b0 and a[0][1].item() >= 18
    assert bits(a[0][1:2]) == bits(d[0][1:2]) and bits(a[1][1:2]) == bits(d[1][1:2]) and bits(a[2][1:2]) == bits(d[2][1:2])
    assert bits(a[3][s0:s0 + n1]) == bits(d[3][b0:b0 + n1])
    # the pair at p = 1 draws another sample stream than the fixture's p = 0: checked against the oracle at p = 1
    o = PN.pnp_pair(kp, X, None, match, Ks[0], 1, PN.TH, case["iters"], case["refine"], PN.RUN_SEED)
    assert o["margin"] >= 1e-7 and a[0][1].item() == o["inliers"]
    np.testing.assert_array_equal(a[3][s0:s0 + n1].cpu().numpy(), o["mask"])


HEAVY = (80, 90, 60, 0.25, PN.NOISE, "general", 4242)   # 45 of 60 matches are outliers


def test_seed_changes_the_winner(cuda):
    """three seeds give three winners.  On the outlier-heavy pair (a quarter of its matches planted) nothing
    but the samples decides which hypothesis first hits three planted records: the oracle's winning t
    differs with the seed and the engine returns each seed's own count, mask and pose.  On the all-outlier
    case every sample scores its own three records, so t = 0 wins by the tie rule for every seed; its
    sample, and with it the pose and the mask, still change with the seed."""
    from cirtorch.search import localize_pairs
    q = PN.scene(*HEAVY)
    ts, poses = [], []
    for seed in (PN.RUN_SEED, 1, 2):
        a, b = (PN.pnp_pair(q["kp"], q["X"], None, q["match"], PN.K, 0, PN.TH, 300, 2, seed, route) for route in "AB")
        tol = max(100 * PN.pose_err(b["R"], b["t"], a["R"], a["t"]), 1e-12)
        assert min(a["margin"], b["margin"]) >= 1e-7 and (a["t_win"], a["sol"], a["inliers"]) == (b["t_win"], b["sol"], b["inliers"])
        got = localize_pairs(dev(q["kp"], cuda), dev(q["X"], cuda), dev(q["match"], cuda), dev(PN.K, cuda), th=PN.TH, iters=300,
                             refine=2, seed=seed)
        e = PN.pose_err(got[1][0].cpu().numpy(), got[2][0, :, 0].cpu().numpy(), a["R"], a["t"])
        print("heavy: seed", seed, "winner", a["t_win"], a["sol"], "inliers", a["inliers"], "margin", a["margin"], "pose err", e, "tol", tol)
        assert got[0].item() == a["inliers"] >= 12 and e <= tol
        np.testing.assert_array_equal(got[3].cpu().numpy(), a["mask"])
        ts.append(a["t_win"])
        poses.append(bits(got[1]) + bits(got[2]))
    assert len(set(ts)) == 3 and len(set(poses)) == 3, ts
    case, inputs, want, tol, _, _ = case_named("outliers")
    kp, off1, X, valid, off2, match, Ks = inputs
    first = run_ragged(cuda, inputs, case)
    poses = [bits(first[1]) + bits(first[2])]
    for seed in (1, 2):
        o = PN.pnp_pair(kp, X, valid, match, Ks[0], 0, PN.TH, case["iters"], case["refine"], seed)
        got = run_ragged(cuda, inputs, case, seed=seed)
        print("outliers: seed", seed, "winner", o["t_win"], o["sol"], "inliers", o["inliers"], "margin", o["margin"])
        assert o["margin"] >= 1e-7 and got[0].item() == o["inliers"]
        np.testing.assert_array_equal(got[3].cpu().numpy(), o["mask"])
        poses.append(bits(got[1]) + bits(got[2]))
    assert len(set(poses)) == 3


def test_graph_capture_replay_equals_eager(cuda):
    """one stream, no parallel branches: the three kernels of the call in a torch.cuda.graph"""
    from cirtorch.search import localize_pairs
    from cirtorch.utils.graph import GraphedForward
    parts = dense_parts(300, 4)
    kp = [dev(np.stack([q["kp"] for q in parts[i:i + 2]]), cuda) for i in (0, 2)]
    X = [dev(np.stack([q["X"] for q in parts[i:i + 2]]), cuda) for i in (0, 2)]
    m = [dev(np.stack([q["match"] for q in parts[i:i + 2]]), cuda) for i in (0, 2)]
    K = dev(np.stack([PN.K] * 2), cuda)
    # one float64 input tensor per replay: keypoints (float32 values), points and the match list (exact in float64)
    x = [torch.cat([kp[i].double().reshape(2, -1), X[i].reshape(2, -1), m[i].double()], 1) for i in (0, 1)]

    def fn(t):
        a = t[:, :140].reshape(2, 70, 2).float().contiguous()
        b = t[:, 140:332].reshape(2, 64, 3).contiguous()
        mm = t[:, 332:].long()
        return localize_pairs(a, b, mm, K, th=PN.TH, iters=300, refine=2, seed=9)

    g = GraphedForward(fn, x[0])
    for t in (x[1], x[0]):
        gi, gR, gt, gm = [o.clone() for o in g(t)]
        ei, eR, et, em = fn(t)
        assert torch.equal(gi, ei) and torch.equal(gm, em) and bits(gR) == bits(eR) and bits(gt) == bits(et)
        assert ei.min().item() >= 12


# ---------------------------------------------------------------- 4. the noise-free pair
def test_noise_free_pair(cuda):
    """keypoints on a 1/16 px grid (exact in float32) that are the projections of their points: every planted
    match is an inlier and the pose is the planted one within the fixture's bound"""
    g = golden("pnp.npz")
    case, inputs, want, tol, planted, parts = case_named("exact")
    got = run_ragged(cuda, inputs, case)
    check_outputs(got, want, tol, "exact")
    assert planted.sum() == 50 and got[0].item() == 50 and got[3].cpu().numpy()[planted].all()
    e = PN.pose_err(got[1][0].cpu().numpy(), got[2][0, :, 0].cpu().numpy(), parts[0]["R"], parts[0]["t"])
    print("noise-free pair: against the planted pose", e, "bound", float(g["x_tol"]))
    assert e <= g["x_tol"]


# ---------------------------------------------------------------- 5. the chain
def test_chain_localizes_a_third_view(cuda):
    """verify_pairs(model="fundamental") -> recover_pose -> localize_pairs(valid=front_mask), all on the device:
    the third camera's rotation and translation direction in view a's frame (the scale is not observable)"""
    from cirtorch.search import localize_pairs, recover_pose, verify_pairs
    case, inputs, want, tol, planted, parts = case_named("chain")
    ch = parts[0]["chain"]
    ab = ch["ab"]
    a_kp, b_kp, m_ab = dev(ab["kp1"], cuda), dev(ab["kp2"], cuda), dev(ab["match"], cuda)
    inl, F, m = verify_pairs(a_kp, b_kp, m_ab, model="fundamental", **PN.CHAIN_VER)
    Rab, tab, X, front_mask, front = recover_pose(a_kp, b_kp, m_ab, F, dev(ab["K1"], cuda), dev(ab["K2"], cuda), mask=m)
    assert tuple(X.shape) == (len(ab["kp1"]), 3) and X.dtype == torch.float64 and front.item() >= 0.9 * inl.item()
    li, R, t, mask = localize_pairs(dev(ch["kq"], cuda), X, dev(ch["match"], cuda), dev(ch["Kq"], cuda), th=PN.TH,
                                    iters=case["iters"], refine=case["refine"], seed=PN.RUN_SEED, valid=front_mask)
    rot = PC.rot_angle_deg(R[0].cpu().numpy(), ch["Rq"])
    direc = PC.dir_angle_deg(t[0, :, 0].cpu().numpy(), ch["tq"])
    got = int((mask.cpu().numpy() & ch["planted"]).sum())
    print("chain: a-b inliers %d front %d; query inliers %d (planted %d, recovered %d); against the planted pose: rotation %.4f deg, "
          "direction %.4f deg" % (inl.item(), front.item(), li.item(), ch["planted"].sum(), got, rot, direc))
    assert li.item() >= 0.8 * ch["planted"].sum() and got >= 0.8 * ch["planted"].sum()
    assert rot < 2.0 and direc < 2.0


def test_rerank_by_inliers_takes_the_counts(cuda):
    """rerank_by_inliers works on localize_pairs' counts unchanged"""
    from cirtorch.search import rerank_by_inliers
    case, inputs, want, tol, _, _ = case_named("ragged4")
    inl = run_ragged(cuda, inputs, case)[0]
    idx = torch.arange(4, device=cuda).view(4, 1)
    order = rerank_by_inliers(idx, inl.view(4, 1))
    assert order.view(-1).tolist() == [3, 2, 0, 1] and inl.tolist() == want[0].tolist()
