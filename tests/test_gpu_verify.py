"""Spatial verification on the GPU (rr_verify_pairs / rr_homography_dlt, cirtorch.search.verify_pairs,
cirtorch.geometry.homography) against the H matrices the reference's homography.py produced in
float64 (tests/golden/verify.npz) and the float64 numpy restatement of tests/verify_cases.py.

Tolerances.  Inlier counts and masks are exact: the fixture's generator asserts that no residual
of any hypothesis or refit lies within 1e-7 px of th, six orders above float64 rounding on pixel
coordinates.  H matrices are compared by the transfer of the four image corners in pixels against
the fixture's per-case tol_px: 100 x the difference between two other solvers (numpy's eigh /
solve and the reference's torch.svd) on the same points, floor 1e-9 px (make_golden_verify.py)."""

import functools

import numpy as np
import pytest
import torch

import verify_cases as VC
from conftest import golden

pytestmark = pytest.mark.gpu


def dev(x, cuda):
    return torch.from_numpy(np.array(x)).to(cuda)   # a copy: the cached cases are read-only


@functools.lru_cache(maxsize=None)
def vcase(k):
    """case k: inputs, the oracle's outputs (computed once, never modified) and tol_px"""
    g = golden("verify.npz")
    case = VC.VERIFY_CASES[k]
    kp1, off1, kp2, off2, match, planted = VC.build_case(case, int(g["v_seeds"][k]))
    np.testing.assert_allclose(VC.checksum(kp1, kp2, match), g["v_chk"][k], rtol=0, atol=1e-6)
    inl, Hs, mask, infos = VC.verify_batch(kp1, off1, kp2, off2, match, VC.TH, case["iters"], case["refine"], VC.RUN_SEED)
    np.testing.assert_array_equal(inl, g["v%d_inl" % k])
    for a in (kp1, off1, kp2, off2, match, inl, Hs, mask):
        a.setflags(write=False)
    return case, (kp1, off1, kp2, off2, match), (inl, Hs, mask, infos), g["v%d_tol" % k]


def run_ragged(cuda, inputs, case, seed=VC.RUN_SEED, **kw):
    from cirtorch.search import verify_pairs
    kp1, off1, kp2, off2, match = inputs
    return verify_pairs(dev(kp1, cuda), dev(kp2, cuda), dev(match, cuda), th=VC.TH, iters=case["iters"],
                        refine=case["refine"], seed=seed, offsets1=dev(off1, cuda), offsets2=dev(off2, cuda), **kw)


def check_outputs(got, want, tol, what=""):
    inl, H, mask = got
    winl, wH, wmask = want[:3]
    assert inl.dtype == torch.int32 and H.dtype == torch.float64 and mask.dtype == torch.bool
    assert tuple(H.shape) == (len(winl), 3, 3)
    np.testing.assert_array_equal(inl.cpu().numpy(), winl, err_msg=what)
    np.testing.assert_array_equal(mask.cpu().numpy(), wmask, err_msg=what)
    Hn = H.cpu().numpy()
    assert np.isfinite(Hn).all()
    for p in range(len(winl)):
        if winl[p] == 0:
            assert not Hn[p].any(), what
        else:
            e = VC.corner_err(Hn[p], wH[p])
            print(what, "pair", p, "inliers", winl[p], "corner err px", e, "tol", tol[p])
            assert e <= tol[p], (what, p, e, tol[p])


# ---------------------------------------------------------------- DLT against the reference
@functools.lru_cache(maxsize=None)
def dcase(k):
    g = golden("verify.npz")
    b, n, weighted = VC.DLT_CASES[k]
    p1, p2, w = VC.dlt_points(b, n, weighted, int(g["dlt_seeds"][k]))
    np.testing.assert_allclose(VC.checksum(p1, p2, np.ones((b, n)) if w is None else w), g["dlt_chk"][k], rtol=0, atol=1e-6)
    return p1, p2, w, g["dlt%d_H" % k], g["dlt%d_Hit" % k], float(g["dlt_tol"][k]), float(g["dlt_tol_it"][k])


@pytest.mark.parametrize("k", range(len(VC.DLT_CASES)))
def test_dlt_vs_reference(cuda, k):
    """find_homography_dlt / find_homography_dlt_iterated == the reference's float64 H within tol_px;
    float32 input == .float() of the float64-input result of the same values"""
    from cirtorch.geometry.homography import find_homography_dlt, find_homography_dlt_iterated
    p1, p2, w, Hr, Hi, tol, tol_it = dcase(k)
    b, n = p1.shape[:2]
    t1, t2 = dev(p1, cuda), dev(p2, cuda)
    tw = None if w is None else dev(w, cuda)
    H = find_homography_dlt(t1, t2, tw)
    Hit = find_homography_dlt_iterated(t1, t2, torch.ones(b, n, dtype=torch.float64, device=cuda) if tw is None else tw)
    assert H.dtype == torch.float64 and tuple(H.shape) == (b, 3, 3) and H.is_cuda and Hit.dtype == torch.float64
    for i in range(b):
        e, ei = VC.corner_err(H[i].cpu().numpy(), Hr[i]), VC.corner_err(Hit[i].cpu().numpy(), Hi[i])
        print("dlt case", k, i, "corner err px", e, "tol", tol, "iterated", ei, "tol", tol_it)
        assert e <= tol and ei <= tol_it
    # float32 in: float64 arithmetic on the same values, rounded once
    f1, f2 = t1.float(), t2.float()
    fw = None if tw is None else tw.float()
    H32 = find_homography_dlt(f1, f2, fw)
    H64 = find_homography_dlt(f1.double(), f2.double(), None if fw is None else fw.double())
    assert H32.dtype == torch.float32 and torch.equal(H32, H64.float())
    wi = torch.ones(b, n, device=cuda) if fw is None else fw
    assert torch.equal(find_homography_dlt_iterated(f1, f2, wi), find_homography_dlt_iterated(f1.double(), f2.double(), wi.double()).float())


# ---------------------------------------------------------------- verify_pairs against the oracle
@pytest.mark.parametrize("k", range(len(VC.VERIFY_CASES)))
def test_verify_pairs_vs_oracle(cuda, k):
    case, inputs, want, tol = vcase(k)
    check_outputs(run_ragged(cuda, inputs, case), want, tol, case["name"])


def test_dense_equals_ragged(cuda):
    """a dense [P, N, 2] batch == the same pairs through the ragged form, bit for bit"""
    from cirtorch.search import verify_pairs
    case = VC.VERIFY_CASES[4]
    parts = [VC.planted_pair(70, 64, 40, 0.5, 0.5, 900 + s) for s in range(3)]
    k1, k2, m = (np.stack([q[i] for q in parts]) for i in range(3))
    dense = verify_pairs(dev(k1, cuda), dev(k2, cuda), dev(m, cuda), th=VC.TH, iters=case["iters"], seed=5)
    off1, off2 = np.arange(4, dtype=np.int64) * 70, np.arange(4, dtype=np.int64) * 64
    rag = verify_pairs(dev(k1.reshape(-1, 2), cuda), dev(k2.reshape(-1, 2), cuda), dev(m.reshape(-1), cuda), th=VC.TH,
                       iters=case["iters"], seed=5, offsets1=dev(off1, cuda), offsets2=dev(off2, cuda), max_n1=70)
    assert tuple(dense[2].shape) == (3, 70) and tuple(rag[2].shape) == (210,)
    assert torch.equal(dense[0], rag[0]) and torch.equal(dense[2].reshape(-1), rag[2])
    assert dense[1].cpu().numpy().tobytes() == rag[1].cpu().numpy().tobytes()
    winl, wH, wmask, _ = VC.verify_batch(k1.reshape(-1, 2), off1, k2.reshape(-1, 2), off2, m.reshape(-1), VC.TH, case["iters"], 2, 5)
    np.testing.assert_array_equal(dense[0].cpu().numpy(), winl)
    np.testing.assert_array_equal(rag[2].cpu().numpy(), wmask)
    assert winl.min() >= 18
    # one pair, [N, 2] keypoints
    one = verify_pairs(dev(k1[1], cuda), dev(k2[1], cuda), dev(m[1], cuda), th=VC.TH, iters=case["iters"], seed=5)
    assert tuple(one[0].shape) == (1,) and tuple(one[1].shape) == (1, 3, 3) and tuple(one[2].shape) == (70,)


def test_pair_alone_equals_pair_in_batch_and_reruns(cuda):
    """the bits of inliers, mask and H of a pair alone (P = 1) == those of the same pair as pair 0
    of a batch of 45 (the hash takes the pair's index, so the pair keeps index 0), and of the
    four pairs of the ragged case in front of 40 more; two runs of one call are bit-identical"""
    bits = lambda t: t.cpu().numpy().tobytes()  # noqa: E731
    case, inputs, want, tol = vcase(9)        # ragged P = 4, iters 300, refine 2
    kp1, off1, kp2, off2, match = inputs
    a = run_ragged(cuda, inputs, case)
    b = run_ragged(cuda, inputs, case)
    assert all(bits(x) == bits(y) for x, y in zip(a, b))
    _, one, _, _ = vcase(4)                   # P = 1, the same iters and refine
    assert VC.VERIFY_CASES[4]["iters"] == case["iters"] and VC.VERIFY_CASES[4]["refine"] == case["refine"]
    alone = run_ragged(cuda, one, case)
    assert alone[0].item() >= 18
    # a batch of 45: the single pair, the ragged case's four, 40 copies of another pair
    extra = VC.planted_pair(50, 50, 30, 0.5, 0.5, 77)
    lens1 = [len(one[0])] + list(np.diff(off1)) + [50] * 40
    lens2 = [len(one[2])] + list(np.diff(off2)) + [50] * 40
    big = (np.concatenate([one[0], kp1] + [extra[0]] * 40), np.cumsum([0] + lens1).astype(np.int64),
           np.concatenate([one[2], kp2] + [extra[1]] * 40), np.cumsum([0] + lens2).astype(np.int64),
           np.concatenate([one[4], match] + [extra[2]] * 40))
    d = run_ragged(cuda, big, case)
    n = len(one[0])
    assert bits(d[0][:1]) == bits(alone[0]) and bits(d[1][:1]) == bits(alone[1]) and bits(d[2][:n]) == bits(alone[2])
    # pairs 1..4 of the batch are the ragged case's pairs at other indices: other samples, the same
    # verdict on the pairs whose outcome no sample can change
    assert d[0][1:3].tolist() == [0, 0] and d[0][4].item() == a[0][3].item() == 50


def test_seed_changes_the_winner(cuda):
    """a designed case: 20 noisy inliers among 20 outliers, refine = 0, so H is the winner's own
    4-point fit and about one hypothesis in 16 is all inliers: three seeds have three different
    winners t in the oracle, and the engine returns each seed's own count, mask and a different H"""
    case = dict(iters=300, refine=0)
    kp1, kp2, match, planted, _ = VC.planted_pair(60, 60, 40, 0.5, 0.5, 4242)
    off1, off2 = np.array([0, 60], dtype=np.int64), np.array([0, 60], dtype=np.int64)
    ts, Hs = [], []
    for seed in (1, 2, 3):
        o = VC.verify_pair(kp1, kp2, match, 0, VC.TH, 300, 0, seed)
        assert o["margin"] >= 1e-7 and o["t"] >= 0
        got = run_ragged(cuda, (kp1, off1, kp2, off2, match), case, seed=seed)
        assert got[0].item() == o["inliers"]
        np.testing.assert_array_equal(got[2].cpu().numpy(), o["mask"])
        ts.append(o["t"])
        Hs.append(got[1][0].cpu().numpy().tobytes())
    assert len(set(ts)) == 3 and len(set(Hs)) == 3, ts


def test_degenerate_inputs_give_finite_outputs(cuda):
    """every side-2 keypoint identical; exactly collinear points; a line with a float32-rounded slope"""
    from cirtorch.search import verify_pairs
    r = np.random.default_rng(8)
    n = 48
    k1 = r.uniform([0, 0], [VC.W, VC.H_IMG], (4, n, 2)).astype(np.float32)
    k2 = r.uniform([0, 0], [VC.W, VC.H_IMG], (4, n, 2)).astype(np.float32)
    k2[0] = k2[0, 0]                                       # all identical
    x = np.arange(n, dtype=np.float32) * 16
    k1[1] = np.stack([x, 2 * x + 5], 1)                    # exactly collinear, both sides
    k2[1] = np.stack([x + 3, x + 7], 1)
    k1[2] = np.stack([x, (x * np.float32(0.3737) + np.float32(11.13)).astype(np.float32)], 1)   # rounded slope
    k2[2] = k1[2] + np.float32(2.5)
    k2[3] = k1[3]                                          # control: the identity
    m = np.tile(np.arange(n, dtype=np.int64), (4, 1))
    inl, H, mask = verify_pairs(dev(k1, cuda), dev(k2, cuda), dev(m, cuda), th=3.0, iters=256, refine=2, seed=3)
    Hn, inl, mask = H.cpu().numpy(), inl.cpu().numpy(), mask.cpu().numpy()
    assert np.isfinite(Hn).all()
    assert inl[0] == 0 and inl[1] == 0 and not Hn[:2].any() and not mask[:2].any()
    assert 0 <= inl[2] <= n and mask[2].sum() == inl[2]
    assert inl[3] == n and mask[3].all() and VC.corner_err(Hn[3], np.eye(3)) < 1e-6
    want = VC.verify_batch(k1.reshape(-1, 2), np.arange(5) * n, k2.reshape(-1, 2), np.arange(5) * n, m.reshape(-1), 3.0, 256, 2, 3)
    np.testing.assert_array_equal(inl[[0, 1, 3]], want[0][[0, 1, 3]])


def test_graph_capture_replay_equals_eager(cuda):
    from cirtorch.search import verify_pairs
    from cirtorch.utils.graph import GraphedForward
    parts = [VC.planted_pair(70, 64, 40, 0.5, 0.5, 300 + s) for s in range(4)]
    k1 = [dev(np.stack([q[0] for q in parts[i:i + 2]]), cuda) for i in (0, 2)]
    k2 = [dev(np.stack([q[1] for q in parts[i:i + 2]]), cuda) for i in (0, 2)]
    m = [dev(np.stack([q[2] for q in parts[i:i + 2]]), cuda) for i in (0, 2)]
    # one input tensor per replay: keypoints of both sides and the match list (indices < 2^24: exact in float32)
    x = [torch.cat([k1[i].reshape(2, -1), k2[i].reshape(2, -1), m[i].float()], 1) for i in (0, 1)]

    def fn(t):
        a = t[:, :140].reshape(2, 70, 2).contiguous()
        b = t[:, 140:268].reshape(2, 64, 2).contiguous()
        mm = t[:, 268:].long()
        return verify_pairs(a, b, mm, th=VC.TH, iters=300, refine=2, seed=9)

    g = GraphedForward(fn, x[0])
    for t in (x[1], x[0]):
        gi, gH, gm = [o.clone() for o in g(t)]
        ei, eH, em = fn(t)
        assert torch.equal(gi, ei) and torch.equal(gm, em) and gH.cpu().numpy().tobytes() == eH.cpu().numpy().tobytes()
        assert ei.min().item() >= 18


def test_match_verify_rerank_end_to_end(cuda):
    """one query against 6 shortlisted images, 2 of them planted true views (their keypoints are
    the query's under a homography, their descriptors the query's plus noise): match_pairs(smnn)
    -> verify_pairs -> rerank_by_inliers puts the two true images first"""
    from cirtorch.search import match_pairs, rerank_by_inliers, verify_pairs
    r = np.random.default_rng(21)
    n, d, true_views = 120, 32, (2, 4)
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)  # noqa: E731
    qk = r.uniform([0, 0], [VC.W, VC.H_IMG], (n, 2)).astype(np.float32)
    qd = unit(r.standard_normal((n, d))).astype(np.float32)
    kp2 = r.uniform([0, 0], [VC.W, VC.H_IMG], (6, n, 2)).astype(np.float32)
    de2 = unit(r.standard_normal((6 * n, d))).reshape(6, n, d).astype(np.float32)
    for v in true_views:
        perm = r.permutation(n)
        img = VC.transfer(VC.true_homography(r), qk.astype(np.float64)) + 0.5 * r.standard_normal((n, 2))
        kp2[v, perm] = img.astype(np.float32)
        de2[v, perm] = unit(qd + 0.05 * r.standard_normal((n, d))).astype(np.float32)
    k1 = dev(np.tile(qk, (6, 1, 1)), cuda)
    d1 = dev(np.tile(qd, (6, 1, 1)), cuda)
    match, _ = match_pairs(d1, dev(de2, cuda), mode="smnn", th=0.9)
    inl, H, mask = verify_pairs(k1, dev(kp2, cuda), match, th=VC.TH, iters=256, refine=2, seed=0)
    shortlist = torch.tensor([[10], [11], [12], [13], [14], [15]], device=cuda)     # [k, Q = 1]
    ranked = rerank_by_inliers(shortlist, inl.view(6, 1))
    print("inliers", inl.tolist(), "ranked", ranked[:, 0].tolist())
    assert sorted(ranked[:2, 0].tolist()) == [12, 14]
    assert inl[list(true_views)].min().item() >= 60 and inl[[0, 1, 3, 5]].max().item() <= 8
    assert int(mask[2].sum()) == inl[2].item() and tuple(H.shape) == (6, 3, 3)
