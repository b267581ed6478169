"""The one-block-per-pair kernels on batches of more pairs than their 65535-block cap (tests/gridcap_cases.py):
blocks 0 .. 69 of every launch walk `for (p = blockIdx; p < npairs; p += gridDim)` a second time, from one
kind of pair to another, with the LDS they reuse.

Entries whose result does not depend on the pair's index run once on the seven distinct pairs (P = 7) and once
on P = 65605 pairs tiled from them on the device; every pair of the big batch must have the bits of its
distinct pair, and the seven must equal their float64 numpy restatement.  Which kernel's second trip each
test executes:

  test_match_pairs_and_top2_past_the_cap      k_match_top2 (s_o reused by the merge; no == 0 and row0 >= nq
                                              between ordinary pairs), k_match_final
  test_dlt_and_fundamental_fits_past_the_cap  k_fit_batch<Homography>, k_fit_batch<Fundamental> (FitLds<M>)
  test_epipolar_distances_past_the_cap        k_epi_distance
  test_triangulate_past_the_cap               k_triangulate (s_P)
  test_recover_pose_past_the_cap              k_recover_pose (PoseLds, s_cnt)
  test_essential_decompose_past_the_cap       k_essential_decompose (256 matrices per block)
  test_verify_pairs_past_the_cap              k_verify_compact (s_w), k_ransac<M> for both models (s_rec behind the
                                              barrier inside `if (m >= M::SAMPLE)`, 4 / 7: staged, unstaged and
                                              skipped pairs in every order), k_refit<M> for both models

Tolerances of the restatements are those of the modules they come from: indices, counts and masks exact (the
margins are asserted in test_host_gridcap.py), matrices and points within 100 x the difference of two float64
solvers on the same input with the module's floor."""

import time

import numpy as np
import pytest
import torch

import epipolar_cases as EC
import gridcap_cases as GC
import match_cases as MC
import pose_cases as PC
import verify_cases as VC
from test_gpu_epipolar import check_outputs as check_epipolar
from test_gpu_match import RTOL, check_fixed
from test_gpu_pose import check_pair
from test_gpu_verify import check_outputs as check_homography

pytestmark = pytest.mark.gpu


def dev(x, cuda):
    return torch.from_numpy(np.array(x)).to(cuda)


def same_bits(a, b):
    if a.dtype == torch.float64:
        a, b = a.view(torch.int64), b.view(torch.int64)
    elif a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def tile(cuda, lens, kind):
    """the ragged layout of the big batch on the device: pair p has the lens[kind[p]] rows of distinct pair kind[p]
    -> (off int64 [P + 1], src int64 [rows]: the row of the concatenated distinct pairs each row copies, pair
    int64 [rows], kind on the device)"""
    lens_t = torch.tensor(list(lens), dtype=torch.int64, device=cuda)
    kind_t = dev(kind, cuda)
    n = lens_t[kind_t]
    off = torch.zeros(len(kind) + 1, dtype=torch.int64, device=cuda)
    off[1:] = torch.cumsum(n, 0)
    pair = torch.repeat_interleave(torch.arange(len(kind), device=cuda), n)
    first = torch.cumsum(lens_t, 0) - lens_t
    src = first[kind_t[pair]] + torch.arange(pair.numel(), device=cuda) - off[pair]
    return off, src, pair, kind_t


def cat(cuda, parts, dtype):
    return dev(np.concatenate([np.asarray(q, dtype=dtype) for q in parts]), cuda)


def off7(cuda, parts):
    return dev(GC.offsets(len(q) for q in parts), cuda)


# ---------------------------------------------------------------- matching
def test_match_pairs_and_top2_past_the_cap(cuda):
    from cirtorch import _ops
    from cirtorch.search import match_pairs
    seven = GC.match_seven()
    a7, b7 = cat(cuda, [a for a, _ in seven], np.float32), cat(cuda, [b for _, b in seven], np.float32)
    oa, ob = off7(cuda, [a for a, _ in seven]), off7(cuda, [b for _, b in seven])
    mx = dict(max_n1=GC.MATCH_MAX, max_n2=GC.MATCH_MAX)
    small = {mode: match_pairs(a7, b7, mode=mode, th=GC.MATCH_TH, offsets1=oa, offsets2=ob, **mx) for mode in ("nn", "smnn")}
    small_top2 = _ops.match_top2(a7, oa, b7, ob, **mx)
    # the seven against float64 numpy
    ha, hb = oa.cpu().numpy(), ob.cpu().numpy()
    tol = (8 * GC.D + 12) * 2.0 ** -53
    for k, (a, b) in enumerate(seven):
        ra, rb = slice(ha[k], ha[k + 1]), slice(hb[k], hb[k + 1])
        exp = MC.rules(a, b, GC.MATCH_TH)
        for mode in ("nn", "smnn"):
            check_fixed(small[mode][0][ra], small[mode][1][ra], *exp[mode], what="pair %d %s" % (k, mode))
        dm2 = MC.dist2(a, b)
        d12, i12, d21, i21 = (t.cpu().numpy() for t in small_top2)
        for got_d, got_i, m in ((d12[ra], i12[ra], dm2), (d21[rb], i21[rb], dm2.T)):
            ed, ei = MC.top2(m)
            np.testing.assert_array_equal(got_i, ei)
            fin = np.isfinite(ed)
            assert np.array_equal(np.isinf(got_d), ~fin) and (got_d >= 0).all()
            np.testing.assert_allclose(got_d[fin], ed[fin], rtol=0, atol=tol)
    assert RTOL == 2e-6
    # the big batch
    kind = GC.kinds()
    offa, srca, _, _ = tile(cuda, [len(a) for a, _ in seven], kind)
    offb, srcb, _, _ = tile(cuda, [len(b) for _, b in seven], kind)
    A, B = a7[srca].contiguous(), b7[srcb].contiguous()
    for mode in ("nn", "smnn"):
        match, dist = match_pairs(A, B, mode=mode, th=GC.MATCH_TH, offsets1=offa, offsets2=offb, **mx)
        assert torch.equal(match, small[mode][0][srca]) and same_bits(dist, small[mode][1][srca]), mode
    big = _ops.match_top2(A, offa, B, offb, **mx)
    for got, want, src in zip(big, small_top2, (srca, srca, srcb, srcb)):
        assert same_bits(got, want[src])
    assert (small["nn"][0] >= 0).sum().item() > 80 and (small["smnn"][0] >= 0).sum().item() > 5


# ---------------------------------------------------------------- batched fits
def fits(cuda, sets, entry, restate, tolfn, err, least):
    p1, p2, w = (cat(cuda, [q[i] for q in sets], np.float64).reshape(-1, 2) if i < 2 else cat(cuda, [q[i] for q in sets], np.float64)
                 for i in range(3))
    small = entry(p1, p2, w, off7(cuda, [q[0] for q in sets]))
    got = small.cpu().numpy()
    assert np.isfinite(got).all()
    for k, (a, b, ww) in enumerate(sets):
        if len(a) < least:
            assert not got[k].any(), k
            continue
        e, tol = err(got[k], restate(a, b, ww)), tolfn(a, b, ww)
        print(entry.__name__, "set", k, "n", len(a), "err", e, "tol", tol)
        assert e <= tol, (k, e, tol)
    off, src, _, kind_t = tile(cuda, [len(q[0]) for q in sets], GC.kinds())
    big = entry(p1[src].contiguous(), p2[src].contiguous(), w[src].contiguous(), off)
    assert tuple(big.shape) == (GC.P, 3, 3) and same_bits(big, small[kind_t])


def test_dlt_and_fundamental_fits_past_the_cap(cuda):
    from cirtorch import _ops
    fits(cuda, GC.dlt_seven(), _ops.homography_dlt, VC.dlt, GC.dlt_tol, VC.corner_err, 4)
    fits(cuda, GC.fund_seven(), _ops.fundamental_dlt, EC.fundamental, GC.fund_tol, EC.f_err, 8)


def test_epipolar_distances_past_the_cap(cuda):
    from cirtorch import _ops
    sets = GC.dist_seven()
    p1, p2 = (cat(cuda, [q[i] for q in sets], np.float64).reshape(-1, 2) for i in range(2))
    F7 = dev(np.stack([q[2] for q in sets]), cuda)
    o7 = off7(cuda, [q[0] for q in sets])
    ho = o7.cpu().numpy()
    off, src, _, kind_t = tile(cuda, [len(q[0]) for q in sets], GC.kinds())
    P1, P2, Fb = p1[src].contiguous(), p2[src].contiguous(), F7[kind_t].contiguous()
    for kind, squared in GC.DIST_KINDS:
        small = _ops.epipolar_distance(p1, p2, F7, o7, kind, squared)
        got = small.cpu().numpy()
        for k, (a, b, F) in enumerate(sets):
            if len(a):
                want, g = EC.distance(a, b, F, kind, squared), got[ho[k]:ho[k + 1]]
                e, tol = np.abs(g - want).max() / np.abs(want).max(), GC.dist_tol(a, b, F, kind, squared)
                print(kind, squared, "set", k, "rel err", e, "tol", tol)
                assert e <= tol, (kind, squared, k, e, tol)
        assert same_bits(_ops.epipolar_distance(P1, P2, Fb, off, kind, squared), small[src]), (kind, squared)


def test_triangulate_past_the_cap(cuda):
    from cirtorch import _ops
    sets = GC.tri_seven()
    p1, p2 = (cat(cuda, [t["rec"][:, c] for t in sets], np.float64).reshape(-1, 2) for c in (slice(0, 2), slice(2, 4)))
    P1, P2 = dev(np.stack([t["P1"] for t in sets]), cuda), dev(np.stack([t["P2"] for t in sets]), cuda)
    o7 = off7(cuda, [t["rec"] for t in sets])
    ho = o7.cpu().numpy()
    small = _ops.triangulate_points(p1, p2, P1, P2, o7)
    got = small.cpu().numpy()
    for k, t in enumerate(sets):
        if len(t["rec"]):
            e, tol = np.abs(got[ho[k]:ho[k + 1]] - PC.triangulate(t["P1"], t["P2"], t["rec"])[0]).max() / t["scale"], GC.tri_tol(t)
            print("triangulate set", k, "n", len(t["rec"]), "err", e, "tol", tol)
            assert e <= tol, (k, e, tol)
    off, src, _, kind_t = tile(cuda, [len(t["rec"]) for t in sets], GC.kinds())
    big = _ops.triangulate_points(p1[src].contiguous(), p2[src].contiguous(), P1[kind_t].contiguous(), P2[kind_t].contiguous(), off)
    assert same_bits(big, small[src])


# ---------------------------------------------------------------- pose
def test_recover_pose_past_the_cap(cuda):
    from cirtorch import _ops
    seven = GC.pose_seven()
    sc = [c["scene"] for c in seven]
    kp1, kp2 = cat(cuda, [s["kp1"] for s in sc], np.float32).reshape(-1, 2), cat(cuda, [s["kp2"] for s in sc], np.float32).reshape(-1, 2)
    match, mask = cat(cuda, [s["match"] for s in sc], np.int64), cat(cuda, [c["mask"] for c in seven], bool)
    F7, K1, K2 = (dev(np.stack([c[q] for c in seven]), cuda) for q in ("F", "K1", "K2"))
    o1, o2 = off7(cuda, [s["kp1"] for s in sc]), off7(cuda, [s["kp2"] for s in sc])
    small = _ops.recover_pose(kp1, o1, kp2, o2, match, mask, F7, K1, K2)
    R, t, E, front, X, fmask = (o.cpu().numpy() for o in small)
    h1 = o1.cpu().numpy()
    for k, c in enumerate(seven):
        a, w = slice(h1[k], h1[k + 1]), c["want"]
        check_pair((R[k], t[k], E[k], front[k], X[a], fmask[a]), (w["R"], w["t"], w["points3d"], w["front"], w["front_mask"]),
                   c["tol"], c["scale"], c["name"])
    assert front.tolist()[:3] == [0, 0, 0] and front[3:].min() >= 6
    kind = GC.kinds()
    off1, src1, _, kind_t = tile(cuda, [len(s["kp1"]) for s in sc], kind)
    off2, src2, _, _ = tile(cuda, [len(s["kp2"]) for s in sc], kind)
    big = _ops.recover_pose(kp1[src1].contiguous(), off1, kp2[src2].contiguous(), off2, match[src1].contiguous(), mask[src1].contiguous(),
                            F7[kind_t].contiguous(), K1[kind_t].contiguous(), K2[kind_t].contiguous())
    for i in range(4):          # R, t, E, front: per pair
        assert same_bits(big[i], small[i][kind_t]), i
    for i in (4, 5):            # points3d, front_mask: per row
        assert same_bits(big[i], small[i][src1]), i


def test_essential_decompose_past_the_cap(cuda):
    """n = 65535 x 256 + 1000 matrices tiled from 11: blocks 0 .. 3 stride to a second matrix per thread"""
    from cirtorch import _ops
    E11 = GC.essential_eleven()
    small = _ops.essential_decompose(dev(E11, cuda))
    got = [o.cpu().numpy() for o in small]
    for i in range(GC.DEC_DISTINCT):
        want = PC.decompose(E11[i])
        if want is None:
            assert not any(g[i].any() for g in got), i
            continue
        e, tol = GC.decompose_diff((got[0][i], got[1][i], got[2][i]), want[:3]), GC.decompose_tol(E11[i])
        print("decompose matrix", i, "err", e, "tol", tol)
        assert e <= tol, (i, e, tol)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    src = torch.arange(GC.DEC_N, device=cuda) % GC.DEC_DISTINCT
    big = _ops.essential_decompose(dev(E11, cuda)[src].contiguous())
    for o, s in zip(big, small):
        assert same_bits(o, s[src])
    torch.cuda.synchronize()
    print("essential_decompose on %d matrices: %.2f s wall with the comparison" % (GC.DEC_N, time.perf_counter() - t0))


# ---------------------------------------------------------------- the RANSAC verifiers
@pytest.mark.parametrize("model", ["homography", "fundamental"])
def test_verify_pairs_past_the_cap(cuda, model):
    from cirtorch.search import verify_pairs
    mod = VC if model == "homography" else EC
    eight, kind, least = GC.verify_eight(model), GC.kinds(GC.SPECIAL), GC.MINIMAL[model]
    lens2 = [len(q[1]) for q in eight]
    off1, src1, pair1, kind_t = tile(cuda, [len(q[0]) for q in eight], kind)
    off2, src2, _, _ = tile(cuda, lens2, kind)
    kp1 = cat(cuda, [q[0] for q in eight], np.float32).reshape(-1, 2)[src1].contiguous()
    kp2 = cat(cuda, [q[1] for q in eight], np.float32).reshape(-1, 2)[src2].contiguous()
    match = cat(cuda, [q[2] for q in eight], np.int64)[src1].contiguous()

    def run():
        return verify_pairs(kp1, kp2, match, th=mod.TH, iters=GC.ITERS, refine=GC.REFINE, seed=mod.RUN_SEED, offsets1=off1,
                            offsets2=off2, model=model)

    inl, M, mask = run()
    again = run()
    assert torch.equal(inl, again[0]) and same_bits(M, again[1]) and torch.equal(mask, again[2])
    assert tuple(inl.shape) == (GC.P,) and tuple(M.shape) == (GC.P, 3, 3) and tuple(mask.shape) == tuple(match.shape)
    # every pair, on the device
    zeros = torch.zeros(GC.P, dtype=torch.int64, device=cuda)
    n2 = torch.tensor(lens2, dtype=torch.int64, device=cuda)[kind_t]
    m_p = zeros.clone().index_add_(0, pair1, ((match >= 0) & (match < n2[pair1])).long())
    assert torch.equal(zeros.clone().index_add_(0, pair1, mask.long()), inl.long())
    assert bool((inl.long() <= m_p).all()) and bool(torch.isfinite(M).all())
    below = m_p < least
    assert torch.equal(inl == 0, below) and torch.equal((M.reshape(GC.P, 9) == 0).all(1), below)
    assert below.sum().item() > 3 * (GC.P // 7) - 8 and (m_p == VC.STAGE + 1).sum().item() == len(GC.SPECIAL)
    # the compared pairs against the oracle at their own p
    orc = GC.verify_oracle(model)
    idx = sorted(orc)
    h1 = off1.cpu().numpy()
    it = dev(np.array(idx), cuda)
    got = (inl[it], M[it], torch.cat([mask[h1[p]:h1[p + 1]] for p in idx]))
    key = "H" if model == "homography" else "F"
    want = (np.array([orc[p]["info"]["inliers"] for p in idx], dtype=np.int32), np.stack([orc[p]["info"][key] for p in idx]),
            np.concatenate([orc[p]["info"]["mask"] for p in idx]))
    tol = np.array([orc[p]["tol"] for p in idx])
    (check_homography if model == "homography" else check_epipolar)(got, want, tol, "%s past the cap" % model)
