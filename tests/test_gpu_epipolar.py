"""Epipolar verification on the GPU (rr_verify_pairs_epipolar / rr_fundamental_dlt / rr_epipolar_distance,
cirtorch.search.verify_pairs(model="fundamental"), cirtorch.geometry.epipolar) against the matrices
and distances the reference's fundamental.py / metrics.py produced in float64
(tests/golden/epipolar.npz) and the float64 numpy restatement of tests/epipolar_cases.py.

Tolerances.  Inlier counts and masks are exact: the fixture's generator asserts that no Sampson
distance of any root of any hypothesis or refit lies within 1e-7 px of th, and that two independent
null-space solvers agree on the winner and on every count near it.  F matrices are compared after
scaling to unit Frobenius norm and aligning the sign, by the largest absolute entry difference,
against the fixture's per-case tolerance: 100 x the difference between two other solvers on the same
points, floor 1e-12.  Distances: relative to the set's largest, tolerance derived the same way
(make_golden_epipolar.py)."""

import functools

import numpy as np
import pytest
import torch

import epipolar_cases as EC
import verify_cases as VC
from conftest import golden

pytestmark = pytest.mark.gpu
KINDS = (("sam", "sampson", True), ("sam_rt", "sampson", False), ("sym", "symmetrical", True), ("sym_rt", "symmetrical", False))


def dev(x, cuda):
    return torch.from_numpy(np.array(x)).to(cuda)   # a copy: the cached cases are read-only


def bits(t):
    return t.cpu().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def ecase(k):
    """case k: inputs, the oracle's outputs (computed once, never modified) and the tolerances"""
    g = golden("epipolar.npz")
    case = EC.EPI_CASES[k]
    kp1, off1, kp2, off2, match, planted = EC.build_case(case, int(g["e_seeds"][k]))
    np.testing.assert_allclose(EC.checksum(kp1, kp2, match), g["e_chk"][k], rtol=0, atol=1e-6)
    inl, Fs, mask, infos = EC.epipolar_batch(kp1, off1, kp2, off2, match, EC.TH, case["iters"], case["refine"], EC.RUN_SEED)
    np.testing.assert_array_equal(inl, g["e%d_inl" % k])
    for a in (kp1, off1, kp2, off2, match, planted, inl, Fs, mask):
        a.setflags(write=False)
    return case, (kp1, off1, kp2, off2, match), (inl, Fs, mask, infos), g["e%d_tol" % k], planted


def case_named(name):
    return ecase([c["name"] for c in EC.EPI_CASES].index(name))


def run_ragged(cuda, inputs, case, seed=EC.RUN_SEED, **kw):
    from cirtorch.search import verify_pairs
    kp1, off1, kp2, off2, match = inputs
    return verify_pairs(dev(kp1, cuda), dev(kp2, cuda), dev(match, cuda), th=EC.TH, iters=case["iters"], refine=case["refine"],
                        seed=seed, offsets1=dev(off1, cuda), offsets2=dev(off2, cuda), model="fundamental", **kw)


def check_outputs(got, want, tol, what=""):
    inl, F, mask = got
    winl, wF, wmask = want[:3]
    assert inl.dtype == torch.int32 and F.dtype == torch.float64 and mask.dtype == torch.bool
    assert tuple(F.shape) == (len(winl), 3, 3)
    np.testing.assert_array_equal(inl.cpu().numpy(), winl, err_msg=what)
    np.testing.assert_array_equal(mask.cpu().numpy(), wmask, err_msg=what)
    Fn = F.cpu().numpy()
    assert np.isfinite(Fn).all()
    for p in range(len(winl)):
        if winl[p] == 0:
            assert not Fn[p].any(), what
        else:
            e = EC.f_err(Fn[p], wF[p])
            print(what, "pair", p, "inliers", winl[p], "F err", e, "tol", tol[p])
            assert e <= tol[p], (what, p, e, tol[p])
            # rr.h step e: unit Frobenius norm, the largest entry positive
            assert abs(np.sqrt((Fn[p] ** 2).sum()) - 1) < 1e-14 and Fn[p].reshape(-1)[np.argmax(np.abs(Fn[p]))] > 0


# ---------------------------------------------------------------- 8-point fit and distances against the reference
@pytest.mark.parametrize("k", range(len(EC.FUND_CASES)))
def test_fit_and_distances_vs_reference(cuda, k):
    from cirtorch.geometry.epipolar import find_fundamental, sampson_epipolar_distance, symmetrical_epipolar_distance
    g = golden("epipolar.npz")
    b, n, weighted = EC.FUND_CASES[k]
    p1, p2, w = EC.fund_points(b, n, weighted, int(g["fund_seeds"][k]))
    np.testing.assert_allclose(EC.checksum(p1, p2, w), g["fund_chk"][k], rtol=0, atol=1e-6)
    tol, tol_d = float(g["fund_tol"][k]), float(g["fund_tol_d"][k])
    t1, t2, tw = dev(p1, cuda), dev(p2, cuda), dev(w, cuda)
    F = find_fundamental(t1, t2, tw)
    assert F.dtype == torch.float64 and tuple(F.shape) == (b, 3, 3) and F.is_cuda
    Fr = g["fund%d_F" % k]
    for i in range(b):
        e = EC.f_err(F[i].cpu().numpy(), Fr[i])
        print("8-point case", k, i, "F err", e, "tol", tol)
        assert e <= tol
    # float32 in: float64 arithmetic on the same values, rounded once
    f1, f2, fw = t1.float(), t2.float(), tw.float()
    F32 = find_fundamental(f1, f2, fw)
    assert F32.dtype == torch.float32 and torch.equal(F32, find_fundamental(f1.double(), f2.double(), fw.double()).float())
    # distances under the reference's F
    tF = dev(Fr, cuda)
    ones = torch.ones(b, n, 1, dtype=torch.float64, device=cuda)
    for key, kind, squared in KINDS:
        fn = sampson_epipolar_distance if kind == "sampson" else symmetrical_epipolar_distance
        d = fn(t1, t2, tF, squared=squared)
        assert d.dtype == torch.float64 and tuple(d.shape) == (b, n)
        want = g["fund%d_%s" % (k, key)]
        for i in range(b):
            e = np.abs(d[i].cpu().numpy() - want[i]).max() / np.abs(want[i]).max()
            print("8-point case", k, i, key, "rel err", e, "tol", tol_d)
            assert e <= tol_d
        # homogeneous points: the same bits
        assert torch.equal(fn(torch.cat([t1, ones], 2), torch.cat([t2, ones], 2), tF, squared=squared), d)
    with pytest.raises(ValueError):
        sampson_epipolar_distance(torch.cat([t1, 2 * ones], 2), t2, tF)


# ---------------------------------------------------------------- verify_pairs(model="fundamental") against the oracle
@pytest.mark.parametrize("k", range(len(EC.EPI_CASES)))
def test_epipolar_pairs_vs_oracle(cuda, k):
    case, inputs, want, tol, _ = ecase(k)
    check_outputs(run_ragged(cuda, inputs, case), want, tol, case["name"])


def test_dense_equals_ragged(cuda):
    """a dense [P, N, 2] batch == the same pairs through the ragged form, bit for bit"""
    from cirtorch.search import verify_pairs
    parts = [EC.planted_pair(70, 64, 40, 0.6, 0.3, 900 + s) for s in range(3)]
    k1, k2, m = (np.stack([q[i] for q in parts]) for i in range(3))
    kw = dict(th=EC.TH, iters=300, seed=5, model="fundamental")
    dense = verify_pairs(dev(k1, cuda), dev(k2, cuda), dev(m, cuda), **kw)
    off1, off2 = np.arange(4, dtype=np.int64) * 70, np.arange(4, dtype=np.int64) * 64
    rag = verify_pairs(dev(k1.reshape(-1, 2), cuda), dev(k2.reshape(-1, 2), cuda), dev(m.reshape(-1), cuda),
                       offsets1=dev(off1, cuda), offsets2=dev(off2, cuda), max_n1=70, **kw)
    assert tuple(dense[2].shape) == (3, 70) and tuple(rag[2].shape) == (210,)
    assert torch.equal(dense[0], rag[0]) and torch.equal(dense[2].reshape(-1), rag[2]) and bits(dense[1]) == bits(rag[1])
    assert dense[0].min().item() >= 18 and dense[2].sum(1).tolist() == dense[0].tolist()
    one = verify_pairs(dev(k1[1], cuda), dev(k2[1], cuda), dev(m[1], cuda), **kw)   # one pair, [N, 2] keypoints
    assert tuple(one[0].shape) == (1,) and tuple(one[1].shape) == (1, 3, 3) and tuple(one[2].shape) == (70,)


def test_pair_in_another_batch_and_reruns(cuda):
    """a pair keeps its bits (inliers, mask, F) when the batch around it changes: as pair 1 of two
    pairs, and as pair 1 of 44 at another row offset (the hash takes the pair's index p, so p is
    held equal); two runs of one call are bit-identical"""
    case, inputs, want, tol, _ = case_named("m40")
    kp1, off1, kp2, off2, match = inputs
    n1, n2 = len(kp1), len(kp2)
    fa = EC.planted_pair(30, 28, 20, 0.6, 0.3, 77)
    fb = EC.planted_pair(55, 50, 35, 0.6, 0.3, 78)

    def batch(front, extra):
        parts = [front, (kp1, kp2, match)] + [fa] * extra
        o1 = np.cumsum([0] + [len(q[0]) for q in parts]).astype(np.int64)
        o2 = np.cumsum([0] + [len(q[1]) for q in parts]).astype(np.int64)
        return (np.concatenate([q[0] for q in parts]), o1, np.concatenate([q[1] for q in parts]), o2,
                np.concatenate([q[2] for q in parts])), int(o1[1])

    small, s0 = batch(fa, 0)
    big, b0 = batch(fb, 42)
    a = run_ragged(cuda, small, case)
    a2 = run_ragged(cuda, small, case)
    assert all(bits(x) == bits(y) for x, y in zip(a, a2))
    d = run_ragged(cuda, big, case)
    assert s0 != b0 and a[0][1].item() >= 18
    assert bits(a[0][1:2]) == bits(d[0][1:2]) and bits(a[1][1:2]) == bits(d[1][1:2])
    assert bits(a[2][s0:s0 + n1]) == bits(d[2][b0:b0 + n1])
    # the oracle at p = 1
    o = EC.epipolar_pair(kp1, kp2, match, 1, EC.TH, case["iters"], case["refine"], EC.RUN_SEED)
    assert o["margin"] >= 1e-7 and a[0][1].item() == o["inliers"]
    np.testing.assert_array_equal(a[2][s0:s0 + n1].cpu().numpy(), o["mask"])


def test_two_runs_are_bit_identical(cuda):
    case, inputs, _, _, _ = case_named("ragged4")
    a, b = run_ragged(cuda, inputs, case), run_ragged(cuda, inputs, case)
    assert all(bits(x) == bits(y) for x, y in zip(a, b))
    case, inputs, _, _, _ = case_named("m1025")
    a, b = run_ragged(cuda, inputs, case), run_ragged(cuda, inputs, case)
    assert all(bits(x) == bits(y) for x, y in zip(a, b))


def test_seed_changes_the_winner(cuda):
    """the all-outlier case: nothing but the samples decides, so another seed has another winner t
    in the oracle, and the engine returns each seed's own count, mask and F"""
    case, inputs, want, tol, _ = case_named("outliers")
    kp1, off1, kp2, off2, match = inputs
    ts, Fs = [want[3][0]["t"]], [bits(run_ragged(cuda, inputs, case)[1])]
    for seed in (1, 2):
        o = EC.epipolar_pair(kp1, kp2, match, 0, EC.TH, case["iters"], case["refine"], seed)
        got = run_ragged(cuda, inputs, case, seed=seed)
        print("seed", seed, "winner", o["t"], o["root"], "inliers", o["inliers"], "margin", o["margin"])
        assert o["margin"] >= 1e-7 and got[0].item() == o["inliers"]
        np.testing.assert_array_equal(got[2].cpu().numpy(), o["mask"])
        ts.append(o["t"])
        Fs.append(bits(got[1]))
    assert len(set(ts)) == 3 and len(set(Fs)) == 3, ts


def test_noise_free_pair(cuda):
    """the noise-free pair of the ragged case (exact in float32): every planted match is an inlier and
    every planted correspondence has Sampson distance below 1e-6 px under the returned F"""
    case, inputs, want, tol, planted = case_named("ragged4")
    kp1, off1, kp2, off2, match = inputs
    inl, F, mask = run_ragged(cuda, inputs, case)
    a, b = slice(off1[3], off1[4]), slice(off2[3], off2[4])
    assert planted[a].sum() == 50 and inl[3].item() == 50
    assert mask.cpu().numpy()[a][planted[a]].all()
    rows = np.nonzero(planted[a])[0]
    rec = np.concatenate([kp1[a][rows], kp2[b][match[a][rows]]], 1).astype(np.float64)
    d = EC.sampson(F[3].cpu().numpy(), rec)[1]
    print("noise-free pair: largest Sampson distance px", d.max())
    assert d.max() < 1e-6
    # the same through the package's distance, on the device
    from cirtorch.geometry.epipolar import sampson_epipolar_distance
    dd = sampson_epipolar_distance(dev(rec[None, :, :2], cuda), dev(rec[None, :, 2:], cuda), F[3:4], squared=True)
    assert dd.max().item() < 1e-12


def test_graph_capture_replay_equals_eager(cuda):
    """one stream, no parallel branches: the three kernels of the call in a torch.cuda.graph"""
    from cirtorch.search import verify_pairs
    from cirtorch.utils.graph import GraphedForward
    parts = [EC.planted_pair(70, 64, 40, 0.6, 0.3, 300 + s) for s in range(4)]
    k1 = [dev(np.stack([q[0] for q in parts[i:i + 2]]), cuda) for i in (0, 2)]
    k2 = [dev(np.stack([q[1] for q in parts[i:i + 2]]), cuda) for i in (0, 2)]
    m = [dev(np.stack([q[2] for q in parts[i:i + 2]]), cuda) for i in (0, 2)]
    # one input tensor per replay: keypoints of both sides and the match list (indices < 2^24: exact in float32)
    x = [torch.cat([k1[i].reshape(2, -1), k2[i].reshape(2, -1), m[i].float()], 1) for i in (0, 1)]

    def fn(t):
        a = t[:, :140].reshape(2, 70, 2).contiguous()
        b = t[:, 140:268].reshape(2, 64, 2).contiguous()
        mm = t[:, 268:].long()
        return verify_pairs(a, b, mm, th=EC.TH, iters=300, refine=2, seed=9, model="fundamental")

    g = GraphedForward(fn, x[0])
    for t in (x[1], x[0]):
        gi, gF, gm = [o.clone() for o in g(t)]
        ei, eF, em = fn(t)
        assert torch.equal(gi, ei) and torch.equal(gm, em) and bits(gF) == bits(eF)
        assert ei.min().item() >= 18


def test_default_model_is_the_homography_path(cuda):
    """verify_pairs without `model`, and with model="homography", equal the verify.npz fixture on one
    of its cases (read-only use of tests/verify_cases.py)"""
    from cirtorch.search import verify_pairs
    g = golden("verify.npz")
    k = 4
    case = VC.VERIFY_CASES[k]
    kp1, off1, kp2, off2, match, _ = VC.build_case(case, int(g["v_seeds"][k]))
    kw = dict(th=VC.TH, iters=case["iters"], refine=case["refine"], seed=VC.RUN_SEED, offsets1=dev(off1, cuda), offsets2=dev(off2, cuda))
    a = verify_pairs(dev(kp1, cuda), dev(kp2, cuda), dev(match, cuda), **kw)
    b = verify_pairs(dev(kp1, cuda), dev(kp2, cuda), dev(match, cuda), model="homography", **kw)
    assert all(bits(x) == bits(y) for x, y in zip(a, b))
    np.testing.assert_array_equal(a[0].cpu().numpy(), g["v%d_inl" % k])
    np.testing.assert_array_equal(a[2].cpu().numpy(), g["v%d_mask" % k])
    assert VC.corner_err(a[1][0].cpu().numpy(), g["v%d_H" % k][0]) <= g["v%d_tol" % k][0]
