"""The engine's own solvers on hard geometry (tests/hard_geometry_cases.py), each alone and many pairs per call.

A pair with exactly the minimal number of matches, iters = 1 and refine = 0 returns the minimal solver's
own answer, so verify_pairs is f_from7 / h_from4 on the pair's records in hash order: scenes with
rotations up to 0.6 rad per axis, forward motion with the epipole in the image, a baseline of 0.01 and
three of four points nearly on a line.  rr_essential_decompose and rr_triangulate_points are run on
rotations by 0 .. pi, scales 1e-6 .. 1e6, near-essential matrices, focal lengths up to 5000 and
depth over baseline up to 5e5.

Bounds.  Seven-point: th = 1e-6 px where the float64 oracle fits every tuple within 4.2e-10 px
(test_host_hard_geometry.py asserts it on the same tuples); F against the oracle's Gauss-Jordan route within
100 x the spread of the oracle's own float64 routes to that root, floor 1e-12: the rule of test_gpu_epipolar.py
(100 x the difference of two solvers) with more routes, because the two null-space routines share one evaluation
of the cubic and agree to 1e-14 on tuples where the closed form itself is 4e-10 off its extended-precision value
(hard_geometry_cases.fund_spread).  Four-point: th = 1e-6 px where the oracle's solve fits every kept tuple
within 1e-6 / 16 px, the gate's determinants a factor 4 clear of RR_VERIFY_DET_EPS; tuples whose near-collinear
three are on side 2 at th = 1 px, where the oracle reaches them.  Decomposition: 16 x the worst error of numpy's SVD route on the same
matrices (hard_geometry_cases.ORACLE_WORST), floor 1e-12.  Triangulation: the residual |A h| against
sigma_min(A) from np.linalg.svd, and X at 1e-9 of |X| up to depth over baseline 50."""

import numpy as np
import pytest
import torch

import epipolar_cases as EC
import hard_geometry_cases as HG
import verify_cases as VC

pytestmark = pytest.mark.gpu


def dev(x, cuda):
    return torch.from_numpy(np.array(x)).to(cuda)


def run_minimal(cuda, tuples, model, th=HG.TH_MIN):
    from cirtorch.search import verify_pairs
    kp1, off1, kp2, off2, match = HG.ragged(tuples)
    inl, M, mask = verify_pairs(dev(kp1, cuda), dev(kp2, cuda), dev(match, cuda), th=th, iters=1, refine=0, seed=HG.RUN_SEED,
                                offsets1=dev(off1, cuda), offsets2=dev(off2, cuda), model=model)
    m = len(tuples[0]["rec"])
    return inl.cpu().numpy(), M.cpu().numpy(), mask.cpu().numpy().reshape(len(tuples), m)


def test_seven_point_solver_alone(cuda):
    """f_from7 on 800 seven-tuples of four kinds of scene: all seven records within 1e-6 px of the returned F,
    det F = 0, and F the root the oracle's winner rule picks"""
    tuples, _ = HG.fund_tuples()
    inl, F, mask = run_minimal(cuda, tuples, "fundamental")
    assert np.isfinite(F).all()
    bad, worst = [], {k: [0.0, 0.0, 0.0] for k in HG.KINDS}
    for p, t in enumerate(tuples):
        d = EC.sampson(F[p], t["rec"])[1].max() if F[p].any() else np.inf
        det = abs(np.linalg.det(F[p]))
        err = EC.f_err(F[p], t["gj"]["F"]) if F[p].any() else np.inf
        w = worst[t["kind"]]
        w[0], w[1], w[2] = max(w[0], d), max(w[1], det), max(w[2], err / t["tol"])
        ok = inl[p] == 7 and mask[p].all() and d <= HG.TH_MIN and det <= 1e-12 and err <= t["tol"] \
            and abs(np.sqrt((F[p] ** 2).sum()) - 1) < 1e-14
        if not ok:
            bad.append((p, t["kind"], int(inl[p]), t["nroots"], t["gj"]["root"], d, det, err, t["tol"]))
    for k in HG.KINDS:
        print("seven-point %-8s worst Sampson px %.3g, |det F| %.3g, F err / tol %.3g" % ((k,) + tuple(worst[k])))
    assert not bad, "pair, kind, inliers, roots, oracle root, Sampson px, |det|, F err, tol: %s" % (bad[:10],)


def test_four_point_solver_alone(cuda):
    """h_from4 on four-tuples of planted homographies, planes under the four kinds of motion, and three of four
    points within 1e-3 px of a line on both sides of the determinant gate"""
    tuples, _ = HG.homog_tuples()
    inl, H, mask = run_minimal(cuda, tuples, "homography")
    assert np.isfinite(H).all()
    bad, worst = [], {k: 0.0 for k in HG.H_KINDS}
    for p, t in enumerate(tuples):
        if t["accept"]:
            ok_w, res = VC.residuals(H[p], t["rec"]) if H[p].any() else (np.zeros(4, dtype=bool), np.full(4, np.inf))
            worst[t["kind"]] = max(worst[t["kind"]], res.max())
            ok = inl[p] == 4 and mask[p].all() and ok_w.all() and res.max() <= HG.TH_MIN and H[p, 2, 2] == 1.0
            if not ok:
                bad.append((p, t["kind"], "accepted", int(inl[p]), t["det"], res.max()))
        elif inl[p] != 0 or H[p].any() or mask[p].any():
            bad.append((p, t["kind"], "rejected", int(inl[p]), t["det"], None))
    for k in HG.H_KINDS:
        print("four-point %-14s worst transfer px %.3g" % (k, worst[k]))
    assert not bad, "pair, kind, oracle, inliers, smallest determinant, transfer px: %s" % (bad[:10],)


def test_four_point_gate_on_side_two(cuda):
    """three of the four side-2 points within 1e-3 px of a line, their determinant above the gate: the sample is
    not rejected, and H maps all four within 1 px (the oracle: within 1 / 16 px)"""
    tuples, _ = HG.gate_tuples()
    inl, H, mask = run_minimal(cuda, tuples, "homography", HG.TH_GATE)
    assert np.isfinite(H).all()
    bad, worst = [], 0.0
    for p, t in enumerate(tuples):
        ok_w, res = VC.residuals(H[p], t["rec"]) if H[p].any() else (np.zeros(4, dtype=bool), np.full(4, np.inf))
        worst = max(worst, res.max())
        if not (inl[p] == 4 and mask[p].all() and ok_w.all() and res.max() <= HG.TH_GATE):
            bad.append((p, int(inl[p]), t["det"], res.max()))
    print("four-point gate on side 2: worst transfer px %.3g" % worst)
    assert not bad, "pair, inliers, smallest determinant, transfer px: %s" % (bad[:10],)


def test_essential_decompose_hard_cases(cuda):
    """rotations by 0, 1e-8, 1e-3, 1, pi - 1e-3 and pi, t along the axes, the rotation axis and random, scales
    1e-6 .. 1e6, and K'^T F K' with two unequal singular values: R1, R2 rotations, t a unit null vector of E^T,
    the true motion among the candidates, each within 16 x what numpy's SVD route reaches"""
    from cirtorch import _ops
    from cirtorch.geometry.epipolar import decompose_essential_matrix
    cases = HG.essential_cases()
    E = dev(np.stack([c["E"] for c in cases]), cuda)
    R1, R2, t = (o.cpu().numpy() for o in _ops.essential_decompose(E))
    assert np.isfinite(R1).all() and np.isfinite(R2).all() and np.isfinite(t).all()
    worst = HG.worst_errors(list(zip(R1, R2, t)))
    bad = []
    for group, rec in HG.ORACLE_WORST.items():
        for q in rec:
            print("decompose %-5s %-7s engine %.3g oracle %.3g bound %.3g" % (group, q, worst[group][q], rec[q], HG.engine_bound(group, q)))
    for i, c in enumerate(cases):
        for q, v in HG.decompose_errors(R1[i], R2[i], t[i], c).items():
            if not v <= HG.engine_bound(c["group"], q):
                bad.append((i, c["what"], q, float(v), HG.engine_bound(c["group"], q)))
    assert not bad, bad[:10]
    # the reference-named function is the same entry
    p1, p2, pt = decompose_essential_matrix(E)
    assert torch.equal(p1.cpu(), torch.from_numpy(R1)) and torch.equal(p2.cpu(), torch.from_numpy(R2)) and tuple(pt.shape) == (len(cases), 3, 1)
    # what rr.h refuses: zeros
    Z = _ops.essential_decompose(dev(HG.refused_essentials(), cuda))
    for o in Z:
        assert not o.cpu().numpy().any()


def test_triangulate_low_parallax_and_long_focal(cuda):
    """focal lengths 500 / 900 / 5000, image coordinates up to 4000, depth over baseline 5 .. 5e5, sets of 1, 255,
    256 and 257 points: the returned point is the smallest singular vector of the 4 x 4 (the one-sided Jacobi
    converged), and equals the oracle's X where the parallax conditions it"""
    from cirtorch import _ops
    sets = HG.tri_sets()
    off = np.cumsum([0] + [len(s["rec"]) for s in sets]).astype(np.int64)
    rec = np.concatenate([s["rec"] for s in sets])
    X = _ops.triangulate_points(dev(rec[:, :2], cuda), dev(rec[:, 2:], cuda), dev(np.stack([s["P1"] for s in sets]), cuda),
                                dev(np.stack([s["P2"] for s in sets]), cuda), dev(off, cuda)).cpu().numpy()
    assert np.isfinite(X).all()
    bad, table = [], {}
    for k, s in enumerate(sets):
        Xs = X[off[k]:off[k + 1]]
        res, smin, nrm = HG.tri_residuals(s, Xs)
        ok = HG.tri_residual_ok(res, smin, nrm)
        ex = np.abs(Xs - s["X"]).max(1) / np.linalg.norm(s["X"], axis=1)
        row = table.setdefault((s["f"], s["ratio"]), [0.0, 0.0])
        row[0], row[1] = max(row[0], ((res - 1e-12 * nrm) / smin).max()), max(row[1], ex.max())
        if not ok.all():
            bad.append((s["f"], s["ratio"], len(Xs), "residual", float((res / smin).max())))
        if s["ratio"] <= HG.X_RATIO and not (ex <= HG.X_RTOL).all():
            bad.append((s["f"], s["ratio"], len(Xs), "X", float(ex.max())))
    for (f, ratio), row in table.items():
        print("triangulate f %-6g depth/baseline %-8g worst (|A h| - 1e-12 |A|) / sigma_min %.9g, |X - oracle| / |X| %.3g" % (f, ratio, row[0], row[1]))
    assert not bad, bad[:10]
