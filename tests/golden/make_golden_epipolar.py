"""Generate tests/golden/epipolar.npz (build container only, like make_golden_verify.py).

    python tests/golden/make_golden_epipolar.py

From the reference, unmodified and imported as a package: cirtorch/geometry/epipolar/fundamental.py
(find_fundamental) and metrics.py (sampson_epipolar_distance, symmetrical_epipolar_distance), run in
float64 on the point sets of tests/epipolar_cases.py, with and without weights (the reference takes
weights always: ones when unweighted).  No reference source is copied: the fixture holds seeds,
checksums, F matrices, distances, inlier counts and tolerances; inputs are rebuilt from the seeds.

F matrices are compared after scaling both to unit Frobenius norm and aligning the sign, by the
largest absolute entry difference (epipolar_cases.f_err).  The tolerance of a case is 100 x the
difference between two other solvers on the same points -- the numpy restatement (np.linalg.eigh)
and the reference's torch.svd route --, floor 1e-12.  Distances are compared relative to the
largest distance of the set, max |a - b| / max |b| (a distance near zero is a cancelled sum and has
no relative accuracy of its own); tolerance 100 x the same two routes' difference, floor 1e-12.

RANSAC cases (rr_verify_pairs_epipolar, restated by epipolar_cases.epipolar_batch).  The case seed
advances until, for every pair,
  * no residual of any root of any hypothesis or refit lies within 1e-7 px of th;
  * the two null-space solvers (SVD, Gauss-Jordan) give the same winner (t, root) and outputs;
  * they give the same count table for every hypothesis whose best count is within 1 of the winner's;
  * the final inlier set holds at least 80 % of the planted matches (pairs with >= 8 planted
    matches and iters >= 256) -- so a case is a verification that works, not only one that is stable.
The tolerance of a pair's F is 100 x the difference of two solvers on the records the returned F
was fitted to: numpy eigh against the reference's find_fundamental for a refitted F, the SVD route
against the Gauss-Jordan route for a seven-point F; floor 1e-12.

Arrays: fund_seeds / fund_chk / fund<k>_F / fund<k>_{sam,sam_rt,sym,sym_rt} / fund_tol / fund_tol_d per
8-point case k; e_seeds / e_chk / e<k>_inl / e<k>_F / e<k>_mask / e<k>_t / e<k>_root / e<k>_tol per RANSAC case.
"""

import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the reference tree
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("RR_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REF)   # the reference's cirtorch package, not this repository's

import numpy as np  # noqa: E402
import torch  # noqa: E402

import epipolar_cases as EC  # noqa: E402
from cirtorch.geometry.epipolar import fundamental as RF  # noqa: E402
from cirtorch.geometry.epipolar import metrics as RM  # noqa: E402

assert os.path.abspath(RF.__file__).startswith(os.path.abspath(REF)), RF.__file__
MARGIN = 1e-7
FLOOR = 1e-12
KINDS = [("sam", "sampson", True), ("sam_rt", "sampson", False), ("sym", "symmetrical", True), ("sym_rt", "symmetrical", False)]


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def ref_fund(p1, p2, w=None):
    w = np.ones(len(p1)) if w is None else w
    return RF.find_fundamental(t64(p1)[None], t64(p2)[None], t64(w)[None])[0].numpy()


def ref_dist(p1, p2, F, kind, squared):
    fn = RM.sampson_epipolar_distance if kind == "sampson" else RM.symmetrical_epipolar_distance
    return fn(t64(p1)[None], t64(p2)[None], t64(F)[None], squared=squared)[0].numpy()


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def fund_cases(out):
    seeds, chk, tol, tol_d = [], [], [], []
    for k, (b, n, weighted) in enumerate(EC.FUND_CASES):
        seed = EC.FUND_SEED + 10 * k
        p1, p2, w = EC.fund_points(b, n, weighted, seed)
        Fr = np.stack([ref_fund(p1[i], p2[i], w[i]) for i in range(b)])
        Fb = RF.find_fundamental(t64(p1), t64(p2), t64(w)).numpy()   # the batched call agrees with the per-set calls
        assert max(EC.f_err(Fb[i], Fr[i]) for i in range(b)) < 1e-9
        d = max(EC.f_err(EC.fundamental(p1[i], p2[i], w[i]), Fr[i]) for i in range(b))
        dd = 0.0
        for key, kind, squared in KINDS:
            ref = np.stack([ref_dist(p1[i], p2[i], Fr[i], kind, squared) for i in range(b)])
            dd = max(dd, max(rel(EC.distance(p1[i], p2[i], Fr[i], kind, squared), ref[i]) for i in range(b)))
            out["fund%d_%s" % (k, key)] = ref
        seeds.append(seed)
        chk.append(EC.checksum(p1, p2, w))
        tol.append(max(100 * d, FLOOR))
        tol_d.append(max(100 * dd, FLOOR))
        out["fund%d_F" % k] = Fr
        print("  8-point case %d (B %d, N %d, %s): eigh vs svd %.3g -> tol %.3g; distances rel %.3g -> tol %.3g" % (
            k, b, n, "weighted" if weighted else "unweighted", d, tol[-1], dd, tol_d[-1]))
    out.update(fund_seeds=np.array(seeds, dtype=np.int64), fund_chk=np.array(chk), fund_tol=np.array(tol),
               fund_tol_d=np.array(tol_d))


def pair_ok(spec, a, b, planted):
    """the conditions on one pair (a: the SVD route, b: the Gauss-Jordan route) -> (ok, text)"""
    n1, n2, m, frac, noise = spec["pair"]
    if not (a["margin"] >= MARGIN and b["margin"] >= MARGIN):
        return False, "margin %.3g / %.3g" % (a["margin"], b["margin"])
    if (a["t"], a["root"], a["inliers"]) != (b["t"], b["root"], b["inliers"]) or not np.array_equal(a["mask"], b["mask"]):
        return False, "winners (%d, %d): %d vs (%d, %d): %d" % (a["t"], a["root"], a["inliers"], b["t"], b["root"], b["inliers"])
    if a["t"] >= 0:
        top = a["counts"].max()
        near = (a["counts"].max(1) >= top - 1) | (b["counts"].max(1) >= top - 1)
        if not np.array_equal(a["counts"][near], b["counts"][near]):
            return False, "count tables differ near the winner"
    nplant = int(planted.sum())
    if nplant >= 8 and spec["iters"] >= 256:
        got = int((a["mask"] & planted).sum())
        if got < 0.8 * nplant:
            return False, "recovered %d of %d" % (got, nplant)
    return True, "margin %.3g, roots differ in %d hypotheses" % (min(a["margin"], b["margin"]), int((a["nroots"] != b["nroots"]).sum()))


def pair_tol(a, b):
    fit = a["fit"]
    if fit is None:
        return FLOOR
    if len(fit) >= 8:
        d = EC.f_err(EC.fundamental(fit[:, :2], fit[:, 2:]), ref_fund(fit[:, :2], fit[:, 2:]))
    else:
        d = EC.f_err(a["F"], b["F"])
    return max(100 * d, FLOOR)


def epi_cases(out):
    seeds, chk = [], []
    for k, case in enumerate(EC.EPI_CASES):
        for attempt in range(50):
            seed = EC.EPI_SEED + 100 * k + 1000 * attempt
            kp1, off1, kp2, off2, match, planted = EC.build_case(case, seed)
            args = (kp1, off1, kp2, off2, match, EC.TH, case["iters"], case["refine"], EC.RUN_SEED)
            inl, Fs, mask, A = EC.epipolar_batch(*args)
            _, _, _, B = EC.epipolar_batch(*args, null=EC.null_gj)
            res = [pair_ok(dict(pair=case["pairs"][p], iters=case["iters"]), A[p], B[p], planted[off1[p]:off1[p + 1]])
                   for p in range(len(A))]
            if all(r[0] for r in res):
                break
            print("    case %s seed %d refused: %s" % (case["name"], seed, [r[1] for r in res]))
        assert all(r[0] for r in res), "no seed of case %s meets the conditions" % case["name"]
        tol = np.array([pair_tol(A[p], B[p]) for p in range(len(A))])
        seeds.append(seed)
        chk.append(EC.checksum(kp1, kp2, match))
        out["e%d_inl" % k], out["e%d_F" % k], out["e%d_mask" % k] = inl, Fs, mask
        out["e%d_t" % k] = np.array([o["t"] for o in A], dtype=np.int64)
        out["e%d_root" % k] = np.array([o["root"] for o in A], dtype=np.int64)
        out["e%d_tol" % k] = tol
        print("  epipolar case %s seed %d: M %s, winners (t, root) %s, inliers %s (planted %s), runner-up %s, %s, tol %s" % (
            case["name"], seed, [o["m"] for o in A], [(o["t"], o["root"]) for o in A], inl.tolist(),
            [int(planted[off1[p]:off1[p + 1]].sum()) for p in range(len(A))], [o["runner"] for o in A], [r[1] for r in res],
            ["%.2g" % v for v in tol]))
    out.update(e_seeds=np.array(seeds, dtype=np.int64), e_chk=np.array(chk))


def main():
    out = {}
    fund_cases(out)
    epi_cases(out)
    path = os.path.join(HERE, "epipolar.npz")
    np.savez_compressed(path, **out)
    print("  epipolar.npz: %d arrays, %.0f KB" % (len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
