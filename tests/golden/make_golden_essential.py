"""Generate tests/golden/essential.npz.

    python tests/golden/make_golden_essential.py

The upstream project has no five-point solver and no RANSAC on the essential matrix, so nothing here
is generated from it: the oracle is the float64 numpy restatement of tests/essential_cases.py with its
two independent minimal solvers (A: SVD null space, action matrix, np.linalg.eig; B: the header's
construction with np.roots).  The fixture holds seeds, input checksums, the oracle's inlier counts,
masks, winners and matrices, and tolerances; inputs are rebuilt from the seeds.

Matrices are compared after scaling both to unit Frobenius norm and aligning the sign, by the largest
absolute entry difference (epipolar_cases.f_err).  The tolerance of a pair's E, and of a sample's
solutions in the minimal-solver set, is 100 x the difference between solvers A and B on it, floor 1e-12.

RANSAC cases (essential_cases.ALL_CASES).  The case seed advances until, for every pair,
  * no Sampson distance of any root of any hypothesis or refit lies within 1e-7 px of th (A and B);
  * A and B agree on the winning t, on its count, on the mask and on the number of real roots of the
    winning sample;
  * the winner's count is not shared by another root of the same t -- where it can be: with M = 5 every
    root of every sample passes through all five records, and the winner is root 0 of t = 0 by the
    tie rule (root asc), which then checks the ascending order itself;
  * a pair with >= 8 planted matches and iters >= 256 recovers at least 80 % of them.
For the planar case the generator also asserts that the essential model's false-inlier count is not
above the fundamental model's (epipolar_cases.epipolar_pair on the same pair), and stores both.

Minimal-solver set (essential_cases.solver_samples): samples whose degree-10 polynomial has two roots
within 1e-4 (relative) of each other or of the real axis are dropped, at most 2 % of them; A and B must
agree on the number of roots of every kept sample.  s_resid is 100 x the oracle's own largest
|h2^T E h1| over the kept samples.

Arrays: c_seeds / c_chk and c<k>_inl / c<k>_E / c<k>_mask / c<k>_t / c<k>_root / c<k>_tol per case k;
planar_false (essential, fundamental); s_seed / s_chk / s_nroots / s_tol / s_resid / s_drop.
"""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402

import epipolar_cases as EC  # noqa: E402
import essential_cases as SC  # noqa: E402

MARGIN = 1e-7
FLOOR = 1e-12


def pair_ok(spec, a, b, planted):
    """the conditions on one pair (a: solver A, b: solver B) -> (ok, text)"""
    if spec["pair"][5] == "singular":
        return a["t"] == -1 and b["t"] == -1 and a["inliers"] == 0, "singular K"
    if not (a["margin"] >= MARGIN and b["margin"] >= MARGIN):
        return False, "margin %.3g / %.3g" % (a["margin"], b["margin"])
    if (a["t"], a["inliers"]) != (b["t"], b["inliers"]) or not np.array_equal(a["mask"], b["mask"]):
        return False, "winners %d: %d vs %d: %d" % (a["t"], a["inliers"], b["t"], b["inliers"])
    if a["t"] >= 0:
        t = a["t"]
        if a["root"] != b["root"] or a["nroots"][t] != b["nroots"][t]:
            return False, "roots of the winning sample: %d of %d vs %d of %d" % (a["root"], a["nroots"][t], b["root"], b["nroots"][t])
        for o in (a, b):
            if o["m"] > 5 and (o["counts"][t] == o["counts"][t].max()).sum() != 1:
                return False, "the winner's count is shared by another root"
    nplant = int(planted.sum())
    if nplant >= 8 and spec["iters"] >= 256:
        got = int((a["mask"] & planted).sum())
        if got < 0.8 * nplant:
            return False, "recovered %d of %d" % (got, nplant)
    return True, "margin %.3g" % min(a["margin"], b["margin"])


def cases(out):
    seeds, chk = [], []
    for k, case in enumerate(SC.ALL_CASES):
        for attempt in range(50):
            seed = SC.ESS_SEED + 100 * k + 2000 * attempt
            kp1, off1, kp2, off2, match, planted, K1, K2, parts = SC.build_case(case, seed)
            args = (kp1, off1, kp2, off2, match, K1, K2, SC.TH, case["iters"], case["refine"], SC.RUN_SEED)
            inl, Es, mask, B = SC.essential_batch(*args, solver="B")
            _, EsA, _, A = SC.essential_batch(*args, solver="A")
            res = [pair_ok(dict(pair=case["pairs"][p], iters=case["iters"]), A[p], B[p], planted[off1[p]:off1[p + 1]])
                   for p in range(len(A))]
            ok = all(r[0] for r in res)
            false = None
            if ok and case["name"] == "planar":
                f = EC.epipolar_pair(kp1, kp2, match, 0, SC.TH, case["iters"], case["refine"], SC.RUN_SEED)
                false = (int((mask & ~planted).sum()), int((f["mask"] & ~planted).sum()))
                if false[0] > false[1]:
                    ok, res = False, [(False, "false inliers: essential %d, fundamental %d" % false)]
            if ok:
                break
            print("    case %s seed %d refused: %s" % (case["name"], seed, [r[1] for r in res]))
        assert ok, "no seed of case %s meets the conditions" % case["name"]
        if false is not None:
            out["planar_false"] = np.array(false, dtype=np.int64)
        tol = np.array([max(100 * EC.f_err(EsA[p], Es[p]), FLOOR) if inl[p] else FLOOR for p in range(len(A))])
        seeds.append(seed)
        chk.append(SC.checksum(kp1, kp2, match))
        out["c%d_inl" % k], out["c%d_E" % k], out["c%d_mask" % k] = inl, Es, mask
        out["c%d_t" % k] = np.array([o["t"] for o in B], dtype=np.int64)
        out["c%d_root" % k] = np.array([o["root"] for o in B], dtype=np.int64)
        out["c%d_tol" % k] = tol
        print("  case %s seed %d: M %s, winners (t, root) %s, inliers %s (planted %s), %s, tol %s%s" % (
            case["name"], seed, [o["m"] for o in B], [(o["t"], o["root"]) for o in B], inl.tolist(),
            [int(planted[off1[p]:off1[p + 1]].sum()) for p in range(len(B))], [r[1] for r in res], ["%.2g" % v for v in tol],
            "" if false is None else ", false inliers essential %d / fundamental %d" % false))
    out.update(c_seeds=np.array(seeds, dtype=np.int64), c_chk=np.array(chk))


def solver_set(out):
    x1, x2, E, nroots, drop, diffs, resid = SC.solver_samples()
    assert drop <= 0.02, drop
    assert (nroots % 2 == 0).all() and nroots.max() <= 10
    out.update(s_seed=np.int64(SC.SOLVER_SEED), s_chk=np.array(SC.checksum(x1, x2)), s_nroots=nroots,
               s_tol=np.maximum(100 * diffs, FLOOR), s_resid=np.float64(100 * resid), s_drop=np.float64(drop))
    print("  minimal solver: %d samples kept, %.2f %% dropped, roots histogram %s, A - B up to %.3g (median %.3g), "
          "largest residual %.3g -> bound %.3g" % (len(x1), 100 * drop, np.bincount(nroots, minlength=11).tolist(), diffs.max(),
                                                   np.median(diffs), resid, 100 * resid))


def main():
    out = {}
    solver_set(out)
    cases(out)
    path = os.path.join(HERE, "essential.npz")
    np.savez_compressed(path, **out)
    print("  essential.npz: %d arrays, %.0f KB" % (len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
