"""Generate tests/golden/verify.npz (build container only, like make_golden_match.py).

    python tests/golden/make_golden_verify.py

From the reference, unmodified and imported as a package: cirtorch/geometry/homography.py
(find_homography_dlt, find_homography_dlt_iterated), run in float64 on the point sets of
tests/verify_cases.py, with and without weights.  No reference source is copied: the fixture
holds seeds, checksums, H matrices, inlier lists and tolerances.

The reference's own float32 run is no usable target (its corner transfer differs from its
float64 run by 4e-4 .. 1.4e-3 px at N >= 8 and by up to 247 px at N = 4, weighted).

H matrices are compared by the transfer of the four image corners, in pixels.  tol_px of a case is
100 x the difference between the numpy restatement (np.linalg.eigh; np.linalg.solve for a 4-point
fit) and the reference's float64 torch.svd route on the same points, floor 1e-9 px: the
conditioning of the case as seen by two solvers, times a factor for solver constants.

RANSAC cases (rr_verify_pairs, restated by verify_cases.verify_batch).  The case seed advances
until, for every pair,
  * no residual of any hypothesis or refit lies within 1e-7 px of th;
  * the winner's count exceeds every other hypothesis's -- asserted where the counts can differ
    (pairs with planted outliers and at least 40 matches, iters > 1): a pair of 4 or 5 matches,
    a noise-free pair and an all-outlier pair tie by construction, and there the winner is the
    lowest t among equals, exact given the residual margin (``strict`` records which pairs were
    held to it);
  * the final inlier set holds at least 90 % of the planted inliers (pairs with >= 4 planted
    inliers and iters >= 256).

Arrays: dlt_seeds / dlt_chk / dlt<k>_H / dlt<k>_Hit / dlt_tol / dlt_tol_it per DLT case k;
v_seeds / v_chk / v<k>_inl / v<k>_H / v<k>_mask / v<k>_t / v<k>_tol / v<k>_strict per RANSAC case.
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

import verify_cases as VC  # noqa: E402
from cirtorch.geometry import homography as RH  # noqa: E402

assert os.path.abspath(RH.__file__).startswith(os.path.abspath(REF)), RH.__file__
MARGIN = 1e-7
FLOOR = 1e-9


def ref_dlt(p1, p2, w=None):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))[None]  # noqa: E731
    return RH.find_homography_dlt(t(p1), t(p2), t(w))[0].numpy()


def ref_iter(p1, p2, w):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))[None]  # noqa: E731
    return RH.find_homography_dlt_iterated(t(p1), t(p2), t(w))[0].numpy()


def dlt_cases(out):
    seeds, chk, tol, tol_it = [], [], [], []
    for k, (b, n, weighted) in enumerate(VC.DLT_CASES):
        seed = VC.DLT_SEED + 10 * k
        p1, p2, w = VC.dlt_points(b, n, weighted, seed)
        ones = np.ones((b, n))
        Hr = np.stack([ref_dlt(p1[i], p2[i], None if w is None else w[i]) for i in range(b)])
        Hi = np.stack([ref_iter(p1[i], p2[i], ones[i] if w is None else w[i]) for i in range(b)])
        # the batched call of the reference agrees with its per-set calls
        Hb = RH.find_homography_dlt(torch.from_numpy(p1), torch.from_numpy(p2), None if w is None else torch.from_numpy(w)).numpy()
        assert max(VC.corner_err(Hb[i], Hr[i]) for i in range(b)) < 1e-9
        d = max(VC.corner_err(VC.dlt(p1[i], p2[i], None if w is None else w[i]), Hr[i]) for i in range(b))
        di = max(VC.corner_err(VC.dlt_iterated(p1[i], p2[i], ones[i] if w is None else w[i]), Hi[i]) for i in range(b))
        seeds.append(seed)
        chk.append(VC.checksum(p1, p2, ones if w is None else w))
        tol.append(max(100 * d, FLOOR))
        tol_it.append(max(100 * di, FLOOR))
        out["dlt%d_H" % k], out["dlt%d_Hit" % k] = Hr, Hi
        print("  dlt case %d (B %d, N %d, %s): eigh vs svd %.3g px (iterated %.3g) -> tol %.3g / %.3g px" % (
            k, b, n, "weighted" if weighted else "unweighted", d, di, tol[-1], tol_it[-1]))
    out.update(dlt_seeds=np.array(seeds, dtype=np.int64), dlt_chk=np.array(chk), dlt_tol=np.array(tol),
               dlt_tol_it=np.array(tol_it))


def pair_ok(spec, info, planted):
    """the three conditions on one pair -> (ok, strict, text)"""
    n1, n2, m, frac, noise = spec["pair"]
    iters = spec["iters"]
    strict = m >= 40 and 0.0 < frac < 1.0 and noise > 0 and iters > 1
    if not info["margin"] >= MARGIN:
        return False, strict, "margin %.3g" % info["margin"]
    if strict and not (info["t"] >= 0 and info["count0"] > info["runner"]):
        return False, strict, "winner %d vs runner-up %d" % (info["count0"], info["runner"])
    nplant = int(planted.sum())
    if nplant >= 4 and iters >= 256:
        rec = int((info["mask"] & planted).sum())
        if rec < 0.9 * nplant:
            return False, strict, "recovered %d of %d" % (rec, nplant)
    return True, strict, "margin %.3g" % info["margin"]


def pair_tol(info):
    """100 x (numpy restatement vs the reference's svd route) on the points the returned H was fitted to"""
    fit = info["fit"]
    if fit is None:
        return FLOOR
    Hr = ref_dlt(fit[:, :2], fit[:, 2:])
    d = VC.corner_err(VC.dlt(fit[:, :2], fit[:, 2:]), Hr)
    if len(fit) == 4:
        d = max(d, VC.corner_err(VC.four_point(fit[:, :2], fit[:, 2:]), Hr))
    return max(100 * d, FLOOR)


def verify_cases(out):
    seeds, chk = [], []
    for k, case in enumerate(VC.VERIFY_CASES):
        for attempt in range(50):
            seed = VC.VERIFY_SEED + 100 * k + 1000 * attempt
            kp1, off1, kp2, off2, match, planted = VC.build_case(case, seed)
            inl, Hs, mask, infos = VC.verify_batch(kp1, off1, kp2, off2, match, VC.TH, case["iters"], case["refine"], VC.RUN_SEED)
            oks, stricts, notes = [], [], []
            for p, info in enumerate(infos):
                # the winner's own count before any refit, for the runner-up condition
                o0 = VC.verify_pair(kp1[off1[p]:off1[p + 1]], kp2[off2[p]:off2[p + 1]], match[off1[p]:off1[p + 1]], p,
                                    VC.TH, case["iters"], 0, VC.RUN_SEED)
                info["count0"] = o0["inliers"]
                ok, strict, note = pair_ok(dict(pair=case["pairs"][p], iters=case["iters"]), info, planted[off1[p]:off1[p + 1]])
                oks.append(ok)
                stricts.append(strict)
                notes.append(note)
            if all(oks):
                break
            print("    case %s seed %d refused: %s" % (case["name"], seed, notes))
        assert all(oks), "no seed of case %s meets the conditions" % case["name"]
        tol = np.array([pair_tol(info) for info in infos])
        seeds.append(seed)
        chk.append(VC.checksum(kp1, kp2, match))
        out["v%d_inl" % k], out["v%d_H" % k], out["v%d_mask" % k] = inl, Hs, mask
        out["v%d_t" % k] = np.array([info["t"] for info in infos], dtype=np.int64)
        out["v%d_tol" % k] = tol
        out["v%d_strict" % k] = np.array(stricts, dtype=bool)
        print("  verify case %s seed %d: M %s, winners t %s, inliers %s (planted %s), runner-up %s, %s, tol %s px" % (
            case["name"], seed, [i["m"] for i in infos], [i["t"] for i in infos], inl.tolist(),
            [int(planted[off1[p]:off1[p + 1]].sum()) for p in range(len(infos))], [i["runner"] for i in infos], notes,
            ["%.2g" % v for v in tol]))
    out.update(v_seeds=np.array(seeds, dtype=np.int64), v_chk=np.array(chk))


def main():
    out = {}
    dlt_cases(out)
    verify_cases(out)
    path = os.path.join(HERE, "verify.npz")
    np.savez_compressed(path, **out)
    print("  verify.npz: %d arrays, %.0f KB" % (len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
