"""Generate tests/golden/pnp.npz.

    RR_REFERENCE=<checkout of the reference> python tests/golden/make_golden_pnp.py

The upstream project has no absolute pose, so the localization part of the fixture is not generated from
it: the oracle is the float64 numpy restatement of tests/pnp_cases.py with its two independent routes
(A: the header's quartic with np.roots, the pose from the triangles' frames, the refit by the normal
equations; B: points 1 and 3 exchanged, Kabsch, np.linalg.lstsq).  The fixture holds seeds, input
checksums, the oracle's inlier counts, masks, winners (t, solution) and poses, and tolerances; inputs are
rebuilt from the seeds.  Only the camera part (cam_*) comes from the reference, imported unmodified as a
package: project_points / unproject_points of cirtorch/geometry/camera/perspective.py on seeded inputs.

Poses are compared by pnp_cases.pose_err: the largest absolute entry difference of R, and of t divided by
max(1, |t|).  The tolerance of a pair's pose, and of a sample's solutions in the minimal-solver set, is
100 x the difference between routes A and B on it, floor 1e-12.

RANSAC cases (pnp_cases.ALL_CASES).  The case seed advances until, for every pair,
  * no reprojection error of any solution of any hypothesis or refit lies within 1e-7 px of th (A and B);
  * A and B agree on the winning t, on its solution index, on its count and on the mask;
  * the winner's count is not shared by another solution of the same t, where M > 3 (with M = 3 every
    solution of the one sample there is passes through all three records, and the winner is solution 0
    of t = 0 by the tie rule);
  * a pair with >= 8 planted matches and iters >= 256 recovers at least 80 % of them.
For the noise-free case x_tol is the bound on the distance to the planted pose: 100 x the oracle's own
distance to it, at least the pair's tolerance.  For the chain case the generator asserts that the oracle
alone (numpy verifier -> numpy pose -> numpy localization) stays within 1.0 degree of the planted rotation
and translation direction, half of what the GPU test allows.

Minimal-solver set (pnp_cases.solver_samples): samples whose quartic has two roots within 1e-4 (relative) of
each other or of the real axis are dropped, at most 2 % of them; A and B must agree on the number of
solutions of every kept sample, and the counts seen include 1, 2 and 4.  s_resid is 100 x the oracle's own
largest reprojection residual (normalised coordinates) over the kept samples.

Arrays: c_seeds / c_chk and c<k>_inl / c<k>_R / c<k>_t / c<k>_mask / c<k>_tw / c<k>_sol / c<k>_tol per case k;
x_tol; chain_deg; s_seed / s_chk / s_nsol / s_tol / s_resid / s_drop; cam_seed / cam_uv / cam_xyz / cam_ray.
"""

import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the reference tree
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("RR_REFERENCE", "")
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402

import pnp_cases as PN  # noqa: E402
import pose_cases as PC  # noqa: E402

MARGIN = 1e-7
FLOOR = 1e-12


def pair_ok(spec, a, b, planted):
    """the conditions on one pair (a: route A, b: route B) -> (ok, text)"""
    if spec["pair"][5] == "singular":
        return a["t_win"] == -1 and b["t_win"] == -1 and a["inliers"] == 0, "singular K"
    if not (a["margin"] >= MARGIN and b["margin"] >= MARGIN):
        return False, "margin %.3g / %.3g" % (a["margin"], b["margin"])
    if (a["t_win"], a["sol"], a["inliers"]) != (b["t_win"], b["sol"], b["inliers"]) or not np.array_equal(a["mask"], b["mask"]):
        return False, "winners (%d, %d): %d vs (%d, %d): %d" % (a["t_win"], a["sol"], a["inliers"], b["t_win"], b["sol"], b["inliers"])
    if a["t_win"] >= 0:
        t = a["t_win"]
        if a["nsol"][t] != b["nsol"][t]:
            return False, "solutions of the winning sample: %d vs %d" % (a["nsol"][t], b["nsol"][t])
        for o in (a, b):
            if o["m"] > 3 and (o["counts"][t] == o["counts"][t].max()).sum() != 1:
                return False, "the winner's count is shared by another solution"
    nplant = int(planted.sum())
    if nplant >= 8 and spec["iters"] >= 256:
        got = int((a["mask"] & planted).sum())
        if got < 0.8 * nplant:
            return False, "recovered %d of %d" % (got, nplant)
    return True, "margin %.3g" % min(a["margin"], b["margin"])


def cases(out):
    seeds, chk = [], []
    for k, case in enumerate(PN.ALL_CASES):
        for attempt in range(50):
            seed = PN.PNP_SEED + 100 * k + 2000 * attempt
            kp, off1, X, valid, off2, match, planted, Ks, parts = PN.build_case(case, seed)
            args = (kp, off1, X, valid, off2, match, Ks, PN.TH, case["iters"], case["refine"], PN.RUN_SEED)
            inl, Rs, ts, mask, A = PN.pnp_batch(*args, route="A")
            _, Rb, tb, _, B = PN.pnp_batch(*args, route="B")
            res = [pair_ok(dict(pair=case["pairs"][p], iters=case["iters"]), A[p], B[p], planted[off1[p]:off1[p + 1]])
                   for p in range(len(A))]
            ok = all(r[0] for r in res)
            deg = None
            if ok and case["name"] == "chain":
                deg = (PC.rot_angle_deg(Rs[0], parts[0]["R"]), PC.dir_angle_deg(ts[0], parts[0]["t"]))
                if not (inl[0] > 0 and max(deg) < 1.0):
                    ok, res = False, [(False, "the oracle's chain: rotation %.3f deg, direction %.3f deg" % deg)]
            if ok:
                break
            print("    case %s seed %d refused: %s" % (case["name"], seed, [r[1] for r in res]))
        assert ok, "no seed of case %s meets the conditions" % case["name"]
        tol = np.array([max(100 * PN.pose_err(Rb[p], tb[p], Rs[p], ts[p]), FLOOR) if inl[p] else FLOOR for p in range(len(A))])
        if case["name"] == "exact":
            own = PN.pose_err(Rs[0], ts[0], parts[0]["R"], parts[0]["t"])
            out["x_tol"] = np.float64(max(100 * own, tol[0]))
            assert planted.sum() == 50 and inl[0] == 50 and mask[planted].all()
            print("  noise-free pair: the oracle's distance to the planted pose %.3g -> bound %.3g" % (own, out["x_tol"]))
        if deg is not None:
            out["chain_deg"] = np.array(deg)
        seeds.append(seed)
        chk.append(PN.case_checksum(kp, X, match))
        out["c%d_inl" % k], out["c%d_R" % k], out["c%d_t" % k], out["c%d_mask" % k] = inl, Rs, ts, mask
        out["c%d_tw" % k] = np.array([o["t_win"] for o in A], dtype=np.int64)
        out["c%d_sol" % k] = np.array([o["sol"] for o in A], dtype=np.int64)
        out["c%d_tol" % k] = tol
        print("  case %s seed %d: M %s, winners (t, solution) %s, inliers %s (planted %s), %s, tol %s%s" % (
            case["name"], seed, [o["m"] for o in A], [(o["t_win"], o["sol"]) for o in A], inl.tolist(),
            [int(planted[off1[p]:off1[p + 1]].sum()) for p in range(len(A))], [r[1] for r in res], ["%.2g" % v for v in tol],
            "" if deg is None else ", chain rotation %.3f deg direction %.3f deg" % deg))
    out.update(c_seeds=np.array(seeds, dtype=np.int64), c_chk=np.array(chk))


def solver_set(out):
    x, X, R, t, nsol, drop, diffs, resid = PN.solver_samples()
    assert drop <= 0.02, drop
    assert nsol.max() <= 4 and set(nsol.tolist()) >= {1, 2, 4}, np.bincount(nsol)
    out.update(s_seed=np.int64(PN.SOLVER_SEED), s_chk=np.array(PN.checksum(x, X)), s_nsol=nsol,
               s_tol=np.maximum(100 * diffs, FLOOR), s_resid=np.float64(100 * resid), s_drop=np.float64(drop))
    print("  minimal solver: %d samples kept, %.2f %% dropped, solutions histogram %s, A - B up to %.3g (median %.3g), "
          "largest residual %.3g -> bound %.3g" % (len(x), 100 * drop, np.bincount(nsol, minlength=5).tolist(), diffs.max(),
                                                   np.median(diffs), resid, 100 * resid))


def camera(out):
    assert REF, "set RR_REFERENCE to a checkout of the reference: the camera values come from its functions"
    sys.path.insert(0, REF)   # the reference's cirtorch package, not this repository's
    import torch
    import cirtorch.geometry.camera.perspective as RP
    assert os.path.abspath(RP.__file__).startswith(os.path.abspath(REF)), RP.__file__
    pts, Ks, uv, depth = (torch.from_numpy(a) for a in PN.cam_inputs())
    out.update(cam_seed=np.int64(PN.CAM_SEED), cam_uv=RP.project_points(pts, Ks).numpy(),
               cam_xyz=RP.unproject_points(uv, depth, Ks).numpy(),
               cam_ray=RP.unproject_points(uv, depth, Ks, normalize=True).numpy())
    print("  camera: project_points %s, unproject_points %s" % (out["cam_uv"].shape, out["cam_xyz"].shape))


def main():
    out = {}
    solver_set(out)
    cases(out)
    camera(out)
    path = os.path.join(HERE, "pnp.npz")
    np.savez_compressed(path, **out)
    print("  pnp.npz: %d arrays, %.0f KB" % (len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
