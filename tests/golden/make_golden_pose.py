"""Generate tests/golden/pose.npz (build container only, like make_golden_epipolar.py).

    python tests/golden/make_golden_pose.py

From the reference, unmodified and imported as a package: cirtorch/geometry/epipolar/essential.py
(essential_from_fundamental, motion_from_essential_choose_solution and through it
decompose_essential_matrix, motion_from_essential), triangulation.py (triangulate_points) and
projection.py (projection_from_KRt, depth), run in float64 on the CPU on the cases of
tests/pose_cases.py -- ONE PAIR PER CALL: the reference indexes Rs[:, mask_indices][:, 0, 0]
(essential.py:149-151), which applies the choice of pair 0 to a whole batch.  It is given the used
records of a pair and no mask.  No reference source is copied: the fixture holds seeds, input
checksums, R, t, points3d, counts and tolerances; inputs are rebuilt from the seeds.

Conditions.  The case seed advances until, for every pair,
  1. under each of the four candidates no used record has a depth with |d| < 1e-6 x the median scene depth;
  2. under each of the four candidates no used record has |w| within 1e-6 relative of 1e-8;
  3. the winner's count exceeds the runner-up's;
so that `front` and `front_mask` can be compared exactly and the choice does not depend on the signs
an SVD leaves open.  The reference and the numpy restatement (pose_cases.pose_pair) must then agree on
the choice.

Tolerances.  Per pair 100 x the difference between two independent CPU solvers on the same inputs --
the reference's torch.svd path and the numpy restatement (np.linalg.svd) --, floor 1e-12: the largest
absolute entry difference for R and for t, and for the points the largest absolute coordinate
difference relative to the median depth of the pair's true points.

End to end (verify_pairs(model="fundamental") -> recover_pose).  The two chains are the numpy
restatements (epipolar_cases.epipolar_pair, then pose_pair) and the reference's find_fundamental on the
records the returned F was fitted to followed by the reference's pose path; the conditions of
make_golden_epipolar.py on the verification (no residual within 1e-7 px of th, both null-space solvers
agree) hold, and the numpy chain stays below 1 degree of the planted rotation and translation direction.

Arrays: p_seeds / p_chk / p<k>_{R,t,X,front,fmask,tol} per single-pair case k; r_seed / r_chk /
r_{R,t,X,front,fmask,tol} for the ragged batch; e_seed / e_chk / e_{R,t,X,front,fmask,inl,tol} for the
end-to-end batch.  tol rows are (R, t, points).
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
import pose_cases as PC  # noqa: E402
from cirtorch.geometry.epipolar import essential as RE  # noqa: E402
from cirtorch.geometry.epipolar import fundamental as RF  # noqa: E402

assert os.path.abspath(RE.__file__).startswith(os.path.abspath(REF)), RE.__file__
FLOOR = 1e-12
GAP = 1e-6


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def ref_pose(F, Ka, Kb, rec):
    """the reference on the used records of one pair -> R [3, 3], t [3], X [M, 3]"""
    E = RE.essential_from_fundamental(t64(F)[None], t64(Ka)[None], t64(Kb)[None])
    R, t, X = RE.motion_from_essential_choose_solution(E, t64(Ka)[None], t64(Kb)[None], t64(rec[:, :2])[None],
                                                       t64(rec[:, 2:])[None], mask=None)
    return R[0].numpy(), t[0, :, 0].numpy(), X[0].numpy()


def pair_ok(o, scale):
    """conditions 1 - 3 on the restatement's diagnostics of one pair -> (ok, text)"""
    if o["slot"] < 0:
        return True, "zeros"
    c = np.sort(o["counts"])[::-1]
    if not o["depth"] >= GAP * scale:
        return False, "depth %.3g" % o["depth"]
    if not o["wgap"] >= GAP:
        return False, "w gap %.3g" % o["wgap"]
    if not c[0] > c[1]:
        return False, "counts %s" % o["counts"]
    return True, "counts %s, depth %.3g, w gap %.3g" % (o["counts"], o["depth"], o["wgap"])


def compare(o, s, F, mask):
    """the reference against the restatement on one pair -> (R, t, X [n1, 3] of the reference, tol [3])"""
    n1 = len(s["kp1"])
    if o["slot"] < 0:
        return np.zeros((3, 3)), np.zeros(3), np.zeros((n1, 3)), np.full(3, FLOOR)
    rows, rec = PC.records(s, mask)
    R, t, X = ref_pose(F, s["K1"], s["K2"], rec)
    scale = PC.median_depth(s["X"][rows])
    d = np.array([np.abs(R - o["R"]).max(), np.abs(t - o["t"]).max(), np.abs(X - o["points3d"][rows]).max() / scale])
    assert d[0] < 1e-6 and d[1] < 1e-6, ("the reference chose another motion", d, o["counts"])
    front = (X[:, 2] > 0) & ((X @ R.T)[:, 2] + t[2] > 0)
    assert np.array_equal(front, o["front_mask"][rows]) and front.sum() == o["front"]
    Xf = np.zeros((n1, 3))
    Xf[rows] = X
    return R, t, Xf, np.maximum(100 * d, FLOOR)


def single_cases(out):
    seeds, chk = [], []
    for k, case in enumerate(PC.CASES):
        for attempt in range(50):
            seed = PC.POSE_SEED + 100 * k + 10000 * attempt
            s, F, mask = PC.build_case(case, seed)
            o = PC.pose_pair(s["kp1"], s["kp2"], s["match"], mask, F, s["K1"], s["K2"])
            ok, text = pair_ok(o, PC.median_depth(s["X"]))
            if ok:
                break
            print("    case %s seed %d refused: %s" % (case["name"], seed, text))
        assert ok, "no seed of case %s meets the conditions" % case["name"]
        assert len(o["rows"]) == (case["m"] if mask is None else int(mask.sum()))
        R, t, X, tol = compare(o, s, F, mask)
        seeds.append(seed)
        chk.append(PC.checksum(s["kp1"], s["kp2"], s["match"], F, np.zeros(0) if mask is None else mask))
        out["p%d_R" % k], out["p%d_t" % k], out["p%d_X" % k], out["p%d_tol" % k] = R, t, X, tol
        out["p%d_front" % k], out["p%d_fmask" % k] = np.int32(o["front"]), o["front_mask"]
        err = "" if o["slot"] < 0 else ", rotation %.3f deg, direction %.3f deg of the truth" % (
            PC.rot_angle_deg(R, s["R"]), PC.dir_angle_deg(t, s["t"]))
        print("  pose case %s seed %d: used %d, %s%s, tol R %.2g t %.2g X %.2g" % (case["name"], seed, len(o["rows"]), text, err, *tol))
    out.update(p_seeds=np.array(seeds, dtype=np.int64), p_chk=np.array(chk))


def ragged_case(out):
    for attempt in range(50):
        seed = PC.RAGGED_SEED + 1000 * attempt
        scenes, Fs, mask = PC.build_ragged(seed)
        kp1, off1, kp2, off2, match = PC.ragged_arrays(scenes)
        infos = PC.pose_batch(kp1, off1, kp2, off2, match, mask, Fs, PC.K1, PC.K1)[6]
        res = [pair_ok(o, PC.median_depth(s["X"])) for o, s in zip(infos, scenes)]
        if all(r[0] for r in res):
            break
        print("    ragged seed %d refused: %s" % (seed, [r[1] for r in res]))
    assert all(r[0] for r in res)
    parts = [compare(o, s, Fs[p], mask[off1[p]:off1[p + 1]]) for p, (o, s) in enumerate(zip(infos, scenes))]
    out.update(r_seed=np.int64(seed), r_chk=np.array(PC.checksum(kp1, kp2, match, Fs, mask)),
               r_R=np.stack([q[0] for q in parts]), r_t=np.stack([q[1] for q in parts]),
               r_X=np.concatenate([q[2] for q in parts]), r_tol=np.stack([q[3] for q in parts]),
               r_front=np.array([o["front"] for o in infos], dtype=np.int32),
               r_fmask=np.concatenate([o["front_mask"] for o in infos]))
    ex = parts[4]   # the noise-free pair: the truth itself
    assert np.abs(ex[0] - np.eye(3)).max() < 1e-9 and np.abs(ex[1] - PC.T_EXACT).max() < 1e-9
    print("  ragged seed %d: fronts %s, %s, tol %s" % (seed, [o["front"] for o in infos], [r[1] for r in res],
                                                      [["%.2g" % v for v in q[3]] for q in parts]))


def e2e_case(out):
    for attempt in range(50):
        seed = PC.E2E_SEED + 1000 * attempt
        scenes = [PC.scene(*spec, seed + 17 * k) for k, spec in enumerate(PC.E2E)]
        ok, chains = True, []
        for p, s in enumerate(scenes):
            a = EC.epipolar_pair(s["kp1"], s["kp2"], s["match"], p, **PC.VER)
            b = EC.epipolar_pair(s["kp1"], s["kp2"], s["match"], p, null=EC.null_gj, **PC.VER)
            o = PC.pose_pair(s["kp1"], s["kp2"], s["match"], a["mask"], a["F"], s["K1"], s["K2"])
            same = (a["t"], a["root"], a["inliers"]) == (b["t"], b["root"], b["inliers"]) and np.array_equal(a["mask"], b["mask"])
            good = a["margin"] >= 1e-7 and b["margin"] >= 1e-7 and same and a["fit"] is not None and len(a["fit"]) >= 8 \
                and pair_ok(o, PC.median_depth(s["X"]))[0] and o["slot"] >= 0 \
                and PC.rot_angle_deg(o["R"], s["R"]) < 1.0 and PC.dir_angle_deg(o["t"], s["t"]) < 1.0
            ok = ok and good
            chains.append((a, o))
        if ok:
            break
        print("    end-to-end seed %d refused" % seed)
    assert ok
    parts = []
    for s, (a, o) in zip(scenes, chains):
        fit = a["fit"]
        w = torch.ones(1, len(fit), dtype=torch.float64)
        Fr = EC.unit(RF.find_fundamental(t64(fit[:, :2])[None], t64(fit[:, 2:])[None], w)[0].numpy())
        parts.append(compare(o, s, Fr, a["mask"]))
        print("  end-to-end pair: inliers %d, fronts %d, rotation %.3f deg, direction %.3f deg, F err between the chains %.2g, tol %s" % (
            a["inliers"], o["front"], PC.rot_angle_deg(o["R"], s["R"]), PC.dir_angle_deg(o["t"], s["t"]),
            EC.f_err(Fr, a["F"]), ["%.2g" % v for v in parts[-1][3]]))
    kp1, off1, kp2, off2, match = PC.ragged_arrays(scenes)
    # the stored values are the numpy chain's: the engine is compared with it
    out.update(e_seed=np.int64(seed), e_chk=np.array(PC.checksum(kp1, kp2, match)),
               e_R=np.stack([o["R"] for _, o in chains]), e_t=np.stack([o["t"] for _, o in chains]),
               e_X=np.concatenate([o["points3d"] for _, o in chains]), e_tol=np.stack([q[3] for q in parts]),
               e_front=np.array([o["front"] for _, o in chains], dtype=np.int32),
               e_fmask=np.concatenate([o["front_mask"] for _, o in chains]),
               e_inl=np.array([a["inliers"] for a, _ in chains], dtype=np.int32))


def main():
    out = {}
    single_cases(out)
    ragged_case(out)
    e2e_case(out)
    path = os.path.join(HERE, "pose.npz")
    np.savez_compressed(path, **out)
    print("  pose.npz: %d arrays, %.0f KB" % (len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
