"""Timing of batched epipolar verification (rr_verify_pairs_epipolar, verify_pairs(model="fundamental"))
beside the homography call (rr_verify_pairs) in the same process and on the same pairs: the shapes of
tools/verify_probe.py -- P = 1024 pairs, N1 = N2 = 1024 keypoints, about half of the side-1 rows
matched, half of those planted correspondences of a two-view scene (0.3 px noise), iters = 1024,
refine = 2.  HIP events around every call, warm-up, the two models alternating call by call, median and
min-max of the repeats.
    python tools/epipolar_probe.py [--reps 20] [--pairs 1024] [--n 1024] [--iters 1024] [--host-pairs 1]
Prints one JSON line:
  fundamental_us, homography_us (+ _min_max)   one verify_pairs call over all P pairs
  ratio                                        fundamental_us / homography_us (medians)
  roots_per_hypothesis                         mean number of real roots on the --host-pairs pairs (numpy restatement)
  inliers_equal                                the engine's counts == the restatement's on those pairs
  mean_inliers_fundamental / _homography       the planted scene is 3-D: the homography finds a plane's worth
Developer tool; A/B two builds with RR_LIB.
"""

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image-retrieval-for-image-based-localization_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_pairs(p, n, seed):
    """kp1, kp2 float32 [p, n, 2], match int64 [p, n]: about half of the rows matched, half of the
    matched rows true correspondences of the pair's two-view scene plus 0.3 px noise"""
    import epipolar_cases as EC
    parts = [EC.planted_pair(n, n, n // 2, 0.5, 0.3, seed + i) for i in range(p)]
    return tuple(np.stack([q[i] for q in parts]) for i in range(3))


def once(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return 1000 * t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=1024)
    ap.add_argument("--refine", type=int, default=2)
    ap.add_argument("--th", type=float, default=1.5)
    ap.add_argument("--host-pairs", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("epipolar_probe needs a GPU")
    import epipolar_cases as EC
    from cirtorch import _engine as E
    from cirtorch.search import verify_pairs
    from tools.src_digest import digest
    kp1, kp2, match = make_pairs(args.pairs, args.n, 1700)
    d1, d2, dm = (torch.from_numpy(a).cuda() for a in (kp1, kp2, match))
    run = {m: (lambda m=m: verify_pairs(d1, d2, dm, th=args.th, iters=args.iters, refine=args.refine, seed=1, model=m))
           for m in ("fundamental", "homography")}
    times = {m: [] for m in run}
    for r in range(args.warmup + args.reps):
        for m in run:
            t = once(run[m])
            if r >= args.warmup:
                times[m].append(t)
    inl = {m: run[m]()[0].cpu().numpy() for m in run}
    host = [EC.epipolar_pair(kp1[i], kp2[i], match[i], i, args.th, args.iters, args.refine, 1) for i in range(args.host_pairs)]
    med = {m: statistics.median(times[m]) for m in run}
    out = {"pairs": args.pairs, "n": args.n, "iters": args.iters, "refine": args.refine, "th": args.th, "reps": args.reps,
           "kept_fraction": round(float((match >= 0).mean()), 3), "build": E.lib().rr_build_info().decode(),
           "tree_digest": digest(), "device": E.device_arch()}
    for m in run:
        out[m + "_us"] = round(med[m], 1)
        out[m + "_us_min_max"] = [round(min(times[m]), 1), round(max(times[m]), 1)]
        out["mean_inliers_" + m] = round(float(inl[m].mean()), 1)
    out["ratio"] = round(med["fundamental"] / med["homography"], 2)
    out["roots_per_hypothesis"] = round(float(np.mean([o["nroots"].mean() for o in host])), 3) if host else None
    out["inliers_equal"] = bool((inl["fundamental"][:args.host_pairs] == np.array([o["inliers"] for o in host], dtype=np.int32)).all())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
