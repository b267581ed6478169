"""Timing of batched spatial verification (rr_verify_pairs) against its float64 numpy restatement
on the host, at P = 1024 pairs, N1 = N2 = 1024 keypoints, about half of the side-1 rows matched
(half of those planted inliers of a homography, 0.5 px noise), iters = 1024, refine = 2.  HIP
events around every call, warm-up, median and min-max of the repeats.
    python tools/verify_probe.py [--reps 20] [--pairs 1024] [--n 1024] [--iters 1024] [--host-pairs 2]
Prints one JSON line:
  verify_us, verify_us_min_max   one verify_pairs call over all P pairs
  pairs_per_s                    P / median
  transfers                      P x iters x mean(M): the point transfers of the scoring walk
  f64_ops_per_transfer           12 (9 fused multiply-adds + 3 multiplies; compares not counted)
  model_floor_us                 transfers x 12 / 39.3e12 (the 78.6 TFLOP/s float64 vector peak counts an
                                 FMA as two operations)
  share_of_model                 model_floor_us / verify_us
  numpy_pairs_per_s              tests/verify_cases.verify_pair on --host-pairs of the same pairs
  inliers_equal                  the engine's counts == the restatement's on those pairs
Developer tool; A/B two builds with RR_LIB.
"""

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image-retrieval-for-image-based-localization_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

OPS_PER_TRANSFER = 12
F64_INSTR_PER_S = 78.6e12 / 2


def make_pairs(p, n, seed):
    """kp1, kp2 float32 [p, n, 2], match int64 [p, n]: half of the rows matched to a permutation
    of side 2, half of the matched rows images under the pair's homography plus 0.5 px noise"""
    import verify_cases as VC
    r = np.random.default_rng(seed)
    kp1 = r.uniform([0, 0], [VC.W, VC.H_IMG], (p, n, 2)).astype(np.float32)
    kp2 = r.uniform([0, 0], [VC.W, VC.H_IMG], (p, n, 2)).astype(np.float32)
    match = np.full((p, n), -1, dtype=np.int64)
    for i in range(p):
        Ht = VC.true_homography(r)
        kept = r.random(n) < 0.5
        rows = np.nonzero(kept)[0]
        cols = r.permutation(n)[:len(rows)]
        match[i, rows] = cols
        inl = r.random(len(rows)) < 0.5
        img = VC.transfer(Ht, kp1[i, rows[inl]].astype(np.float64)) + 0.5 * r.standard_normal((int(inl.sum()), 2))
        kp2[i, cols[inl]] = img.astype(np.float32)
    return kp1, kp2, match


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
    ap.add_argument("--host-pairs", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("verify_probe needs a GPU")
    import verify_cases as VC
    from cirtorch import _engine as E
    from cirtorch.search import verify_pairs
    from tools.src_digest import digest
    kp1, kp2, match = make_pairs(args.pairs, args.n, 17)
    d1, d2, dm = (torch.from_numpy(a).cuda() for a in (kp1, kp2, match))
    run = lambda: verify_pairs(d1, d2, dm, th=3.0, iters=args.iters, refine=args.refine, seed=1)  # noqa: E731
    times = []
    for r in range(args.warmup + args.reps):
        t = once(run)
        if r >= args.warmup:
            times.append(t)
    inl = run()[0].cpu().numpy()
    t0 = time.perf_counter()
    host = [VC.verify_pair(kp1[i], kp2[i], match[i], i, 3.0, args.iters, args.refine, 1)["inliers"] for i in range(args.host_pairs)]
    host_s = time.perf_counter() - t0
    med = statistics.median(times)
    transfers = float(args.iters) * float((match >= 0).sum())
    floor_us = transfers * OPS_PER_TRANSFER / F64_INSTR_PER_S * 1e6
    out = {"pairs": args.pairs, "n": args.n, "iters": args.iters, "refine": args.refine, "reps": args.reps,
           "kept_fraction": round(float((match >= 0).mean()), 3), "mean_inliers": round(float(inl.mean()), 1),
           "build": E.lib().rr_build_info().decode(), "tree_digest": digest(), "device": E.device_arch(),
           "verify_us": round(med, 1), "verify_us_min_max": [round(min(times), 1), round(max(times), 1)],
           "pairs_per_s": round(args.pairs / med * 1e6, 1), "transfers": transfers,
           "f64_ops_per_transfer": OPS_PER_TRANSFER, "model_floor_us": round(floor_us, 1),
           "share_of_model": round(floor_us / med, 3),
           "numpy_pairs_per_s": round(args.host_pairs / host_s, 3) if args.host_pairs else None,
           "inliers_equal": bool((inl[:args.host_pairs] == np.array(host, dtype=inl.dtype)).all())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
