"""Timing of calibrated verification (rr_verify_pairs_essential, verify_pairs(model="essential")) beside
the uncalibrated call (rr_verify_pairs_epipolar, model="fundamental") in the same process and on the
same pairs: the re-ranking shape k = 100 x Q = 128 -> P = 12 800 pairs of N1 = N2 = 2048 keypoints with
300 kept matches, half of them planted correspondences of the pair's two-view scene (0.3 px noise),
iters 1024, refine 2, th 1.5 px.  --distinct scenes are generated and repeated to P pairs.  HIP events
around every call, warm-up, the models alternating, median and min-max.
    python tools/essential_probe.py [--reps 10] [--pairs 12800] [--n 2048] [--matched 300] [--iters 1024] [--out profiles/essential_probe.json]
Prints (and writes to --out) one JSON line:
  essential_us, fundamental_us (+ _min_max)   one verify_pairs call over all P pairs
  ratio                                       essential_us / fundamental_us
  mean_inliers_essential / _fundamental, mean_planted
  five_point_us, mean_roots                   rr_essential_5pt alone on P x 1024 / 16 samples, and their mean number of real roots
No time is fixed in advance.  The five-point solver does several times the arithmetic of the
seven-point one and scores up to ten matrices per sample instead of three, so a ratio well above 1 is
expected; one above about 10 would point at scratch traffic inside the scoring walk.
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


def make_pairs(p, n, matched, distinct, seed):
    """kp1, kp2 float32 [p, n, 2], match int64 [p, n], planted bool [p, n]"""
    import epipolar_cases as EC
    parts = [EC.planted_pair(n, n, matched, 0.5, 0.3, seed + i) for i in range(distinct)]
    idx = np.arange(p) % distinct
    return tuple(np.stack([q[i] for q in parts])[idx] for i in range(4))


def once(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return 1000 * t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=12800)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--matched", type=int, default=300)
    ap.add_argument("--iters", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "essential_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("essential_probe needs a GPU")
    import epipolar_cases as EC
    from cirtorch import _engine as E
    from cirtorch.geometry.epipolar import run_5point
    from cirtorch.search import verify_pairs
    from tools.src_digest import digest
    kp1, kp2, match, planted = make_pairs(args.pairs, args.n, args.matched, min(args.distinct, args.pairs), 2900)
    d1, d2, dm = (torch.from_numpy(a).cuda() for a in (kp1, kp2, match))
    K = torch.from_numpy(EC.K).cuda()
    kw = dict(th=EC.TH, iters=args.iters, refine=2, seed=3)
    # five-point samples: the first five planted matches of every pair, repeated
    Ki = np.linalg.inv(EC.K)
    ns = max(1, args.pairs * args.iters // 16)
    rows = np.stack([np.nonzero(planted[i])[0][:5] for i in range(min(args.distinct, args.pairs))])
    a = np.concatenate([kp1[np.arange(len(rows))[:, None], rows], np.ones(rows.shape + (1,))], -1) @ Ki.T
    b = np.concatenate([kp2[np.arange(len(rows))[:, None], match[np.arange(len(rows))[:, None], rows]], np.ones(rows.shape + (1,))], -1) @ Ki.T
    rep = np.arange(ns) % len(rows)
    x1, x2 = torch.from_numpy(a[rep, :, :2].copy()).cuda(), torch.from_numpy(b[rep, :, :2].copy()).cuda()
    run = {"essential": lambda: verify_pairs(d1, d2, dm, model="essential", K1=K, K2=K, **kw),
           "fundamental": lambda: verify_pairs(d1, d2, dm, model="fundamental", **kw),
           "five_point": lambda: run_5point(x1, x2)}
    times = {m: [] for m in run}
    for r in range(args.warmup + args.reps):
        for m in run:
            t = once(run[m])
            if r >= args.warmup:
                times[m].append(t)
    ie, _, _ = run["essential"]()
    jf, _, _ = run["fundamental"]()
    _, nr = run["five_point"]()
    med = {m: statistics.median(times[m]) for m in run}
    out = {"pairs": args.pairs, "n": args.n, "matched": args.matched, "iters": args.iters, "distinct": min(args.distinct, args.pairs),
           "reps": args.reps, "build": E.lib().rr_build_info().decode(), "tree_digest": digest(), "device": E.device_arch()}
    for m in run:
        out[m + "_us"] = round(med[m], 1)
        out[m + "_us_min_max"] = [round(min(times[m]), 1), round(max(times[m]), 1)]
    out["ratio"] = round(med["essential"] / med["fundamental"], 2)
    out["five_point_samples"] = ns
    out["mean_roots"] = round(float(nr.float().mean().item()), 2)
    out["mean_inliers_essential"] = round(float(ie.float().mean().item()), 1)
    out["mean_inliers_fundamental"] = round(float(jf.float().mean().item()), 1)
    out["mean_planted"] = round(float(planted.sum(1).mean()), 1)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
