"""Timing of batched localization (rr_localize_pairs, cirtorch.search.localize_pairs) beside calibrated
verification (rr_verify_pairs_essential, verify_pairs(model="essential")) in the same process and on the
same pairs: the re-ranking shape of tools/pose_probe.py, k = 100 x Q = 128 -> P = 12 800 pairs of N1 = N2 =
2048 keypoints with 300 kept matches, half of them planted (0.3 px noise), iters 1024, refine 2.  A pair
is a two-view scene of tests/pose_cases.py seen from its second view: the query keypoints are that view's,
the 3-D points are the scene's in the first view's frame (indexed by the first view's keypoint rows), and the
match list is the scene's, inverted.  The essential verifier gets the same query keypoints, the first view's
keypoints and the same match list, so both calls walk the same 300 records per pair.  --distinct scenes
are generated and repeated to P pairs.  HIP events around every call, warm-up, the calls alternating,
median and min-max.
    python tools/pnp_probe.py [--reps 10] [--pairs 12800] [--n 2048] [--matched 300] [--iters 1024] [--out profiles/pnp_probe.json]
Prints (and writes to --out) one JSON line:
  localize_us, essential_us (+ _min_max)   one call over all P pairs;  _per_pair beside them
  ratio                                    localize_us / essential_us
  p3p_us, mean_solutions                   rr_p3p alone on P x 1024 / 16 samples, and their mean number of solutions
  mean_inliers_localize / _essential, mean_planted, max_rot_deg, max_dir_deg (against the planted pose)
No time is fixed in advance.
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
    """kq, ka float32 [p, n, 2] (query = view 2, database = view 1), X float64 [p, n, 3], match int64 [p, n] (query
    row -> database row), planted bool [p, n], R [p, 3, 3], t [p, 3]"""
    import pose_cases as PC
    out = []
    for i in range(distinct):
        s = PC.scene(n, n, matched, 0.5, 0.3, seed + i)
        inv = np.full(n, -1, dtype=np.int64)
        rows = np.nonzero(s["match"] >= 0)[0]
        inv[s["match"][rows]] = rows
        planted = np.zeros(n, dtype=bool)
        planted[s["match"][rows[s["planted"][rows]]]] = True
        out.append((s["kp2"], s["kp1"], s["X"], inv, planted, s["R"], s["t"]))
    idx = np.arange(p) % distinct
    return tuple(np.stack([q[i] for q in out])[idx] for i in range(7))


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pnp_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pnp_probe needs a GPU")
    import epipolar_cases as EC
    import pose_cases as PC
    from cirtorch import _engine as E
    from cirtorch.geometry.pnp import solve_p3p
    from cirtorch.search import localize_pairs, verify_pairs
    from tools.src_digest import digest
    distinct = min(args.distinct, args.pairs)
    kq, ka, X, match, planted, Rt, tt = make_pairs(args.pairs, args.n, args.matched, distinct, 2700)
    dq, da, dX, dm = (torch.from_numpy(a).cuda() for a in (kq, ka, X, match))
    K = torch.from_numpy(EC.K).cuda()
    run = {"localize": lambda: localize_pairs(dq, dX, dm, K, th=3.0, iters=args.iters, refine=2, seed=1),
           "essential": lambda: verify_pairs(dq, da, dm, th=1.5, iters=args.iters, refine=2, seed=1, model="essential", K1=K, K2=K)}
    # the minimal solver alone: the first three kept rows of each pair, repeated
    ns = args.pairs * args.iters // 16
    rows = np.stack([np.nonzero(match[i] >= 0)[0][:3] for i in range(distinct)])
    h = np.concatenate([kq[np.arange(distinct)[:, None], rows].astype(np.float64), np.ones((distinct, 3, 1))], 2) @ np.linalg.inv(EC.K).T
    x3 = torch.from_numpy(np.ascontiguousarray(h[:, :, :2])[np.arange(ns) % distinct]).cuda()
    X3 = torch.from_numpy(X[np.arange(distinct)[:, None], match[np.arange(distinct)[:, None], rows]][np.arange(ns) % distinct]).cuda()
    run["p3p"] = lambda: solve_p3p(x3, X3)
    times = {m: [] for m in run}
    for r in range(args.warmup + args.reps):
        for m in run:
            t = once(run[m])
            if r >= args.warmup:
                times[m].append(t)
    li, R, t, _ = run["localize"]()
    ei = run["essential"]()[0]
    nsol = run["p3p"]()[2]
    Rn, tn = R[:distinct].cpu().numpy(), t[:distinct, :, 0].cpu().numpy()
    med = {m: statistics.median(times[m]) for m in run}
    out = {"pairs": args.pairs, "n": args.n, "matched": args.matched, "iters": args.iters, "distinct": distinct, "reps": args.reps,
           "build": E.lib().rr_build_info().decode(), "tree_digest": digest(), "device": E.device_arch()}
    for m in run:
        out[m + "_us"] = round(med[m], 1)
        out[m + "_us_min_max"] = [round(min(times[m]), 1), round(max(times[m]), 1)]
    out["localize_us_per_pair"] = round(med["localize"] / args.pairs, 3)
    out["essential_us_per_pair"] = round(med["essential"] / args.pairs, 3)
    out["ratio"] = round(med["localize"] / med["essential"], 3)
    out["p3p_samples"] = ns
    out["mean_solutions"] = round(float(nsol.float().mean().item()), 2)
    out["mean_inliers_localize"] = round(float(li.float().mean().item()), 1)
    out["mean_inliers_essential"] = round(float(ei.float().mean().item()), 1)
    out["mean_planted"] = round(float(planted.sum(1).mean()), 1)
    out["max_rot_deg"] = round(max(PC.rot_angle_deg(Rn[i], Rt[i]) for i in range(distinct)), 4)
    out["max_dir_deg"] = round(max(PC.dir_angle_deg(tn[i], tt[i]) for i in range(distinct)), 4)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
