"""Timing of the batched local-descriptor matcher (rr_match_pairs) against the per-pair
path it complements (cirtorch.search.mutual_nn: two KnnIndex builds + two certified
top-1 searches per pair), at 2048 x 2048 x 128 unit descriptors.  One process, the
variants interleaved round by round, HIP events around every call, warm-up, median
and min-max.
    python tools/match_probe.py [--reps 30] [--n 2048] [--d 128] [--pairs 16]
Prints one JSON line (microseconds):
  mutual_nn_us         (a) mutual_nn(d0, d1), one pair
  match_mnn_p1_us      (b) match_pairs(mode="mnn"), P = 1
  mutual_nn_xP_us      16 sequential (a), one per pair
  match_mnn_pP_us      (c) match_pairs(mode="mnn"), P = 16 in one call
  match_smnn_pP_us     (d) match_pairs(mode="smnn"), P = 16 in one call
  *_min_max            the spread of each; mnn_equal: (b) == (a) on the probe's pair
  f64_mfma_tflops_pP   2 directions x 2 N^2 D flops x P / (c)
Developer tool; A/B two builds with RR_LIB.
"""

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image-retrieval-for-image-based-localization_amd"))
sys.path.insert(0, REPO)

import torch  # noqa: E402


def once(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return 1000 * t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=16)
    args = ap.parse_args()
    from cirtorch import _engine as E
    from cirtorch import _ops
    from cirtorch.search import match_pairs, mutual_nn
    from tools.src_digest import digest
    n, d, p = args.n, args.d, args.pairs
    d0 = _ops.fill_unit_rows(p * n, d, seed=11, device="cuda").view(p, n, d)
    noise = _ops.fill_unit_rows(p * n, d, seed=12, device="cuda").view(p, n, d)
    d1 = torch.nn.functional.normalize(d0.flip(1) + 0.3 * noise, dim=2).contiguous()   # true matches + noise

    variants = {
        "mutual_nn_us": lambda: mutual_nn(d0[0], d1[0]),
        "match_mnn_p1_us": lambda: match_pairs(d0[0], d1[0], mode="mnn"),
        "mutual_nn_xP_us": lambda: [mutual_nn(d0[i], d1[i]) for i in range(p)],
        "match_mnn_pP_us": lambda: match_pairs(d0, d1, mode="mnn"),
        "match_smnn_pP_us": lambda: match_pairs(d0, d1, mode="smnn", th=0.8),
    }
    times = {k: [] for k in variants}
    for r in range(args.warmup + args.reps):
        for k, fn in variants.items():   # interleaved: drift hits every variant alike
            t = once(fn)
            if r >= args.warmup:
                times[k].append(t)
    out = {"n": n, "d": d, "pairs": p, "reps": args.reps, "build": E.lib().rr_build_info().decode(),
           "tree_digest": digest(), "device": E.device_arch()}
    for k, v in times.items():
        out[k] = round(statistics.median(v), 1)
        out[k + "_min_max"] = [round(min(v), 1), round(max(v), 1)]
    out["mnn_equal"] = bool(torch.equal(mutual_nn(d0[0], d1[0]), match_pairs(d0[0], d1[0], mode="mnn")[0]))
    out["mutual_fraction"] = round(float((match_pairs(d0, d1, mode="mnn")[0] >= 0).float().mean()), 3)
    out["speedup_p1"] = round(out["mutual_nn_us"] / out["match_mnn_p1_us"], 2)
    out["speedup_pP"] = round(out["mutual_nn_xP_us"] / out["match_mnn_pP_us"], 2)
    out["f64_mfma_tflops_pP"] = round(2 * 2.0 * n * n * d * p / out["match_mnn_pP_us"] / 1e6, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
