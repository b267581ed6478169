"""Timing of the regional pooling kernel (k_region_pool) at the bench's mod5 map:
128 x 2048 x 24 x 32 fp16, channels_last, GeM with the device-resident p = 3,
the 21 regions of the L = 3 grid.  HIP events around every call, warm-up, median.
    python tools/region_pool_probe.py [--reps 30] [--n 128]
Prints one JSON line:
  region_pool_us      rr_region_pool, all 21 regions in one launch
  global_pool_us      (a) rr_global_pool on the same map: the floor of reading the map once
  loop_pool_us        (b) 21 rr_global_pool calls on narrowed, contiguous copies made beforehand
  loop_copy_pool_us   (b) with the 21 narrowing copies timed as well
Developer tool; A/B two builds with RR_LIB.
"""

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image-retrieval-for-image-based-localization_amd"))

import torch  # noqa: E402


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(1000 * t0.elapsed_time(t1))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--hw", type=int, nargs=2, default=[24, 32])
    ap.add_argument("--c", type=int, default=2048)
    args = ap.parse_args()
    from cirtorch import _engine as E
    from cirtorch import _ops
    from cirtorch.layers.regions import roi_regions
    h, w = args.hw
    x = torch.rand(args.n, args.c, h, w, device="cuda", dtype=torch.float16).to(memory_format=torch.channels_last)
    p = torch.full((1,), 3.0, device="cuda")
    regs = roi_regions(h, w, 3)

    def narrowed():
        return [x[:, :, y0:y0 + rh, x0:x0 + rw].contiguous(memory_format=torch.channels_last)
                for (y0, x0, rh, rw) in regs]

    copies = narrowed()
    out = {"n": args.n, "c": args.c, "hw": [h, w], "regions": len(regs), "build": E.lib().rr_build_info().decode()}
    for key, fn in (("region_pool_us", lambda: _ops.region_pool(x, regs, E.RR_POOL_GEM, p)),
                    ("global_pool_us", lambda: _ops.global_pool(x, E.RR_POOL_GEM, p)),
                    ("loop_pool_us", lambda: [_ops.global_pool(v, E.RR_POOL_GEM, p) for v in copies]),
                    ("loop_copy_pool_us", lambda: [_ops.global_pool(v, E.RR_POOL_GEM, p) for v in narrowed()])):
        med, lo, hi = timed(fn, args.reps)
        out[key] = round(med, 2)
        out[key + "_min_max"] = [round(lo, 2), round(hi, 2)]
    a = _ops.region_pool(x, regs, E.RR_POOL_GEM, p)
    b = torch.stack([_ops.global_pool(v, E.RR_POOL_GEM, p) for v in copies], dim=1)
    out["max_rel_diff_vs_loop"] = float(((a - b).abs() / b.abs()).max())
    out["ratio_to_global"] = round(out["region_pool_us"] / out["global_pool_us"], 2)
    out["speedup_vs_loop"] = round(out["loop_pool_us"] / out["region_pool_us"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
