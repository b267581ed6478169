"""Timing of the learned patch descriptors (rr_patchnet_trunk, rr_patchnet_head, rr_patchnet_describe and
cirtorch.search.describe_keypoints(descriptor=...)) on the README's local workload, 128 images x 2048
keypoints = 262 144 patches, beside the same network run by torch in fp16 on the device (the
reference's layer list, eval mode, channels_last) and beside the SIFT describer on the same frames.
    python tools/patchnet_probe.py [--reps 5] [--images 128] [--kpts 2048] [--hw 480 640] [--out profiles/patchnet_probe.json]
One patch is 39.1 M multiply-adds (78.2 MFLOP, counted from the layer shapes below), the workload
20.5 TFLOP; rates are that work over the median time.  HIP events around every call, warm-up first,
all variants interleaved in one process, median and min-max.  The trunk and the head are timed on the
patches of one chunk (RR_TUNE_PATCHNET_CHUNK) and scaled to the workload by the chunk count; the fused
call and describe_keypoints run the whole workload.  --clock-seconds of back-to-back fused calls come
first, and the shader clock the chip holds under that load is read from the sysfs node of the card
(pp_dpm_sclk, the starred level) while they run: an upper bound of the in-kernel clock.
Prints (and writes to --out) one JSON line.  Developer tool; A/B two builds with RR_LIB.
"""

import argparse
import glob
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

# (cout, cin, kernel, output side) of layers 1 .. 7
SHAPES = ((32, 1, 3, 32), (32, 32, 3, 32), (64, 32, 3, 16), (64, 64, 3, 16), (128, 64, 3, 8), (128, 128, 3, 8), (128, 128, 8, 1))
MACS = sum(co * ci * k * k * s * s for co, ci, k, s in SHAPES)   # 39,092,224 per patch


def once(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def sclk_mhz():
    """the active level of every card's pp_dpm_sclk, MHz (empty when the node cannot be read)"""
    out = []
    for path in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            for line in open(path):
                if line.rstrip().endswith("*"):
                    out.append(int(line.split(":")[1].strip().lower().replace("mhz", "").replace("*", "").strip()))
        except (OSError, ValueError, IndexError):
            pass
    return out


def torch_net(state, variant):
    """the reference's layer list in torch, fp16, channels_last: (module, input normalisation, output normalisation)"""
    import torch.nn as nn
    import torch.nn.functional as F
    layers = []
    for i, (co, ci, k, _) in enumerate(SHAPES):
        stride = 2 if i in (2, 4) else 1
        layers += [nn.Conv2d(ci, co, k, stride=stride, padding=1 if k == 3 else 0, bias=False), nn.BatchNorm2d(co, affine=False)]
        if i < 6:
            layers.append(nn.ReLU())
    net = nn.Sequential(*layers)
    w, m, v = state
    convs = [x for x in net if isinstance(x, nn.Conv2d)]
    bns = [x for x in net if isinstance(x, nn.BatchNorm2d)]
    for c, b, wi, mi, vi in zip(convs, bns, w, m, v):
        c.weight.data.copy_(torch.from_numpy(wi))
        b.running_mean.copy_(torch.from_numpy(mi))
        b.running_var.copy_(torch.from_numpy(vi))
    net = net.cuda().eval().half().to(memory_format=torch.channels_last)

    def run(x):   # x [B, 1, 32, 32] float32
        with torch.no_grad():
            if variant == "hardnet":
                sp, mp = torch.std_mean(x, dim=(-3, -2, -1), keepdim=True)
                xn = (x - mp) / (sp + 1e-6)
            else:
                xn = F.instance_norm(x)
            f = net(xn.half().contiguous(memory_format=torch.channels_last)).float().view(x.shape[0], 128)
            if variant == "hardnet":
                return F.normalize(f, dim=1)
            f = f + 1e-10
            return f / f.norm(dim=1, keepdim=True)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--kpts", type=int, default=2048)
    ap.add_argument("--hw", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--torch-batch", type=int, default=16384)
    ap.add_argument("--clock-seconds", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "patchnet_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("patchnet_probe needs a GPU")
    import time

    import patchnet_cases as NC
    from cirtorch import _engine as E, _ops
    from cirtorch.features import HardNet, SOSNet
    from cirtorch.search import describe_keypoints
    from tools.src_digest import digest
    n = args.images * args.kpts
    flop = 2.0 * MACS * n
    chunk = min(E.get_tuning("PATCHNET_CHUNK"), n)
    nchunks = -(-n // chunk)
    g = torch.Generator(device="cuda").manual_seed(5)
    patches = torch.rand((n, 32, 32), device="cuda", generator=g)
    h, w = args.hw
    images = torch.rand((args.images, 1, h, w), device="cuda", generator=g)
    kp = torch.stack([torch.rand((args.images, args.kpts), device="cuda", generator=g) * (w - 40) + 20,
                      torch.rand((args.images, args.kpts), device="cuda", generator=g) * (h - 40) + 20], dim=-1)
    nets = {}
    for variant, cls in (("hardnet", HardNet), ("sosnet", SOSNet)):
        params = NC.net_params(NC.SEEDS[variant])
        net = cls(False)
        net.load_state_dict({k: torch.from_numpy(np.asarray(a)) for k, a in NC.state_dict(variant, params).items()}, strict=True)
        nets[variant] = (net.cuda().eval(), torch_net(params, variant))
    hard, hard_torch = nets["hardnet"]
    sos = nets["sosnet"][0]
    packed = hard.packed()
    maps = _ops.patchnet_trunk(patches[:chunk], packed, "hardnet")
    out_buf = torch.empty((n, 128), device="cuda")
    tb = min(args.torch_batch, n)

    def torch_all():
        for b0 in range(0, n, tb):
            hard_torch(patches[b0:b0 + tb, None])

    run = {
        "trunk_chunk": lambda: _ops.patchnet_trunk(patches[:chunk], packed, "hardnet"),
        "head_chunk": lambda: _ops.patchnet_head(maps, packed, "hardnet"),
        "fused": lambda: _ops.patchnet_describe(patches, packed, "hardnet", out_buf),
        "fused_sosnet": lambda: _ops.patchnet_describe(patches, sos.packed(), "sosnet", out_buf),
        "torch_fp16": torch_all,
        "describe_sift": lambda: describe_keypoints(images, kp),
        "describe_hardnet": lambda: describe_keypoints(images, kp, descriptor=hard),
        "describe_sosnet": lambda: describe_keypoints(images, kp, descriptor=sos),
    }
    # the clock under load: back-to-back fused calls, the sysfs level sampled while they run
    clocks, t_end = [], time.time() + args.clock_seconds
    while time.time() < t_end:
        run["fused"]()
        clocks += sclk_mhz()[:1]
        torch.cuda.synchronize()
    times = {m: [] for m in run}
    for r in range(args.warmup + args.reps):
        for m in run:
            t = once(run[m])
            if r >= args.warmup:
                times[m].append(t)
    med = {m: statistics.median(times[m]) for m in run}
    got = _ops.patchnet_describe(patches[:4096], packed, "hardnet")
    ref = hard_torch(patches[:4096, None])
    out = {"patches": n, "chunk": chunk, "chunks": nchunks, "mflop_per_patch": round(2e-6 * MACS, 2), "tflop": round(flop / 1e12, 2),
           "reps": args.reps, "build": E.lib().rr_build_info().decode(), "tree_digest": digest(), "device": E.device_arch(),
           "sclk_mhz_under_load": [min(clocks), max(clocks)] if clocks else "not readable",
           "max_diff_vs_torch_fp16": float((got - ref).abs().max().item())}
    for m in run:
        out[m + "_ms"] = round(med[m], 3)
        out[m + "_ms_min_max"] = [round(min(times[m]), 3), round(max(times[m]), 3)]
    out["trunk_ms_workload"] = round(med["trunk_chunk"] * n / chunk, 2)
    out["head_ms_workload"] = round(med["head_chunk"] * n / chunk, 2)
    trunk_flop = 2.0 * (MACS - 128 * 128 * 64) * n
    out["trunk_tflops"] = round(trunk_flop / (med["trunk_chunk"] * n / chunk * 1e-3) / 1e12, 1)
    out["head_tflops"] = round((flop - trunk_flop) / (med["head_chunk"] * n / chunk * 1e-3) / 1e12, 1)
    out["fused_tflops"] = round(flop / (med["fused"] * 1e-3) / 1e12, 1)
    out["torch_fp16_tflops"] = round(flop / (med["torch_fp16"] * 1e-3) / 1e12, 1)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
