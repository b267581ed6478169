#!/usr/bin/env python
"""Extract-and-match benchmark (BASELINE.json metric).

One step (per rank): extract B synthetic 3x768x1024 images with ResNet50-GeM
(+ whitening head) in fp16 on the MFMA engine (the precision that meets the
north-star descriptor bar; bf16, BASELINE config 2, is the e2e_bf16 sub-line),
all-gather the B x world query
descriptors, search them (top-100 cosine kNN, exact ordering) against a
1M x 2048 database sharded over the ranks (per-shard top-k -> RCCL all-gather
-> on-GPU merge).  Per-rank work is fixed as ranks grow (images per rank,
and queries x local rows per rank), so scaling is weak.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the K
steps and prints the headline (value, ms_per_step, the extractor roofline of
those steps).  --dump-outputs DIR writes what the last timed step returned
(descriptors.npy, knn_scores.npy, knn_indices.npy); the inputs are seeded, so
two builds can be compared output for output.  --full also measures (separate
loops, same process): the other 16-bit precision end to end, extract-only
images/s, PCIe-inclusive extraction, kNN-only queries/s at Q=1024 against the
1M DB, the collectives (N > 1), the local head, single-image latency, the
drop-in file path, every precision with its reference parity, configs 3/4/5,
and the CPU baseline (rank 0, N=1 only), which times the oracle restatement
of the reference path on a bounded sample (oracle/ is the checker, not the
product).
"""

import argparse
import json
import os
import platform
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(REPO, "image-retrieval-for-image-based-localization_amd")
for _p in (PKG, REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0   # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_I8_TOPS = 5000.0       # dense int8 MFMA: v_mfma_i32_16x16x64_i8 at 2x the bf16 rate per clock
PEAK_F32_TFLOPS = 157.3     # exact-f32 MFMA
PEAK_HBM_GBS = 8000.0
METRIC = "images/sec extract + queries/sec 1M-desc kNN, ResNet50-GeM 1024×768"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128, help="images (= queries) per rank per step")
    ap.add_argument("--extract-batch", type=int, default=128,
                    help="images per extractor launch chain (the step's batch runs as batch/extract-batch chains)")
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--arch", default="resnet50")
    ap.add_argument("--precision", default="fp16", choices=["bf16", "fp16", "fp32"],
                    help="headline precision: fp16 meets the north-star descriptor bar (cosine >= 1 - 1e-4 vs the "
                         "reference); bf16 (BASELINE config 2) runs as the e2e_bf16 sub-line")
    ap.add_argument("--screen", default="fp16", choices=["int8", "bf16", "fp16", "fp32"],
                    help="kNN screening copy of the database; every search is CERTIFIED (each query's screening "
                         "margin is checked against the dtype's error bound on the device, uncertified queries are "
                         "re-searched in float32) and the top-k is the exact float64 re-score.  fp16 (default): "
                         "the bound (~1e-3) certifies random 2048-d data; int8's residual bound (~0.02) does not, "
                         "so int8 is timed uncertified as the knn.int8_screen sub-line")
    ap.add_argument("--query-batch", type=int, default=1024,
                    help="queries per rank per search: the step's descriptors are searched in batches of this many "
                         "(the reference ranks all extracted queries in one np.dot, scripts/test.py:236-248); every "
                         "batch, the last one flushed, is searched inside the timed region.  0 = one search per step")
    ap.add_argument("--db-rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--knn-q", type=int, default=1024, help="queries for the kNN-only sub-benchmark (0 = skip)")
    ap.add_argument("--knn-steps", type=int, default=5)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--pcie-steps", type=int, default=4, help="PCIe-inclusive extract sub-benchmark steps (0 = skip)")
    ap.add_argument("--local-kpts", type=int, default=2048, help="keypoints per image for the local-head sub-benchmark (0 = skip)")
    ap.add_argument("--latency", type=int, default=1, help="single-image extract latency, eager vs HIP-graph replay (0 = skip)")
    ap.add_argument("--no-overlap", dest="overlap", action="store_false",
                    help="run each step's match on the extraction stream (default: on a second stream, overlapping "
                         "the next step's extraction; +0.8-1.5 %% on one GPU, DESIGN.md)")
    ap.add_argument("--search-cus", type=int, default=0,
                    help="cap the CUs the step's persistent search kernels spread over (RR_TUNE_GRID_CUS set "
                         "around the search launches only), leaving the rest to the overlapped extraction; 0 = all")
    ap.add_argument("--cpu-images", type=int, default=24,
                    help="images of the CPU baseline's extract sample (batch 1, as scripts/test.py)")
    ap.add_argument("--cpu-queries", type=int, default=64, help="queries of the CPU baseline's match sample")
    ap.add_argument("--cpu-db-rows", type=int, default=1_000_000,
                    help="rows of the CPU baseline's match sample (1M = the full headline DB, no extrapolation)")
    ap.add_argument("--no-extras", dest="extras", action="store_false",
                    help="skip the single-GPU extra lines (precisions + reference parity, configs 3/4/5)")
    ap.add_argument("--c3-batch", type=int, default=16, help="config 3: images per multi-scale R101 step")
    ap.add_argument("--c5-batch", type=int, default=64, help="config 5: images per R152 fp16 step")
    ap.add_argument("--c5-db-rows", type=int, default=10_000_000, help="config 5: fp16 database rows (0 = skip)")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="N > 1 process group: nccl (= RCCL over xGMI, the measured path) or gloo (host-copy "
                         "rehearsal of the same code path)")
    ap.add_argument("--one-device", action="store_true",
                    help="rehearsal on a 1-GPU box: every rank on cuda:0 (with --dist-backend gloo)")
    ap.add_argument("--extract-priority", type=int, default=int(os.environ.get("RR_BENCH_PRIO", "0")),
                    help="1: run the extraction on a high-priority stream (the overlapped search keeps the default)")
    ap.add_argument("--match-priority", type=int, default=int(os.environ.get("RR_BENCH_MPRIO", "0")),
                    help="1: run the overlapped search on a high-priority stream (its blocks go first when a CU frees)")
    ap.add_argument("--graph", type=int, default=int(os.environ.get("RR_BENCH_GRAPH", "1")),
                    help="1: each extractor chain is recorded once as a hipGraph (torch.cuda.CUDAGraph) reading the "
                         "resident images in place and replayed every step (all kernels still run); 0: eager launches")
    ap.add_argument("--tune", default="", help="developer A/B: rr_set_tuning pairs key=value[,key=value]")
    ap.add_argument("--alt-steps", "--fp16-steps", dest="alt_steps", type=int, default=10,
                    help="steps of the end-to-end line in the other 16-bit precision (e2e_bf16 beside an fp16 "
                         "headline, e2e_fp16 beside a bf16 one; 0 = skip)")
    ap.add_argument("--cpu-baseline-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--cpu-pin", default="", help=argparse.SUPPRESS)
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="CPU baseline threads (0: OMP_NUM_THREADS, else the usable CPUs), pinned one per physical "
                         "core of one socket")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run every sub-benchmark and check (other precisions, extract-only, "
                         "PCIe, kNN-only, collectives, local head, latency, configs 3/4/5 with reference parity, the "
                         "CPU baseline); without it only the headline steps run and those fields are null / absent")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps write what the last timed step returned as DIR/<name>.npy: its "
                         "descriptors (D x B float32) and the scores / indices of the last search (float64)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if not args.full:   # a plain run: set up, warm up, time the steps, print the line
        args.alt_steps = args.pcie_steps = args.knn_q = args.local_kpts = args.latency = 0
        args.extras, args.no_cpu_baseline = False, True
    return args


DUMP_BYTES_MAX = 64 << 20   # all of --dump-outputs together


def dump_outputs(path, arrays):
    """{name: tensor} -> path/<name>.npy (float32 stays float32, everything else float64).
    Arrays over their share of DUMP_BYTES_MAX are cut to a fixed, seeded sample of their
    leading-dimension slices (sorted, so the same slices in every run)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    share = DUMP_BYTES_MAX // max(1, len(arrays))
    for name, t in arrays.items():
        a = t.detach().cpu().numpy()
        a = np.ascontiguousarray(a, dtype=np.float32 if a.dtype == np.float32 else np.float64)
        if a.nbytes > share and a.ndim:
            per = max(1, a.nbytes // a.shape[0])
            keep = np.sort(np.random.default_rng(0xD0A7).choice(a.shape[0], max(1, share // per), replace=False))
            a = a[keep]
        np.save(os.path.join(path, name + ".npy"), a)


def conv_flops_per_image(body, h, w):
    """2 x MACs of every conv of the body at input h x w (algorithmic FLOPs)."""
    tot = 0
    hh, ww = h, w

    def out(s, k, st, p):
        return (s + 2 * p - k) // st + 1

    c = body.mod1.conv1
    hh, ww = out(hh, 7, 2, 3), out(ww, 7, 2, 3)
    tot += 2 * hh * ww * c.out_channels * c.in_channels * 49
    hh, ww = out(hh, 3, 2, 1), out(ww, 3, 2, 1)
    for m in range(2, 6):
        for blk in getattr(body, "mod%d" % m).children():
            convs = [blk.convs.conv1, blk.convs.conv2] + ([blk.convs.conv3] if blk.is_bottleneck else [])
            h0, w0 = hh, ww
            for cv in convs:
                k, st, p = cv.kernel_size[0], cv.stride[0], cv.padding[0]
                hh, ww = out(hh, k, st, p), out(ww, k, st, p)
                tot += 2 * hh * ww * cv.out_channels * cv.in_channels * k * k
            if hasattr(blk, "proj_conv"):
                cv = blk.proj_conv
                tot += 2 * out(h0, 1, cv.stride[0], 0) * out(w0, 1, cv.stride[0], 0) * cv.out_channels * cv.in_channels
    return tot


def layer_costs(body, h, w, esz=2):
    """Per-layer algorithmic (FLOPs, HBM bytes) of one image through the body:
    each conv reads its input map and (conv3) the residual once and writes its
    output once (esz bytes per activation); the fused stem reads the float32
    image and writes the pooled map.  Used for the layer-resolved roofline
    floor sum_l max(flops_l / peak_mfma, bytes_l / peak_hbm)."""
    def out(s, k, st, p):
        return (s + 2 * p - k) // st + 1
    costs = []
    c = body.mod1.conv1
    hh, ww = out(h, 7, 2, 3), out(w, 7, 2, 3)
    hp, wp = out(hh, 3, 2, 1), out(ww, 3, 2, 1)
    costs.append((2 * hh * ww * c.out_channels * c.in_channels * 49, h * w * 3 * 4 + hp * wp * 64 * esz))
    hh, ww = hp, wp
    for m in range(2, 6):
        for blk in getattr(body, "mod%d" % m).children():
            convs = [blk.convs.conv1, blk.convs.conv2] + ([blk.convs.conv3] if blk.is_bottleneck else [])
            h0, w0, c0 = hh, ww, convs[0].in_channels
            for i, cv in enumerate(convs):
                k, st, p = cv.kernel_size[0], cv.stride[0], cv.padding[0]
                hi, wi = hh, ww
                hh, ww = out(hh, k, st, p), out(ww, k, st, p)
                nout = hh * ww * cv.out_channels * esz
                res = nout if i == len(convs) - 1 else 0
                costs.append((2 * hh * ww * cv.out_channels * cv.in_channels * k * k,
                              hi * wi * cv.in_channels * esz + nout + res))
            if hasattr(blk, "proj_conv"):
                cv = blk.proj_conv
                ho, wo = out(h0, 1, cv.stride[0], 0), out(w0, 1, cv.stride[0], 0)
                costs.append((2 * ho * wo * cv.out_channels * cv.in_channels,
                              ho * wo * c0 * esz + ho * wo * cv.out_channels * esz))
    return costs


def cpu_baseline(args):
    """Oracle restatement of the reference CPU path, timed on this host in a child
    process (no GPU in it) pinned before start-up to one CPU per physical core."""
    import subprocess
    threads = args.cpu_threads or int(os.environ.get("OMP_NUM_THREADS", 0)) or len(os.sched_getaffinity(0))
    cores = pick_physical_cores(threads)
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-child",
           "--cpu-pin", ",".join(str(c) for c in cores), "--cpu-threads", str(len(cores) or threads),
           "--cpu-images", str(args.cpu_images), "--cpu-queries", str(args.cpu_queries),
           "--cpu-db-rows", str(args.cpu_db_rows), "--db-rows", str(args.db_rows), "--dim", str(args.dim),
           "--height", str(args.height), "--width", str(args.width), "--arch", args.arch]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1800)
    if r.returncode != 0:
        raise RuntimeError("cpu baseline child failed (rc %d): %s" % (r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def cpu_baseline_child(args):
    """the timed CPU run (see cpu_baseline); pinned first, before torch's thread pool exists"""
    cores = [int(c) for c in args.cpu_pin.split(",") if c] if args.cpu_pin else []
    if cores:
        try:
            os.sched_setaffinity(0, cores)
        except OSError:
            cores = []
    import numpy as np
    from oracle import backbone as obb, data, weights

    threads = args.cpu_threads
    torch.set_num_threads(threads)
    net = obb.OracleNet(args.arch, weights.backbone_state(args.arch), weights.head_state(weights.OUTPUT_DIM[args.arch]))
    imgs = torch.from_numpy(data.images(args.cpu_images, args.height, args.width))
    with torch.no_grad():
        net.forward_padded(imgs[:1])  # warm
        t0 = time.perf_counter()
        for i in range(args.cpu_images):
            net.forward_padded(imgs[i:i + 1])     # reference test batch size is 1 (base.ini:143)
        t_ext = (time.perf_counter() - t0) / args.cpu_images
    db = data.database(args.cpu_db_rows, args.dim)
    q = data.queries(args.cpu_queries, args.dim)
    t0 = time.perf_counter()
    scores = np.dot(db, q.T)                      # scripts/test.py:247
    ranks = np.argsort(-scores, axis=0)           # scripts/test.py:248
    t_match = (time.perf_counter() - t0) / q.shape[0] * (args.db_rows / args.cpu_db_rows)
    del ranks, scores, db
    per_img = t_ext + t_match
    model, sockets = host_cpu()
    per_socket = socket_cores()
    scaled = "" if args.cpu_db_rows == args.db_rows else ", scaled x%.0f to %d rows" % (
        args.db_rows / args.cpu_db_rows, args.db_rows)
    return {"value": 1.0 / per_img, "unit": "images/s", "cores": threads, "kind": "port",
            "host_cpu": model, "sockets": sockets, "logical_cpus": os.cpu_count(),
            "physical_cores_per_socket": per_socket, "pinned_cpus": cores,
            "extract_s_per_image": t_ext, "match_s_per_query": t_match,
            "sample": ("oracle restatement (torch-CPU conv/BN/leaky + GeM/L2N/whiten) of %d x 3x%dx%d images "
                       "at batch 1 (%.3f s/img) + the reference match np.dot + np.argsort(-scores, axis=0) of %d "
                       "queries against a %d x %d float32 DB%s (%.3f s/query); host %s, %d socket(s) of %s physical "
                       "cores; %d threads used, pinned one per physical core of socket 0 (%s) -- the GPU box's CPU "
                       "share per GPU is 16 (OMP_NUM_THREADS), so a full socket is not available to this run"
                       % (args.cpu_images, args.height, args.width, t_ext, args.cpu_queries, args.cpu_db_rows, args.dim,
                          scaled, t_match, model, sockets, per_socket, threads,
                          "pinned" if cores else "not pinned: affinity unavailable"))}


def _cpu_topology():
    """{cpu: (socket, core)} of the CPUs this process may run on (sysfs)"""
    topo = {}
    for cpu in sorted(os.sched_getaffinity(0)):
        base = "/sys/devices/system/cpu/cpu%d/topology/" % cpu
        try:
            topo[cpu] = (int(open(base + "physical_package_id").read()), int(open(base + "core_id").read()))
        except (OSError, ValueError):
            return {}
    return topo


def socket_cores():
    """physical cores per socket of this host (all CPUs, not only the usable ones)"""
    cores = set()
    try:
        for d in os.listdir("/sys/devices/system/cpu"):
            if d.startswith("cpu") and d[3:].isdigit():
                base = "/sys/devices/system/cpu/%s/topology/" % d
                cores.add((int(open(base + "physical_package_id").read()), int(open(base + "core_id").read())))
    except (OSError, ValueError):
        return None
    socks = {s for s, _ in cores}
    return len(cores) // max(1, len(socks)) if cores else None


def pick_physical_cores(n):
    """n usable CPUs on distinct physical cores (no SMT siblings), from the socket with
    the most usable cores first; [] if the topology is unavailable"""
    topo = _cpu_topology()
    if not topo:
        return []
    by_sock = {}
    for cpu, (sk, core) in topo.items():
        by_sock.setdefault(sk, {}).setdefault(core, cpu)
    picked = []
    for sk in sorted(by_sock, key=lambda k: -len(by_sock[k])):
        picked += sorted(by_sock[sk].values())
        if len(picked) >= n:
            break
    return picked[:n]


def host_cpu():
    """(model name, socket count) of this host from /proc/cpuinfo (lscpu's sources)."""
    model, phys = platform.processor() or "cpu", set()
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name") and model in ("cpu", "x86_64", ""):
                model = line.split(":", 1)[1].strip()
            elif line.startswith("physical id"):
                phys.add(line.split(":", 1)[1].strip())
    except OSError:
        pass
    return model, max(1, len(phys))



def kernel_source_digest():
    """sha1 (12 hex) of the HIP sources of librr.so (csrc/*.hip, *.h, include/rr.h): a PMC
    traffic file is attached to the roofline only if it was collected on these sources."""
    import glob
    import hashlib
    h = hashlib.sha1()
    files = sorted(glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.h"))) + \
        [os.path.join(REPO, "include", "rr.h")]
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:12]


def build_provenance():
    """which sources the loaded librr.so was built from (rr_build_info) vs the tree it runs in"""
    from cirtorch import _engine as E
    info = E.lib().rr_build_info().decode()
    built = dict(kv.split("=", 1) for kv in info.split())
    tree = kernel_source_digest()
    return {"library": os.path.relpath(E.LIB_PATH, REPO), "library_source_digest": built.get("source_digest"),
            "tree_source_digest": tree, "match": built.get("source_digest") == tree}


def pmc_file(kind, match):
    """newest profiles/r*_pmc_<kind>.json whose config satisfies match(config) ->
    (data, path, fresh): fresh = collected on the current kernel sources"""
    import glob
    digest = kernel_source_digest()
    best = None
    for path in sorted(glob.glob(os.path.join(REPO, "profiles", "r*_pmc_%s.json" % kind)), reverse=True):
        try:
            d = json.load(open(path))
        except (OSError, ValueError):
            continue
        c = d.get("config", {})
        if not match(c):
            continue
        fresh = c.get("source_digest") == digest
        if fresh:
            return d, path, True
        best = best or (d, path, False)
    return best if best else (None, None, False)


GOLDEN = os.path.join(REPO, "tests", "golden")
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
PEAK = {"bf16": PEAK_BF16_TFLOPS, "fp16": PEAK_BF16_TFLOPS, "fp32": PEAK_F32_TFLOPS}


def _cos_min(a, b):
    import numpy as np
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(((a * b).sum(0) / (np.linalg.norm(a, axis=0) * np.linalg.norm(b, axis=0))).min())


def reference_parity(arch, precision, fname, scales, dev):
    """Min descriptor cosine of the engine (this precision, normalisation fused
    in the stem) against the REFERENCE output stored in a committed fixture
    (tests/golden/<fname>, produced by the reference modules on the same
    synthetic parameters and images; cirtorch.utils.synthetic redraws them)."""
    import numpy as np
    from cirtorch.models.GF_net import make_net
    from cirtorch.utils import synthetic
    g = np.load(os.path.join(GOLDEN, fname), allow_pickle=False)
    net = make_net(arch, precision=precision, mean=MEAN, std=STD)
    synthetic.load_into(net, arch, head_bias=g["head_bias"])
    net = net.to(dev).eval()
    imgs = synthetic.structured_images(int(g["n"]), int(g["res"][0]), int(g["res"][1]), seed=int(g["seed"]))
    got = net.extract(torch.from_numpy(imgs).to(dev), scales=scales).cpu().numpy()
    key = "desc_s" + "_".join("%g" % s for s in scales)
    return _cos_min(got, g[key])


def time_extract(net, x, steps, scales=(1,)):
    """ms per net.extract(x) on the current stream (HIP events), after one warm call."""
    net.extract(x, scales=scales)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        net.extract(x, scales=scales)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def bench_precisions(args, images, dev):
    """R50 extract at every engine precision on the headline images, each with
    its roofline against its own MFMA peak and its descriptor cosine against
    the reference fixture (north_star bar: >= 1 - 1e-4)."""
    from cirtorch.models.GF_net import make_net
    from cirtorch.models.init import random_init_
    out = {}
    B, H, W = images.shape[0], images.shape[2], images.shape[3]
    for prec in ("bf16", "fp16", "fp32"):
        net = make_net("resnet50", precision=prec, mean=MEAN, std=STD)
        random_init_(net, seed=0)
        net = net.to(dev).eval()
        fl = conv_flops_per_image(net.body, H, W)
        ms = time_extract(net, images, 5 if prec != "fp32" else 2)
        tf = fl * B / (ms * 1e-3) / 1e12
        out[prec] = {"images_per_sec": B / (ms * 1e-3), "ms_per_batch": ms, "batch": B,
                     "roofline": {"bound": "mfma", "achieved": tf, "peak": PEAK[prec], "unit": "TFLOP/s",
                                  "frac": tf / PEAK[prec]},
                     "cos_vs_reference": reference_parity("resnet50", prec, "r50.npz", (1,), dev),
                     "meets_north_star_bar": None}
        out[prec]["meets_north_star_bar"] = out[prec]["cos_vs_reference"] >= 1 - 1e-4
        del net
        torch.cuda.empty_cache()
    out["note"] = ("R50-GeM+whiten extract of the headline's %d x 3x%dx%d images (whole forward incl. head, HIP "
                   "events); cos_vs_reference = min descriptor cosine vs tests/golden/r50.npz (reference modules, "
                   "2 images at 768x1024, same synthetic weights); roofline = 128.12 GFLOP/img of the convs over "
                   "the forward time vs the dtype's dense MFMA peak" % (B, H, W))
    return out


def bench_config3(args, images, dev, prec):
    """BASELINE config 3: R101-GeM multi-scale (x0.5 / 1 / 2 of 3x768x1024,
    GF_net.py:20-40,74-92) — the kNN half (1M DB sharded over the ranks, RCCL
    top-k all-gather) is the headline's match."""
    from cirtorch.models.GF_net import make_net
    from cirtorch.models.init import random_init_
    net = make_net("resnet101", precision=prec, mean=MEAN, std=STD)
    random_init_(net, seed=0)
    net = net.to(dev).eval()
    B, H, W = args.c3_batch, images.shape[2], images.shape[3]
    scales = (0.5, 1, 2)
    fl = sum(conv_flops_per_image(net.body, int(H * s), int(W * s)) for s in scales)
    ms = time_extract(net, images[:B], 3, scales)
    tf = fl * B / (ms * 1e-3) / 1e12
    del net
    torch.cuda.empty_cache()
    cos3 = reference_parity("resnet101", prec, "r101ms.npz", scales, dev)
    return {"images_per_sec": B / (ms * 1e-3), "batch": B, "scales": list(scales), "dtype": prec,
            "gflop_per_image": fl / 1e9, "ms_per_batch": ms,
            "roofline": {"bound": "mfma", "achieved": tf, "peak": PEAK[prec], "unit": "TFLOP/s", "frac": tf / PEAK[prec]},
            "cos_vs_reference": cos3, "meets_north_star_bar": bool(cos3 >= 1 - 1e-4),
            "note": "R101-GeM+whiten, per step B images through the 3-level pyramid (one batched bilinear resize "
                    "per level, one extractor chain per level, scale mean); cos vs tests/golden/r101ms.npz (reference "
                    "run, 1 image 768x1024 at scales 0.5/1/2); kNN part = the headline 1M-row sharded search"}


def bench_config5(args, images, dev):
    """BASELINE config 5: R152 fp16 extract + the local head on its mod3 map,
    and a 10M x 2048 fp16-screened database searched by 1024 queries."""
    from cirtorch import _ops
    from cirtorch.models.GF_net import make_net
    from cirtorch.models.init import random_init_
    from cirtorch.search import KnnIndex
    net = make_net("resnet152", precision="fp16", mean=MEAN, std=STD)
    random_init_(net, seed=0)
    net = net.to(dev).eval()
    B, H, W = args.c5_batch, images.shape[2], images.shape[3]
    fl = conv_flops_per_image(net.body, H, W)
    ms = time_extract(net, images[:B], 3)
    tf = fl * B / (ms * 1e-3) / 1e12
    out = {"extract": {"images_per_sec": B / (ms * 1e-3), "batch": B, "dtype": "fp16", "gflop_per_image": fl / 1e9,
                       "ms_per_batch": ms,
                       "roofline": {"bound": "mfma", "achieved": tf, "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                                    "frac": tf / PEAK_BF16_TFLOPS},
                       "cos_vs_reference": reference_parity("resnet152", "fp16", "r152.npz", (1,), dev)}}
    out["extract"]["meets_north_star_bar"] = bool(out["extract"]["cos_vs_reference"] >= 1 - 1e-4)
    # local head (local_head.py:19-71) on the R152 mod3 map of 8 images, 2048 keypoints each
    with torch.no_grad():
        m3 = net.body(images[:8], normalize=(MEAN, STD))["mod3"]
    g = torch.Generator(device=dev).manual_seed(55)
    kp = torch.rand((8, 2048, 2), generator=g, device=dev) * 2 - 1
    wl = torch.randn((128, m3.shape[1]), generator=g, device=dev) * m3.shape[1] ** -0.5
    bl = torch.zeros(128, device=dev)
    _ops.local_head(m3, kp, wl, bl)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        _ops.local_head(m3, kp, wl, bl)
    e1.record()
    torch.cuda.synchronize()
    t = e0.elapsed_time(e1) / 10
    out["local_head"] = {"keypoints_per_sec": 8 * 2048 / (t * 1e-3), "map": list(m3.shape), "ms_per_batch": t}
    del net, m3
    torch.cuda.empty_cache()
    if args.c5_db_rows > 0:
        n, d, q, k = args.c5_db_rows, args.dim, 1024, args.k
        db = _ops.fill_unit_rows(n, d, seed=0x10D5EED, device=dev)
        index = KnnIndex(db, "fp16")
        qq = _ops.fill_unit_rows(q, d, seed=0x10E5EED, device=dev)
        index.search(qq, k, verify="deferred")[2].resolve()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pends = [index.search(qq, k, verify="deferred")[2] for _ in range(3)]
        nre = sum(p_.resolve() for p_ in pends)
        torch.cuda.synchronize()
        t = (time.perf_counter() - t0) / 3
        flops = 2.0 * q * n * d
        out["knn"] = {"queries_per_sec": q / t, "q": q, "db_rows": n, "k": k, "ms_per_batch": t * 1e3,
                      "screen_dtype": "fp16", "certified": True, "requeried": nre,
                      "roofline": {"bound": "mfma", "achieved": flops / t / 1e12, "peak": PEAK_BF16_TFLOPS,
                                   "unit": "TFLOP/s", "frac": flops / t / 1e12 / PEAK_BF16_TFLOPS,
                                   "hbm_gbs_fp16_db_scan": n * d * 2 / t / 1e9},
                      "note": "10M x 2048 float32 rows + fp16 screening copy resident on one GPU (123 GB); fp16 "
                              "score GEMM + running-threshold select + exact float64 re-score, every query's "
                              "screening margin certified (requeried: re-searched in float32, timed)"}
        del index, db, qq
        torch.cuda.empty_cache()
    return out


def bench_config4(args, images, dev):
    """BASELINE config 4 end to end: 4993 DB + 70 query images (3x768x1024,
    R50-GeM + head whitening, fp16), post-hoc Lw applied on the GPU in float64
    (whitenapply), full ranks (np.argsort equivalent), revisited E/M/H mAP
    (scripts/test.py:236-259).  whitenlearn (host, once per model) is outside
    the timed region, as in the reference driver where it precedes the
    datasets (scripts/test.py:205)."""
    import numpy as np
    from cirtorch.models.GF_net import make_net
    from cirtorch.models.init import random_init_
    from cirtorch.search import rank
    from cirtorch.utils.evaluation.ParisOxfordEval import compute_map_and_print
    from cirtorch.utils.whiten import whitenapply, whitenlearn
    ndb, nq, B = 4993, 70, min(128, images.shape[0])
    net = make_net("resnet50", precision="fp16", mean=MEAN, std=STD)
    random_init_(net, seed=0)
    net = net.to(dev).eval()
    net.extract(images[:B])
    r = np.random.default_rng(45)
    qidx = r.integers(0, ndb, 3000)
    pidx = (qidx + r.integers(1, 7, 3000)) % ndb
    gnd = []
    for _ in range(nq):
        perm = r.permutation(ndb)
        gnd.append({"easy": perm[:20], "hard": perm[20:35], "junk": perm[35:40]})
    # structured images (a random colour field upsampled + noise): distinct
    # descriptors, so the learned whitening is well conditioned
    # pre-generated before the timed region (47 GB of float32 images in HBM)
    gen = torch.Generator(device=dev).manual_seed(46)
    chunks = []
    for c0 in range(0, ndb + nq, B):
        nb = min(B, ndb + nq - c0)
        field = torch.rand((nb, 3, 6, 8), generator=gen, device=dev)
        chunks.append(0.8 * torch.nn.functional.interpolate(field, size=tuple(images.shape[2:]), mode="bilinear",
                                                            align_corners=True)
                      + 0.2 * torch.rand((nb, 3) + tuple(images.shape[2:]), generator=gen, device=dev))
    vecs = torch.empty((2048, ndb + nq), device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for ci, c0 in enumerate(range(0, ndb + nq, B)):
        vecs[:, c0:c0 + chunks[ci].shape[0]] = net.extract(chunks[ci])
    torch.cuda.synchronize()
    t_ext = time.perf_counter() - t0
    dv, qv = vecs[:, :ndb], vecs[:, ndb:]
    m, P = whitenlearn(dv.double().cpu().numpy(), qidx, pidx)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    dw, qw = whitenapply(dv, m, P), whitenapply(qv, m, P)
    ranks = rank(dw, qw)
    score = compute_map_and_print("roxford5k", ranks, gnd, lambda *a: None)
    torch.cuda.synchronize()
    t_rest = time.perf_counter() - t1
    del net, vecs, chunks
    torch.cuda.empty_cache()
    return {"images": ndb + nq, "extract_s": t_ext, "whiten_rank_map_s": t_rest, "dataset_s": t_ext + t_rest,
            "images_per_sec": (ndb + nq) / t_ext, "mAP": score["mAP"],
            "note": "roxford-shaped synthetic dataset (structured random images, random gnd; mAP value is not meaningful, its "
                    "parity is tested in tests/test_gpu_configs.py); extract in 128-image chains, Lw (float64 "
                    "f64-MFMA whitenapply), full GPU ranks 4993 x 70, vectorised E/M/H mAP"}


def decode_workers():
    """host decode threads: the CPUs this process may run on, capped at 16 (the GPU box's
    CPU share per GPU; nproc there reports the whole machine)"""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    return max(1, min(16, n))


def bench_dropin(net, H, W, dev, n_files=128, distinct=16):
    """The drop-in path scripts/test.py calls (extract_vectors, :236-238) on
    n_files same-size image files: PNG (compress_level 1) and JPEG (quality 90,
    the reference datasets' format, cirtorch/datasets/globalFeatures/misc.py:17-30);
    PIL decode on the host's decode threads + batched uint8 chains, vs the same
    images already decoded."""
    import shutil
    import tempfile
    import numpy as np
    from PIL import Image
    from cirtorch.models.GF_net import extract_vectors, _decode
    workers = decode_workers()
    d = tempfile.mkdtemp(prefix="rr_dropin_")
    try:
        r = np.random.default_rng(3)
        paths = {"png": [], "jpg": []}
        for i in range(distinct):
            field = r.random((6, 8, 3))
            up = np.kron(field, np.ones((H // 6 + 1, W // 8 + 1, 1)))[:H, :W]
            arr = (np.clip(0.8 * up + 0.2 * r.random((H, W, 3)), 0, 1) * 255).astype(np.uint8)
            p = os.path.join(d, "im%02d.png" % i)
            Image.fromarray(arr).save(p, compress_level=1)
            paths["png"].append(p)
            p = os.path.join(d, "im%02d.jpg" % i)
            Image.fromarray(arr).save(p, quality=90)
            paths["jpg"].append(p)
        out = {}
        for fmt in ("png", "jpg"):
            ps = [paths[fmt][i % distinct] for i in range(n_files)]
            extract_vectors(net, ps, None, workers=workers)  # warm: the pinned host blocks stay cached
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v = extract_vectors(net, ps, None, workers=workers)
            out["%s_files_images_per_sec" % fmt] = n_files / (time.perf_counter() - t0)
            t0 = time.perf_counter()
            for p in ps[:32]:
                _decode(p, None, None, None, None)
            out["%s_decode_ms_per_image_one_thread" % fmt] = (time.perf_counter() - t0) / 32 * 1e3
            if fmt == "jpg":
                one = extract_vectors(net, ps[:1], None, workers=1)   # batch-1 result of the same file
                out["jpg_equals_batch1"] = bool(torch.equal(v[:, :1], one))
                dec = [_decode(p, None, None, None, None) for p in ps]
        extract_vectors(net, dec, None)  # warm: the pinned staging buffers of full chains stay allocated
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        extract_vectors(net, dec, None)
        t_dec = time.perf_counter() - t0
    finally:
        shutil.rmtree(d, ignore_errors=True)
    out.update({"decoded_uint8_images_per_sec": n_files / t_dec, "files": n_files, "image": [3, H, W],
                "decode_threads": workers,
                "note": "extract_vectors (upstream scripts/test.py entry point) on %d same-size %dx%d PNG / JPEG "
                        "files: %d decode threads running up to 256 files ahead, decoded straight into pinned HWC "
                        "uint8, same-size chains of 64 copied on a copy stream and transposed on the GPU (steady "
                        "state: a warm-up call of the same size first); decoded = the same images passed as uint8 "
                        "tensors (GPU-side rate incl. H2D and the D2H of the result)" % (n_files, W, H, workers)})
    return out


def main():
    args = parse()
    if args.cpu_baseline_child:      # the CPU baseline's own process: no GPU here
        print(json.dumps(cpu_baseline_child(args)))
        return
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = 0 if args.one_device else int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        import datetime
        try:
            if args.dist_backend == "nccl":   # RCCL over xGMI
                dist.init_process_group("nccl", device_id=dev, timeout=datetime.timedelta(minutes=10))
            else:
                dist.init_process_group("gloo", timeout=datetime.timedelta(minutes=10))
            dist.barrier()                    # the communicator is really up before anything is timed
        except Exception as e:                # noqa: BLE001 -- any init failure ends the run, loudly
            print("bench.py: rank %d/%d: %s process-group init failed: %s: %s"
                  % (rank, world, args.dist_backend, type(e).__name__, e), file=sys.stderr, flush=True)
            sys.exit(3)

    def max_over_ranks(x):
        """max of a host float over the ranks (RCCL: a device tensor; gloo: a host one)"""
        if world == 1:
            return x
        t = torch.tensor([x], device=dev if args.dist_backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    from cirtorch import _ops
    from cirtorch import _engine as E
    from cirtorch.models.GF_net import make_net
    from cirtorch.models.init import random_init_
    from cirtorch.search import ShardedIndex, all_gather_stacked
    for kv in filter(None, args.tune.split(",")):
        k_, v_ = kv.split("=")
        E.check(E.lib().rr_set_tuning(int(k_), int(v_)), "rr_set_tuning")

    net = make_net(args.arch, precision=args.precision, mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
    random_init_(net, seed=0)
    net = net.to(dev).eval()
    B, H, W = args.batch, args.height, args.width
    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    images = torch.rand((B, 3, H, W), generator=g, device=dev)

    per = (args.db_rows + world - 1) // world
    r0 = rank * per
    n_local = max(0, min(per, args.db_rows - r0))
    db32 = _ops.fill_unit_rows(n_local, args.dim, seed=0xDB5EED, row0=r0, device=dev)
    index = ShardedIndex(db32, r0, precision=args.screen)

    ev_pairs = []

    if args.extract_priority:
        # extraction on a high-priority stream: the overlapped search (default
        # priority) fills the extractor's gaps instead of competing with it
        torch.cuda.set_stream(torch.cuda.Stream(dev, priority=-1))
    main_stream = torch.cuda.current_stream(dev)
    match_stream = (torch.cuda.Stream(dev, priority=-1 if args.match_priority else 0) if args.overlap
                    else main_stream)

    state = {"net": net, "index": index}

    def match(desc):
        """the certified search of a batch of this rank's queries (D x n) and, for N > 1, every
        other rank's: (scores, idx, pending certificate)"""
        q = desc.t().contiguous()
        if world > 1:
            q = all_gather_stacked(q).reshape(world * q.shape[0], q.shape[1])
        if args.search_cus <= 0:
            return state["index"].search(q, args.k, verify="deferred")
        # the cap is read when a kernel is launched: only the search's launches see it
        from cirtorch import _engine as E
        E.check(E.lib().rr_set_tuning(7, args.search_cus), "rr_set_tuning")
        try:
            return state["index"].search(q, args.k, verify="deferred")
        finally:
            E.lib().rr_set_tuning(7, 0)

    def resolve(res):
        """read step i's certificate (once step i+1's work is queued) and re-search its
        uncertified queries on the search stream; -> how many there were"""
        with torch.cuda.stream(match_stream):
            return res[2].resolve()

    QB = 0 if args.query_batch <= 0 else max(B, args.query_batch // B * B)  # queries per rank per search
    queued = []   # this rank's extracted, not yet searched descriptors (D x B each)
    last = {}     # what the latest step returned: its descriptors, the latest search's (scores, idx)

    def search_queued():
        """launch the certified search of the queued descriptors on the search stream"""
        desc = queued[0] if len(queued) == 1 else torch.cat(queued, dim=1)
        queued.clear()
        if match_stream is main_stream:
            return match(desc)
        ready = torch.cuda.Event()
        ready.record(main_stream)
        with torch.cuda.stream(match_stream):
            match_stream.wait_event(ready)
            desc.record_stream(match_stream)
            return match(desc)

    def run_steps(n, record):
        """n steps; a search is launched whenever QB queries are queued (every step with
        --query-batch 0) and the rest are flushed at the end; each search's certificate is
        resolved after the next search is queued, the last one before returning (inside
        the caller's timed region) -> (re-searched queries, searches)"""
        prev, requeried, searches = None, 0, 0
        for i in range(n):
            queued.append(extract_all(record))
            last["descriptors"] = queued[-1]
            if QB == 0 or len(queued) * B >= QB or i == n - 1:
                res = search_queued()
                searches += 1
                if prev is not None:
                    requeried += resolve(prev)
                prev = res
        if prev is not None:
            requeried += resolve(prev)
            last["knn_scores"], last["knn_indices"] = prev[0], prev[1]
        return requeried, searches

    EB = max(1, min(args.extract_batch, B))

    graphs = {}  # (id(net), chain) -> (hipGraph, its static output)

    def run_chain(c):
        """one extractor chain; --graph: replay of its recorded launches (the first call runs
        eagerly once -- weight packing, workspaces -- then records)"""
        x = images[c:c + EB]
        if not args.graph:
            return state["net"].extract(x)
        key = (id(state["net"]), c)
        if key not in graphs:
            state["net"].extract(x)
            torch.cuda.synchronize()
            try:
                g = torch.cuda.CUDAGraph()
                # thread_local: only this thread's calls are checked during the capture (RCCL's
                # proxy threads may touch the device meanwhile on N > 1)
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    out = state["net"].extract(x)
            except RuntimeError as e:  # capture refused: run eager from here on, and say so
                print("bench: hipGraph capture failed (%s); extracting with eager launches" % e, file=sys.stderr)
                args.graph = 0
                torch.cuda.synchronize()
                return state["net"].extract(x)
            graphs[key] = (g, out)
        g, out = graphs[key]
        g.replay()
        return out.clone()  # the static output is overwritten by the next replay

    def extract_all(record):
        """the step's B images as B/EB extractor chains -> D x B descriptors"""
        descs = []
        for c in range(0, B, EB):
            if record:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(main_stream)
            descs.append(run_chain(c))
            if record:
                e1.record(main_stream)
                ev_pairs.append((e0, e1))
        return descs[0] if len(descs) == 1 else torch.cat(descs, dim=1)

    with torch.no_grad():
        run_steps(args.warmup, False)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        step_requeried, step_searches = run_steps(args.steps, True)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        elapsed = max_over_ranks(time.perf_counter() - t0)
        body_ms = sum(a.elapsed_time(b) for a, b in ev_pairs) / args.steps   # extractor time per step
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, last)

        # the same step in the other 16-bit precision (bf16 = BASELINE config 2 beside
        # the fp16 headline, which meets the north_star descriptor bar)
        e2e_alt, alt = None, {"fp16": "bf16", "bf16": "fp16"}.get(args.precision)
        if args.alt_steps > 0 and alt is not None:
            net_a = make_net(args.arch, precision=alt, mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
            random_init_(net_a, seed=0)
            net_a = net_a.to(dev).eval()
            index_a = ShardedIndex(db32, r0, precision=args.screen)
            saved = (state["net"], state["index"])
            state["net"], state["index"] = net_a, index_a
            run_steps(max(2, args.warmup), False)
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            ta = time.perf_counter()
            alt_requeried, _ = run_steps(args.alt_steps, False)
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            el_a = max_over_ranks(time.perf_counter() - ta)
            state["net"], state["index"] = saved
            for key in [k_ for k_ in graphs if k_[0] == id(net_a)]:
                del graphs[key]
            e2e_alt = {"value": world * B * args.alt_steps / el_a, "unit": "images/s", "dtype": alt,
                       "ms_per_step": el_a / args.alt_steps * 1e3, "steps": args.alt_steps,
                       "requeried": alt_requeried,
                       "note": "the headline step (extract B images + certified top-k search of all queries vs the "
                               "sharded 1M DB, %s screening) with %s operands/activations; descriptor cosine vs the "
                               "reference: precisions.%s" % (args.screen, alt, alt)}
            del net_a, index_a
            torch.cuda.empty_cache()

        # extract-only loop (same net, no matching); warm-up first: the model swap and
        # empty_cache above returned the activation buffers, which must not be
        # re-allocated inside the timed loop
        ext_only = None
        if args.full:
            n_ext = max(3, args.steps // 2)
            for _ in range(max(2, args.warmup)):
                extract_all(False)
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            t1 = time.perf_counter()
            for _ in range(n_ext):
                extract_all(False)
            torch.cuda.synchronize()
            ext_only = n_ext * B / max_over_ranks(time.perf_counter() - t1)

        # PCIe-inclusive extraction (not `value`: the timed step starts with the
        # images resident in HBM): the step's B images from pinned host memory,
        # H2D on a copy stream double-buffered against the extractor; decoded
        # uint8 pixels (the fused stem reads x / 255) and float32 [0, 1] images.
        pcie = None
        if args.pcie_steps > 0:
            cs = torch.cuda.Stream(dev)

            def pcie_rate(host):
                bufs = [torch.empty(host.shape, dtype=host.dtype, device=dev) for _ in range(2)]
                ca, cb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                bufs[0].copy_(host, non_blocking=True)
                torch.cuda.synchronize()
                ca.record(cs)
                with torch.cuda.stream(cs):
                    for _ in range(3):
                        bufs[0].copy_(host, non_blocking=True)
                cb.record(cs)
                torch.cuda.synchronize()
                t_h2d = ca.elapsed_time(cb) / 3 * 1e-3
                copied = [torch.cuda.Event(), torch.cuda.Event()]
                freed = [torch.cuda.Event(), torch.cuda.Event()]
                for e in freed:
                    e.record(main_stream)
                net.extract(bufs[0][:EB])
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                for i in range(args.pcie_steps):
                    j = i % 2
                    cs.wait_event(freed[j])
                    with torch.cuda.stream(cs):
                        bufs[j].copy_(host, non_blocking=True)
                    copied[j].record(cs)
                    main_stream.wait_event(copied[j])
                    for c in range(0, B, EB):
                        net.extract(bufs[j][c:c + EB])
                    freed[j].record(main_stream)
                torch.cuda.synchronize()
                t_pipe = (time.perf_counter() - t3) / args.pcie_steps
                return B / t_pipe, t_h2d

            host8 = (images * 255.0).to(torch.uint8).cpu().pin_memory()
            r8, h8 = pcie_rate(host8)
            del host8
            host32 = images.cpu().pin_memory()
            r32, h32 = pcie_rate(host32)
            del host32
            pcie = {"images_per_sec": r8, "h2d_ms": h8 * 1e3, "h2d_gbs": B * 3 * H * W / h8 / 1e9,
                    "fp32_images_per_sec": r32, "fp32_h2d_ms": h32 * 1e3,
                    "fp32_serial_images_per_sec": B / (h32 + B / ext_only),
                    "note": "B 3x%dx%d images per step from pinned host memory, H2D on a copy stream double-buffered "
                            "against the extractor: uint8 pixels (rr_stem_conv_pool_u8) and float32 [0,1] images; "
                            "fp32 serial = H2D then extract" % (H, W)}

        # kNN-only loop: Q queries (same on every rank) vs the sharded 1M DB
        knn = None
        if args.knn_q > 0:
            qk = _ops.fill_unit_rows(args.knn_q, args.dim, seed=0x0E5EED, row0=0, device=dev)

            def timed_searches(qq, n):
                """n certified searches back to back; every certificate is resolved (and any
                uncertified query re-searched) inside the timed region"""
                index.search(qq, args.k, verify="deferred")[2].resolve()
                torch.cuda.synchronize()
                if world > 1:
                    dist.barrier()
                t_ = time.perf_counter()
                pends = [index.search(qq, args.k, verify="deferred")[2] for _ in range(n)]
                nre = sum(p_.resolve() for p_ in pends)
                torch.cuda.synchronize()
                if world > 1:
                    dist.barrier()
                return max_over_ranks((time.perf_counter() - t_) / n), nre

            tk, knn_requeried = timed_searches(qk, args.knn_steps)
            flops = 2.0 * args.knn_q * n_local * args.dim
            peak = {"fp32": PEAK_F32_TFLOPS, "int8": PEAK_I8_TOPS}.get(args.screen, PEAK_BF16_TFLOPS)
            knn = {"queries_per_sec": args.knn_q / tk, "q": args.knn_q, "db_rows": args.db_rows, "k": args.k,
                   "ms_per_batch": tk * 1e3, "screen_dtype": args.screen, "certified": True,
                   "requeried": knn_requeried, "searches": args.knn_steps,
                   "roofline": {"bound": "mfma", "achieved": flops / tk / 1e12, "peak": peak,
                                "unit": "TOP/s" if args.screen == "int8" else "TFLOP/s",
                                "frac": flops / tk / 1e12 / peak, "traffic": None,
                                "note": "per-rank screening GEMM operations 2*Q*n_local*D / whole search time, vs the "
                                        "dense MFMA peak of the screening dtype; every query's screening margin is "
                                        "certified on the device (requeried = uncertified queries re-searched in "
                                        "float32, inside the timed region), so the returned top-k are the exact "
                                        "float64 order"}}
            # the step's own search alone (B x world queries, no extraction beside it):
            # at <= 128 queries the score GEMM streams the screening copy of the DB
            qs1 = _ops.fill_unit_rows(B * world, args.dim, seed=0x0E5EED + 1, row0=0, device=dev)
            ts, step_search_requeried = timed_searches(qs1, args.knn_steps)
            db_bytes = float(n_local) * args.dim * {"fp32": 4, "int8": 1}.get(args.screen, 2)
            knn["step_search"] = {"q": B * world, "ms_per_search": ts * 1e3, "queries_per_sec": B * world / ts,
                                  "certified": True, "requeried": step_search_requeried,
                                  "roofline": {"bound": "hbm", "achieved": db_bytes / ts / 1e9, "peak": PEAK_HBM_GBS,
                                               "unit": "GB/s", "frac": db_bytes / ts / 1e9 / PEAK_HBM_GBS,
                                               "note": "screening-copy DB bytes per rank / whole search time"}}
            # the same searches on an int8 screening copy WITHOUT a certificate (its residual
            # bound does not certify dense random data): throughput beside its recall against
            # the certified result -- an approximate mode, never the headline
            if args.screen != "int8" and world == 1:
                from cirtorch.search import KnnIndex
                ref_i = index.search(qk, args.k, verify=True)[1]
                ref_s1 = index.search(qs1, args.k, verify=True)[1]
                ib = KnnIndex(db32, "int8")
                sub = {}
                for name, qq, ref in (("q%d" % args.knn_q, qk, ref_i), ("q%d" % (B * world), qs1, ref_s1)):
                    ib.search(qq, args.k, verify=False)
                    torch.cuda.synchronize()
                    t4 = time.perf_counter()
                    for _ in range(args.knn_steps):
                        ib.search(qq, args.k, verify=False)
                    torch.cuda.synchronize()
                    tb = (time.perf_counter() - t4) / args.knn_steps
                    got = ib.search(qq, args.k, verify=False)[1]
                    hits = sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(got.cpu(), ref.cpu()))
                    sub[name] = {"ms_per_batch": tb * 1e3, "queries_per_sec": qq.shape[0] / tb,
                                 "recall_at_k": hits / float(ref.numel()),
                                 "queries_exact": int((got == ref).all(1).sum()), "queries": int(qq.shape[0])}
                knn["int8_screen"] = dict(sub, certified=False,
                                          note="int8 screening copy (one scale per database tensor, per query row), "
                                               "exact float64 re-score of its candidates but NO certificate: "
                                               "approximate, recall vs the certified %s search" % args.screen)
                del ib
                torch.cuda.empty_cache()
            kt, kpath, kfresh = pmc_file("knn_q%d" % args.knn_q, lambda c: (
                c.get("db_rows"), c.get("dim"), c.get("k"), c.get("screen")) == (
                args.db_rows, args.dim, args.k, args.screen))
            if kt is not None and world == 1:
                kc = kt.get("config", {})
                if kfresh:
                    knn["roofline"]["traffic"] = kt["hbm_bytes_per_search"]
                knn["roofline"]["traffic_note"] = (
                    "HBM bytes of one search from rocprofv3 PMC (2 x FETCH_SIZE + WRITE_SIZE), %s, commit %s%s"
                    % (os.path.relpath(kpath, REPO), kc.get("source_commit", "?"),
                       "" if kfresh else "; STALE (kernel sources changed since: digest %s vs %s), not attached"
                       % (kc.get("source_digest", "?"), kernel_source_digest())))

        # the step's two collectives on their own (N > 1): the query all-gather
        # (B x D fp32 per rank) and the per-shard top-k exchange (one all-gather of
        # the packed (score, index) lists + the merge), HIP events on this stream
        comm = None
        if args.full and world > 1:
            qd = torch.randn((B, args.dim), generator=g, device=dev)
            sl, il = index.local.search(all_gather_stacked(qd).reshape(world * B, args.dim), args.k, verify=False)
            ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            res = {}
            for name, fn in (("query_allgather", lambda: all_gather_stacked(qd)),
                             ("topk_allgather_merge", lambda: index.exchange(sl, il, args.k))):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                dist.barrier()
                ea.record()
                for _ in range(20):
                    fn()
                eb.record()
                torch.cuda.synchronize()
                res[name] = max_over_ranks(ea.elapsed_time(eb) / 20)
            comm = {"query_allgather_ms": res["query_allgather"],
                    "topk_allgather_merge_ms": res["topk_allgather_merge"],
                    "query_bytes_per_rank": B * args.dim * 4, "topk_bytes_per_rank": world * B * args.k * 16,
                    "share_of_step": (res["query_allgather"] + res["topk_allgather_merge"]) / (elapsed / args.steps * 1e3),
                    "backend": dist.get_backend(), "world_size": dist.get_world_size(),
                    "note": "max over ranks of the mean of 20 back-to-back calls (HIP events); in the step the "
                            "two collectives run on the search stream beside the next extraction"}

    traffic, traffic_note = None, "no PMC traffic file for this config"
    t, tpath, tfresh = pmc_file("traffic", lambda c: (c.get("arch"), c.get("precision"), c.get("image")) == (
        args.arch, args.precision, [3, H, W]))
    if t is not None:
        c = t.get("config", {})
        if tfresh:
            traffic = t["hbm_bytes_per_image"] * B
        traffic_note = ("HBM bytes of the step's extractor dispatches from rocprofv3 PMC (2 x FETCH_SIZE + "
                        "WRITE_SIZE, %s, %d-image forwards, commit %s, kernel-source digest %s)%s"
                        % (os.path.relpath(tpath, REPO), c.get("batch", 0), c.get("source_commit", "?"),
                           c.get("source_digest", "?"), "" if tfresh else
                           "; STALE: the kernel sources changed since (current digest %s), not attached"
                           % kernel_source_digest()))
    # local-descriptor head: 2048 keypoints per image on an
    # R50 mod4-shaped bf16 map (1024 ch at H/16 x W/16), E = 128, + mutual NN of two images
    local = None
    if args.local_kpts > 0:
        from cirtorch.search import mutual_nn
        nb, c4, h4, w4 = 8, 1024, H // 16, W // 16
        fmap = torch.randn((nb, h4, w4, c4), generator=g, device=dev).to(torch.bfloat16).permute(0, 3, 1, 2)
        kp = torch.rand((nb, args.local_kpts, 2), generator=g, device=dev) * 2 - 1
        wl = torch.randn((128, c4), generator=g, device=dev) * c4 ** -0.5
        bl = torch.zeros(128, device=dev)
        _ops.local_head(fmap, kp, wl, bl)
        torch.cuda.synchronize()
        ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ea.record()
        for _ in range(10):
            d = _ops.local_head(fmap, kp, wl, bl)
        eb.record()
        torch.cuda.synchronize()
        t_head = ea.elapsed_time(eb) / 10 * 1e-3
        mutual_nn(d[0], d[1])
        torch.cuda.synchronize()
        ea.record()
        for _ in range(10):
            mutual_nn(d[0], d[1])
        eb.record()
        torch.cuda.synchronize()
        t_mnn = ea.elapsed_time(eb) / 10 * 1e-3
        local = {"keypoints_per_sec": nb * args.local_kpts / t_head, "map": [nb, c4, h4, w4], "kpts": args.local_kpts,
                 "embedding": 128, "ms_per_batch": t_head * 1e3, "mutual_nn_ms": t_mnn * 1e3,
                 "note": "rr_local_head (bilinear sample + exact-f32 MFMA Linear + normalize) on a synthetic bf16 map; "
                         "mutual_nn = two exact top-1 searches (%d x %d x 128) + rr_mutual_nn"
                         % (args.local_kpts, args.local_kpts)}
    # serving latency: one image through the extractor, eager launches vs one
    # HIP-graph replay of the same launches (cirtorch.utils.graph)
    latency = None
    if args.latency and rank == 0:
        from cirtorch.utils.graph import GraphedForward
        x1 = images[:1].contiguous()
        gf = GraphedForward(lambda t: net.extract(t), x1)
        ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        res = {}
        for name, fn in (("eager", lambda: net.extract(x1)), ("graph", lambda: gf(x1))):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ea.record()
            for _ in range(20):
                fn()
            eb.record()
            torch.cuda.synchronize()
            res[name] = ea.elapsed_time(eb) / 20
        latency = {"batch": 1, "eager_ms": res["eager"], "graph_ms": res["graph"],
                   "note": "one 3x%dx%d image, extract (body + GeM/L2N/whiten/L2N); graph = torch.cuda.CUDAGraph "
                           "(hipGraph) capture of the same librr launches, replayed" % (H, W)}
        del gf
    fl_img = conv_flops_per_image(net.body, H, W)
    costs = layer_costs(net.body, H, W, 4 if args.precision == "fp32" else 2)
    peak_m = (PEAK_F32_TFLOPS if args.precision == "fp32" else PEAK_BF16_TFLOPS) * 1e12
    floor_ms = B * sum(max(f / peak_m, b / (PEAK_HBM_GBS * 1e9)) for f, b in costs) * 1e3
    bytes_img = sum(b for _, b in costs)
    achieved = fl_img * B / (body_ms * 1e-3) / 1e12
    peak = PEAK_F32_TFLOPS if args.precision == "fp32" else PEAK_BF16_TFLOPS
    value = world * B * args.steps / elapsed
    out = {
        "metric": METRIC,
        "value": value,
        "unit": "images/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "full": args.full,
        "ms_per_step": elapsed / args.steps * 1e3,
        "requeried": step_requeried,
        "searches": step_searches,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": args.precision,
        "data": "synthetic (U[0,1) images, random-init weights, counter-hash N(0,1) unit DB rows)",
        "config": {"workload": "%s-GeM+whiten %s extract %dx%d, B=%d/GPU per step (chains of %d); every extracted "
                               "image is a query: top-%d cosine kNN vs %d x %d DB sharded over %d GPU(s) (%s screening, "
                               "certified per query, exact float64 re-score), %s, all inside the timed region%s"
                               % (args.arch, args.precision, W, H, B, EB, args.k, args.db_rows, args.dim, world,
                                  args.screen, ("searched in batches of %d queries per GPU (%d gathered per search; the "
                                                "last batch flushed)" % (QB, QB * world)) if QB else
                                  "searched every step (%d queries gathered)" % (B * world),
                                  "; the searches on a second stream beside the extraction" if args.overlap else ""),
                   "global_batch": B * world, "query_batch": QB * world if QB else B * world, "extract_batch": EB, "image": [3, H, W], "db_rows": args.db_rows,
                   "dim": args.dim,
                   "k": args.k, "parallelism": "dp%d (images) x db-shard%d" % (world, world),
                   "launch": "extractor chains replayed as hipGraphs" if args.graph else "eager launches"},
        "roofline": {"bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s",
                     "frac": achieved / peak, "traffic": traffic, "traffic_note": traffic_note,
                     "algorithmic_bytes": bytes_img * B,
                     "note": "dominant kernel family = the extractor body's 53 conv layers per forward (k_stem_pool3, "
                             "k_gemm8 / k_gemm8a, k_c3s_w128, k_c3w64 / k_conv3x3, k_wres1x1 / k_stream1x1, fused boundaries k_c3pair / k_pair_mid_ring, "
                             "k_igemm; "
                             "their per-kernel rocprof averages sum to this time, see profiles/); algorithmic_bytes = "
                             "per-layer unfused input + output (+ residual) bytes, so the fused boundaries can bring "
                             "the PMC traffic below it; "
                             "%.2f GFLOP/img x %d img / extract-body event time %.3f ms" % (fl_img / 1e9, B, body_ms)},
        "roofline_layers": {"floor_ms": floor_ms, "measured_ms": body_ms, "frac": floor_ms / body_ms,
                            "hbm_bytes_per_img": bytes_img, "peak_mfma_tflops": peak_m / 1e12,
                            "peak_hbm_gbs": PEAK_HBM_GBS,
                            "note": "sum over the body's 53 conv layers of max(FLOPs/peak_mfma, algorithmic HBM bytes/"
                                    "peak_hbm) for the step's images, over the measured extractor time"},
        "extract_images_per_sec": ext_only * world if ext_only is not None else None,
        "build": build_provenance(),
        "dist": {"world_size": dist.get_world_size() if dist.is_initialized() else 1,
                 "backend": dist.get_backend() if dist.is_initialized() else None,
                 "note": "backend nccl = RCCL over xGMI on ROCm"},
        "e2e_%s" % alt if alt else "e2e_alt": e2e_alt,
        "comm": comm,
        "knn": knn,
        "local": local,
        "latency": latency,
        "pcie": pcie,
    }
    if world == 1 and args.extras:
        del index, db32
        torch.cuda.empty_cache()
        with torch.no_grad():
            # the drop-in API first: after config 5's 123 GB index its decoded-tensor rate read
            # 1.3-1.6k img/s in every round-5 run vs 3.9k standalone (tools/dropin_parts.py)
            out["dropin"] = bench_dropin(net, H, W, dev)
            out["precisions"] = bench_precisions(args, images, dev)
            out["config3"] = bench_config3(args, images, dev, "fp16" if args.precision == "fp32" else args.precision)
            out["config4"] = bench_config4(args, images, dev)
            out["config5"] = bench_config5(args, images, dev)
        # the headline precision's descriptor parity on every config that has a reference golden
        bars = {"config2_r50": out["precisions"][args.precision]["meets_north_star_bar"],
                "config3_r101_ms": out["config3"]["meets_north_star_bar"]}
        if args.precision == "fp16":
            bars["config5_r152"] = out["config5"]["extract"]["meets_north_star_bar"]
        out["north_star_parity"] = {"dtype": args.precision, "bar": "min descriptor cosine vs the reference golden "
                                    ">= 1 - 1e-4", "configs": bars, "all_meet": all(bars.values())}
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args)
    if rank == 0:
        out["build"] = out.pop("build")  # last: inside the tail of stdout a driver keeps
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
