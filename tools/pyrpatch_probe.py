"""Timing of the patch pyramid: the pyramid build alone (rr_patch_pyramid), describe_keypoints with
pyramid=True (rr_describe_keypoints_pyramid) and with pyramid=False (rr_describe_keypoints) on the
same frames, with orientation off and on, at 128 images of 3 x 768 x 1024 uint8 and at one image.
The 2048 frames per image come from detect_keypoints_scale_space (Hessian).  One process, the
variants interleaved round by round, HIP events around every call, warm-up, median and min-max.
    python tools/pyrpatch_probe.py [--reps 10] [--batch 128] [--h 768] [--w 1024] [--num 2048] [--parent-lib PATH]
Prints one JSON line (microseconds; GB/s):
  levels_hist                   frames per pyramid level at patch size 32 (live slots of all images)
  build_b<B>_us                 (a) levels 1 .. last of the gray image from the uint8 batch
  pyr_o<0|1>_b<B>_us            (b) describe_keypoints(pyramid=True)
  flat_o<0|1>_b<B>_us           (c) describe_keypoints(pyramid=False), the same frames
  parent_o<0|1>_b<B>_us         rr_describe_keypoints of the library given by --parent-lib (another
                                build, loaded beside this one), called through ctypes on preallocated
                                outputs;  same_o<0|1>_b<B>_us: this build called the same way
  *_min_max                     the spread of each
  build_b<B>_gbps               the build's bytes (image read once, every level written once and every
                                level but the last read once) over its time;  copy_gbps: a device copy
                                of the uint8 batch (read + write) in the same run
  gap_o<O>_b<B>_us              (b) - ((c) + (a)), to be held against the spread of (c)
Developer tool.
"""

import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image-retrieval-for-image-based-localization_amd"))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PS = 32


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
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--h", type=int, default=768)
    ap.add_argument("--w", type=int, default=1024)
    ap.add_argument("--num", type=int, default=2048)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pyrpatch_probe needs a GPU")
    from cirtorch import _engine as E
    from cirtorch import _ops
    from cirtorch.search import describe_keypoints, detect_keypoints_scale_space
    from tools.src_digest import digest
    dev = torch.device("cuda:0")
    b, h, w, num = args.batch, args.h, args.w, args.num
    gen = torch.Generator(device=dev).manual_seed(5)
    u8 = torch.empty((b, 3, h, w), dtype=torch.uint8, device=dev)
    for i in range(0, b, 16):      # structure at every scale: noise on grids of 4 .. 128 px
        f = sum(F.interpolate(torch.rand((min(16, b - i), 3, h // p, w // p), device=dev, generator=gen), size=(h, w), mode="bilinear")
                for p in (4, 8, 16, 32, 64, 128)) / 6
        u8[i:i + 16] = (f * 255).round().clamp(0, 255).to(torch.uint8)
    lafs = torch.empty((b, num, 2, 3), device=dev)
    count = torch.empty(b, dtype=torch.int32, device=dev)
    for i in range(0, b, 16):
        lafs[i:i + 16], _, count[i:i + 16] = detect_keypoints_scale_space(u8[i:i + 16], num)
    live = torch.arange(num, device=dev)[None, :] < count[:, None]
    s = (lafs[..., 0, 0] * lafs[..., 1, 1] - lafs[..., 1, 0] * lafs[..., 0, 1] + 1e-10).abs().sqrt().double()
    lv = ((2.0 * s / PS).log2() + 0.5).floor().clamp(min=0).long()[live]
    sizes_hw = _ops.pyramid_levels(h, w, PS)
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        parent.rr_describe_keypoints.argtypes, parent.rr_describe_keypoints.restype = E._SIGS["rr_describe_keypoints"]
        parent.rr_build_info.restype = ctypes.c_char_p
        desc = torch.empty((b, num, 128), device=dev)
        ang = torch.empty((b, num), device=dev)
        ws = torch.empty(256, dtype=torch.uint8, device=dev)

        def parent_call(nb, o, lib=parent):
            rc = lib.rr_describe_keypoints(E.ptr(u8), nb, 3, h, w, 1, None, E.ptr(count), num, 12.0, E.ptr(lafs), o, 36, PS, 8, 4, 1, 0.2,
                                              E.ptr(desc), E.ptr(ang), None, E.ptr(ws), 256, E.stream_ptr())
            assert rc == 0, rc
    batch_sizes = sorted({1, b})
    variants = {}
    for nb in batch_sizes:
        variants["build_b%d_us" % nb] = lambda nb=nb: _ops.patch_pyramid(u8[:nb], PS, gray=True)
        for o in (0, 1):
            variants["pyr_o%d_b%d_us" % (o, nb)] = lambda nb=nb, o=o: describe_keypoints(
                u8[:nb], None, count[:nb], lafs=lafs[:nb], orientation=bool(o), patch_size=PS, pyramid=True)
            variants["flat_o%d_b%d_us" % (o, nb)] = lambda nb=nb, o=o: describe_keypoints(
                u8[:nb], None, count[:nb], lafs=lafs[:nb], orientation=bool(o), patch_size=PS)
            if parent is not None:
                variants["parent_o%d_b%d_us" % (o, nb)] = lambda nb=nb, o=o: parent_call(nb, o)
                variants["same_o%d_b%d_us" % (o, nb)] = lambda nb=nb, o=o: parent_call(nb, o, E.lib())
    variants["copy_u8_us"] = lambda: u8.clone()
    times = {k: [] for k in variants}
    for r in range(args.warmup + args.reps):
        for k, fn in variants.items():   # interleaved: drift hits every variant alike
            t = once(fn)
            if r >= args.warmup:
                times[k].append(t)
    out = {"batch": b, "h": h, "w": w, "num": num, "reps": args.reps, "ps": PS, "build": E.lib().rr_build_info().decode(),
           "tree_digest": digest(), "device": E.device_arch(), "count_min_max": [int(count.min()), int(count.max())],
           "levels": sizes_hw, "levels_hist": torch.bincount(lv).tolist(),
           "scale_min_median_max": [round(float(v), 2) for v in (s[live].min(), s[live].median(), s[live].max())]}
    if parent is not None:
        out["parent_build"] = parent.rr_build_info().decode()
        parent_call(b, 1)
        mine = describe_keypoints(u8, None, count, lafs=lafs, orientation=True, patch_size=PS)
        out["parent_bits_equal"] = bool(torch.equal(mine[0], desc) and torch.equal(mine[1], ang))
    for k, v in times.items():
        out[k] = round(statistics.median(v), 1)
        out[k + "_min_max"] = [round(min(v), 1), round(max(v), 1)]
    px = [a * c for a, c in sizes_hw]
    for nb in batch_sizes:
        traffic = nb * (3 * px[0] + 4 * (2 * sum(px[1:]) - px[-1] if len(px) > 1 else 0))
        out["build_b%d_gbps" % nb] = round(traffic / out["build_b%d_us" % nb] / 1e3, 1)
        for o in (0, 1):
            out["gap_o%d_b%d_us" % (o, nb)] = round(out["pyr_o%d_b%d_us" % (o, nb)] - out["flat_o%d_b%d_us" % (o, nb)]
                                                    - out["build_b%d_us" % nb], 1)
    out["copy_gbps"] = round(2 * u8.numel() / out["copy_u8_us"] / 1e3, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
