"""Timing of the affine-shape stage: estimate_affine_shape (rr_laf_affine_shape: pyramid build + one
fused kernel) against the chain of separate entries, a torch composition of the same arithmetic and
describe_keypoints(pyramid=True) without orientation, all at the same frames: 128 images of
3 x 768 x 1024 uint8 and one image, the 2048 frames per image from detect_keypoints_scale_space
(Hessian).  One process, the variants interleaved round by round, HIP events around every call,
warm-up, median and min-max.
    python tools/affine_probe.py [--reps 10] [--batch 128] [--h 768] [--w 1024] [--num 2048] [--chunk 16]
Prints one JSON line (microseconds):
  levels_hist            frames per pyramid level at patch size 32 (live slots of all images)
  circles, live          live frames the estimator leaves circular (both moments under eps) and all live frames
  axis_ratio_median_max  |A00 / A11| of the live frames that changed
  build_b<B>_us          levels 1 .. last of the gray image from the uint8 batch (rr_patch_pyramid)
  affine_b<B>_us         (a) estimate_affine_shape
  inplace_b<B>_us        the same written over its input frames, as detect_keypoints_scale_space(affine=True) calls it
  chain_b<B>_us          (b) rr_patch_pyramid -> rr_extract_patches_pyramid -> rr_patch_affine_shape ->
                         rr_ellipse_to_laf -> rescaling in torch, `chunk` images at a time (the patches of
                         128 x 2048 frames are 1 GiB)
  torch_b<B>_us          (c) the engine's pyramid patches, then torch in float32: Sobel by conv2d on the
                         replicate-padded patch, the window, the three means, the degenerate rule, the
                         normalisation, ellipse_to_laf in closed form, the rescaling; `chunk` images at a time
  describe_b<B>_us       (d) describe_keypoints(pyramid=True, orientation=False), the same frames
  *_min_max              the spread of each
  chain_bits_equal       (b) == (a) bit for bit;  torch_max_err: max |(c) - (a)| over the input scale
Developer tool.
"""

import argparse
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image-retrieval-for-image-based-localization_amd"))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PS = 32
EPS = 1e-10


def once(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return 1000 * t0.elapsed_time(t1)


def scale_of(f):
    return ((f[..., 0, 0] * f[..., 1, 1] - f[..., 1, 0] * f[..., 0, 1]) + 1e-10).abs().sqrt()


def rescale(E, lafs, dtype):
    out = E.to(dtype)
    r = scale_of(lafs.to(dtype)) / scale_of(out)
    return torch.cat([out[..., :2] * r[..., None, None], out[..., 2:]], dim=-1).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--h", type=int, default=768)
    ap.add_argument("--w", type=int, default=1024)
    ap.add_argument("--num", type=int, default=2048)
    ap.add_argument("--chunk", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("affine_probe needs a GPU")
    from cirtorch import _engine as E
    from cirtorch import _ops
    from cirtorch.features.laf import make_upright
    from cirtorch.search import describe_keypoints, detect_keypoints_scale_space, estimate_affine_shape
    from tools.src_digest import digest
    dev = torch.device("cuda:0")
    b, h, w, num = args.batch, args.h, args.w, args.num
    gen = torch.Generator(device=dev).manual_seed(5)
    u8 = torch.empty((b, 3, h, w), dtype=torch.uint8, device=dev)
    for i in range(0, b, 16):      # structure at every scale: noise on grids of 4 .. 128 px (the image of pyrpatch_probe.py)
        f = sum(F.interpolate(torch.rand((min(16, b - i), 3, h // p, w // p), device=dev, generator=gen), size=(h, w), mode="bilinear")
                for p in (4, 8, 16, 32, 64, 128)) / 6
        u8[i:i + 16] = (f * 255).round().clamp(0, 255).to(torch.uint8)
    lafs = torch.empty((b, num, 2, 3), device=dev)
    count = torch.empty(b, dtype=torch.int32, device=dev)
    for i in range(0, b, 16):
        lafs[i:i + 16], _, count[i:i + 16] = detect_keypoints_scale_space(u8[i:i + 16], num)
    live = torch.arange(num, device=dev)[None, :] < count[:, None]
    s = scale_of(lafs.double())
    lv = ((2.0 * s / PS).log2() + 0.5).floor().clamp(min=0).long()[live]

    # the window and the Sobel pair / 8 of the torch composition
    xs = torch.arange(PS, dtype=torch.float64) - PS // 2 + (0.0 if PS % 2 else 0.5)
    g1 = torch.exp(-(xs * xs) / float(PS * PS))
    g1 = (g1 / g1.sum()).float().to(dev)
    window = g1[:, None] * g1[None, :]
    kx = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]], device=dev) / 8.0
    sobel = torch.stack([kx, kx.t()])[:, None]
    circle = torch.tensor([1.0, 0.0, 1.0], device=dev)

    def patches_of(x, fr):
        pyr = _ops.patch_pyramid(x, PS, gray=True)[1]
        return _ops.extract_patches_pyramid(x, make_upright(fr.double()).float(), PS, gray=True, pyr=pyr)[:, :, 0]

    def chunks(nb, fn):
        ends = [(i, min(i + args.chunk, nb)) for i in range(0, nb, args.chunk)]
        return torch.cat([fn(u8[i:j], lafs[i:j], live[i:j]) for i, j in ends])

    def chain(x, fr, lv_):
        abc = _ops.patch_affine_shape(patches_of(x, fr))
        out = rescale(_ops.ellipse_to_laf(torch.cat([fr[..., 2], abc], dim=-1)), fr, torch.float64)
        return torch.where(lv_[..., None, None], out, torch.zeros_like(out))

    def composed(x, fr, lv_):
        P = patches_of(x, fr).reshape(-1, 1, PS, PS)
        g = F.conv2d(F.pad(P, (1, 1, 1, 1), mode="replicate"), sobel) * window
        gx, gy = g[:, 0], g[:, 1]
        m = torch.stack([(gx * gx).mean(dim=(1, 2)), (gx * gy).mean(dim=(1, 2)), (gy * gy).mean(dim=(1, 2))], dim=1)
        bad = ((m < EPS).sum(dim=1, keepdim=True) >= 2).float()
        m = m * (1.0 - bad) + circle * bad
        m = (m / m.max(dim=1, keepdim=True)[0]).view(fr.shape[0], fr.shape[1], 3)
        a11, a22 = m[..., 0].abs().sqrt(), m[..., 2].abs().sqrt()
        a21 = m[..., 1] / (a11 + a22).clamp(1e-9)
        zero = torch.zeros_like(a11)
        Efr = torch.stack([1.0 / a11, zero, fr[..., 0, 2], -a21 / (a11 * a22), 1.0 / a22, fr[..., 1, 2]], dim=-1).view(*fr.shape)
        out = rescale(Efr, fr, torch.float32)
        return torch.where(lv_[..., None, None], out, torch.zeros_like(out))

    batch_sizes = sorted({1, b})
    variants = {}
    for nb in batch_sizes:
        variants["build_b%d_us" % nb] = lambda nb=nb: _ops.patch_pyramid(u8[:nb], PS, gray=True)
        variants["affine_b%d_us" % nb] = lambda nb=nb: estimate_affine_shape(u8[:nb], lafs[:nb], count[:nb], PS)
        variants["chain_b%d_us" % nb] = lambda nb=nb: chunks(nb, chain)
        variants["torch_b%d_us" % nb] = lambda nb=nb: chunks(nb, composed)
        variants["describe_b%d_us" % nb] = lambda nb=nb: describe_keypoints(
            u8[:nb], None, count[:nb], lafs=lafs[:nb], orientation=False, patch_size=PS, pyramid=True)
    scratch = lafs.clone()

    def inplace(nb):
        scratch[:nb].copy_(lafs[:nb])
        return once(lambda: _ops.laf_affine_shape(u8[:nb], scratch[:nb], count[:nb], PS, out=scratch[:nb]))

    times = {k: [] for k in variants}
    times.update({"inplace_b%d_us" % nb: [] for nb in batch_sizes})
    for r in range(args.warmup + args.reps):
        for k, fn in variants.items():   # interleaved: drift hits every variant alike
            t = once(fn)
            if r >= args.warmup:
                times[k].append(t)
        for nb in batch_sizes:
            t = inplace(nb)
            if r >= args.warmup:
                times["inplace_b%d_us" % nb].append(t)
    got = estimate_affine_shape(u8, lafs, count, PS)
    ratio = (got[..., 0, 0] / got[..., 1, 1]).abs()[live]
    changed = ratio[(ratio - 1).abs() > 1e-6]
    norm = s.float()[..., None, None]
    out = {"batch": b, "h": h, "w": w, "num": num, "reps": args.reps, "ps": PS, "chunk": args.chunk,
           "build": E.lib().rr_build_info().decode(), "tree_digest": digest(), "device": E.device_arch(),
           "count_min_max": [int(count.min()), int(count.max())], "levels": _ops.pyramid_levels(h, w, PS),
           "levels_hist": torch.bincount(lv).tolist(), "live": int(live.sum()), "circles": int(live.sum()) - int(changed.numel()),
           "axis_ratio_median_max": [round(float(changed.median()), 3), round(float(changed.max()), 3)] if changed.numel() else None,
           "chain_bits_equal": bool(torch.equal(chunks(b, chain), got)),
           "inplace_bits_equal": bool(torch.equal(scratch, got)),
           "torch_max_err": float(((chunks(b, composed) - got)[..., :2] / norm).abs().nan_to_num(math.inf).max())}
    for k, v in times.items():
        out[k] = round(statistics.median(v), 1)
        out[k + "_min_max"] = [round(min(v), 1), round(max(v), 1)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
