"""Timing of keypoint detection (cirtorch.search.detect_keypoints: rr_response -> candidates ->
top-N selection) against a torch-on-GPU composition of the same operators, at 128 images of
3 x 768 x 1024 (uint8 and float32) and at one image (latency), for the three responses.  One
process, the variants interleaved round by round, HIP events around every call, warm-up, median
and min-max.
    python tools/detect_probe.py [--reps 20] [--batch 128] [--h 768] [--w 1024] [--num 2048]
Prints one JSON line (microseconds; GB/s):
  <kind>_<dtype>_b<B>_us        detect_keypoints, B images
  <kind>_response_u8_b<B>_us    the response kernel alone (gray reduction included)
  torch_<kind>_b<B>_us          the composition (float32 input): gray, replicate pad + Sobel
                                conv2d, products, reflect pad + 7 x 7 Gaussian conv2d (5 x 5 Sobel
                                conv2d for Hessian), score, 5 x 5 max-pool NMS (x == pool(x), x > 0:
                                cheaper than the reference's one-hot convolution; ties and edge pixels aside), topk
  *_min_max                     the spread of each
  <kind>_<dtype>_b<B>_gbps      the contract's traffic (image read + score write + score read)
                                over the detect time;  copy_gbps: a device copy of the float32 batch
                                (read + write) on the same box, for scale
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
import torch.nn.functional as F  # noqa: E402

KINDS = ("harris", "gftt", "hessian")


def once(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return 1000 * t0.elapsed_time(t1)


class TorchDetector:
    """the same operators as plain torch ops on the device (float32)"""

    def __init__(self, dev):
        sx = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], device=dev) / 8
        self.sobel = torch.stack([sx, sx.t()])[:, None]
        g = torch.exp(-(torch.arange(7, device=dev, dtype=torch.float32) - 3) ** 2 / 2)
        g = g / g.sum()
        self.gauss = (g[:, None] * g[None, :])[None, None].repeat(3, 1, 1, 1)
        gxx = torch.tensor([[-1., 0., 2., 0., -1.], [-4., 0., 8., 0., -4.], [-6., 0., 12., 0., -6.], [-4., 0., 8., 0., -4.],
                            [-1., 0., 2., 0., -1.]], device=dev) / 64
        gxy = torch.tensor([[-1., -2., 0., 2., 1.], [-2., -4., 0., 4., 2.], [0., 0., 0., 0., 0.], [2., 4., 0., -4., -2.],
                            [1., 2., 0., -2., -1.]], device=dev) / 36
        self.hess = torch.stack([gxx, gxy, gxx.t()])[:, None]

    def response(self, x, kind, k=0.04):
        gray = 0.299 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.114 * x[:, 2:3]
        if kind == "hessian":
            d = F.conv2d(F.pad(gray, (2, 2, 2, 2), mode="replicate"), self.hess)
            return d[:, 0:1] * d[:, 2:3] - d[:, 1:2] ** 2
        d = F.conv2d(F.pad(gray, (1, 1, 1, 1), mode="replicate"), self.sobel)
        dx, dy = d[:, 0:1], d[:, 1:2]
        m = F.conv2d(F.pad(torch.cat([dx * dx, dy * dy, dx * dy], 1), (3, 3, 3, 3), mode="reflect"), self.gauss, groups=3)
        det, tr = m[:, 0:1] * m[:, 1:2] - m[:, 2:3] ** 2, m[:, 0:1] + m[:, 1:2]
        if kind == "harris":
            return det - k * tr * tr
        return 0.5 * (tr - torch.sqrt((tr * tr - 4 * det).abs()))

    def detect(self, x, kind, num):
        s = self.response(x, kind)
        keep = (s == F.max_pool2d(s, 5, 1, 2)) & (s > 0)
        val, idx = torch.topk((s * keep).flatten(1), num, dim=1)
        w = s.shape[-1]
        return torch.stack([idx % w, idx // w], -1).float(), val


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--h", type=int, default=768)
    ap.add_argument("--w", type=int, default=1024)
    ap.add_argument("--num", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("detect_probe needs a GPU")
    from cirtorch import _engine as E
    from cirtorch import _ops
    from cirtorch.search import detect_keypoints
    from tools.src_digest import digest
    dev = torch.device("cuda:0")
    b, h, w, num = args.batch, args.h, args.w, args.num
    gen = torch.Generator(device=dev).manual_seed(5)
    # a smooth field plus pixel noise, like the tests' structured images
    low = torch.rand((b, 3, h // 64, w // 64), device=dev, generator=gen)
    f32 = (0.8 * F.interpolate(low, size=(h, w), mode="bilinear") + 0.2 * torch.rand((b, 3, h, w), device=dev, generator=gen))
    u8 = (f32 * 255).round().clamp(0, 255).to(torch.uint8)
    f32 = (u8.float() / 255).contiguous()
    tdet = TorchDetector(dev)
    sizes = sorted({1, b})
    variants = {}
    for kind in KINDS:
        for nb in sizes:
            variants["%s_u8_b%d_us" % (kind, nb)] = lambda kind=kind, nb=nb: detect_keypoints(u8[:nb], num, kind)
            variants["%s_f32_b%d_us" % (kind, nb)] = lambda kind=kind, nb=nb: detect_keypoints(f32[:nb], num, kind)
            variants["%s_response_u8_b%d_us" % (kind, nb)] = lambda kind=kind, nb=nb: _ops.response(u8[:nb], kind, gray=True)
            variants["torch_%s_b%d_us" % (kind, nb)] = lambda kind=kind, nb=nb: tdet.detect(f32[:nb], kind, num)
    variants["copy_f32_us"] = lambda: f32.clone()
    times = {k: [] for k in variants}
    for r in range(args.warmup + args.reps):
        for k, fn in variants.items():   # interleaved: drift hits every variant alike
            t = once(fn)
            if r >= args.warmup:
                times[k].append(t)
    out = {"batch": b, "h": h, "w": w, "num": num, "reps": args.reps, "build": E.lib().rr_build_info().decode(),
           "tree_digest": digest(), "device": E.device_arch()}
    for k, v in times.items():
        out[k] = round(statistics.median(v), 1)
        out[k + "_min_max"] = [round(min(v), 1), round(max(v), 1)]
    for kind in KINDS:
        for nb in sizes:
            for dt, elem in (("u8", 1), ("f32", 4)):
                traffic = nb * (3 * h * w * elem + 2 * h * w * 4)   # image read + score write + score read
                out["%s_%s_b%d_gbps" % (kind, dt, nb)] = round(traffic / out["%s_%s_b%d_us" % (kind, dt, nb)] / 1e3, 1)
            out["speedup_%s_b%d" % (kind, nb)] = round(out["torch_%s_b%d_us" % (kind, nb)] / out["%s_f32_b%d_us" % (kind, nb)], 2)
    out["copy_gbps"] = round(2 * f32.numel() * 4 / out["copy_f32_us"] / 1e3, 1)
    cnt = detect_keypoints(u8, num, "harris")[2]
    out["harris_count_min_max"] = [int(cnt.min()), int(cnt.max())]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
