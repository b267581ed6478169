"""Shared by tests/test_gpu_head_ops.py: the case lists of the pooling / head /
resampling sweep, the seeded CPU input generators and the float64 restatements
the kernels are compared with.  Inputs are generated on the CPU, rounded to the
dtype under test, and every reference is computed from the rounded tensor."""

import zlib

import numpy as np
import torch
import torch.nn.functional as F

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def dt_id(dt):
    return str(dt).replace("torch.", "")


def gen(*key):
    """a torch.Generator seeded by the case's key (stable across runs and processes)"""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------ global pooling
# (name, kind, p, exponent as a one-element device tensor)
POOL_MODES = [
    ("gem_p3", "gem", 3.0, False), ("gem_p2", "gem", 2.0, False), ("gem_p1", "gem", 1.0, False),
    ("gem_p2.5", "gem", 2.5, False), ("gem_p3_dev", "gem", 3.0, True), ("gem_p2.5_dev", "gem", 2.5, True),
    ("mac", "mac", None, False), ("spoc", "spoc", None, False),
]
POOL_MODES_SHORT = [m for m in POOL_MODES if m[0] in ("gem_p3", "mac")]

# k_pool_nhwc_h16x8: hw = 1, 15, 16, 17, 48, 49, 63, 64, 65, 130, 207 -- around the 16 waves of a
# block, the point where wave 0 (hw = 49) and then every wave (hw = 64) enters the 4x-unrolled
# loop, and several trips of it
H16_HW = [(1, 1), (3, 5), (4, 4), (1, 17), (6, 8), (7, 7), (7, 9), (8, 8), (5, 13), (10, 13), (9, 23)]
H16_C = [8, 520, 1032]           # < one lane group row, a second channel block, a third
H16_HW_ALL_MODES = [(1, 17), (5, 13), (9, 23)]

# k_pool_nhwc: f32 maps, 16-bit maps with c % 8 == 4
NHWC_DT_C = [(F32, 4), (F32, 252), (F32, 260), (F32, 516), (BF16, 12), (BF16, 260), (F16, 12), (F16, 260)]
NHWC_HW = [(1, 1), (1, 3), (5, 1), (5, 7), (10, 13)]          # hw = 1, 3, 5, 35, 130

# k_pool_nchw: one wave per plane, 4 planes per block
NCHW_PLANES = [1, 3, 5, 7]
NCHW_HW = [(1, 1), (7, 9), (8, 8), (5, 13), (10, 13)]         # hw = 1, 63, 64, 65, 130


def pool_map(n, c, h, w, dtype, sign, channels_last, *key):
    """[n, c, h, w] (NCHW-contiguous, or a channels_last view of an NHWC buffer) in `dtype`.
    sign "pos": (rand + 0.05) * a per-pixel ramp, so no two pixels are interchangeable;
    "mixed": randn * 0.5 + 0.2, so GeM's clamp(min=eps) acts."""
    g = gen("pool", n, c, h, w, sign, *key)
    shape = (n, h, w, c) if channels_last else (n, c, h, w)
    if sign == "pos":
        ramp = 0.5 + torch.arange(1, h * w + 1, dtype=torch.float32) / (h * w)
        ramp = ramp.reshape(1, h, w, 1) if channels_last else ramp.reshape(1, 1, h, w)
        x = (torch.rand(shape, generator=g) + 0.05) * ramp
    else:
        x = torch.randn(shape, generator=g) * 0.5 + 0.2
    x = x.to(dtype)
    return x.permute(0, 3, 1, 2) if channels_last else x


def pool_ref(x, kind, p, eps=1e-6):
    """pools.py:10-38 in float64 on the rounded map: [n, c]"""
    xd = x.double()
    if kind == "gem":
        return xd.clamp(min=eps).pow(p).mean(dim=(2, 3)).pow(1.0 / p)
    if kind == "mac":
        return xd.amax(dim=(2, 3))
    return xd.mean(dim=(2, 3))


# ------------------------------------------------------------------ l2n
L2N_ROWS = [1, 3]
L2N_DIMS = [1, 63, 64, 255, 256, 257, 2049]


def l2n_rows_input(rows, dim):
    """float32 rows; a batch of 3 holds a random row, an all-zero row and a row of norm 1e-5
    (where the + eps of x / (||x|| + eps) is a tenth of the denominator)"""
    g = gen("l2n", rows, dim)
    x = torch.randn(rows, dim, generator=g)
    if rows == 3:
        x[1] = 0.0
        v = torch.randn(dim, generator=g).double()
        x[2] = (v * (1e-5 / v.norm())).float()
    return x


def l2n_ref(x, eps=1e-6):
    """normalizations.py:9-16 in float64: x / (||x||_2 + eps)"""
    xd = x.double()
    return xd / (xd.norm(dim=1, keepdim=True) + eps)


# ------------------------------------------------------------------ linear / head tail
LINEAR_CASES = [(1, 4, 1), (15, 12, 15), (16, 16, 16), (17, 20, 17), (63, 124, 40), (64, 128, 16), (65, 132, 17),
                (130, 516, 40)]
HEAD_TAIL_CASES = [(1, 16), (2, 36), (65, 520)]


def linear_input(rows, in_dim, out_dim):
    g = gen("linear", rows, in_dim, out_dim)
    x = torch.randn(rows, in_dim, generator=g)
    w = torch.randn(out_dim, in_dim, generator=g) / in_dim ** 0.5
    b = torch.randn(out_dim, generator=g) * 0.5
    return x, w, b


def linear_ref_and_bound(x, w, b):
    """float64 x W^T + b and the elementwise float32 dot-product bound
    (in_dim + 8) 2^-24 (|x| |W|^T + |b|): in_dim products and additions of unit roundoff
    2^-24 each, in any summation order, plus the bias addition and the slack of the
    first-order bound.  A missing or doubled term exceeds it by orders of magnitude."""
    xd, wd = x.double(), w.double()
    ref = xd @ wd.t()
    mag = xd.abs() @ wd.abs().t()
    if b is not None:
        ref = ref + b.double()
        mag = mag + b.double().abs()
    return ref, (x.shape[1] + 8) * 2.0 ** -24 * mag


def head_tail_input(rows, dim):
    g = gen("head_tail", rows, dim)
    x = torch.randn(rows, dim, generator=g) * 0.5 + 0.2
    w = torch.randn(dim, dim, generator=g) / dim ** 0.5
    b = torch.randn(dim, generator=g) * 0.1
    return x, w, b


def head_tail_ref(x, w, b, whiten):
    """global_head.py:59-64 in float64: L2N(W L2N(x) + b), or L2N(x) without whitening"""
    y = l2n_ref(x)
    if whiten:
        y = y @ w.double().t()
        if b is not None:
            y = y + b.double()
        y = y / (y.norm(dim=1, keepdim=True) + 1e-6)
    return y


# ------------------------------------------------------------------ whitenapply
WHITEN_CASES = [(1, 16, 1), (17, 48, 15), (64, 128, 16), (65, 144, 17), (130, 128, 128), (5, 30, 7)]


def whiten_input(rows, dim, d_out):
    """x: float32 unit rows; m = randn * 0.1 and P = randn / sqrt(dim) in float64"""
    r = np.random.default_rng(zlib.crc32(repr(("whiten", rows, dim, d_out)).encode()))
    x = r.standard_normal((rows, dim))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    m = r.standard_normal(dim) * 0.1
    P = r.standard_normal((dim, dim)) / np.sqrt(dim)
    return x, m, P


def whiten_ref(x, m, P, d_out):
    """whiten.py:4-12 in numpy float64 on rows: L2N(P[:d] (x - m)), + 1e-6 on the norm"""
    y = (x.astype(np.float64) - m[None, :]) @ P[:d_out].T
    return y / (np.linalg.norm(y, axis=1, keepdims=True) + 1e-6)


# ------------------------------------------------------------------ localHead
LOCAL_CASES = [(BF16, 8), (BF16, 520), (F16, 520), (F32, 4), (F32, 260)]
LOCAL_H, LOCAL_W, LOCAL_E, LOCAL_NPTS = 5, 7, 24, 5


def local_keypoints():
    """[2, 5, 2] normalised (x, y), different per image: the exact centre of a pixel; (-1, -1);
    (1, 1); a point outside the map with some taps in and some out; a point two pixels outside
    (all taps out).  In pixel units a pixel is 2 / size wide.  Image 0's fourth point is half a
    pixel left of the map (ix = -1: the west taps are out, the east taps in with weight ~0);
    image 1's is a quarter pixel below it (iy = h - 0.25: north taps in with weight 1/4)."""
    h, w = LOCAL_H, LOCAL_W
    px, py = 2.0 / w, 2.0 / h
    k0 = [[0.0, 0.0], [-1.0, -1.0], [1.0, 1.0], [-1.0 - 0.5 * px, 0.3], [-1.0 - 2.0 * px, -1.0 - 2.0 * py]]
    cx, cy = (2 * 1 + 1) / w - 1.0, (2 * 3 + 1) / h - 1.0          # centre of pixel (x = 1, y = 3)
    k1 = [[cx, cy], [-1.0, -1.0], [1.0, 1.0], [0.3, 1.0 + 0.25 * py], [1.0 + 2.0 * px, 0.1]]
    return torch.tensor([k0, k1], dtype=torch.float32)


def local_input(dtype, c):
    g = gen("local", dt_id(dtype), c)
    x = (torch.randn(2, LOCAL_H, LOCAL_W, c, generator=g) * 0.5 + 0.2).to(dtype).permute(0, 3, 1, 2)
    w = torch.randn(LOCAL_E, c, generator=g) / c ** 0.5
    b = torch.randn(LOCAL_E, generator=g) * 0.1
    return x, w, b


def local_ref(x, kpts, w, b):
    """local_head.py:43-71 in float64: grid_sample (bilinear, zeros, align_corners=False) ->
    Linear -> F.normalize, [n, npts, e]"""
    s = F.grid_sample(x.double(), kpts.double().unsqueeze(2), mode="bilinear", padding_mode="zeros",
                      align_corners=False)
    s = s.squeeze(3).permute(0, 2, 1)
    return F.normalize(s @ w.double().t() + b.double(), dim=2)


# ------------------------------------------------------------------ max-pool
MAXPOOL_HW = [(1, 1), (2, 2), (7, 8), (8, 7), (21, 19)]
MAXPOOL_KSP = [(3, 2, 1), (2, 2, 0), (3, 1, 1)]
MAXPOOL_DT_C = [(BF16, 8), (BF16, 72), (BF16, 12), (F16, 12), (F32, 3), (F32, 64)]
MAXPOOL_NAN_DT_C = [(BF16, 8), (BF16, 12), (F16, 12), (F32, 3)]     # both bf16 kernels, fp16, f32


def pooled_extent(size, k, stride, pad):
    return (size + 2 * pad - k) // stride + 1


MAXPOOL_CASES = [(hw, ksp, dc) for hw in MAXPOOL_HW for ksp in MAXPOOL_KSP for dc in MAXPOOL_DT_C
                 if pooled_extent(hw[0], ksp[0], ksp[1], ksp[2]) > 0 and pooled_extent(hw[1], ksp[0], ksp[1], ksp[2]) > 0]


def maxpool_input(h, w, c, dtype):
    """NHWC [2, h, w, c]"""
    return torch.randn(2, h, w, c, generator=gen("maxpool", h, w, c, dt_id(dtype))).to(dtype)


def maxpool_ref(x, k, stride, pad):
    """F.max_pool2d on the rounded values (the maximum is exact in any float type), NHWC float32"""
    return F.max_pool2d(x.float().permute(0, 3, 1, 2), k, stride, pad).permute(0, 2, 3, 1)


# ------------------------------------------------------------------ bilinear resize
# (1, 2, 3) and (1, 3, 2) keep one extent at sqrt 2 (and (1, 4, 7) at 1.2 below): that axis is
# sampled at scale 1, the other at 1 / s
RESIZE_SHAPES = [(1, 2, 2), (1, 2, 3), (1, 3, 2), (3, 3, 5), (3, 37, 50), (2, 64, 64), (2, 3, 10, 13)]
RESIZE_SCALES = [0.5, 2.0, 2.0 ** -0.5, 2.0 ** 0.5, 0.7, 1.0]
RESIZE_CASES = [(sh, s) for sh in RESIZE_SHAPES for s in RESIZE_SCALES if int(sh[-2] * s) > 0 and int(sh[-1] * s) > 0]
RESIZE_CASES.append(((1, 4, 7), 1.2))          # 4 x 7 -> 4 x 8: only the rows keep their extent
