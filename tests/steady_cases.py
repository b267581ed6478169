"""Shared by tests/test_host_steady.py and tests/test_gpu_steady.py: the persistent conv kernels of the
backbone (rr_stream.hip, rr_c3pair.hip, rr_conv3.hip) run past their ring depth.

A persistent launch is min(tiles, CUs) blocks, so on a 256-CU device the shapes of test_gpu_kernels.py give
a block one to three tiles: a ring never wraps, a counted wait never runs with older stores in flight, and
no block ends on a tail.  RR_TUNE_GRID_CUS caps the grid; caps of 1 .. 128 on maps of 851 .. 8710 pixels give
the counts below at shapes that cost milliseconds.  Three parts:

  * the launch arithmetic of every launcher restated as plain functions (*_plan) that return
    Plan(grid, G, nslices, xmap, counts): G the blocks that share one channel slice, counts the sorted set of
    tiles per block or strips per wave.  test_host_steady.py asserts on them what every row is there to
    reach; test_gpu_steady.py asserts that rr_last_launch reports the same kernel, variant, grid and xmap;
  * float64 references of conv + affine (+ residual | projection) + leaky on operands already rounded to
    the storage type, each with pre = |scale| conv(|x|, |w|) + |shift| + |shortcut|, and the element-wise
    bound   |got - ref| <= u |ref| + (Ktot + 4) 2^-23 pre + a   (u = 2^-8 bf16, 2^-11 fp16: the output
    rounding; a = 2^-24 for fp16 subnormals; the middle term twice the textbook bound of a float32 sum of
    Ktot exact products).  Stages are chained through the kernel's own 16-bit output (z of a pair from the y
    that came back, y of the fused block from the t2 of the unfused 3x3 launch), so the double rounding of
    an intermediate never enters a tolerance;
  * the case tables.

Reached per kernel (ring depth; tiles per block or strips per wave under the caps of the tables):
  k_wres1x1        3 buffers (residual, and WRES_RING = 0), 6 (K = 256 plain), 4 (K = 512 plain);
                   16/17, 17/18, 34/35, 45/46, 67 and 137 tiles per block
  k_stream1x1      D = 2, 3, 4 register sets; 4/5, 8/9, 17/18, 33/34, 34/35 strips per wave
  k_stream_pair    D = 2; 3/4 and 6/7 strips per wave
  k_pair_mid_ring  4 residual slots, 2 x buffers; 9, 13/14 and 27 tiles per block
  k_pair_mid       2 residual buffers; 4/5 and 14 tiles per block
  k_c3pair         4-slot tile ring, two-tile unroll, one tile of lookahead; 1 .. 7 tiles per block
  k_conv3x3        two-tile software pipeline; 3/4, 4, 6, 6/7 and 12 tiles per block
  k_c3w64          two patch buffers; 3/4 tiles per block

The bound: no widening was needed.  On the host a float32 conv of the same operands, rounded to the storage type,
reaches 0.993 of it at worst (test_host_steady.py); on an MI355X every kernel stays below 0.994 of it as well, so the
tiled engine was never consulted (the figures per kernel are in test_gpu_steady.py's docstring).

torch and numpy only; every function takes tensors on any device."""

import collections
import functools

import torch

Plan = collections.namedtuple("Plan", "grid G nslices xmap counts")

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
A = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -24}
SLOPE = 0.01


def ceil_div(a, b):
    return -(-a // b)


def round_robin(items, workers):
    """sorted set of the non-zero item counts of workers g = 0 .. workers - 1 taking items g, g + workers, ..."""
    return sorted({ceil_div(items - g, workers) for g in range(min(workers, items))})


# ---------------------------------------------------------------- launch arithmetic
def wres_cw(K):
    """launch_stream1x1's launch_wres<K, CW> (rr_stream.hip:997-1006)"""
    return {512: 32, 256: 64, 128: 64}[K]


def wres_nbuf(K, res, ring):
    """k_wres1x1's NBUF (rr_stream.hip:769): 3 with the residual tile or WRES_RING = 0, else 6 where a tile is
    16 KiB (K = 256) and 4 at 32 KiB (K = 512)"""
    return 3 if res or not ring else (6 if 32 * K * 2 <= 16384 else 4)


def wres_plan(P, C, BC, cap):
    """launch_wres (rr_stream.hip:948-966): C / BC channel slices, cap / slices blocks per slice, 32-pixel tiles"""
    nslices = C // BC
    per = max(cap // nslices, 1)
    ntiles = ceil_div(P, 32)
    ps = min(per, ntiles)
    grid = ps * nslices
    return Plan(grid, ps, nslices, int(nslices > 1 and grid % (8 * nslices) == 0), round_robin(ntiles, ps))


def stream_plan(P, TC, K, FN, D, NW, C, cap):
    """launch_s_t (rr_stream.hip:916-926): strips of 16 FN pixels over per_slice x NW waves per channel slice"""
    lds = TC * K * 2 + TC * 8
    per_cu = (4 if NW <= 4 else 2) if (160 * 1024 // lds) >= 2 and NW <= 8 else 1
    nslices = C // TC
    nstrips = ceil_div(P, 16 * FN)
    per_slice = min(max(per_cu * cap // nslices, 1), ceil_div(nstrips, NW))
    grid = per_slice * nslices
    return Plan(grid, per_slice, nslices, int(nslices > 1 and grid % (8 * nslices) == 0), round_robin(nstrips, per_slice * NW))


def stream_variant(K, C):
    """(TC, K, FN, D, NW) of launch_stream1x1's table (rr_stream.hip:1012-1032)"""
    table = {(64, 64): (64, 64, 2, 4, 8), (64, 256): (256, 64, 1, 2, 8), (256, 64): (64, 256, 1, 4, 8),
             (256, 128): (128, 256, 1, 3, 8), (128, 512): (256, 128, 1, 3, 8), (512, 128): (128, 512, 1, 2, 8),
             (256, 1024): (256, 256, 1, 2, 8), (256, 512): (256, 256, 1, 2, 8), (512, 2048): (128, 512, 1, 2, 8),
             (512, 256): (128, 512, 1, 2, 8), (512, 1024): (128, 512, 1, 2, 8)}
    return table[(K, C)]


def pair_plan(P, cap):
    """rr_conv1x1_pair, the 64 / 256 boundary (rr_stream.hip:1096-1098): 16-pixel strips, 8 waves per block"""
    nstrips = ceil_div(P, 16)
    grid = min(ceil_div(nstrips, 8), cap)
    return Plan(grid, grid, 0, 0, round_robin(nstrips, grid * 8))


def mid_plan(P, cap, TP):
    """rr_conv1x1_pair, the 128 / 512 boundary (rr_stream.hip:1078-1079): TP = 32 (k_pair_mid_ring) or 64 (k_pair_mid)"""
    ntiles = ceil_div(P, TP)
    grid = min(ntiles, cap)
    return Plan(grid, grid, 0, 0, round_robin(ntiles, grid))


def c3pair_plan(n, h, w, cap):
    """rr_conv3x3_pair (rr_c3pair.hip:535-539) and k_c3pair's two tile walks (rr_c3pair.hip:148-156, rr_tilewalk.h) ->
    (static Plan, dynamic Plan).  4 x 32 tiles, a grid of a multiple of 8 blocks (at least 8).  Static: block b takes
    tiles i G + (b & 7) (G / 8) + (b >> 3); counts per block.  Dynamic: XCD x owns a contiguous range of
    ntiles / 8 (+ 1) tiles that its G / 8 blocks share through a counter; counts per XCD (per block where G = 8)."""
    ntiles = n * (h // 4) * (w // 32)
    grid = max(min(ntiles, cap) & ~7, 8)
    static = sorted({c for c in (len(range((b & 7) * (grid >> 3) + (b >> 3), ntiles, grid)) for b in range(grid)) if c})
    dynamic = sorted({c for c in (ntiles // 8 + (x < ntiles % 8) for x in range(8)) if c})
    return Plan(grid, grid, 0, 1, static), Plan(grid, grid, 0, 1, dynamic)


def c3_plan(n, h, w, c_out, TC, TH, TW, cap):
    """launch_c3 (rr_conv3.hip:528-531) and k_conv3x3's walk (rr_conv3.hip:84-88): block b takes tiles b, b + G, ..."""
    ntiles = n * (h // TH) * (w // TW) * (c_out // TC)
    grid = min(ntiles, cap)
    return Plan(grid, grid, c_out // TC, 0, round_robin(ntiles, grid))


def c3w64_plan(n, h, w, cap):
    """the k_c3w64 site (rr_conv3.hip:567-570) and its round walk (rr_conv3.hip:427, rr_tilewalk.h): 8 x 32 tiles"""
    ntiles = n * (h // 8) * (w // 32)
    grid = max(min(ntiles, cap) & ~7, 8)
    counts = sorted({c for c in (len(range((b & 7) * (grid >> 3) + (b >> 3), ntiles, grid)) for b in range(grid)) if c})
    return Plan(grid, grid, 0, 1, counts)


def c3_variant(c_in, c_out, h, mode, cap, n=0, w=0):
    """launch_conv3x3's choice under CONV3S = 0 (rr_conv3.hip:567-606) -> ("k_c3w64", None) or
    ("k_conv3x3", (TC, TH, TW, WC, WP, NSA))"""
    if c_in == 64 and c_out == 64 and h % 8 == 0:
        if mode in (9, 1):
            return "k_c3w64", None
        return "k_conv3x3", (64, 8, 32, 1, 8, 2) if mode == 4 else (64, 8, 32, 1, 4, 2) if mode == 6 else (64, 8, 32, 2, 4, 2)
    assert c_out % 128 == 0 and c_out <= 512
    if mode in (1, 8) and c_out % 256 == 0 and h % 6 == 0:
        return "k_conv3x3", (256, 6, 32, 4, 2, 2)
    t8 = n * (h // 8) * (w // 32) * (c_out // 128) if h % 8 == 0 else 0
    want8 = mode == 2 or (mode != 3 and t8 >= 2 * cap)
    nsa = 3 if mode == 7 else 2
    if t8 > 0 and (want8 or h % 4):
        return "k_conv3x3", (128, 8, 32, 2, 4, nsa)
    assert h % 4 == 0
    return "k_conv3x3", (128, 4, 32, 2, 4, nsa)


# ---------------------------------------------------------------- operands and float64 references
def rounded(t, dt):
    return t.to(dt).float()


def affine(c, g):
    """scale in +-[0.5, 1.5) with every 7th channel negative and every 11th (from 3) zero; shift ~ 0.1 N(0, 1)"""
    scale = torch.rand(c, generator=g) + 0.5
    scale[::7] *= -1
    scale[3::11] = 0
    return scale, torch.randn(c, generator=g) * 0.1


def conv_nhwc(x, w, stride=1, pad=0):
    """x [n, h, w, ci] * w [co, ci, kh, kw] -> [n, ho, wo, co] as one matrix product per tap, in x's dtype"""
    co, ci, kh, kw = w.shape
    n, h, wd, _ = x.shape
    ho, wo = (h + 2 * pad - kh) // stride + 1, (wd + 2 * pad - kw) // stride + 1
    if pad:
        x = torch.nn.functional.pad(x, (0, 0, pad, pad, pad, pad))
    out = None
    for dy in range(kh):
        for dx in range(kw):
            xs = x[:, dy:dy + (ho - 1) * stride + 1:stride, dx:dx + (wo - 1) * stride + 1:stride, :]
            t = xs.reshape(-1, ci) @ w[:, :, dy, dx].t()
            out = t if out is None else out + t
    return out.reshape(n, ho, wo, co)


def leaky_(t, leaky):
    return torch.where(t > 0, t, t * SLOPE) if leaky else t


def reference(x, w, scale, shift, leaky, stride=1, pad=0, residual=None, proj=None):
    """float64 act(conv(x, w) scale + shift + shortcut) of NHWC x (values already rounded to the storage type) ->
    (ref, pre, Ktot); shortcut = residual [n, ho, wo, co] or proj = (xp, wp, scalep, shiftp) (a 1x1)"""
    d = lambda t: t.double()  # noqa: E731
    ref = conv_nhwc(d(x), d(w), stride, pad) * d(scale) + d(shift)
    pre = conv_nhwc(d(x).abs(), d(w).abs(), stride, pad) * d(scale).abs() + d(shift).abs()
    ktot = w.shape[1] * w.shape[2] * w.shape[3]
    if residual is not None:
        ref, pre = ref + d(residual), pre + d(residual).abs()
    if proj is not None:
        xp, wp, sp, hp = proj
        ref = ref + conv_nhwc(d(xp), d(wp)) * d(sp) + d(hp)
        pre = pre + conv_nhwc(d(xp).abs(), d(wp).abs()) * d(sp).abs() + d(hp).abs()
        ktot += wp.shape[1]
    return leaky_(ref, leaky), pre, ktot


def bound(ref, pre, ktot, dt):
    return U[dt] * ref.abs() + (ktot + 4) * 2.0 ** -23 * pre + A[dt]


def excess(got, ref, pre, ktot, dt):
    """the largest |got - ref| / bound over the elements (<= 1: inside) and the index of that element"""
    r = ((got.double() - ref).abs() / bound(ref, pre, ktot, dt)).flatten()
    i = int(torch.argmax(r))
    return float(r[i]), i


def float32_conv(x, w, scale, shift, leaky, dt, stride=1, pad=0, residual=None, proj=None):
    """the same op in float32 with the output rounded to dt: what a correct kernel may return (host check of the bound)"""
    v = conv_nhwc(x.float(), w.float(), stride, pad) * scale.float() + shift.float()
    if residual is not None:
        v = v + residual.float()
    if proj is not None:
        xp, wp, sp, hp = proj
        v = v + (conv_nhwc(xp.float(), wp.float()) * sp.float() + hp.float())
    return leaky_(v, leaky).to(dt)


# ---------------------------------------------------------------- case tables
MAP_A = (1, 65, 67)      # 4355 px: 137 tiles of 32 (the last holds 3 pixels), 273 strips of 16
MAP_A2 = (2, 65, 67)     # 8710 px: 273 strips of 32, 545 of 16
MAP_S2 = (2, 83, 101)    # stride 2 -> 2 x 42 x 51 = 4284 px: 134 tiles, 268 strips
MAP_P = (1, 23, 37)      # 851 px: 54 strips of 16, 27 tiles of 32, 14 of 64

# k_wres1x1: (c_in, c_out, residual, leaky, stride, map, caps)
WRES_ROWS = [
    (512, 2048, True, True, 1, MAP_A, (8, 24, 64)),
    (256, 1024, True, False, 1, MAP_A, (8, 16)),
    (128, 512, True, True, 1, MAP_A, (8,)),
    (512, 256, False, True, 1, MAP_A, (8,)),
    (512, 1024, False, False, 2, MAP_S2, (8, 32)),
    (512, 2048, False, True, 1, MAP_A, (64,)),
    (256, 512, False, True, 2, MAP_S2, (8,)),
    (256, 1024, False, True, 1, MAP_A, (8, 16)),
]

# k_stream1x1: (c_in, c_out, residual, leaky, stride, map, caps, WRES)
STREAM_ROWS = [
    (64, 64, False, True, 1, MAP_A2, (1,), 0),
    (64, 256, True, True, 1, MAP_A, (1,), 0),
    (64, 256, False, False, 1, MAP_A, (1,), 0),
    (256, 64, False, True, 1, MAP_A, (1,), 0),
    (256, 128, False, True, 1, MAP_A, (1,), 0),
    (128, 512, False, True, 1, MAP_A, (1,), 0),
    (128, 512, False, False, 1, MAP_A2, (8,), 0),
    (512, 128, False, True, 1, MAP_A, (1,), 0),
    (512, 2048, True, True, 1, MAP_A, (16, 128), 0),
    (256, 1024, True, False, 1, MAP_A, (4, 32), 0),
    (256, 512, False, True, 2, MAP_S2, (2, 16), 0),
    (512, 256, False, True, 1, MAP_A, (1,), 1),
    (512, 1024, False, False, 1, MAP_A, (1,), 1),
]

# k_stream_pair: (c_out, projection), map MAP_P, caps 1 and 2
PAIR_ROWS = [(64, False), (64, True), (128, False), (128, True)]
PAIR_CAPS = (1, 2)
# the 128 / 512 boundary: PAIR_MID -> caps
MID_CAPS = {1: (1, 2, 3), 0: (1, 3)}

# k_c3pair: (map, forms) with form = (c_out, projection, conv1); cap 8, and cap 16 where tiles >= 16
C3PAIR_FORMS = {"res64": (64, False, False), "res128": (128, False, False), "proj": (64, True, False),
                "proj_conv1": (64, True, True)}
C3PAIR_ROWS = [
    ((1, 4, 32), ("res64", "proj_conv1")),
    ((1, 36, 32), ("res128", "proj")),
    ((1, 52, 32), ("res64", "proj_conv1")),
    ((2, 28, 64), ("res128", "proj")),
    ((5, 12, 64), ("res64", "proj_conv1")),
    ((3, 20, 96), ("res128", "proj")),
    ((3, 36, 64), ("res64", "res128", "proj", "proj_conv1")),
]

# direct 3x3 under CONV3S = 0: ((n, c_in, h, w, c_out), leaky, ((mode, cap), ...))
C3_ROWS = [
    ((3, 64, 24, 96, 64), True, ((9, 8), (4, 8), (6, 8), (2, 8))),
    ((3, 64, 24, 96, 128), False, ((2, 8), (3, 8), (7, 8))),
    ((2, 128, 24, 64, 128), True, ((2, 4), (3, 4), (7, 4))),
    ((2, 256, 24, 64, 256), True, ((8, 4), (2, 4), (3, 4))),
    ((1, 512, 24, 32, 512), True, ((8, 2), (3, 4))),
]


def out_map(shape, stride):
    n, h, w = shape
    return n, (h - 1) // stride + 1, (w - 1) // stride + 1


def pixels(shape, stride=1):
    n, h, w = out_map(shape, stride)
    return n * h * w


def seed_of(*key):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) & 0x7FFFFFFF


@functools.lru_cache(maxsize=None)
def conv_operands(c_in, c_out, k, shape, stride, res, dt):
    """NHWC operands of one conv, rounded to dt, on the CPU: dict(x, w [co, ci, k, k], scale, shift, residual | None)"""
    g = torch.Generator().manual_seed(seed_of(c_in, c_out, k, stride, res, *shape))
    n, h, w = shape
    x = rounded(torch.randn(n, h, w, c_in, generator=g), dt)
    wt = rounded(torch.randn(c_out, c_in, k, k, generator=g) * (2.0 / (c_in * k * k)) ** 0.5, dt)
    scale, shift = affine(c_out, g)
    residual = rounded(torch.randn(*out_map(shape, stride), c_out, generator=g), dt) if res else None
    return dict(x=x, w=wt, scale=scale, shift=shift, residual=residual)


@functools.lru_cache(maxsize=None)
def pair_operands(c_in, c_mid, c_out, shape, proj, dt):
    """operands of a 1x1 boundary (conv3 + shortcut, then conv1): dict(x, w3, s3, h3, residual | None, xp, wp, sp, hp, w1, s1, h1)"""
    g = torch.Generator().manual_seed(seed_of(c_in, c_mid, c_out, proj, *shape))
    n, h, w = shape
    o = dict(x=rounded(torch.randn(n, h, w, c_in, generator=g), dt))
    o["w3"] = rounded(torch.randn(c_mid, c_in, 1, 1, generator=g) * (2.0 / c_in) ** 0.5, dt)
    o["w1"] = rounded(torch.randn(c_out, c_mid, 1, 1, generator=g) * (2.0 / c_mid) ** 0.5, dt)
    o["s3"], o["h3"] = affine(c_mid, g)
    o["s1"], o["h1"] = affine(c_out, g)
    o["residual"] = None if proj else rounded(torch.randn(n, h, w, c_mid, generator=g), dt)
    o["xp"] = rounded(torch.randn(n, h, w, c_in, generator=g), dt)
    o["wp"] = rounded(torch.randn(c_mid, c_in, 1, 1, generator=g) * (2.0 / c_in) ** 0.5, dt)
    o["sp"], o["hp"] = affine(c_mid, g)
    return o


@functools.lru_cache(maxsize=None)
def block_operands(shape, c_out, proj, dt):
    """operands of the fused 256-channel block: pair_operands(64, 256, c_out) whose x is t2's place, plus the 3x3
    (t1, w33, s2, h2) and the block's conv1 (w0, s0, h0) for the conv1 form, where xp is the block input"""
    o = dict(pair_operands(64, 256, c_out, shape, proj, dt))
    g = torch.Generator().manual_seed(seed_of(9, c_out, proj, *shape))
    n, h, w = shape
    o["t1"] = rounded(torch.randn(n, h, w, 64, generator=g), dt)
    o["w33"] = rounded(torch.randn(64, 64, 3, 3, generator=g) * (2.0 / 576) ** 0.5, dt)
    o["s2"], o["h2"] = affine(64, g)
    o["w0"] = rounded(torch.randn(64, 64, 1, 1, generator=g) * (2.0 / 64) ** 0.5, dt)
    o["s0"], o["h0"] = affine(64, g)
    return o
