"""Inputs and a numpy restatement of the learned patch descriptors (HardNet, SOSNet), numpy only.

Seeded weights and patches, the state-dict layout of the two reference modules, and quantised_net: the
arithmetic that include/rr.h states for rr_patchnet_trunk / rr_patchnet_head -- fp16 at the stated
rounding points (weights, the normalised patch, every layer's output of layers 1 .. 6), everything
else in float64.  tests/golden/make_golden_patchnet.py compares it with the reference modules in
float64 and derives the tolerances of tests/golden/patchnet.npz from that difference.

Further down, for tests/test_gpu_patchnet_edges.py and tests/test_host_patchnet_edges.py: quantised_net_f32 (the
same rounding points, float32 accumulation), probe weights with one entry +-1 per output channel and their
index-arithmetic map, the patches of tests/golden/patchnet_edges.npz with the altered normalisations each
group must expose, the seven patches of the batches past the 65535-block cap, and a batch with non-finite
patches.
"""

import numpy as np

# (cout, cin, kernel, stride, pad) of layers 1 .. 7
LAYERS = ((32, 1, 3, 1, 1), (32, 32, 3, 1, 1), (64, 32, 3, 2, 1), (64, 64, 3, 1, 1), (128, 64, 3, 2, 1), (128, 128, 3, 1, 1),
          (128, 128, 8, 1, 0))
VARIANTS = ("hardnet", "sosnet")
# index of conv l + 1 in the reference's nn.Sequential (its BatchNorm is the next index)
CONV_INDEX = {"hardnet": (0, 3, 6, 9, 12, 15, 19), "sosnet": (1, 4, 7, 10, 13, 16, 20)}
PREFIX = {"hardnet": "features", "sosnet": "layers"}
SEEDS = {"hardnet": 20261, "sosnet": 20262}
OTHER_SEED = 20263       # a second set of weights (module cache test)
PATCH_SEED = 20264
NPATCH = 129
BATCHES = (1, 2, 63, 64, 65, 129)
MAP_PATCHES = (0, 6, 7)  # the patches whose layer-6 map is in the fixture: a corner pixel, noise, smoothed noise
CONSTANT, ZERO = 4, 5    # indices of the constant and the all-zero patch


def net_params(seed):
    """weights [cout, cin, k, k] ~ N(0, 2 / fan_in), running_mean ~ U(-0.5, 0.5), running_var ~ U(0.5, 2),
    float32, layer 1 first"""
    rng = np.random.default_rng(seed)
    w, m, v = [], [], []
    for cout, cin, k, _, _ in LAYERS:
        w.append((rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32))
        m.append(rng.uniform(-0.5, 0.5, cout).astype(np.float32))
        v.append(rng.uniform(0.5, 2.0, cout).astype(np.float32))
    return w, m, v


def state_dict(variant, params):
    """{key: array} in the order of the reference module's state_dict()"""
    w, m, v = params
    out = {}
    for l, i in enumerate(CONV_INDEX[variant]):
        out["%s.%d.weight" % (PREFIX[variant], i)] = w[l]
        out["%s.%d.running_mean" % (PREFIX[variant], i + 1)] = m[l]
        out["%s.%d.running_var" % (PREFIX[variant], i + 1)] = v[l]
        out["%s.%d.num_batches_tracked" % (PREFIX[variant], i + 1)] = np.array(0, dtype=np.int64)
    return out


def _smooth5(x):
    p = np.pad(x, 2, mode="edge")
    return np.mean(np.lib.stride_tricks.sliding_window_view(p, (5, 5)), axis=(2, 3))


def patches(seed=PATCH_SEED, n=NPATCH):
    """float32 [n, 32, 32]: 0 .. 3 one bright pixel in each corner (the halo), 4 constant, 5 zero, then
    uniform noise, 5 x 5-smoothed noise and values in 0 .. 255 in turn"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 32, 32), dtype=np.float64)
    for i in range(n):
        if i < 4:
            out[i] = 0.1 * rng.uniform(0.0, 1.0, (32, 32))
            out[i, (0, 0, 31, 31)[i], (0, 31, 0, 31)[i]] = 8.0
        elif i == CONSTANT:
            out[i] = 0.5
        elif i == ZERO:
            pass
        elif i % 3 == 0:
            out[i] = rng.uniform(0.0, 1.0, (32, 32))
        elif i % 3 == 1:
            out[i] = _smooth5(rng.uniform(0.0, 1.0, (32, 32)))
        else:
            out[i] = np.floor(rng.uniform(0.0, 256.0, (32, 32)))
    return out.astype(np.float32)


def checksum(arrays):
    """a float64 figure that moves with any value and with the order"""
    tot = 0.0
    for a in arrays:
        a = np.asarray(a, dtype=np.float64).ravel()
        tot += float(np.sum(a * np.cos(np.arange(a.size, dtype=np.float64))))
    return tot


def f16(x):
    """one rounding to fp16 (nearest even), back in float64"""
    return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def conv_nhwc(x, w, stride, pad):
    """x [B, H, W, C] float64, w [cout, cin, k, k] -> [B, Ho, Wo, cout] float64"""
    k = w.shape[2]
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    win = np.lib.stride_tricks.sliding_window_view(xp, (k, k), axis=(1, 2))[:, ::stride, ::stride]   # [B, Ho, Wo, C, k, k]
    b, ho, wo = win.shape[:3]
    return (win.reshape(b * ho * wo, -1) @ w.astype(np.float64).reshape(w.shape[0], -1).T).reshape(b, ho, wo, -1)


def normalise_input(x, variant):
    """x [B, 32, 32] float64 -> the patch by its own statistics, float64"""
    mean = x.mean(axis=(1, 2), keepdims=True)
    ss = ((x - mean) ** 2).sum(axis=(1, 2), keepdims=True)
    den = np.sqrt(ss / 1023.0) + 1e-6 if variant == "hardnet" else np.sqrt(ss / 1024.0 + 1e-5)
    return (x - mean) / den


def normalise_output(f, variant):
    """f [B, 128] float64 after layer 7's BatchNorm -> the descriptor"""
    if variant == "hardnet":
        return f / np.maximum(np.sqrt((f * f).sum(axis=1, keepdims=True)), 1e-12)
    v = f + 1e-10
    return v / np.sqrt((v * v).sum(axis=1, keepdims=True))


def quantised_net(x, params, variant, block=32):
    """x [B, 32, 32] float32 -> (descriptors float64 [B, 128], layer-6 maps [B, 8, 8, 128], fp16 values in float64)"""
    w, m, v = params
    descs, maps = [], []
    for b0 in range(0, x.shape[0], block):
        a = f16(normalise_input(x[b0:b0 + block].astype(np.float64), variant))[..., None]
        for l, (_, _, _, stride, pad) in enumerate(LAYERS):
            scale = 1.0 / np.sqrt(v[l].astype(np.float64) + 1e-5)
            y = (conv_nhwc(a, f16(w[l]), stride, pad) - m[l].astype(np.float64)) * scale
            if l == 5:
                maps.append(f16(np.maximum(y, 0.0)))
            a = f16(np.maximum(y, 0.0)) if l < 6 else y
        descs.append(normalise_output(a.reshape(a.shape[0], 128), variant))
    return np.concatenate(descs), np.concatenate(maps)


# ---------------------------------------------------------------- the float32-accumulating restatement
def quantised_net_f32(x, params, variant, block=32):
    """quantised_net with the same rounding points (fp16 weights, normalised patch and the outputs of layers
    1 .. 6; float64 patch statistics) but the accumulation of every layer as a float32 matmul, scale and
    shift as the float32 values rr_patchnet_pack stores, BatchNorm, ReLU, layer 7 and the descriptor
    normalisation in float32.  Same return as quantised_net.  The difference of the two is the room a
    float32 accumulation order has; the kernels' own order is a third one."""
    w, m, v = params
    f32 = np.float32
    descs, maps = [], []
    for b0 in range(0, x.shape[0], block):
        a = normalise_input(x[b0:b0 + block].astype(np.float64), variant).astype(np.float16).astype(f32)[..., None]
        for l, (_, _, k, stride, pad) in enumerate(LAYERS):
            s64 = 1.0 / np.sqrt(v[l].astype(np.float64) + 1e-5)
            scale, shift = s64.astype(f32), (-m[l].astype(np.float64) * s64).astype(f32)
            xp = np.pad(a, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
            win = np.lib.stride_tricks.sliding_window_view(xp, (k, k), axis=(1, 2))[:, ::stride, ::stride]
            b, ho, wo = win.shape[:3]
            w16 = w[l].astype(np.float16).astype(f32).reshape(w[l].shape[0], -1)
            acc = (np.ascontiguousarray(win).reshape(b * ho * wo, -1) @ w16.T).reshape(b, ho, wo, -1)
            assert acc.dtype == f32
            y = acc * scale + shift
            if l < 6:
                a = np.maximum(y, f32(0)).astype(np.float16).astype(f32)
                if l == 5:
                    maps.append(a.astype(np.float64))
            else:
                f = y.reshape(b, 128)
        if variant == "hardnet":
            d = f / np.maximum(np.sqrt((f * f).sum(axis=1, keepdims=True, dtype=f32)), f32(1e-12))
        else:
            f = f + f32(1e-10)
            d = f / np.sqrt((f * f).sum(axis=1, keepdims=True, dtype=f32))
        assert d.dtype == f32
        descs.append(d.astype(np.float64))
    return np.concatenate(descs), np.concatenate(maps)


# ---------------------------------------------------------------- probe weights: one entry per output channel
PROBE_VAR = np.float32(1.0 - 1e-5)   # float32(1 / sqrt(float64(PROBE_VAR) + 1e-5)) == 1: the packed scale is 1.0f exactly
CENTRE = 1                           # ky = kx = 1 of a 3 x 3 kernel


def centre_spec():
    """the routing every probe starts from, per layer 1 .. 6 a dict of int arrays over cout: ci, ky, kx, sign.
    Layers 2 .. 6 take the centre tap of input channel co mod cin; where a layer widens (3 and 5, stride 2) the
    upper copies take tap (2, 2) instead, the odd rows and columns up to the last one.  So no two channels of a
    map past layer 1 are equal, map channels below 32 sample rows 4 Y (row 0: the top and left halo of the
    layer under test) and those from 96 rows 4 Y + 3 (row 31, row 15 of a 16 x 16 map: the bottom and right halo).
    Layer 1 takes tap co mod 9 with sign + - + - over co // 9: 18 distinct channels, co and co + 18 alike."""
    spec = []
    for l, (cout, cin, _, _, _) in enumerate(LAYERS[:6]):
        co = np.arange(cout)
        if l == 0:
            spec.append(dict(ci=np.zeros(cout, int), ky=(co % 9) // 3, kx=(co % 9) % 3, sign=1 - 2 * ((co // 9) % 2)))
        else:
            spec.append(dict(ci=co % cin, ky=CENTRE + (co >= cin), kx=CENTRE + (co >= cin), sign=np.ones(cout, int)))
    return spec


def window_spec():
    """the normalisation window: map channel c holds relu(s n[4 Y + ay + 2 by, 4 X + ax + 2 bx]) with
    c mod 32 = 16 (s < 0) + 8 ay + 4 ax + 2 by + bx.  Layer 1 takes the tap (1 + ay, 1 + ax) with sign s, layer 4
    the tap (1 + by, 1 + bx), every other layer the centre tap of channel co mod cin.  Over the 64 pixels and 16
    phases every one of the 1024 normalised pixels appears once with each sign, and no tap reads a halo."""
    spec = []
    for l, (cout, cin, _, _, _) in enumerate(LAYERS[:6]):
        c = np.arange(cout) % 32
        one, ctr = np.ones(cout, int), np.full(cout, CENTRE)
        if l == 0:
            spec.append(dict(ci=np.zeros(cout, int), ky=1 + (c >> 3 & 1), kx=1 + (c >> 2 & 1), sign=1 - 2 * (c >> 4)))
        elif l == 3:
            spec.append(dict(ci=np.arange(cout) % cin, ky=1 + (c >> 1 & 1), kx=1 + (c & 1), sign=one))
        else:
            spec.append(dict(ci=np.arange(cout) % cin, ky=ctr, kx=ctr, sign=one))
    return spec


GEOMETRY_A, GEOMETRY_B = 5, 3        # the channel map of the layer under test: ci = (5 co + 3) mod cin


def geometry_spec(layer, tap):
    """centre_spec with layer `layer` (2 .. 6) reading tap `tap` (0 .. 8, ky = tap // 3) of input channel
    (GEOMETRY_A co + GEOMETRY_B) mod cin in every output channel"""
    assert 2 <= layer <= 6 and 0 <= tap < 9
    spec = centre_spec()
    cout, cin = LAYERS[layer - 1][:2]
    co = np.arange(cout)
    spec[layer - 1] = dict(ci=(GEOMETRY_A * co + GEOMETRY_B) % cin, ky=np.full(cout, tap // 3), kx=np.full(cout, tap % 3),
                           sign=np.ones(cout, int))
    return spec


HEAD_POS_A, HEAD_POS_B, HEAD_CH_A, HEAD_CH_B = 37, 11, 5, 3


def head_spec():
    """layer 7: f[co] = map[ky, kx, ci] with 8 ky + kx = (37 co + 11) mod 64, ci = (5 co + 3) mod 128"""
    co = np.arange(128)
    pos = (HEAD_POS_A * co + HEAD_POS_B) % 64
    return dict(ci=(HEAD_CH_A * co + HEAD_CH_B) % 128, ky=pos // 8, kx=pos % 8, sign=np.ones(128, int))


def probe_params(spec, head=None):
    """(weights, means, variances) of a spec: one entry +-1 per output channel, running_mean 0, running_var
    PROBE_VAR.  Layer 7 is head_spec() unless given."""
    w, m, v = [], [], []
    for l, (cout, cin, k, _, _) in enumerate(LAYERS):
        s = spec[l] if l < 6 else (head or head_spec())
        wl = np.zeros((cout, cin, k, k), dtype=np.float32)
        wl[np.arange(cout), s["ci"], s["ky"], s["kx"]] = s["sign"]
        w.append(wl)
        m.append(np.zeros(cout, dtype=np.float32))
        v.append(np.full(cout, PROBE_VAR, dtype=np.float32))
    return w, m, v


def probe_map(n16, spec):
    """the layer-6 map of a spec by index arithmetic alone: n16 [B, 32, 32] the normalised patch in fp16 values
    -> [B, 8, 8, 128]; every layer is out[y, x, co] = max(sign in[s y + ky - 1, s x + kx - 1, ci], 0) with zeros
    outside the map"""
    a = np.asarray(n16, dtype=np.float64)[..., None]
    for l, (cout, _, _, stride, _) in enumerate(LAYERS[:6]):
        s = spec[l]
        side = a.shape[1] // stride
        ap = np.pad(a, ((0, 0), (1, 1), (1, 1), (0, 0)))
        y = stride * np.arange(side)[:, None, None] + s["ky"][None, None, :]
        x = stride * np.arange(side)[None, :, None] + s["kx"][None, None, :]
        a = np.maximum(ap[:, y, x, s["ci"][None, None, :]] * s["sign"], 0.0) + 0.0
    return a


def head_maps(B):
    """hand-made fp16 maps [B, 8, 8, 128]: integers 0 .. 250 that differ between neighbouring positions, channels
    and patches; patch 2 (when there is one) is the zero map"""
    b, y, x, c = np.meshgrid(np.arange(B), np.arange(8), np.arange(8), np.arange(128), indexing="ij")
    maps = ((31 * (8 * y + x) + 17 * c + 5 * b) % 251).astype(np.float16)
    if B > 2:
        maps[2] = 0
    return maps


def head_expected(maps, variant, head=None):
    """float64 descriptors of head_maps under the one-hot layer 7 (scale 1, shift 0: exact integers)"""
    s = head or head_spec()
    f = maps.astype(np.float64)[:, s["ky"], s["kx"], s["ci"]] * s["sign"]
    return normalise_output(f, variant)


# ---------------------------------------------------------------- patches that make each constant matter
EDGE_SEED = 20265
# group -> (the alteration of normalise_input it must expose, the variant it is about)
EDGE_GROUPS = ("hard_eps", "sos_eps", "offset", "huge", "ulp")


def _noise(rng):
    return rng.uniform(-1.0, 1.0, (32, 32))


def edge_patches():
    """{group: float32 [n, 32, 32]}
    hard_eps  s noise with the sample standard deviation at about 0.5e-6, 1e-6, 2e-6 (HardNet's + 1e-6)
    sos_eps   s noise with the variance at about 0.5e-5, 1e-5, 2e-5 (SOSNet's + 1e-5)
    offset    1e6 + integers in 0 .. 255: exact in float32; one-pass float32 statistics cancel
    huge      1e19 noise: every square is a float32, their sum is not
    ulp       0.5 everywhere but one pixel, one float32 ulp above"""
    rng = np.random.default_rng(EDGE_SEED)
    out = {}
    z = [_noise(rng) for _ in range(3)]
    out["hard_eps"] = np.stack([t * (s / t.std(ddof=1)) for t, s in zip(z, (0.5e-6, 1e-6, 2e-6))])
    z = [_noise(rng) for _ in range(3)]
    out["sos_eps"] = np.stack([t * np.sqrt(s / t.var()) for t, s in zip(z, (0.5e-5, 1e-5, 2e-5))])
    out["offset"] = 1e6 + np.floor(rng.uniform(0.0, 256.0, (2, 32, 32)))
    out["huge"] = 1e19 * np.stack([_noise(rng) for _ in range(2)])
    u = np.full((2, 32, 32), 0.5)
    u[0, 13, 21] = u[1, 0, 31] = np.nextafter(np.float32(0.5), np.float32(1.0))
    out["ulp"] = u
    return {g: a.astype(np.float32) for g, a in out.items()}


def normalise_input_altered(x, variant, how):
    """normalise_input with one constant or precision changed: 'no_eps' drops the variant's eps, 'n1024' /
    'n1023' swaps the divisor of the variance, 'f32_onepass' takes the variance as E[x^2] - E[x]^2 in float32,
    'f32_twopass' the mean and the centred sum of squares in float32 (numpy's pairwise sums)"""
    hard = variant == "hardnet"
    eps = 0.0 if how == "no_eps" else (1e-6 if hard else 1e-5)
    div = 1023.0 if hard else 1024.0
    if how in ("n1024", "n1023"):
        div = 1024.0 if hard else 1023.0
    if how == "f32_onepass":
        x32 = x.astype(np.float32)
        mean32 = x32.sum(axis=(1, 2), keepdims=True, dtype=np.float32) / np.float32(1024)
        ex2 = (x32 * x32).sum(axis=(1, 2), keepdims=True, dtype=np.float32) / np.float32(1024)
        with np.errstate(invalid="ignore", over="ignore"):
            ss = np.maximum((ex2 - mean32 * mean32).astype(np.float64), 0.0) * 1024.0
        mean = mean32.astype(np.float64)
    elif how == "f32_twopass":
        x32 = x.astype(np.float32)
        mean32 = x32.sum(axis=(1, 2), keepdims=True, dtype=np.float32) / np.float32(1024)
        d32 = x32 - mean32
        with np.errstate(over="ignore"):
            ss = (d32 * d32).sum(axis=(1, 2), keepdims=True, dtype=np.float32).astype(np.float64)
        mean = mean32.astype(np.float64)
    else:
        mean = x.mean(axis=(1, 2), keepdims=True)
        ss = ((x - mean) ** 2).sum(axis=(1, 2), keepdims=True)
    den = np.sqrt(ss / div) + eps if hard else np.sqrt(ss / div + eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (x - mean) / den


ALTERATIONS = ("no_eps", "n1024", "f32_onepass", "f32_twopass")
# what each group pins: (variant, alteration) pairs whose altered restatement must miss the float64 reference by
# more than 10 x the group's tolerance (asserted by the generator and by test_host_patchnet_edges.py)
EDGE_PINS = {
    "hard_eps": (("hardnet", "no_eps"), ("sosnet", "no_eps")),
    "sos_eps": (("sosnet", "no_eps"),),
    "offset": (("hardnet", "f32_onepass"), ("sosnet", "f32_onepass")),
    "huge": (("hardnet", "f32_twopass"), ("sosnet", "f32_twopass"), ("hardnet", "f32_onepass"), ("sosnet", "f32_onepass")),
    "ulp": (("hardnet", "no_eps"), ("sosnet", "no_eps")),
}


def quantised_net_altered(x, params, variant, how):
    """quantised_net's descriptors with normalise_input_altered in place of normalise_input"""
    global normalise_input
    keep = normalise_input
    normalise_input = lambda t, var: normalise_input_altered(t, var, how)   # noqa: E731
    try:
        return quantised_net(x, params, variant)[0]
    finally:
        normalise_input = keep


# ---------------------------------------------------------------- past the 65535-block cap
CAP = 65535
CAP_P = CAP + 70                     # trunk and fused entry: blocks 0 .. 69 take a second patch
CAP_HEAD_B = 16 * CAP + 37           # head: 65538 tiles of 16 maps, blocks 0 .. 2 take a second tile
assert CAP % 7 == 1


def cap_seven():
    """float32 [7, 32, 32]: zero, bright corner, constant, noise, near-constant, smoothed noise, values in 0 .. 255.
    Patch p of a capped batch is kind p mod 7 and block b's second patch is of kind (b + 1) mod 7, so in some
    block the bright corner follows the zero patch, the zero patch follows the 0 .. 255 patch (the largest
    values), the constant patch follows the bright corner and the near-constant patch follows noise."""
    x = patches()
    near = edge_patches()["hard_eps"][1]
    return np.stack([x[ZERO], x[3], x[CONSTANT], x[6], near, x[7], x[8]])


def cap_kinds(n):
    return np.arange(n, dtype=np.int64) % 7


# ---------------------------------------------------------------- non-finite patches
NONFINITE_AT = {0: "nan", 16: "+inf", 17: "-inf", 36: "all"}   # position in the batch -> what is wrong with the patch


def nonfinite_batch():
    """(float32 [37, 32, 32], the positions of the non-finite patches): the first 33 patches() with a NaN-pixel
    patch first, a +Inf-pixel and a -Inf-pixel patch in the middle and an all-NaN patch last"""
    fin = list(patches()[:33])
    src = patches()[40:44].copy()
    src[0, 5, 9] = np.nan
    src[1, 31, 0] = np.inf
    src[2, 0, 0] = -np.inf
    src[3] = np.nan
    out, k = [], 0
    for pos in range(37):
        if pos in NONFINITE_AT:
            out.append(src[list(NONFINITE_AT).index(pos)])
        else:
            out.append(fin[k])
            k += 1
    assert k == 33
    return np.stack(out).astype(np.float32), sorted(NONFINITE_AT)
