"""Inputs and a numpy restatement of the learned patch descriptors (HardNet, SOSNet), numpy only.

Seeded weights and patches, the state-dict layout of the two reference modules, and quantised_net: the
arithmetic that include/rr.h states for rr_patchnet_trunk / rr_patchnet_head -- fp16 at the stated
rounding points (weights, the normalised patch, every layer's output of layers 1 .. 6), everything
else in float64.  tests/golden/make_golden_patchnet.py compares it with the reference modules in
float64 and derives the tolerances of tests/golden/patchnet.npz from that difference.
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
