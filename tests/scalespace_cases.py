"""Cases of the scale-space detection tests: the case table, the input builders and a float64 numpy
restatement of the rules include/rr.h states for rr_gaussian_blur, rr_scale_pyramid,
rr_dog_response, rr_scale_space_extrema and rr_scale_space_select.  Shared by
tests/golden/make_golden_scalespace.py (which compares the restatement with the reference),
tests/test_host_scalespace.py and tests/test_gpu_scalespace.py.
"""

import math

import numpy as np

import detect_cases as DC

LEVELS, SIGMA, MIN_SIZE = 3, 1.6, 15
L = LEVELS + 3

# (n, c, h, w): two octaves, 40 x 56 and 20 x 28, the kernel cap active in the second; odd sizes, the
# second octave 18 x 26; the gray path as uint8; one octave whose frames are all outside with
# mr_size = 6 (count 0); planted Gaussian blobs, three octaves
CASES = [(2, 1, 40, 56), (2, 1, 37, 53), (1, 3, 48, 64), (1, 1, 24, 30), (1, 1, 96, 128)]
U8_CASE, EMPTY_CASE, BLOB_CASE = 2, 3, 4
PYRAMID_CASES = (0, 1, 2, 3)       # the fixture holds these pyramids level by level
SEED = 4200
BLUR_SIZES = ((11, 1.226273498465408), (25, 3.090015587289592))   # gaussian_blur2d alone, on case 1

# list cases: (case, response, mr_size, minima, N)
LISTS = [(0, "hessian", 1.0, False, 64), (1, "hessian", 1.0, False, 64), (U8_CASE, "hessian", 1.0, False, 64),
         (EMPTY_CASE, "hessian", 6.0, False, 16), (BLOB_CASE, "dog", 2.0, True, 16), (BLOB_CASE, "hessian", 2.0, False, 16)]
RESP_LIST = 0                      # the fixture holds this list's float32 response volumes
SMALL_NUMS = (1, 4)
BONUS = 10.0                       # ConvQuadInterp3d(10.0) of the generator

# float32 values of sin and cos of the float32 linspace(0, 2 pi, 11) (the generator asserts them)
SIN11 = np.array([float.fromhex(v) for v in (
    "0x0.0p+0", "0x1.2cf23p-1", "0x1.e6f0e2p-1", "0x1.e6f0ep-1", "0x1.2cf22ep-1", "-0x1.777a5cp-24", "-0x1.2cf234p-1",
    "-0x1.e6f0ep-1", "-0x1.e6f0ep-1", "-0x1.2cf226p-1", "0x1.777a5cp-23")])
COS11 = np.array([float.fromhex(v) for v in (
    "0x1.0p+0", "0x1.9e377ap-1", "0x1.3c6ef2p-2", "-0x1.3c6ef6p-2", "-0x1.9e377ap-1", "-0x1.0p+0", "-0x1.9e3778p-1",
    "-0x1.3c6efap-2", "0x1.3c6efcp-2", "0x1.9e3782p-1", "0x1.0p+0")])


def blobs(seed):
    """(float32 [1, 1, 96, 128] in (0, 1), [(x, y, sigma, sign)]): twelve Gaussian blobs, one per 32 x 32
    cell, centres at sub-pixel positions, on a smooth texture a hundredth of their height (a flat ground
    gives the difference of Gaussians extrema of rounding noise).  Their sigmas, 2.3 to 3.2, lie inside
    the scales of the first octave's interior levels, 2.0 to 3.6."""
    r = np.random.default_rng(seed)
    h, w = CASES[BLOB_CASE][2:]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 0.5 + 0.003 * np.sin(0.23 * xx + 0.4) * np.sin(0.31 * yy + 1.1) + 0.002 * np.sin(0.11 * xx - 0.17 * yy)
    planted = []
    for cy in range(3):
        for cx in range(4):
            x, y = 16 + 32 * cx + r.uniform(-4, 4), 16 + 32 * cy + r.uniform(-4, 4)
            s, sign = r.uniform(2.3, 3.2), (1.0 if (cx + cy) % 2 == 0 else -1.0)
            img += sign * r.uniform(0.25, 0.4) * np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / (2 * s * s))
            planted.append((x, y, s, sign))
    return img.astype(np.float32)[None, None], planted


def images(k, seed=None):
    """float32 [n, c, h, w] in [0, 1) of case k (the uint8 case: the float32 values v / 255 of its bytes)"""
    n, c, h, w = CASES[k]
    seed = SEED + 10 * k if seed is None else int(seed)
    if k == BLOB_CASE:
        return blobs(seed)[0]
    x = np.random.default_rng(seed).random((n, c, h, w)).astype(np.float32)
    if k == U8_CASE:
        x = DC.to_u8(x).astype(np.float32) / np.float32(255.0)
    return np.ascontiguousarray(x)


def as_u8(x):
    """the bytes of a uint8 case's float32 image"""
    return np.rint(x.astype(np.float64) * 255.0).astype(np.uint8)


# ---------------------------------------------------------------- pyramid
def taps(ks, sigma):
    """float32 values (as float64) of get_gaussian_kernel1d(ks, sigma): exp in float64, sum ascending"""
    e = [math.exp(-(float(i - ks // 2) * float(i - ks // 2)) / (2.0 * sigma * sigma)) for i in range(ks)]
    s = 0.0
    for v in e:
        s += v
    return np.array([np.float32(v / s) for v in e], dtype=np.float64)


def blur(x, ks, sigma):
    """float64 planes [..., h, w] blurred along x, then along y, taps ascending, reflect borders"""
    t = taps(ks, sigma)
    p = ks // 2
    h, w = x.shape[-2:]
    v = np.pad(x.astype(np.float64), [(0, 0)] * (x.ndim - 2) + [(p, p), (p, p)], mode="reflect")
    hx = np.zeros(v.shape[:-1] + (w,))
    for d in range(ks):
        hx = hx + t[d] * v[..., :, d:d + w]
    out = np.zeros(x.shape)
    for d in range(ks):
        out = out + t[d] * hx[..., d:d + h, :]
    return out


def kernel_size(s):
    ks = int(2.0 * 4.0 * s + 1.0)
    return ks + 1 if ks % 2 == 0 else ks


def plan(h, w, levels=LEVELS, sigma=SIGMA, min_size=MIN_SIZE):
    """(first blur (ksize, sigma) or None, [octave dict(h, w, sigmas [L], blurs [L - 1] of (ksize, sigma))])"""
    step = 2 ** (1. / float(levels))
    cur, first = 0.5, None
    if sigma > cur:
        s0 = max(math.sqrt(sigma ** 2 - cur ** 2), 0.01)
        first, cur = (kernel_size(s0), s0), sigma
    octs = []
    while True:
        o = dict(h=h, w=w, sigmas=[cur], blurs=[])
        for _ in range(1, levels + 3):
            s = cur * math.sqrt(step ** 2 - 1.0)
            ks = min(kernel_size(s), min(h, w))
            ks = ks + 1 if ks % 2 == 0 else ks
            cur *= step
            o["sigmas"].append(cur)
            o["blurs"].append((ks, s))
        octs.append(o)
        h, w, cur = h // 2, w // 2, sigma
        if min(h, w) <= min_size:
            return first, octs


def pyramid(x, levels=LEVELS, sigma=SIGMA, min_size=MIN_SIZE):
    """x float32 [n, 1|3, h, w] -> ([float64 [n, L, h_o, w_o] per octave], octaves of plan()); each level
    is blurred from the unrounded level before"""
    n, c, h, w = x.shape
    g = DC.gray(x)[:, 0] if c == 3 else x[:, 0].astype(np.float64)
    first, octs = plan(h, w, levels, sigma, min_size)
    cur = blur(g, *first) if first else g
    out = []
    for i, o in enumerate(octs):
        lv = [cur]
        for ks, s in o["blurs"]:
            lv.append(blur(lv[-1], ks, s))
        out.append(np.stack(lv, axis=1))
        if i + 1 < len(octs):
            cur = lv[-3][:, 0:2 * (o["h"] // 2):2, 0:2 * (o["w"] // 2):2]
    return out, octs


def responses(pyr, octs, kind):
    """float32 volumes [n, L - 1, h_o, w_o] per octave from the float32 levels"""
    out = []
    for lv, o in zip(pyr, octs):
        lv = lv.astype(np.float32)
        n, nl, h, w = lv.shape
        if kind == "dog":
            out.append(lv[:, 1:] - lv[:, :-1])
        else:
            sg = np.tile(np.array(o["sigmas"], dtype=np.float32), n)
            r = DC.response(lv.reshape(n * nl, 1, h, w), kind, DC.HARRIS_K, False, sg)
            out.append(r.reshape(n, nl, h, w)[:, :-1].astype(np.float32))
    return out


# ---------------------------------------------------------------- extrema
def extrema_mask(v, minima=False):
    """uint8 [n, D, h, w]: 1 where v > 0 and v > its 26 neighbours at clamped coordinates, 2 (minima)
    where the same holds for -v; NaN never"""
    def peaks(x):
        D, h, w = x.shape[-3:]
        p = np.pad(x, [(0, 0)] * (x.ndim - 3) + [(1, 1)] * 3, mode="edge")
        with np.errstate(invalid="ignore"):
            keep = x > 0
            for dd in range(3):
                for dy in range(3):
                    for dx in range(3):
                        if (dd, dy, dx) != (1, 1, 1):
                            keep &= x > p[..., dd:dd + D, dy:dy + h, dx:dx + w]
        return keep
    m = peaks(v).astype(np.uint8)
    if minima:
        m[peaks(-v)] = 2
    return m


def solve3(A, b):
    """-A^-1 b by elimination with partial pivoting (lower row on equal pivots), or None"""
    A = [[float(v) for v in row] for row in A]
    b = [float(v) for v in b]
    for c in range(3):
        pv = c
        for r in range(c + 1, 3):
            if abs(A[r][c]) > abs(A[pv][c]):
                pv = r
        if not abs(A[pv][c]) > 0.0:
            return None
        if pv != c:
            A[c], A[pv] = A[pv], A[c]
            b[c], b[pv] = b[pv], b[c]
        for r in range(c + 1, 3):
            f = A[r][c] / A[c][c]
            for k in range(c, 3):
                A[r][k] -= f * A[c][k]
            b[r] -= f * b[c]
    x = [0.0, 0.0, 0.0]
    x[2] = b[2] / A[2][2]
    x[1] = (b[1] - A[1][2] * x[2]) / A[1][1]
    x[0] = ((b[0] - A[0][1] * x[1]) - A[0][2] * x[2]) / A[0][0]
    x = [-v for v in x]
    return x if all(math.isfinite(v) for v in x) else None


def refine(vol, d, y, x, sign=1.0):
    """vol float32 [D, h, w], an interior voxel -> ((ox, oy, os), value) in float64"""
    p = lambda dd, dy, dx: sign * float(vol[d + dd, y + dy, x + dx])  # noqa: E731
    c = p(0, 0, 0)
    g = [0.5 * (p(0, 0, 1) - p(0, 0, -1)), 0.5 * (p(0, 1, 0) - p(0, -1, 0)), 0.5 * (p(-1, 0, 0) - p(1, 0, 0))]
    dxx = (p(0, 0, -1) + p(0, 0, 1)) - 2.0 * c
    dyy = (p(0, -1, 0) + p(0, 1, 0)) - 2.0 * c
    dss = (p(-1, 0, 0) + p(1, 0, 0)) - 2.0 * c
    dxy = 0.25 * (((p(0, -1, -1) - p(0, -1, 1)) - p(0, 1, -1)) + p(0, 1, 1))
    dys = 0.25 * (((p(-1, 1, 0) - p(-1, -1, 0)) + p(1, -1, 0)) - p(1, 1, 0))
    dxs = 0.25 * (((p(-1, 0, 1) - p(-1, 0, -1)) + p(1, 0, -1)) - p(1, 0, 1))
    off = solve3([[dxx, dxy, dxs], [dxy, dyy, dys], [dxs, dys, dss]], g)
    if off is None or max(abs(v) for v in off) > 0.7:
        off = [0.0, 0.0, 0.0]
    return off, c + 0.5 * ((g[0] * off[0] + g[1] * off[1]) + g[2] * off[2])


def extrema(v, minima=False):
    """the dense outputs of rr_scale_space_extrema: (mask uint8 [n, D, h, w], offsets float32
    [n, 3, D, h, w] in the order (level, x, y), values float32 [n, D, h, w])"""
    m = extrema_mask(v, minima)
    offs = np.zeros((v.shape[0], 3) + v.shape[1:], dtype=np.float32)
    vals = v.astype(np.float32).copy()
    for b, d, y, x in zip(*np.nonzero(m)):
        off, val = refine(v[b], d, y, x, 1.0 if m[b, d, y, x] == 1 else -1.0)
        offs[b, :, d, y, x] = (off[2], off[0], off[1])
        vals[b, d, y, x] = val
    return m, offs, vals


def frame(o, d, y, x, off, levels, mr):
    """((a, cx, cy) in octave pixels, inside) of a refined voxel of octave o"""
    a = mr * (o["sigmas"][0] * float(np.exp2((d + off[2]) / float(levels))))
    cx, cy = x + off[0], y + off[1]
    px, py = a * SIN11 + cx, a * COS11 + cy
    inside = (0.0 <= cx <= o["w"] and 0.0 <= cy <= o["h"] and (px >= 0).all() and (px <= o["w"]).all()
              and (py >= 0).all() and (py <= o["h"]).all())
    return (a, cx, cy), bool(inside)


def select(vols, octs, H, W, num, mr, minima=False, levels=LEVELS):
    """vols: float32 [n, D, h_o, w_o] per octave -> (lafs float32 [n, num, 2, 3], scores [n, num], count
    int32 [n], voxels: per image the selected (octave, voxel index, (ox, oy, os)) in order)"""
    n = vols[0].shape[0]
    lafs = np.zeros((n, num, 2, 3), dtype=np.float32)
    scores = np.zeros((n, num), dtype=np.float32)
    count = np.zeros(n, dtype=np.int32)
    voxels = []
    masks = [extrema_mask(v, minima) for v in vols]
    for b in range(n):
        cand = []
        for oi, (v, o, m) in enumerate(zip(vols, octs, masks)):
            for d, y, x in zip(*np.nonzero(m[b])):
                off, val = refine(v[b], d, y, x, 1.0 if m[b, d, y, x] == 1 else -1.0)
                (a, cx, cy), inside = frame(o, d, y, x, off, levels, mr)
                if inside:
                    mo = float(min(o["h"], o["w"]))
                    laf = ((a / mo) * float(min(H, W)), (cx * (1.0 / o["w"])) * W, (cy * (1.0 / o["h"])) * H)
                    cand.append((-float(np.float32(val)), oi, int((d * o["h"] + y) * o["w"] + x), laf, off))
        cand.sort(key=lambda e: e[:3])
        cand = cand[:num]
        count[b] = len(cand)
        for i, (s, oi, idx, laf, off) in enumerate(cand):
            lafs[b, i] = [[laf[0], 0.0, laf[1]], [0.0, laf[0], laf[2]]]
            scores[b, i] = -s
        voxels.append([(oi, idx, tuple(off)) for _, oi, idx, _, off in cand])
    return lafs, scores, count, voxels


def detect(x, kind, num, mr, minima=False):
    """the whole restatement: float32 images -> select(...)"""
    pyr, octs = pyramid(x)
    return select(responses(pyr, octs, kind), octs, x.shape[2], x.shape[3], num, mr, minima)


def candidate_bound(octs, D=L - 1):
    return sum(2 * ((D + 1) // 2) * ((o["h"] + 1) // 2) * ((o["w"] + 1) // 2) for o in octs)


def check_blobs(lafs, voxels, planted, octs):
    """asserts that every planted blob has a keypoint of lafs [N, 2, 3] (with their (octave, voxel, offsets))
    within a pixel, refined toward its centre on each axis"""
    W = octs[0]["w"]
    for bx, by, _, _ in planted:
        d2 = (lafs[:, 0, 2] - bx) ** 2 + (lafs[:, 1, 2] - by) ** 2
        i = int(np.argmin(d2))
        assert d2[i] < 1.0, (bx, by, lafs[i])
        oi, idx, off = voxels[i]
        if not any(off):
            continue   # an offset above 0.7 was dropped: the keypoint stays on its voxel
        o = octs[oi]
        sx = W / o["w"]
        vx, vy = (idx % o["w"]) * sx, (idx // o["w"] % o["h"]) * sx
        # a quadratic through samples one pixel apart of a blob of sigma >= 2 pixels finds its peak to
        # well under a third of a pixel; an x offset that lands on y (and y on x) is off by up to 1.4.
        # Where the voxel itself is farther than that from the centre, the refinement moves toward it.
        for got, vox, true in ((lafs[i, 0, 2], vx, bx), (lafs[i, 1, 2], vy, by)):
            assert abs(got - true) < 0.3 * sx, (bx, by, lafs[i])
            assert abs(vox - true) <= 0.3 * sx or abs(got - true) < abs(vox - true), (bx, by, lafs[i])


# ---------------------------------------------------------------- planted volume
def _quad_block(ustar, c=10.0):
    """27 samples of c - 0.5 (n - u*)^T M (n - u*) + 0.5 u*^T M u*: the centre is the strict maximum of
    the block and the refinement's offset is u* up to rounding"""
    M = np.array([[1.0, -1.5, 0.0], [-1.5, 4.0, 0.0], [0.0, 0.0, 2.0]])   # (x, y, s)
    u = np.array(ustar)
    blk = np.zeros((3, 3, 3))
    for ds in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                # the level axis of the reference's taps is flipped: a positive s offset points at d - 1
                nv = np.array([dx, dy, -ds], dtype=np.float64)
                blk[ds + 1, dy + 1, dx + 1] = c - 0.5 * (nv - u) @ M @ (nv - u) + 0.5 * u @ M @ u
    return blk


PLANTED_BELOW, PLANTED_ABOVE = (2, 4, 4), (2, 4, 12)   # (d, y, x) of the two quadratic blocks' centres


def planted_volume():
    """float32 [1, 5, 20, 24]: a faint positive texture with two equal neighbouring peaks, a plateau, a
    peak on each of the six faces, a negative hole with a peak of -0.5 in it, and two quadratic blocks
    whose x offsets are 0.69 and 0.71"""
    r = np.random.default_rng(SEED + 99)
    v = (r.random((5, 20, 24)) * 0.01).astype(np.float64)
    v[2, 10, 5] = v[2, 10, 6] = 0.5                 # equal neighbours: neither is strict
    v[1:4, 14:17, 3:6] = 0.25                       # plateau
    for d, y, x in ((0, 9, 12), (4, 9, 12), (2, 0, 12), (2, 19, 12), (2, 9, 0), (2, 9, 23)):
        v[d, y, x] = 0.9                            # faces
    v[1:4, 12:17, 16:21] = -1.0
    v[2, 14, 18] = -1.5                             # a strict minimum (kept with minima only)
    v[2, 10, 20] = 0.7                              # an ordinary interior peak
    for (d, y, x), ox in ((PLANTED_BELOW, 0.69), (PLANTED_ABOVE, 0.71)):
        v[d - 1:d + 2, y - 1:y + 2, x - 1:x + 2] = _quad_block((ox, 0.2, 0.0))
    return v.astype(np.float32)[None]
