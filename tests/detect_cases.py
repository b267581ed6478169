"""Cases of the keypoint-detection tests: the case table, the input builders, a checksum and a
float64 numpy restatement of the rules include/rr.h states for rr_response, rr_nms2d and
rr_select_keypoints.  Shared by tests/golden/make_golden_detect.py (which compares the restatement
with the reference), tests/test_host_detect.py and tests/test_gpu_detect.py.
"""

import numpy as np

from oracle import data

TILE = 32   # side of k_response's tile (D_T in csrc/rr_detect.hip)

# (n, c, h, w): all border; tiny; odd sizes that are no multiple of the tile (image 1 is uniform
# noise); the gray path with n > 1; exactly one tile plus one row and one column
CASES = [(1, 1, 4, 4), (1, 1, 8, 8), (2, 1, 37, 53), (3, 3, 48, 64), (1, 1, TILE + 1, TILE + 1)]
GRAY_CASE = 3            # also scored as [n, 1, h, w] after the gray reduction
NOISE_CASE = 2
SEED = 4100
KINDS = ("harris", "gftt", "hessian")
HARRIS_K = 0.04
SIGMAS = (1.5, 2.25, 0.75)   # float32-exact; the first n of them scale a case's images in the sigma test

# selection cases: (response case, gray) whose golden harris maps feed nms2d / select_keypoints
SELECT_MAPS = [(NOISE_CASE, False), (GRAY_CASE, True)]
NMS_SIZES = (3, 5, 9)
SELECT_KS = 5
NUMS = (1, 64, 1024)     # 1024 exceeds ceil(48 / 2) * ceil(64 / 2) = 768, the most candidates of a map

# float32 values of the reference's get_gaussian_kernel1d(7, 1.0) (the generator asserts them)
GAUSS7 = np.array([float.fromhex(v) for v in ("0x1.228634p-8", "0x1.ba69e8p-5", "0x1.efb0bp-3", "0x1.98a0a2p-2",
                                              "0x1.efb0bp-3", "0x1.ba69e8p-5", "0x1.228634p-8")])
GXX = np.array([[-1, 0, 2, 0, -1], [-4, 0, 8, 0, -4], [-6, 0, 12, 0, -6], [-4, 0, 8, 0, -4], [-1, 0, 2, 0, -1]], dtype=np.float64)
GXY = np.array([[-1, -2, 0, 2, 1], [-2, -4, 0, 4, 2], [0, 0, 0, 0, 0], [2, 4, 0, -4, -2], [1, 2, 0, -2, -1]], dtype=np.float64)


def images(k, seed=None):
    """float32 [n, c, h, w] in [0, 1) of case k"""
    n, c, h, w = CASES[k]
    seed = SEED + 10 * k if seed is None else int(seed)
    x = data.structured_images(n, h, w, seed=seed)[:, :c]
    if k == NOISE_CASE:
        x[1] = np.random.default_rng(seed + 1).random((c, h, w)).astype(np.float32)
    return np.ascontiguousarray(x)


def to_u8(x):
    return np.clip(np.rint(x * 255.0), 0, 255).astype(np.uint8)


def checksum(*arrays):
    return np.array([np.asarray(a, dtype=np.float64).sum() for a in arrays], dtype=np.float64)


def gray(x):
    x = x.astype(np.float64)
    return ((0.299 * x[:, 0] + 0.587 * x[:, 1]) + 0.114 * x[:, 2])[:, None]


def _corr(p, kern):
    """valid correlation of padded planes [..., H + 2r, W + 2r] with kern [2r + 1, 2r + 1], rows then columns"""
    kh, kw = kern.shape
    h, w = p.shape[-2] - kh + 1, p.shape[-1] - kw + 1
    out = np.zeros(p.shape[:-2] + (h, w))
    for r in range(kh):
        for q in range(kw):
            if kern[r, q] != 0.0:
                out = out + kern[r, q] * p[..., r:r + h, q:q + w]
    return out


def response(x, kind, k=HARRIS_K, to_gray=False, sigmas=None):
    """float64 scores [n, c, h, w] ([n, 1, h, w] with to_gray) of float32 images by the rules of rr_response"""
    x = gray(x) if to_gray else x.astype(np.float64)
    pad = [(0, 0), (0, 0)]
    if kind == "hessian":
        p = np.pad(x, pad + [(2, 2), (2, 2)], mode="edge")
        dxx, dyy = _corr(p, GXX) / 64.0, _corr(p, GXX.T) / 64.0
        dxy = _corr(p, GXY) * np.float64(np.float32(1.0) / np.float32(36.0))
        s = dxx * dyy - dxy * dxy
    else:
        p = np.pad(x, pad + [(1, 1), (1, 1)], mode="edge")
        h, w = x.shape[-2:]
        a = lambda r, q: p[..., r:r + h, q:q + w]  # noqa: E731
        dx = ((a(0, 2) - a(0, 0)) + 2.0 * (a(1, 2) - a(1, 0)) + (a(2, 2) - a(2, 0))) * 0.125
        dy = ((a(2, 0) - a(0, 0)) + 2.0 * (a(2, 1) - a(0, 1)) + (a(2, 2) - a(0, 2))) * 0.125

        def blur(v):
            v = np.pad(v, pad + [(3, 3), (3, 3)], mode="reflect")
            hx = sum(GAUSS7[d] * v[..., :, d:d + w] for d in range(7))
            return sum(GAUSS7[d] * hx[..., d:d + h, :] for d in range(7))

        A, B, C = blur(dx * dx), blur(dy * dy), blur(dx * dy)
        det, tr = A * B - C * C, A + B
        s = det - k * (tr * tr) if kind == "harris" else 0.5 * (tr - np.sqrt(np.abs(tr * tr - 4.0 * det)))
    if sigmas is not None:
        sg = np.asarray(sigmas, dtype=np.float32).astype(np.float64)
        s = s * ((sg * sg) * (sg * sg))[:, None, None, None]
    return s


def nms_mask(x, ks):
    """bool mask of planes [..., h, w]: greater than 0 and than every other window position at
    clamped coordinates (so no edge pixel is kept); NaN never"""
    r = ks // 2
    h, w = x.shape[-2:]
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(r, r), (r, r)], mode="edge")
    with np.errstate(invalid="ignore"):
        keep = x > 0
        for dy in range(ks):
            for dx in range(ks):
                if dy == r and dx == r:
                    continue
                keep &= x > p[..., dy:dy + h, dx:dx + w]
    return keep


def select(score, ks, num, min_score=0.0, border=0):
    """score float32 [n, h, w] -> (kpts float32 [n, num, 2] (x, y), scores [n, num], count int32 [n])
    by (score desc, y * w + x asc); padding (-1, -1) and 0"""
    n, h, w = score.shape
    keep = nms_mask(score, ks)
    with np.errstate(invalid="ignore"):
        keep &= score > np.float32(min_score)
    inside = np.zeros((h, w), dtype=bool)
    inside[border:h - border, border:w - border] = True
    keep &= inside
    kpts = np.full((n, num, 2), -1.0, dtype=np.float32)
    scores = np.zeros((n, num), dtype=np.float32)
    count = np.zeros(n, dtype=np.int32)
    for b in range(n):
        idx = np.flatnonzero(keep[b])
        val = score[b].reshape(-1)[idx]
        order = np.lexsort((idx, -val.astype(np.float64)))[:num]
        m = len(order)
        count[b] = m
        kpts[b, :m, 0], kpts[b, :m, 1] = idx[order] % w, idx[order] // w
        scores[b, :m] = val[order]
    return kpts, scores, count


def candidate_bound(h, w):
    return ((h + 1) // 2) * ((w + 1) // 2)


def tie_map():
    """float32 [1, 24, 32]: a faint positive texture with three equal peaks, two equal peaks on the
    diagonal of one 5 x 5 window apart, a flat plateau (no strict maximum inside), a peak on the
    edge and a negative "peak" in a hole"""
    r = np.random.default_rng(SEED + 99)
    m = (r.random((24, 32)) * 0.01).astype(np.float32)
    for y, x in ((5, 20), (5, 5), (15, 9)):
        m[y, x] = 0.5
    m[10, 25] = m[13, 28] = 0.75     # 3 apart: both survive ks 3 and 5, neither survives ks 9
    m[18:22, 3:8] = 0.25
    m[0, 12] = 0.9
    m[8:13, 12:17] = -1.0
    m[10, 14] = -0.5
    return m[None]
