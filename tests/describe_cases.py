"""Cases of the keypoint-description tests: the case table, the input builders (images, frames and
planted patches from the repository's counter hash, no RNG state), a checksum and a float64 numpy
restatement of the rules include/rr.h states for rr_extract_patches, rr_patch_orientation,
rr_sift_describe and rr_describe_keypoints.  Shared by tests/golden/make_golden_describe.py (which
compares the restatement with the reference), tests/test_host_describe.py and
tests/test_gpu_describe.py.
"""

import numpy as np

from verify_cases import mix

PI32 = float(np.float32(3.14159265358979323846))   # the reference's pi tensor is float32
ORIENT_BINS = 36

# (ps, num_ang_bins, num_spatial_bins): the default; an odd size (ksize 16, stride 10, pad 4); 6 x 3 x 3
CONFIGS = [(32, 8, 4), (41, 8, 4), (24, 6, 3)]
MAIN = (2, 1, 40, 56)      # n, c, h, w
NPTS = 24
U8 = (1, 3, 33, 47)
U8_NPTS = 12
ROT = (1, 1, 48, 48)       # square: rotated by 90 degrees with an exact index permutation
ROT_NPTS = 10
ROT_SCALE = 7.0
SCALE = 6.0                # the scale of the kpts + scale form
SEED = 5200
# the one fused form whose restatement is held to tol instead of tol / 2 (given frames with orientation:
# the float32 rounding of the upright and of the turned frame, tests/golden/make_golden_describe.py)
FULL_TOL_FORM = "l1"
VARIANTS = [(False, 0.2), (True, 1.0), (False, 1.0)]   # (rootsift, clipval) beside the default (True, 0.2), on config 0


def uniform(seed, count):
    """count float64 values in [0, 1): the counter hash of tests/verify_cases.py on (seed, index)"""
    s = mix(np.uint64(int(seed) & 0xFFFFFFFF) + np.uint64(0x9E3779B9))
    v = mix(s + np.arange(count, dtype=np.uint64))
    v = mix(v ^ np.uint64(0x5BD1E995))
    return v.astype(np.float64) / 4294967296.0


def smooth_images(shape, seed):
    """float32 [n, c, h, w] in [0, 1]: hash noise smoothed by three 3 x 3 binomial passes (edge
    padding), stretched, plus a ramp, so that gradients are non-trivial everywhere"""
    n, c, h, w = shape
    x = uniform(seed, n * c * h * w).reshape(n, c, h, w)
    for _ in range(3):
        p = np.pad(x, [(0, 0), (0, 0), (1, 1), (1, 1)], mode="edge")
        x = (p[..., :-2, :] + 2.0 * p[..., 1:-1, :] + p[..., 2:, :]) * 0.25
        x = (x[..., :-2] + 2.0 * x[..., 1:-1] + x[..., 2:]) * 0.25
    x = (x - x.min()) / (x.max() - x.min())
    ramp = (np.arange(h)[:, None] / float(h) + 2.0 * np.arange(w)[None, :] / float(w)) / 3.0
    return np.ascontiguousarray((0.75 * x + 0.25 * ramp).astype(np.float32))


def to_u8(x):
    return np.clip(np.rint(x * 255.0), 0, 255).astype(np.uint8)


def frames(shape, npts, seed):
    """float32 [n, npts, 2, 3]: scales 4 .. 11 px, any rotation, mild anisotropy and shear; of every
    image, frames 0 - 3 have centres within 2 px of the left, right, top and bottom edge and frame 4
    lies outside the image"""
    n, _, h, w = shape
    u = uniform(seed + 1, n * npts * 6).reshape(n, npts, 6)
    s = 4.0 + 7.0 * u[..., 0]
    th = 2.0 * np.pi * u[..., 1]
    ar = 0.8 + 0.4 * u[..., 2]
    sh = 0.3 * (u[..., 3] - 0.5)
    cx, cy = 2.0 + (w - 4.0) * u[..., 4], 2.0 + (h - 4.0) * u[..., 5]
    cx[:, 0], cx[:, 1] = 2.0 * u[:, 0, 4], w - 2.0 * u[:, 1, 4]
    cy[:, 2], cy[:, 3] = 2.0 * u[:, 2, 5], h - 2.0 * u[:, 3, 5]
    cx[:, 4], cy[:, 4] = w + 3.0, -2.5
    c, sn = np.cos(th), np.sin(th)
    A = np.empty((n, npts, 2, 3))
    # (anisotropic scale, shear) . rotation
    A[..., 0, 0], A[..., 0, 1] = s * ar * c, s * ar * sn
    A[..., 1, 0], A[..., 1, 1] = s / ar * (sh * c - sn), s / ar * (sh * sn + c)
    A[..., 0, 2], A[..., 1, 2] = cx, cy
    return A.astype(np.float32)


def keypoints(shape, npts, seed, margin):
    """float32 [n, npts, 2] pixel (x, y), at least margin from every edge"""
    n, _, h, w = shape
    u = uniform(seed + 2, n * npts * 2).reshape(n, npts, 2)
    return np.stack([margin + (w - 2 * margin) * u[..., 0], margin + (h - 2 * margin) * u[..., 1]], axis=-1).astype(np.float32)


def planted_patches(ps):
    """float32 [3, ps, ps]: a flat patch (mag = sqrt(eps) everywhere, every ori on a bin edge), a pure
    ramp along x (one orientation holds all of the mass) and a ramp along -y"""
    j = np.arange(ps, dtype=np.float64)
    flat = np.full((ps, ps), 0.5)
    rx = np.broadcast_to(0.25 + 0.5 * j / ps, (ps, ps))
    ry = np.broadcast_to((0.75 - 0.5 * j / ps)[:, None], (ps, ps))
    return np.stack([flat, rx, ry]).astype(np.float32)


def scale_frames(kpts, scale):
    f = np.zeros(kpts.shape[:-1] + (2, 3), dtype=np.float32)
    f[..., 0, 0] = f[..., 1, 1] = np.float32(scale)
    f[..., 0, 2], f[..., 1, 2] = kpts[..., 0], kpts[..., 1]
    return f


def rot90_pair(img, kpts):
    """img [1, 1, s, s], kpts [1, N, 2] -> the image turned by 90 degrees (an exact index permutation)
    and the keypoints turned along: a point (X, Y), pixel centres at k + 0.5, goes to (Y, s - X)"""
    s = img.shape[-1]
    r = np.ascontiguousarray(np.rot90(img, k=1, axes=(2, 3)))
    k = np.stack([kpts[..., 1], np.float32(s) - kpts[..., 0]], axis=-1).astype(np.float32)
    return r, k


def checksum(*arrays):
    return np.array([np.asarray(a, dtype=np.float64).sum() for a in arrays], dtype=np.float64)


# ---------------------------------------------------------------- the restatement
def gray(x):
    x = x.astype(np.float64)
    return ((0.299 * x[:, 0] + 0.587 * x[:, 1]) + 0.114 * x[:, 2])[:, None]


def extract_patches(x, lafs, ps, to_gray=False):
    """x float32 [n, c, h, w], lafs float32 [n, N, 2, 3] -> float64 [n, N, c, ps, ps] (before the
    rounding to float32)"""
    x = gray(x) if to_gray else x.astype(np.float64)
    n, c, h, w = x.shape
    A = lafs.astype(np.float64)
    N = A.shape[1]
    t = (2.0 * np.arange(ps) + 1.0) / float(ps) - 1.0
    u, v = t[None, None, None, :], t[None, None, :, None]
    a = lambda r, q: A[:, :, r, q][:, :, None, None]  # noqa: E731
    sx = np.clip(((a(0, 0) * u + a(0, 1) * v) + a(0, 2)) - 0.5, 0.0, w - 1.0)
    sy = np.clip(((a(1, 0) * u + a(1, 1) * v) + a(1, 2)) - 0.5, 0.0, h - 1.0)
    bad = ~np.isfinite(A).all(axis=(2, 3))
    sx[bad], sy[bad] = 0.0, 0.0
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = sx - x0, sy - y0
    out = np.empty((n, N, c, ps, ps))
    for b in range(n):
        for ch in range(c):
            p = x[b, ch]
            out[b, :, ch] = ((p[y0[b], x0[b]] * ((1 - fx[b]) * (1 - fy[b])) + p[y0[b], x1[b]] * (fx[b] * (1 - fy[b])))
                             + p[y1[b], x0[b]] * ((1 - fx[b]) * fy[b])) + p[y1[b], x1[b]] * (fx[b] * fy[b])
    out[bad] = 0.0
    return out


def _soft_bins(o, mag, nb):
    """planes [B, nb, ps, ps] of the soft-binned orientation o >= 0 with weight mag"""
    f = np.floor(o)
    w1 = o - f
    b0 = np.mod(f, nb).astype(np.int64)
    b1 = np.mod(b0 + 1, nb)
    planes = np.zeros((o.shape[0], nb) + o.shape[1:])
    for a in range(nb):
        planes[:, a] = (b0 == a) * ((1.0 - w1) * mag) + (b1 == a) * (w1 * mag)
    return planes


def orientation_histogram(patches, nb=ORIENT_BINS):
    """float32 patches [B, ps, ps] -> the smoothed histogram [B, nb] (float64)"""
    p = np.pad(patches.astype(np.float64), [(0, 0), (1, 1), (1, 1)], mode="edge")
    ps = patches.shape[-1]
    a = lambda r, q: p[:, r:r + ps, q:q + ps]  # noqa: E731
    dx = ((a(0, 2) - a(0, 0)) + 2.0 * (a(1, 2) - a(1, 0)) + (a(2, 2) - a(2, 0))) * 0.125
    dy = ((a(2, 0) - a(0, 0)) + 2.0 * (a(2, 1) - a(0, 1)) + (a(2, 2) - a(0, 2))) * 0.125
    mag = np.sqrt((dx * dx + dy * dy) + 1e-8)
    ori = np.arctan2(dy, dx + 1e-8) + 2.0 * PI32
    hist = _soft_bins((nb * (ori + PI32)) / (2.0 * PI32), mag, nb).sum(axis=(2, 3)) / float(ps * ps)
    k0, k1 = float(np.float32(0.33)), float(np.float32(0.34))
    return (k0 * np.roll(hist, 1, axis=1) + k1 * hist) + k0 * np.roll(hist, -1, axis=1)


def patch_orientation(patches, nb=ORIENT_BINS):
    """float32 patches [B, ps, ps] -> float32 angles [B]"""
    idx = np.argmax(orientation_histogram(patches, nb), axis=1).astype(np.float64)   # the first maximum
    return (-(((2.0 * PI32) * idx) / float(nb) - PI32)).astype(np.float32)


def sift_geometry(ps, ns):
    ksize, stride = 2 * int(ps / (ns + 1)), ps // ns
    pad = ksize // 4
    if ksize < 1 or (ps + 2 * pad - (ksize - 1) - 1) // stride + 1 != ns:
        return None
    return ksize, stride, pad


def gaussian_window(ps):
    """float32-valued [ps, ps]: 1-D weights in float64, rounded to float32, multiplied in float32"""
    x = np.arange(ps) - ps // 2 + (0.0 if ps % 2 else 0.5)
    e = np.exp(-(x * x) / (float(ps) * float(ps)))
    g = (e / e.sum()).astype(np.float32)
    return np.outer(g, g).astype(np.float64)      # float32 outer product, then widened


def pooling_kernel(ksize):
    half = np.float32(ksize) * np.float32(0.5)
    xc = half - np.abs((np.arange(ksize, dtype=np.float32) + np.float32(0.5)) - half)
    return (np.outer(xc, xc) / (half * half)).astype(np.float64)   # float32 throughout


def sift_describe(patches, nb=8, ns=4, rootsift=True, clipval=0.2):
    """float32 patches [B, ps, ps] -> float64 descriptors [B, nb ns^2] (before the rounding)"""
    B, ps = patches.shape[0], patches.shape[-1]
    ksize, stride, pad = sift_geometry(ps, ns)
    p = np.pad(patches.astype(np.float64), [(0, 0), (1, 1), (1, 1)], mode="edge")
    gx = (p[:, 1:-1, 2:] - p[:, 1:-1, :-2]) * 0.5
    gy = (p[:, 2:, 1:-1] - p[:, :-2, 1:-1]) * 0.5
    mag = np.sqrt((gx * gx + gy * gy) + 1e-10) * gaussian_window(ps)[None]
    ori = np.arctan2(gy, gx + 1e-10) + 2.0 * PI32
    planes = _soft_bins((nb * ori) / (2.0 * PI32), mag, nb)
    big = ns * stride + ksize
    padded = np.zeros((B, nb, pad + big, pad + big))
    padded[:, :, pad:pad + ps, pad:pad + ps] = planes
    pk = pooling_kernel(ksize)
    out = np.zeros((B, nb, ns, ns))
    for cy in range(ns):
        for cx in range(ns):
            win = padded[:, :, cy * stride:cy * stride + ksize, cx * stride:cx * stride + ksize]
            out[:, :, cy, cx] = (win * pk).sum(axis=(2, 3))
    v = out.reshape(B, -1)
    v = v / np.maximum(np.sqrt((v * v).sum(1, keepdims=True)), 1e-12)
    v = np.clip(v, 0.0, clipval)
    v = v / np.maximum(np.sqrt((v * v).sum(1, keepdims=True)), 1e-12)
    if rootsift:
        v = np.sqrt(v / np.maximum(np.abs(v).sum(1, keepdims=True), 1e-12) + 1e-10)
    return v


def make_upright(lafs):
    """float32 [.., 2, 3] -> float32 upright frames, float64 arithmetic rounded once"""
    A = lafs.astype(np.float64)
    a00, a01, a10, a11 = A[..., 0, 0], A[..., 0, 1], A[..., 1, 0], A[..., 1, 1]
    det = np.sqrt(np.abs((a00 * a11 - a10 * a01) + 1e-10))
    b2a2 = np.sqrt(a01 * a01 + a00 * a00) + 1e-9
    U = np.zeros_like(A)
    U[..., 0, 0] = det * (b2a2 / det)
    U[..., 1, 0] = det * ((a11 * a01 + a10 * a00) / (b2a2 * det))
    U[..., 1, 1] = det * (det / b2a2)
    U[..., 2] = A[..., 2]
    return U.astype(np.float32)


def rotate_frames(upright, angles):
    """upright float32 [.., 2, 3] (a01 = 0), angles float32 [..] -> upright . [[c, s], [-s, c]], float32"""
    U = upright.astype(np.float64)
    c, s = np.cos(angles.astype(np.float64)), np.sin(angles.astype(np.float64))
    F = U.copy()
    F[..., 0, 0], F[..., 0, 1] = U[..., 0, 0] * c, U[..., 0, 0] * s
    F[..., 1, 0], F[..., 1, 1] = U[..., 1, 0] * c - U[..., 1, 1] * s, U[..., 1, 0] * s + U[..., 1, 1] * c
    return F.astype(np.float32)


def describe_keypoints(x, kpts=None, count=None, scale=SCALE, lafs=None, orient=False, ps=32, nb=8, ns=4, rootsift=True,
                       clipval=0.2):
    """the fused entry as the chain of the three: (desc float64 [n, N, dim], angles float32 [n, N],
    frames float32 [n, N, 2, 3])"""
    to_gray = x.shape[1] == 3
    F = scale_frames(kpts, scale) if lafs is None else lafs.astype(np.float32)
    n, N = F.shape[:2]
    angles = np.zeros((n, N), dtype=np.float32)
    if orient:
        U = F if lafs is None else make_upright(F)
        P = extract_patches(x, U, ps, to_gray).astype(np.float32)[:, :, 0]
        angles = patch_orientation(P.reshape(n * N, ps, ps)).reshape(n, N)
        F = rotate_frames(U, angles)
    P = extract_patches(x, F, ps, to_gray).astype(np.float32)[:, :, 0]
    desc = sift_describe(P.reshape(n * N, ps, ps), nb, ns, rootsift, clipval).reshape(n, N, -1)
    dead = (F[..., 0, 2] == -1) & (F[..., 1, 2] == -1)
    if count is not None:
        dead |= np.arange(N)[None, :] >= np.asarray(count)[:, None]
    desc[dead], angles[dead], F = 0.0, 0.0, F.copy()
    F[dead] = 0.0
    return desc, angles, F
