"""Cases of the affine-shape tests: shapes, seeded inputs and a float64 numpy restatement of the
rules include/rr.h states for rr_patch_affine_shape, rr_ellipse_to_laf and rr_laf_affine_shape.
Shared by tests/golden/make_golden_affine.py (which compares the restatement with the reference),
tests/test_host_affine.py and tests/test_gpu_affine.py.  Images, frames, the upright frame and the
pyramid patches are those of tests/describe_cases.py and tests/pyrpatch_cases.py.
"""

import numpy as np

import describe_cases as QC
import pyrpatch_cases as PC

EPS = 1e-10                  # PatchAffineShapeEstimator's default
BAND = (EPS / 2, 2 * EPS)    # no raw moment of the fixture lies in here: the degenerate rule is decided alike in every precision
TOL_CAP = 1e-5
SEED = 8100

# rr_patch_affine_shape: fewer pixels than lanes, an odd size, the default of the LAF module, 16 pixels per lane
PATCH_PS = (8, 19, 32, 64)
PATCH_B = 7
PATCH_FLAT = (3, 5)          # the patches of 1e-3 of the contrast: degenerate at every size
ELLIPSES = 16

# rr_laf_affine_shape on the stratified frames of pyrpatch_cases (levels 0 .. past the last): name, image, ps, uint8
FUSED = [("m16", PC.MAIN, 16, False), ("m32", PC.MAIN, 32, False), ("c16", PC.COLOR, 16, True)]
NPTS = PC.NPTS
DIM = ("m32", 1e-3)          # the image of a fused case times 1e-3: every frame falls under the threshold

# analytic images of 96 x 128 under circular frames at PS 32
FLAT = (1, 1, 96, 128)
FLAT_PS = 32
BLOBS = [(6.0, 6.0), (12.0, 6.0), (6.0, 12.0)]     # (sigma_x, sigma_y) px
BLOB_SCALE = 12.0
DEGENERATE = ("constant", "ramp", "edge")
DEG_SCALES = (12.0, 24.0)    # level 0 and level 1; float32 values, so that the circle's scale is exact
DEG_NPTS = 8

E2E = PC.E2E
E2E_SEED = PC.E2E_SEED


def patches(ps, seed):
    """float32 [PATCH_B, ps, ps] in [0, 1]: hash noise of amplitude 0.3 plus diagonal stripes of amplitude
    0.2 (patch k along x + y or x - y: b is of either sign and of the size of a and c), strong enough
    for the raw moments to clear eps at PS 64 (where the window is of order 1 / 64^2); patches
    PATCH_FLAT have the contrast 1e-3 of that and fall under it at every size"""
    u = QC.uniform(seed + ps, PATCH_B * ps * ps).reshape(PATCH_B, ps, ps)
    y, x = np.arange(ps)[None, :, None], np.arange(ps)[None, None, :]
    sign = np.where(np.arange(PATCH_B) % 2, -1.0, 1.0)[:, None, None]
    p = 0.3 * (u - 0.5) + 0.2 * np.sin(0.9 * (x + sign * y))
    p[list(PATCH_FLAT)] *= 1e-3
    return (0.5 + p).astype(np.float32)


def ellipses(seed):
    """float32 [1, ELLIPSES, 5] = (x, y, a, b, c): positive definite, a and c in [0.2, 1], |b| <= 0.8 sqrt(a c)"""
    u = QC.uniform(seed + 5, ELLIPSES * 5).reshape(1, ELLIPSES, 5)
    a, c = 0.2 + 0.8 * u[..., 2], 0.2 + 0.8 * u[..., 4]
    b = 1.6 * (u[..., 3] - 0.5) * np.sqrt(a * c)
    return np.stack([130.0 * u[..., 0], 96.0 * u[..., 1], a, b, c], axis=-1).astype(np.float32)


def _binomial(g):
    p = np.pad(g, [(0, 0), (0, 0), (1, 1), (1, 1)], mode="edge")
    g = (p[..., :-2, :] + 2.0 * p[..., 1:-1, :] + p[..., 2:, :]) * 0.25
    return (g[..., :-2] + 2.0 * g[..., 1:-1] + g[..., 2:]) * 0.25


def contrast_images(shape, seed):
    """float32 [n, c, h, w] in [0, 1], two-valued with soft edges: hash noise on grids of pitch 2, 4 and
    8 px (as pyrpatch_cases.coarse_images: repeated to pixels, smoothed by pitch / 2 binomial passes,
    stretched, summed), cut at its median into 0 / 1 and smoothed by one 3 x 3 binomial pass.
    The window of the shape estimator is of order 1 / PS^2 and enters the moments squared: at PS 32 the raw
    moments of coarse_images itself are 6e-12 .. 1e-9, around eps = 1e-10, and a fixture on it would
    test on which side of the threshold a rounding falls.  Edges of full contrast at every pyramid
    level put the moments of a patch that holds an edge at 1e-9 .. 1e-7 and leave a patch that
    holds none at rounding noise, so that a seed exists for which no moment lies within a factor
    2 of eps."""
    n, c, h, w = shape
    x = np.zeros(shape)
    for k, pitch in enumerate((2, 4, 8)):
        hh, ww = -(-h // pitch), -(-w // pitch)
        g = QC.uniform(seed + 31 * (k + 1), n * c * hh * ww).reshape(n, c, hh, ww)
        g = np.repeat(np.repeat(g, pitch, axis=2), pitch, axis=3)[..., :h, :w]
        for _ in range(pitch // 2):
            g = _binomial(g)
        x += (g - g.min()) / (g.max() - g.min())
    return np.ascontiguousarray(_binomial((x > np.median(x)).astype(np.float64)).astype(np.float32))


def fused_inputs(k, seed):
    """(image float32 [n, c, h, w] in [0, 1] -- for a uint8 case the values v / 255 of the uint8 image,
    which to_u8 turns back exactly --, frames float32 [n, NPTS, 2, 3])"""
    name, shape, ps, u8 = FUSED[k]
    x = contrast_images(shape, seed)
    if u8:
        x = QC.to_u8(x).astype(np.float32) / np.float32(255.0)
    return x, PC.frames(shape, NPTS, seed)


def blob(sx, sy):
    """float32 [1, 1, 96, 128]: exp(-(dx^2 / (2 sx^2) + dy^2 / (2 sy^2))) about the image centre, pixel centres at k + 0.5"""
    _, _, h, w = FLAT
    dy = (np.arange(h) + 0.5 - h / 2.0)[:, None]
    dx = (np.arange(w) + 0.5 - w / 2.0)[None, :]
    return np.exp(-(dx * dx / (2.0 * sx * sx) + dy * dy / (2.0 * sy * sy))).astype(np.float32)[None, None]


def blob_frame():
    _, _, h, w = FLAT
    return QC.scale_frames(np.array([[[w / 2.0, h / 2.0]]], dtype=np.float32), BLOB_SCALE)


def degenerate_image(kind):
    """float32 [1, 1, 96, 128]: a constant, a pure ramp along x, a vertical step edge.  The ramp rises
    by 0.5 over the width: its raw moment a is 8e-12 at scale 12 and 3.2e-11 at scale 24, below the band
    around eps (all three moments are small); a frame across the edge has a of 1e-8 with b = c = 0."""
    _, _, h, w = FLAT
    j = np.arange(w, dtype=np.float64)
    row = {"constant": np.full(w, 0.5), "ramp": 0.25 + 0.5 * j / w, "edge": (j >= w // 2).astype(np.float64)}[kind]
    return np.ascontiguousarray(np.broadcast_to(row, (h, w))).astype(np.float32)[None, None]


def degenerate_frames():
    """float32 [1, DEG_NPTS, 2, 3]: circles, the first half of scale 12 (level 0), the rest of scale 24 (level 1)"""
    kp = QC.keypoints(FLAT, DEG_NPTS, SEED + 9, 2.0)
    fr = QC.scale_frames(kp, DEG_SCALES[0])
    fr[:, DEG_NPTS // 2:, 0, 0] = fr[:, DEG_NPTS // 2:, 1, 1] = np.float32(DEG_SCALES[1])
    return fr


def input_scale(lafs):
    """float64 [..]: sqrt|det + 1e-10| of float32 frames, what every comparison divides the 2 x 2 part by"""
    A = lafs.astype(np.float64)
    return np.sqrt(np.abs((A[..., 0, 0] * A[..., 1, 1] - A[..., 1, 0] * A[..., 0, 1]) + 1e-10))


def normalised(out, lafs):
    """the 2 x 2 parts [.., 2, 2] of frames `out` over the scale of the input frames `lafs`, float64"""
    return np.asarray(out, dtype=np.float64)[..., :2] / input_scale(lafs)[..., None, None]


# ---------------------------------------------------------------- the restatement
def raw_moments(p):
    """float32 patches [B, ps, ps] -> float64 [B, 3]: mean(gx^2), mean(gx gy), mean(gy^2) of the
    Sobel / 8 gradients times the float32-valued Gaussian window of sigma = ps / sqrt 2"""
    ps = p.shape[-1]
    q = np.pad(p.astype(np.float64), [(0, 0), (1, 1), (1, 1)], mode="edge")
    a = lambda r, c: q[:, r:r + ps, c:c + ps]  # noqa: E731
    dx = ((a(0, 2) - a(0, 0)) + 2.0 * (a(1, 2) - a(1, 0)) + (a(2, 2) - a(2, 0))) * 0.125
    dy = ((a(2, 0) - a(0, 0)) + 2.0 * (a(2, 1) - a(0, 1)) + (a(2, 2) - a(0, 2))) * 0.125
    G = QC.gaussian_window(ps)[None]
    gx, gy = dx * G, dy * G
    n = float(ps * ps)
    return np.stack([(gx * gx).sum(axis=(1, 2)) / n, (gx * gy).sum(axis=(1, 2)) / n, (gy * gy).sum(axis=(1, 2)) / n], axis=1)


def patch_affine_shape(p, eps=EPS):
    """float32 patches [B, ps, ps] -> float64 [B, 3] (before the rounding): the degenerate rule on
    the raw moments, then the division by the largest"""
    m = raw_moments(p)
    bad = (m < eps).sum(axis=1) >= 2
    m[bad] = (1.0, 0.0, 1.0)
    return m / m.max(axis=1, keepdims=True)


def ellipse_to_laf(ells):
    """float32 ellipses [.., 5] -> float64 frames [.., 2, 3] (before the rounding)"""
    e = ells.astype(np.float64)
    a11, a22 = np.sqrt(np.abs(e[..., 2])), np.sqrt(np.abs(e[..., 4]))
    a21 = e[..., 3] / np.maximum(a11 + a22, 1e-9)
    out = np.zeros(e.shape[:-1] + (2, 3))
    out[..., 0, 0], out[..., 0, 2] = 1.0 / a11, e[..., 0]
    out[..., 1, 0], out[..., 1, 1], out[..., 1, 2] = 0.0 - a21 / (a11 * a22), 1.0 / a22, e[..., 1]
    return out


def laf_affine_shape(x, lafs, count=None, ps=32, eps=EPS):
    """the fused entry as its chain: x float32 [n, 1 | 3, h, w], lafs float32 [n, N, 2, 3] ->
    (frames float64 [n, N, 2, 3] before the last rounding, raw moments [n, N, 3], unclamped levels
    of the upright frames [n, N])"""
    to_gray = x.shape[1] == 3
    n, N = lafs.shape[:2]
    U = QC.make_upright(lafs)
    P, lv = PC.extract_patches_pyramid(x, U, ps, to_gray)
    P = P.astype(np.float32)[:, :, 0].reshape(n * N, ps, ps)
    raw = raw_moments(P).reshape(n, N, 3)
    abc = patch_affine_shape(P, eps).astype(np.float32).reshape(n, N, 3)
    E = ellipse_to_laf(np.concatenate([lafs[..., 2], abc], axis=-1)).astype(np.float32)
    r = input_scale(lafs) / input_scale(E)
    out = E.astype(np.float64)
    out[..., :2] *= r[..., None, None]
    dead = ((lafs[..., 0, 2] == -1) & (lafs[..., 1, 2] == -1)) | ~np.isfinite(lafs).all(axis=(-1, -2))
    if count is not None:
        dead |= np.arange(N)[None, :] >= np.asarray(count)[:, None]
    out[dead] = 0.0
    return out, raw, lv
