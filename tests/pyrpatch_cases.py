"""Cases of the patch-pyramid tests: shapes, seeded inputs and a float64 numpy restatement of the
rules include/rr.h states for rr_pyrdown, rr_patch_pyramid, rr_extract_patches_pyramid and
rr_describe_keypoints_pyramid.  Shared by tests/golden/make_golden_pyrpatch.py (which compares the
restatement with the reference), tests/test_host_pyrpatch.py and tests/test_gpu_pyrpatch.py.  The
level-0 rules, the orientation and the descriptor are those of tests/describe_cases.py.
"""

import numpy as np

import describe_cases as QC

# rr_pyrdown: the reflect border at the smallest size, odd and even in each axis, one, one plus a pixel
# and several 32-wide output tiles
DOWN_SHAPES = [(3, 3), (4, 5), (7, 6), (33, 47), (64, 64), (65, 66), (66, 67), (97, 131)]
DOWN_N, DOWN_C = 2, (1, 3)

MAIN = (2, 1, 97, 131)     # levels 97x131, 48x65, 24x32 at PS 16; 97x131, 48x65 at PS 32
COLOR = (1, 3, 80, 96)     # levels 80x96, 40x48, 20x24 at PS 16
NPTS = 24
PATCH_CASES = [("m16", MAIN, 16), ("m32", MAIN, 32), ("c16", COLOR, 16)]
SEED = 7300

BOARDS = [(96, 80), (97, 131)]     # the checkerboard witness
BOARD_SCALE, BOARD_PS, BOARD_NPTS = 13.0, 16, 6

# fused forms (name, image, ps, scale of the kpts + scale forms, forms): the SIFT shape is (ps, 8, 4)
FUSED = [("m16", MAIN, 16, 40.0, ("l0", "l1", "s0", "s1")),    # s: level 2; l: the mixed frames, levels 0 .. 3
         ("m32", MAIN, 32, 24.0, ("s0", "s1"))]                # level 1
U8_SCALE, U8_PS, U8_NPTS = 24.0, 16, 12                         # uint8, three channels, level 2
FULL_TOL_FORM = QC.FULL_TOL_FORM
MARGIN = 1e-3              # |log2(2 s / ps) + 0.5 - integer| of every frame of the fixture

E2E = (1, 1, 160, 192)
E2E_SEED = 7411


def level_sizes(h, w, ps):
    """[(h_l, w_l)] of levels 0 .. last: level l + 1 is (h_l // 2, w_l // 2) while its smaller side is >= ps"""
    out = [(h, w)]
    while min(out[-1][0] // 2, out[-1][1] // 2) >= ps:
        out.append((out[-1][0] // 2, out[-1][1] // 2))
    return out


def pyramid_bytes(n, c, h, w, ps):
    return 4 * n * c * sum(a * b for a, b in level_sizes(h, w, ps)[1:])


def frames(shape, npts, seed):
    """float32 [n, npts, 2, 3] of scale exactly s (the determinant of the shape part is 1): any
    rotation, mild anisotropy and shear, s = 4 * 2^t with t stratified over eight half-octave strata of
    [0, 4) (frame k in stratum k % 8, away from the stratum's ends), so that at PS 16 nine frames of an
    image are of level 0, six of level 1, six of level 2 and three of level 3, and at PS 32 fifteen,
    six and three of levels 0, 1, 2.  Frames 0 - 3 lie within 2 px of an edge, frame 4 outside."""
    n, _, h, w = shape
    u = QC.uniform(seed + 1, n * npts * 6).reshape(n, npts, 6)
    t = ((np.arange(npts) % 8)[None, :] + 0.05 + 0.9 * u[..., 0]) * 0.5
    s = 4.0 * 2.0 ** t
    th = 2.0 * np.pi * u[..., 1]
    ar = 0.8 + 0.4 * u[..., 2]
    sh = 0.3 * (u[..., 3] - 0.5)
    cx, cy = 2.0 + (w - 4.0) * u[..., 4], 2.0 + (h - 4.0) * u[..., 5]
    cx[:, 0], cx[:, 1] = 2.0 * u[:, 0, 4], w - 2.0 * u[:, 1, 4]
    cy[:, 2], cy[:, 3] = 2.0 * u[:, 2, 5], h - 2.0 * u[:, 3, 5]
    cx[:, 4], cy[:, 4] = w + 3.0, -2.5
    c, sn = np.cos(th), np.sin(th)
    A = np.empty((n, npts, 2, 3))
    A[..., 0, 0], A[..., 0, 1] = s * ar * c, s * ar * sn
    A[..., 1, 0], A[..., 1, 1] = s / ar * (sh * c - sn), s / ar * (sh * sn + c)
    A[..., 0, 2], A[..., 1, 2] = cx, cy
    return A.astype(np.float32)


def coarse_images(shape, seed):
    """float32 [n, c, h, w] in [0, 1] with structure at every pyramid level: hash noise on grids of
    pitch 2, 4, 8 and 16 px, each repeated to pixels and smoothed by `pitch` 3 x 3 binomial passes, summed,
    stretched, plus the ramp of describe_cases.smooth_images.  The images of the fused forms: a
    descriptor of level 1 or 2 of smooth_images sees little but the ramp (two 5 x 5 blurs remove the
    3-px noise), every orientation bin but one holds rounding noise of the stored float32 level, and
    RootSIFT's square root near zero multiplies that noise by up to 5e4; the comparison with the
    reference's float64 run (whose levels are float64) is then noise against noise."""
    n, c, h, w = shape
    x = np.zeros(shape)
    for k, pitch in enumerate((2, 4, 8, 16)):
        hh, ww = -(-h // pitch), -(-w // pitch)
        g = QC.uniform(seed + 31 * (k + 1), n * c * hh * ww).reshape(n, c, hh, ww)
        g = np.repeat(np.repeat(g, pitch, axis=2), pitch, axis=3)[..., :h, :w]
        for _ in range(pitch):
            p = np.pad(g, [(0, 0), (0, 0), (1, 1), (1, 1)], mode="edge")
            g = (p[..., :-2, :] + 2.0 * p[..., 1:-1, :] + p[..., 2:, :]) * 0.25
            g = (g[..., :-2] + 2.0 * g[..., 1:-1] + g[..., 2:]) * 0.25
        x += g
    x = (x - x.min()) / (x.max() - x.min())
    ramp = (np.arange(h)[:, None] / float(h) + 2.0 * np.arange(w)[None, :] / float(w)) / 3.0
    return np.ascontiguousarray((0.75 * x + 0.25 * ramp).astype(np.float32))


def fused_keypoints(shape, npts, seed, scale):
    """float32 [n, npts, 2]: keypoints of the kpts + scale forms, at least `scale` from every edge, so
    that the whole patch lies inside the image.  Where a patch of 2 * scale = 48 .. 80 px hangs over
    the edge of a 97 x 131 image, most of it is the border pixel repeated: the gradient there is zero
    in exact arithmetic and rounding noise otherwise (a level is stored in float32), the noise lands
    in arbitrary orientation bins and RootSIFT's square root near zero multiplies it by up to 5e4 --
    the reference's own float32 and float64 runs then differ by 1.8e-4 instead of 8e-7 (measured
    with the generator), and a comparison against that tolerance compares noise with noise.  The
    border rule itself is covered by the patch cases and the l0 / l1 forms, whose frames 0 - 4 lie on
    and past the edges."""
    return QC.keypoints(shape, npts, seed, float(scale))


def checkerboard(h, w):
    i, j = np.arange(h)[:, None], np.arange(w)[None, :]
    return (0.5 + 0.5 * (-1.0) ** (i + j)).astype(np.float32)[None, None]


def board_keypoints(h, w):
    """float32 [1, BOARD_NPTS, 2]: the patch of scale 13 stays inside the image"""
    u = QC.uniform(SEED + 7 * h + w, BOARD_NPTS * 2).reshape(1, BOARD_NPTS, 2)
    m = BOARD_SCALE + 2.0
    return np.stack([m + (w - 2 * m) * u[..., 0], m + (h - 2 * m) * u[..., 1]], axis=-1).astype(np.float32)


# ---------------------------------------------------------------- the restatement
C6 = np.array([1.0, 5.0, 10.0, 10.0, 5.0, 1.0]) / 32.0


def pyrdown(x):
    """[..., h, w] (h, w >= 3) -> float64 [..., h // 2, w // 2], before the rounding to float32"""
    x = np.asarray(x, dtype=np.float64)
    h, w = x.shape[-2:]
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(2, 2), (2, 2)], mode="reflect")
    h2, w2 = h // 2, w // 2
    mid = 0.0
    for a in range(6):      # along x, ascending taps
        mid = C6[a] * p[..., :, a:a + 2 * w2:2] if a == 0 else mid + C6[a] * p[..., :, a:a + 2 * w2:2]
    out = 0.0
    for a in range(6):
        out = C6[a] * mid[..., a:a + 2 * h2:2, :] if a == 0 else out + C6[a] * mid[..., a:a + 2 * h2:2, :]
    return out


def pyramid(x, ps, to_gray=False):
    """x float32 [n, c, h, w] -> [level 0 as float64 (gray when asked), level 1, ...] with levels >= 1
    float32: level 1 from the unrounded float64 image, level l + 1 from the float32 level l"""
    x0 = QC.gray(x) if to_gray else x.astype(np.float64)
    lev = [x0]
    for _ in level_sizes(x.shape[2], x.shape[3], ps)[1:]:
        lev.append(pyrdown(lev[-1]).astype(np.float32))
    return lev


def frame_levels(lafs, ps):
    """(unclamped level int64 [..], t = log2(2 s / ps) + 0.5) of float32 frames [.., 2, 3]"""
    A = lafs.astype(np.float64)
    s = np.sqrt(np.abs((A[..., 0, 0] * A[..., 1, 1] - A[..., 1, 0] * A[..., 0, 1]) + 1e-10))
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.log2((2.0 * s) / float(ps)) + 0.5
    lv = np.where(t >= 1.0, np.floor(t), 0.0)
    lv[~np.isfinite(A).all(axis=(-1, -2))] = 0.0
    return lv.astype(np.int64), t


def level_frames(lafs, h, w, hl, wl):
    """float64 frames on a level of size (hl, wl) of an (h, w) image"""
    A = lafs.astype(np.float64).copy()
    A[..., :2] *= float(min(hl, wl)) / float(min(h, w))
    A[..., 0, 2] *= float(wl) / float(w)
    A[..., 1, 2] *= float(hl) / float(h)
    return A


def extract_patches_pyramid(x, lafs, ps, to_gray=False, lev=None):
    """x float32 [n, c, h, w], lafs float32 [n, N, 2, 3] -> (float64 [n, N, c or 1, ps, ps] before the
    rounding, unclamped levels [n, N]); a frame past the last level is sampled from the last"""
    lev = pyramid(x, ps, to_gray) if lev is None else lev
    h, w = x.shape[2:]
    lv, _ = frame_levels(lafs, ps)
    use = np.minimum(lv, len(lev) - 1)
    out = np.zeros(lafs.shape[:2] + (lev[0].shape[1], ps, ps))
    for l, plane in enumerate(lev):
        hl, wl = plane.shape[2:]
        fr = lafs if l == 0 else level_frames(lafs, h, w, hl, wl)
        p = QC.extract_patches(plane, fr, ps)      # float64 arithmetic on the frames as given
        out[use == l] = p[use == l]
    return out, lv


def describe_keypoints_pyramid(x, kpts=None, count=None, scale=QC.SCALE, lafs=None, orient=False, ps=32, nb=8, ns=4,
                               rootsift=True, clipval=0.2):
    """the fused entry as the chain: (desc float64 [n, N, dim], angles float32 [n, N], frames float32
    [n, N, 2, 3], levels of the described frames)"""
    to_gray = x.shape[1] == 3
    lev = pyramid(x, ps, to_gray)
    F = QC.scale_frames(kpts, scale) if lafs is None else lafs.astype(np.float32)
    n, N = F.shape[:2]
    angles = np.zeros((n, N), dtype=np.float32)
    if orient:
        U = F if lafs is None else QC.make_upright(F)
        P = extract_patches_pyramid(x, U, ps, to_gray, lev)[0].astype(np.float32)[:, :, 0]
        angles = QC.patch_orientation(P.reshape(n * N, ps, ps)).reshape(n, N)
        F = QC.rotate_frames(U, angles)
    P, lv = extract_patches_pyramid(x, F, ps, to_gray, lev)
    P = P.astype(np.float32)[:, :, 0]
    desc = QC.sift_describe(P.reshape(n * N, ps, ps), nb, ns, rootsift, clipval).reshape(n, N, -1)
    dead = (F[..., 0, 2] == -1) & (F[..., 1, 2] == -1)
    if count is not None:
        dead |= np.arange(N)[None, :] >= np.asarray(count)[:, None]
    desc[dead], angles[dead], F = 0.0, 0.0, F.copy()
    F[dead] = 0.0
    return desc, angles, F, lv
