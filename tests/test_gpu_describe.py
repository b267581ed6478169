"""GPU checks of keypoint description (rr_extract_patches, rr_patch_orientation, rr_sift_describe,
rr_describe_keypoints) against tests/golden/describe.npz and the numpy restatement of
tests/describe_cases.py.

Tolerances are the fixture's: per case the reference's own float32 error against its float64 run.
Orientation angles are compared for equality (the fixture's generator keeps only inputs whose
argmax is safe)."""

import functools
import math

import numpy as np
import pytest
import torch

import describe_cases as QC
import verify_cases as VC
from conftest import golden

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def G():
    return golden("describe.npz")


@functools.lru_cache(maxsize=None)
def main_inputs():
    seed = int(G()["seeds"][0])
    return QC.smooth_images(QC.MAIN, seed), QC.frames(QC.MAIN, QC.NPTS, seed), QC.keypoints(QC.MAIN, QC.NPTS, seed, 8.0)


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def close(got, ref, tol, what):
    assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape, (what, got.dtype, tuple(got.shape), ref.shape)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref.astype(np.float64)).max()
    print("%s: max |engine - reference float64| %.3g (tol %.3g)" % (what, err, tol))
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize("c", range(len(QC.CONFIGS)))
def test_entries_vs_reference(cuda, c):
    """patches, descriptors (and the rootsift / clipval variants) within tol of the reference's float64
    run, angles equal to it; the planted flat and ramp patches; functions and modules agree"""
    from cirtorch.features import laf as L
    from cirtorch.features.orientation import PatchDominantGradientOrientation
    from cirtorch.features.siftdesc import SIFTDescriptor, sift_describe
    g = G()
    x, lafs, _ = main_inputs()
    ps, nb, ns = QC.CONFIGS[c]
    n = QC.MAIN[0]
    xt, lt = dev(x, cuda), dev(lafs, cuda)
    p = L.extract_patches_simple(xt, lt, ps)
    close(p, g["p%d" % c], float(g["ptol"][c]), "patches ps %d" % ps)
    assert bits(L.extract_patches_from_pyramid(xt, lt, ps)) == bits(p)           # every frame is level 0
    # frames normalised beforehand (in float64: the round trip then returns the float32 frames)
    assert bits(L.extract_patches_simple(xt, L.normalize_laf(lt.double(), xt), ps, False)) == bits(p)
    gp = dev(g["p%d" % c].reshape(-1, 1, ps, ps), cuda)
    d = SIFTDescriptor(ps, nb, ns)(gp)
    close(d.view(n, QC.NPTS, -1), g["d%d" % c], float(g["dtol"][c]), "sift %s" % ((ps, nb, ns),))
    assert bits(sift_describe(gp, ps, nb, ns)) == bits(d)
    # float64 patches (what the reference also takes) are converted: the same float32 descriptors and angles
    d64 = SIFTDescriptor(ps, nb, ns)(gp.double())
    assert d64.dtype == torch.float32 and bits(d64) == bits(d)
    a = PatchDominantGradientOrientation(ps, QC.ORIENT_BINS)(gp)
    assert a.dtype == torch.float32 and bits(a) == g["a%d" % c].tobytes()
    assert bits(PatchDominantGradientOrientation(ps, QC.ORIENT_BINS)(gp.double())) == bits(a)
    if c == 0:
        for j, (rootsift, clipval) in enumerate(QC.VARIANTS):
            dv = SIFTDescriptor(ps, nb, ns, rootsift, clipval)(gp)
            close(dv.view(n, QC.NPTS, -1), g["dv%d" % j], float(g["dvtol"][j]), "sift variant %s" % ((rootsift, clipval),))
    pl = dev(QC.planted_patches(ps)[:, None], cuda)
    close(SIFTDescriptor(ps, nb, ns)(pl), g["pl%d_d" % c], float(g["pl%d_dtol" % c]), "planted patches ps %d" % ps)
    assert bits(PatchDominantGradientOrientation(ps, QC.ORIENT_BINS)(pl)) == g["pl%d_a" % c].tobytes()
    # a frame with a non-finite entry gives a zero patch and leaves its neighbours alone
    bad = lafs.copy()
    bad[0, 2, 1, 0], bad[1, 7, 0, 2] = np.nan, np.inf
    pb = L.extract_patches_simple(xt, dev(bad, cuda), ps)
    assert not pb[0, 2].any() and not pb[1, 7].any()
    keep = torch.ones(n, QC.NPTS, dtype=torch.bool)
    keep[0, 2] = keep[1, 7] = False
    assert bits(pb[keep]) == bits(p[keep])


def test_patch_sizes_and_bins_vs_restatement(cuda):
    """the sizes at which the kernel takes another path: the smallest and largest patch (LDS above
    64 KiB), one spatial bin (a 64 x 64 pooling window), 16 x 8 x 8 = 1024 outputs (more outputs than
    threads), 1 and 64 orientation bins -- against the float64 restatement, to a bound from the
    formats: float32 rounding of values <= 1 (6e-8) plus float64 noise, RootSIFT's square root near
    zero aside (plain SIFT is compared)"""
    from cirtorch import _ops
    x, lafs, _ = main_inputs()
    xt, lt = dev(x, cuda), dev(lafs[:, :6], cuda)
    for ps, nb, ns in ((8, 4, 2), (64, 8, 1), (64, 16, 8), (33, 1, 3), (16, 16, 4)):
        p = _ops.extract_patches(xt, lt, ps)
        want = QC.extract_patches(x, lafs[:, :6], ps)
        assert np.abs(p.cpu().numpy() - want).max() <= 6e-8 + 1e-12
        flat = p.view(-1, ps, ps)
        d = _ops.sift_describe(flat, nb, ns, rootsift=False, clipval=0.2)
        wd = QC.sift_describe(flat.cpu().numpy(), nb, ns, rootsift=False, clipval=0.2)
        assert tuple(d.shape) == wd.shape == (12, nb * ns * ns)
        assert np.abs(d.cpu().numpy() - wd).max() <= 6e-8 + 1e-9, (ps, nb, ns)
        for ob in (1, 7, 36, 64):
            h = QC.orientation_histogram(flat.cpu().numpy(), ob)
            top = np.sort(h, axis=1)[:, -2:]
            safe = ob == 1 or bool(((top[:, 1] - top[:, 0]) >= 1e-9 * top[:, 1]).all())
            a = _ops.patch_orientation(flat, ob)
            if safe:
                assert bits(a) == QC.patch_orientation(flat.cpu().numpy(), ob).tobytes(), (ps, ob)


def fused(cuda, x, form, c=0, **kw):
    from cirtorch import _ops
    _, lafs, kpts = main_inputs()
    ps, nb, ns = QC.CONFIGS[c]
    src = dict(lafs=dev(lafs, cuda)) if form[0] == "l" else dict(kpts=dev(kpts, cuda), scale=QC.SCALE)
    return _ops.describe_keypoints(x, orient=form[1] == "1", orient_bins=QC.ORIENT_BINS, ps=ps, num_ang_bins=nb,
                                   num_spatial_bins=ns, **src, **kw)


def test_fused_vs_reference(cuda):
    """rr_describe_keypoints within tol of the reference's chain (extract, orient, extract, describe)
    in float64, angles equal: frames with and without orientation, kpts + scale with and without,
    the three configurations; the public function gives the same bits"""
    from cirtorch.search import describe_keypoints
    g = G()
    x, lafs, kpts = main_inputs()
    xt = dev(x, cuda)
    for c, (ps, nb, ns) in enumerate(QC.CONFIGS):
        for form in (("l0", "l1", "s0", "s1") if c == 0 else ("s1",)):
            d, a = fused(cuda, xt, form, c)
            close(d, g["f_%s%d" % (form, c)], float(g["ftol_%s%d" % (form, c)]), "fused %s config %d" % (form, c))
            assert bits(a) == g["fa_%s%d" % (form, c)].tobytes(), (form, c)
            kw = dict(lafs=dev(lafs, cuda)) if form[0] == "l" else dict(scale=QC.SCALE)
            pub = describe_keypoints(xt, dev(kpts, cuda), None, orientation=form[1] == "1", patch_size=ps, num_ang_bins=nb,
                                     num_spatial_bins=ns, **kw)
            assert bits(pub[0]) == bits(d) and bits(pub[1]) == bits(a)


def test_uint8_gray_path(cuda):
    """[1, 3, 33, 47] uint8: within tol of the reference on its gray image, angles equal, and bit-equal
    to the float32 path fed x.float() / 255 (IEEE division on the host) reduced to gray by the kernel"""
    from cirtorch import _ops
    from cirtorch.search import describe_keypoints
    g = G()
    seed = int(g["seeds"][1])
    x8 = QC.to_u8(QC.smooth_images(QC.U8, seed))
    kpts = dev(QC.keypoints(QC.U8, QC.U8_NPTS, seed, 7.0), cuda)
    u8, unit = dev(x8, cuda), dev(x8.astype(np.float32) / np.float32(255.0), cuda)
    d, a = describe_keypoints(u8, kpts, scale=QC.SCALE, orientation=True)
    close(d, g["u8_d"], float(g["u8_tol"]), "uint8 gray")
    assert bits(a) == g["u8_a"].tobytes()
    for orient in (False, True):
        got, want = describe_keypoints(u8, kpts, scale=QC.SCALE, orientation=orient), describe_keypoints(unit, kpts, scale=QC.SCALE, orientation=orient)
        assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1])
    lafs = dev(QC.scale_frames(kpts.cpu().numpy(), QC.SCALE), cuda)
    assert bits(_ops.extract_patches(u8, lafs, 32)) == bits(_ops.extract_patches(unit, lafs, 32))
    assert bits(_ops.extract_patches(u8, lafs, 32, gray=True)) == bits(_ops.extract_patches(unit, lafs, 32, gray=True))


@pytest.mark.parametrize("orient", (False, True))
def test_fused_equals_the_three_entries(cuda, orient):
    """bit-identical to rr_extract_patches -> rr_patch_orientation -> rr_sift_describe: with frames
    and with kpts + scale, gray and three-channel input; the frames the kernel reports are the
    restatement's to a float32 ulp"""
    from cirtorch import _ops
    x, lafs, kpts = main_inputs()
    seed = int(G()["seeds"][1])
    x3 = QC.smooth_images(QC.U8, seed)
    k3 = QC.keypoints(QC.U8, QC.U8_NPTS, seed, 7.0)
    for img, kw, start in ((x, dict(lafs=lafs), lafs), (x, dict(kpts=kpts, scale=QC.SCALE), QC.scale_frames(kpts, QC.SCALE)),
                           (x3, dict(kpts=k3, scale=QC.SCALE), QC.scale_frames(k3, QC.SCALE))):
        for ps, nb, ns in QC.CONFIGS[:2]:
            it = dev(img, cuda)
            gray = img.shape[1] == 3
            args = {k: (dev(v, cuda) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
            d, a, F = _ops.describe_keypoints(it, orient=orient, orient_bins=QC.ORIENT_BINS, ps=ps, num_ang_bins=nb,
                                              num_spatial_bins=ns, return_lafs=True, **args)
            if orient:
                U = QC.make_upright(start) if "lafs" in kw else start
                pu = _ops.extract_patches(it, dev(U, cuda), ps, gray=gray)
                assert bits(_ops.patch_orientation(pu[:, :, 0], QC.ORIENT_BINS)) == bits(a)
                want = QC.rotate_frames(U, a.cpu().numpy())
                assert np.abs(F.cpu().numpy() - want).max() <= np.spacing(np.float32(np.abs(want[..., :2]).max()))
            else:
                assert bits(F) == start.tobytes() and not a.any()
            p = _ops.extract_patches(it, F, ps, gray=gray)
            assert bits(_ops.sift_describe(p[:, :, 0], nb, ns)) == bits(d), (ps, orient)


def test_dead_slots_batch_and_run_invariance(cuda):
    """slots past count and (-1, -1) keypoints give zeros and their neighbours the bits of the full
    run; an image alone and inside a batch of 3 give the same bits; two runs agree"""
    from cirtorch.search import describe_keypoints
    shape = (3,) + QC.MAIN[1:]
    x = dev(QC.smooth_images(shape, QC.SEED + 3), cuda)
    kpts = QC.keypoints(shape, 16, QC.SEED + 3, 8.0)
    for orient in (False, True):
        full = describe_keypoints(x, dev(kpts, cuda), scale=QC.SCALE, orientation=orient)
        again = describe_keypoints(x, dev(kpts, cuda), scale=QC.SCALE, orientation=orient)
        assert bits(full[0]) == bits(again[0]) and bits(full[1]) == bits(again[1])
        assert bool(full[0].abs().sum(-1).min() > 0)
        for i in range(3):
            one = describe_keypoints(x[i:i + 1], dev(kpts[i:i + 1], cuda), scale=QC.SCALE, orientation=orient)
            assert bits(one[0][0]) == bits(full[0][i]) and bits(one[1][0]) == bits(full[1][i])
        kp = kpts.copy()
        kp[0, 3] = kp[2, 0] = -1.0
        count = torch.tensor([16, 5, 16], dtype=torch.int32, device=cuda)
        d, a = describe_keypoints(x, dev(kp, cuda), count, scale=QC.SCALE, orientation=orient)
        live = torch.ones(3, 16, dtype=torch.bool)
        live[0, 3] = live[2, 0] = False
        live[1, 5:] = False
        assert not d[~live].any() and not a[~live].any()
        assert bits(d[live]) == bits(full[0][live]) and bits(a[live]) == bits(full[1][live])
        # count = 0 and no keypoints at all
        d0, _ = describe_keypoints(x, dev(kp, cuda), torch.zeros(3, dtype=torch.int32, device=cuda), scale=QC.SCALE)
        assert not d0.any()
        assert describe_keypoints(x, dev(kp[:, :0], cuda))[0].shape == (3, 0, 128)


def test_translation_equivariance(cuda):
    """a crop shifted by whole pixels, keypoints shifted along: descriptors of keypoints whose patch
    stays inside both images are bit-identical (whole-pixel keypoints and a power-of-two scale: every
    sample position is exact in float64)"""
    from cirtorch.search import describe_keypoints
    img = QC.smooth_images((1, 1, 64, 80), QC.SEED + 4)
    y0, x0, h, w = 5, 7, 52, 66
    full = dev(img, cuda)
    crop = full[:, :, y0:y0 + h, x0:x0 + w].contiguous()
    kp = np.floor(QC.keypoints((1, 1, h, w), 20, QC.SEED + 4, 13.0))       # the patch of scale 8 turned by any angle stays inside
    for orient in (False, True):
        a = describe_keypoints(crop, dev(kp, cuda), scale=8.0, orientation=orient)
        b = describe_keypoints(full, dev(kp + np.float32([x0, y0]), cuda), scale=8.0, orientation=orient)
        assert bits(a[0]) == bits(b[0]) and bits(a[1]) == bits(b[1])
        assert orient == bool(a[1].any())


def test_rotation_by_90_degrees(cuda):
    """an image turned by 90 degrees (exact index permutation), keypoints turned along, orientation on:
    the angles differ by pi / 2 up to one bin, the descriptors agree to the cosine the reference's own
    float64 chain reaches on the same pair (fixture), less what the descriptor tolerance allows: two
    unit vectors moved by at most tol per element change their cosine by at most 2 tol sqrt(dim)
    each, to first order"""
    from cirtorch.search import describe_keypoints
    g = G()
    seed = int(g["seeds"][2])
    x = QC.smooth_images(QC.ROT, seed)
    kpts = QC.keypoints(QC.ROT, QC.ROT_NPTS, seed, 14.0)
    xr, kr = QC.rot90_pair(x, kpts)
    da, aa = describe_keypoints(dev(x, cuda), dev(kpts, cuda), scale=QC.ROT_SCALE, orientation=True)
    db, ab = describe_keypoints(dev(xr, cuda), dev(kr, cuda), scale=QC.ROT_SCALE, orientation=True)
    assert bits(aa) == g["rot_a"].tobytes() and bits(ab) == g["rot_ar"].tobytes()
    diff = np.mod((aa - ab).cpu().numpy().astype(np.float64) + math.pi, 2 * math.pi) - math.pi
    width = 2 * math.pi / QC.ORIENT_BINS
    assert (np.abs(np.abs(diff) - math.pi / 2) <= width + 1e-6).all(), diff
    assert len(set(np.sign(diff).ravel().tolist())) == 1       # all turned the same way
    va, vb = da[0].double().cpu().numpy(), db[0].double().cpu().numpy()
    cos = (va * vb).sum(1) / (np.linalg.norm(va, axis=1) * np.linalg.norm(vb, axis=1))
    slack = 4 * float(g["rot_tol"]) * math.sqrt(va.shape[1])
    print("rotation: cosines %.9f .. %.9f, reference %.9f .. %.9f, slack %.3g" % (cos.min(), cos.max(), g["rot_cos"].min(),
                                                                                   g["rot_cos"].max(), slack))
    assert (cos >= g["rot_cos"] - slack).all()


def test_graph_capture_replay_equals_eager(cuda):
    from cirtorch.search import describe_keypoints
    from cirtorch.utils.graph import GraphedForward
    shape = (2, 3, 48, 64)
    xs = [dev(QC.to_u8(QC.smooth_images(shape, QC.SEED + 60 + i)), cuda) for i in range(2)]
    kpts = dev(QC.keypoints(shape, 32, QC.SEED + 60, 8.0), cuda)
    count = torch.tensor([32, 20], dtype=torch.int32, device=cuda)

    def fn(t):
        return describe_keypoints(t, kpts, count, scale=QC.SCALE, orientation=True)

    g = GraphedForward(fn, xs[0])
    for t in (xs[1], xs[0]):
        got = [o.clone() for o in g(t)]
        want = fn(t)
        assert all(bits(a) == bits(b) for a, b in zip(got, want))
        assert bool(want[0][1, :20].any()) and not want[0][1, 20:].any()


def warp_image(img, Hm):
    """img [h, w] float64 -> the image seen through Hm (a point p of img appears at Hm p), bilinear"""
    h, w = img.shape
    ys, xs = np.mgrid[0:h, 0:w]
    src = VC.transfer(np.linalg.inv(Hm), np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1)) - 0.5
    sx, sy = np.clip(src[:, 0], 0, w - 1), np.clip(src[:, 1], 0, h - 1)
    x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = sx - x0, sy - y0
    out = (img[y0, x0] * (1 - fx) + img[y0, x1] * fx) * (1 - fy) + (img[y1, x0] * (1 - fx) + img[y1, x1] * fx) * fy
    return out.reshape(h, w)


CHAIN_H = np.array([[0.98, -0.06, 5.0], [0.05, 1.01, -3.0], [1e-4, -5e-5, 1.0]])


def dlt_svd(p1, p2):
    """the DLT of verify_cases.dlt on the singular vectors of the design matrix instead of the
    eigenvectors of its normal matrix: the second solver of the tol_px rule"""
    q1, T1 = VC.normalize_points(np.asarray(p1, dtype=np.float64))
    q2, T2 = VC.normalize_points(np.asarray(p2, dtype=np.float64))
    x1, y1, x2, y2 = q1[:, 0], q1[:, 1], q2[:, 0], q2[:, 1]
    o, z = np.ones_like(x1), np.zeros_like(x1)
    ax = np.stack([z, z, z, -x1, -y1, -o, y2 * x1, y2 * y1, y2], 1)
    ay = np.stack([x1, y1, o, z, z, z, -x2 * x1, -x2 * y1, -x2], 1)
    v = np.linalg.svd(np.stack([ax, ay], 1).reshape(-1, 9))[2][-1]
    Hm = np.linalg.inv(T2) @ (v.reshape(3, 3) @ T1)
    return Hm / Hm[2, 2]


def test_chain_detect_describe_match_verify(cuda):
    """image -> keypoints -> SIFT descriptors -> matches -> inliers on raw images with no host step
    and no weights: an image and a known homographic warp of it, 96 x 128.
    The recovered H is held to the tol_px rule of test_gpu_verify.py against the host oracle
    (verify_cases.verify_pair) on the keypoints and matches the chain produced: equal inlier count and
    mask (the oracle's margin shows that no residual is within 1e-7 px of th), corner transfer within
    100 x the difference of two DLT solvers on the fitted set, floor 1e-9 px.
    Against the planted H exact coordinates do not exist: keypoints are whole pixels, so a keypoint is up
    to sqrt(2) / 2 px off in its own image and its partner as much in the other, (1 + s) sqrt(2) / 2 px
    together with s the largest stretch of the planted H (1.4 px here).  A fit over many such
    correspondences must move the corners no further than one of them is off, and a true
    correspondence lies within th of the recovered H, so within th plus that of the planted position.
    The pair has more inliers than an unrelated pair."""
    from cirtorch.search import describe_keypoints, detect_keypoints, match_pairs, verify_pairs
    n, th, h, w = 96, 3.0, 96, 128
    a = QC.smooth_images((2, 1, h, w), QC.SEED + 70).astype(np.float64)
    views = [a[0, 0], warp_image(a[0, 0], CHAIN_H), a[1, 0]]
    x = dev(np.stack(views)[:, None].astype(np.float32), cuda)
    kp, sc, cnt = detect_keypoints(x, n, "harris", nms=5, border=14)
    assert int(cnt.min()) == n
    desc, ang = describe_keypoints(x, kp, cnt, scale=10.0, orientation=True)
    assert desc.shape == (3, n, 128) and desc.dtype == torch.float32 and desc.device == kp.device and ang.shape == (3, n)
    d1, d2 = desc[[0, 0]], desc[[1, 2]]
    match, dist = match_pairs(d1, d2, mode="smnn", th=0.9)
    inl, Hm, mask = verify_pairs(kp[[0, 0]], kp[[1, 2]], match, th=th, iters=1024, seed=1)
    assert int(inl[0]) >= 12 and int(inl[0]) > 2 * int(inl[1])
    corners = np.array([[0, 0], [w, 0], [w, h], [0, h]], dtype=np.float64)

    def corner_err(Ha, Hb):
        return float(np.sqrt(((VC.transfer(Ha, corners) - VC.transfer(Hb, corners)) ** 2).sum(1)).max())

    # the host oracle on the chain's own keypoints and matches
    Hn = Hm[0].cpu().numpy()
    kn, mn = kp.cpu().numpy(), match.cpu().numpy()
    o = VC.verify_pair(kn[0], kn[1], mn[0], 0, th, 1024, 2, 1)
    assert o["margin"] >= 1e-7 and o["fit"] is not None
    assert int(inl[0]) == o["inliers"]
    np.testing.assert_array_equal(mask[0].cpu().numpy(), o["mask"])
    tol_px = max(100 * corner_err(VC.dlt(o["fit"][:, :2], o["fit"][:, 2:]), dlt_svd(o["fit"][:, :2], o["fit"][:, 2:])), 1e-9)
    e_oracle = corner_err(Hn, o["H"])
    # the planted H: CHAIN_H is on positions with pixel centres at k + 0.5, Hn on pixel indices
    quant = (1 + np.linalg.svd(CHAIN_H[:2, :2], compute_uv=False)[0]) * math.sqrt(2) / 2
    err = float(np.sqrt(((VC.transfer(Hn, corners - 0.5) + 0.5 - VC.transfer(CHAIN_H, corners)) ** 2).sum(1)).max())
    rows = mask[0].nonzero()[:, 0]
    p1, p2 = kp[0][rows].double().cpu().numpy(), kp[1][match[0][rows]].double().cpu().numpy()
    res = np.sqrt(((VC.transfer(CHAIN_H, p1 + 0.5) - 0.5 - p2) ** 2).sum(1))
    print("chain: matches %s, inliers %s; corner error vs oracle %.3g px (tol_px %.3g), vs planted %.3f px (bound %.3f); "
          "inlier residual under the planted H max %.3f px" % ((match >= 0).sum(1).tolist(), inl.tolist(), e_oracle, tol_px, err,
                                                             quant, res.max()))
    assert e_oracle <= tol_px
    assert err <= quant
    assert res.max() <= th + quant
