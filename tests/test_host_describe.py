"""CPU checks of keypoint description's host side: the describe.npz fixture (generator checksums, the
numpy restatement of rr_extract_patches / rr_patch_orientation / rr_sift_describe /
rr_describe_keypoints against the reference's results), the argument checks of the four entries and
the workspace function (they return before anything is enqueued, so they run without a GPU), the
Python surface's errors and the LAF helper identities."""

import ctypes
import math
import os

import numpy as np
import pytest
import torch

import describe_cases as QC
from conftest import PKG, golden

LIB = os.path.join(PKG, "librr.so")


def main_inputs(g):
    seed = int(g["seeds"][0])
    return QC.smooth_images(QC.MAIN, seed), QC.frames(QC.MAIN, QC.NPTS, seed), QC.keypoints(QC.MAIN, QC.NPTS, seed, 8.0)


def within(mine, ref, tol, what, share=0.5):
    """the float64 restatement stays within share * tol of the reference's float64 result (here: of
    its float32 rounding, which adds at most half a float32 ulp of the largest value)"""
    assert ref.dtype == np.float32 and ref.shape == mine.shape and tol > 0, what
    ulp = float(np.spacing(np.abs(ref).max()))
    err = np.abs(mine - ref.astype(np.float64)).max()
    assert err <= share * tol + ulp / 2, (what, err, tol)


def test_fixture_checksums_and_cases():
    g = golden("describe.npz")
    assert [tuple(int(v) for v in c) for c in g["configs"]] == QC.CONFIGS
    x, lafs, kpts = main_inputs(g)
    assert x.dtype == np.float32 and x.shape == QC.MAIN and lafs.shape == (QC.MAIN[0], QC.NPTS, 2, 3)
    np.testing.assert_allclose(QC.checksum(x, lafs, kpts), g["main_chk"], rtol=0, atol=1e-9)
    h, w = QC.MAIN[2:]
    c = lafs[..., 2]
    # the border cases: within 2 px of each edge, and one centre outside the image
    assert (c[:, 0, 0] <= 2).all() and (c[:, 1, 0] >= w - 2).all() and (c[:, 2, 1] <= 2).all() and (c[:, 3, 1] >= h - 2).all()
    assert (c[:, 4, 0] > w).all() and (c[:, 4, 1] < 0).all()
    s = np.sqrt(np.abs(lafs[..., 0, 0] * lafs[..., 1, 1] - lafs[..., 0, 1] * lafs[..., 1, 0]))
    assert s.min() >= 4 and s.max() <= 11 and s.max() - s.min() > 4
    x8 = QC.to_u8(QC.smooth_images(QC.U8, int(g["seeds"][1])))
    np.testing.assert_allclose(QC.checksum(x8, QC.keypoints(QC.U8, QC.U8_NPTS, int(g["seeds"][1]), 7.0)), g["u8_chk"], rtol=0, atol=1e-9)
    xr = QC.smooth_images(QC.ROT, int(g["seeds"][2]))
    np.testing.assert_allclose(QC.checksum(xr, QC.keypoints(QC.ROT, QC.ROT_NPTS, int(g["seeds"][2]), 14.0)), g["rot_chk"], rtol=0, atol=1e-9)
    assert (g["ptol"] > 0).all() and (g["dtol"] > 0).all() and (g["dvtol"] > 0).all()
    # odd size: ksize 16, stride 10, pad 4
    assert QC.sift_geometry(41, 4) == (16, 10, 4) and QC.sift_geometry(32, 4) == (12, 8, 3) and QC.sift_geometry(24, 3) == (12, 8, 3)


@pytest.mark.parametrize("c", range(len(QC.CONFIGS)))
def test_restatement_entries(c):
    g = golden("describe.npz")
    x, lafs, kpts = main_inputs(g)
    ps, nb, ns = QC.CONFIGS[c]
    within(QC.extract_patches(x, lafs, ps), g["p%d" % c], float(g["ptol"][c]), "patches")
    flat = g["p%d" % c].reshape(-1, ps, ps)
    n = QC.MAIN[0]
    within(QC.sift_describe(flat, nb, ns).reshape(n, QC.NPTS, -1), g["d%d" % c], float(g["dtol"][c]), "sift")
    np.testing.assert_array_equal(QC.patch_orientation(flat).reshape(n, QC.NPTS), g["a%d" % c])
    if c == 0:
        for j, (rootsift, clipval) in enumerate(QC.VARIANTS):
            within(QC.sift_describe(flat, nb, ns, rootsift, clipval).reshape(n, QC.NPTS, -1), g["dv%d" % j],
                   float(g["dvtol"][j]), "variant %d" % j)
    pl = QC.planted_patches(ps)
    within(QC.sift_describe(pl, nb, ns), g["pl%d_d" % c], float(g["pl%d_dtol" % c]), "planted")
    np.testing.assert_array_equal(QC.patch_orientation(pl), g["pl%d_a" % c])


def test_restatement_planted_patches():
    """the flat patch: mag = sqrt(eps) everywhere and every orientation on a bin edge, so all mass is in
    angular bin 0 and the descriptor is the pooled Gaussian; the ramp: one bin holds all of the mass"""
    ps, nb, ns = QC.CONFIGS[0]
    pl = QC.planted_patches(ps)
    d = QC.sift_describe(pl, nb, ns, rootsift=False, clipval=1.0).reshape(3, nb, ns * ns)
    for k, bins in ((0, (0,)), (1, (0,)), (2, (5, 6))):   # along x: angle 0; along -y: atan2(-g, 0) + 2 pi = 1.5 pi -> bin 6 (float32 pi: just below)
        mass = (d[k] ** 2).sum(1)
        assert mass[list(bins)].sum() > 1 - 1e-6, (k, mass)
    a = QC.patch_orientation(pl)
    assert a[0] == a[1]                         # no gradient and a gradient along +x: the same bin
    assert abs(abs(float(a[2]) - float(a[1])) - math.pi / 2) < 2 * math.pi / QC.ORIENT_BINS


def test_restatement_fused_forms():
    g = golden("describe.npz")
    x, lafs, kpts = main_inputs(g)
    for c, (ps, nb, ns) in enumerate(QC.CONFIGS):
        for form in (("l0", "l1", "s0", "s1") if c == 0 else ("s1",)):
            orient = form[1] == "1"
            kw = dict(lafs=lafs) if form[0] == "l" else dict(kpts=kpts)
            d, a, _ = QC.describe_keypoints(x, orient=orient, ps=ps, nb=nb, ns=ns, **kw)
            within(d, g["f_%s%d" % (form, c)], float(g["ftol_%s%d" % (form, c)]), form, 1.0 if form == QC.FULL_TOL_FORM else 0.5)
            np.testing.assert_array_equal(a, g["fa_%s%d" % (form, c)])
    # dead slots: past count and (-1, -1)
    kp = kpts.copy()
    kp[0, 3] = -1.0
    d, a, F = QC.describe_keypoints(x, kp, count=[QC.NPTS, 5], orient=True)
    assert not d[0, 3].any() and not d[1, 5:].any() and a[0, 3] == 0 and not a[1, 5:].any() and not F[1, 5:].any()
    assert d[0, 2].any() and d[1, 4].any()


def _lib():
    if not os.path.exists(LIB):
        pytest.skip("librr.so not built (run __graft_entry__.build())")
    from cirtorch import _engine
    return _engine, _engine.lib()


def test_describe_argument_checks():
    """every refusal happens on the host: these calls pass made-up device addresses and must return
    before a kernel launch"""
    E, lib = _lib()
    p = ctypes.c_void_p(0x1000)   # "non-null, aligned"; never dereferenced
    null = ctypes.c_void_p(0)
    need = lib.rr_describe_workspace_bytes(2, 24, 32, 8, 4)
    assert need > 0 and lib.rr_describe_workspace_bytes(0, 0, 32, 8, 4) > 0
    assert lib.rr_describe_workspace_bytes(128, 2048, 64, 16, 8) >= need

    def ext(x=p, n=2, c=1, h=16, w=16, gray=0, lafs=p, npts=24, ps=32, out=p):
        return lib.rr_extract_patches(x, n, c, h, w, 0, gray, lafs, npts, ps, out, null)

    def ori(x=p, B=5, ps=32, nb=36, out=p):
        return lib.rr_patch_orientation(x, B, ps, nb, out, null)

    def sift(x=p, B=5, ps=32, nb=8, ns=4, clipval=0.2, out=p):
        return lib.rr_sift_describe(x, B, ps, nb, ns, 1, clipval, out, null)

    def desc(x=p, n=2, c=1, h=16, w=16, kp=p, cnt=null, npts=24, scale=6.0, lafs=null, orient=1, obins=36, ps=32, nb=8,
             ns=4, clipval=0.2, out=p, ws=p, wsb=need):
        return lib.rr_describe_keypoints(x, n, c, h, w, 0, kp, cnt, npts, scale, lafs, orient, obins, ps, nb, ns, 1, clipval,
                                         out, null, null, ws, wsb, null)

    bad = [(ext, dict(x=null)), (ext, dict(lafs=null)), (ext, dict(out=null)), (ext, dict(ps=7)), (ext, dict(ps=65)),
           (ext, dict(c=0)), (ext, dict(h=0)), (ext, dict(w=0)), (ext, dict(n=-1)), (ext, dict(npts=-1)), (ext, dict(gray=1)),
           (ext, dict(gray=2, c=3)), (ext, dict(n=1 << 10, h=1 << 10, w=(1 << 11) + 1)),
           (ext, dict(n=1 << 15, npts=1 << 15, ps=64)), (ext, dict(n=1 << 12, npts=1 << 12)),
           (ext, dict(n=1 << 12, c=2, npts=1 << 11)),
           (ori, dict(x=null)), (ori, dict(out=null)), (ori, dict(ps=7)), (ori, dict(ps=65)), (ori, dict(nb=0)),
           (ori, dict(nb=65)), (ori, dict(B=-1)), (ori, dict(B=1 << 31)), (ori, dict(B=1 << 24)),
           (sift, dict(x=null)), (sift, dict(out=null)), (sift, dict(ps=7)), (sift, dict(ps=65)), (sift, dict(nb=0)),
           (sift, dict(nb=17)), (sift, dict(ns=0)), (sift, dict(ns=9)), (sift, dict(B=-1)), (sift, dict(B=1 << 31)), (sift, dict(B=1 << 24)),
           (sift, dict(clipval=float("nan"))), (sift, dict(ps=8, ns=8)), (sift, dict(ps=12, ns=5)),
           (desc, dict(x=null)), (desc, dict(kp=null)), (desc, dict(out=null)), (desc, dict(c=2)), (desc, dict(c=4)),
           (desc, dict(orient=2)), (desc, dict(obins=0)), (desc, dict(obins=65)), (desc, dict(scale=0.0)),
           (desc, dict(scale=float("nan"))), (desc, dict(scale=float("inf"))), (desc, dict(ps=7)), (desc, dict(nb=17)),
           (desc, dict(ns=9)), (desc, dict(ps=12, ns=5)), (desc, dict(npts=-1)), (desc, dict(ws=null)),
           (desc, dict(wsb=need - 1)), (desc, dict(n=1 << 16, npts=1 << 16)), (desc, dict(n=1 << 12, npts=1 << 12)),
           (desc, dict(n=1 << 10, h=1 << 10, w=(1 << 11) + 1))]
    for fn, kw in bad:
        assert fn(**kw) != 0, (fn.__name__, kw)
    assert desc(wsb=need - 1) == -3 and "workspace" in lib.rr_last_error().decode()   # RR_ENOSPACE
    assert ext(ps=7) == -1   # RR_EINVAL
    for fn, name in ((ext, "rr_extract_patches"), (ori, "rr_patch_orientation"), (sift, "rr_sift_describe"),
                     (desc, "rr_describe_keypoints")):
        assert fn(x=null) != 0
        assert lib.rr_last_error().decode().startswith(name), name
    # a grid of 256-thread blocks holds fewer than 2^32 threads: 2^24 - 1 patches or slots is the most a
    # call takes, and the refusal comes from the checks, not from the launch
    for fn, kw in ((ori, dict(B=(1 << 24) - 1)), (sift, dict(B=(1 << 24) - 1)), (ext, dict(n=(1 << 12) - 1, npts=1 << 12)),
                   (desc, dict(n=(1 << 12) - 1, npts=1 << 12, h=4, w=4))):
        assert fn(x=null, **kw) == -1 and "null" in lib.rr_last_error().decode(), (fn.__name__, kw)
    for fn, kw in ((ori, dict(B=1 << 24)), (sift, dict(B=1 << 24)), (ext, dict(n=1 << 12, npts=1 << 12)),
                   (desc, dict(n=1 << 12, npts=1 << 12, h=4, w=4))):
        assert fn(**kw) == -1 and "2^24" in lib.rr_last_error().decode(), (fn.__name__, kw)
    # the compatibility rule of (ps, num_spatial_bins) is the reference's
    for ps in range(8, 65):
        for ns in range(1, 9):
            assert (sift(x=null, ps=ps, ns=ns) != 0) and (("incompatible" in lib.rr_last_error().decode())
                                                         == (QC.sift_geometry(ps, ns) is None)), (ps, ns)
    # an empty batch is no error (and launches nothing); lafs stand in for kpts
    assert ext(x=null, n=0, lafs=null, out=null) == 0 and ext(npts=0, lafs=null, out=null) == 0
    assert ori(x=null, B=0, out=null) == 0 and sift(x=null, B=0, out=null) == 0
    assert desc(x=null, n=0, kp=null, out=null) == 0 and desc(npts=0, kp=null, out=null) == 0
    assert desc(kp=null, lafs=null) != 0


def test_errors_match_the_reference():
    from cirtorch.features import laf as L
    from cirtorch.features import orientation as O
    from cirtorch.features import siftdesc as S
    with pytest.raises(ValueError, match="incompatible"):
        S.get_sift_bin_ksize_stride_pad(12, 5)
    with pytest.raises(ValueError, match="incompatible"):
        S.SIFTDescriptor(8, 8, 8)
    assert S.get_sift_bin_ksize_stride_pad(41, 4) == (16, 10, 4) and S.get_sift_bin_ksize_stride_pad(32, 4) == (12, 8, 3)
    pk = S.get_sift_pooling_kernel(12)
    assert pk.dtype == torch.float32 and (pk.double().numpy() == QC.pooling_kernel(12)).all()
    m = S.SIFTDescriptor(32)
    assert (m.bin_ksize, m.bin_stride, m.pad) == (12, 8, 3) and m.get_pooling_kernel().shape == (1, 1, 12, 12)
    gk = m.get_weighting_kernel()
    assert gk.shape == (32, 32) and abs(float(gk.sum()) - 1) < 1e-5
    np.testing.assert_allclose(gk.double().numpy(), QC.gaussian_window(32), rtol=1e-6, atol=0)
    for mod in (m, O.PatchDominantGradientOrientation(32)):
        with pytest.raises(ValueError, match="Bx1xHxW"):
            mod(torch.zeros(32, 32))
        with pytest.raises(TypeError, match="Bx1x32x32"):
            mod(torch.zeros(2, 1, 41, 41))
        with pytest.raises(TypeError, match="Bx1x32x32"):
            mod(torch.zeros(2, 3, 32, 32))
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            mod(torch.zeros(2, 1, 32, 32))
    with pytest.raises(TypeError, match="not a torch.Tensor"):
        O.PatchDominantGradientOrientation(32)(np.zeros((2, 1, 32, 32)))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        S.sift_describe(torch.zeros(2, 1, 41, 41))
    laf = torch.zeros(2, 5, 2, 3)
    for fn in (L.get_laf_scale, L.get_laf_center, L.get_laf_orientation, L.make_upright):
        with pytest.raises(TypeError, match="not a torch.Tensor"):
            fn(np.zeros((2, 5, 2, 3)))
        with pytest.raises(ValueError, match="BxNx2x3"):
            fn(torch.zeros(5, 2, 3))
        with pytest.raises(ValueError, match="BxNx2x3"):
            fn(torch.zeros(2, 5, 3, 2))
    with pytest.raises(TypeError, match="scale_coef"):
        L.scale_laf(laf, 2)
    with pytest.raises(TypeError):
        L.laf_from_center_scale_ori(torch.zeros(2, 5, 2), torch.zeros(2, 5, 1), torch.zeros(2, 5, 1))
    img = torch.zeros(2, 1, 40, 56)
    ori = O.LAFOrienter(32)
    with pytest.raises(ValueError, match="BxNx2x3"):
        ori(torch.zeros(5, 2, 3), img)
    with pytest.raises(ValueError, match="BxCxHxW"):
        ori(laf, img[0])
    with pytest.raises(ValueError, match="Batch size"):
        ori(laf, img[:1])
    assert O.PassLAF()(laf, img) is laf
    with pytest.raises(ValueError, match="Batch size"):
        L.extract_patches_simple(img[:1], laf)


def test_cpu_tensors_and_gradients_are_refused():
    from cirtorch.features import laf as L
    from cirtorch.features.orientation import LAFOrienter
    from cirtorch.search import describe_keypoints
    img = torch.rand(2, 1, 40, 56)
    laf = L.laf_from_center_scale_ori(torch.full((2, 5, 2), 20.0), torch.full((2, 5, 1, 1), 6.0), torch.zeros(2, 5, 1))
    kp = torch.full((2, 5, 2), 20.0)
    for call in (lambda: L.extract_patches_simple(img, laf), lambda: L.extract_patches_from_pyramid(img, laf),
                 lambda: LAFOrienter(32)(laf, img), lambda: describe_keypoints(img, kp),
                 lambda: describe_keypoints(img.mul(255).to(torch.uint8), kp, orientation=True),
                 lambda: describe_keypoints(img, None, lafs=laf)):
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            call()
    with pytest.raises(NotImplementedError, match="level"):
        L.extract_patches_from_pyramid(img, L.scale_laf(laf, 4.0))    # 2 * 24 / 32 >= sqrt(2)
    with pytest.raises(ValueError):
        describe_keypoints(torch.zeros(2, 2, 40, 56), kp)
    with pytest.raises(ValueError):
        describe_keypoints(img[0], kp)


def test_gradient_refusal_comes_before_the_kernel():
    from cirtorch import _ops
    t = torch.zeros(2, 32, 32, requires_grad=True)
    # the device check comes first for CPU tensors; the gradient check is a host-side rule of its own
    with pytest.raises(RuntimeError, match="gradients are not supported"):
        _ops._no_grad("sift_describe", t)
    _ops._no_grad("sift_describe", t.detach(), None)


def test_laf_helper_identities():
    from cirtorch.features import laf as L
    u = torch.from_numpy(QC.uniform(77, 2 * 9 * 4).reshape(2, 9, 4)).double()
    xy = torch.stack([5 + 40 * u[..., 0], 5 + 30 * u[..., 1]], dim=-1)
    scale = (3 + 9 * u[..., 2]).view(2, 9, 1, 1)
    ori = (340 * u[..., 3] - 170).view(2, 9, 1)
    laf = L.laf_from_center_scale_ori(xy, scale, ori)
    assert laf.shape == (2, 9, 2, 3)
    torch.testing.assert_close(L.get_laf_scale(laf), scale, rtol=1e-9, atol=0)
    assert torch.equal(L.get_laf_center(laf), xy)
    torch.testing.assert_close(L.get_laf_orientation(laf), ori, rtol=0, atol=1e-5)   # pi is float32
    # rotation [[cos, sin], [-sin, cos]] of degrees
    one = L.laf_from_center_scale_ori(torch.zeros(1, 1, 2), torch.ones(1, 1, 1, 1), torch.full((1, 1, 1), 90.0))
    torch.testing.assert_close(one[0, 0, :, :2], torch.tensor([[0.0, 1.0], [-1.0, 0.0]]), rtol=0, atol=1e-6)
    img = torch.zeros(2, 1, 40, 56)
    torch.testing.assert_close(L.denormalize_laf(L.normalize_laf(laf, img), img), laf, rtol=1e-12, atol=0)
    nl = L.normalize_laf(laf, img)
    torch.testing.assert_close(nl[..., 0, 2], laf[..., 0, 2] / 56.0, rtol=1e-12, atol=0)
    torch.testing.assert_close(nl[..., 1, 2], laf[..., 1, 2] / 40.0, rtol=1e-12, atol=0)
    torch.testing.assert_close(nl[..., :2], laf[..., :2] / 40.0, rtol=1e-12, atol=0)
    up = L.make_upright(laf)
    torch.testing.assert_close(L.get_laf_scale(up), scale, rtol=1e-8, atol=0)
    assert torch.equal(L.get_laf_center(up), xy) and float(up[..., 0, 1].abs().max()) == 0.0
    torch.testing.assert_close(up.float(), torch.from_numpy(QC.make_upright(laf.float().numpy())), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(L.scale_laf(laf, 2.0)[..., :2], 2.0 * laf[..., :2], rtol=0, atol=0)
    inside = L.laf_is_inside_image(laf, img)
    assert inside.shape == (2, 9) and inside.dtype == torch.bool
    far = L.laf_from_center_scale_ori(torch.tensor([[[28.0, 20.0], [2.0, 20.0]]]), torch.full((1, 2, 1, 1), 5.0), torch.zeros(1, 2, 1))
    assert L.laf_is_inside_image(far, img[:1]).tolist() == [[True, False]]
