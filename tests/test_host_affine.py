"""CPU checks of the affine-shape stage's host side: the affine.npz fixture (checksums, the
conditions its generator asserts, the numpy restatement of rr_patch_affine_shape / rr_ellipse_to_laf
/ rr_laf_affine_shape against the reference's results), the argument checks and byte counts of the
new entries (they return before anything is enqueued, so they run without a GPU) and the Python
surface: module arguments, shape errors, exports and refusals."""

import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import affine_cases as AC
import describe_cases as QC
import pyrpatch_cases as PC
from conftest import PKG, golden
from test_host_describe import within

LIB = os.path.join(PKG, "librr.so")


def _lib():
    if not os.path.exists(LIB):
        pytest.skip("librr.so not built (run __graft_entry__.build())")
    from cirtorch import _engine
    return _engine, _engine.lib()


def within_frames(mine, lafs, ref, tol, what, share=0.5):
    """the float64 restatement's frames stay within share * tol of the reference's float64 frames, both
    over the input scale (the fixture holds their float32 rounding, which adds at most half a float32
    ulp of each entry); the centres are the input's"""
    assert ref.dtype == np.float32 and ref.shape == mine.shape == lafs.shape and tol > 0, what
    half_ulp = np.spacing(np.abs(ref[..., :2])).astype(np.float64) / 2 / AC.input_scale(lafs)[..., None, None]
    err = np.abs(AC.normalised(mine, lafs) - AC.normalised(ref, lafs))
    assert (err <= share * tol + half_ulp).all(), (what, err.max(), tol)
    assert (ref[..., 2] == lafs[..., 2]).all() and (mine[..., 2] == lafs[..., 2]).all(), what


def degenerate(raw):
    return (raw < AC.EPS).sum(-1) >= 2


def outside_band(raw):
    return not ((raw >= AC.BAND[0]) & (raw <= AC.BAND[1])).any()


def test_fixture_checksums_and_conditions():
    g = golden("affine.npz")
    seeds = [int(s) for s in g["seeds"]]
    assert len(seeds) == 2 + len(AC.FUSED)
    assert os.path.getsize(os.path.join(PKG, "..", "tests", "golden", "affine.npz")) < 200 * 1024
    chk = []
    for ps in AC.PATCH_PS:
        p = AC.patches(ps, seeds[0])
        raw = AC.raw_moments(p)
        assert p.shape == (AC.PATCH_B, ps, ps) and p.min() >= 0 and p.max() <= 1 and outside_band(raw)
        assert sorted(np.nonzero(degenerate(raw))[0].tolist()) == sorted(AC.PATCH_FLAT)
        assert (raw[:, 1] < 0).any() and (raw[:, 1] >= AC.EPS).any()      # b of either sign among the live patches
        assert 0 < float(g["pstol_%d" % ps]) <= AC.TOL_CAP
        chk.append(QC.checksum(p))
    np.testing.assert_allclose(np.concatenate(chk), g["patch_chk"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(QC.checksum(AC.ellipses(seeds[1])), g["ell_chk"], rtol=0, atol=1e-9)
    for k, (name, shape, ps, u8) in enumerate(AC.FUSED):
        x, lafs = AC.fused_inputs(k, seeds[2 + k])
        chk = [QC.checksum(x, lafs)]
        if u8:
            assert (QC.to_u8(x).astype(np.float32) / np.float32(255.0) == x).all()
        _, raw, lv = AC.laf_affine_shape(x, lafs, None, ps)
        # the reference's float64 run keeps float64 levels and patches, the chain rounds both to float32
        np.testing.assert_allclose(raw, g["raw_" + name], rtol=1e-4, atol=1e-18)
        assert outside_band(raw) and outside_band(g["raw_" + name])
        t = PC.frame_levels(QC.make_upright(lafs), ps)[1]
        assert np.abs(t - np.rint(t)).min() >= PC.MARGIN
        last = len(PC.level_sizes(shape[2], shape[3], ps)) - 1
        for l in range(last + 1):
            assert (lv == l).sum() >= 3, (name, l)
        assert (lv > last).sum() >= 2, name
        assert 0 < float(g["ftol_" + name]) <= AC.TOL_CAP
        if name == AC.DIM[0]:
            xd = (x.astype(np.float64) * AC.DIM[1]).astype(np.float32)
            chk.append(QC.checksum(xd))
            rawd = AC.laf_affine_shape(xd, lafs, None, ps)[1]
            assert degenerate(rawd).all() and outside_band(rawd) and not degenerate(raw).all()
            assert 0 < float(g["dim_tol"]) <= AC.TOL_CAP
        np.testing.assert_allclose(np.concatenate(chk), g["chk_" + name], rtol=0, atol=1e-9)
    for k, (sx, sy) in enumerate(AC.BLOBS):
        raw = AC.laf_affine_shape(AC.blob(sx, sy), AC.blob_frame(), None, AC.FLAT_PS)[1]
        assert outside_band(raw) and not degenerate(raw).any() and 0 < float(g["blobtol_%d" % k]) <= AC.TOL_CAP
    for kind in AC.DEGENERATE:
        _, raw, lv = AC.laf_affine_shape(AC.degenerate_image(kind), AC.degenerate_frames(), None, AC.FLAT_PS)
        assert outside_band(raw) and degenerate(raw).all() and sorted(set(lv.ravel().tolist())) == [0, 1]
    edge = AC.laf_affine_shape(AC.degenerate_image("edge"), AC.degenerate_frames(), None, AC.FLAT_PS)[1]
    assert (edge[..., 0] >= AC.EPS).any()      # a frame across the edge: a is live, b and c are not


def test_window_is_the_sift_window():
    """G of the reference's estimator is get_gaussian_kernel2d((ps, ps), (ps / sqrt 2, ps / sqrt 2), True),
    the window of SIFTDescriptor: one table (describe_cases.gaussian_window) serves both restatements"""
    for ps in AC.PATCH_PS:
        G = QC.gaussian_window(ps)
        assert G.shape == (ps, ps) and abs(G.sum() - 1) < 1e-6 and (G == G.T).all()
        assert (G.astype(np.float32) == G).all()          # float32-valued


@pytest.mark.parametrize("ps", AC.PATCH_PS)
def test_restatement_patch_shape(ps):
    g = golden("affine.npz")
    p = AC.patches(ps, int(g["seeds"][0]))
    mine = AC.patch_affine_shape(p)
    within(mine, g["ps_%d" % ps], float(g["pstol_%d" % ps]), "shape %d" % ps)
    assert (mine[list(AC.PATCH_FLAT)] == (1.0, 0.0, 1.0)).all() and mine.max() == 1.0
    # the rule's order: normalising first would leave a maximum of 1 and nothing to threshold
    raw = AC.raw_moments(p)
    assert (raw.max(axis=1) < 1e-3).all()
    # eps is an argument: a huge one makes every patch a circle, zero none
    assert (AC.patch_affine_shape(p, 1.0) == (1.0, 0.0, 1.0)).all()
    assert not (AC.patch_affine_shape(p, 0.0)[:, 1] == 0.0).all()


def test_restatement_ellipse_to_laf():
    g = golden("affine.npz")
    e = AC.ellipses(int(g["seeds"][1]))
    mine = AC.ellipse_to_laf(e)
    within(mine, g["ell"], float(g["ell_tol"]), "ellipse_to_laf")
    assert (mine[..., 2] == e[..., :2]).all() and not mine[..., 0, 1].any()
    # the frame is the inverse of the lower-triangular square root of [[a, b], [b, c]] (b enters through a21)
    a11, a22 = np.sqrt(e[0, :, 2].astype(np.float64)), np.sqrt(e[0, :, 4].astype(np.float64))
    for i in range(AC.ELLIPSES):
        R = np.array([[a11[i], 0.0], [e[0, i, 3] / (a11[i] + a22[i]), a22[i]]])
        np.testing.assert_allclose(mine[0, i, :, :2] @ R, np.eye(2), rtol=0, atol=1e-12)


@pytest.mark.parametrize("k", range(len(AC.FUSED)))
def test_restatement_fused(k):
    g = golden("affine.npz")
    name, shape, ps, u8 = AC.FUSED[k]
    x, lafs = AC.fused_inputs(k, int(g["seeds"][2 + k]))
    mine = AC.laf_affine_shape(x, lafs, None, ps)[0]
    within_frames(mine, lafs, g["f_" + name], float(g["ftol_" + name]), "fused " + name)
    assert (mine[..., 2] == lafs[..., 2]).all()
    np.testing.assert_allclose(AC.input_scale(mine), AC.input_scale(lafs), rtol=1e-6)     # the scale is kept
    if name == AC.DIM[0]:
        xd = (x.astype(np.float64) * AC.DIM[1]).astype(np.float32)
        dim = AC.laf_affine_shape(xd, lafs, None, ps)[0]
        within_frames(dim, lafs, g["dim"], float(g["dim_tol"]), "dim")
        n = AC.normalised(dim, lafs)
        assert np.abs(n[..., 0, 0] - 1).max() < 1e-9 and np.abs(n[..., 1, 1] - 1).max() < 1e-9 and not n[..., 1, 0].any()
        assert np.abs(AC.normalised(mine, lafs)[..., 0, 0] - 1).max() > 0.05      # full contrast: not circles
    count = np.array([5] + [AC.NPTS] * (shape[0] - 1))
    bad = lafs.copy()
    bad[0, 1, 0, 0] = np.nan
    bad[0, 2, :, 2] = -1.0
    dead = AC.laf_affine_shape(x, bad, count, ps)[0]
    assert not dead[0, 1].any() and not dead[0, 2].any() and not dead[0, 5:].any()
    assert (dead[0, 0] == mine[0, 0]).all() and (dead[0, 3:5] == mine[0, 3:5]).all()


def test_restatement_blobs_and_degenerate_images():
    g = golden("affine.npz")
    fr = AC.blob_frame()
    n = []
    for k, (sx, sy) in enumerate(AC.BLOBS):
        mine = AC.laf_affine_shape(AC.blob(sx, sy), fr, None, AC.FLAT_PS)[0]
        within_frames(mine, fr, g["blob_%d" % k], float(g["blobtol_%d" % k]), "blob %d" % k)
        n.append(AC.normalised(mine, fr)[0, 0])
    assert np.abs(n[0] - np.eye(2)).max() <= float(g["blobtol_0"])           # isotropic: the input frame
    assert n[1][0, 0] > 1.5 * n[1][1, 1] and n[2][1, 1] > 1.5 * n[2][0, 0]   # the long axis of the frame along the blob's
    fr = AC.degenerate_frames()
    for kind in AC.DEGENERATE:
        mine = AC.laf_affine_shape(AC.degenerate_image(kind), fr, None, AC.FLAT_PS)[0]
        within_frames(mine, fr, g["deg_" + kind], float(g["degtol_" + kind]), kind)
        want = np.zeros_like(fr)
        want[..., 0, 0] = want[..., 1, 1] = fr[..., 0, 0]
        want[..., 2] = fr[..., 2]
        assert (mine.astype(np.float32) == want).all(), kind       # exactly the upright circle of the input scale


def test_modules_arguments_and_shape_errors():
    from cirtorch import features as F
    from cirtorch.features.affine_shape import LAFAffineShapeEstimator, PatchAffineShapeEstimator
    assert F.LAFAffineShapeEstimator is LAFAffineShapeEstimator and F.PatchAffineShapeEstimator is PatchAffineShapeEstimator
    assert F.ellipse_to_laf is F.laf.ellipse_to_laf
    p = PatchAffineShapeEstimator()
    assert (p.patch_size, p.eps) == (19, 1e-10) and repr(p) == "PatchAffineShapeEstimator(patch_size=19, eps=1e-10)"
    assert repr(PatchAffineShapeEstimator(32, 1e-6)) == "PatchAffineShapeEstimator(patch_size=32, eps=1e-06)"
    with pytest.raises(TypeError, match="not a torch.Tensor"):
        p(np.zeros((1, 1, 19, 19)))
    with pytest.raises(ValueError, match="Bx1xHxW"):
        p(torch.zeros(1, 19, 19))
    for shape in ((2, 1, 19, 20), (2, 1, 32, 32), (2, 3, 19, 19)):
        with pytest.raises(TypeError, match=r"\[Bx1x19x19\]"):
            p(torch.zeros(shape))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        p(torch.zeros(2, 1, 19, 19))
    m = LAFAffineShapeEstimator()
    assert m.patch_size == 32 and repr(m) == "LAFAffineShapeEstimator(patch_size=32)"
    assert isinstance(m.affine_shape_detector, PatchAffineShapeEstimator) and m.affine_shape_detector.patch_size == 32
    assert repr(LAFAffineShapeEstimator(19)) == "LAFAffineShapeEstimator(patch_size=19)"
    img, laf = torch.rand(2, 1, 40, 56), torch.rand(2, 5, 2, 3)
    with pytest.raises(TypeError, match="Laf type"):
        m(laf.numpy(), img)
    with pytest.raises(ValueError, match="BxNx2x3"):
        m(laf[:, :, :, :2], img)
    with pytest.raises(TypeError, match="img type"):
        m(laf, img.numpy())
    with pytest.raises(ValueError, match="BxCxHxW"):
        m(laf, img[0])
    with pytest.raises(ValueError, match="Batch size"):
        m(laf, img[:1])
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        m(laf, img)
    for bad in (torch.zeros(2, 5), torch.zeros(2, 3, 6), np.zeros((1, 2, 5))):
        with pytest.raises(TypeError, match="BxNx5"):
            F.ellipse_to_laf(bad)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        F.ellipse_to_laf(torch.ones(1, 2, 5))


def test_scale_space_detector_accepts_the_estimator():
    from cirtorch.features import LAFAffineShapeEstimator, LAFOrienter, PassLAF, ScaleSpaceDetector
    d = ScaleSpaceDetector(aff_module=LAFAffineShapeEstimator())
    assert type(d.aff) is LAFAffineShapeEstimator and type(d.ori) is PassLAF
    d = ScaleSpaceDetector(64, aff_module=LAFAffineShapeEstimator(19), ori_module=LAFOrienter())
    assert d.aff.patch_size == 19
    assert type(ScaleSpaceDetector().aff) is PassLAF
    for bad in (LAFOrienter(), torch.nn.Identity()):
        with pytest.raises(NotImplementedError, match="aff_module"):
            ScaleSpaceDetector(aff_module=bad)


def test_search_surface():
    from cirtorch import search
    sig = inspect.signature(search.detect_keypoints_scale_space)
    assert sig.parameters["affine"].default is False and sig.parameters["affine_patch_size"].default == 32
    sig = inspect.signature(search.estimate_affine_shape)
    assert list(sig.parameters) == ["images", "lafs", "count", "patch_size"] and sig.parameters["patch_size"].default == 32
    img, laf = torch.rand(2, 1, 40, 56), torch.rand(2, 5, 2, 3)
    with pytest.raises(ValueError, match=r"\[B, 1, H, W\]"):
        search.estimate_affine_shape(img[0], laf)
    with pytest.raises(ValueError, match=r"\[B, 1, H, W\]"):
        search.estimate_affine_shape(torch.rand(2, 2, 40, 56), laf)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        search.estimate_affine_shape(img, laf)
    with pytest.raises(ValueError, match="affine_patch_size"):
        search.detect_keypoints_scale_space(img, 16, affine=True, affine_patch_size=65)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        search.detect_keypoints_scale_space(img, 16, affine=True)


def test_workspace_bytes_and_argument_checks():
    """every refusal happens on the host: made-up device addresses, nothing is launched"""
    E, lib = _lib()
    p, null = ctypes.c_void_p(0x1000), ctypes.c_void_p(0)
    need = lib.rr_laf_affine_shape_workspace_bytes(2, 1, 97, 131, 24, 16)
    assert need == lib.rr_describe_pyramid_workspace_bytes(2, 1, 97, 131, 24, 16, 8, 4) and need >= 256 + PC.pyramid_bytes(2, 1, 97, 131, 16)
    assert lib.rr_laf_affine_shape_workspace_bytes(2, 3, 97, 131, 24, 16) == need      # the gray pyramid
    assert lib.rr_laf_affine_shape_workspace_bytes(2, 1, 40, 56, 24, 32) == 256        # no level 1

    def shape(x=p, B=7, ps=19, eps=1e-10, out=p):
        return lib.rr_patch_affine_shape(x, B, ps, eps, out, null)

    def ell(x=p, B=16, out=p):
        return lib.rr_ellipse_to_laf(x, B, out, null)

    def fused(x=p, n=2, c=1, h=97, w=131, lafs=p, cnt=null, npts=24, ps=16, eps=1e-10, out=p, ws=p, wsb=need):
        return lib.rr_laf_affine_shape(x, n, c, h, w, 0, lafs, cnt, npts, ps, eps, out, ws, wsb, null)

    bad = [(shape, dict(x=null)), (shape, dict(out=null)), (shape, dict(B=-1)), (shape, dict(B=1 << 24)), (shape, dict(ps=7)),
           (shape, dict(ps=65)), (shape, dict(eps=float("nan"))), (shape, dict(eps=float("inf"))),
           (ell, dict(x=null)), (ell, dict(out=null)), (ell, dict(B=-1)), (ell, dict(B=1 << 24)),
           (fused, dict(x=null)), (fused, dict(lafs=null)), (fused, dict(out=null)), (fused, dict(c=2)), (fused, dict(c=0)),
           (fused, dict(h=0)), (fused, dict(n=-1)), (fused, dict(npts=-1)), (fused, dict(ps=7)), (fused, dict(ps=65)),
           (fused, dict(eps=float("nan"))), (fused, dict(n=1 << 12, npts=1 << 12, h=4, w=4, ps=8))]
    for fn, kw in bad:
        assert fn(**kw) == -1, (fn.__name__, kw)           # RR_EINVAL
    for fn, kw in ((fused, dict(ws=null)), (fused, dict(wsb=need - 1)), (fused, dict(wsb=256))):
        assert fn(**kw) == -3 and "workspace" in lib.rr_last_error().decode(), kw      # RR_ENOSPACE
    for fn, name in ((shape, "rr_patch_affine_shape"), (ell, "rr_ellipse_to_laf"), (fused, "rr_laf_affine_shape")):
        assert fn(x=null) != 0
        assert lib.rr_last_error().decode().startswith(name + ":"), name
    # empty inputs launch nothing
    assert shape(x=null, B=0, out=null) == 0 and ell(x=null, B=0, out=null) == 0
    assert fused(x=null, n=0, lafs=null, out=null) == 0 and fused(npts=0, lafs=null, out=null) == 0
