"""GPU checks of the affine-shape stage (rr_patch_affine_shape, rr_ellipse_to_laf,
rr_laf_affine_shape) against tests/golden/affine.npz and the numpy restatement of
tests/affine_cases.py.

Tolerances are the fixture's: per case the reference's own float32 error against its float64 run.
Frames are compared after the 2 x 2 part is divided by the input frame's scale, centres for equality."""

import functools

import numpy as np
import pytest
import torch

import affine_cases as AC
import describe_cases as QC
import pyrpatch_cases as PC
from conftest import golden
from test_gpu_describe import bits, close, dev

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def G():
    return golden("affine.npz")


@functools.lru_cache(maxsize=None)
def fused_inputs(k):
    return AC.fused_inputs(k, int(G()["seeds"][2 + k]))


def close_frames(got, lafs, ref, tol, what):
    """the 2 x 2 parts over the input scale within tol, the centres equal to the input's"""
    assert got.dtype == torch.float32 and tuple(got.shape) == lafs.shape, (what, got.dtype, tuple(got.shape))
    out = got.cpu().numpy()
    assert ref.dtype == np.float32 and ref.shape == lafs.shape, what
    err = np.abs(AC.normalised(out, lafs) - AC.normalised(ref, lafs)).max()
    print("%s: max |engine - reference float64| %.3g (tol %.3g)" % (what, err, tol))
    assert err <= tol, (what, err, tol)
    assert out[..., 2].tobytes() == lafs[..., 2].tobytes(), what


def chain(x, lafs, ps, cuda, eps=AC.EPS):
    """the separate entries: pyramid -> patches of the upright frames -> shape -> ellipse frame -> the rescaling in float64"""
    from cirtorch import _ops
    it, lt = dev(x, cuda), dev(lafs, cuda)
    gray = x.shape[1] == 3
    pyr = _ops.patch_pyramid(it, ps, gray)[1]
    P = _ops.extract_patches_pyramid(it, dev(QC.make_upright(lafs), cuda), ps, gray, pyr=pyr)[:, :, 0]
    E = _ops.ellipse_to_laf(torch.cat([lt[..., 2], _ops.patch_affine_shape(P, eps)], dim=-1))

    def scale(f):
        f = f.double()
        return ((f[..., 0, 0] * f[..., 1, 1] - f[..., 1, 0] * f[..., 0, 1]) + 1e-10).abs().sqrt()

    out = E.double()
    out[..., :2] = out[..., :2] * (scale(lt) / scale(E))[..., None, None]
    return out.float()


@pytest.mark.parametrize("ps", AC.PATCH_PS)
def test_patch_shape_vs_reference(cuda, ps):
    """fewer pixels than lanes (8), an odd size (19), 32, and 16 pixels per lane (64); the two flat
    patches are (1, 0, 1); function and module agree"""
    from cirtorch import _ops
    from cirtorch.features import PatchAffineShapeEstimator
    g = G()
    p = AC.patches(ps, int(g["seeds"][0]))
    got = _ops.patch_affine_shape(dev(p, cuda))
    close(got, g["ps_%d" % ps], float(g["pstol_%d" % ps]), "shape ps %d" % ps)
    assert np.abs(got.cpu().numpy() - AC.patch_affine_shape(p)).max() <= 6e-8       # float32 rounding of values <= 1
    flat = got[list(AC.PATCH_FLAT)].cpu().numpy()
    assert (flat == np.array([1.0, 0.0, 1.0], dtype=np.float32)).all()
    mod = PatchAffineShapeEstimator(ps)(dev(p, cuda)[:, None])
    assert tuple(mod.shape) == (AC.PATCH_B, 1, 3) and bits(mod) == bits(got)
    assert bits(PatchAffineShapeEstimator(ps)(dev(p, cuda)[:, None].double())) == bits(got)
    # eps is an argument: at 1.0 every patch is a circle; a result does not depend on the batch
    assert (_ops.patch_affine_shape(dev(p, cuda), 1.0).cpu().numpy() == np.array([1.0, 0.0, 1.0], dtype=np.float32)).all()
    assert bits(_ops.patch_affine_shape(dev(p, cuda)[2:5])) == bits(got[2:5])


def test_ellipse_to_laf_vs_reference(cuda):
    from cirtorch.features import ellipse_to_laf
    g = G()
    e = AC.ellipses(int(g["seeds"][1]))
    got = ellipse_to_laf(dev(e, cuda))
    close(got, g["ell"], float(g["ell_tol"]), "ellipse_to_laf")
    assert bits(got[..., 2]) == e[..., :2].tobytes() and not got[..., 0, 1].any()
    np.testing.assert_allclose(got.cpu().numpy(), AC.ellipse_to_laf(e), rtol=2.0 ** -23, atol=0)      # one float32 rounding
    circle = ellipse_to_laf(torch.tensor([[[3.0, 4.0, 1.0, 0.0, 1.0]]], device=cuda))
    assert circle.cpu().numpy().tolist() == [[[[1.0, 0.0, 3.0], [0.0, 1.0, 4.0]]]]


@pytest.mark.parametrize("k", range(len(AC.FUSED)))
def test_fused_vs_reference(cuda, k):
    """rr_laf_affine_shape within tol of the reference's LAFAffineShapeEstimator in float64 (composed on
    the last level for the frames past it); module and function agree; uint8 = its float image"""
    from cirtorch.features import LAFAffineShapeEstimator
    from cirtorch.search import estimate_affine_shape
    g = G()
    name, shape, ps, u8 = AC.FUSED[k]
    x, lafs = fused_inputs(k)
    xt = dev(QC.to_u8(x) if u8 else x, cuda)
    got = estimate_affine_shape(xt, dev(lafs, cuda), None, ps)
    close_frames(got, lafs, g["f_" + name], float(g["ftol_" + name]), "fused " + name)
    assert bits(LAFAffineShapeEstimator(ps)(dev(lafs, cuda), xt)) == bits(got)
    if u8:
        assert bits(estimate_affine_shape(dev(x, cuda), dev(lafs, cuda), None, ps)) == bits(got)
    assert not got[..., 0, 1].any()      # upright


def test_threshold_before_normalisation(cuda):
    """the image times 1e-3: every frame is a circle of its own scale, where full contrast gives
    none -- a threshold applied after the normalisation (largest moment 1) would see no difference"""
    from cirtorch.search import estimate_affine_shape
    g = G()
    k = [c[0] for c in AC.FUSED].index(AC.DIM[0])
    name, shape, ps, u8 = AC.FUSED[k]
    x, lafs = fused_inputs(k)
    xd = (x.astype(np.float64) * AC.DIM[1]).astype(np.float32)
    dim = estimate_affine_shape(dev(xd, cuda), dev(lafs, cuda), None, ps)
    close_frames(dim, lafs, g["dim"], float(g["dim_tol"]), "dim")
    d = dim.cpu().numpy()
    assert (d[..., 0, 0] == d[..., 1, 1]).all() and not d[..., 1, 0].any() and not d[..., 0, 1].any()
    full = estimate_affine_shape(dev(x, cuda), dev(lafs, cuda), None, ps).cpu().numpy()
    assert not ((full[..., 0, 0] == full[..., 1, 1]) & (full[..., 1, 0] == 0)).any()
    assert (np.abs(full[..., 0, 0] / full[..., 1, 1] - 1) > 1e-3).sum() >= lafs.shape[0] * lafs.shape[1] // 2


def test_blob_witnesses(cuda):
    """an isotropic blob returns the input frame; a blob elongated along x gives |A00| > |A11|; the
    transposed image gives the frame with its axes exchanged"""
    from cirtorch.search import estimate_affine_shape
    g = G()
    fr = AC.blob_frame()
    out = []
    for k, (sx, sy) in enumerate(AC.BLOBS):
        got = estimate_affine_shape(dev(AC.blob(sx, sy), cuda), dev(fr, cuda), None, AC.FLAT_PS)
        close_frames(got, fr, g["blob_%d" % k], float(g["blobtol_%d" % k]), "blob %g x %g" % (sx, sy))
        out.append(AC.normalised(got.cpu().numpy(), fr)[0, 0])
    assert np.abs(out[0] - np.eye(2)).max() <= float(g["blobtol_0"])
    assert abs(out[1][0, 0]) > abs(out[1][1, 1]) and abs(out[2][1, 1]) > abs(out[2][0, 0])
    # transposed: (a, b, c) -> (c, b, a), so the diagonal is exchanged and the shear entry stays
    xt = np.ascontiguousarray(AC.blob(*AC.BLOBS[1]).transpose(0, 1, 3, 2))
    ft = QC.scale_frames(fr[..., [1, 0], 2], AC.BLOB_SCALE)
    t = AC.normalised(estimate_affine_shape(dev(xt, cuda), dev(ft, cuda), None, AC.FLAT_PS).cpu().numpy(), ft)[0, 0]
    tol = float(g["blobtol_1"])
    assert abs(t[0, 0] - out[1][1, 1]) <= tol and abs(t[1, 1] - out[1][0, 0]) <= tol and abs(t[1, 0] - out[1][1, 0]) <= tol


@pytest.mark.parametrize("kind", AC.DEGENERATE)
def test_degenerate_images_give_the_upright_circle(cuda, kind):
    from cirtorch.search import estimate_affine_shape
    g = G()
    fr = AC.degenerate_frames()
    got = estimate_affine_shape(dev(AC.degenerate_image(kind), cuda), dev(fr, cuda), None, AC.FLAT_PS)
    close_frames(got, fr, g["deg_" + kind], float(g["degtol_" + kind]), kind)
    want = np.zeros_like(fr)
    want[..., 0, 0] = want[..., 1, 1] = fr[..., 0, 0]
    want[..., 2] = fr[..., 2]
    assert (got.cpu().numpy() == want).all(), kind


@pytest.mark.parametrize("k", range(len(AC.FUSED)))
def test_fused_equals_the_entries(cuda, k):
    """the ABI's bit-identity: rr_patch_pyramid -> rr_extract_patches_pyramid on the upright frames ->
    rr_patch_affine_shape -> rr_ellipse_to_laf -> the rescaling in float64; also at an eps that is the
    median of the case's raw moments a (half of the frames fall under it)"""
    from cirtorch import _ops
    name, shape, ps, u8 = AC.FUSED[k]
    x, lafs = fused_inputs(k)
    mid = float(np.median(G()["raw_" + name][..., 0]))
    for img in ((QC.to_u8(x), x) if u8 else (x,)):
        for eps in (AC.EPS, mid):
            got = _ops.laf_affine_shape(dev(img, cuda), dev(lafs, cuda), None, ps, eps)
            assert bits(got) == bits(chain(img, lafs, ps, cuda, eps)), (name, eps)
    assert bits(got) != bits(_ops.laf_affine_shape(dev(x, cuda), dev(lafs, cuda), None, ps))
    # the restatement rounds at the same three places (shape, ellipse frame, result): an ulp each at the most
    np.testing.assert_allclose(got.cpu().numpy(), AC.laf_affine_shape(x, lafs, None, ps, mid)[0], rtol=4 * 2.0 ** -24, atol=0)


def test_dead_slots_invariance_and_in_place(cuda):
    """slots past count, (-1, -1) centres and non-finite frames give zero frames; a live frame's bits
    do not depend on the batch position, the batch size or the run; in place equals out of place"""
    from cirtorch import _ops
    from cirtorch.search import estimate_affine_shape
    shape = (3,) + PC.MAIN[1:]
    x = dev(AC.contrast_images(shape, AC.SEED + 3), cuda)
    lafs = PC.frames(shape, 16, AC.SEED + 3)
    lt = dev(lafs, cuda)
    full, again = estimate_affine_shape(x, lt, None, 16), estimate_affine_shape(x, lt, None, 16)
    assert bits(full) == bits(again) and bool(torch.isfinite(full).all())
    for i in range(3):
        assert bits(estimate_affine_shape(x[i:i + 1], lt[i:i + 1], None, 16)[0]) == bits(full[i])
    swapped = estimate_affine_shape(x.flip(0), lt.flip(0), None, 16)
    assert bits(swapped.flip(0)) == bits(full)
    lf = lafs.copy()
    lf[0, 3, :, 2] = lf[2, 0, :, 2] = -1.0
    lf[0, 7, 1, 1] = np.nan
    lf[2, 9, 0, 2] = np.inf
    count = torch.tensor([16, 5, 16], dtype=torch.int32, device=cuda)
    got = estimate_affine_shape(x, dev(lf, cuda), count, 16)
    live = torch.ones(3, 16, dtype=torch.bool)
    live[0, 3] = live[2, 0] = live[0, 7] = live[2, 9] = False
    live[1, 5:] = False
    assert not got[~live].any() and bits(got[live]) == bits(full[live])
    np.testing.assert_allclose(got.cpu().numpy(), AC.laf_affine_shape(x.cpu().numpy(), lf, count.cpu().numpy(), 16)[0],
                               rtol=4 * 2.0 ** -24, atol=0)
    buf = dev(lf, cuda)
    ret = _ops.laf_affine_shape(x, buf, count, 16, out=buf)
    assert ret is buf and bits(buf) == bits(got)
    assert estimate_affine_shape(x, lt[:, :0], None, 16).shape == (3, 0, 2, 3)


def test_graph_capture_replay_equals_eager(cuda):
    from cirtorch.search import estimate_affine_shape
    from cirtorch.utils.graph import GraphedForward
    shape = (2, 3, 80, 96)
    xs = [dev(QC.to_u8(AC.contrast_images(shape, AC.SEED + 60 + i)), cuda) for i in range(2)]
    lafs = dev(PC.frames(shape, 16, AC.SEED + 60), cuda)
    count = torch.tensor([16, 9], dtype=torch.int32, device=cuda)

    def fn(t):
        return estimate_affine_shape(t, lafs, count, 16)

    g = GraphedForward(fn, xs[0])
    for t in (xs[1], xs[0]):
        got = g(t).clone()
        want = fn(t)
        assert bits(got) == bits(want)
        assert bool(want[1, :9].any()) and not want[1, 9:].any()
    assert bits(fn(xs[0])) != bits(fn(xs[1]))


def test_refusals_enqueue_nothing(cuda):
    """RR_EINVAL / RR_ENOSPACE from the entry itself leave the output untouched; the Python surface refuses CPU tensors"""
    from cirtorch import _engine as E
    from cirtorch.search import detect_keypoints_scale_space, estimate_affine_shape
    x, lafs = fused_inputs(0)
    xt, lt = dev(x, cuda), dev(lafs, cuda)
    n, c, h, w = x.shape
    lib = E.lib()
    need = int(lib.rr_laf_affine_shape_workspace_bytes(n, c, h, w, AC.NPTS, 16))
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    out = torch.full((n, AC.NPTS, 2, 3), 7.0, device=cuda)
    abc = torch.full((n * AC.NPTS, 3), 7.0, device=cuda)
    st = E.stream_ptr()

    def fused(ps=16, eps=1e-10, wsb=need, c_=c):
        return lib.rr_laf_affine_shape(E.ptr(xt), n, c_, h, w, 0, E.ptr(lt), None, AC.NPTS, ps, eps, E.ptr(out), E.ptr(ws), wsb, st)

    assert fused(ps=7) == -1 and fused(ps=65) == -1 and fused(eps=float("nan")) == -1 and fused(c_=2) == -1      # RR_EINVAL
    assert fused(wsb=need - 1) == -3 and "workspace" in lib.rr_last_error().decode()                              # RR_ENOSPACE
    assert lib.rr_patch_affine_shape(E.ptr(xt), 4, 7, 1e-10, E.ptr(abc), st) == -1
    assert lib.rr_patch_affine_shape(E.ptr(xt), 1 << 24, 8, 1e-10, E.ptr(abc), st) == -1
    assert lib.rr_ellipse_to_laf(E.ptr(xt), -1, E.ptr(out), st) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((abc == 7.0).all())
    assert fused() == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        estimate_affine_shape(xt, lt.cpu())
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        estimate_affine_shape(xt.cpu(), lt)
    with pytest.raises(ValueError, match="count must be int32"):
        estimate_affine_shape(xt, lt, torch.zeros(n, dtype=torch.int64, device=cuda))
    with pytest.raises(ValueError, match=r"outside \[8, 64\]"):
        estimate_affine_shape(xt, lt, None, 7)
    with pytest.raises(ValueError, match="affine_patch_size"):
        detect_keypoints_scale_space(xt, 16, affine=True, affine_patch_size=7)


def test_end_to_end_hessian_affine(cuda):
    """detect_keypoints_scale_space(affine=True) -> describe_keypoints(lafs=, orientation=True,
    pyramid=True) on 1 x 1 x 160 x 192 with 64 keypoints: finite descriptors; every live frame keeps the
    detector's scale to float32 rounding (each of the two diagonal entries carries at most 2^-24, the
    determinant 2^-23, its root 2^-24; bound 2^-23) and its centre; the default leaves today's result;
    ScaleSpaceDetector(aff_module=LAFAffineShapeEstimator(), ori_module=LAFOrienter()) runs"""
    from cirtorch.features import LAFAffineShapeEstimator, LAFOrienter, ScaleSpaceDetector, get_laf_scale
    from cirtorch.search import describe_keypoints, detect_keypoints_scale_space, estimate_affine_shape
    x = dev(PC.coarse_images(AC.E2E, AC.E2E_SEED), cuda)
    plain = detect_keypoints_scale_space(x, 64)
    lafs, scores, count = detect_keypoints_scale_space(x, 64, affine=True)
    n = int(count[0])
    assert n >= 8 and bits(scores) == bits(plain[1]) and bits(count) == bits(plain[2])
    assert all(bits(a) == bits(b) for a, b in zip(detect_keypoints_scale_space(x, 64, affine=False), plain))
    assert bits(lafs) == bits(estimate_affine_shape(x, plain[0], count))
    assert bits(lafs[..., 2]) == bits(plain[0][..., 2]) and not lafs[0, n:].any()
    s_in, s_out = plain[0][0, :n, 0, 0].double(), get_laf_scale(lafs.double())[0, :n, 0, 0]
    rel = float(((s_out - s_in) / s_in).abs().max())
    ratio = (lafs[0, :n, 0, 0] / lafs[0, :n, 1, 1]).cpu().numpy()
    print("end to end: %d detections, scale kept to %.3g, axis ratios %.2f .. %.2f" % (n, rel, ratio.min(), ratio.max()))
    assert rel <= 2.0 ** -23
    assert (np.abs(ratio - 1) > 1e-3).any()           # some frames did change shape
    d, a = describe_keypoints(x, None, count, lafs=lafs, orientation=True, pyramid=True)
    assert bool(torch.isfinite(d).all()) and bool(d[0, :n].any(dim=-1).all()) and not d[0, n:].any()
    out = ScaleSpaceDetector(64, aff_module=LAFAffineShapeEstimator(), ori_module=LAFOrienter())(x)
    assert out[0].shape == (1, 64, 2, 3) and bool(torch.isfinite(out[0]).all())
    assert bits(ScaleSpaceDetector(64, aff_module=LAFAffineShapeEstimator())(x)[0][0, :n]) == bits(lafs[0, :n])
