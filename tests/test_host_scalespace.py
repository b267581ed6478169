"""CPU checks of scale-space detection's host side: the scalespace.npz fixture (generator checksum, the
numpy restatement of the pyramid, the extrema and the lists against the reference's results), the
workspace functions, the argument checks of the new entries (which return before anything is
enqueued, so they run without a GPU) and the Python surface's refusals."""

import ctypes
import os

import numpy as np
import pytest
import torch

import scalespace_cases as SC
from conftest import PKG, golden

LIB = os.path.join(PKG, "librr.so")


def _img(g, k):
    return SC.images(k, int(g["seeds"][k]))


def test_fixture_checksum_and_cases():
    g = golden("scalespace.npz")
    assert [tuple(int(v) for v in c) for c in g["cases"]] == SC.CASES
    for k, shape in enumerate(SC.CASES):
        x = _img(g, k)
        assert x.dtype == np.float32 and x.shape == shape
        np.testing.assert_allclose(x.astype(np.float64).sum(), g["chk"][k], rtol=0, atol=1e-9)
    assert (SC.as_u8(_img(g, SC.U8_CASE)).astype(np.float32) / np.float32(255) == _img(g, SC.U8_CASE)).all()


def test_plan_sizes_sigmas_and_kernel_cap():
    first, octs = SC.plan(40, 56)
    assert first[0] == 13 and [(o["h"], o["w"]) for o in octs] == [(40, 56), (20, 28)]
    assert [b[0] for b in octs[0]["blurs"]] == [11, 13, 17, 21, 25]
    assert [b[0] for b in octs[1]["blurs"]] == [11, 13, 17, 21, 21]          # 25 capped at min(20, 28), made odd
    assert [(o["h"], o["w"]) for o in SC.plan(37, 53)[1]] == [(37, 53), (18, 26)]
    assert len(SC.plan(24, 30)[1]) == 1 and len(SC.plan(96, 128)[1]) == 3
    assert octs[1]["sigmas"][0] == SC.SIGMA and abs(octs[0]["sigmas"][3] - 2 * SC.SIGMA) < 1e-12
    assert SC.plan(40, 56, sigma=0.4)[0] is None
    t = SC.taps(11, 1.2)
    assert t.shape == (11,) and (t == t[::-1]).all() and abs(t.sum() - 1) < 1e-6 and (t.astype(np.float32) == t).all()


@pytest.mark.parametrize("k", SC.PYRAMID_CASES)
def test_restatement_pyramid(k):
    """the restatement stays within tol / 2 of the reference's float64 levels (here: of their float32
    rounding, which adds at most half a float32 ulp)"""
    g = golden("scalespace.npz")
    pyr, octs = SC.pyramid(_img(g, k))
    for oi, lv in enumerate(pyr):
        ref, tol = g["p%d_%d" % (k, oi)], g["ptol%d_%d" % (k, oi)]
        assert ref.dtype == np.float32 and ref.shape == lv.shape and tol.shape == (SC.L,) and (tol > 0).all()
        ulp = float(np.spacing(np.float32(np.abs(ref).max())))
        assert (np.abs(lv - ref).max(axis=(0, 2, 3)) <= tol / 2 + ulp / 2).all(), (k, oi)


def test_restatement_blur():
    g = golden("scalespace.npz")
    x = _img(g, 1)
    for j, (ks, s) in enumerate(SC.BLUR_SIZES):
        assert np.abs(SC.blur(x, ks, s) - g["b%d" % j]).max() <= g["btol"][j] / 2 + 3e-8


def _volumes(g):
    return [g["v_%d" % oi] for oi in range(2)]


def test_restatement_extrema():
    g = golden("scalespace.npz")
    for oi, v in enumerate(_volumes(g)):
        ref = np.unpackbits(g["vm_%d" % oi])[:v.size].reshape(v.shape).astype(bool)
        m, offs, vals = SC.extrema(v)
        np.testing.assert_array_equal(m == 1, ref)
        assert not (ref[:, 0].any() or ref[:, -1].any() or ref[:, :, 0].any() or ref[:, :, -1].any()
                    or ref[..., 0].any() or ref[..., -1].any())
        mb = np.broadcast_to(ref[:, None], offs.shape)
        assert np.abs(offs[mb] - g["vo_%d" % oi]).max() <= float(g["votol"]) + 1e-7
        assert np.abs(vals[ref] - g["vv_%d" % oi]).max() <= float(g["vvtol"]) + 1e-8
        assert (np.abs(offs) <= 0.7).all() and (offs[~mb] == 0).all() and (vals[~ref] == v[~ref]).all()


def test_restatement_planted_volume():
    v = SC.planted_volume()
    m, offs, vals = SC.extrema(v, False)
    m2, offs2, vals2 = SC.extrema(v, True)
    assert not m[0, 2, 10, 5] and not m[0, 2, 10, 6]               # equal neighbours
    assert not m[0, 1:4, 14:17, 3:6].any()                         # plateau
    for d, y, x in ((0, 9, 12), (4, 9, 12), (2, 0, 12), (2, 19, 12), (2, 9, 0), (2, 9, 23)):
        assert not m2[0, d, y, x]                                  # faces
    assert m[0, 2, 10, 20] == 1 and m2[0, 2, 10, 20] == 1
    assert m[0, 2, 14, 18] == 0 and m2[0, 2, 14, 18] == 2          # the hole's minimum: with minima only
    assert vals2[0, 2, 14, 18] >= 1.5 and vals[0, 2, 14, 18] == np.float32(-1.5)
    assert ((m2 == 1) == (m == 1)).all()
    d, y, x = SC.PLANTED_BELOW
    assert m[0, d, y, x] == 1 and abs(offs[0, 1, d, y, x] - 0.69) < 1e-5 and abs(offs[0, 2, d, y, x] - 0.2) < 1e-5
    assert abs(offs[0, 0, d, y, x]) < 1e-5 and vals[0, d, y, x] > 10.0
    d, y, x = SC.PLANTED_ABOVE
    assert m[0, d, y, x] == 1 and (offs[0, :, d, y, x] == 0).all() and vals[0, d, y, x] == v[0, d, y, x]


@pytest.mark.parametrize("j", range(len(SC.LISTS)))
def test_restatement_lists(j):
    g = golden("scalespace.npz")
    k, kind, mr, minima, num = SC.LISTS[j]
    lafs, scores, count, voxels = SC.detect(_img(g, k), kind, num, mr, minima)
    np.testing.assert_array_equal(count, g["l%d_count" % j])
    for b, vx in enumerate(voxels):
        assert [v[0] for v in vx] == g["l%d_oct" % j][b, :count[b]].tolist()
        assert [v[1] for v in vx] == g["l%d_vox" % j][b, :count[b]].tolist()
    assert np.abs(lafs - g["l%d_lafs" % j]).max() <= float(g["l%d_ltol" % j]) + 4e-6   # float32 storage of ~64
    assert np.abs(scores - g["l%d_scores" % j]).max() <= float(g["l%d_stol" % j]) + 1e-9
    if k == SC.EMPTY_CASE:
        assert count.max() == 0 and not lafs.any() and not scores.any()
    else:
        assert count.min() >= 8
    for b in range(len(count)):
        assert not lafs[b, count[b]:].any() and not scores[b, count[b]:].any()
        assert (np.diff(scores[b, :count[b]]) < 0).all()


def test_restatement_small_n_and_swap():
    g = golden("scalespace.npz")
    x = _img(g, 0)
    full = SC.detect(x, "hessian", 64, 1.0)
    for num in SC.SMALL_NUMS:
        lafs, scores, count, _ = SC.detect(x, "hessian", num, 1.0)
        assert (count == num).all()
        np.testing.assert_array_equal(lafs, full[0][:, :num])
        np.testing.assert_array_equal(scores, full[1][:, :num])
    # the blob image: every planted blob has a keypoint within a pixel, refined toward its centre
    img, planted = SC.blobs(int(g["seeds"][SC.BLOB_CASE]))
    lafs, _, count, voxels = SC.detect(img, "dog", 64, 2.0, True)
    SC.check_blobs(lafs[0, :count[0]], voxels[0], planted, SC.plan(*img.shape[2:])[1])


def _lib():
    if not os.path.exists(LIB):
        pytest.skip("librr.so not built (run __graft_entry__.build())")
    from cirtorch import _engine
    return _engine, _engine.lib()


def test_workspace_bytes_and_python_plan():
    E, lib = _lib()
    from cirtorch import _ops
    ob, wb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for n, c, h, w in SC.CASES + [(128, 3, 768, 1024)]:
        assert lib.rr_scale_pyramid_bytes(n, c, h, w, SC.LEVELS, SC.SIGMA, SC.MIN_SIZE, ctypes.byref(ob), ctypes.byref(wb)) == 0
        octs = _ops.pyramid_plan(n, h, w, SC.LEVELS, SC.SIGMA, SC.MIN_SIZE)
        first, mine = SC.plan(h, w)
        assert [(o["h"], o["w"], o["sigmas"]) for o in octs] == [(o["h"], o["w"], o["sigmas"]) for o in mine]
        assert octs[0]["blurs"][0] == first and [o["blurs"][1:] for o in octs] == [o["blurs"] for o in mine]
        total = octs[-1]["off"] + n * SC.L * octs[-1]["h"] * octs[-1]["w"]
        assert total * 4 <= ob.value < total * 4 + 512 and all(o["off"] % 64 == 0 for o in octs)
        assert wb.value >= 3 * n * h * w * 8
        need = lib.rr_detect_scale_space_workspace_bytes(n, c, h, w, SC.LEVELS, SC.SIGMA, SC.MIN_SIZE)
        # two float32 pyramids (levels, responses), the working planes, a key per possible candidate
        assert need >= 2 * total * 4 + wb.value + n * SC.candidate_bound(mine) * 8
    assert lib.rr_detect_scale_space_workspace_bytes(0, 1, 40, 56, 3, 1.6, 15) > 0
    assert lib.rr_detect_scale_space_workspace_bytes(1, 2, 40, 56, 3, 1.6, 15) == 0
    # no two 26-neighbours are both strict maxima: a lattice of period 2 reaches the bound per sign
    v = np.zeros((1, 5, 9, 11), dtype=np.float32)
    v[0, 1:-1:2, 1:-1:2, 1:-1:2] = 1.0
    assert (SC.extrema_mask(v) == 1).sum() == 2 * 4 * 5 <= SC.candidate_bound([dict(h=9, w=11)], 5) // 2


def test_argument_checks():
    """every refusal happens on the host: these calls pass made-up device addresses and must return
    before a kernel launch"""
    E, lib = _lib()
    p = ctypes.c_void_p(0x1000)   # "non-null, aligned"; never dereferenced
    null = ctypes.c_void_p(0)
    ob, wb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.rr_scale_pyramid_bytes(2, 1, 40, 56, 3, 1.6, 15, ctypes.byref(ob), ctypes.byref(wb)) == 0
    need = lib.rr_detect_scale_space_workspace_bytes(2, 1, 40, 56, 3, 1.6, 15)

    def blur(x=p, planes=2, h=16, w=16, ks=11, sigma=1.2, out=p):
        return lib.rr_gaussian_blur(x, planes, h, w, ks, sigma, out, null)

    def pyr(x=p, n=2, c=1, h=40, w=56, levels=3, sigma=1.6, min_size=15, out=p, outb=None, ws=p, wsb=None):
        return lib.rr_scale_pyramid(x, n, c, h, w, 0, levels, sigma, min_size, out, ob.value if outb is None else outb, ws,
                                    wb.value if wsb is None else wsb, null)

    def dog(x=p, n=2, L=6, h=16, w=16, out=p):
        return lib.rr_dog_response(x, n, L, h, w, out, null)

    def ext(x=p, n=2, D=5, h=16, w=16, minima=0, mask=p, offs=p, vals=p):
        return lib.rr_scale_space_extrema(x, n, D, h, w, minima, mask, offs, vals, null)

    def sel(x=p, n=2, h=40, w=56, levels=3, sigma=1.6, min_size=15, minima=0, mr=6.0, num=64, lafs=p, sc=p, cnt=p, ws=p,
            wsb=need):
        return lib.rr_scale_space_select(x, n, h, w, levels, sigma, min_size, minima, mr, num, lafs, sc, cnt, ws, wsb, null)

    def det(x=p, n=2, c=1, h=40, w=56, levels=3, sigma=1.6, min_size=15, kind=E.RR_RESP_HESSIAN, k=0.04, minima=0, mr=6.0,
            num=64, lafs=p, sc=p, cnt=p, ws=p, wsb=need):
        return lib.rr_detect_scale_space(x, n, c, h, w, 0, levels, sigma, min_size, kind, k, minima, mr, num, lafs, sc, cnt,
                                         ws, wsb, null)

    nan = float("nan")
    bad = [(blur, dict(x=null)), (blur, dict(out=null)), (blur, dict(ks=10)), (blur, dict(ks=65)), (blur, dict(ks=-1)),
           (blur, dict(ks=33)), (blur, dict(h=5)), (blur, dict(sigma=0.0)), (blur, dict(sigma=nan)), (blur, dict(planes=-1)),
           (blur, dict(h=0)), (blur, dict(planes=1 << 40)),
           (pyr, dict(x=null)), (pyr, dict(out=null)), (pyr, dict(c=2)), (pyr, dict(levels=0)), (pyr, dict(levels=9)),
           (pyr, dict(sigma=0.0)), (pyr, dict(sigma=nan)), (pyr, dict(min_size=0)), (pyr, dict(h=6)), (pyr, dict(w=5)),
           (pyr, dict(n=-1)), (pyr, dict(outb=ob.value - 1)), (pyr, dict(ws=null)), (pyr, dict(wsb=wb.value - 1)),
           (pyr, dict(sigma=9.0)), (pyr, dict(n=1 << 20, h=1 << 10, w=1 << 10)),
           (dog, dict(x=null)), (dog, dict(out=null)), (dog, dict(L=1)), (dog, dict(h=0)), (dog, dict(n=-1)),
           (dog, dict(n=1 << 20, h=1 << 10, w=1 << 10)),
           (ext, dict(x=null)), (ext, dict(mask=null)), (ext, dict(offs=null)), (ext, dict(vals=null)), (ext, dict(D=0)),
           (ext, dict(w=0)), (ext, dict(minima=2)), (ext, dict(n=-1)), (ext, dict(n=1 << 20, h=1 << 10, w=1 << 10)),
           (sel, dict(x=null)), (sel, dict(lafs=null)), (sel, dict(sc=null)), (sel, dict(cnt=null)), (sel, dict(num=0)),
           (sel, dict(num=8193)), (sel, dict(minima=-1)), (sel, dict(mr=0.0)), (sel, dict(mr=nan)), (sel, dict(ws=null)),
           (sel, dict(wsb=1024)), (sel, dict(levels=0)), (sel, dict(h=3)),
           (det, dict(x=null)), (det, dict(c=4)), (det, dict(kind=4)), (det, dict(kind=-1)), (det, dict(kind=0, k=nan)),
           (det, dict(h=6)), (det, dict(w=6)), (det, dict(num=0)), (det, dict(num=8193)), (det, dict(lafs=null)),
           (det, dict(sc=null)), (det, dict(cnt=null)), (det, dict(ws=null)), (det, dict(wsb=need - 1)), (det, dict(mr=-1.0)),
           (det, dict(minima=2)), (det, dict(levels=12)), (det, dict(min_size=-3))]
    for fn, kw in bad:
        assert fn(**kw) != 0, (fn.__name__, kw)
    for fn, name in ((blur, "rr_gaussian_blur"), (pyr, "rr_scale_pyramid"), (dog, "rr_dog_response"),
                     (ext, "rr_scale_space_extrema"), (sel, "rr_scale_space_select"), (det, "rr_detect_scale_space")):
        assert fn(x=null) != 0
        assert lib.rr_last_error().decode().startswith(name + ":"), name
    assert det(h=6) != 0 and "reflect" in lib.rr_last_error().decode()
    assert lib.rr_scale_pyramid_bytes(2, 1, 6, 56, 3, 1.6, 15, ctypes.byref(ob), ctypes.byref(wb)) != 0
    # an empty batch is no error (and launches nothing)
    assert blur(x=null, planes=0, out=null) == 0
    assert pyr(x=null, n=0, out=null) == 0
    assert dog(x=null, n=0, out=null) == 0
    assert ext(x=null, n=0, mask=null, offs=null, vals=null) == 0
    assert sel(x=null, n=0, lafs=null, sc=null, cnt=null) == 0
    assert det(x=null, n=0, lafs=null, sc=null, cnt=null) == 0


def test_python_refusals():
    from cirtorch.features import BlobDoG, BlobHessian, LAFOrienter, PassLAF, ScaleSpaceDetector, dog_response
    from cirtorch.filters import GaussianBlur2d, gaussian_blur2d
    from cirtorch.geometry.subpix import ConvQuadInterp3d, ConvSoftArgmax3d, conv_quad_interp3d
    from cirtorch.geometry.transform import ScalePyramid
    from cirtorch.search import detect_keypoints_scale_space

    x = torch.zeros(2, 1, 40, 56)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        gaussian_blur2d(x, (11, 11), (1.2, 1.2))
    with pytest.raises(NotImplementedError):
        gaussian_blur2d(x, (11, 11), (1.2, 1.2), "constant")
    with pytest.raises(TypeError):
        gaussian_blur2d(x, (10, 10), (1.2, 1.2))
    with pytest.raises(NotImplementedError):
        GaussianBlur2d((11, 13), (1.2, 1.2))
    with pytest.raises(ValueError, match="BxCxHxW"):
        gaussian_blur2d(x[0], (11, 11), (1.2, 1.2))

    with pytest.raises(NotImplementedError, match="double_image"):
        ScalePyramid(double_image=True)
    sp = ScalePyramid(3, 1.6, 15)
    assert sp.n_levels == 3 and sp.init_sigma == 1.6 and sp.extra_levels == 3 and abs(sp.sigma_step - 2 ** (1 / 3)) < 1e-15
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        sp(x)

    with pytest.raises(ValueError, match="BxCxDxHxW"):
        dog_response(x)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        BlobDoG()(torch.zeros(1, 1, 6, 8, 8))
    with pytest.raises(ValueError, match="BxCxDxHxW"):
        conv_quad_interp3d(x)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        ConvQuadInterp3d(10.0)(torch.zeros(1, 1, 5, 8, 8))
    with pytest.raises(NotImplementedError, match="every voxel"):
        ConvSoftArgmax3d((3, 3, 3), (1, 1, 1), (1, 1, 1), normalized_coordinates=False, output_value=True)(
            torch.zeros(1, 1, 5, 8, 8))

    det = ScaleSpaceDetector(100)
    assert isinstance(det.nms, ConvQuadInterp3d) and det.nms.strict_maxima_bonus == 10.0 and det.mr_size == 6.0
    assert isinstance(ScaleSpaceDetector(ori_module=LAFOrienter()).ori, LAFOrienter)
    with pytest.raises(NotImplementedError, match="nms_module"):
        ScaleSpaceDetector(nms_module=ConvSoftArgmax3d())
    with pytest.raises(NotImplementedError, match="aff_module"):
        ScaleSpaceDetector(aff_module=LAFOrienter())
    with pytest.raises(NotImplementedError, match="ori_module"):
        ScaleSpaceDetector(ori_module=BlobHessian())
    with pytest.raises(ValueError, match="scale_space_response"):
        ScaleSpaceDetector(resp_module=BlobDoG())
    assert ScaleSpaceDetector(resp_module=BlobDoG(), scale_space_response=True, minima_are_also_good=True)._kind == "dog"
    with pytest.raises(NotImplementedError, match="mask"):
        det(x, mask=torch.ones(2, 1, 40, 56))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        det(x)
    assert isinstance(det.aff, PassLAF)

    with pytest.raises(ValueError, match="response"):
        detect_keypoints_scale_space(x, response="sift")
    with pytest.raises(ValueError):
        detect_keypoints_scale_space(torch.zeros(2, 2, 40, 56))
    with pytest.raises(TypeError):
        detect_keypoints_scale_space(x.double())
    with pytest.raises(ValueError, match="num_features"):
        detect_keypoints_scale_space(x, num_features=0)
    for im in (x, x.to(torch.uint8), torch.zeros(1, 3, 40, 56)):
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            detect_keypoints_scale_space(im, response="dog")
