"""CPU checks of keypoint detection's host side: the detect.npz fixture (generator checksum, the
numpy restatement of rr_response / rr_nms2d / rr_select_keypoints against the reference's
results), the workspace function, the argument checks of the four entries (which return before
anything is enqueued, so they run without a GPU) and the Python surface's refusals."""

import ctypes
import os

import numpy as np
import pytest
import torch

import detect_cases as DC
from conftest import PKG, golden

LIB = os.path.join(PKG, "librr.so")


def test_fixture_checksum_and_cases():
    g = golden("detect.npz")
    assert [tuple(int(v) for v in c) for c in g["cases"]] == DC.CASES
    assert DC.CASES[-1][2:] == (DC.TILE + 1, DC.TILE + 1)
    for k, (n, c, h, w) in enumerate(DC.CASES):
        x = DC.images(k, int(g["seeds"][k]))
        assert x.dtype == np.float32 and x.shape == (n, c, h, w)
        np.testing.assert_allclose(DC.checksum(x)[0], g["chk"][k], rtol=0, atol=1e-9)


@pytest.mark.parametrize("k", range(len(DC.CASES)))
def test_restatement_responses(k):
    """the float64 restatement stays within tol / 2 of the reference's float64 result (here: of its
    float32 rounding, which adds at most half a float32 ulp of the score)"""
    g = golden("detect.npz")
    x = DC.images(k, int(g["seeds"][k]))
    n = x.shape[0]
    for kind in DC.KINDS:
        checks = [(DC.response(x, kind), g["r%d_%s" % (k, kind)], float(g["tol_%s" % kind][k]))]
        if k == DC.GRAY_CASE:
            checks.append((DC.response(x, kind, to_gray=True), g["g_%s" % kind], float(g["gtol_%s" % kind])))
        if k == DC.NOISE_CASE:
            checks.append((DC.response(x, kind, sigmas=DC.SIGMAS[:n]), g["sg_%s" % kind], float(g["sgtol_%s" % kind])))
        for mine, ref, tol in checks:
            assert ref.dtype == np.float32 and ref.shape == mine.shape and tol > 0
            ulp = float(np.spacing(np.abs(ref).max()))
            assert np.abs(mine - ref.astype(np.float64)).max() <= tol / 2 + ulp / 2, (kind, tol)


@pytest.mark.parametrize("j", range(len(DC.SELECT_MAPS)))
def test_restatement_masks_and_lists(j):
    g = golden("detect.npz")
    k, to_gray = DC.SELECT_MAPS[j]
    smap = (g["g_harris"] if to_gray else g["r%d_harris" % k])[:, 0]
    for ks in DC.NMS_SIZES:
        ref = np.unpackbits(g["m%d_ks%d" % (j, ks)])[:smap.size].reshape(smap.shape).astype(bool)
        mine = DC.nms_mask(smap, ks)
        np.testing.assert_array_equal(mine, ref)
        assert not (ref[:, 0].any() or ref[:, -1].any() or ref[:, :, 0].any() or ref[:, :, -1].any())
        assert ref.reshape(len(ref), -1).sum(1).max() <= DC.candidate_bound(*smap.shape[1:])
    for num in DC.NUMS:
        kp, sc, cnt = DC.select(smap, DC.SELECT_KS, num)
        np.testing.assert_array_equal(kp, g["l%d_n%d_kpts" % (j, num)])
        np.testing.assert_array_equal(sc, g["l%d_n%d_scores" % (j, num)])
        np.testing.assert_array_equal(cnt, g["l%d_n%d_count" % (j, num)])
    assert (g["l%d_n%d_count" % (j, DC.NUMS[-1])] < DC.NUMS[-1]).all()   # N above the candidate count


def test_restatement_tie_map():
    m = DC.tie_map()
    for ks, both in ((3, True), (5, True), (9, False)):
        keep = DC.nms_mask(m, ks)[0]
        assert keep[5, 5] and keep[5, 20] and keep[15, 9]
        assert bool(keep[10, 25]) == both and bool(keep[13, 28]) == both
        assert not keep[18:22, 3:8].any() and not keep[0, 12] and not keep[10, 14]
    kp, sc, cnt = DC.select(m, 5, 8)
    assert cnt[0] >= 5
    np.testing.assert_array_equal(kp[0, :5], [[25, 10], [28, 13], [5, 5], [20, 5], [9, 15]])   # ties: the lower index first
    np.testing.assert_array_equal(sc[0, :5], np.float32([0.75, 0.75, 0.5, 0.5, 0.5]))


def _lib():
    if not os.path.exists(LIB):
        pytest.skip("librr.so not built (run __graft_entry__.build())")
    from cirtorch import _engine
    return _engine, _engine.lib()


def test_workspace_bytes_and_candidate_bound():
    E, lib = _lib()
    f = lib.rr_detect_workspace_bytes
    for n, h, w in ((1, 4, 4), (2, 37, 53), (3, 48, 64), (128, 768, 1024)):
        need = f(n, h, w, 2048)
        # the score map, one 8-byte key per possible candidate, one counter per image
        assert need >= n * h * w * 4 + n * DC.candidate_bound(h, w) * 8 + n * 4
        assert f(n + 1, h, w, 2048) >= need and f(n, h + 1, w, 2048) >= need and f(n, h, w + 1, 2048) >= need
        assert f(n, h, w, 8192) >= f(n, h, w, 1)
    assert f(0, 48, 64, 16) > 0
    # no two 8-neighbours are both strict maxima: a checkerboard of period 2 reaches the bound
    for h, w in ((7, 9), (8, 8)):
        m = np.zeros((1, h + 2, w + 2), dtype=np.float32)
        m[0, 1:-1:2, 1:-1:2] = 1.0
        assert DC.nms_mask(m, 3).sum() == DC.candidate_bound(h, w) <= DC.candidate_bound(h + 2, w + 2)


def test_detect_argument_checks():
    """every refusal happens on the host: these calls pass made-up device addresses and must return
    before a kernel launch"""
    E, lib = _lib()
    p = ctypes.c_void_p(0x1000)   # "non-null, aligned"; never dereferenced
    null = ctypes.c_void_p(0)
    need = lib.rr_detect_workspace_bytes(2, 16, 16, 64)

    def resp(x=p, n=2, c=1, h=16, w=16, gray=0, kind=E.RR_RESP_HARRIS, k=0.04, out=p):
        return lib.rr_response(x, n, c, h, w, 0, gray, kind, k, null, out, null)

    def nms(x=p, planes=2, h=16, w=16, ks=5, out=p):
        return lib.rr_nms2d(x, planes, h, w, ks, 1, out, null)

    def sel(x=p, n=2, h=16, w=16, ks=5, num=64, min_score=0.0, border=0, kp=p, sc=p, cnt=p, ws=p, wsb=need):
        return lib.rr_select_keypoints(x, n, h, w, ks, num, min_score, border, kp, sc, cnt, ws, wsb, null)

    def det(x=p, n=2, c=1, h=16, w=16, kind=E.RR_RESP_GFTT, ks=5, num=64, border=0, kp=p, sc=p, cnt=p, ws=p, wsb=need):
        return lib.rr_detect_keypoints(x, n, c, h, w, 0, kind, 0.04, null, ks, num, 0.0, border, kp, sc, cnt, null, ws, wsb,
                                       null)

    bad = [(resp, dict(x=null)), (resp, dict(out=null)), (resp, dict(kind=3)), (resp, dict(kind=-1)), (resp, dict(h=3)),
           (resp, dict(w=3)), (resp, dict(gray=1)), (resp, dict(gray=1, c=4)), (resp, dict(gray=2, c=3)), (resp, dict(c=0)),
           (resp, dict(n=-1)), (resp, dict(k=float("nan"))), (resp, dict(n=1 << 10, h=1 << 10, w=(1 << 11) + 1)),
           (resp, dict(n=1 << 30, c=1 << 30, h=1 << 30, w=1 << 30)),
           (nms, dict(x=null)), (nms, dict(out=null)), (nms, dict(ks=4)), (nms, dict(ks=1)), (nms, dict(ks=11)),
           (nms, dict(h=0)), (nms, dict(planes=-1)), (nms, dict(planes=1 << 40)),
           (sel, dict(x=null)), (sel, dict(kp=null)), (sel, dict(sc=null)), (sel, dict(cnt=null)), (sel, dict(ks=6)),
           (sel, dict(num=0)), (sel, dict(num=8193)), (sel, dict(h=0)), (sel, dict(w=0)), (sel, dict(border=-1)),
           (sel, dict(min_score=float("nan"))), (sel, dict(ws=null)), (sel, dict(wsb=need - 257)), (sel, dict(n=-1)),
           (det, dict(x=null)), (det, dict(c=2)), (det, dict(c=4)), (det, dict(kind=7)), (det, dict(h=3)), (det, dict(ks=2)),
           (det, dict(num=0)), (det, dict(num=8193)), (det, dict(kp=null)), (det, dict(sc=null)), (det, dict(cnt=null)),
           (det, dict(ws=null)), (det, dict(wsb=need - 257)), (det, dict(border=-2))]
    for fn, kw in bad:
        assert fn(**kw) != 0, (fn.__name__, kw)
    for fn, name in ((resp, "rr_response"), (nms, "rr_nms2d"), (sel, "rr_select_keypoints"), (det, "rr_detect_keypoints")):
        assert fn(x=null) != 0
        assert lib.rr_last_error().decode().startswith(name), name
    # exactly 2^31 pixels is still a size the checks accept: the refusal comes from the null input
    assert resp(x=null, n=1 << 10, h=1 << 10, w=1 << 11) != 0
    assert "null" in lib.rr_last_error().decode()
    # an empty batch is no error (and launches nothing)
    assert resp(x=null, n=0, out=null) == 0
    assert nms(x=null, planes=0, out=null) == 0
    assert sel(x=null, n=0, kp=null, sc=null, cnt=null) == 0
    assert det(x=null, n=0, kp=null, sc=null, cnt=null) == 0


def test_response_errors_match_the_reference():
    from cirtorch.features import responses as R
    x = torch.zeros(2, 1, 8, 8)
    for fn in (R.harris_response, R.gftt_response, R.hessian_response):
        with pytest.raises(ValueError, match="BxCxHxW"):
            fn(torch.zeros(8, 8))
        with pytest.raises(NotImplementedError):
            fn(x, grads_mode="diff")
        with pytest.raises(TypeError):
            fn(x, grads_mode="scharr")
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            fn(x)
    with pytest.raises(TypeError, match="sigmas type"):
        R.harris_response(x, sigmas=[1.0, 1.0])
    for fn in (R.harris_response, R.hessian_response):
        with pytest.raises(ValueError, match="sigmas shape"):
            fn(x, sigmas=torch.ones(3))
        with pytest.raises(ValueError, match="sigmas shape"):
            fn(x, sigmas=torch.ones(2, 1))
    m = R.CornerHarris(torch.tensor(0.05))
    assert "k" in dict(m.named_buffers()) and abs(m._k - 0.05) < 1e-8
    assert float(R.CornerHarris(0.04).k) == pytest.approx(0.04)
    for mod in (m, R.CornerGFTT(), R.BlobHessian()):
        assert mod.grads_mode == "sobel"
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            mod(x)
    with pytest.raises(NotImplementedError):
        R.BlobHessian("diff")(x)


def test_nms_errors():
    from cirtorch.features import nms as N
    x = torch.zeros(1, 1, 8, 8)
    with pytest.raises(NotImplementedError, match="scale pyramid"):
        N.nms3d(torch.zeros(1, 1, 3, 8, 8), (3, 3, 3))
    with pytest.raises(ValueError, match="square"):
        N.nms2d(x, (3, 5))
    with pytest.raises(ValueError):
        N.nms2d(x, (4, 4))
    with pytest.raises(AssertionError):
        N.nms2d(x, 3)
    with pytest.raises(AssertionError):
        N.nms2d(torch.zeros(8, 8), (3, 3))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        N.nms2d(x, (3, 3))
    assert N.NonMaximaSuppression2d((5, 5)).kernel_size == (5, 5)


def test_detect_keypoints_refusals():
    from cirtorch.search import detect_keypoints
    x = torch.zeros(2, 3, 16, 16)
    with pytest.raises(ValueError, match="response"):
        detect_keypoints(x, response="dog")
    with pytest.raises(ValueError):
        detect_keypoints(torch.zeros(2, 2, 16, 16))
    with pytest.raises(ValueError):
        detect_keypoints(torch.zeros(3, 16, 16))
    with pytest.raises(TypeError):
        detect_keypoints(x.double())
    with pytest.raises(ValueError, match="square"):
        detect_keypoints(x, nms=(3, 5))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        detect_keypoints(x)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        detect_keypoints(x.to(torch.uint8))


def test_pixel_coordinate_conversions():
    from cirtorch.geometry.conversions import denormalize_pixel_coordinates, normalize_pixel_coordinates
    h, w = 48, 64
    p = torch.tensor([[0.0, 0.0], [63.0, 47.0], [31.5, 23.5], [10.0, 40.0]])
    q = normalize_pixel_coordinates(p, h, w)
    torch.testing.assert_close(q[:3], torch.tensor([[-1.0, -1.0], [1.0, 1.0], [0.0, 0.0]]), rtol=0, atol=1e-6)
    expect = torch.tensor(2.0) / torch.tensor([63.0, 47.0]) * p - 1
    assert torch.equal(q, expect)
    torch.testing.assert_close(denormalize_pixel_coordinates(q, h, w), p, rtol=0, atol=1e-4)
    assert torch.isfinite(normalize_pixel_coordinates(p, 1, 1)).all()   # size 1: the clamp by eps
    for fn in (normalize_pixel_coordinates, denormalize_pixel_coordinates):
        with pytest.raises(ValueError, match=r"\(\*, 2\)"):
            fn(torch.zeros(4, 3), h, w)
