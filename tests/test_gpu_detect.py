"""GPU checks of keypoint detection (rr_response, rr_nms2d, rr_select_keypoints,
rr_detect_keypoints) against tests/golden/detect.npz and the numpy restatement of
tests/detect_cases.py."""

import numpy as np
import pytest
import torch

import detect_cases as DC
from conftest import golden
from oracle import data

pytestmark = pytest.mark.gpu

_G = {}


def G():
    if "g" not in _G:
        _G["g"] = golden("detect.npz")
    return _G["g"]


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def u8_pair(x, cuda):
    """uint8 pixels and their float32 values v / 255 by IEEE division (on the host: torch's device
    division by a scalar multiplies by the reciprocal)"""
    u8 = DC.to_u8(x)
    return dev(u8, cuda), dev(u8.astype(np.float32) / np.float32(255.0), cuda)


def case_images(k):
    return DC.images(k, int(G()["seeds"][k]))


def select_map(j):
    k, to_gray = DC.SELECT_MAPS[j]
    return (G()["g_harris"] if to_gray else G()["r%d_harris" % k])[:, 0]


def fns():
    from cirtorch.features import responses as R
    return {"harris": (lambda x, s=None: R.harris_response(x, DC.HARRIS_K, "sobel", s), R.CornerHarris(DC.HARRIS_K)),
            "gftt": (lambda x, s=None: R.gftt_response(x, "sobel", s), R.CornerGFTT()),
            "hessian": (lambda x, s=None: R.hessian_response(x, "sobel", s), R.BlobHessian())}


def close(got, ref, tol, what):
    assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape, what
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref.astype(np.float64)).max()
    print("%s: max |engine - reference float64| %.3g (tol %.3g)" % (what, err, tol))
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize("k", range(len(DC.CASES)))
def test_responses_vs_reference(cuda, k):
    """functions and modules within tol of the reference's float64 result: every plane of a C = 3
    batch on its own, with sigmas, and uint8 input bit-equal to the float32 path"""
    g = G()
    x = case_images(k)
    xt = dev(x, cuda)
    n = x.shape[0]
    for kind, (fn, mod) in fns().items():
        got = fn(xt)
        close(got, g["r%d_%s" % (k, kind)], float(g["tol_%s" % kind][k]), "case %d %s" % (k, kind))
        assert bits(mod.to(cuda)(xt)) == bits(got)
        assert bits(fn(xt)) == bits(got)   # run to run
        if k == DC.NOISE_CASE:
            sg = torch.tensor(DC.SIGMAS[:n], dtype=torch.float32, device=cuda)
            close(fn(xt, sg), g["sg_%s" % kind], float(g["sgtol_%s" % kind]), "case %d %s sigmas" % (k, kind))
            assert bits(mod(xt, sg)) == bits(fn(xt, sg))
        u8, unit = u8_pair(x, cuda)
        assert bits(fn(u8)) == bits(fn(unit))


@pytest.mark.parametrize("j", range(len(DC.SELECT_MAPS)))
def test_nms2d_equals_reference(cuda, j):
    from cirtorch.features.nms import NonMaximaSuppression2d, nms2d
    g = G()
    smap = select_map(j)
    xt = dev(smap[:, None], cuda)
    for ks in DC.NMS_SIZES:
        ref = np.unpackbits(g["m%d_ks%d" % (j, ks)])[:smap.size].reshape(smap.shape).astype(bool)
        mask = nms2d(xt, (ks, ks), mask_only=True)
        assert mask.dtype == torch.bool and tuple(mask.shape) == tuple(xt.shape)
        m = mask[:, 0].cpu().numpy()
        np.testing.assert_array_equal(m, ref)
        assert not (m[:, 0].any() or m[:, -1].any() or m[:, :, 0].any() or m[:, :, -1].any())
        sup = NonMaximaSuppression2d((ks, ks))(xt)
        assert sup.dtype == torch.float32
        assert bits(sup[:, 0]) == (smap * ref.astype(np.float32)).tobytes()


def check_lists(got, want, what):
    kp, sc, cnt = got
    assert kp.dtype == torch.float32 and sc.dtype == torch.float32 and cnt.dtype == torch.int32, what
    np.testing.assert_array_equal(cnt.cpu().numpy(), want[2], err_msg=what)
    np.testing.assert_array_equal(kp.cpu().numpy(), want[0], err_msg=what)
    assert bits(sc) == want[1].tobytes(), what


@pytest.mark.parametrize("j", range(len(DC.SELECT_MAPS)))
def test_select_keypoints_vs_reference(cuda, j):
    from cirtorch import _ops
    g = G()
    smap = select_map(j)
    st = dev(smap, cuda)
    for num in DC.NUMS:
        want = tuple(g["l%d_n%d_%s" % (j, num, f)] for f in ("kpts", "scores", "count"))
        got = _ops.select_keypoints(st, num, DC.SELECT_KS)
        check_lists(got, want, "map %d top-%d" % (j, num))
        cnt = want[2]
        for b in range(len(cnt)):   # padding slots
            assert (got[0][b, cnt[b]:] == -1).all() and (got[1][b, cnt[b]:] == 0).all()
    # min_score and border, against the restatement
    med = float(np.median(g["l%d_n%d_scores" % (j, 64)][0, :int(g["l%d_n%d_count" % (j, 64)][0])]))
    for ks, ms, border in ((3, 0.0, 0), (9, 0.0, 0), (5, med, 0), (5, 0.0, 7), (3, med, 11)):
        check_lists(_ops.select_keypoints(st, 96, ks, ms, border), DC.select(smap, ks, 96, ms, border),
                    "map %d ks %d min_score %g border %d" % (j, ks, ms, border))


def test_select_ties_nan_and_large_n(cuda):
    """planted exact ties resolve to the lower index; a NaN pixel is never selected (nor is a pixel
    with a NaN in its window: no comparison with NaN holds); num = 8192 with more candidates than
    num, against the restatement"""
    from cirtorch import _ops
    m = DC.tie_map()
    for ks in (3, 5, 9):
        check_lists(_ops.select_keypoints(dev(m, cuda), 16, ks), DC.select(m, ks, 16), "tie map ks %d" % ks)
        check_lists(_ops.select_keypoints(dev(m, cuda), 2, ks), DC.select(m, ks, 2), "tie map ks %d top-2" % ks)
    kp = _ops.select_keypoints(dev(m, cuda), 8, 5)[0][0, :5].cpu().numpy()
    np.testing.assert_array_equal(kp, [[25, 10], [28, 13], [5, 5], [20, 5], [9, 15]])
    bad = m.copy()
    bad[0, 5, 5] = np.nan
    bad[0, 15, 10] = np.nan     # next to the peak at (15, 9)
    got = _ops.select_keypoints(dev(bad, cuda), 16, 3)
    check_lists(got, DC.select(bad, 3, 16), "NaN map")
    pts = got[0][0, :int(got[2][0])].cpu().numpy().tolist()
    assert [5.0, 5.0] not in pts and [10.0, 15.0] not in pts and [9.0, 15.0] not in pts
    # a period-2 lattice of distinct peaks: 97 * 129 = 12513 candidates > 8192
    r = np.random.default_rng(DC.SEED + 7)
    big = np.zeros((2, 196, 260), dtype=np.float32)
    big[:, 1:-1:2, 1:-1:2] = (1.0 + r.permutation(2 * 97 * 129).reshape(2, 97, 129)).astype(np.float32)
    check_lists(_ops.select_keypoints(dev(big, cuda), 8192, 3), DC.select(big, 3, 8192), "lattice top-8192")
    check_lists(_ops.select_keypoints(dev(big, cuda), 100, 3), DC.select(big, 3, 100), "lattice top-100")


@pytest.mark.parametrize("kind", DC.KINDS)
def test_detect_equals_response_then_select(cuda, kind):
    """detect_keypoints == response -> select called separately, bit for bit; two runs agree; an
    image alone == the same image inside a batch of 3; the score map is within tol of the fixture"""
    from cirtorch import _ops
    from cirtorch.search import detect_keypoints
    g = G()
    for k, to_gray in ((DC.GRAY_CASE, True), (DC.NOISE_CASE, False)):
        x = case_images(k)
        xt = dev(x, cuda)
        kw = dict(num_features=80, response=kind, k=DC.HARRIS_K, nms=5)
        kp, sc, cnt, smap = detect_keypoints(xt, return_response=True, **kw)
        assert tuple(smap.shape) == (x.shape[0], 1) + x.shape[2:]
        close(smap, g["g_%s" % kind] if to_gray else g["r%d_%s" % (k, kind)],
              float(g["gtol_%s" % kind]) if to_gray else float(g["tol_%s" % kind][k]), "detect case %d %s map" % (k, kind))
        resp = _ops.response(xt, kind, DC.HARRIS_K, None, gray=to_gray)
        assert bits(resp) == bits(smap)
        kp2, sc2, cnt2 = _ops.select_keypoints(resp[:, 0], 80, 5)
        assert bits(kp) == bits(kp2) and bits(sc) == bits(sc2) and bits(cnt) == bits(cnt2)
        check_lists((kp, sc, cnt), DC.select(smap[:, 0].cpu().numpy(), 5, 80), "detect case %d %s" % (k, kind))
        assert int(cnt.min()) > 0
        again = detect_keypoints(xt, **kw)
        assert bits(again[0]) == bits(kp) and bits(again[1]) == bits(sc) and bits(again[2]) == bits(cnt)
        u8, unit = u8_pair(x, cuda)
        a, b = detect_keypoints(u8, **kw), detect_keypoints(unit, **kw)
        assert all(bits(p) == bits(q) for p, q in zip(a, b))
        for i in range(x.shape[0]):
            one = detect_keypoints(xt[i:i + 1], **kw)
            assert bits(one[0][0]) == bits(kp[i]) and bits(one[1][0]) == bits(sc[i]) and int(one[2][0]) == int(cnt[i])


def test_crop_equivariance(cuda):
    """scores whose response window (4) lies inside the crop are bit-identical at the shifted
    position; with the NMS window (2) inside as well, the keypoints are the image's, shifted"""
    from cirtorch.search import detect_keypoints
    img = data.structured_images(1, 96, 128, seed=DC.SEED + 50)
    y0, y1, x0, x1 = 16, 80, 24, 104
    full = dev(img, cuda)
    crop = full[:, :, y0:y1, x0:x1].contiguous()
    for kind, halo in (("harris", 4), ("gftt", 4), ("hessian", 2)):
        _, _, _, mf = detect_keypoints(full, 8192, kind, return_response=True)
        _, _, _, mc = detect_keypoints(crop, 8192, kind, return_response=True)
        inner = mc[0, 0, halo:(y1 - y0) - halo, halo:(x1 - x0) - halo]
        assert bits(inner) == bits(mf[0, 0, y0 + halo:y1 - halo, x0 + halo:x1 - halo]), kind
        margin = halo + 2
        kc, sc, cc = detect_keypoints(crop, 8192, kind, nms=5, border=margin)
        kf, sf, cf = detect_keypoints(full, 8192, kind, nms=5)
        kc, sc = kc[0, :int(cc[0])].cpu().numpy(), sc[0, :int(cc[0])].cpu().numpy()
        kf, sf = kf[0, :int(cf[0])].cpu().numpy(), sf[0, :int(cf[0])].cpu().numpy()
        inside = (kf[:, 0] >= x0 + margin) & (kf[:, 0] < x1 - margin) & (kf[:, 1] >= y0 + margin) & (kf[:, 1] < y1 - margin)
        assert len(kc) > 0 and len(kc) == int(inside.sum()), kind
        want = sorted((float(s), float(x - x0), float(y - y0)) for (x, y), s in zip(kf[inside], sf[inside]))
        assert sorted((float(s), float(x), float(y)) for (x, y), s in zip(kc, sc)) == want, kind


def test_graph_capture_replay_equals_eager(cuda):
    from cirtorch.search import detect_keypoints
    from cirtorch.utils.graph import GraphedForward
    xs = [dev(DC.to_u8(data.structured_images(2, 48, 64, seed=DC.SEED + 60 + i)), cuda) for i in range(2)]

    def fn(t):
        return detect_keypoints(t, 64, "harris", nms=5, return_response=True)

    g = GraphedForward(fn, xs[0])
    for t in (xs[1], xs[0]):
        got = [o.clone() for o in g(t)]
        want = fn(t)
        assert all(bits(a) == bits(b) for a, b in zip(got, want))
        assert int(want[2].min()) > 0


def test_chain_detect_describe_match_verify(cuda):
    """image -> keypoints -> descriptors -> matches -> inliers with no host step: shapes, dtypes and
    devices connect, and the keypoints passed on are the ones detected.  The second image is a
    translated crop of the first; the recovered H is not asserted (the descriptors come from a
    random feature map)."""
    from cirtorch.geometry.conversions import denormalize_pixel_coordinates, normalize_pixel_coordinates
    from cirtorch.modules.heads.local_head import localHead
    from cirtorch.search import detect_keypoints, match_pairs, verify_pairs
    n, th = 32, 3.0
    img = data.structured_images(1, 96, 128, seed=DC.SEED + 70)
    full = dev(img, cuda)
    y0, x0, h, w = 8, 12, 80, 104
    views = [full[:, :, :h, :w].contiguous(), full[:, :, y0:y0 + h, x0:x0 + w].contiguous()]
    torch.manual_seed(3)
    head = localHead(16, 32).to(cuda).eval()
    fmap = torch.randn(1, 16, 96 // 4, 128 // 4, device=cuda)
    # the feature map of a view: the crop of the full map at stride 4 (y0, x0 are multiples of 4)
    feats = [fmap[:, :, :h // 4, :w // 4].contiguous(), fmap[:, :, y0 // 4:(y0 + h) // 4, x0 // 4:(x0 + w) // 4].contiguous()]
    kps, descs = [], []
    for v, f in zip(views, feats):
        kp, sc, cnt = detect_keypoints(v, n, "harris", nms=5, border=8)
        assert kp.shape == (1, n, 2) and kp.dtype == torch.float32 and kp.device == v.device
        assert sc.shape == (1, n) and cnt.shape == (1,) and int(cnt[0]) == n
        grid = normalize_pixel_coordinates(kp, h, w)
        assert grid.shape == kp.shape and grid.device == kp.device and float(grid.abs().max()) <= 1.0
        torch.testing.assert_close(denormalize_pixel_coordinates(grid, h, w), kp, rtol=0, atol=1e-3)
        d = head(f, grid)
        assert d.shape == (1, n, 32) and d.dtype == torch.float32 and d.device == kp.device
        kps.append(kp)
        descs.append(d)
    match, dist = match_pairs(descs[0], descs[1], mode="mnn")
    assert match.shape == (1, n) and match.dtype == torch.int64 and match.device == kps[0].device
    inl, H, mask = verify_pairs(kps[0], kps[1], match, th=th, iters=512, seed=1)
    assert inl.shape == (1,) and H.shape == (1, 3, 3) and mask.shape == (1, n) and mask.dtype == torch.bool
    assert int(inl[0]) == int(mask.sum()) and int(inl[0]) <= int((match >= 0).sum())
    # the keypoints passed on are the ones detected: whole pixels inside the border, and every
    # verified row is a matched row
    for kp in kps:
        assert bits(kp) == bits(kp.round()) and float(kp.min()) >= 8
        assert float(kp[..., 0].max()) < w - 8 and float(kp[..., 1].max()) < h - 8
    assert bool((match[mask] >= 0).all())
    print("chain: %d matches, %d inliers" % (int((match >= 0).sum()), int(inl[0])))
