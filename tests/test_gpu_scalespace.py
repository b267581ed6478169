"""GPU checks of scale-space detection (rr_gaussian_blur, rr_scale_pyramid, rr_dog_response,
rr_scale_space_extrema, rr_scale_space_select, rr_detect_scale_space) against
tests/golden/scalespace.npz and the numpy restatement of tests/scalespace_cases.py."""

import numpy as np
import pytest
import torch

import scalespace_cases as SC
from conftest import golden

pytestmark = pytest.mark.gpu

_G = {}


def G():
    if "g" not in _G:
        _G["g"] = golden("scalespace.npz")
    return _G["g"]


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def case_images(k):
    return SC.images(k, int(G()["seeds"][k]))


def case_input(k, cuda):
    """the tensor the engine gets: the bytes of the uint8 case, float32 otherwise"""
    x = case_images(k)
    return dev(SC.as_u8(x), cuda) if k == SC.U8_CASE else dev(x, cuda)


def restated(j):
    """the restatement's lists of list j, computed once"""
    if ("r", j) not in _G:
        k, kind, mr, minima, num = SC.LISTS[j]
        _G[("r", j)] = SC.detect(case_images(k), kind, num, mr, minima)
    return _G[("r", j)]


def np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("k", SC.PYRAMID_CASES)
def test_pyramid_vs_reference(cuda, k):
    """every level within tol_l = max |reference float32 run - reference float64 run| of the reference's
    float64 levels; sizes and sigma lists equal; uint8 bit-equal to x.float() / 255; run to run"""
    from cirtorch.geometry.transform import ScalePyramid
    g = G()
    sp = ScalePyramid(SC.LEVELS, SC.SIGMA, SC.MIN_SIZE)
    x = case_input(k, cuda)
    pyr, sigmas, dists = sp(x)
    _, octs = SC.plan(*SC.CASES[k][2:])
    assert len(pyr) == len(sigmas) == len(dists) == len(octs)
    n = SC.CASES[k][0]
    for oi, (lv, o) in enumerate(zip(pyr, octs)):
        ref, tol = g["p%d_%d" % (k, oi)], g["ptol%d_%d" % (k, oi)]
        assert lv.dtype == torch.float32 and tuple(lv.shape) == (n, 1, SC.L, o["h"], o["w"])
        err = np.abs(np64(lv[:, 0]) - ref).max(axis=(0, 2, 3))
        print("case %d octave %d: max |engine - reference float64| per level %s (tol %s)" % (k, oi, err, tol))
        assert (err <= tol).all(), (k, oi, err, tol)
        assert bits(sigmas[oi]) == bits(torch.tensor(o["sigmas"], dtype=torch.float32).repeat(n, 1))
        assert bits(dists[oi]) == bits(torch.full((n, SC.L), float(2 ** oi)))
    again = sp(x)[0]
    assert all(bits(a) == bits(b) for a, b in zip(pyr, again))
    if k == SC.U8_CASE:
        unit = sp(dev(case_images(k), cuda))[0]
        assert all(bits(a) == bits(b) for a, b in zip(pyr, unit))


def test_gaussian_blur_vs_reference(cuda):
    from cirtorch.filters import GaussianBlur2d, gaussian_blur2d
    g = G()
    x = dev(case_images(1), cuda)
    for j, (ks, s) in enumerate(SC.BLUR_SIZES):
        got = gaussian_blur2d(x, (ks, ks), (s, s))
        err = np.abs(np64(got) - g["b%d" % j]).max()
        print("blur %d taps: max |engine - reference float64| %.3g (tol %.3g)" % (ks, err, g["btol"][j]))
        assert got.dtype == torch.float32 and got.shape == x.shape and err <= g["btol"][j]
        assert bits(GaussianBlur2d((ks, ks), (s, s))(x)) == bits(got)
        assert bits(gaussian_blur2d(x[1:], (ks, ks), (s, s))) == bits(got[1:])   # independent of the batch
    # more than 43 taps take the 16-wide tile; a plane of one tile row; against the restatement
    y = case_images(3)
    for ks, s in ((45, 5.5), (63, 7.9)):
        if ks // 2 < min(y.shape[2:]):
            got = gaussian_blur2d(dev(y, cuda), (ks, ks), (s, s))
            assert np.abs(np64(got) - SC.blur(y, ks, s)).max() <= 6e-8   # half a float32 ulp below 1
    wide = np.random.default_rng(SC.SEED + 5).random((1, 1, 40, 70)).astype(np.float32)
    for ks, s in ((45, 5.5), (63, 7.9)):
        got = gaussian_blur2d(dev(wide, cuda), (ks, ks), (s, s))
        assert np.abs(np64(got) - SC.blur(wide, ks, s)).max() <= 6e-8


def test_extrema_vs_reference(cuda):
    """on the golden float32 response volumes the decisions are exact: the candidate set equals the
    reference's nms3d mask; offsets (the reference's second and third swapped back) and refined values
    within the reference's float32-vs-float64 difference"""
    from cirtorch import _ops
    from cirtorch.geometry.subpix import ConvQuadInterp3d
    g = G()
    for oi in range(2):
        v = g["v_%d" % oi]
        ref = np.unpackbits(g["vm_%d" % oi])[:v.size].reshape(v.shape).astype(bool)
        mask, offs, vals = _ops.scale_space_extrema(dev(v, cuda))
        np.testing.assert_array_equal(mask.cpu().numpy() == 1, ref)
        mb = np.broadcast_to(ref[:, None], tuple(offs.shape))
        eo = np.abs(np64(offs)[mb] - g["vo_%d" % oi]).max()
        ev = np.abs(np64(vals)[ref] - g["vv_%d" % oi]).max()
        print("volume %d: offsets %.3g (tol %.3g), values %.3g (tol %.3g)" % (oi, eo, g["votol"], ev, g["vvtol"]))
        # the fixture stores the float64 results as float32: half an ulp of 0.7 and of the values
        assert eo <= float(g["votol"]) + 3e-8 and ev <= float(g["vvtol"]) + np.spacing(np.float32(np.abs(v).max())) / 2
        assert (np64(offs)[~mb] == 0).all() and bits(vals[~torch.from_numpy(ref)]) == bits(dev(v, cuda)[~torch.from_numpy(ref)])
        # the module: coordinates (level, x, y) and the bonus on y_max
        co, ym = ConvQuadInterp3d(10.0)(dev(v, cuda)[:, None])
        assert tuple(co.shape) == (v.shape[0], 1, 3) + v.shape[1:] and tuple(ym.shape) == (v.shape[0], 1) + v.shape[1:]
        D, H, W = v.shape[1:]
        grid = np.stack(np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij"))[[0, 2, 1]]
        np.testing.assert_array_equal(co[:, 0].cpu().numpy(), (grid[None] + offs.cpu().numpy()).astype(np.float32))
        np.testing.assert_array_equal(ym[:, 0].cpu().numpy(), vals.cpu().numpy() + np.float32(10.0) * ref)


def test_extrema_planted_volume(cuda):
    """equal neighbouring peaks, a plateau, a peak on each face, a negative hole with and without minima,
    an offset just above and just below 0.7: against the restatement"""
    from cirtorch import _ops
    v = SC.planted_volume()
    for minima in (False, True):
        m, offs, vals = SC.extrema(v, minima)
        mask, go, gv = _ops.scale_space_extrema(dev(v, cuda), minima)
        np.testing.assert_array_equal(mask.cpu().numpy(), m)
        assert np.abs(np64(go) - offs).max() <= 1e-6 and np.abs(np64(gv) - vals).max() <= 1e-5
    d, y, x = SC.PLANTED_BELOW
    assert abs(float(go[0, 1, d, y, x]) - 0.69) < 1e-5 and float(gv[0, d, y, x]) > float(v[0, d, y, x])
    d, y, x = SC.PLANTED_ABOVE
    assert not go[0, :, d, y, x].any() and float(gv[0, d, y, x]) == float(v[0, d, y, x])
    nan = v.copy()
    nan[0, 2, 10, 19] = np.nan                         # beside the ordinary peak at (2, 10, 20)
    mask = _ops.scale_space_extrema(dev(nan, cuda), True)[0]
    assert int(mask[0, 2, 10, 20]) == 0 and int(mask[0, 2, 10, 19]) == 0


@pytest.mark.parametrize("j", range(len(SC.LISTS)))
def test_lists_vs_reference(cuda, j):
    """voxels, order and count equal the reference's (through the restatement, which the host tests pin
    to the fixture's voxels); scores and LAF entries within the stored tolerance of the reference"""
    from cirtorch.search import detect_keypoints_scale_space
    g = G()
    k, kind, mr, minima, num = SC.LISTS[j]
    lafs, scores, count = detect_keypoints_scale_space(case_input(k, cuda), num, kind, SC.LEVELS, SC.SIGMA, SC.MIN_SIZE, mr,
                                                       minima)
    n = SC.CASES[k][0]
    assert tuple(lafs.shape) == (n, num, 2, 3) and tuple(scores.shape) == (n, num) and tuple(count.shape) == (n,)
    assert lafs.dtype == scores.dtype == torch.float32 and count.dtype == torch.int32
    np.testing.assert_array_equal(count.cpu().numpy(), g["l%d_count" % j])
    el = np.abs(np64(lafs) - g["l%d_lafs" % j]).max()
    es = np.abs(np64(scores) - g["l%d_scores" % j]).max()
    print("list %d: lafs %.3g (tol %.3g), scores %.3g (tol %.3g)" % (j, el, g["l%d_ltol" % j], es, g["l%d_stol" % j]))
    # the fixture stores the float64 lists as float32: half an ulp of the largest coordinate, 128
    assert el <= float(g["l%d_ltol" % j]) + 4e-6 and es <= float(g["l%d_stol" % j]) + 1e-9
    # the same voxels in the same order: a frame's centre identifies its voxel to within the 0.7 offset
    rl, rs, rc, vox = restated(j)
    _, octs = SC.plan(*SC.CASES[k][2:])
    H, W = SC.CASES[k][2:]
    got = lafs.cpu().numpy()
    for b in range(n):
        for i, (oi, idx, off) in enumerate(vox[b]):
            o = octs[oi]
            assert oi == int(g["l%d_oct" % j][b, i]) and idx == int(g["l%d_vox" % j][b, i])
            x, y = got[b, i, 0, 2] * o["w"] / W, got[b, i, 1, 2] * o["h"] / H
            assert abs(x - (idx % o["w"] + off[0])) < 1e-3 and abs(y - (idx // o["w"] % o["h"] + off[1])) < 1e-3
            d = idx // (o["w"] * o["h"])
            a = mr * o["sigmas"][0] * 2 ** ((d + off[2]) / SC.LEVELS) * min(H, W) / min(o["h"], o["w"])
            assert abs(got[b, i, 0, 0] - a) < 1e-3 * a and got[b, i, 0, 0] == got[b, i, 1, 1]
        c = int(count[b])
        assert not lafs[b, c:].any() and not scores[b, c:].any() and not lafs[b, :, 0, 1].any() and not lafs[b, :, 1, 0].any()
    assert np.abs(np64(scores) - rs).max() <= 1e-6 and np.abs(np64(lafs) - rl).max() <= 1e-3


@pytest.mark.parametrize("num", SC.SMALL_NUMS)
def test_small_n(cuda, num):
    from cirtorch.search import detect_keypoints_scale_space
    x = dev(case_images(0), cuda)
    rl, rs, rc, _ = restated(0)
    lafs, scores, count = detect_keypoints_scale_space(x, num, "hessian", mr_size=1.0)
    assert count.tolist() == [num] * x.shape[0]
    assert np.abs(np64(lafs) - rl[:, :num]).max() <= 1e-3 and np.abs(np64(scores) - rs[:, :num]).max() <= 1e-6
    full = detect_keypoints_scale_space(x, 64, "hessian", mr_size=1.0)
    assert bits(lafs) == bits(full[0][:, :num]) and bits(scores) == bits(full[1][:, :num])


@pytest.mark.parametrize("kind,k", [("hessian", 0), ("dog", SC.BLOB_CASE), ("harris", SC.U8_CASE)])
def test_fused_equals_staged_batch_and_runs(cuda, kind, k):
    """rr_detect_scale_space is bit-identical to the staged entries, a batch to each image alone, a run
    to the next, uint8 to x.float() / 255"""
    from cirtorch import _ops
    from cirtorch.features import responses as R
    x = case_input(k, cuda)
    n, c, h, w = x.shape
    minima, mr, num = kind == "dog", 0.5, 32   # small frames: every image keeps some
    fused = _ops.detect_scale_space(x, num, kind, SC.LEVELS, SC.SIGMA, SC.MIN_SIZE, mr, minima, 0.04, return_pyramid=True)
    assert int(fused[2].min()) > 0
    pyr, octs = _ops.scale_pyramid(x, SC.LEVELS, SC.SIGMA, SC.MIN_SIZE)
    assert all(bits(a) == bits(b) for a, b in zip(pyr, fused[3]))
    total = octs[-1]["off"] + n * SC.L * octs[-1]["h"] * octs[-1]["w"]
    resp = torch.zeros(total, dtype=torch.float32, device=cuda)
    for lv, o in zip(pyr, octs):
        view = resp[o["off"]:o["off"] + lv.numel()].view(n, SC.L, o["h"], o["w"])
        if kind == "dog":
            view[:, :-1] = R.dog_response(lv)[:, 0]
        else:
            sg = torch.tensor(o["sigmas"], dtype=torch.float32, device=cuda).repeat(n)
            fn = R.hessian_response if kind == "hessian" else R.harris_response
            view.copy_(fn(lv[:, 0].reshape(n * SC.L, 1, o["h"], o["w"]), sigmas=sg).view(n, SC.L, o["h"], o["w"]))
    staged = _ops.scale_space_select(resp, n, h, w, num, SC.LEVELS, SC.SIGMA, SC.MIN_SIZE, minima, mr)
    assert all(bits(a) == bits(b) for a, b in zip(staged, fused[:3]))
    again = _ops.detect_scale_space(x, num, kind, SC.LEVELS, SC.SIGMA, SC.MIN_SIZE, mr, minima, 0.04)
    assert all(bits(a) == bits(b) for a, b in zip(again, fused[:3]))
    for b in range(n):
        one = _ops.detect_scale_space(x[b:b + 1], num, kind, SC.LEVELS, SC.SIGMA, SC.MIN_SIZE, mr, minima, 0.04)
        assert all(bits(a) == bits(f[b:b + 1]) for a, f in zip(one, fused[:3]))
    if k == SC.U8_CASE:
        unit = _ops.detect_scale_space(dev(case_images(k), cuda), num, kind, SC.LEVELS, SC.SIGMA, SC.MIN_SIZE, mr, minima, 0.04)
        assert all(bits(a) == bits(b) for a, b in zip(unit, fused[:3]))


def test_graph_capture_replay_equals_eager(cuda):
    from cirtorch.search import detect_keypoints_scale_space
    from cirtorch.utils.graph import GraphedForward
    xs = [dev(SC.images(0, SC.SEED + 500 + i), cuda) for i in range(2)]

    def fn(t):
        return detect_keypoints_scale_space(t, 32, "hessian", mr_size=1.0)

    gr = GraphedForward(fn, xs[0])
    for t in (xs[1], xs[0]):
        got = [o.clone() for o in gr(t)]
        want = fn(t)
        assert all(bits(a) == bits(b) for a, b in zip(got, want))
        assert int(want[2].min()) > 0


def test_blobs_found_and_refined_on_their_own_axes(cuda):
    """every planted blob has a keypoint within a pixel, and its sub-pixel x and y move toward the true
    centre: this fails when the x offset is added to y and the y offset to x"""
    from cirtorch.search import detect_keypoints_scale_space
    seed = int(G()["seeds"][SC.BLOB_CASE])
    img, planted = SC.blobs(seed)
    lafs, scores, count = detect_keypoints_scale_space(dev(img, cuda), 64, "dog", mr_size=2.0)
    rl, rs, rc, vox = SC.detect(img, "dog", 64, 2.0, True)
    c = int(count[0])
    assert c == int(rc[0]) and np.abs(np64(lafs) - rl).max() <= 1e-3
    SC.check_blobs(lafs[0, :c].cpu().numpy(), vox[0], planted, SC.plan(*img.shape[2:])[1])
    # the transposed image gives the transposed keypoints: x and y are treated alike
    lt, st, ct = detect_keypoints_scale_space(dev(np.ascontiguousarray(img.transpose(0, 1, 3, 2)), cuda), 64, "dog", mr_size=2.0)
    assert int(ct[0]) == c
    a = np64(lafs)[0, :c][np.argsort(-np64(scores)[0, :c], kind="stable")]
    b = np64(lt)[0, :c][np.argsort(-np64(st)[0, :c], kind="stable")]
    assert np.abs(a[:, 0, 2] - b[:, 1, 2]).max() < 1e-3 and np.abs(a[:, 1, 2] - b[:, 0, 2]).max() < 1e-3


def test_detector_module_and_pipeline(cuda):
    """ScaleSpaceDetector returns what the reference returns, (lafs, responses); its frames go
    through describe_keypoints, match_pairs and verify_pairs with no host step"""
    from cirtorch.features import BlobDoG, LAFOrienter, ScaleSpaceDetector, get_laf_center
    from cirtorch.geometry.transform import ScalePyramid
    from cirtorch.search import describe_keypoints, detect_keypoints_scale_space, match_pairs, verify_pairs
    img, _ = SC.blobs(SC.SEED + 77)
    x = dev(img, cuda)
    det = ScaleSpaceDetector(32, 2.0, ScalePyramid(3, 1.6, 15), BlobDoG(), minima_are_also_good=True,
                             scale_space_response=True).to(cuda)
    lafs, resp = det(x)
    want = detect_keypoints_scale_space(x, 32, "dog", mr_size=2.0)
    assert bits(lafs) == bits(want[0]) and bits(resp) == bits(want[1])
    r2, l2 = det.detect(x, 32)
    assert bits(l2) == bits(lafs) and bits(r2) == bits(resp)
    up = ScaleSpaceDetector(32, 2.0, resp_module=BlobDoG(), ori_module=LAFOrienter(), minima_are_also_good=True,
                            scale_space_response=True).to(cuda)(x)[0]
    assert up.shape == lafs.shape and bits(get_laf_center(up)) == bits(get_laf_center(lafs))
    # two views of one image, 6 pixels apart
    views = [x[:, :, :88, :120].contiguous(), x[:, :, 4:92, 6:126].contiguous()]
    kps, descs = [], []
    for v in views:
        lf, sc, cnt = detect_keypoints_scale_space(v, 32, "dog", mr_size=2.0)
        desc, _ = describe_keypoints(v, None, lafs=lf)
        assert desc.shape[:2] == (1, 32) and int(cnt[0]) >= 8
        kps.append(get_laf_center(lf).contiguous())
        descs.append(desc)
    match, _ = match_pairs(descs[0], descs[1], mode="mnn")
    inl, H, mask = verify_pairs(kps[0], kps[1], match, th=3.0, iters=256, seed=1)
    assert inl.shape == (1,) and H.shape == (1, 3, 3) and int(inl[0]) == int(mask.sum())
    print("pipeline: %d matches, %d inliers" % (int((match >= 0).sum()), int(inl[0])))
