"""GPU checks of the patch pyramid (rr_pyrdown, rr_patch_pyramid, rr_extract_patches_pyramid,
rr_describe_keypoints_pyramid) against tests/golden/pyrpatch.npz and the numpy restatement of
tests/pyrpatch_cases.py.

Tolerances are the fixture's: per case the reference's own float32 error against its float64 run.
Orientation angles are compared for equality (the generator keeps only inputs whose argmax is safe)."""

import functools

import numpy as np
import pytest
import torch

import describe_cases as QC
import pyrpatch_cases as PC
from conftest import golden
from test_gpu_describe import bits, close, dev

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def G():
    return golden("pyrpatch.npz")


@functools.lru_cache(maxsize=None)
def fused_inputs(k):
    name, shape, ps, scale, forms = PC.FUSED[k]
    seed = int(G()["seeds"][1])
    return PC.coarse_images(shape, seed), PC.frames(shape, PC.NPTS, seed), PC.fused_keypoints(shape, PC.NPTS, seed, scale)


@pytest.mark.parametrize("c", PC.DOWN_C)
def test_pyrdown_vs_reference(cuda, c):
    """the reflect border at 3 x 3, odd and even sizes, one, one plus a pixel and several output tiles;
    every level of rr_patch_pyramid is rr_pyrdown of the level before, bit for bit"""
    from cirtorch import _ops
    from cirtorch.geometry.transform import PyrDown, pyrdown
    g = G()
    for h, w in PC.DOWN_SHAPES:
        x = QC.uniform(PC.SEED + 100 * c + h + w, PC.DOWN_N * c * h * w).reshape(PC.DOWN_N, c, h, w).astype(np.float32)
        key = "%d_%dx%d" % (c, h, w)
        got = pyrdown(dev(x, cuda))
        close(got, g["down_" + key], float(g["down_tol_" + key]), "pyrdown " + key)
        assert np.abs(got.cpu().numpy() - PC.pyrdown(x)).max() <= 6e-8      # float32 rounding of values < 1
        assert bits(PyrDown()(dev(x, cuda).double())) == bits(got)
    x = dev(QC.smooth_images((2, c, 97, 131), PC.SEED + 5), cuda)
    levels, _ = _ops.patch_pyramid(x, 16)
    assert [tuple(v.shape[2:]) for v in levels] == [(48, 65), (24, 32)]
    assert bits(levels[0]) == bits(pyrdown(x)) and bits(levels[1]) == bits(pyrdown(levels[0]))
    assert _ops.patch_pyramid(x, 64)[0] == []


@pytest.mark.parametrize("k", range(len(PC.PATCH_CASES)))
def test_patches_vs_reference(cuda, k):
    """every frame from its level, frames past the last level from the last (the composed golden);
    beyond="raise" raises; levels_out is the restatement's; level-0 frames have the bits of
    extract_patches_simple; a non-finite frame gives a zero patch of level 0"""
    from cirtorch import _ops
    from cirtorch.features import laf as L
    g = G()
    name, shape, ps = PC.PATCH_CASES[k]
    seed = int(g["seeds"][0])
    x, lafs = QC.smooth_images(shape, seed), PC.frames(shape, PC.NPTS, seed)
    xt, lt = dev(x, cuda), dev(lafs, cuda)
    p = L.extract_patches_from_pyramid(xt, lt, ps, beyond="clamp")
    close(p, g["p_" + name], float(g["ptol_" + name]), "pyramid patches " + name)
    last = len(PC.level_sizes(shape[2], shape[3], ps)) - 1
    with pytest.raises(NotImplementedError, match="level %d" % (last + 1)):
        L.extract_patches_from_pyramid(xt, lt, ps)
    p2, lv, flag = _ops.extract_patches_pyramid(xt, lt, ps, return_levels=True)
    assert bits(p2) == bits(p) and lv.dtype == torch.int32 and int(flag) == 1
    np.testing.assert_array_equal(lv.cpu().numpy(), g["lv_" + name])
    zero = lv.cpu() == 0
    assert bits(p[zero]) == bits(L.extract_patches_simple(xt, lt, ps)[zero])
    # frames of existing levels only: the flag stays clear and the default (beyond="raise") returns the same bits
    inside = torch.from_numpy(g["lv_" + name] <= last)
    keep = int(inside.sum(1).min())
    sub = torch.stack([lt[i][inside[i]][:keep] for i in range(shape[0])])
    q, _, f2 = _ops.extract_patches_pyramid(xt, sub, ps, return_levels=True)
    assert int(f2) == 0 and bits(L.extract_patches_from_pyramid(xt, sub, ps)) == bits(q)
    assert bits(q) == bits(torch.stack([p[i][inside[i]][:keep] for i in range(shape[0])]))
    bad = lafs.copy()
    bad[0, 20, 1, 0] = np.nan
    pb, lb, _ = _ops.extract_patches_pyramid(xt, dev(bad, cuda), ps, return_levels=True)
    assert not pb[0, 20].any() and int(lb[0, 20]) == 0 and bits(pb[0, :20]) == bits(p[0, :20])


def test_uint8_and_gray_levels(cuda):
    """level 1 from uint8 and from three channels reduced to gray: the bits of the float32 path fed
    x.float() / 255, and within float32 rounding of the restatement"""
    from cirtorch import _ops
    seed = int(G()["seeds"][2])
    x8 = QC.to_u8(PC.coarse_images(PC.COLOR, seed))
    xf = x8.astype(np.float32) / np.float32(255.0)
    lafs = dev(PC.frames(PC.COLOR, PC.NPTS, seed), cuda)
    for gray in (False, True):
        a, b = _ops.patch_pyramid(dev(x8, cuda), 16, gray)[0], _ops.patch_pyramid(dev(xf, cuda), 16, gray)[0]
        want = PC.pyramid(xf, 16, gray)[1:]
        assert len(a) == 2 and all(bits(u) == bits(v) for u, v in zip(a, b))
        for u, v in zip(a, want):
            assert tuple(u.shape) == v.shape and np.abs(u.cpu().numpy() - v).max() <= 6e-8
        pa = _ops.extract_patches_pyramid(dev(x8, cuda), lafs, 16, gray)
        assert bits(pa) == bits(_ops.extract_patches_pyramid(dev(xf, cuda), lafs, 16, gray))
        assert np.abs(pa.cpu().numpy() - PC.extract_patches_pyramid(xf, lafs.cpu().numpy(), 16, gray)[0]).max() <= 6e-8


@pytest.mark.parametrize("hw", PC.BOARDS)
def test_checkerboard_witness(cuda, hw):
    """frames of scale 13 at PS 16 on a one-pixel checkerboard: the pyramid patch is 0.5, the simple
    patch swings; describe_keypoints(pyramid=True) gives the descriptor of a constant patch"""
    from cirtorch import _ops
    from cirtorch.features import laf as L
    from cirtorch.search import describe_keypoints
    h, w = hw
    x = dev(PC.checkerboard(h, w), cuda)
    kp = PC.board_keypoints(h, w)
    fr = dev(QC.scale_frames(kp, PC.BOARD_SCALE), cuda)
    p = L.extract_patches_from_pyramid(x, fr, PC.BOARD_PS)
    assert float((p - 0.5).abs().max()) <= 1e-6
    s = L.extract_patches_simple(x, fr, PC.BOARD_PS)
    assert float((s.amax(dim=(-1, -2)) - s.amin(dim=(-1, -2))).min()) > 0.5
    const = _ops.sift_describe(torch.full((1, PC.BOARD_PS, PC.BOARD_PS), 0.5, device=cuda), 8, 4)
    for orient in (False, True):
        d, _ = describe_keypoints(x, dev(kp, cuda), scale=PC.BOARD_SCALE, orientation=orient, patch_size=PC.BOARD_PS, pyramid=True)
        assert all(bits(d[0, i]) == bits(const[0]) for i in range(PC.BOARD_NPTS))
    plain, _ = describe_keypoints(x, dev(kp, cuda), scale=PC.BOARD_SCALE, patch_size=PC.BOARD_PS)
    assert all(bits(plain[0, i]) != bits(const[0]) for i in range(PC.BOARD_NPTS))


def fused(cuda, k, form, **kw):
    from cirtorch import _ops
    name, shape, ps, scale, forms = PC.FUSED[k]
    x, lafs, kpts = fused_inputs(k)
    src = dict(lafs=dev(lafs, cuda)) if form[0] == "l" else dict(kpts=dev(kpts, cuda), scale=scale)
    return _ops.describe_keypoints(dev(x, cuda), orient=form[1] == "1", orient_bins=QC.ORIENT_BINS, ps=ps, pyramid=True, **src, **kw)


@pytest.mark.parametrize("k", range(len(PC.FUSED)))
def test_fused_vs_reference(cuda, k):
    """rr_describe_keypoints_pyramid within tol of the reference's chain (LAFOrienter, pyramid patches,
    SIFTDescriptor) in float64, angles equal; the public function gives the same bits"""
    from cirtorch.search import describe_keypoints
    g = G()
    name, shape, ps, scale, forms = PC.FUSED[k]
    x, lafs, kpts = fused_inputs(k)
    for form in forms:
        d, a = fused(cuda, k, form)
        close(d, g["f_%s_%s" % (form, name)], float(g["ftol_%s_%s" % (form, name)]), "fused %s %s" % (form, name))
        assert bits(a) == g["fa_%s_%s" % (form, name)].tobytes(), (form, name)
        kw = dict(lafs=dev(lafs, cuda)) if form[0] == "l" else dict(scale=scale)
        pub = describe_keypoints(dev(x, cuda), dev(kpts, cuda), None, orientation=form[1] == "1", patch_size=ps, pyramid=True, **kw)
        assert bits(pub[0]) == bits(d) and bits(pub[1]) == bits(a)


def test_uint8_gray_fused(cuda):
    from cirtorch.search import describe_keypoints
    g = G()
    seed = int(g["seeds"][2])
    x8 = QC.to_u8(PC.coarse_images(PC.COLOR, seed))
    kpts = dev(PC.fused_keypoints(PC.COLOR, PC.U8_NPTS, seed, PC.U8_SCALE), cuda)
    u8, unit = dev(x8, cuda), dev(x8.astype(np.float32) / np.float32(255.0), cuda)
    d, a = describe_keypoints(u8, kpts, scale=PC.U8_SCALE, orientation=True, patch_size=PC.U8_PS, pyramid=True)
    close(d, g["u8_d"], float(g["u8_tol"]), "uint8 gray, level 2")
    assert bits(a) == g["u8_a"].tobytes()
    want = describe_keypoints(unit, kpts, scale=PC.U8_SCALE, orientation=True, patch_size=PC.U8_PS, pyramid=True)
    assert bits(d) == bits(want[0]) and bits(a) == bits(want[1])


@pytest.mark.parametrize("orient", (False, True))
def test_fused_equals_the_entries(cuda, orient):
    """the ABI's bit-identities: descriptors = rr_patch_pyramid -> rr_extract_patches_pyramid on
    lafs_out -> rr_sift_describe; angles = rr_patch_orientation on the pyramid patches of the upright
    frames; where every frame is of level 0 the bits of rr_describe_keypoints"""
    from cirtorch import _ops
    seed = int(G()["seeds"][2])
    x3 = QC.to_u8(PC.coarse_images(PC.COLOR, seed))
    k3 = PC.fused_keypoints(PC.COLOR, PC.U8_NPTS, seed, PC.U8_SCALE)
    x, lafs, kpts = fused_inputs(0)
    for img, kw, start, ps in ((x, dict(lafs=lafs), lafs, 16), (x, dict(lafs=lafs), lafs, 32), (x, dict(kpts=kpts, scale=40.0), QC.scale_frames(kpts, 40.0), 16),
                               (x3, dict(kpts=k3, scale=24.0), QC.scale_frames(k3, 24.0), 16)):
        it = dev(img, cuda)
        gray = img.shape[1] == 3
        args = {k: (dev(v, cuda) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        d, a, F = _ops.describe_keypoints(it, orient=orient, orient_bins=QC.ORIENT_BINS, ps=ps, return_lafs=True, pyramid=True, **args)
        pyr = _ops.patch_pyramid(it, ps, gray)[1]
        if orient:
            U = QC.make_upright(start) if "lafs" in kw else start
            pu = _ops.extract_patches_pyramid(it, dev(U, cuda), ps, gray, pyr=pyr)
            assert bits(_ops.patch_orientation(pu[:, :, 0], QC.ORIENT_BINS)) == bits(a)
        else:
            assert bits(F) == start.tobytes() and not a.any()
        p, lv, _ = _ops.extract_patches_pyramid(it, F, ps, gray, return_levels=True, pyr=pyr)
        assert bits(_ops.sift_describe(p[:, :, 0], 8, 4)) == bits(d), (ps, orient)
        assert int(lv.max()) >= 2
    # level 0 only: small frames, and an image too small for a level 1
    small = dev(QC.scale_frames(kpts, 5.0), cuda)
    for it, ps in ((dev(x, cuda), 16), (dev(x, cuda)[:, :, :40, :56].contiguous(), 32)):
        a0 = _ops.describe_keypoints(it, lafs=small, orient=orient, ps=ps, pyramid=True)
        b0 = _ops.describe_keypoints(it, lafs=small, orient=orient, ps=ps)
        assert bits(a0[0]) == bits(b0[0]) and bits(a0[1]) == bits(b0[1])


def test_dead_slots_batch_and_run_invariance(cuda):
    from cirtorch.search import describe_keypoints
    shape = (3,) + PC.MAIN[1:]
    x = dev(PC.coarse_images(shape, PC.SEED + 3), cuda)
    lafs = PC.frames(shape, 16, PC.SEED + 3)
    for orient in (False, True):
        kw = dict(lafs=dev(lafs, cuda), orientation=orient, patch_size=16, pyramid=True)
        full, again = describe_keypoints(x, None, **kw), describe_keypoints(x, None, **kw)
        assert bits(full[0]) == bits(again[0]) and bits(full[1]) == bits(again[1])
        for i in range(3):
            one = describe_keypoints(x[i:i + 1], None, **dict(kw, lafs=dev(lafs[i:i + 1], cuda)))
            assert bits(one[0][0]) == bits(full[0][i]) and bits(one[1][0]) == bits(full[1][i])
        lf = lafs.copy()
        lf[0, 3, :, 2] = lf[2, 0, :, 2] = -1.0
        count = torch.tensor([16, 5, 16], dtype=torch.int32, device=cuda)
        d, a = describe_keypoints(x, None, count, **dict(kw, lafs=dev(lf, cuda)))
        live = torch.ones(3, 16, dtype=torch.bool)
        live[0, 3] = live[2, 0] = False
        live[1, 5:] = False
        assert not d[~live].any() and not a[~live].any()
        assert bits(d[live]) == bits(full[0][live]) and bits(a[live]) == bits(full[1][live])
        assert describe_keypoints(x, None, **dict(kw, lafs=dev(lafs[:, :0], cuda)))[0].shape == (3, 0, 128)


def test_graph_capture_replay_equals_eager(cuda):
    from cirtorch.search import describe_keypoints
    from cirtorch.utils.graph import GraphedForward
    shape = (2, 3, 80, 96)
    xs = [dev(QC.to_u8(PC.coarse_images(shape, PC.SEED + 60 + i)), cuda) for i in range(2)]
    lafs = dev(PC.frames(shape, 16, PC.SEED + 60), cuda)
    count = torch.tensor([16, 9], dtype=torch.int32, device=cuda)

    def fn(t):
        return describe_keypoints(t, None, count, lafs=lafs, orientation=True, patch_size=16, pyramid=True)

    g = GraphedForward(fn, xs[0])
    for t in (xs[1], xs[0]):
        got = [o.clone() for o in g(t)]
        want = fn(t)
        assert all(bits(a) == bits(b) for a, b in zip(got, want))
        assert bool(want[0][1, :9].any()) and not want[0][1, 9:].any()


def test_refusals_on_the_device(cuda):
    from cirtorch.search import describe_keypoints
    from cirtorch.utils.parallel import PackedSequence
    x = dev(PC.coarse_images(PC.MAIN, PC.SEED), cuda)
    kp = dev(PC.fused_keypoints(PC.MAIN, 4, PC.SEED, 40.0), cuda)
    with pytest.raises(ValueError, match=r"\[B, 1, H, W\]"):
        describe_keypoints(PackedSequence([x[0], x[1]]), kp, pyramid=True)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        describe_keypoints(x, kp.cpu(), pyramid=True)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        describe_keypoints(x.cpu(), kp, pyramid=True)


def test_end_to_end_scale_space(cuda):
    """detect_keypoints_scale_space -> describe_keypoints(lafs=, pyramid=True, orientation=True) on
    1 x 1 x 160 x 192: finite RootSIFT descriptors (unit L1 norm before the root) for every detection,
    frames of level >= 1 among them; ScaleSpaceDetector(ori_module=LAFOrienter()) runs on the image"""
    from cirtorch.features.orientation import LAFOrienter
    from cirtorch.features.scale_space_detector import ScaleSpaceDetector
    from cirtorch.search import describe_keypoints, detect_keypoints_scale_space
    x = dev(PC.coarse_images(PC.E2E, PC.E2E_SEED), cuda)
    lafs, scores, count = detect_keypoints_scale_space(x, 64)
    n = int(count[0])
    assert n >= 8
    lv = PC.frame_levels(lafs[0, :n].cpu().numpy(), 32)[0]
    print("end to end: %d detections, levels %s" % (n, np.bincount(lv).tolist()))
    assert (lv >= 1).any()
    d, a = describe_keypoints(x, None, count, lafs=lafs, orientation=True, pyramid=True)
    assert bool(torch.isfinite(d).all()) and not d[0, n:].any()
    l1 = (d[0, :n].double() ** 2 - 1e-10).sum(-1)
    assert float((l1 - 1).abs().max()) <= 1e-5
    out = ScaleSpaceDetector(64, ori_module=LAFOrienter())(x)
    assert out[0].shape[-2:] == (2, 3) and bool(torch.isfinite(out[0]).all())
