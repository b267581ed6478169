"""CPU checks of the patch pyramid's host side: the pyrpatch.npz fixture (checksums, the conditions
its generator asserts, the numpy restatement of rr_pyrdown / rr_patch_pyramid /
rr_extract_patches_pyramid / rr_describe_keypoints_pyramid against the reference's results), the
argument checks and byte counts of the new entries (they return before anything is enqueued, so
they run without a GPU) and the Python surface's refusals."""

import ctypes
import os

import numpy as np
import pytest
import torch

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


def test_fixture_checksums_and_conditions():
    g = golden("pyrpatch.npz")
    seeds = [int(s) for s in g["seeds"]]
    chk = []
    for name, shape, ps in PC.PATCH_CASES:
        x, lafs = QC.smooth_images(shape, seeds[0]), PC.frames(shape, PC.NPTS, seeds[0])
        chk.append(QC.checksum(x, lafs))
        lv, t = PC.frame_levels(lafs, ps)
        assert np.abs(t - np.rint(t)).min() >= PC.MARGIN
        np.testing.assert_array_equal(lv, g["lv_" + name])
        last = len(PC.level_sizes(shape[2], shape[3], ps)) - 1
        assert last == {"m16": 2, "m32": 1, "c16": 2}[name]
        for l in range(last + 1):
            assert ((lv == l).sum(axis=1) >= 3).all(), (name, l)
        assert (lv > last).sum() >= 2, name
        s = np.sqrt(np.abs(lafs[..., 0, 0] * lafs[..., 1, 1] - lafs[..., 0, 1] * lafs[..., 1, 0]))
        assert s.min() >= 4 and s.max() <= 64
        assert float(g["ptol_" + name]) > 0
    np.testing.assert_allclose(np.concatenate(chk), g["patch_chk"], rtol=0, atol=1e-9)
    chk = []
    for name, shape, ps, scale, forms in PC.FUSED:
        chk.append(QC.checksum(PC.coarse_images(shape, seeds[1]), PC.frames(shape, PC.NPTS, seeds[1]),
                               PC.fused_keypoints(shape, PC.NPTS, seeds[1], scale)))
        assert QC.sift_geometry(ps, 4) is not None
    np.testing.assert_allclose(np.concatenate(chk), g["fused_chk"], rtol=0, atol=1e-9)
    x8 = QC.to_u8(PC.coarse_images(PC.COLOR, seeds[2]))
    np.testing.assert_allclose(QC.checksum(x8, PC.fused_keypoints(PC.COLOR, PC.U8_NPTS, seeds[2], PC.U8_SCALE)), g["u8_chk"],
                               rtol=0, atol=1e-9)
    assert PC.level_sizes(97, 131, 16) == [(97, 131), (48, 65), (24, 32)] and PC.level_sizes(97, 131, 32) == [(97, 131), (48, 65)]
    assert PC.level_sizes(80, 96, 16) == [(80, 96), (40, 48), (20, 24)] and PC.level_sizes(40, 56, 32) == [(40, 56)]


@pytest.mark.parametrize("c", PC.DOWN_C)
def test_restatement_pyrdown(c):
    g = golden("pyrpatch.npz")
    for h, w in PC.DOWN_SHAPES:
        x = QC.uniform(PC.SEED + 100 * c + h + w, PC.DOWN_N * c * h * w).reshape(PC.DOWN_N, c, h, w).astype(np.float32)
        key = "%d_%dx%d" % (c, h, w)
        within(PC.pyrdown(x), g["down_" + key], float(g["down_tol_" + key]), key)
    # the 6-tap form is the 5 x 5 binomial blur (reflect) followed by the mean of 2 x 2: on an odd and an even size
    for h, w in ((7, 6), (33, 47)):
        x = QC.uniform(11 + h, h * w).reshape(h, w)
        b = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
        p = np.pad(x, 2, mode="reflect")
        blur = sum(b[i] * b[j] * p[i:i + h, j:j + w] for i in range(5) for j in range(5))
        h2, w2 = h // 2, w // 2
        mean = 0.25 * (blur[0:2 * h2:2, 0:2 * w2:2] + blur[0:2 * h2:2, 1:2 * w2:2] + blur[1:2 * h2:2, 0:2 * w2:2] + blur[1:2 * h2:2, 1:2 * w2:2])
        np.testing.assert_allclose(PC.pyrdown(x), mean, rtol=0, atol=1e-15)


def test_restatement_patches_and_board():
    g = golden("pyrpatch.npz")
    seed = int(g["seeds"][0])
    for name, shape, ps in PC.PATCH_CASES:
        x, lafs = QC.smooth_images(shape, seed), PC.frames(shape, PC.NPTS, seed)
        p, lv = PC.extract_patches_pyramid(x, lafs, ps)
        within(p, g["p_" + name], float(g["ptol_" + name]), name)
        # level 0 is the simple extraction, bit for bit
        simple = QC.extract_patches(x, lafs, ps)
        assert (p[lv == 0] == simple[lv == 0]).all() and (lv == 0).any()
    for h, w in PC.BOARDS:
        x = PC.checkerboard(h, w)
        fr = QC.scale_frames(PC.board_keypoints(h, w), PC.BOARD_SCALE)
        p, lv = PC.extract_patches_pyramid(x, fr, PC.BOARD_PS)
        assert (lv == 1).all() and np.abs(p - 0.5).max() <= 1e-6
        s = QC.extract_patches(x, fr, PC.BOARD_PS)
        assert (s.max(axis=(-1, -2)) - s.min(axis=(-1, -2))).min() > 0.5
        assert g["board_%dx%d" % (h, w)][0] <= 1e-6 and g["board_%dx%d" % (h, w)][1] > 0.5


def test_restatement_fused_forms():
    g = golden("pyrpatch.npz")
    seed = int(g["seeds"][1])
    for name, shape, ps, scale, forms in PC.FUSED:
        x, lafs = PC.coarse_images(shape, seed), PC.frames(shape, PC.NPTS, seed)
        kpts = PC.fused_keypoints(shape, PC.NPTS, seed, scale)
        for form in forms:
            kw = dict(lafs=lafs) if form[0] == "l" else dict(kpts=kpts, scale=scale)
            d, a, _, _ = PC.describe_keypoints_pyramid(x, orient=form[1] == "1", ps=ps, **kw)
            within(d, g["f_%s_%s" % (form, name)], float(g["ftol_%s_%s" % (form, name)]), form + name,
                   1.0 if form == PC.FULL_TOL_FORM else 0.5)
            np.testing.assert_array_equal(a, g["fa_%s_%s" % (form, name)])
    seed = int(g["seeds"][2])
    x8 = QC.to_u8(PC.coarse_images(PC.COLOR, seed))
    kpts = PC.fused_keypoints(PC.COLOR, PC.U8_NPTS, seed, PC.U8_SCALE)
    d, a, _, lv = PC.describe_keypoints_pyramid(x8.astype(np.float32) / np.float32(255.0), kpts, scale=PC.U8_SCALE, orient=True, ps=PC.U8_PS)
    within(d, g["u8_d"], float(g["u8_tol"]), "uint8")
    np.testing.assert_array_equal(a, g["u8_a"])
    assert (lv == 2).all()


def test_byte_counts_and_last_level():
    E, lib = _lib()
    last = ctypes.c_int(-1)

    def nbytes(n, c, h, w, ps):
        b = lib.rr_patch_pyramid_bytes(n, c, h, w, ps, ctypes.byref(last))
        return b, last.value

    for (h, w, ps), want in (((97, 131, 16), 2), ((97, 131, 32), 1), ((80, 96, 16), 2), ((40, 56, 32), 0), ((160, 192, 32), 2),
                             ((768, 1024, 32), 4), ((64, 64, 32), 1), ((63, 64, 32), 0), ((3, 3, 8), 0)):
        for n, c in ((1, 1), (2, 3)):
            assert nbytes(n, c, h, w, ps) == (PC.pyramid_bytes(n, c, h, w, ps), want), (h, w, ps)
            assert len(PC.level_sizes(h, w, ps)) - 1 == want
    assert lib.rr_patch_pyramid_bytes(2, 1, 97, 131, 16, None) == 4 * 2 * (48 * 65 + 24 * 32)
    # monotonic: non-decreasing in n, c, h, w, non-increasing in ps
    base = (2, 2, 100, 120, 16)
    for i in range(4):
        prev = 0
        for v in range(1, 3 * base[i]):
            a = list(base)
            a[i] = v
            b = nbytes(*a)[0]
            assert b >= prev, (i, v)
            prev = b
    sizes = [nbytes(2, 2, 100, 120, ps)[0] for ps in range(8, 65)]
    assert all(a >= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > sizes[-1]
    # out of range: 0 bytes, last level 0
    for a in ((0, 1, 64, 64, 16), (1, 0, 64, 64, 16), (1, 1, 0, 64, 16), (1, 1, 64, 64, 7), (1, 1, 64, 64, 65), (1 << 10, 1, 1 << 11, (1 << 10) + 1, 16)):
        assert nbytes(*a) == (0, 0), a
    need = lib.rr_describe_pyramid_workspace_bytes(2, 3, 97, 131, 24, 16, 8, 4)
    assert need >= lib.rr_describe_workspace_bytes(2, 24, 16, 8, 4) + PC.pyramid_bytes(2, 1, 97, 131, 16)
    assert lib.rr_describe_pyramid_workspace_bytes(2, 1, 40, 56, 24, 32, 8, 4) == lib.rr_describe_workspace_bytes(2, 24, 32, 8, 4)
    assert lib.rr_describe_pyramid_workspace_bytes(3, 1, 97, 131, 24, 16, 8, 4) > need


def test_pyramid_argument_checks():
    """every refusal happens on the host: made-up device addresses, nothing is launched"""
    E, lib = _lib()
    p, null = ctypes.c_void_p(0x1000), ctypes.c_void_p(0)
    pb = lib.rr_patch_pyramid_bytes(2, 1, 64, 64, 16, None)
    need = lib.rr_describe_pyramid_workspace_bytes(2, 1, 64, 64, 24, 16, 8, 4)
    assert pb == 4 * 2 * (32 * 32 + 16 * 16) and need >= 256 + pb

    def down(x=p, n=2, c=1, h=16, w=16, out=p):
        return lib.rr_pyrdown(x, n, c, h, w, out, null)

    def pyr(x=p, n=2, c=1, h=64, w=64, gray=0, ps=16, buf=p, nbytes=pb):
        return lib.rr_patch_pyramid(x, n, c, h, w, 0, gray, ps, buf, nbytes, null)

    def ext(x=p, n=2, c=1, h=64, w=64, gray=0, buf=p, lafs=p, npts=24, ps=16, out=p):
        return lib.rr_extract_patches_pyramid(x, n, c, h, w, 0, gray, buf, lafs, npts, ps, out, null, null, null)

    def desc(x=p, n=2, c=1, h=64, w=64, kp=p, cnt=null, npts=24, scale=20.0, lafs=null, orient=1, obins=36, ps=16, nb=8, ns=4,
             clipval=0.2, out=p, ws=p, wsb=need):
        return lib.rr_describe_keypoints_pyramid(x, n, c, h, w, 0, kp, cnt, npts, scale, lafs, orient, obins, ps, nb, ns, 1,
                                                 clipval, out, null, null, ws, wsb, null)

    bad = [(down, dict(x=null)), (down, dict(out=null)), (down, dict(h=2)), (down, dict(w=2)), (down, dict(c=0)), (down, dict(n=-1)),
           (down, dict(n=1 << 10, h=1 << 10, w=(1 << 11) + 1)), (down, dict(n=1 << 24, h=3, w=3)),
           (pyr, dict(x=null)), (pyr, dict(buf=null)), (pyr, dict(ps=7)), (pyr, dict(ps=65)), (pyr, dict(gray=1)), (pyr, dict(gray=2, c=3)),
           (pyr, dict(h=0)), (pyr, dict(c=0)), (pyr, dict(n=-1)), (pyr, dict(nbytes=pb - 1)),
           (ext, dict(x=null)), (ext, dict(lafs=null)), (ext, dict(out=null)), (ext, dict(buf=null)), (ext, dict(ps=7)), (ext, dict(ps=65)),
           (ext, dict(gray=1)), (ext, dict(npts=-1)), (ext, dict(w=0)), (ext, dict(n=1 << 12, npts=1 << 12, h=8, w=8, ps=8)),
           (desc, dict(x=null)), (desc, dict(kp=null)), (desc, dict(out=null)), (desc, dict(c=2)), (desc, dict(orient=2)),
           (desc, dict(obins=65)), (desc, dict(scale=0.0)), (desc, dict(scale=float("inf"))), (desc, dict(ps=7)), (desc, dict(nb=17)),
           (desc, dict(ns=9)), (desc, dict(ps=12, ns=5)), (desc, dict(npts=-1)), (desc, dict(ws=null)), (desc, dict(wsb=need - 1)),
           (desc, dict(wsb=256)), (desc, dict(n=1 << 12, npts=1 << 12, h=4, w=4))]
    for fn, kw in bad:
        assert fn(**kw) != 0, (fn.__name__, kw)
    assert desc(wsb=need - 1) == -3 and "workspace" in lib.rr_last_error().decode()     # RR_ENOSPACE
    assert pyr(nbytes=pb - 1) == -3 and "too small" in lib.rr_last_error().decode()
    assert down(h=2) == -1 and "at least 3" in lib.rr_last_error().decode()
    assert down(n=1 << 24, h=3, w=3) == -1 and "2^24" in lib.rr_last_error().decode()
    for fn, name in ((down, "rr_pyrdown"), (pyr, "rr_patch_pyramid"), (ext, "rr_extract_patches_pyramid"),
                     (desc, "rr_describe_keypoints_pyramid")):
        assert fn(x=null) != 0
        assert lib.rr_last_error().decode().startswith(name + ":"), name
    # empty inputs and images without a level 1 launch nothing
    assert down(x=null, n=0, out=null) == 0
    assert pyr(x=null, n=0, buf=null, nbytes=0) == 0 and pyr(h=20, w=40, buf=null, nbytes=0) == 0
    assert ext(x=null, n=0, lafs=null, out=null, buf=null) == 0 and ext(npts=0, lafs=null, out=null) == 0
    assert desc(x=null, n=0, kp=null, out=null) == 0 and desc(npts=0, kp=null, out=null) == 0


def test_python_refusals():
    from cirtorch.features import laf as L
    from cirtorch.geometry.transform import PyrDown, pyrdown
    from cirtorch.search import describe_keypoints
    with pytest.raises(NotImplementedError, match="border_type"):
        pyrdown(torch.zeros(1, 1, 8, 8), border_type="replicate")
    with pytest.raises(NotImplementedError, match="align_corners"):
        PyrDown(align_corners=True)
    with pytest.raises(TypeError, match="not a torch.Tensor"):
        pyrdown(np.zeros((1, 1, 8, 8)))
    with pytest.raises(ValueError, match="BxCxHxW"):
        pyrdown(torch.zeros(8, 8))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        pyrdown(torch.zeros(1, 1, 8, 8))
    img = torch.rand(2, 1, 97, 131)
    laf = L.laf_from_center_scale_ori(torch.full((2, 5, 2), 40.0), torch.full((2, 5, 1, 1), 6.0), torch.zeros(2, 5, 1))
    # levels 1 and 2 exist at PS 16: the frames are sampled, which needs the GPU
    for s in (1.0, 3.0, 6.0):
        for beyond in ("raise", "clamp"):
            with pytest.raises(RuntimeError, match="GPU tensors only"):
                L.extract_patches_from_pyramid(img, L.scale_laf(laf, s), 16, beyond=beyond)
    with pytest.raises(NotImplementedError, match="level 3"):
        L.extract_patches_from_pyramid(img, L.scale_laf(laf, 10.0), 16)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        L.extract_patches_from_pyramid(img, L.scale_laf(laf, 10.0), 16, beyond="clamp")
    with pytest.raises(ValueError, match="beyond"):
        L.extract_patches_from_pyramid(img, laf, 16, beyond="zero")
    kp = torch.full((2, 5, 2), 40.0)
    for call in (lambda: describe_keypoints(img, kp, scale=40.0, patch_size=16, pyramid=True),
                 lambda: describe_keypoints(img, None, lafs=laf, orientation=True, pyramid=True)):
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            call()
    from cirtorch.utils.parallel import PackedSequence
    with pytest.raises(ValueError, match=r"\[B, 1, H, W\]"):
        describe_keypoints(PackedSequence([torch.zeros(1, 8, 8)]), kp, pyramid=True)


def test_end_to_end_image_yields_large_frames():
    """the image of the GPU end-to-end test: the scale-space restatement detects frames of level >= 1 at PS 32"""
    import scalespace_cases as SC
    lafs, _, count = SC.detect(PC.coarse_images(PC.E2E, PC.E2E_SEED), "hessian", 64, 6.0)[:3]
    n = int(np.asarray(count).ravel()[0])
    lv = PC.frame_levels(np.asarray(lafs, dtype=np.float32)[0, :n], 32)[0]
    assert n >= 8 and (lv >= 1).sum() >= 2, (n, np.bincount(lv))
