"""Generate tests/golden/pyrpatch.npz (build container only, like make_golden_describe.py).

    python tests/golden/make_golden_pyrpatch.py

From the reference, unmodified and imported as a package: cirtorch/geometry/transform/pyramid.py
(pyrdown), cirtorch/features/laf.py (extract_patches_from_pyramid, extract_patches_simple,
normalize_laf, make_upright), orientation.py (PatchDominantGradientOrientation, LAFOrienter),
siftdesc.py (SIFTDescriptor) and enhance/color/gray.py, run on the inputs of tests/pyrpatch_cases.py.
No reference source is copied: the fixture holds seeds, checksums, results and tolerances.

Tolerances follow describe.npz: per case the reference's float64 run rounded to float32 and
tol = max |its float32 run - its float64 run|; the numpy restatement of pyrpatch_cases is asserted
within tol / 2 of the float64 run (tol for the one form describe_cases.FULL_TOL_FORM, for the reason
make_golden_describe.py gives), the GPU tests assert the kernels within tol.  Orientation angles are
compared for equality under that file's safe-argmax rule; a case's seed advances otherwise.

The reference leaves a zero patch for a frame whose level does not exist.  The engine samples the
last level there, so the expected values of every frame are composed from the reference's functions:
pyrdown repeated, normalize_laf against the image, and extract_patches_simple on the level with the
normalised frames (normalize_lafs_before_extraction=False) -- the statements of
extract_patches_from_pyramid's loop body.  For every frame whose level exists the composition is
asserted equal, bit for bit, to extract_patches_from_pyramid itself, and where no frame is past the
last level the composed orientation chain is asserted equal to LAFOrienter.
  down_<c>_<h>x<w>, down_tol_<..>   pyrdown of hash noise [2, c, h, w]
  p_<case>, ptol_<case>, lv_<case>  patches and unclamped levels of the stratified frames
  f_<form>_<case>, ftol_.., fa_..   the fused forms (describe_cases: l0 / l1 / s0 / s1)
  u8_d, u8_tol, u8_a                the uint8 three-channel case (s1 form on the reference's gray image)
  board_<h>x<w>                     the largest |pyramid patch - 0.5| and the smallest range of a simple
                                    patch of the checkerboard witness, from the reference's float64 run
Conditions asserted here: every frame's log2(2 s / PS) + 0.5 is at least 1e-3 from an integer (also
the upright and the turned frames of the fused forms, which must keep their level); every existing
level of a patch case holds at least 3 frames per image; every patch case holds at least 2 frames past
the last level.
"""

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))

import make_golden_describe as GD  # noqa: E402  (sets up the paths: the reference's cirtorch package)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import describe_cases as QC  # noqa: E402
import pyrpatch_cases as PC  # noqa: E402
from cirtorch.enhance.color.gray import rgb_to_grayscale  # noqa: E402
from cirtorch.features import laf as RL  # noqa: E402
from cirtorch.features import orientation as RO  # noqa: E402
from cirtorch.geometry.conversions import rad2deg  # noqa: E402
from cirtorch.geometry.transform import pyramid as RP  # noqa: E402
from cirtorch.geometry.transform.imgwarp import angle_to_rotation_matrix  # noqa: E402

assert os.path.abspath(RP.__file__).startswith(os.path.abspath(GD.REF)), RP.__file__


def ref_levels(img, ps):
    lev = [img]
    with torch.no_grad():
        while min(lev[-1].shape[2] // 2, lev[-1].shape[3] // 2) >= ps:
            lev.append(RP.pyrdown(lev[-1]))
    return lev


def check_margin(frames, ps, what):
    lv, t = PC.frame_levels(frames, ps)
    d = np.abs(t - np.rint(t))[np.isfinite(t)].min()
    assert d >= PC.MARGIN, (what, d)
    return lv


def ref_pyr_patches(img, laf, ps, lv):
    """composed pyramid patches [n, N, c, ps, ps] of torch img / laf in their dtype; lv: the levels
    (numpy, unclamped).  Asserted equal to extract_patches_from_pyramid where the level exists."""
    lev = ref_levels(img, ps)
    use = np.minimum(lv, len(lev) - 1)
    with torch.no_grad():
        nlaf = RL.normalize_laf(laf, img)
        out = torch.zeros(laf.shape[0], laf.shape[1], img.shape[1], ps, ps, dtype=img.dtype)
        for l, cur in enumerate(lev):
            p = RL.extract_patches_simple(cur, nlaf, ps, normalize_lafs_before_extraction=False)
            m = torch.from_numpy(use == l)
            out[m] = p[m]
        theirs = RL.extract_patches_from_pyramid(img, laf, ps)
    inside = torch.from_numpy(lv < len(lev))
    assert torch.equal(theirs[inside], out[inside]), "composition differs from extract_patches_from_pyramid"
    assert not theirs[~inside].any()
    return out


def ref_chain(x, frames, ps, orient, upright_first, dtype):
    """the reference's LAFOrienter -> pyramid patches -> SIFTDescriptor on x [n, 1, h, w] (numpy):
    (desc, angles or None, the patches whose orientation was estimated or None)"""
    img, laf = torch.from_numpy(x).to(dtype), torch.from_numpy(frames).to(dtype)
    n, N = laf.shape[:2]
    ang = opatch = None
    last = len(PC.level_sizes(x.shape[2], x.shape[3], ps)) - 1
    with torch.no_grad():
        if orient:
            up = RL.make_upright(laf) if upright_first else laf
            ulv = check_margin(up.float().numpy(), ps, "upright")
            opatch = ref_pyr_patches(img, up, ps, ulv).view(-1, 1, ps, ps)
            ang, _ = GD.ref_orientation(opatch)
            rot = angle_to_rotation_matrix(rad2deg(torch.from_numpy(ang).view(n, N))).view(n * N, 2, 2)
            laf = torch.cat([torch.bmm(RL.make_upright(up).view(n * N, 2, 3)[:, :2, :2], rot),
                             up.view(n * N, 2, 3)[:, :2, 2:]], dim=2).view(n, N, 2, 3)
            if ulv.max() <= last and not upright_first:
                assert torch.equal(RO.LAFOrienter(ps, QC.ORIENT_BINS)(up, img), laf), "composition differs from LAFOrienter"
            ang = ang.reshape(n, N)
            opatch = opatch.numpy()[:, 0]
        lv = check_margin(laf.float().numpy(), ps, "described")
        assert (lv == PC.frame_levels(frames, ps)[0]).all(), "a frame changes its level when it is turned"
        patches = ref_pyr_patches(img, laf, ps, lv).view(-1, 1, ps, ps)
    return GD.ref_sift(patches, 8, 4).reshape(n, N, -1), ang, opatch


def fused_entry(x, what, ps, orient, kpts=None, lafs=None, scale=None):
    frames = QC.scale_frames(kpts, scale) if lafs is None else lafs
    check_margin(frames, ps, what)
    d32, a32, _ = ref_chain(x, frames, ps, orient, lafs is not None, torch.float32)
    d64, a64, op = ref_chain(x, frames, ps, orient, lafs is not None, torch.float64)
    ang = np.zeros(frames.shape[:2], dtype=np.float32)
    if orient:
        ang, safe, gap = GD.orientation_ok(op.astype(np.float32))
        ang = ang.reshape(frames.shape[:2])
        if not (safe and GD.same_bin(a32, a64) and (ang == a64.astype(np.float32)).all()):
            return None, None, None, False
    mine, mang, _, _ = PC.describe_keypoints_pyramid(x, kpts, None, scale, lafs, orient, ps, 8, 4)
    assert (mang == ang).all(), what
    d, tol = GD.entry(d32, d64, mine, what, 1.0 if what.split()[0] == PC.FULL_TOL_FORM else 0.5)
    return d, tol, ang, True


def down_cases(out):
    for c in PC.DOWN_C:
        for h, w in PC.DOWN_SHAPES:
            x = QC.uniform(PC.SEED + 100 * c + h + w, PC.DOWN_N * c * h * w).reshape(PC.DOWN_N, c, h, w).astype(np.float32)
            with torch.no_grad():
                r32 = RP.pyrdown(torch.from_numpy(x)).numpy()
                r64 = RP.pyrdown(torch.from_numpy(x).double()).numpy()
            assert r64.shape == (PC.DOWN_N, c, h // 2, w // 2)
            key = "%d_%dx%d" % (c, h, w)
            out["down_" + key], out["down_tol_" + key] = GD.entry(r32, r64, PC.pyrdown(x), "pyrdown " + key)


def patch_cases(seed, out):
    chk = []
    for name, shape, ps in PC.PATCH_CASES:
        x = QC.smooth_images(shape, seed)
        lafs = PC.frames(shape, PC.NPTS, seed)
        lv = check_margin(lafs, ps, name)
        last = len(PC.level_sizes(shape[2], shape[3], ps)) - 1
        for l in range(last + 1):
            assert ((lv == l).sum(axis=1) >= 3).all(), (name, l)
        assert (lv > last).sum() >= 2, name
        r32 = ref_pyr_patches(torch.from_numpy(x), torch.from_numpy(lafs), ps, lv).numpy()
        r64 = ref_pyr_patches(torch.from_numpy(x).double(), torch.from_numpy(lafs).double(), ps, lv).numpy()
        mine, mlv = PC.extract_patches_pyramid(x, lafs, ps)
        assert (mlv == lv).all()
        out["p_" + name], out["ptol_" + name] = GD.entry(r32, r64, mine, "patches " + name)
        out["lv_" + name] = lv.astype(np.int32)
        chk.append(QC.checksum(x, lafs))
    out["patch_chk"] = np.concatenate(chk)
    return True


def fused_cases(seed, out):
    chk = []
    for name, shape, ps, scale, forms in PC.FUSED:
        x = PC.coarse_images(shape, seed)
        lafs = PC.frames(shape, PC.NPTS, seed)
        kpts = PC.fused_keypoints(shape, PC.NPTS, seed, scale)
        for form in forms:
            kw = dict(lafs=lafs) if form[0] == "l" else dict(kpts=kpts, scale=scale)
            d, t, a, safe = fused_entry(x, "%s %s" % (form, name), ps, form[1] == "1", **kw)
            if not safe:
                print("    seed %d refused: orientation of form %s of %s" % (seed, form, name))
                return False
            out["f_%s_%s" % (form, name)], out["ftol_%s_%s" % (form, name)], out["fa_%s_%s" % (form, name)] = d, t, a
        chk.append(QC.checksum(x, lafs, kpts))
    out["fused_chk"] = np.concatenate(chk)
    return True


def u8_case(seed, out):
    x8 = QC.to_u8(PC.coarse_images(PC.COLOR, seed))
    xf = x8.astype(np.float32) / np.float32(255.0)
    kpts = PC.fused_keypoints(PC.COLOR, PC.U8_NPTS, seed, PC.U8_SCALE)
    with torch.no_grad():
        g32 = rgb_to_grayscale(torch.from_numpy(xf)).numpy()
        g64 = rgb_to_grayscale(torch.from_numpy(xf).double()).numpy()
    frames = QC.scale_frames(kpts, PC.U8_SCALE)
    d32, a32, _ = ref_chain(g32, frames, PC.U8_PS, True, False, torch.float32)
    d64, a64, op = ref_chain(g64, frames, PC.U8_PS, True, False, torch.float64)   # keeps its gray image in float64
    ang, safe, gap = GD.orientation_ok(op.astype(np.float32))
    if not (safe and GD.same_bin(a32.reshape(-1), a64.reshape(-1)) and (ang == a64.reshape(-1).astype(np.float32)).all()):
        print("    seed %d refused: orientation of the uint8 case (gap %.3g)" % (seed, gap))
        return False
    mine, mang, _, lv = PC.describe_keypoints_pyramid(xf, kpts, None, PC.U8_SCALE, None, True, PC.U8_PS, 8, 4)
    assert (mang.reshape(-1) == ang).all() and (lv == 2).all()
    out["u8_d"], out["u8_tol"] = GD.entry(d32, d64, mine, "uint8 gray s1")
    out["u8_a"] = ang.reshape(1, -1)
    out["u8_chk"] = QC.checksum(x8, kpts)
    return True


def board_cases(out):
    for h, w in PC.BOARDS:
        x = PC.checkerboard(h, w)
        fr = QC.scale_frames(PC.board_keypoints(h, w), PC.BOARD_SCALE)
        lv = check_margin(fr, PC.BOARD_PS, "board")
        assert (lv == 1).all()
        img, laf = torch.from_numpy(x).double(), torch.from_numpy(fr).double()
        with torch.no_grad():
            pyr = RL.extract_patches_from_pyramid(img, laf, PC.BOARD_PS).numpy()
            simple = RL.extract_patches_simple(img, laf, PC.BOARD_PS).numpy()
        rng = (simple.max(axis=(-1, -2)) - simple.min(axis=(-1, -2))).min()
        out["board_%dx%d" % (h, w)] = np.array([np.abs(pyr - 0.5).max(), rng])
        print("  board %dx%d: pyramid patch within %.3g of 0.5, simple patch range >= %.3g" % (h, w, np.abs(pyr - 0.5).max(), rng))
        assert np.abs(pyr - 0.5).max() < 1e-9 and rng > 0.5
        mine = PC.extract_patches_pyramid(x, fr, PC.BOARD_PS)[0]
        assert np.abs(mine - 0.5).max() < 1e-9


def main():
    out = {}
    down_cases(out)
    board_cases(out)
    seeds = []
    for k, fn in enumerate((patch_cases, fused_cases, u8_case)):
        for attempt in range(50):
            seed = PC.SEED + 10 * k + 1000 * attempt
            part = {}
            if fn(seed, part):
                break
        else:
            raise AssertionError("no seed of case %d gives safe orientations" % k)
        out.update(part)
        seeds.append(seed)
    out["seeds"] = np.array(seeds, dtype=np.int64)
    path = os.path.join(HERE, "pyrpatch.npz")
    np.savez_compressed(path, **out)
    print("  pyrpatch.npz: %d arrays, %.0f KB" % (len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
