"""Generate tests/golden/affine.npz (build container only, like make_golden_pyrpatch.py).

    python tests/golden/make_golden_affine.py

From the reference, unmodified: cirtorch/features/affine_shape.py (PatchAffineShapeEstimator,
LAFAffineShapeEstimator), run on the inputs of tests/affine_cases.py.  That file imports its helpers
from `kornia`, which is not installed; stand-in modules kornia, kornia.filters, kornia.feature and
kornia.feature.laf are registered in sys.modules whose attributes are the reference's own objects:
get_gaussian_kernel2d (cirtorch/filters/kernels.py), SpatialGradient (cirtorch/filters/sobel.py),
ellipse_to_laf, get_laf_scale, raise_error_if_laf_is_not_valid, scale_laf, make_upright and
extract_patches_from_pyramid (cirtorch/features/laf.py).  No reference source is copied: the fixture
holds seeds, checksums, results and tolerances.

Tolerances follow describe.npz: per case the reference's float64 run rounded to float32 and
tol = max |its float32 run - its float64 run|; the numpy restatement of affine_cases is asserted
within tol / 2 of the float64 run, the GPU tests assert the kernels within tol.  Frames are stored as
the float64 run's frames rounded to float32 and compared, as tol is computed, after the 2 x 2 part is
divided by the input frame's scale (affine_cases.normalised); the centres of both runs are asserted
equal to the input's.

The reference leaves a zero patch, hence a circle, for a frame whose level does not exist; the engine
samples the last level there.  So the expected frames are composed from the reference's functions
-- make_upright, the composed pyramid patches of make_golden_pyrpatch.py, PatchAffineShapeEstimator,
ellipse_to_laf, get_laf_scale, scale_laf: the statements of LAFAffineShapeEstimator.forward -- and the
composition is asserted equal, bit for bit, to LAFAffineShapeEstimator wherever the level exists.
  ps_<ps>, pstol_<ps>        (a, b, c) of the seeded patches
  ell, ell_tol               ellipse_to_laf of the seeded ellipses
  f_<case>, ftol_<case>      frames of the fused cases; raw_<case> the raw moments of the float64 run
  dim, dim_tol               the image of case DIM times 1e-3
  blob_<k>, blobtol_<k>      the analytic blobs;  deg_<kind>, degtol_<kind>  constant, ramp, edge
Conditions asserted here (a case's seed advances otherwise, 50 attempts at the most): every raw moment
of the float64 run lies outside [eps / 2, 2 eps]; every upright frame's log2(2 s / PS) + 0.5 is at
least pyrpatch_cases.MARGIN from an integer; tol <= 1e-5; a fused case holds at least 3 frames of
every existing level and at least 2 past the last.
"""

import importlib
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))

import make_golden_pyrpatch as GP  # noqa: E402  (and through it make_golden_describe: the paths, the reference's package)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import affine_cases as AC  # noqa: E402
import describe_cases as QC  # noqa: E402
import pyrpatch_cases as PC  # noqa: E402
from cirtorch.enhance.color.gray import rgb_to_grayscale  # noqa: E402
from cirtorch.features import laf as RL  # noqa: E402
from cirtorch.filters.kernels import get_gaussian_kernel2d  # noqa: E402
from cirtorch.filters.sobel import SpatialGradient  # noqa: E402

GD = GP.GD


def reference_affine_shape():
    """the reference's affine_shape.py, unmodified, with stand-ins for the kornia modules it names"""
    names = ("kornia", "kornia.filters", "kornia.feature", "kornia.feature.laf")
    assert not any(n in sys.modules for n in names)
    mods = {n: types.ModuleType(n) for n in names}
    mods["kornia.filters"].get_gaussian_kernel2d = get_gaussian_kernel2d
    mods["kornia.filters"].SpatialGradient = SpatialGradient
    for f in ("ellipse_to_laf", "get_laf_scale", "raise_error_if_laf_is_not_valid", "scale_laf", "make_upright"):
        setattr(mods["kornia.feature.laf"], f, getattr(RL, f))
    mods["kornia.feature"].extract_patches_from_pyramid = RL.extract_patches_from_pyramid
    mods["kornia.feature"].laf = mods["kornia.feature.laf"]
    mods["kornia"].filters, mods["kornia"].feature = mods["kornia.filters"], mods["kornia.feature"]
    sys.modules.update(mods)
    try:
        m = importlib.import_module("cirtorch.features.affine_shape")
    finally:
        for n in names:
            del sys.modules[n]
    assert os.path.abspath(m.__file__).startswith(os.path.abspath(GD.REF)), m.__file__
    return m


RA = reference_affine_shape()


def outside_band(raw, what):
    inside = (raw >= AC.BAND[0]) & (raw <= AC.BAND[1])
    if inside.any():
        print("    %s: %d raw moments inside [eps / 2, 2 eps]" % (what, int(inside.sum())))
    return not inside.any()


def ref_raw(det, t):
    """the raw moments [B, 3] of the reference's estimator det on patches t [B, 1, ps, ps]: its own
    gradient module and window, the three means of its forward"""
    with torch.no_grad():
        g = det.gradient(t) * det.weighting.to(t.dtype)
        gx, gy = g[:, :, 0], g[:, :, 1]
        return torch.cat([gx.pow(2).mean(dim=2).mean(dim=2, keepdim=True), (gx * gy).mean(dim=2).mean(dim=2, keepdim=True),
                          gy.pow(2).mean(dim=2).mean(dim=2, keepdim=True)], dim=2)[:, 0].numpy()


def ref_shape(p, dtype):
    """reference (a, b, c) [B, 3] and raw moments [B, 3] of float32 patches [B, ps, ps] in dtype"""
    det = RA.PatchAffineShapeEstimator(p.shape[-1])
    t = torch.from_numpy(p)[:, None].to(dtype)
    with torch.no_grad():
        out = det(t)[:, 0].numpy()
    return out, ref_raw(det, t)


def patch_cases(seed, out):
    chk = []
    for ps in AC.PATCH_PS:
        p = AC.patches(ps, seed)
        r32, _ = ref_shape(p, torch.float32)
        r64, raw = ref_shape(p, torch.float64)
        if not outside_band(raw, "patches %d" % ps):
            return False
        assert np.abs(AC.raw_moments(p) - raw).max() <= 1e-6 * np.abs(raw).max()
        out["ps_%d" % ps], out["pstol_%d" % ps] = GD.entry(r32, r64, AC.patch_affine_shape(p), "shape ps %d" % ps)
        assert out["pstol_%d" % ps] <= AC.TOL_CAP
        deg = (raw < AC.EPS).sum(1) >= 2
        assert sorted(np.nonzero(deg)[0].tolist()) == sorted(AC.PATCH_FLAT), (ps, deg)
        assert (raw[:, 1] < 0).any() and (raw[:, 1] >= AC.EPS).any()
        chk.append(QC.checksum(p))
    out["patch_chk"] = np.concatenate(chk)
    return True


def ellipse_case(seed, out):
    e = AC.ellipses(seed)
    with torch.no_grad():
        r32 = RL.ellipse_to_laf(torch.from_numpy(e)).numpy()
        r64 = RL.ellipse_to_laf(torch.from_numpy(e).double()).numpy()
    out["ell"], out["ell_tol"] = GD.entry(r32, r64, AC.ellipse_to_laf(e), "ellipse_to_laf")
    out["ell_chk"] = QC.checksum(e)
    return True


def ref_frames(x, lafs, ps, dtype):
    """the statements of LAFAffineShapeEstimator.forward on image x [n, 1, h, w] and frames (numpy),
    with the composed pyramid patches: (frames [n, N, 2, 3], raw moments [n, N, 3]); asserted equal to
    the module where the level exists"""
    img, laf = torch.from_numpy(x).to(dtype), torch.from_numpy(lafs).to(dtype)
    n, N = laf.shape[:2]
    est = RA.LAFAffineShapeEstimator(ps)
    with torch.no_grad():
        up = RL.make_upright(laf)
        lv = GP.check_margin(up.float().numpy(), ps, "upright")
        patches = GP.ref_pyr_patches(img, up, ps, lv).view(-1, 1, ps, ps)
        shape = est.affine_shape_detector(patches)
        ells = torch.cat([laf.view(-1, 2, 3)[..., 2].unsqueeze(1), shape], dim=2).view(n, N, 5)
        scale_orig = RL.get_laf_scale(laf)
        e = RL.ellipse_to_laf(ells)
        res = RL.scale_laf(e, scale_orig / RL.get_laf_scale(e))
        theirs = est(laf, img)
    last = len(PC.level_sizes(x.shape[2], x.shape[3], ps)) - 1
    inside = torch.from_numpy(lv <= last)
    assert torch.equal(theirs[inside], res[inside]), "composition differs from LAFAffineShapeEstimator"
    assert torch.equal(res[..., 2], laf[..., 2]), "a centre moved"
    return res.numpy(), ref_raw(est.affine_shape_detector, patches).reshape(n, N, 3), lv


def frame_entry(x, lafs, ps, what, xin=None, x32=None):
    """(normalised float64 run rounded to float32, tol, raw moments, levels) or None when a condition fails;
    x: the gray image of the reference's float64 run (x32: of its float32 run), xin: what the
    restatement (and the engine) is given"""
    try:
        r32, _, _ = ref_frames(x.astype(np.float32) if x32 is None else x32, lafs, ps, torch.float32)
        r64, raw, lv = ref_frames(x, lafs, ps, torch.float64)
    except AssertionError as e:
        if "upright" in str(e):
            print("    %s: an upright frame within the margin of a level boundary" % what)
            return None
        raise
    mine, mraw, mlv = AC.laf_affine_shape(x.astype(np.float32) if xin is None else xin, lafs, None, ps)
    assert (mlv == lv).all() and (mine[..., 2] == lafs[..., 2]).all()
    if not (outside_band(raw, what) and outside_band(mraw, what + " (restatement)")):
        return None
    assert (((raw < AC.EPS).sum(-1) >= 2) == ((mraw < AC.EPS).sum(-1) >= 2)).all()
    _, tol = GD.entry(AC.normalised(r32, lafs).astype(np.float32), AC.normalised(r64, lafs), AC.normalised(mine, lafs), what)
    d = r64.astype(np.float32)      # stored as the engine returns frames: in pixels, normalised where they are compared
    f32 = np.abs(AC.normalised(mine.astype(np.float32), lafs) - AC.normalised(r64, lafs)).max()
    print("    %s: restatement rounded to float32 vs float64 %.3g; %d of %d frames degenerate; largest axis ratio %.2f"
          % (what, f32, int(((raw < AC.EPS).sum(-1) >= 2).sum()), raw.shape[0] * raw.shape[1],
             float((np.abs(r64[..., 0, 0]) / np.abs(r64[..., 1, 1])).max())))
    if tol > AC.TOL_CAP:
        print("    %s: tol %.3g above the cap" % (what, tol))
        return None
    return d, tol, raw, lv


def fused_case(k, seed, out):
    chk = []
    name, shape, ps, u8 = AC.FUSED[k]
    x, lafs = AC.fused_inputs(k, seed)
    xin, g32 = x, None
    if shape[1] == 3:   # the reference's own gray image, kept in float64 for its float64 run
        with torch.no_grad():
            g = rgb_to_grayscale(torch.from_numpy(x).double()).numpy()
            g32 = rgb_to_grayscale(torch.from_numpy(x)).numpy()
    else:
        g = x.astype(np.float64)
    got = frame_entry(g, lafs, ps, "fused " + name, xin, g32)
    if got is None:
        return False
    d, tol, raw, lv = got
    last = len(PC.level_sizes(shape[2], shape[3], ps)) - 1
    for l in range(last + 1):
        assert (lv == l).sum() >= 3, (name, l)
    assert (lv > last).sum() >= 2, name
    out["f_" + name], out["ftol_" + name], out["raw_" + name] = d, tol, raw
    chk.append(QC.checksum(xin, lafs))
    if name == AC.DIM[0]:
        xd = (x.astype(np.float64) * AC.DIM[1]).astype(np.float32)
        got = frame_entry(xd.astype(np.float64), lafs, ps, "dim " + name, xd)
        if got is None:
            return False
        assert ((got[2] < AC.EPS).sum(-1) >= 2).all() and not ((raw < AC.EPS).sum(-1) >= 2).all()
        out["dim"], out["dim_tol"] = got[0], got[1]
        chk.append(QC.checksum(xd))
    out["chk_" + name] = np.concatenate(chk)
    return True


def flat_cases(out):
    fr = AC.blob_frame()
    for k, (sx, sy) in enumerate(AC.BLOBS):
        got = frame_entry(AC.blob(sx, sy).astype(np.float64), fr, AC.FLAT_PS, "blob %g x %g" % (sx, sy))
        assert got is not None
        assert not ((got[2] < AC.EPS).sum(-1) >= 2).any(), "a blob falls under the threshold"
        out["blob_%d" % k], out["blobtol_%d" % k] = got[0], got[1]
    assert abs(out["blob_0"][0, 0, 0, 0] / AC.BLOB_SCALE - 1) < 1e-4 and out["blob_1"][0, 0, 0, 0] > out["blob_1"][0, 0, 1, 1]
    fr = AC.degenerate_frames()
    for kind in AC.DEGENERATE:
        got = frame_entry(AC.degenerate_image(kind).astype(np.float64), fr, AC.FLAT_PS, kind)
        assert got is not None and ((got[2] < AC.EPS).sum(-1) >= 2).all()
        assert set(got[3].ravel().tolist()) == {0, 1}
        out["deg_" + kind], out["degtol_" + kind] = got[0], got[1]


def main():
    out = {}
    flat_cases(out)
    seeds = []
    fused = [lambda seed, part, k=k: fused_case(k, seed, part) for k in range(len(AC.FUSED))]
    for k, fn in enumerate([patch_cases, ellipse_case] + fused):   # seeds: patches, ellipses, then one per fused case
        for attempt in range(50):
            seed = AC.SEED + 10 * k + 1000 * attempt
            part = {}
            if fn(seed, part):
                break
            print("    seed %d refused" % seed)
        else:
            raise AssertionError("no seed of case %d meets the conditions" % k)
        out.update(part)
        seeds.append(seed)
    out["seeds"] = np.array(seeds, dtype=np.int64)
    path = os.path.join(HERE, "affine.npz")
    np.savez_compressed(path, **out)
    print("  affine.npz: %d arrays, %.0f KB" % (len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
