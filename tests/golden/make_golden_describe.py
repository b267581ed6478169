"""Generate tests/golden/describe.npz (build container only, like make_golden_detect.py).

    python tests/golden/make_golden_describe.py

From the reference, unmodified and imported as a package: cirtorch/features/laf.py
(extract_patches_simple, make_upright), cirtorch/features/orientation.py
(PatchDominantGradientOrientation, LAFOrienter), cirtorch/features/siftdesc.py (SIFTDescriptor) and
cirtorch/enhance/color/gray.py (rgb_to_grayscale), run on the inputs of tests/describe_cases.py.  No
reference source is copied: the fixture holds seeds, checksums, results and tolerances.

Tolerances follow detect.npz.  Per case the fixture stores the reference's float64 run rounded to
float32 and tol = max |its float32 run - its float64 run|; the numpy restatement of
describe_cases is asserted to stay within tol / 2 of the float64 run, the GPU tests assert the
kernels within tol.  One form is the exception to tol / 2, describe_cases.FULL_TOL_FORM = "l1"
(given frames with orientation): rr_describe_keypoints rounds the upright frame and the turned frame
to float32 (it promises the bits of the chain through rr_extract_patches, whose frames are float32);
on frames of any shape both roundings move the samples by up to a float32 ulp of the frame, an error
of the same kind as the float32 run's own frames, which RootSIFT's square root near zero carries to
0.69 tol.  Its restatement is asserted within tol, which is also what the GPU tests ask of the
kernel.  Every other form, the oriented kpts + scale forms, the uint8 case and the rotation pair
included, is held to tol / 2.
  p<c>, ptol[c]      patches of the mixed frames at config c (describe_cases.CONFIGS)
  d<c>, dtol[c]      SIFT descriptors of p<c> (the float32 patches are the input of both runs)
  dv<j>, dvtol[j]    the (rootsift, clipval) variants on p0
  a<c>               orientation angles of p<c>, 36 bins
  pl<c>_d, pl<c>_a   descriptors and angles of the planted patches (flat, two ramps) at config c
  f_<form><c>, ftol_<form><c>, fa_<form><c>   the fused forms: l0 / l1 = the mixed frames without /
                     with orientation, s0 / s1 = kpts + scale without / with orientation
  u8_*               the uint8 three-channel case (s1 form on the reference's gray image)
  rot_cos, rot_tol   the rotation pair: the cosine, per keypoint, between the reference's float64
                     descriptors of an image and of its exact 90-degree turn (s1 form), and the
                     larger of the two descriptor tolerances
Orientation is an argmax: a case's seed advances until, for every patch whose orientation is
estimated, the two largest smoothed bins of the reference's float64 run differ by at least 1e-6 of
the larger and its float32 run picks the same bin.  Then angles are compared for equality.

The oriented chain is composed here from the reference's functions with extract_patches_simple in
the place of LAFOrienter's extract_patches_from_pyramid (the pyramid returns zeros for an image
smaller than the patch); where the pyramid applies (level 0, image at least the patch) LAFOrienter
itself is run and asserted equal.
"""

import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the reference tree
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("RR_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REF)   # the reference's cirtorch package, not this repository's

import numpy as np  # noqa: E402
import torch  # noqa: E402

import describe_cases as QC  # noqa: E402
from cirtorch.enhance.color.gray import rgb_to_grayscale  # noqa: E402
from cirtorch.features import laf as RL  # noqa: E402
from cirtorch.features import orientation as RO  # noqa: E402
from cirtorch.features import siftdesc as RS  # noqa: E402
from cirtorch.geometry.conversions import rad2deg  # noqa: E402
from cirtorch.geometry.transform.imgwarp import angle_to_rotation_matrix  # noqa: E402

for m in (RL, RO, RS):
    assert os.path.abspath(m.__file__).startswith(os.path.abspath(REF)), m.__file__

GAP = 1e-6


def ref_orientation(patches):
    """torch [B, 1, ps, ps] -> (angles, smoothed histogram [B, 36]) of the reference"""
    det = RO.PatchDominantGradientOrientation(patches.shape[-1], QC.ORIENT_BINS)
    seen = []
    hook = det.angular_smooth.register_forward_hook(lambda mod, inp, out: seen.append(out.detach()))
    with torch.no_grad():
        ang = det(patches)
    hook.remove()
    return ang.numpy(), seen[0].reshape(len(ang), -1).numpy()


def ref_sift(patches, nb, ns, rootsift=True, clipval=0.2):
    with torch.no_grad():
        return RS.SIFTDescriptor(patches.shape[-1], nb, ns, rootsift, clipval)(patches).numpy()


def orientation_ok(patches32):
    """(angles of the float64 run rounded to float32, whether the argmax is safe) for float32 patches [B, ps, ps]"""
    t = torch.from_numpy(patches32)[:, None]
    a64, h64 = ref_orientation(t.double())
    a32, h32 = ref_orientation(t)
    top = np.sort(h64, axis=1)[:, -2:]
    gap = ((top[:, 1] - top[:, 0]) / top[:, 1]).min()
    same = (np.argmax(h64, axis=1) == np.argmax(h32, axis=1)).all()
    mine = QC.patch_orientation(patches32)
    ok = bool(gap >= GAP and same)
    if ok:
        assert (mine == a64.astype(np.float32)).all(), "restatement angles differ"
    return a64.astype(np.float32), ok, float(gap)


def same_bin(a32, a64):
    """the float32 run's angles name the bins of the float64 run's (its own arithmetic may round the
    angle of a bin differently in the last place)"""
    return bool((np.abs(a32.astype(np.float64) - a64) < np.pi / (2 * QC.ORIENT_BINS)).all())


def entry(r32, r64, mine, what, share=0.5):
    """(float64 run rounded to float32, tol): the restatement must be within share * tol"""
    assert r32.dtype == np.float32 and r64.dtype == np.float64, what
    tol = float(np.abs(r32.astype(np.float64) - r64).max())
    err = float(np.abs(mine - r64).max())
    print("  %-22s restatement vs float64 %.3g, float32 vs float64 (tol) %.3g" % (what, err, tol))
    assert tol > 0 and err <= share * tol, (what, err, tol)
    return r64.astype(np.float32), np.float64(tol)


def ref_chain(x, frames, ps, nb, ns, orient, upright_first, dtype):
    """the reference's chain on image x [n, 1, h, w] and frames [n, N, 2, 3] (numpy float32) in dtype:
    (desc [n, N, dim], angles [n, N] or None, the patches whose orientation was estimated or None)"""
    img, laf = torch.from_numpy(x).to(dtype), torch.from_numpy(frames).to(dtype)
    n, N = laf.shape[:2]
    ang = opatch = None
    with torch.no_grad():
        if orient:
            up = RL.make_upright(laf) if upright_first else laf
            opatch = RL.extract_patches_simple(img, up, ps).view(-1, 1, ps, ps)
            ang, _ = ref_orientation(opatch)
            rot = angle_to_rotation_matrix(rad2deg(torch.from_numpy(ang).view(n, N))).view(n * N, 2, 2)
            laf = torch.cat([torch.bmm(RL.make_upright(up).view(n * N, 2, 3)[:, :2, :2], rot),
                             up.view(n * N, 2, 3)[:, :2, 2:]], dim=2).view(n, N, 2, 3)
            if min(img.shape[2:]) >= ps and not upright_first:   # the pyramid applies: LAFOrienter itself
                theirs = RO.LAFOrienter(ps, QC.ORIENT_BINS)(up, img)
                assert torch.equal(theirs, laf), "composition differs from LAFOrienter"
            ang = ang.reshape(n, N)
            opatch = opatch.numpy()[:, 0]
        patches = RL.extract_patches_simple(img, laf, ps).view(-1, 1, ps, ps)
    return ref_sift(patches, nb, ns).reshape(n, N, -1), ang, opatch


def fused_entry(x, what, ps, nb, ns, orient, kpts=None, lafs=None, scale=QC.SCALE):
    """(desc, tol, angles, safe): both runs of the chain and the restatement"""
    frames = QC.scale_frames(kpts, scale) if lafs is None else lafs
    d32, a32, _ = ref_chain(x, frames, ps, nb, ns, orient, lafs is not None, torch.float32)
    d64, a64, op = ref_chain(x, frames, ps, nb, ns, orient, lafs is not None, torch.float64)
    safe, ang = True, np.zeros(frames.shape[:2], dtype=np.float32)
    if orient:
        ang, safe, gap = orientation_ok(op.astype(np.float32))
        ang = ang.reshape(frames.shape[:2])
        safe = safe and same_bin(a32, a64) and (ang == a64.astype(np.float32)).all()
        if not safe:
            return None, None, None, False
    mine, mang, _ = QC.describe_keypoints(x, kpts, None, scale, lafs, orient, ps, nb, ns)
    assert (mang == ang).all(), what
    d, tol = entry(d32, d64, mine, what, 1.0 if what.split()[0] == QC.FULL_TOL_FORM else 0.5)
    return d, tol, ang, True


def main_case(seed, out):
    x = QC.smooth_images(QC.MAIN, seed)
    lafs = QC.frames(QC.MAIN, QC.NPTS, seed)
    kpts = QC.keypoints(QC.MAIN, QC.NPTS, seed, 8.0)
    n = QC.MAIN[0]
    ptol, dtol = [], []
    for c, (ps, nb, ns) in enumerate(QC.CONFIGS):
        with torch.no_grad():
            r32 = RL.extract_patches_simple(torch.from_numpy(x), torch.from_numpy(lafs), ps).numpy()
            r64 = RL.extract_patches_simple(torch.from_numpy(x).double(), torch.from_numpy(lafs).double(), ps).numpy()
        p, t = entry(r32, r64, QC.extract_patches(x, lafs, ps), "patches ps %d" % ps)
        out["p%d" % c] = p
        ptol.append(t)
        flat = p.reshape(-1, ps, ps)
        tp = torch.from_numpy(flat)[:, None]
        d, t = entry(ref_sift(tp, nb, ns), ref_sift(tp.double(), nb, ns), QC.sift_describe(flat, nb, ns), "sift %s" % ((ps, nb, ns),))
        out["d%d" % c] = d.reshape(n, QC.NPTS, -1)
        dtol.append(t)
        ang, safe, gap = orientation_ok(flat)
        if not safe:
            print("    seed %d refused: orientation gap %.3g at config %d" % (seed, gap, c))
            return False
        print("  orientation ps %d: smallest relative gap %.3g" % (ps, gap))
        out["a%d" % c] = ang.reshape(n, QC.NPTS)
        if c == 0:
            dv = []
            for j, (rootsift, clipval) in enumerate(QC.VARIANTS):
                d, t = entry(ref_sift(tp, nb, ns, rootsift, clipval), ref_sift(tp.double(), nb, ns, rootsift, clipval),
                             QC.sift_describe(flat, nb, ns, rootsift, clipval), "sift variant %s" % ((rootsift, clipval),))
                out["dv%d" % j] = d.reshape(n, QC.NPTS, -1)
                dv.append(t)
            out["dvtol"] = np.array(dv)
        forms = [("l0", False, None, lafs), ("l1", True, None, lafs), ("s0", False, kpts, None), ("s1", True, kpts, None)]
        for form, orient, kp, lf in forms if c == 0 else forms[3:]:
            d, t, a, safe = fused_entry(x, "%s config %d" % (form, c), ps, nb, ns, orient, kp, lf)
            if not safe:
                print("    seed %d refused: orientation of form %s at config %d" % (seed, form, c))
                return False
            out["f_%s%d" % (form, c)], out["ftol_%s%d" % (form, c)], out["fa_%s%d" % (form, c)] = d, t, a
        # planted patches: the restatement against the reference; no seed to advance
        pl = QC.planted_patches(ps)
        tpl = torch.from_numpy(pl)[:, None]
        out["pl%d_d" % c], out["pl%d_dtol" % c] = entry(ref_sift(tpl, nb, ns), ref_sift(tpl.double(), nb, ns),
                                                        QC.sift_describe(pl, nb, ns), "planted sift ps %d" % ps)
        a, safe, gap = orientation_ok(pl)
        assert safe, ("planted patches", ps, gap)
        out["pl%d_a" % c] = a
    out["ptol"], out["dtol"] = np.array(ptol), np.array(dtol)
    out["main_chk"] = QC.checksum(x, lafs, kpts)
    return True


def u8_case(seed, out):
    x8 = QC.to_u8(QC.smooth_images(QC.U8, seed))
    xf = x8.astype(np.float32) / np.float32(255.0)
    kpts = QC.keypoints(QC.U8, QC.U8_NPTS, seed, 7.0)
    ps, nb, ns = QC.CONFIGS[0]
    frames = QC.scale_frames(kpts, QC.SCALE)
    with torch.no_grad():
        g32 = rgb_to_grayscale(torch.from_numpy(xf)).numpy()
        g64 = rgb_to_grayscale(torch.from_numpy(xf).double()).numpy()
    d32, a32, _ = ref_chain(g32, frames, ps, nb, ns, True, False, torch.float32)
    # the float64 run keeps its gray image in float64
    img = torch.from_numpy(g64)
    laf = torch.from_numpy(frames).double()
    with torch.no_grad():
        op = RL.extract_patches_simple(img, laf, ps).view(-1, 1, ps, ps)
        a64, _ = ref_orientation(op)
        rot = angle_to_rotation_matrix(rad2deg(torch.from_numpy(a64).view(1, -1))).view(-1, 2, 2)
        laf2 = torch.cat([torch.bmm(RL.make_upright(laf).view(-1, 2, 3)[:, :2, :2], rot), laf.view(-1, 2, 3)[:, :2, 2:]],
                         dim=2).view(1, -1, 2, 3)
        d64 = ref_sift(RL.extract_patches_simple(img, laf2, ps).view(-1, 1, ps, ps).double(), nb, ns).reshape(1, QC.U8_NPTS, -1)
    ang, safe, gap = orientation_ok(op.numpy()[:, 0].astype(np.float32))
    if not (safe and same_bin(a32.reshape(-1), a64) and (ang == a64.astype(np.float32)).all()):
        print("    seed %d refused: orientation of the uint8 case (gap %.3g)" % (seed, gap))
        return False
    mine, mang, _ = QC.describe_keypoints(xf, kpts, None, QC.SCALE, None, True, ps, nb, ns)
    assert (mang.reshape(-1) == ang).all()
    out["u8_d"], out["u8_tol"] = entry(d32, d64, mine, "uint8 gray s1")
    out["u8_a"] = ang.reshape(1, -1)
    out["u8_chk"] = QC.checksum(x8, kpts)
    return True


def rot_case(seed, out):
    x = QC.smooth_images(QC.ROT, seed)
    kpts = QC.keypoints(QC.ROT, QC.ROT_NPTS, seed, 14.0)
    xr, kr = QC.rot90_pair(x, kpts)
    ps, nb, ns = QC.CONFIGS[0]
    res = []
    for what, img, kp in (("rot original", x, kpts), ("rot turned", xr, kr)):
        frames = QC.scale_frames(kp, QC.ROT_SCALE)
        d64, a64, _ = ref_chain(img, frames, ps, nb, ns, True, False, torch.float64)
        d, t, a, safe = fused_entry(img, what, ps, nb, ns, True, kp, None, QC.ROT_SCALE)
        if not safe:
            print("    seed %d refused: orientation of the rotation pair" % seed)
            return False
        res.append((d64[0], t, a))
    (da, ta, aa), (db, tb, ab) = res
    out["rot_cos"] = (da * db).sum(1) / (np.linalg.norm(da, axis=1) * np.linalg.norm(db, axis=1))
    out["rot_tol"] = np.float64(max(ta, tb))
    out["rot_a"], out["rot_ar"] = aa, ab
    out["rot_chk"] = QC.checksum(x, kpts)
    print("  rotation pair: reference cosines %.12f .. %.12f" % (out["rot_cos"].min(), out["rot_cos"].max()))
    return True


def main():
    out = {"configs": np.array(QC.CONFIGS, dtype=np.int64)}
    seeds = []
    for k, fn in enumerate((main_case, u8_case, rot_case)):
        for attempt in range(50):
            seed = QC.SEED + 10 * k + 1000 * attempt
            part = {}
            if fn(seed, part):
                break
        else:
            raise AssertionError("no seed of case %d gives safe orientations" % k)
        out.update(part)
        seeds.append(seed)
    out["seeds"] = np.array(seeds, dtype=np.int64)
    path = os.path.join(HERE, "describe.npz")
    np.savez_compressed(path, **out)
    print("  describe.npz: %d arrays, %.0f KB" % (len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
