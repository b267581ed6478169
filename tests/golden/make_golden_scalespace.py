"""Generate tests/golden/scalespace.npz (build container only, like make_golden_detect.py).

    python tests/golden/make_golden_scalespace.py

From the reference, unmodified and imported as a package: cirtorch/filters/gaussian.py
(gaussian_blur2d), cirtorch/geometry/transform/pyramid.py (ScalePyramid), cirtorch/features/responses.py
(BlobHessian, BlobDoG), cirtorch/features/nms.py (nms3d), cirtorch/geometry/subpix/spatial_soft_argmax.py
(ConvQuadInterp3d(10.0, eps=0.0)), cirtorch/features/scale_space_detector.py (_scale_index_to_scale) and
cirtorch/features/laf.py (laf_is_inside_image, normalize_laf, denormalize_laf), run on the images of
tests/scalespace_cases.py.  No reference source is copied: the fixture holds seeds, checksums, levels,
response volumes, masks, keypoint lists and tolerances.

The reference's detector does not run as written: ScalePyramid.forward reads self.init_sigma and the
detector self.scale_pyr.n_levels, which ScalePyramid.__init__ never sets, and conv_quad_interp3d calls
torch.solve, which torch has removed.  The two attributes are set on the instance and torch.solve is
supplied over torch.linalg.solve; nothing else is touched.

Pyramid.  Per case of PYRAMID_CASES and octave: the reference's float64 run rounded to float32 (p<k>_<o>)
and per level tol = max |its float32 run - its float64 run| (ptol<k>_<o>); the restatement is asserted
within tol / 2, the octave sizes and sigma lists equal.  The same for gaussian_blur2d alone (b<j>, btol).

Extrema.  The float32 Hessian volumes of list RESP_LIST (v_<o>), the reference's nms3d mask (bit-packed,
vm_<o>), at its voxels the offsets in the order (level, x, y) -- the reference's second and third
offsets swapped back -- and the refined values without the bonus from the float64 run (vo_<o>, vv_<o>),
and their float32-vs-float64 differences (votol, vvtol).

Lists.  The detector's flow -- pyramid, response, ConvQuadInterp3d on the response (and on its
negative with minima), frames, inside test, normalisation, the best N -- composed here from the
reference's own functions with the two deviations include/rr.h states: each offset goes to its own
axis, and only strict extrema (y_max > bonus / 2) are candidates, scored without the bonus.  Per list:
octave and voxel index, lafs, scores and count of the float64 run (l<j>_*) and the float32-vs-float64
differences (l<j>_ltol, l<j>_stol).  A case's seed advances until the float32 and float64 runs give the
same voxels in the same order, no two of the first N + 1 scores are equal, no |offset| is within 1e-3
of 0.7, no boundary point is within 1e-3 of its octave's border, N is at least each octave's extremum
count (the reference cuts every octave to N before the inside test; the blob image, whose smooth
ground has many weak extrema that the bonus makes equal in float32, is exempt and takes its N = 16
from all of them) and every image has at least 8 keypoints (the empty case: none).  With the offsets left swapped
and the bonus kept, the composition is asserted equal to the reference's own detect() on list 0.
"""

import math
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

torch.solve = lambda B, A: (torch.linalg.solve(A, B), None)   # removed from torch; conv_quad_interp3d calls it

import scalespace_cases as SC  # noqa: E402
from cirtorch.features import laf as RL  # noqa: E402
from cirtorch.features import responses as RR  # noqa: E402
from cirtorch.features import scale_space_detector as RD  # noqa: E402
from cirtorch.features.nms import nms3d  # noqa: E402
from cirtorch.filters.gaussian import gaussian_blur2d  # noqa: E402
from cirtorch.geometry.subpix.spatial_soft_argmax import ConvQuadInterp3d  # noqa: E402
from cirtorch.geometry.transform.pyramid import ScalePyramid  # noqa: E402

for mod in (RL, RR, RD):
    assert os.path.abspath(mod.__file__).startswith(os.path.abspath(REF)), mod.__file__


def ref_pyramid(x):
    sp = ScalePyramid(SC.LEVELS, SC.SIGMA, SC.MIN_SIZE)
    sp.init_sigma, sp.n_levels = sp.sigma, sp.levels
    return sp, sp(x)


def gray(x):
    """the engine's gray rule on a torch image (float32 products like the reference's rgb_to_grayscale
    would differ from it by rounding; the pyramid's input is the point here)"""
    if x.shape[1] == 1:
        return x
    return ((0.299 * x[:, 0] + 0.587 * x[:, 1]) + 0.114 * x[:, 2])[:, None]


def ref_flow(x, kind, num, mr, minima, fix=True):
    """x torch [n, 1, h, w] (float32 or float64) -> dict of the composed detector's outputs"""
    sp, (pyr, sigmas, _) = ref_pyramid(x)
    nms = ConvQuadInterp3d(SC.BONUS, eps=0.0)
    B = x.shape[0]
    per_image = [[] for _ in range(B)]
    vols, dense, n_ext = [], [], []
    margin, offmargin = 1e9, 1e9
    for oi, octave in enumerate(pyr):
        _, CH, L, H, W = octave.shape
        if kind == "dog":
            resp = RR.BlobDoG()(octave, sigmas[oi].view(-1))
        else:
            resp = RR.BlobHessian()(octave.permute(0, 2, 1, 3, 4).reshape(B * L, CH, H, W), sigmas[oi].view(-1))
            resp = resp.view(B, L, CH, H, W).permute(0, 2, 1, 3, 4)[:, :, :-1]
        vols.append(resp[:, 0])
        coords, ymax = nms(resp)
        if minima:
            cmin, ymin = nms(-resp)
            take = ymin > ymax
            ymax = torch.where(take, ymin, ymax)
            coords = torch.where(take.unsqueeze(2), cmin, coords)
        D = resp.shape[2]
        grid = torch.stack(torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij"))
        grid = torch.stack([grid[0], grid[2], grid[1]]).to(x.dtype)   # (d, x, y)
        off = coords[:, 0] - grid[None]                              # the reference's (ds, dy, dx)
        if fix:
            off = off[:, [0, 2, 1]]                                  # (ds, dx, dy): each on its own axis
        coords = grid[None] + off
        ext = ymax[:, 0] > SC.BONUS / 2
        dense.append((ext, off, ymax[:, 0] - SC.BONUS))
        n_ext.append(int(ext.reshape(B, -1).sum(1).max()))
        for b in range(B):
            idx = torch.nonzero(ext[b].reshape(-1))[:, 0]
            if len(idx) == 0:
                continue
            cb = coords[b].reshape(3, -1)[:, idx].t()[None]          # [1, N, 3] (d, x, y)
            sc = (ymax[b, 0].reshape(-1)[idx] - (SC.BONUS if fix else 0.0))[None]
            ob = off[b].reshape(3, -1)[:, idx].t()
            offmargin = min(offmargin, float((ob.abs() - 0.7).abs().min()))
            cs = RD._scale_index_to_scale(cb, sigmas[oi][b:b + 1], sp.n_levels)
            N = cs.shape[1]
            rot = torch.eye(2, dtype=x.dtype).view(1, 1, 2, 2)
            lafs = torch.cat([mr * cs[:, :, 0].view(1, N, 1, 1) * rot, cs[:, :, 1:3].view(1, N, 2, 1)], dim=3)
            pts = RL.laf_to_boundary_points(lafs, 12)[0]
            good = RL.laf_is_inside_image(lafs, octave[b:b + 1, 0])[0]
            m = torch.stack([pts[..., 0], W - pts[..., 0], pts[..., 1], H - pts[..., 1]]).abs().min()
            margin = min(margin, float(m))
            lafs = RL.normalize_laf(lafs, octave[b:b + 1, 0])
            for i in range(N):
                if bool(good[i]):
                    per_image[b].append((float(sc[0, i]), oi, int(idx[i]), lafs[0, i]))
    out = dict(vols=vols, dense=dense, n_ext=n_ext, margin=margin, offmargin=offmargin, per_image=per_image, img=x,
               pyr=pyr, sigmas=sigmas)
    return out


def lists_of(flow, num):
    """(octave [n, num], voxel [n, num], lafs [n, num, 2, 3], scores [n, num], count [n], distinct)"""
    B = len(flow["per_image"])
    octv = np.full((B, num), -1, dtype=np.int32)
    vox = np.full((B, num), -1, dtype=np.int64)
    lafs = np.zeros((B, num, 2, 3), dtype=np.float64)
    scores = np.zeros((B, num), dtype=np.float64)
    count = np.zeros(B, dtype=np.int32)
    distinct = True
    for b, cand in enumerate(flow["per_image"]):
        cand = sorted(cand, key=lambda e: (-e[0], e[1], e[2]))
        head = [e[0] for e in cand[:num + 1]]
        distinct = distinct and len(set(head)) == len(head)
        cand = cand[:num]
        count[b] = len(cand)
        if cand:
            L = RL.denormalize_laf(torch.stack([e[3] for e in cand])[None], flow["img"])[0]
            lafs[b, :len(cand)] = L.double().numpy()
        for i, e in enumerate(cand):
            octv[b, i], vox[b, i], scores[b, i] = e[1], e[2], e[0]
    return octv, vox, lafs, scores, count, distinct


def main():
    t = torch.linspace(0, 2 * math.pi, 11)
    assert (torch.sin(t).double().numpy() == SC.SIN11).all() and (torch.cos(t).double().numpy() == SC.COS11).all()
    out = {"cases": np.array(SC.CASES, dtype=np.int64)}
    seeds = {}

    def run_lists(k, seed):
        x = SC.images(k, seed)
        res = []
        for j, (kk, kind, mr, minima, num) in enumerate(SC.LISTS):
            if kk != k:
                continue
            g32 = gray(torch.from_numpy(x).double()).float() if x.shape[1] == 3 else torch.from_numpy(x)
            g64 = gray(torch.from_numpy(x).double())
            f32, f64 = ref_flow(g32, kind, num, mr, minima), ref_flow(g64, kind, num, mr, minima)
            l32, l64 = lists_of(f32, num), lists_of(f64, num)
            same = (l32[0] == l64[0]).all() and (l32[1] == l64[1]).all() and (l32[4] == l64[4]).all()
            enough = k == SC.EMPTY_CASE or l64[4].min() >= 8
            ok = (same and l32[5] and l64[5] and min(f32["offmargin"], f64["offmargin"]) > 1e-3
                  and min(f32["margin"], f64["margin"]) > 1e-3 and (k == SC.BLOB_CASE or max(f64["n_ext"]) <= num) and enough)
            if k == SC.EMPTY_CASE:
                ok = ok and l64[4].max() == 0
            if not ok:
                print("    case %d seed %d list %d refused: same %s distinct %s/%s offmargin %.2g margin %.2g ext %s count %s" % (
                    k, seed, j, same, l32[5], l64[5], f64["offmargin"], f64["margin"], f64["n_ext"], l64[4].tolist()))
                return None
            res.append((j, f32, f64, l32, l64))
        return x, res

    for k in range(len(SC.CASES)):
        for attempt in range(200):
            seed = SC.SEED + 10 * k + 1000 * attempt
            got = run_lists(k, seed)
            if got is not None:
                break
        else:
            raise AssertionError("no seed of case %d meets the conditions" % k)
        x, res = got
        seeds[k] = seed
        n, c, h, w = x.shape
        g64 = gray(torch.from_numpy(x).double())
        g32 = g64.float() if c == 3 else torch.from_numpy(x)

        # pyramid
        _, (p32, s32, _) = ref_pyramid(g32)
        _, (p64, s64, _) = ref_pyramid(g64)
        mine, octs = SC.pyramid(x)
        assert len(mine) == len(p64) and [(o["h"], o["w"]) for o in octs] == [tuple(p.shape[-2:]) for p in p64]
        for oi, o in enumerate(octs):
            assert (np.array(o["sigmas"], dtype=np.float32) == s32[oi][0].numpy()).all(), (k, oi)
            r64 = p64[oi][:, 0].numpy()
            tol = np.abs(p32[oi][:, 0].double().numpy() - r64).max(axis=(0, 2, 3))
            err = np.abs(mine[oi] - r64).max(axis=(0, 2, 3))
            print("  case %d octave %d %dx%d: restatement vs float64 %s, tol %s" % (
                k, oi, o["h"], o["w"], np.array2string(err, precision=2), np.array2string(tol, precision=2)))
            if not (c == 3 or (SC.SIGMA <= 0.5 and oi == 0)):
                assert (tol > 0).all()
            assert (err <= tol / 2).all(), (k, oi, err, tol)
            if k in SC.PYRAMID_CASES:
                out["p%d_%d" % (k, oi)], out["ptol%d_%d" % (k, oi)] = r64.astype(np.float32), tol
        if k == 1:
            btol = []
            for j, (ks, s) in enumerate(SC.BLUR_SIZES):
                b32 = gaussian_blur2d(g32, (ks, ks), (s, s)).double().numpy()
                b64 = gaussian_blur2d(g64, (ks, ks), (s, s)).numpy()
                tol = np.abs(b32 - b64).max()
                err = np.abs(SC.blur(x, ks, s) - b64).max()
                assert err <= tol / 2, (ks, err, tol)
                out["b%d" % j] = b64.astype(np.float32)
                btol.append(tol)
                print("  blur %d taps: restatement %.3g, tol %.3g" % (ks, err, tol))
            out["btol"] = np.array(btol)

        for j, f32, f64, l32, l64 in res:
            kk, kind, mr, minima, num = SC.LISTS[j]
            ltol = max(float(np.abs(l32[2] - l64[2]).max()), 1e-30)
            stol = max(float(np.abs(l32[3] - l64[3]).max()), 1e-30)
            mine = SC.detect(x, kind, num, mr, minima)
            for b in range(n):
                got = [(oi, idx) for oi, idx, _ in mine[3][b]]
                want = [(int(l64[0][b, i]), int(l64[1][b, i])) for i in range(l64[4][b])]
                assert got == want, (j, b, got[:5], want[:5])
            assert (mine[2] == l64[4]).all()
            lerr, serr = np.abs(mine[0] - l64[2]).max(), np.abs(mine[1] - l64[3]).max()
            print("  list %d (case %d, %s, mr %.1f, minima %d): count %s, extrema per octave %s; restatement lafs %.3g (tol %.3g) scores %.3g (tol %.3g)" % (
                j, k, kind, mr, minima, l64[4].tolist(), f64["n_ext"], lerr, ltol, serr, stol))
            assert lerr <= ltol and serr <= stol, (j, lerr, ltol, serr, stol)
            out["l%d_oct" % j], out["l%d_vox" % j] = l64[0], l64[1]
            out["l%d_lafs" % j], out["l%d_scores" % j], out["l%d_count" % j] = l64[2].astype(np.float32), l64[3].astype(np.float32), l64[4]
            out["l%d_ltol" % j], out["l%d_stol" % j] = np.float64(ltol), np.float64(stol)

            if j == SC.RESP_LIST:
                # the composition with the offsets left swapped and the bonus kept is the reference's detect()
                det = RD.ScaleSpaceDetector(num, mr, ScalePyramid(SC.LEVELS, SC.SIGMA, SC.MIN_SIZE), RR.BlobHessian(),
                                            ConvQuadInterp3d(SC.BONUS, eps=0.0))
                det.scale_pyr.init_sigma, det.scale_pyr.n_levels = SC.SIGMA, SC.LEVELS
                rresp, rlafs = det.detect(g64, num)
                raw = lists_of(ref_flow(g64, kind, num, mr, minima, fix=False), num)
                for b in range(n):
                    m = int(raw[4][b])
                    assert bool((rresp[b, :m] > SC.BONUS / 2).all()) and not bool((rresp[b, m:] > SC.BONUS / 2).any())
                    assert np.abs(rresp[b, :m].numpy() - raw[3][b, :m]).max() < 1e-12
                    assert np.abs(rlafs[b, :m].numpy() - raw[2][b, :m]).max() < 1e-9
                print("  list %d: the composition without the two deviations equals the reference's detect()" % j)
                # the dense extrema outputs on the float32 volumes the float32 run produced
                votol, vvtol = 0.0, 0.0
                for oi, v in enumerate(f32["vols"]):
                    v = v.numpy()
                    vt = torch.from_numpy(v)[:, None]
                    m = nms3d(vt, (3, 3, 3), True)[:, 0].numpy()
                    assert (m == (SC.extrema_mask(v) == 1)).all()
                    dn = {}
                    for dt in (torch.float32, torch.float64):
                        co, ym = ConvQuadInterp3d(SC.BONUS, eps=0.0)(vt.to(dt))
                        D, H, W = v.shape[1:]
                        grid = torch.stack(torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij"))
                        off = (co[:, 0] - torch.stack([grid[0], grid[2], grid[1]]).to(dt)[None])[:, [0, 2, 1]]
                        dn[dt] = (off.double().numpy(), (ym[:, 0] - SC.BONUS).double().numpy())
                    mo, _, mv = SC.extrema(v)
                    mb = np.broadcast_to(m[:, None], dn[torch.float64][0].shape)
                    ot = np.abs(dn[torch.float32][0] - dn[torch.float64][0])[mb].max()
                    vt_ = np.abs(dn[torch.float32][1] - dn[torch.float64][1])[m].max()
                    votol, vvtol = max(votol, ot), max(vvtol, vt_)
                    _, so, sv = SC.extrema(v)
                    assert np.abs(so.astype(np.float64) - dn[torch.float64][0])[mb].max() <= ot + 1e-7
                    assert np.abs(sv.astype(np.float64) - dn[torch.float64][1])[m].max() <= vt_ + 1e-9
                    out["v_%d" % oi], out["vm_%d" % oi] = v, np.packbits(m.reshape(-1))
                    out["vo_%d" % oi] = dn[torch.float64][0][mb].astype(np.float32)
                    out["vv_%d" % oi] = dn[torch.float64][1][m].astype(np.float32)
                    print("  volume %d: %d maxima, offsets tol %.3g, values tol %.3g" % (oi, m.sum(), ot, vt_))
                out["votol"], out["vvtol"] = np.float64(votol), np.float64(vvtol)

    out["seeds"] = np.array([seeds[k] for k in range(len(SC.CASES))], dtype=np.int64)
    out["chk"] = np.array([SC.images(k, seeds[k]).astype(np.float64).sum() for k in range(len(SC.CASES))])
    path = os.path.join(HERE, "scalespace.npz")
    np.savez_compressed(path, **out)
    print("  scalespace.npz: %d arrays, %.0f KB" % (len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
