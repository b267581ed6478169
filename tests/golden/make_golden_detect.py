"""Generate tests/golden/detect.npz (build container only, like make_golden_verify.py).

    python tests/golden/make_golden_detect.py

From the reference, unmodified and imported as a package: cirtorch/features/responses.py
(harris_response, gftt_response, hessian_response), cirtorch/enhance/color/gray.py
(rgb_to_grayscale) and cirtorch/features/nms.py (nms2d), run on the images of
tests/detect_cases.py.  No reference source is copied: the fixture holds seeds, checksums, score
maps, masks, keypoint lists and tolerances.

Responses.  Per case and kind: the reference's float64 run rounded to float32 (r<k>_<kind>) and
tol = max |its float32 run - its float64 run| (tol_<kind>[k]): the engine computes in float64 and
rounds once, so it must be at least as close to the float64 result as the reference's own float32
arithmetic is.  The same for the gray reduction of the three-channel case (g_<kind>, gtol_<kind>)
and for one case scaled by sigmas (sg_<kind>, sgtol_<kind>).  The numpy restatement of
detect_cases.response is asserted to stay within tol / 2 of the float64 run.

NMS and selection.  The score maps are the rounded Harris maps of detect_cases.SELECT_MAPS.  Stored:
the reference's nms2d masks for ks 3, 5, 9 (bit-packed, m<j>_ks<ks>) and the top-N lists
l<j>_n<N>_{kpts,scores,count} built from torch.topk(x * mask), N in detect_cases.NUMS, keeping the
positive entries.  A case's seed advances until no two of its first N + 1 candidates (all of them
for N above the candidate count) have equal scores, so torch.topk's unspecified tie order cannot
reach the fixture.  Masks and lists are asserted equal to the restatement's; the planted-tie map
of detect_cases.tie_map is checked against the restatement only (by the tests).
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

import detect_cases as DC  # noqa: E402
from cirtorch.enhance.color.gray import rgb_to_grayscale  # noqa: E402
from cirtorch.features import nms as RN  # noqa: E402
from cirtorch.features import responses as RR  # noqa: E402
from cirtorch.filters.kernels import get_gaussian_kernel1d  # noqa: E402

assert os.path.abspath(RR.__file__).startswith(os.path.abspath(REF)), RR.__file__
assert os.path.abspath(RN.__file__).startswith(os.path.abspath(REF)), RN.__file__


def ref_response(x, kind, sigmas=None):
    """x: torch [n, c, h, w] float32 or float64 -> numpy of the same dtype"""
    sg = None if sigmas is None else torch.tensor(sigmas, dtype=x.dtype)
    if kind == "harris":
        return RR.harris_response(x, DC.HARRIS_K, "sobel", sg).numpy()
    if kind == "gftt":
        return RR.gftt_response(x, "sobel", sg).numpy()
    return RR.hessian_response(x, "sobel", sg).numpy()


def response_entry(x, kind, to_gray=False, sigmas=None):
    """(float64 run rounded to float32, tol, restatement error)"""
    t = torch.from_numpy(x)
    if to_gray:
        r32, r64 = ref_response(rgb_to_grayscale(t), kind, sigmas), ref_response(rgb_to_grayscale(t.double()), kind, sigmas)
    else:
        r32, r64 = ref_response(t, kind, sigmas), ref_response(t.double(), kind, sigmas)
    assert r32.dtype == np.float32 and r64.dtype == np.float64
    tol = float(np.abs(r32.astype(np.float64) - r64).max())
    err = float(np.abs(DC.response(x, kind, DC.HARRIS_K, to_gray, sigmas) - r64).max())
    assert tol > 0 and err <= tol / 2, (kind, to_gray, sigmas, err, tol)
    return r64.astype(np.float32), tol, err


def ref_lists(score, ks, num):
    """score float32 [n, h, w] -> lists from torch.topk(x * mask), and whether the first
    num + 1 candidates of every image have distinct scores"""
    n, h, w = score.shape
    x = torch.from_numpy(score)[:, None]
    sup = RN.nms2d(x, (ks, ks)).view(n, -1)
    kk = min(num + 1, h * w)
    val, idx = torch.topk(sup, kk, dim=1)
    val, idx = val.numpy(), idx.numpy()
    kpts = np.full((n, num, 2), -1.0, dtype=np.float32)
    scores = np.zeros((n, num), dtype=np.float32)
    count = np.zeros(n, dtype=np.int32)
    distinct = True
    for b in range(n):
        pos = val[b] > 0
        assert not pos[np.argmin(pos):].any() or pos.all()   # the positive entries come first
        v = val[b][pos]
        distinct = distinct and len(np.unique(v)) == len(v)
        m = min(int(pos.sum()), num)
        count[b] = m
        kpts[b, :m, 0], kpts[b, :m, 1] = idx[b, :m] % w, idx[b, :m] // w
        scores[b, :m] = val[b, :m]
    return kpts, scores, count, distinct


def main():
    g1 = get_gaussian_kernel1d(7, 1.0)
    assert g1.dtype == torch.float32 and (g1.double().numpy() == DC.GAUSS7).all(), g1
    out = {"cases": np.array(DC.CASES, dtype=np.int64)}
    seeds, chk = [], []
    tols = {kind: [] for kind in DC.KINDS}
    select_of = {k: (j, to_gray) for j, (k, to_gray) in enumerate(DC.SELECT_MAPS)}
    for k, (n, c, h, w) in enumerate(DC.CASES):
        for attempt in range(50):
            seed = DC.SEED + 10 * k + 1000 * attempt
            x = DC.images(k, seed)
            entries = {kind: response_entry(x, kind) for kind in DC.KINDS}
            extra = {}
            if k == DC.GRAY_CASE:
                extra = {kind: response_entry(x, kind, to_gray=True) for kind in DC.KINDS}
            if k not in select_of:
                break
            j, to_gray = select_of[k]
            smap = (extra if to_gray else entries)["harris"][0][:, 0]
            lists = {num: ref_lists(smap, DC.SELECT_KS, num) for num in DC.NUMS}
            if all(v[3] for v in lists.values()):
                break
            print("    case %d seed %d refused: equal scores among the first candidates" % (k, seed))
        else:
            raise AssertionError("no seed of case %d gives distinct candidate scores" % k)
        seeds.append(seed)
        chk.append(DC.checksum(x)[0])
        for kind in DC.KINDS:
            out["r%d_%s" % (k, kind)] = entries[kind][0]
            tols[kind].append(entries[kind][1])
            print("  case %d %s %-7s: restatement vs float64 %.3g, float32 vs float64 (tol) %.3g" % (
                k, (n, c, h, w), kind, entries[kind][2], entries[kind][1]))
        if k == DC.GRAY_CASE:
            for kind in DC.KINDS:
                out["g_%s" % kind], out["gtol_%s" % kind] = extra[kind][0], np.float64(extra[kind][1])
                print("  case %d gray %-7s: restatement %.3g, tol %.3g" % (k, kind, extra[kind][2], extra[kind][1]))
        if k == DC.NOISE_CASE:
            for kind in DC.KINDS:
                e = response_entry(x, kind, sigmas=DC.SIGMAS[:n])
                out["sg_%s" % kind], out["sgtol_%s" % kind] = e[0], np.float64(e[1])
                print("  case %d sigmas %-7s: restatement %.3g, tol %.3g" % (k, kind, e[2], e[1]))
        if k in select_of:
            for ks in DC.NMS_SIZES:
                m = RN.nms2d(torch.from_numpy(smap)[:, None], (ks, ks), mask_only=True)[:, 0].numpy()
                assert m.dtype == bool and (m == DC.nms_mask(smap, ks)).all(), (k, ks)
                assert not (m[:, 0].any() or m[:, -1].any() or m[:, :, 0].any() or m[:, :, -1].any())   # 0 border maxima
                out["m%d_ks%d" % (j, ks)] = np.packbits(m.reshape(-1))
                print("  map %d ks %d: %s maxima per image" % (j, ks, m.reshape(len(m), -1).sum(1).tolist()))
            for num, (kp, sc, cnt, _) in lists.items():
                mine = DC.select(smap, DC.SELECT_KS, num)
                assert (mine[0] == kp).all() and (mine[1] == sc).all() and (mine[2] == cnt).all(), (k, num)
                out["l%d_n%d_kpts" % (j, num)], out["l%d_n%d_scores" % (j, num)], out["l%d_n%d_count" % (j, num)] = kp, sc, cnt
                print("  map %d top-%d: count %s" % (j, num, cnt.tolist()))
    out.update(seeds=np.array(seeds, dtype=np.int64), chk=np.array(chk))
    for kind in DC.KINDS:
        out["tol_%s" % kind] = np.array(tols[kind])
    path = os.path.join(HERE, "detect.npz")
    np.savez_compressed(path, **out)
    print("  detect.npz: %d arrays, %.0f KB" % (len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
