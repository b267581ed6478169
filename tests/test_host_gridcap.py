"""What tests/test_gpu_gridcap.py rests on, checked without a GPU: the layout of the batches past the
65535-pair cap (tests/gridcap_cases.py), the conditions under which the float64 oracle decides a pair (the
margin rule of the verifier fixtures on all 140 compared RANSAC pairs, the depth margins of the pose pairs,
the distance of every matching ratio from its threshold) and the workspace the big batches ask for."""

import numpy as np

import epipolar_cases as EC
import gridcap_cases as GC
import match_cases as MC
import verify_cases as VC

GIB = 1 << 30


def _lib():
    from cirtorch import _engine
    return _engine.lib()


def test_layout_of_the_big_batch():
    assert GC.CAP == 65535 and GC.TAIL == 70 and GC.K == 7 and GC.P == GC.CAP + GC.TAIL
    assert GC.CAP % GC.K == 1                      # a block's second pair is the next distinct pair, not the same one
    kind = GC.kinds()
    assert (kind[:GC.TAIL] != kind[GC.CAP:]).all() and set(kind) == set(range(GC.K))
    # every ordered transition (first pair, second pair) of neighbouring distinct pairs happens in some block
    assert {(int(a), int(b)) for a, b in zip(kind[:GC.TAIL], kind[GC.CAP:])} == {(k, (k + 1) % GC.K) for k in range(GC.K)}
    ks = GC.kinds(GC.SPECIAL)
    assert sorted(np.nonzero(ks == GC.K)[0]) == sorted(GC.SPECIAL) and len(set(GC.SPECIAL)) == 6
    a, b, a2, b2, c, d2 = GC.SPECIAL
    assert a < GC.TAIL and b < GC.TAIL and a2 == a + GC.CAP and b2 == b + GC.CAP and a2 < GC.P and b2 < GC.P
    assert c < GC.TAIL and ks[c + GC.CAP] < GC.K and GC.CAP <= d2 < GC.P and ks[d2 - GC.CAP] < GC.K
    cmp = GC.compared()
    assert len(cmp) == 140 and set(GC.SPECIAL) <= set(cmp.tolist())
    assert GC.DEC_N == GC.CAP * 256 + 1000 and GC.DEC_N < 2 ** 31 and GC.DEC_N % GC.DEC_DISTINCT != 0
    assert (GC.CAP * 256) % GC.DEC_DISTINCT != 0   # a thread's second matrix is another one than its first


def test_required_kinds_of_pairs_are_present():
    n1 = [a for a, _ in GC.MATCH_PAIRS]
    n2 = [b for _, b in GC.MATCH_PAIRS]
    assert 0 in n1 and 0 in n2 and min(x for x in n1 if x) < 16 < max(n1) and max(n1) > 32 and max(n1) == GC.MATCH_MAX >= 17
    assert max(n2) == GC.MATCH_MAX and len(set(GC.MATCH_PAIRS)) == GC.K and GC.D == 8
    for sizes, least in ((GC.H_SIZES, 4), (GC.F_SIZES, 8)):
        assert len(sizes) == GC.K and {least, 9, 50, 0} <= set(sizes) and least - 1 in sizes
        ordinary = [s for s in sizes if 8 <= s <= 40 and s != least]
        assert len(set(ordinary)) >= 2
    for model, specs in (("homography", GC.H_PAIRS), ("fundamental", GC.F_PAIRS)):
        least = GC.MINIMAL[model]
        pairs = GC.verify_eight(model)
        m = [GC.kept(match, len(kp2)) for _, kp2, match in pairs]
        assert m == [s[2] for s in specs] and len(pairs) == GC.K + 1
        assert len(pairs[0][0]) == 0                                   # an empty pair
        assert 0 < m[1] < least and m[2] == least and m[6] == 0        # below the minimal sample, exactly it, no kept match
        assert m[7] == VC.STAGE + 1                                    # the unstaged pair
        assert 8 <= len(pairs[4][0]) <= 40 and 8 <= len(pairs[5][0]) <= 40 and len(pairs[4][0]) != len(pairs[5][0])
        # ragged offsets that are multiples of nothing
        assert np.gcd.reduce([len(q[0]) for q in pairs[1:7]]) == 1
    names = [n for n, _, _ in GC.POSE_PAIRS]
    assert names[0] == "empty" and "zeroF" in names and "unused" in names and sum(o for _, _, o in GC.POSE_PAIRS) >= 2


def test_matching_ratios_clear_of_the_threshold():
    """the matchers compare float32 ratios with th; the float64 restatement decides alike where no ratio is
    within 1e-5 of it"""
    gap = np.inf
    for a, b in GC.match_seven():
        if len(a) == 0 or len(b) < 2:
            continue
        dm = MC.dist2(a, b)
        for m in (dm, dm.T):
            if m.shape[1] >= 2:
                d, _ = MC.top2(m)
                gap = min(gap, np.abs(np.sqrt(d[:, 0]) / np.sqrt(d[:, 1]) - GC.MATCH_TH).min())
    print("smallest |ratio - th|", gap)
    assert gap > 1e-5


def test_margins_of_the_compared_ransac_pairs():
    """the rule the compare helpers of test_gpu_verify.py / test_gpu_epipolar.py rest on: no residual of any
    hypothesis or refit of any of the 140 compared pairs lies within 1e-7 px of th; for the fundamental
    model the two null-space routines also agree on the winner, the count and the mask"""
    for model in ("homography", "fundamental"):
        orc = GC.verify_oracle(model)
        assert sorted(orc) == sorted(GC.compared().tolist()) and len(orc) == 140
        margins = []
        for p, o in orc.items():
            info = o["info"]
            margins.append(info["margin"])
            assert info["margin"] >= GC.MARGIN, (model, p, info["margin"])
            least = GC.MINIMAL[model]
            assert (info["inliers"] == 0) == (info["m"] < least), (model, p, info["inliers"], info["m"])
            if model == "fundamental":
                g = o["gj"]
                assert g["margin"] >= GC.MARGIN, (p, g["margin"])
                assert (info["t"], info["root"], info["inliers"]) == (g["t"], g["root"], g["inliers"]), p
                assert np.array_equal(info["mask"], g["mask"]), p
        kinds_seen = {o["kind"] for o in orc.values()}
        print(model, "smallest margin px", min(margins), "largest tolerance", max(o["tol"] for o in orc.values()),
              "inliers of the unstaged pair", [orc[p]["info"]["inliers"] for p in GC.SPECIAL])
        assert kinds_seen == set(range(GC.K + 1))


def test_pose_pairs_are_decided_by_a_margin():
    """front and front_mask are compared exactly: under each of the four candidates no depth of a used record lies
    within 1e-6 x the median depth of zero, no |w| within 1e-6 relative of 1e-8, the winner is unique, and
    the two float64 routes agree on it (the conditions of make_golden_pose.py)"""
    for c in GC.pose_seven():
        w, alt = c["want"], c["alt"]
        assert w["front"] == alt["front"] and np.array_equal(w["front_mask"], alt["front_mask"]), c["name"]
        if c["name"] in ("empty", "zeroF", "unused"):
            assert w["front"] == 0 and not w["R"].any()
            continue
        assert w["depth"] >= 1e-6 * c["scale"] and w["wgap"] >= 1e-6, (c["name"], w["depth"], w["wgap"])
        counts = np.sort(w["counts"])
        assert counts[-1] > counts[-2] and w["front"] == len(w["rows"]), (c["name"], w["counts"])
        print(c["name"], "front", w["front"], "tol", c["tol"])


def test_tolerances_are_at_rounding_level():
    """the second solvers agree with the oracles to far better than anything a wrong kernel would reach"""
    for (p1, p2, w), n in zip(GC.dlt_seven(), GC.H_SIZES):
        assert len(p1) == n and (n < 4 or GC.dlt_tol(p1, p2, w) < 1e-3)
    for (p1, p2, w), n in zip(GC.fund_seven(), GC.F_SIZES):
        assert len(p1) == n and (n < 8 or GC.fund_tol(p1, p2, w) < 1e-6)
    for t in GC.tri_seven():
        assert GC.tri_tol(t) < 1e-6
    E = GC.essential_eleven()
    for i in range(8):
        assert GC.decompose_tol(E[i]) < 1e-6
    from pose_cases import decompose
    assert all(decompose(E[i]) is None for i in (8, 9, 10))


def test_workspaces_of_the_big_batches_stay_small():
    lib = _lib()
    for model, fn in (("homography", lib.rr_verify_workspace_bytes), ("fundamental", lib.rr_verify_epipolar_workspace_bytes)):
        lens = np.array([len(q[0]) for q in GC.verify_eight(model)])
        rows1 = int(lens[GC.kinds(GC.SPECIAL)].sum())
        need = int(fn(rows1, GC.P, GC.ITERS))
        print(model, "rows1", rows1, "workspace MiB", need / 2 ** 20)
        assert 0 < need < GIB
    n1 = np.array([a for a, _ in GC.MATCH_PAIRS])[GC.kinds()].sum()
    n2 = np.array([b for _, b in GC.MATCH_PAIRS])[GC.kinds()].sum()
    for lists in (0, 1):
        need = int(lib.rr_match_workspace_bytes(int(n1), int(n2), lists))
        print("match lists", lists, "rows", int(n1), int(n2), "workspace MiB", need / 2 ** 20)
        assert 0 < need < GIB
