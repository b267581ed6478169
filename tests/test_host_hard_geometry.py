"""The conditions the GPU tests of tests/test_gpu_hard_geometry.py rest on, checked on the CPU with the
float64 numpy oracles alone (tests/hard_geometry_cases.py):

  * the seven-point oracle reaches all 7 records within 1e-6 px on every one of the 800 seven-tuples,
    with either null-space routine and the same winner, and at least a quarter of them have three roots;
  * every four-tuple has the eight determinants of its gate a factor 4 clear of RR_VERIFY_DET_EPS, the
    oracle's 8 x 8 solve fits every accepted one within 1e-6 px and rejects the others;
  * numpy's SVD decomposition stays within the recorded figures the engine's bounds are 16 x of;
  * the triangulation oracle's |w| is 100 x clear of its 1e-8 threshold on every point."""

import numpy as np

import epipolar_cases as EC
import hard_geometry_cases as HG
import pose_cases as PC
import verify_cases as VC


def test_seven_point_oracle_reaches_every_tuple():
    tuples, replaced = HG.fund_tuples()
    assert len(tuples) == len(HG.KINDS) * HG.PER_KIND == 800
    worst = 0.0
    for p, t in enumerate(tuples):
        assert t["kind"] == HG.KINDS[p // HG.PER_KIND]
        for o in (t["svd"], t["gj"]):
            assert o["inliers"] == 7 and o["mask"].all() and o["root"] == t["gj"]["root"]
            worst = max(worst, EC.sampson(o["F"], t["rec"])[1].max())
        assert t["rec"].dtype == np.float64 and np.array_equal(t["rec"], t["rec"].astype(np.float32))
        # the tolerance of F: 100 x the spread of the float64 routes (fund_spread), floor 1e-12
        assert t["tol"] == max(100 * t["spread"], 1e-12) and t["spread"] >= EC.f_err(t["svd"]["F"], t["gj"]["F"]) - 1e-15
    assert np.finfo(np.longdouble).eps < 1e-18      # fund_spread's extended-precision cubic is extended
    three = sum(t["nroots"] == 3 for t in tuples)
    per_kind = {k: sum(t["nroots"] == 3 for t in tuples if t["kind"] == k) for k in HG.KINDS}
    print("seven-tuples: replaced %d, three roots %d %s, worst Sampson px %.3g, largest F tolerance %.3g"
          % (replaced, three, per_kind, worst, max(t["tol"] for t in tuples)))
    assert worst <= HG.TH_MIN
    assert 4 * three >= len(tuples)
    assert replaced <= len(tuples) // 20       # the oracle reaches nearly every first draw: reseeding is the exception


def test_scene_kinds_are_what_they_say():
    tuples, _ = HG.fund_tuples()
    for t in tuples:
        ang = np.degrees(np.arccos(np.clip((np.trace(t["R"]) - 1) / 2, -1, 1)))
        if t["kind"] == "forward":
            e = EC.K @ t["t"]
            e = e[:2] / e[2]            # the epipole in image 1 of a camera that moved along t: inside the frame
            assert abs(t["t"][0]) <= 0.1 and abs(t["t"][1]) <= 0.1 and 0.8 <= t["t"][2] <= 1.5
            assert 0 <= e[0] < HG.W and 0 <= e[1] < HG.H_IMG
        if t["kind"] == "narrow":
            assert np.linalg.norm(t["t"]) <= 0.015
        if t["kind"] != "wide":
            assert ang <= np.degrees(0.25 * 3)
    wide = [np.degrees(np.arccos(np.clip((np.trace(t["R"]) - 1) / 2, -1, 1))) for t in tuples if t["kind"] == "wide"]
    assert max(wide) > 40.0, max(wide)


def test_four_point_gate_band_and_oracle():
    tuples, replaced = HG.homog_tuples()
    assert len(tuples) == sum(HG.H_PER_KIND.values())
    worst, dets = 0.0, {True: [], False: []}
    for p, t in enumerate(tuples):
        d = HG.gate_dets(t["rec"])
        assert ((d <= VC.DET_EPS / HG.BAND) | (d >= VC.DET_EPS * HG.BAND)).all(), (p, d)
        q = t["rec"][None]
        rejected = bool(VC.degenerate(q[:, :, :2])[0] or VC.degenerate(q[:, :, 2:])[0])
        assert rejected == (not t["accept"]) == (d.min() <= VC.DET_EPS / HG.BAND)
        o = t["oracle"]
        if t["accept"]:
            ok, res = VC.residuals(o["H"], t["rec"])
            assert o["inliers"] == 4 and ok.all() and res.max() <= HG.TH_MIN / HG.ENGINE_FACTOR
            worst = max(worst, res.max())
        else:
            assert o["inliers"] == 0 and not o["H"].any()
        if t["kind"] == "collinear":
            dets[t["accept"]].append(d.min())
    print("four-tuples: replaced %d, worst transfer px of the oracle %.3g, near-collinear determinants accepted %.3g .. %.3g, "
          "rejected %.3g .. %.3g" % (replaced, worst, min(dets[True]), max(dets[True]), min(dets[False]), max(dets[False])))
    # both sides of the gate are there, close to it and far from it
    assert min(dets[True]) < 10 * VC.DET_EPS * HG.BAND and max(dets[False]) > VC.DET_EPS / HG.BAND / 10 and min(dets[False]) == 0.0
    assert len(dets[True]) == len(dets[False]) == 100
    # the near-collinear three on side 2, accepted: run at 1 px, where the oracle's solve reaches them
    gate, greplaced = HG.gate_tuples()
    assert len(gate) == HG.GATE_TUPLES
    gw = 0.0
    for t in gate:
        d = HG.gate_dets(t["rec"])
        assert HG.gate_clear(t["rec"]) and d.min() >= VC.DET_EPS * HG.BAND and d[4:].min() == d.min() and d[:4].min() > 1e4
        ok, res = VC.residuals(t["oracle"]["H"], t["rec"])
        assert t["oracle"]["inliers"] == 4 and ok.all() and res.max() <= HG.TH_GATE / HG.ENGINE_FACTOR
        gw = max(gw, res.max())
    print("gate tuples: replaced %d, determinants %.3g .. %.3g, worst transfer px of the oracle %.3g"
          % (greplaced, min(t["det"] for t in gate), max(t["det"] for t in gate), gw))
    assert min(t["det"] for t in gate) < 100 * VC.DET_EPS


def test_decomposition_oracle_within_recorded_figures():
    """ORACLE_WORST is what pose_cases.decompose reaches on essential_cases(); a figure at rounding level moves by
    a few ulp with the LAPACK build, so the oracle is held to 4 x the record, a quarter of the engine's factor"""
    cases = HG.essential_cases()
    assert sum(c["group"] == "exact" for c in cases) == len(HG.ANGLES) * HG.AXES_PER_ANGLE * len(HG.T_KINDS) * len(HG.SCALES)
    assert sum(c["group"] == "near" for c in cases) == len(HG.KINDS) * HG.NEAR_PER_KIND * len(HG.NEAR_FOCALS)
    for c in cases:
        sv = np.linalg.svd(c["E"], compute_uv=False)
        if c["group"] == "exact":
            assert abs(sv[0] - sv[1]) <= 1e-12 * sv[0] and sv[2] <= 1e-12 * sv[0]
        else:
            assert sv[1] < 0.999 * sv[0] and sv[2] <= 1e-9 * sv[0], (c["what"], sv)
    worst = HG.worst_errors(HG.oracle_decompositions())
    print("worst oracle errors", worst)
    for group, rec in HG.ORACLE_WORST.items():
        assert set(worst[group]) == set(rec)
        for q, v in rec.items():
            assert worst[group][q] <= 4 * v + 1e-300, (group, q, worst[group][q], v)
            assert HG.engine_bound(group, q) == max(16 * v, 1e-12)
    for E in HG.refused_essentials():
        assert PC.decompose(E) is None


def test_triangulation_oracle_w_clear_of_threshold():
    sets = HG.tri_sets()
    assert len(sets) == len(HG.TRI_FOCALS) * len(HG.TRI_RATIOS) * len(HG.TRI_SIZES)
    wmin, worst = np.inf, 0.0
    for s in sets:
        X, w = PC.triangulate(s["P1"], s["P2"], s["rec"])
        assert len(s["rec"]) in HG.TRI_SIZES and np.abs(w).min() >= HG.W_CLEAR == 100 * PC.W_EPS
        assert s["rec"].max() < HG.TRI_W and s["rec"].min() >= 0
        wmin = min(wmin, np.abs(w).min())
        # the oracle meets the residual condition the engine is held to
        res, smin, nrm = HG.tri_residuals(s, X)
        assert HG.tri_residual_ok(res, smin, nrm).all()
        worst = max(worst, (res / smin).max())
    print("triangulation: smallest |w| %.3g, worst |A h| / sigma_min of the oracle %.9g" % (wmin, worst))
    assert max(s["rec"].max() for s in sets) > 3900       # image coordinates up to 4000
