"""Batched local-descriptor matching on the GPU (rr_match_top2 / rr_match_pairs,
cirtorch.search.match_pairs, cirtorch.features.matching) against the lists the
reference's cirtorch/features/matching.py produced (tests/golden/match.npz, float64
run) and a float64 numpy restatement (tests/match_cases.py).

Tolerances.  Indices are exact.  Distances and ratios: rtol 2e-6, the project's
pooled-operator tolerance (the engine's value is the float64 result rounded once to
float32, 6e-8).  Squared distances of the top-2 ABI: |a|^2, |b|^2 and a.b are chains
of D fused multiply-adds on partial sums of magnitude <= 1 (unit rows), each
rounding <= 2^-53, and d2 = |a|^2 + |b|^2 - 2 a.b <= 4 adds two more roundings, so
the engine's |error| <= (4 D + 8) 2^-53; the numpy difference form sums D rounded
squares into a partial sum <= 4, |error| <= 4 (D + 1) 2^-53: together (8 D + 12) 2^-53."""

import functools

import numpy as np
import pytest
import torch

import match_cases as MC
from conftest import golden

pytestmark = pytest.mark.gpu

RTOL = 2e-6
MODES = ("nn", "mnn", "snn", "smnn")


@functools.lru_cache(maxsize=None)
def case(k):
    g = golden("match.npz")
    n1, n2, d = MC.CASES[k]
    a, b = MC.descriptors(n1, n2, d, int(g["seeds"][k]))
    np.testing.assert_allclose(MC.checksum(a, b), g["chk"][k], rtol=0, atol=1e-9)
    return a, b


def expected(k, mode, th):
    g = golden("match.npz")
    fn = mode if mode in ("nn", "mnn") else "%s_%s" % (mode, MC.tag(th))
    return g["c%d_%s_i" % (k, fn)].astype(np.int64), g["c%d_%s_d" % (k, fn)]


def dev(x, cuda):
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


def check_fixed(match, dist, exp_match, exp_val, what=""):
    match, dist = match.cpu().numpy(), dist.cpu().numpy()
    assert match.dtype == np.int64 and dist.dtype == np.float32
    np.testing.assert_array_equal(match, exp_match, err_msg=what)
    keep = exp_match >= 0
    assert np.isinf(dist[~keep]).all() and (dist[~keep] > 0).all(), what
    err = np.abs(dist[keep] - exp_val[keep]) / np.abs(exp_val[keep]) if keep.any() else np.zeros(1)
    print(what, "max rel err", err.max())
    np.testing.assert_allclose(dist[keep], exp_val[keep], rtol=RTOL, atol=0, err_msg=what)


@pytest.mark.parametrize("k", range(len(MC.CASES)))
def test_matching_functions_vs_reference(cuda, k):
    """match_nn / match_mnn / match_snn / match_smnn == the reference's lists: indices and
    row order exactly, distances / ratios at rtol 2e-6."""
    from cirtorch.features import matching
    a, b = case(k)
    ta, tb = dev(a, cuda), dev(b, cuda)
    runs = [("nn", None, matching.match_nn(ta, tb)), ("mnn", None, matching.match_mnn(ta, tb))]
    for th in MC.THS:
        runs += [("snn", th, matching.match_snn(ta, tb, th)), ("smnn", th, matching.match_smnn(ta, tb, th=th))]
    for mode, th, (dists, idxs) in runs:
        ei, ed = expected(k, mode, th)
        assert dists.dtype == torch.float32 and idxs.dtype == torch.int64 and dists.is_cuda and idxs.is_cuda
        assert tuple(dists.shape) == (len(ei), 1) and tuple(idxs.shape) == (len(ei), 2), (mode, th)
        np.testing.assert_array_equal(idxs.cpu().numpy(), ei, err_msg="%s %s" % (mode, th))
        got = dists.cpu().numpy().reshape(-1)
        if len(ed):
            print(k, mode, th, "max rel err", (np.abs(got - ed) / ed).max())
        np.testing.assert_allclose(got, ed, rtol=RTOL, atol=0, err_msg="%s %s" % (mode, th))


@pytest.mark.parametrize("k", range(len(MC.CASES)))
def test_match_pairs_vs_reference(cuda, k):
    from cirtorch.search import match_pairs
    a, b = case(k)
    ta, tb = dev(a, cuda), dev(b, cuda)
    for mode in MODES:
        for th in (MC.THS if mode in ("snn", "smnn") else (0.8,)):
            ei, ed = expected(k, mode, th)
            match, dist = match_pairs(ta, tb, mode=mode, th=th)
            assert tuple(match.shape) == (a.shape[0],)
            check_fixed(match, dist, *MC.scatter(ei, ed, a.shape[0]), what="case %d %s %s" % (k, mode, th))


def test_mnn_equals_local_fixture(cuda):
    from cirtorch.search import match_pairs
    g = golden("local.npz")
    match, _ = match_pairs(dev(g["desc_b"][0], cuda), dev(g["nn_d2"], cuda), mode="mnn")
    np.testing.assert_array_equal(match.cpu().numpy(), g["nn_match"])
    assert (g["nn_match"] >= 0).sum() > 0


def test_ragged_batch_equals_per_pair_calls(cuda):
    """Every fixture case plus pairs with N1 = 0, N2 = 0 and N2 = 1 in ONE call (all zero-padded
    to D = 256, which adds exact zeros) == the per-pair calls at their own D, bit for bit:
    lists, matches and values; the N2 = 0 pair gives -1 / inf."""
    from cirtorch import _ops
    from cirtorch.search import match_pairs
    extra = [MC.descriptors(0, 5, 64, 11), MC.descriptors(4, 0, 64, 12), MC.descriptors(6, 1, 64, 13)]
    pairs = [case(k) for k in range(len(MC.CASES))]
    pairs = pairs[:3] + extra[:2] + pairs[3:] + extra[2:]
    pad = lambda x: np.pad(x, ((0, 0), (0, 256 - x.shape[1])))  # noqa: E731
    ta = dev(np.concatenate([pad(a) for a, _ in pairs]), cuda)
    tb = dev(np.concatenate([pad(b) for _, b in pairs]), cuda)
    o1 = np.cumsum([0] + [len(a) for a, _ in pairs])
    o2 = np.cumsum([0] + [len(b) for _, b in pairs])
    off1, off2 = dev(o1.astype(np.int64), cuda), dev(o2.astype(np.int64), cuda)
    lists = [t.cpu().numpy() for t in _ops.match_top2(ta, off1, tb, off2)]
    batch = {m: [t.cpu().numpy() for t in match_pairs(ta, tb, mode=m, th=0.8, offsets1=off1, offsets2=off2)]
             for m in MODES}
    bounded = [t.cpu().numpy() for t in match_pairs(ta, tb, mode="smnn", th=0.8, offsets1=off1, offsets2=off2,
                                                    max_n1=1000, max_n2=1025)]
    assert bounded[0].tobytes() == batch["smnn"][0].tobytes() and bounded[1].tobytes() == batch["smnn"][1].tobytes()
    for p, (a, b) in enumerate(pairs):
        s1, s2 = slice(o1[p], o1[p + 1]), slice(o2[p], o2[p + 1])
        if len(a) == 0:
            continue
        xa, xb = dev(a, cuda), dev(b, cuda)
        one = dev(np.array([0, len(a)], dtype=np.int64), cuda), dev(np.array([0, len(b)], dtype=np.int64), cuda)
        single = [t.cpu().numpy() for t in _ops.match_top2(xa, one[0], xb, one[1])]
        for got, ref, s in zip(lists, single, (s1, s1, s2, s2)):
            assert got[s].tobytes() == ref.tobytes(), "pair %d top-2 lists" % p
        for m in MODES:
            match, dist = [t.cpu().numpy() for t in match_pairs(xa, xb, mode=m, th=0.8)]
            assert batch[m][0][s1].tobytes() == match.tobytes(), "pair %d %s" % (p, m)
            assert batch[m][1][s1].tobytes() == dist.tobytes(), "pair %d %s" % (p, m)
        if len(b) == 0:
            for m in MODES:
                assert (batch[m][0][s1] == -1).all() and np.isposinf(batch[m][1][s1]).all()
            assert np.isposinf(lists[0][s1]).all() and (lists[1][s1] == -1).all()
        if len(b) == 1:
            assert (batch["nn"][0][s1] == 0).all() and (batch["snn"][0][s1] == -1).all()
            assert (batch["smnn"][0][s1] == -1).all() and (batch["mnn"][0][s1] >= 0).sum() == 1
            assert np.isfinite(lists[0][s1][:, 0]).all() and np.isposinf(lists[0][s1][:, 1]).all()
            assert (lists[1][s1] == np.array([0, -1])).all()


@pytest.mark.parametrize("swap", [False, True])
def test_duplicate_rows_resolve_to_lower_index(cuda, swap):
    """oracle.data.nn_descriptors plants a duplicate row on each side: exact ties, lower index."""
    from cirtorch.search import match_pairs
    from oracle import data, ops
    d1, d2 = data.nn_descriptors(300, 260, 128, 801)
    if swap:
        d1, d2 = d2, d1
    from cirtorch import _ops
    d1, d2 = d1.copy(), d2.copy()
    # one more: the nearest row of query 0 again in a higher row (exact tie of first and second)
    j0, last = int(MC.rules(d1, d2, 0.8)["nn"][0][0]), len(d2) - 3
    assert j0 < last
    d2[last] = d2[j0]
    exp = MC.rules(d1, d2, 0.8)
    dup = [j for j in range(len(d2) - 1) if (d2[j] == d2[j + 1]).all()]
    assert dup and (exp["nn"][0] == dup[0] + 1).sum() == 0 and (exp["nn"][0] == last).sum() == 0
    t1, t2 = dev(d1, cuda), dev(d2, cuda)
    off = lambda n: dev(np.array([0, n], dtype=np.int64), cuda)  # noqa: E731
    d12, i12, _, _ = [t.cpu().numpy() for t in _ops.match_top2(t1, off(len(d1)), t2, off(len(d2)))]
    assert d12[0, 0] == d12[0, 1] and tuple(i12[0]) == (j0, last)
    for mode in ("nn", "mnn"):
        match, dist = match_pairs(t1, t2, mode=mode)
        check_fixed(match, dist, *exp[mode], what="duplicates %s" % mode)
    np.testing.assert_array_equal(match_pairs(t1, t2, mode="mnn")[0].cpu().numpy(), ops.nn_matcher(d1, d2))


def test_non_unit_norm_descriptors(cuda):
    """sides scaled by 3 and 0.25: for unit rows the order depends on a.b only, so the nn / mnn
    indices are those of the fixture; values follow the float64 restatement of the scaled rows"""
    from cirtorch.search import match_pairs
    k = 2
    a, b = case(k)
    a3, b4 = (a * np.float32(3)).astype(np.float32), (b * np.float32(0.25)).astype(np.float32)
    exp = MC.rules(a3, b4, 0.8)
    for mode in ("nn", "mnn"):
        ei, ed = expected(k, mode, None)
        np.testing.assert_array_equal(exp[mode][0], MC.scatter(ei, ed, len(a))[0])
        match, dist = match_pairs(dev(a3, cuda), dev(b4, cuda), mode=mode)
        check_fixed(match, dist, *exp[mode], what="scaled %s" % mode)


@pytest.mark.parametrize("shape", [(50, 70, 36, 21), (40, 130, 512, 22), (33, 17, 4, 23)])
def test_padded_and_widest_d(cuda, shape):
    """D = 36 (zero-padded to 48 columns in LDS), D = 512 (four K-chunks), D = 4"""
    from cirtorch.search import match_pairs
    n1, n2, d, seed = shape
    a, b = MC.descriptors(n1, n2, d, seed)
    th = 0.8
    for m in (MC.dist2(a, b), MC.dist2(b, a)):
        s = np.sqrt(np.sort(m, axis=1)[:, :2])
        assert np.abs(s[:, 0] / s[:, 1] - th).min() > 1e-5   # the expectation is not at the threshold
    exp = MC.rules(a, b, th)
    for mode in MODES:
        match, dist = match_pairs(dev(a, cuda), dev(b, cuda), mode=mode, th=th)
        check_fixed(match, dist, *exp[mode], what="D=%d %s" % (d, mode))


def test_nan_row_matches_nothing(cuda):
    """a row holding a NaN (one on each side) has no match and is nobody's match; every other row
    is matched as if the NaN rows were not there"""
    from cirtorch.search import match_pairs
    a, b = case(2)
    a, b = a.copy(), b.copy()
    ia, jb = 5, 9
    a[ia, 17] = np.nan
    b[jb, :] = np.nan
    keep_a = np.arange(len(a)) != ia
    old_j = np.delete(np.arange(len(b)), jb)
    exp = MC.rules(a[keep_a], b[old_j], 0.8)
    for mode in MODES:
        match, dist = match_pairs(dev(a, cuda), dev(b, cuda), mode=mode, th=0.8)
        assert match[ia].item() == -1 and dist[ia].item() == float("inf")
        assert (match != jb).all().item()
        em, ev = exp[mode]
        em = np.where(em >= 0, old_j[np.maximum(em, 0)], -1)
        check_fixed(match[torch.from_numpy(keep_a).to(cuda)], dist[torch.from_numpy(keep_a).to(cuda)], em, ev,
                    what="nan %s" % mode)


def test_two_runs_bit_identical_and_dense_batch(cuda):
    """two runs agree bit for bit; a dense [P, N, D] batch equals its pairs"""
    from cirtorch.search import match_pairs
    a, b = case(5)
    a2, b2 = MC.descriptors(513, 770, 128, 31)
    ta, tb = dev(np.stack([a, a2]), cuda), dev(np.stack([b, b2]), cuda)
    for mode in MODES:
        m1, d1 = match_pairs(ta, tb, mode=mode, th=0.95)
        m2, d2 = match_pairs(ta, tb, mode=mode, th=0.95)
        assert tuple(m1.shape) == (2, 513) and tuple(d1.shape) == (2, 513)
        assert torch.equal(m1, m2) and d1.cpu().numpy().tobytes() == d2.cpu().numpy().tobytes()
        for p in range(2):
            mp, dp = match_pairs(ta[p], tb[p], mode=mode, th=0.95)
            assert torch.equal(mp, m1[p]) and dp.cpu().numpy().tobytes() == d1[p].cpu().numpy().tobytes()


def test_graph_capture_replay_equals_eager(cuda):
    from cirtorch.search import match_pairs
    from cirtorch.utils.graph import GraphedForward
    a, b = case(2)
    a2, _ = MC.descriptors(300, 257, 128, 41)
    tb = dev(np.stack([b, b[::-1]]), cuda)
    x1, x2 = dev(np.stack([a, a2]), cuda), dev(np.stack([a2, a]), cuda)
    g = GraphedForward(lambda x: match_pairs(x, tb, mode="smnn", th=0.8), x1)
    for x in (x2, x1):
        gm, gd = [t.clone() for t in g(x)]
        em, ed = match_pairs(x, tb, mode="smnn", th=0.8)
        assert torch.equal(gm, em) and gd.cpu().numpy().tobytes() == ed.cpu().numpy().tobytes()
        assert (em >= 0).sum().item() > 0


@pytest.mark.parametrize("k", [1, 6])
def test_top2_abi_vs_float64_numpy(cuda, k):
    """rr_match_top2 itself: both directions' two nearest rows by (distance, index), squared
    distances within (8 D + 12) 2^-53 of the float64 difference form (module docstring), d12
    and d21 the same bits"""
    from cirtorch import _ops
    a, b = case(k)
    n1, n2, d = MC.CASES[k]
    off = lambda n: dev(np.array([0, n], dtype=np.int64), cuda)  # noqa: E731
    d12, i12, d21, i21 = [t.cpu().numpy() for t in _ops.match_top2(dev(a, cuda), off(n1), dev(b, cuda), off(n2))]
    assert d12.dtype == np.float64 and i12.dtype == np.int32 and d12.shape == (n1, 2) and i21.shape == (n2, 2)
    dm2 = MC.dist2(a, b)
    tol = (8 * d + 12) * 2.0 ** -53
    for got_d, got_i, m in ((d12, i12, dm2), (d21, i21, dm2.T)):
        ed, ei = MC.top2(m)
        np.testing.assert_array_equal(got_i, ei)
        print("case", k, "max |d2 error|", np.abs(got_d - ed).max(), "bound", tol)
        np.testing.assert_allclose(got_d, ed, rtol=0, atol=tol)
        assert (got_d >= 0).all()
    # the same two rows give the same bits in both directions
    for i in range(n1):
        j = i12[i, 0]
        if i21[j, 0] == i:
            assert d12[i, 0] == d21[j, 0]
