"""CPU checks of the batched matcher's host side: the match.npz fixture (generator
checksum, self-consistency with a numpy restatement of the four rules), the
argument checks of rr_match_top2 / rr_match_pairs (which return before anything is
enqueued, so they run without a GPU), and the Python surface's refusals."""

import ctypes
import os

import numpy as np
import pytest
import torch

import match_cases as MC
from conftest import PKG, golden

LIB = os.path.join(PKG, "librr.so")


def test_fixture_checksum_and_cases():
    g = golden("match.npz")
    assert [tuple(int(v) for v in c) for c in g["cases"]] == MC.CASES
    assert tuple(g["ths"]) == MC.THS
    for k, (n1, n2, d) in enumerate(MC.CASES):
        a, b = MC.descriptors(n1, n2, d, int(g["seeds"][k]))
        assert a.dtype == np.float32 and a.shape == (n1, d) and b.shape == (n2, d)
        np.testing.assert_allclose(MC.checksum(a, b), g["chk"][k], rtol=0, atol=1e-9)


@pytest.mark.parametrize("k", range(len(MC.CASES)))
def test_fixture_equals_numpy_restatement(k):
    """The reference's lists == the four rules restated on float64 ||a - b||: indices
    exactly, values to 1e-12 (torch.cdist in float64 against the direct form)."""
    g = golden("match.npz")
    n1, n2, d = MC.CASES[k]
    a, b = MC.descriptors(n1, n2, d, int(g["seeds"][k]))
    for th in MC.THS:
        mine = MC.rules(a, b, th)
        for mode in ("nn", "mnn", "snn", "smnn"):
            fn = mode if mode in ("nn", "mnn") else "%s_%s" % (mode, MC.tag(th))
            idxs, dists = g["c%d_%s_i" % (k, fn)].astype(np.int64), g["c%d_%s_d" % (k, fn)]
            match, val = MC.scatter(idxs, dists, n1)
            np.testing.assert_array_equal(mine[mode][0], match, err_msg=fn)
            np.testing.assert_allclose(mine[mode][1], val, rtol=1e-12, err_msg=fn)
            # the reference's row order: by the desc2 index for match_mnn with N1 > N2, else by desc1
            col = 1 if (mode == "mnn" and n1 > n2) else 0
            assert (np.diff(idxs[:, col]) > 0).all(), fn


def test_restatement_small_sides():
    """fewer than two rows on the other side: nn / mnn still match, the ratio rules keep nothing"""
    a, b = MC.descriptors(5, 1, 8, 1)
    r = MC.rules(a, b, 0.99)
    assert (r["nn"][0] == 0).all() and (r["mnn"][0] >= 0).sum() == 1
    assert (r["snn"][0] == -1).all() and (r["smnn"][0] == -1).all() and np.isinf(r["snn"][1]).all()
    r = MC.rules(a, b[:0], 0.99)
    assert all((r[m][0] == -1).all() and np.isinf(r[m][1]).all() for m in r)


def _lib():
    if not os.path.exists(LIB):
        pytest.skip("librr.so not built (run __graft_entry__.build())")
    from cirtorch import _engine
    return _engine, _engine.lib()


def test_match_argument_checks():
    """every refusal happens on the host: these calls pass made-up device addresses and
    must return before a kernel launch"""
    E, lib = _lib()
    p = ctypes.c_void_p(0x1000)   # "non-null, 16-byte aligned"; never dereferenced
    null = ctypes.c_void_p(0)
    need0 = lib.rr_match_workspace_bytes(10, 12, 0)
    need1 = lib.rr_match_workspace_bytes(10, 12, 1)
    assert need0 >= (10 + 12) * 8 and need1 >= need0 + (10 + 12) * 24

    def top2(a=p, aoff=p, b=p, boff=p, d=128, out=p, ws=p, wsb=need0, max_n1=10, rows1=10):
        return lib.rr_match_top2(a, aoff, rows1, b, boff, 12, 1, d, max_n1, 12, out, out, out, out, ws, wsb, null)

    def pairs(a=p, aoff=p, d=128, mode=E.RR_MATCH_MNN, out=p, ws=p, wsb=need1):
        return lib.rr_match_pairs(a, aoff, 10, p, p, 12, 1, d, 10, 12, mode, 0.8, out, out, ws, wsb, null)

    bad = [(top2, dict(d=0)), (top2, dict(d=3)), (top2, dict(d=130)), (top2, dict(d=516)), (top2, dict(a=null)),
           (top2, dict(b=null)), (top2, dict(aoff=null)), (top2, dict(boff=null)), (top2, dict(out=null)),
           (top2, dict(ws=null)), (top2, dict(wsb=need0 - 257)), (top2, dict(a=ctypes.c_void_p(0x1004))),
           (top2, dict(max_n1=11)), (top2, dict(rows1=-1)),
           (pairs, dict(d=2)), (pairs, dict(d=1024)), (pairs, dict(a=null)), (pairs, dict(aoff=null)),
           (pairs, dict(mode=4)), (pairs, dict(mode=-1)), (pairs, dict(out=null)), (pairs, dict(ws=null)),
           (pairs, dict(wsb=need0))]
    for fn, kw in bad:
        assert fn(**kw) != 0, (fn.__name__, kw)
        assert lib.rr_last_error().decode().startswith("rr_match_"), (fn.__name__, kw)
    # an empty problem is no error (and launches nothing)
    assert lib.rr_match_pairs(null, p, 0, null, p, 0, 0, 128, 0, 0, E.RR_MATCH_NN, 0.8, null, null, p, 256, null) == 0
    assert lib.rr_match_top2(null, p, 0, null, p, 0, 3, 128, 0, 0, null, null, null, null, p, 256, null) == 0


def test_dm_raises_not_implemented():
    from cirtorch.features import matching
    a, b = torch.zeros(4, 8), torch.zeros(5, 8)
    for fn in (matching.match_nn, matching.match_mnn, matching.match_snn, matching.match_smnn):
        with pytest.raises(NotImplementedError, match="distance matrix"):
            fn(a, b, dm=torch.zeros(4, 5))


def test_cpu_tensors_raise():
    from cirtorch.features import matching
    from cirtorch.search import match_pairs
    a, b = torch.zeros(4, 8), torch.zeros(5, 8)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        match_pairs(a, b)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        matching.match_mnn(a, b)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        matching.match_snn(a, b, 0.8)


def test_match_pairs_refuses_bad_arguments():
    from cirtorch.search import match_pairs
    a, b = torch.zeros(4, 8), torch.zeros(5, 8)
    with pytest.raises(ValueError):
        match_pairs(a, b, mode="ratio")
    with pytest.raises(ValueError):
        match_pairs(a, torch.zeros(5, 12))
    with pytest.raises(ValueError):
        match_pairs(a, b, offsets1=torch.zeros(2, dtype=torch.int64))
