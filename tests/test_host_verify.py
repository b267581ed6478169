"""CPU checks of spatial verification's host side: the verify.npz fixture (generator checksums;
the numpy restatement of tests/verify_cases.py against the reference's float64 H matrices
within the fixture's tol_px, and against the stored RANSAC results), the sampling hash, the
argument checks of rr_verify_pairs / rr_homography_dlt (they return before anything is enqueued,
so they run without a GPU), the Python surface's refusals and rerank_by_inliers."""

import ctypes

import numpy as np
import pytest
import torch

import verify_cases as VC
from conftest import golden


def test_fixture_checksums():
    g = golden("verify.npz")
    for k, (b, n, weighted) in enumerate(VC.DLT_CASES):
        p1, p2, w = VC.dlt_points(b, n, weighted, int(g["dlt_seeds"][k]))
        np.testing.assert_allclose(VC.checksum(p1, p2, np.ones((b, n)) if w is None else w), g["dlt_chk"][k], rtol=0, atol=1e-6)
    for k, case in enumerate(VC.VERIFY_CASES):
        kp1, off1, kp2, off2, match, _ = VC.build_case(case, int(g["v_seeds"][k]))
        assert kp1.dtype == np.float32 and kp2.dtype == np.float32 and match.dtype == np.int64
        np.testing.assert_allclose(VC.checksum(kp1, kp2, match), g["v_chk"][k], rtol=0, atol=1e-6)
        assert kp1.size == 0 or (kp1.min() >= 0 and kp1[:, 0].max() < VC.W and kp1[:, 1].max() < VC.H_IMG)
        assert kp2.size == 0 or (kp2.min() >= 0 and kp2[:, 0].max() < VC.W and kp2[:, 1].max() < VC.H_IMG)


@pytest.mark.parametrize("k", range(len(VC.DLT_CASES)))
def test_dlt_restatement_equals_reference(k):
    """np.linalg.eigh restatement == the reference's float64 torch.svd run, by corner transfer"""
    g = golden("verify.npz")
    b, n, weighted = VC.DLT_CASES[k]
    p1, p2, w = VC.dlt_points(b, n, weighted, int(g["dlt_seeds"][k]))
    assert g["dlt_tol"][k] >= 1e-9 and g["dlt_tol_it"][k] >= 1e-9
    for i in range(b):
        wi = None if w is None else w[i]
        e = VC.corner_err(VC.dlt(p1[i], p2[i], wi), g["dlt%d_H" % k][i])
        ei = VC.corner_err(VC.dlt_iterated(p1[i], p2[i], np.ones(n) if wi is None else wi), g["dlt%d_Hit" % k][i])
        print("dlt case", k, i, "corner err px", e, ei, "tol", g["dlt_tol"][k], g["dlt_tol_it"][k])
        assert e <= g["dlt_tol"][k] and ei <= g["dlt_tol_it"][k]


@pytest.mark.parametrize("k", range(len(VC.VERIFY_CASES)))
def test_verify_restatement_equals_fixture(k):
    g = golden("verify.npz")
    case = VC.VERIFY_CASES[k]
    kp1, off1, kp2, off2, match, planted = VC.build_case(case, int(g["v_seeds"][k]))
    inl, Hs, mask, infos = VC.verify_batch(kp1, off1, kp2, off2, match, VC.TH, case["iters"], case["refine"], VC.RUN_SEED)
    np.testing.assert_array_equal(inl, g["v%d_inl" % k])
    np.testing.assert_array_equal(mask, g["v%d_mask" % k])
    np.testing.assert_array_equal([o["t"] for o in infos], g["v%d_t" % k])
    for p, o in enumerate(infos):
        assert o["m"] == case["pairs"][p][2]
        assert int(mask[off1[p]:off1[p + 1]].sum()) == inl[p]
        if inl[p]:
            assert VC.corner_err(Hs[p], g["v%d_H" % k][p]) <= g["v%d_tol" % k][p]
        else:
            assert not Hs[p].any() and not g["v%d_H" % k][p].any()


def test_sampling_hash():
    """four distinct in-range indices; a pure function of (seed, p, t); known values pin the rule"""
    for m in (4, 5, 7, 40, 1025):
        s = VC.draw4(99, 3, np.arange(200), m)
        assert s.min() >= 0 and s.max() < m
        assert all(len(set(r)) == 4 for r in s.tolist())
        np.testing.assert_array_equal(s[17], VC.draw4(99, 3, [17], m)[0])
    assert not np.array_equal(VC.draw4(1, 0, np.arange(50), 40), VC.draw4(2, 0, np.arange(50), 40))
    assert not np.array_equal(VC.draw4(1, 0, np.arange(50), 40), VC.draw4(1, 1, np.arange(50), 40))
    assert not np.array_equal(VC.draw4(1, 0, np.arange(50), 40), VC.draw4(1 + (1 << 32), 0, np.arange(50), 40))
    assert int(VC.mix(0)) == 0 and int(VC.mix(1)) == 0x688990C0   # the 32-bit mixer itself
    # every index of a small set is drawn about equally often
    c = np.bincount(VC.draw4(5, 0, np.arange(4000), 8).reshape(-1), minlength=8)
    assert c.min() > 1800 and c.max() < 2200


def _lib():
    from cirtorch import _engine
    return _engine, _engine.lib()


def test_verify_argument_checks():
    """every refusal happens on the host: made-up device addresses, nothing is launched"""
    E, lib = _lib()
    p = ctypes.c_void_p(0x1000)
    null = ctypes.c_void_p(0)
    need = lib.rr_verify_workspace_bytes(10, 2, 1024)
    assert need >= 10 * 32 + 2 * 4 + 2 * 4 * 8
    # one 8-byte key per (pair, chunk of 256 hypotheses)
    assert lib.rr_verify_workspace_bytes(10, 100, 1 << 16) >= 10 * 32 + 100 * 4 + 100 * 256 * 8
    assert lib.rr_verify_workspace_bytes(10, 100, 1) < 100 * 256 * 8

    def verify(kp1=p, off1=p, kp2=p, off2=p, match=p, rows1=10, npairs=2, max_n1=10, th=3.0, iters=1024, refine=2,
               inl=p, H=p, mask=p, ws=p, wsb=need):
        return lib.rr_verify_pairs(kp1, off1, rows1, kp2, off2, 12, match, npairs, max_n1, th, iters, refine, 7, inl, H,
                                   mask, ws, wsb, null)

    bad = [dict(kp1=null), dict(kp2=null), dict(off1=null), dict(off2=null), dict(match=null), dict(inl=null),
           dict(H=null), dict(mask=null), dict(ws=null), dict(iters=0), dict(iters=-5), dict(refine=-1), dict(th=0.0),
           dict(th=-1.0), dict(th=float("inf")), dict(th=float("nan")), dict(wsb=need - 257), dict(wsb=0),
           dict(max_n1=11), dict(max_n1=-1), dict(rows1=-1), dict(npairs=-1), dict(kp1=ctypes.c_void_p(0x1004))]
    for kw in bad:
        assert verify(**kw) != 0, kw
        assert lib.rr_last_error().decode().startswith("rr_verify_pairs"), kw
    # an empty problem is no error and launches nothing
    assert verify(npairs=0) == 0
    assert lib.rr_verify_pairs(null, p, 0, null, p, 0, null, 0, 0, 3.0, 1, 0, 0, null, null, null, p, 256, null) == 0

    def dlt(p1=p, p2=p, w=null, off=p, rows=10, npairs=2, H=p):
        return lib.rr_homography_dlt(p1, p2, w, off, rows, npairs, H, null, 0, null)

    for kw in [dict(p1=null), dict(p2=null), dict(off=null), dict(H=null), dict(rows=-1), dict(npairs=-1),
               dict(p1=ctypes.c_void_p(0x1008))]:
        assert dlt(**kw) != 0, kw
        assert lib.rr_last_error().decode().startswith("rr_homography_dlt"), kw
    assert dlt(npairs=0) == 0 and dlt(npairs=0, H=null, w=p) == 0


def test_cpu_tensors_raise():
    from cirtorch.geometry import find_homography_dlt, find_homography_dlt_iterated
    from cirtorch.search import verify_pairs
    k1, k2, m = torch.zeros(2, 6, 2), torch.zeros(2, 7, 2), torch.zeros(2, 6, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        verify_pairs(k1, k2, m)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        verify_pairs(k1.view(12, 2), k2.view(14, 2), m.view(12), offsets1=torch.tensor([0, 6, 12]), offsets2=torch.tensor([0, 7, 14]))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        find_homography_dlt(k1, k1 + 1)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        find_homography_dlt_iterated(k1, k1 + 1, torch.ones(2, 6))


def test_python_refusals():
    from cirtorch.geometry import find_homography_dlt, find_homography_dlt_iterated
    from cirtorch.search import rerank_by_inliers, verify_pairs
    k1, k2, m = torch.zeros(2, 6, 2), torch.zeros(2, 7, 2), torch.zeros(2, 6, dtype=torch.int64)
    for args, kw in [((k1, k2, m), dict(iters=0)), ((k1, k2, m), dict(refine=-1)), ((k1, k2, m), dict(th=0.0)),
                     ((k1, k2, m), dict(th=float("nan"))), ((k1, k2, m), dict(max_n1=5)),
                     ((k1, k2, m.int()), {}), ((k1, k2, m[:, :5]), {}), ((k1, k2[:1], m), {}),
                     ((torch.zeros(2, 6, 3), k2, m), {}), ((k1, k2, m), dict(offsets1=torch.tensor([0, 6, 12]))),
                     ((k1, k2.view(14, 2), m), {}),
                     ((k1, k2, m), dict(offsets1=torch.tensor([0, 6, 12]), offsets2=torch.tensor([0, 7, 14])))]:
        with pytest.raises(ValueError):
            verify_pairs(*args, **kw)
    for fn, args in [(find_homography_dlt, (k1, k2)), (find_homography_dlt, (k1[:, :3], k1[:, :3])),
                     (find_homography_dlt, (k1[0], k1[0])), (find_homography_dlt, (k1, k1.double())),
                     (find_homography_dlt, (k1, k1, torch.ones(2, 5))), (find_homography_dlt, (k1.long(), k1.long())),
                     (find_homography_dlt_iterated, (k1, k2, torch.ones(2, 6))),
                     (find_homography_dlt_iterated, (k1, k1, torch.ones(3, 6)))]:
        with pytest.raises(ValueError):
            fn(*args)
    with pytest.raises(ValueError):
        rerank_by_inliers(torch.zeros(3, 2, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ValueError):
        rerank_by_inliers(torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int32))


def test_rerank_by_inliers_equals_python_sort():
    from cirtorch.search import rerank_by_inliers
    r = np.random.default_rng(3)
    k, q = 9, 5
    idx = np.stack([r.permutation(100)[:k] for _ in range(q)], 1).astype(np.int64)       # [k, Q]
    inl = r.integers(0, 4, (k, q)).astype(np.int32)                                      # many ties
    inl[:, 0] = 7                                                                        # all equal: order kept
    inl[:, 1] = np.arange(k)                                                             # ascending: reversed
    got = rerank_by_inliers(torch.from_numpy(idx), torch.from_numpy(inl)).numpy()
    for c in range(q):
        want = [idx[i, c] for i in sorted(range(k), key=lambda i: (-int(inl[i, c]), i))]
        assert got[:, c].tolist() == want
    assert got[:, 0].tolist() == idx[:, 0].tolist() and got[:, 1].tolist() == idx[::-1, 1].tolist()
    assert got.dtype == np.int64
