"""Shared by tests/golden/make_golden_match.py and the matching tests: the cases of
tests/golden/match.npz, the descriptor generator (regenerated from the stored seed,
guarded by the fixture's float64 checksum) and a numpy float64 restatement of the
top-2 search and of the four matching rules."""

import numpy as np

from oracle import data

CASES = [(2, 2, 32), (65, 64, 256), (300, 257, 128), (37, 1000, 128), (1000, 37, 128), (513, 770, 128), (3, 1025, 64)]
THS = (0.8, 0.95)


def tag(th):
    return "%02d" % round(th * 100)


def descriptors(n1, n2, d, seed):
    """(a [n1, d], b [n2, d]) float32 unit rows: b Gaussian directions; 60 % of the a rows
    are a b row plus noise of relative size s in [0.0175, 0.35] (true matches whose
    first / second ratio spreads over (0, 1)), the others unrelated."""
    r = data.rng(seed)
    b = r.standard_normal((n2, d))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    a = r.standard_normal((n1, d))
    m = int(round(0.6 * n1))
    rows = r.permutation(n1)[:m]
    src = r.integers(0, max(n2, 1), m)
    s = r.uniform(0.0175, 0.35, m)
    if n2:
        a[rows] = b[src] + s[:, None] * r.standard_normal((m, d)) * (3.0 / np.sqrt(d))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    return a.astype(np.float32), b.astype(np.float32)


def checksum(a, b):
    return np.array([a.astype(np.float64).sum(), b.astype(np.float64).sum()], dtype=np.float64)


def dist2(a, b):
    """float64 squared L2 distances of float32 rows, by differences (no cancellation)"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    out = np.empty((a.shape[0], b.shape[0]), dtype=np.float64)
    for i in range(a.shape[0]):
        out[i] = ((a[i][None, :] - b) ** 2).sum(1)
    return out


def top2(dm2):
    """per row of a squared-distance matrix: (d [n, 2], i [n, 2]) by (distance, index);
    (+inf, -1) where the row has fewer than two columns"""
    n, m = dm2.shape
    d = np.full((n, 2), np.inf)
    i = np.full((n, 2), -1, dtype=np.int64)
    if m:
        order = np.argsort(dm2, axis=1, kind="stable")[:, :2]
        k = order.shape[1]
        i[:, :k] = order
        d[:, :k] = np.take_along_axis(dm2, order, axis=1)
    return d, i


def rules(a, b, th):
    """The four matchers restated on float64 distances: {mode: (match [n1] int64, value [n1])}
    in the fixed-shape form of cirtorch.search.match_pairs (-1 / inf where nothing is kept)."""
    dm2 = dist2(a, b)
    d12, i12 = top2(dm2)
    d21, i21 = top2(dm2.T)
    n1, n2 = dm2.shape
    s12, s21 = np.sqrt(d12), np.sqrt(d21)
    with np.errstate(divide="ignore", invalid="ignore"):
        r12 = s12[:, 0] / s12[:, 1]
        r21 = s21[:, 0] / s21[:, 1]
    j = i12[:, 0]
    have = j >= 0
    jj = np.where(have, j, 0)
    mutual = have & (i21[jj, 0] == np.arange(n1)) if n2 else np.zeros(n1, dtype=bool)
    ok12 = have & (n2 >= 2) & (r12 <= th)
    ok21 = (r21[jj] <= th) & (n1 >= 2) if n2 else np.zeros(n1, dtype=bool)
    out = {}
    for mode, keep, val in (("nn", have, s12[:, 0]), ("mnn", mutual, s12[:, 0]), ("snn", ok12, r12),
                            ("smnn", ok12 & mutual & ok21, np.maximum(r12, r21[jj] if n2 else r12))):
        out[mode] = (np.where(keep, j, -1).astype(np.int64), np.where(keep, val, np.inf))
    return out


def scatter(idxs, dists, n1):
    """the compacted (idxs [B3, 2], dists [B3]) of a matcher -> fixed shape (match, value)"""
    match = np.full(n1, -1, dtype=np.int64)
    val = np.full(n1, np.inf)
    match[idxs[:, 0]] = idxs[:, 1]
    val[idxs[:, 0]] = np.asarray(dists).reshape(-1)
    return match, val
