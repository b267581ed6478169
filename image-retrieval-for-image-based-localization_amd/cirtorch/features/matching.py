"""The reference's descriptor matchers (``cirtorch/features/matching.py:5-154``) on
the engine's batched matching kernel (``cirtorch.search.match_pairs``, rr_match_pairs).

Same signatures and return values: ``(dists [B3, 1] float32, idxs [B3, 2] int64)``,
rows in the reference's order.  The reference forms ``torch.cdist(desc1, desc2)``
(an N1 x N2 matrix) and reduces it; here the two nearest rows of both directions
come from one launch in float64 and only the fixed-shape result is compacted on
the device (``nonzero``: the one synchronisation a data-dependent output shape
needs).  A precomputed distance matrix (``dm=``) is not taken: the engine never
forms one.
"""

import torch

from ..search import match_pairs


def _check(desc1, desc2, dm):
    if dm is not None:
        raise NotImplementedError("cirtorch.features.matching: dm= (a precomputed distance matrix) is not supported; "
                                  "the engine matches from the descriptors without forming the N1 x N2 matrix")
    assert len(desc1.shape) == 2
    assert len(desc2.shape) == 2


def _compact(match, dist, first_is_desc1=True):
    """fixed-shape (match, dist) -> the kept rows as (dists [B3, 1], idxs [B3, 2])"""
    rows = torch.nonzero(match >= 0).flatten()
    other = match[rows]
    idxs = torch.stack([rows, other] if first_is_desc1 else [other, rows], dim=1)
    return dist[rows].view(-1, 1), idxs.view(-1, 2)


def match_nn(desc1, desc2, dm=None):
    """Nearest neighbour in desc2 of every desc1 row: dists [B1, 1], idxs [B1, 2]."""
    _check(desc1, desc2, dm)
    return _compact(*match_pairs(desc1, desc2, "nn"))


def match_mnn(desc1, desc2, dm=None):
    """Mutual nearest neighbours: dists [B3, 1], idxs [B3, 2] (desc1 index, desc2 index),
    listed by the desc1 index when B1 <= B2 and by the desc2 index otherwise, like the
    reference."""
    _check(desc1, desc2, dm)
    if desc1.shape[0] <= desc2.shape[0]:
        return _compact(*match_pairs(desc1, desc2, "mnn"))
    return _compact(*match_pairs(desc2, desc1, "mnn"), first_is_desc1=False)


def match_snn(desc1, desc2, th=0.8, dm=None):
    """Nearest neighbours that pass the first / second distance ratio test (<= th):
    dists [B3, 1] hold the ratio."""
    _check(desc1, desc2, dm)
    assert desc2.shape[0] >= 2  # the second-nearest check needs two descriptors
    return _compact(*match_pairs(desc1, desc2, "snn", th))


def match_smnn(desc1, desc2, th=0.8, dm=None):
    """Mutual nearest neighbours that pass the ratio test in both directions:
    dists [B3, 1] hold the larger of the two ratios."""
    _check(desc1, desc2, dm)
    assert desc1.shape[0] >= 2
    assert desc2.shape[0] >= 2
    return _compact(*match_pairs(desc1, desc2, "smnn", th))
