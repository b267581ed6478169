"""The R-MAC region grid of ``Rpool.roipool`` (reference
``cirtorch/modules/pools.py:127-172``) as host arithmetic: no GPU, no sync.

The reference forms the grid with float32 tensor arithmetic (the long-side
step count through ``torch.min(torch.abs(...))`` on a float32 tensor, first
index on ties; the centres through ``torch.floor(wl2 + torch.Tensor(range(k))
* b)``).  A float64 restatement can land on the other side of a ``floor``, so
the same operations run here in numpy float32; ``tests/golden/regions.npz``
holds the rectangles the reference visits for every map up to 40 x 40.
"""

import math

import numpy as np

_F = np.float32


def _centres(wl2, k, b):
    """floor(wl2 + [0 .. k-1] * b) - wl2 in float32 (pools.py:159,164)."""
    c = np.floor(_F(wl2) + np.arange(k, dtype=_F) * _F(b))
    return [int(v) - wl2 for v in c]


def roi_regions(H, W, L=3):
    """[(y0, x0, h, w), ...]: the whole map, then the squares of levels
    1 .. L in the order ``roipool`` pools them (level, then row centre, then
    column centre; levels whose side is 0 are skipped)."""
    H, W, L = int(H), int(W), int(L)
    if H < 1 or W < 1:
        raise ValueError("roi_regions: empty map %dx%d" % (H, W))
    ovr = _F(0.4)  # desired overlap of neighbouring regions
    steps = np.array([2, 3, 4, 5, 6, 7], dtype=_F)  # possible regions for the long dimension
    w = min(W, H)
    b = _F(max(H, W) - w) / (steps - _F(1))
    idx = int(np.argmin(np.abs((_F(w * w) - _F(w) * b) / _F(w * w) - ovr)))
    Wd = idx + 1 if H < W else 0
    Hd = idx + 1 if H > W else 0
    regions = [(0, 0, H, W)]
    for l in range(1, L + 1):
        wl = math.floor(2 * w / (l + 1))
        wl2 = math.floor(wl / 2 - 1)
        b = 0 if l + Wd == 1 else (W - wl) / (l + Wd - 1)
        cen_w = _centres(wl2, l + Wd, b)
        b = 0 if l + Hd == 1 else (H - wl) / (l + Hd - 1)
        cen_h = _centres(wl2, l + Hd, b)
        if wl == 0:
            continue
        for i in cen_h:
            for j in cen_w:
                regions.append((i, j, wl, wl))
    return regions
