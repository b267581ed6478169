"""Pooling modules (reference ``cirtorch/modules/pools.py``: MAC / SPoC / GeM
``:10-38``, GeMmp ``:43-54``, Rpool ``:118-197``)."""

import torch
import torch.nn as nn
from torch.nn.parameter import Parameter

from . import functional as LF
from .normalization import L2N
from .regions import roi_regions


class MAC(nn.Module):
    def forward(self, x):
        return LF.mac(x)

    def __repr__(self):
        return self.__class__.__name__ + "()"


class SPoC(nn.Module):
    def forward(self, x):
        return LF.spoc(x)

    def __repr__(self):
        return self.__class__.__name__ + "()"


class GeM(nn.Module):
    """Generalized-mean pooling with a learnable scalar p (state key ``p``,
    ``pools.py:34``): (mean_hw clamp(x, eps)^p)^(1/p)."""

    def __init__(self, p=3, eps=1e-6):
        super().__init__()
        self.p = Parameter(torch.ones(1) * p)
        self.eps = eps

    def forward(self, x):
        return LF.gem(x, p=self.p, eps=self.eps)

    def __repr__(self):
        return "%s(p=%.4f, eps=%s)" % (self.__class__.__name__, float(self.p.data[0]), self.eps)


class GeMmp(nn.Module):
    """GeM with one exponent per channel (``pools.py:43-54``).  The reference
    ``p`` is a plain tensor of shape [mp, 1, 1], not a Parameter: it is absent
    from the state dict, which stays so here (a non-persistent buffer, so that
    ``.cuda()`` moves it with the module).  Runs as the regional kernel on the
    single whole-map region."""

    def __init__(self, p=3, mp=1, eps=1e-6):
        super().__init__()
        self.mp = mp
        self.register_buffer("p", (torch.ones(self.mp) * p).unsqueeze(-1).unsqueeze(-1), persistent=False)
        self.eps = eps

    def forward(self, x):
        return LF.gemmp(x, p=self.p, eps=self.eps)

    def __repr__(self):
        return "%s(p=[%d], eps=%s)" % (self.__class__.__name__, self.mp, self.eps)


class Rpool(nn.Module):
    """Regional pooling (``pools.py:118-197``): the inner pool over every
    region of the R-MAC grid, each region vector L2N -> (whiten -> L2N), then
    summed and L2N-ed (``aggregate=True``: [N, D, 1, 1]) or returned per region
    (``aggregate=False``: [N, R, D, 1, 1]).  All regions are pooled by one
    engine launch per 32 regions instead of one inner-pool call per region; the
    grid is laid on the map as given (a padded batch's common size), like the
    reference."""

    def __init__(self, rpool, whiten=None, L=3, eps=1e-6):
        super().__init__()
        if not isinstance(rpool, (GeM, MAC, SPoC, GeMmp)):
            raise NotImplementedError("Rpool: the inner pool must be GeM, MAC, SPoC or GeMmp, got %r" % (rpool,))
        if whiten is not None and not (isinstance(whiten, nn.Linear) and whiten.in_features == whiten.out_features):
            raise NotImplementedError("Rpool: the regional whitening must be a square nn.Linear")
        self.rpool = rpool
        self.L = L
        self.whiten = whiten
        self.norm = L2N()
        self.eps = eps

    def regions(self, x):
        return roi_regions(x.shape[-2], x.shape[-1], self.L)

    def roipool(self, x):
        """[N, C, H, W] -> [N, R, C] float32 region vectors (``pools.py:127-172``)."""
        return LF.roipool(x, self.rpool, self.regions(x))

    def forward(self, x, aggregate=True):
        from .. import _ops
        o = self.roipool(x)
        n, R, d = o.shape
        eps = self.norm.eps
        if self.whiten is not None:
            # L2N -> Linear -> L2N on the n * R region rows: the fused head tail
            o = _ops.head_tail(o.reshape(n * R, d), self.whiten.weight, self.whiten.bias, whiten=True, eps=eps)
            o = o.reshape(n, R, d)
            if aggregate:
                return _ops.region_aggregate(o, l2n_rows=False, eps=eps).reshape(n, d, 1, 1)
        elif aggregate:
            return _ops.region_aggregate(o, l2n_rows=True, eps=eps).reshape(n, d, 1, 1)
        else:
            o = _ops.l2n_rows(o.reshape(n * R, d), eps)
        return o.reshape(n, R, d, 1, 1)

    def __repr__(self):
        return "%s(rpool=%r, whiten=%r, L=%d)" % (self.__class__.__name__, self.rpool, self.whiten, self.L)
