"""Absolute pose from 2-D to 3-D correspondences: the minimal three-point solver on the GPU.  The batched
RANSAC on top of it is ``cirtorch.search.localize_pairs`` (rr_localize_pairs); include/rr.h states
every rule.  The reference has no absolute pose."""

import torch

from .. import _ops


def solve_p3p(points2d_normalised, points3d):
    """The camera poses that put three 3-D points on the rays of three image points (rr_p3p, Grunert's
    elimination): points2d_normalised [B, 3, 2] in normalised coordinates (``K^-1 [x, y, 1]``),
    points3d [B, 3, 3] -> (R [B, 4, 3, 3], t [B, 4, 3] with ``[x, y, 1]^T ~ R X + t``, in ascending order
    of the quartic's root and zero past the sample's number of solutions; nsol int32 [B], up to 4).
    Computed in float64, one GPU thread per sample; GPU tensors only."""
    x, X = points2d_normalised, points3d
    if x.dim() != 3 or tuple(x.shape[1:]) != (3, 2) or X.dim() != 3 or tuple(X.shape[1:]) != (3, 3) or x.shape[0] != X.shape[0]:
        raise ValueError("solve_p3p: points must be [B, 3, 2] and [B, 3, 3], got %s and %s" % (tuple(x.shape), tuple(X.shape)))
    if x.dtype not in (torch.float32, torch.float64) or X.dtype not in (torch.float32, torch.float64):
        raise ValueError("solve_p3p: float32 or float64 points, got %s and %s" % (x.dtype, X.dtype))
    _ops.E.require_gpu(x, X)
    R, t, nsol = _ops.p3p(x.double().contiguous(), X.double().contiguous())
    return R, t, nsol
