"""Homography solvers with the signatures of the reference's cirtorch/geometry/homography.py,
on the engine's batched DLT kernel (rr_homography_dlt): Hartley normalisation, the 9 x 9
A^T W A and its smallest eigenvector (cyclic Jacobi) in float64 on the GPU, one block per
batch element.  Inputs [B, N, 2] (N >= 4), output [B, 3, 3] in the input dtype; float32 inputs
are computed in float64 and rounded once.  GPU tensors only."""

import torch

from .. import _ops

_EPS = 1e-8


def _check(points1, points2, weights):
    if points1.shape != points2.shape:
        raise ValueError("homography: points1 %s and points2 %s differ in shape" % (tuple(points1.shape), tuple(points2.shape)))
    if points1.dim() != 3 or points1.shape[-1] != 2:
        raise ValueError("homography: points must be [B, N, 2], got %s" % (tuple(points1.shape),))
    if points1.shape[1] < 4:
        raise ValueError("homography: at least 4 points, got %d" % points1.shape[1])
    if points1.dtype not in (torch.float32, torch.float64) or points2.dtype != points1.dtype:
        raise ValueError("homography: float32 or float64 points of one dtype, got %s and %s" % (points1.dtype, points2.dtype))
    if weights is not None and tuple(weights.shape) != tuple(points1.shape[:2]):
        raise ValueError("homography: weights must be [B, N], got %s" % (tuple(weights.shape),))
    _ops.E.require_gpu(points1, points2, weights)


def _dlt64(p1, p2, w):
    """float64 [B, N, 2] x 2, float64 [B, N] or None -> float64 [B, 3, 3]"""
    b, n = p1.shape[0], p1.shape[1]
    off = torch.arange(b + 1, dtype=torch.int64, device=p1.device) * n
    return _ops.homography_dlt(p1.reshape(b * n, 2).contiguous(), p2.reshape(b * n, 2).contiguous(),
                               None if w is None else w.reshape(b * n).contiguous(), off)


def find_homography_dlt(points1, points2, weights=None):
    """The homography of the weighted DLT (homography.py:11-58 of the reference): the
    least-squares solution over N >= 4 correspondences, weights [B, N] on the points' rows."""
    _check(points1, points2, weights)
    H = _dlt64(points1.double(), points2.double(), None if weights is None else weights.double())
    return H.to(points1.dtype)


def _transfer(H, pts):
    """transform_points of the reference (geometry/linalg.py:187-228): z is divided out where |z| > eps"""
    u = pts @ H[:, :2, :2].transpose(1, 2) + H[:, None, :2, 2]
    z = pts @ H[:, 2:, :2].transpose(1, 2) + H[:, None, 2:, 2]
    return u * torch.where(z.abs() > _EPS, 1.0 / z, torch.ones_like(z))


def find_homography_dlt_iterated(points1, points2, weights, soft_inl_th=3.0, n_iter=5):
    """Iteratively re-weighted least squares (homography.py:61-74 of the reference): n_iter DLT
    solves, the weights of every solve after the first exp(-e^2 / (2 soft_inl_th^2)) of the
    previous H's transfer error e.  The re-weighting runs in torch on the device, in float64."""
    _check(points1, points2, weights)
    p1, p2 = points1.double(), points2.double()
    H = _dlt64(p1, p2, None if weights is None else weights.double())
    for _ in range(n_iter - 1):
        err2 = (_transfer(H, p1) - p2).pow(2).sum(dim=-1)
        H = _dlt64(p1, p2, torch.exp(-err2 / (2.0 * (soft_inl_th ** 2))))
    return H.to(points1.dtype)
