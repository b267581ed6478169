"""Fundamental-matrix routines with the names and signatures of the reference's
cirtorch/geometry/epipolar/fundamental.py.  ``find_fundamental`` runs on the engine's batched
8-point kernel (rr_fundamental_dlt): Hartley normalisation, the 9 x 9 X^T W X and its smallest
eigenvector (cyclic Jacobi), the rank-2 projection and the de-normalisation in float64 on the GPU,
one block per batch element; GPU tensors only.  ``normalize_points``, ``normalize_transformation``
and ``compute_correspond_epilines`` are a few tensor operations each: plain torch on any device."""

import torch

from ... import _ops


def normalize_points(points, eps=1e-8):
    """Isotropic normalisation (Hartley / Zisserman 4.4.4): points [B, N, 2] -> (the points moved to
    zero mean and mean distance sqrt(2) [B, N, 2], the transform that does it [B, 3, 3])."""
    if points.dim() != 3 or points.shape[-1] != 2:
        raise ValueError("normalize_points: points must be [B, N, 2], got %s" % (tuple(points.shape),))
    mean = points.mean(dim=1, keepdim=True)
    scale = (points - mean).norm(dim=-1).mean(dim=-1)
    scale = torch.sqrt(torch.tensor(2.)).to(points.device) / (scale + eps)   # float32 sqrt(2), as the reference
    ones, zeros = torch.ones_like(scale), torch.zeros_like(scale)
    transform = torch.stack([scale, zeros, -scale * mean[..., 0, 0],
                             zeros, scale, -scale * mean[..., 0, 1],
                             zeros, zeros, ones], dim=-1).view(-1, 3, 3)
    points_norm = points @ transform[:, :2, :2].transpose(1, 2) + transform[:, None, :2, 2]
    return points_norm, transform


def normalize_transformation(M, eps=1e-8):
    """M [..., 3, 3] divided by its last entry (+ eps) where that entry's magnitude exceeds eps."""
    if M.dim() < 2:
        raise ValueError("normalize_transformation: M must be [..., R, C], got %s" % (tuple(M.shape),))
    norm_val = M[..., -1:, -1:]
    return torch.where(norm_val.abs() > eps, M / (norm_val + eps), M)


def find_fundamental(points1, points2, weights):
    """The fundamental matrix of the weighted 8-point algorithm: points [B, N, 2] (N >= 8) on both
    sides, weights [B, N] -> F [B, 3, 3] in the input dtype with ``x2^T F x1 = 0``.  float32 inputs
    are computed in float64 and rounded once."""
    if points1.shape != points2.shape:
        raise ValueError("find_fundamental: points1 %s and points2 %s differ in shape" % (tuple(points1.shape), tuple(points2.shape)))
    if points1.dim() != 3 or points1.shape[-1] != 2:
        raise ValueError("find_fundamental: points must be [B, N, 2], got %s" % (tuple(points1.shape),))
    if points1.shape[1] < 8:
        raise ValueError("find_fundamental: at least 8 points, got %d" % points1.shape[1])
    if points1.dtype not in (torch.float32, torch.float64) or points2.dtype != points1.dtype:
        raise ValueError("find_fundamental: float32 or float64 points of one dtype, got %s and %s" % (points1.dtype, points2.dtype))
    if weights is None or tuple(weights.shape) != tuple(points1.shape[:2]):
        raise ValueError("find_fundamental: weights must be [B, N], got %s" % (None if weights is None else tuple(weights.shape),))
    _ops.E.require_gpu(points1, points2, weights)
    b, n = points1.shape[0], points1.shape[1]
    off = torch.arange(b + 1, dtype=torch.int64, device=points1.device) * n
    F = _ops.fundamental_dlt(points1.double().reshape(b * n, 2).contiguous(), points2.double().reshape(b * n, 2).contiguous(),
                             weights.double().reshape(b * n).contiguous(), off)
    return F.to(points1.dtype)


def compute_correspond_epilines(points, F_mat):
    """The epipolar lines F [x, y, 1]^T of points [B, N, 2] -> [B, N, 3], (a, b) scaled to unit length."""
    if points.dim() != 3 or points.shape[2] != 2:
        raise ValueError("compute_correspond_epilines: points must be [B, N, 2], got %s" % (tuple(points.shape),))
    if F_mat.dim() != 3 or tuple(F_mat.shape[-2:]) != (3, 3):
        raise ValueError("compute_correspond_epilines: F_mat must be [B, 3, 3], got %s" % (tuple(F_mat.shape),))
    points_h = torch.nn.functional.pad(points, [0, 1], "constant", 1.0)
    a, b, c = torch.chunk(F_mat @ points_h.permute(0, 2, 1), dim=1, chunks=3)
    nu = a * a + b * b
    nu = torch.where(nu > 0., 1. / torch.sqrt(nu), torch.ones_like(nu))
    return torch.cat([a * nu, b * nu, c * nu], dim=1).permute(0, 2, 1)


def fundamental_from_essential(E_mat, K1, K2):
    """F = K2^-T E K1^-1 (Hartley / Zisserman 9.12, the inverse of ``essential_from_fundamental``): all
    [..., 3, 3] with the same number of dimensions.  It takes the E of
    ``verify_pairs(model="essential")`` to the F that ``recover_pose`` expects."""
    for x, what in ((E_mat, "E_mat"), (K1, "K1"), (K2, "K2")):
        if x.dim() < 2 or tuple(x.shape[-2:]) != (3, 3):
            raise ValueError("fundamental_from_essential: %s must be [..., 3, 3], got %s" % (what, tuple(x.shape)))
    if not E_mat.dim() == K1.dim() == K2.dim():
        raise ValueError("fundamental_from_essential: E_mat, K1 and K2 must have the same number of dimensions")
    return torch.linalg.inv(K2).transpose(-2, -1) @ E_mat @ torch.linalg.inv(K1)
