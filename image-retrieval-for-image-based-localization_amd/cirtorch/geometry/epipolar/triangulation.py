"""``triangulate_points`` with the name and argument order of the reference's
cirtorch/geometry/epipolar/triangulation.py, on the engine's rr_triangulate_points kernel: the
4 x 4 DLT system of a correspondence (Hartley / Zisserman 12.2) and its null vector by one-sided
Jacobi in registers, float64, one block per batch element; GPU tensors only."""

import torch

from ... import _ops


def triangulate_points(P1, P2, points1, points2):
    """The 3-D points of correspondences between two views: projection matrices P1, P2 [B, 3, 4],
    points1, points2 [B, N, 2] -> [B, N, 3] in the input dtype.  float32 inputs are computed in
    float64 and rounded once.  (The reference also takes an extra leading dimension, which it uses
    for its four candidate motions; ``recover_pose`` covers that use.)"""
    if P1.dim() != 3 or tuple(P1.shape[-2:]) != (3, 4) or P2.shape != P1.shape:
        raise ValueError("triangulate_points: P1 and P2 must both be [B, 3, 4], got %s and %s" % (tuple(P1.shape), tuple(P2.shape)))
    if points1.dim() != 3 or points1.shape[-1] != 2 or points2.shape != points1.shape or points1.shape[0] != P1.shape[0]:
        raise ValueError("triangulate_points: points must be [B, N, 2] on both sides with the B of P1, got %s and %s"
                         % (tuple(points1.shape), tuple(points2.shape)))
    if points1.dtype not in (torch.float32, torch.float64) or any(x.dtype != points1.dtype for x in (points2, P1, P2)):
        raise ValueError("triangulate_points: float32 or float64 tensors of one dtype")
    _ops.E.require_gpu(P1, P2, points1, points2)
    b, n = points1.shape[:2]
    off = torch.arange(b + 1, dtype=torch.int64, device=points1.device) * n
    X = _ops.triangulate_points(points1.double().reshape(b * n, 2).contiguous(), points2.double().reshape(b * n, 2).contiguous(),
                                P1.double().contiguous(), P2.double().contiguous(), off)
    return X.view(b, n, 3).to(points1.dtype)
