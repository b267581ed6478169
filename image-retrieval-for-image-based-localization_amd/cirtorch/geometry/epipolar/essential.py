"""Essential-matrix routines with the names and argument order of the reference's
cirtorch/geometry/epipolar/essential.py.  ``decompose_essential_matrix``, ``motion_from_essential``
and ``motion_from_essential_choose_solution`` run on the engine's pose kernels
(rr_essential_decompose, rr_recover_pose): the 3 x 3 decomposition, the four candidate motions, the
triangulation under each and the choice by the depths in float64 on the GPU, without a
``torch.svd``; GPU tensors only.  The others are a few tensor operations each: plain torch on any
device.  float32 inputs are computed in float64 and rounded once.

Which of the two rotations is called R1 and which sign t carries follow the signs an SVD leaves
open: the set {(R1, t), (R1, -t), (R2, t), (R2, -t)} equals the reference's, its order need not."""

import torch

from ... import _ops
from ..linalg import cross_product_matrix


def _mats(x, what, name):
    if x.dim() < 2 or tuple(x.shape[-2:]) != (3, 3):
        raise ValueError("%s: %s must be [..., 3, 3], got %s" % (name, what, tuple(x.shape)))


def essential_from_fundamental(F_mat, K1, K2):
    """E = K2^T F K1 (Hartley / Zisserman 9.12): all [..., 3, 3] with the same number of dimensions."""
    for x, what in ((F_mat, "F_mat"), (K1, "K1"), (K2, "K2")):
        _mats(x, what, "essential_from_fundamental")
    if not F_mat.dim() == K1.dim() == K2.dim():
        raise ValueError("essential_from_fundamental: F_mat, K1 and K2 must have the same number of dimensions")
    return K2.transpose(-2, -1) @ F_mat @ K1


def decompose_essential_matrix(E_mat):
    """E [..., 3, 3] -> (R1, R2 [..., 3, 3], t [..., 3, 1]): the two rotations and the unit translation
    (up to sign) of the motions that E admits; R1 and R2 have determinant +1."""
    _mats(E_mat, "E_mat", "decompose_essential_matrix")
    if E_mat.dtype not in (torch.float32, torch.float64):
        raise ValueError("decompose_essential_matrix: float32 or float64, got %s" % E_mat.dtype)
    _ops.E.require_gpu(E_mat)
    lead = tuple(E_mat.shape[:-2])
    R1, R2, t = _ops.essential_decompose(E_mat.double().reshape(-1, 3, 3).contiguous())
    dt = E_mat.dtype
    return R1.view(lead + (3, 3)).to(dt), R2.view(lead + (3, 3)).to(dt), t.view(lead + (3, 1)).to(dt)


def essential_from_Rt(R1, t1, R2, t2):
    """The essential matrix [t]_x R of the motion from camera (R1, t1) to camera (R2, t2):
    rotations [..., 3, 3], translations [..., 3, 1]."""
    R, t = relative_camera_motion(R1, t1, R2, t2)
    lead = tuple(R.shape[:-2])
    return cross_product_matrix(t[..., 0].reshape(-1, 3)).view(lead + (3, 3)) @ R


def motion_from_essential(E):
    """The four motions of E [..., 3, 3]: Rs [..., 4, 3, 3] = (R1, R1, R2, R2), Ts [..., 4, 3, 1] = (t, -t, t, -t)."""
    R1, R2, t = decompose_essential_matrix(E)
    return torch.stack([R1, R1, R2, R2], dim=-3), torch.stack([t, -t, t, -t], dim=-3)


def motion_from_essential_choose_solution(E_mat, K1, K2, x1, x2, mask=None):
    """The motion among the four of E [B, 3, 3] under which the most correspondences x1, x2
    [B, N, 2] (pixels; K1, K2 [B, 3, 3]) triangulate in front of both cameras, and those points:
    -> (R [B, 3, 3], t [B, 3, 1], points3d [B, N, 3]).  mask bool [B, N] restricts the points that
    are used (the others come back as zeros).  The points are taken as float32 pixel keypoints, the
    engine's keypoint format.  Each batch element chooses its own motion; the reference applies the
    choice of element 0 to the whole batch (essential.py:149-151)."""
    name = "motion_from_essential_choose_solution"
    for x, what in ((E_mat, "E_mat"), (K1, "K1"), (K2, "K2")):
        _mats(x, what, name)
        if x.dim() != 3:
            raise ValueError("%s: %s must be [B, 3, 3], got %s" % (name, what, tuple(x.shape)))
    b = E_mat.shape[0]
    if x1.dim() != 3 or x1.shape[-1] != 2 or x2.shape != x1.shape or x1.shape[0] != b or K1.shape[0] != b or K2.shape[0] != b:
        raise ValueError("%s: x1 and x2 must both be [B, N, 2] with the B of E_mat, K1 and K2, got %s and %s"
                         % (name, tuple(x1.shape), tuple(x2.shape)))
    if mask is not None and (tuple(mask.shape) != tuple(x1.shape[:-1]) or mask.dtype != torch.bool):
        raise ValueError("%s: mask must be bool [B, N], got %s %s" % (name, mask.dtype, tuple(mask.shape)))
    if E_mat.dtype not in (torch.float32, torch.float64):
        raise ValueError("%s: float32 or float64, got %s" % (name, E_mat.dtype))
    _ops.E.require_gpu(E_mat, K1, K2, x1, x2, mask)
    n = x1.shape[1]
    Ka, Kb = K1.double().contiguous(), K2.double().contiguous()
    # the entry takes F and forms K2^T F K1 itself
    F = torch.linalg.inv(Kb).transpose(-2, -1) @ E_mat.double() @ torch.linalg.inv(Ka)
    off = torch.arange(b + 1, dtype=torch.int64, device=x1.device) * n
    match = torch.arange(n, dtype=torch.int64, device=x1.device).repeat(b)    # row i of side 1 with row i of side 2
    R, t, _, _, pts, _ = _ops.recover_pose(x1.float().reshape(b * n, 2).contiguous(), off, x2.float().reshape(b * n, 2).contiguous(),
                                           off, match, None if mask is None else mask.reshape(b * n).contiguous(),
                                           F.contiguous(), Ka, Kb, n, covered=True)
    dt = E_mat.dtype
    return R.to(dt), t.unsqueeze(-1).to(dt), pts.view(b, n, 3).to(dt)


def relative_camera_motion(R1, t1, R2, t2):
    """The motion T2 T1^-1 that takes camera (R1, t1) to camera (R2, t2): (R2 R1^T, t2 - R2 R1^T t1)."""
    for R, t in ((R1, t1), (R2, t2)):
        if R.dim() < 2 or tuple(R.shape[-2:]) != (3, 3) or t.dim() < 2 or tuple(t.shape[-2:]) != (3, 1):
            raise ValueError("relative_camera_motion: rotations [..., 3, 3] and translations [..., 3, 1], got %s and %s"
                             % (tuple(R.shape), tuple(t.shape)))
    R = R2 @ R1.transpose(-2, -1)
    return R, t2 - R @ t1


def run_5point(points1, points2):
    """The essential matrices through five correspondences (rr_essential_5pt): points1, points2
    [B, 5, 2] in normalised coordinates (``K^-1 [x, y, 1]``) -> (E [B, 10, 3, 3] with
    ``[x2, y2, 1] E [x1, y1, 1]^T = 0``, each of unit Frobenius norm, in ascending root order and zero
    past the sample's number of solutions; nroots int32 [B], an even number up to 10).  Computed in
    float64, one GPU thread per sample; GPU tensors only."""
    if points1.dim() != 3 or tuple(points1.shape[1:]) != (5, 2) or points1.shape != points2.shape:
        raise ValueError("run_5point: points must be [B, 5, 2] on both sides, got %s and %s"
                         % (tuple(points1.shape), tuple(points2.shape)))
    if points1.dtype not in (torch.float32, torch.float64) or points2.dtype != points1.dtype:
        raise ValueError("run_5point: float32 or float64 on both sides, got %s and %s" % (points1.dtype, points2.dtype))
    _ops.E.require_gpu(points1, points2)
    Em, nroots = _ops.essential_5pt(points1.double().contiguous(), points2.double().contiguous())
    return Em.to(points1.dtype), nroots
