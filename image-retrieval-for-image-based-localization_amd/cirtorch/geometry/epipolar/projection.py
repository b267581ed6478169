"""Camera-matrix helpers with the names and signatures of the reference's
cirtorch/geometry/epipolar/projection.py.  A few tensor operations each: plain torch on any device."""

import torch

from ..linalg import cross_product_matrix, eye_like, vec_like


def intrinsics_like(focal, input):
    """K [B, 3, 3] for the images `input` [B, C, H, W]: focal length `focal` on both axes, the
    principal point at the image centre (W / 2, H / 2)."""
    if input.dim() != 4 or not focal > 0:
        raise ValueError("intrinsics_like: a positive focal and images [B, C, H, W], got %r and %s" % (focal, tuple(input.shape)))
    h, w = input.shape[-2:]
    K = eye_like(3, input)
    K[..., 0, 0] = focal
    K[..., 1, 1] = focal
    K[..., 0, 2] = w / 2.0
    K[..., 1, 2] = h / 2.0
    return K


def scale_intrinsics(camera_matrix, scale_factor):
    """K of the image resized by `scale_factor`: focal lengths and principal point scaled, a copy."""
    s = torch.ones(3, 3, dtype=camera_matrix.dtype, device=camera_matrix.device)
    s[0, 0] = s[1, 1] = s[0, 2] = s[1, 2] = scale_factor
    return camera_matrix * s


def projection_from_KRt(K, R, t):
    """P = K [R | t]: K, R [..., 3, 3], t [..., 3, 1] -> [..., 3, 4]."""
    if tuple(K.shape[-2:]) != (3, 3) or tuple(R.shape[-2:]) != (3, 3) or tuple(t.shape[-2:]) != (3, 1):
        raise ValueError("projection_from_KRt: K, R [..., 3, 3] and t [..., 3, 1], got %s, %s and %s"
                         % (tuple(K.shape), tuple(R.shape), tuple(t.shape)))
    if not K.dim() == R.dim() == t.dim():
        raise ValueError("projection_from_KRt: K, R and t must have the same number of dimensions")
    return K @ torch.cat([R, t], dim=-1)


def KRt_from_projection(P, eps=1e-6):
    """P [B, 3, 4] -> (K upper triangular with a positive diagonal, R orthogonal, t [B, 3, 1]) with
    ``P = K [R | t]``: an RQ decomposition of the left 3 x 3 block through the QR decomposition of
    its row- and column-reversed transpose."""
    if P.dim() != 3 or tuple(P.shape[-2:]) != (3, 4):
        raise ValueError("KRt_from_projection: P must be [B, 3, 4], got %s" % (tuple(P.shape),))
    M, p4 = P[:, :, :3], P[:, :, 3:]
    flip = torch.eye(3, dtype=P.dtype, device=P.device).flip(0)
    q, r = torch.linalg.qr((flip @ M).transpose(1, 2))
    Q = flip @ q.transpose(1, 2)
    U = flip @ r.transpose(1, 2) @ flip
    sign = torch.diag_embed(torch.sign(torch.diagonal(U, dim1=-2, dim2=-1) + eps))
    K, R = U @ sign, sign @ Q
    return K, R, torch.linalg.inv(K) @ p4


def depth(R, t, X):
    """The depth ``(R X + t)_z`` of points X [..., N, 3] under the rigid motion R [..., 3, 3], t [..., 3, 1]: [..., N]."""
    return (R @ X.transpose(-2, -1))[..., 2, :] + t[..., 2, :]


def projections_from_fundamental(F_mat):
    """A pair of camera matrices compatible with F [B, 3, 3] (Hartley / Zisserman result 9.14):
    P1 = [I | 0], P2 = [[e2]_x F | e2] with e2 the left null vector of F -> [B, 3, 4, 2]."""
    if F_mat.dim() < 2 or tuple(F_mat.shape[-2:]) != (3, 3):
        raise ValueError("projections_from_fundamental: F must be [B, 3, 3], got %s" % (tuple(F_mat.shape),))
    e2 = torch.linalg.svd(F_mat.transpose(-2, -1))[2][..., -1, :]    # F^T e2 = 0
    P1 = torch.cat([eye_like(3, F_mat), vec_like(3, F_mat)], dim=-1)
    P2 = torch.cat([cross_product_matrix(e2) @ F_mat, e2.unsqueeze(-1)], dim=-1)
    return torch.stack([P1, P2], dim=-1)
