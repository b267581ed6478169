"""Pinhole projection and back-projection in plain torch: ``project_points`` and ``unproject_points`` of
the reference's cirtorch/geometry/camera/perspective.py:7-42 and :45-91, the two functions a user of
``localize_pairs``' pose reaches for (``project_points(X @ R.T + t, K)`` is where a 3-D point falls in
the query image).  Any device, any float dtype, differentiable; they read fx, fy, cx, cy of the
camera matrix and ignore a skew, as the reference does."""

import torch


def _intrinsics(camera_matrix):
    if tuple(camera_matrix.shape[-2:]) != (3, 3):
        raise ValueError("camera_matrix must be (*, 3, 3), got %s" % (tuple(camera_matrix.shape),))
    return camera_matrix[..., 0, 0], camera_matrix[..., 1, 1], camera_matrix[..., 0, 2], camera_matrix[..., 1, 2]


def project_points(point_3d, camera_matrix):
    """point_3d (*, 3) in the camera frame, camera_matrix (*, 3, 3) -> pixel coordinates (*, 2):
    u = fx X / Z + cx, v = fy Y / Z + cy.  A point with |Z| <= 1e-8 is not divided (the rule of the
    reference's convert_points_from_homogeneous, conversions.py:67-83)."""
    if point_3d.device != camera_matrix.device:
        raise ValueError("project_points: the inputs must be on one device")
    if point_3d.shape[-1] != 3:
        raise ValueError("project_points: point_3d must be (*, 3), got %s" % (tuple(point_3d.shape),))
    fx, fy, cx, cy = _intrinsics(camera_matrix)
    z = point_3d[..., 2]
    far = z.abs() > 1e-8
    scale = torch.where(far, 1.0 / torch.where(far, z, torch.ones_like(z)), torch.ones_like(z))
    return torch.stack([point_3d[..., 0] * scale * fx + cx, point_3d[..., 1] * scale * fy + cy], dim=-1)


def unproject_points(point_2d, depth, camera_matrix, normalize=False):
    """point_2d (*, 2) pixels, depth (*, 1), camera_matrix (*, 3, 3) -> points (*, 3) in the camera frame:
    ((u - cx) / fx, (v - cy) / fy, 1) times depth; normalize=True scales that ray to unit length first, so
    that depth is the distance along it and not Z."""
    if not (point_2d.device == depth.device == camera_matrix.device):
        raise ValueError("unproject_points: the inputs must be on one device")
    if point_2d.shape[-1] != 2:
        raise ValueError("unproject_points: point_2d must be (*, 2), got %s" % (tuple(point_2d.shape),))
    if depth.shape[-1] != 1:
        raise ValueError("unproject_points: depth must be (*, 1), got %s" % (tuple(depth.shape),))
    fx, fy, cx, cy = _intrinsics(camera_matrix)
    x = (point_2d[..., 0] - cx) / fx
    y = (point_2d[..., 1] - cy) / fy
    ray = torch.stack([x, y, torch.ones_like(x)], dim=-1)
    if normalize:
        ray = torch.nn.functional.normalize(ray, dim=-1, p=2)
    return ray * depth
