"""Epipolar distances with the names and signatures of the reference's
cirtorch/geometry/epipolar/metrics.py, on the engine's rr_epipolar_distance kernel -- the
residual routine the RANSAC scorer of ``verify_pairs(model="fundamental")`` uses.  Points
[B, N, 2], or homogeneous [B, N, 3] with third coordinate 1; Fm [B, 3, 3]; output [B, N] in the
input dtype, computed in float64.  GPU tensors only."""

import torch

from ... import _ops


def _points(pts, what):
    if pts.dim() != 3 or pts.shape[-1] not in (2, 3):
        raise ValueError("%s: points must be [B, N, 2] or [B, N, 3], got %s" % (what, tuple(pts.shape)))
    if pts.shape[-1] == 3:
        # raises from the host: this check reads the tensor back (not for graph capture)
        if not bool((pts[..., 2] == 1).all()):
            raise ValueError("%s: homogeneous points must have third coordinate 1" % what)
        pts = pts[..., :2]
    return pts


def _distance(pts1, pts2, Fm, squared, eps, kind, what):
    if Fm.dim() != 3 or tuple(Fm.shape[-2:]) != (3, 3):
        raise ValueError("Fm must be a (*, 3, 3) tensor. Got {}".format(Fm.shape))
    _ops.E.require_gpu(pts1, pts2, Fm)
    p1, p2 = _points(pts1, what), _points(pts2, what)
    if p1.shape != p2.shape or Fm.shape[0] != p1.shape[0]:
        raise ValueError("%s: pts1 %s, pts2 %s and Fm %s do not agree" % (what, tuple(pts1.shape), tuple(pts2.shape), tuple(Fm.shape)))
    b, n = p1.shape[0], p1.shape[1]
    off = torch.arange(b + 1, dtype=torch.int64, device=p1.device) * n
    out = _ops.epipolar_distance(p1.double().reshape(b * n, 2).contiguous(), p2.double().reshape(b * n, 2).contiguous(),
                                 Fm.double().contiguous(), off, kind, squared, eps)
    return out.view(b, n).to(pts1.dtype)


def sampson_epipolar_distance(pts1, pts2, Fm, squared=True, eps=1e-8):
    """Sampson distance (Hartley / Zisserman 11.9) of correspondences under Fm; squared=False
    returns sqrt(d + eps)."""
    return _distance(pts1, pts2, Fm, squared, eps, "sampson", "sampson_epipolar_distance")


def symmetrical_epipolar_distance(pts1, pts2, Fm, squared=True, eps=1e-8):
    """Symmetrical epipolar distance (Hartley / Zisserman 11.10) of correspondences under Fm;
    squared=False returns sqrt(d + eps)."""
    return _distance(pts1, pts2, Fm, squared, eps, "symmetrical", "symmetrical_epipolar_distance")
