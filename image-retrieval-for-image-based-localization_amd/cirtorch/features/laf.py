"""Local affine frames (``cirtorch/features/laf.py``): the LAF helpers as plain elementwise torch on
whatever device the frames live on, and patch extraction on the engine's kernel (rr_extract_patches).

A LAF is ``[B, N, 2, 3]``: the 2 x 2 part maps the unit patch to the image, the third column is the
centre, in pixels (or normalised by ``normalize_laf``).  Same names, arguments and error types as
the reference.  ``extract_patches_simple`` replaces ``F.affine_grid`` + ``F.grid_sample`` (bilinear,
border, ``align_corners=False``) by one kernel that reads pixels and writes patches, float32 or
uint8 images (a uint8 pixel counts as ``v / 255``).

``extract_patches_from_pyramid`` builds the ``pyrdown`` levels of the image (rr_patch_pyramid) and
samples every frame from its level (rr_extract_patches_pyramid); while ``2 * scale / PS < sqrt(2)``
that is level 0 and the bits are those of the simple extraction.  A frame past the last level
raises NotImplementedError by default (that check reads one value from the device) or, with
``beyond="clamp"``, is sampled from the last level.  ``ellipse_to_laf`` is one kernel
(rr_ellipse_to_laf: the closed-form inverse, float32 frames).  The drawing helpers are not built.
"""

import math

import torch

from .. import _ops
from ..geometry.conversions import rad2deg, deg2rad


def raise_error_if_laf_is_not_valid(laf):
    """
        Verifies that the input is a tensor of shape [B, N, 2, 3]
    """
    if not torch.is_tensor(laf):
        raise TypeError("Laf type is not a torch.Tensor. Got {}".format(type(laf)))
    if len(laf.shape) != 4 or laf.size(2) != 2 or laf.size(3) != 3:
        raise ValueError("Invalid laf shape, we expect BxNx2x3. Got: {}".format(laf.shape))


def get_laf_scale(LAF, eps=1e-10):
    """
        Scale of the LAFs, [B, N, 1, 1]: sqrt(|det + eps|) of the 2 x 2 part
    """
    raise_error_if_laf_is_not_valid(LAF)
    det = LAF[..., 0:1, 0:1] * LAF[..., 1:2, 1:2] - LAF[..., 1:2, 0:1] * LAF[..., 0:1, 1:2] + eps
    return det.abs().sqrt()


def get_laf_center(LAF):
    """
        Centre (keypoint) of the LAFs, [B, N, 2]
    """
    raise_error_if_laf_is_not_valid(LAF)
    return LAF[..., 2]


def get_laf_orientation(LAF):
    """
        Orientation of the LAFs in degrees, [B, N, 1]
    """
    raise_error_if_laf_is_not_valid(LAF)
    return rad2deg(torch.atan2(LAF[..., 0, 1], LAF[..., 0, 0])).unsqueeze(-1)


def _rotation(angle_deg):
    """[..., 2, 2] rotation [[cos, sin], [-sin, cos]] of angles in degrees"""
    rad = deg2rad(angle_deg)
    c, s = torch.cos(rad), torch.sin(rad)
    return torch.stack([c, s, -s, c], dim=-1).view(*angle_deg.shape, 2, 2)


def laf_from_center_scale_ori(xy, scale, ori):
    """
        LAFs from centres xy [B, N, 2], scales [B, N, 1, 1] and orientations in degrees [B, N, 1]
    """
    for name, var, ndim, last in (("xy", xy, 3, 2), ("scale", scale, 4, 1), ("ori", ori, 3, 1)):
        if not torch.is_tensor(var):
            raise TypeError("{} type is not a torch.Tensor. Got {}".format(name, type(var)))
        if len(var.shape) != ndim or var.size(-1) != last or (name == "scale" and var.size(-2) != 1):
            raise TypeError("{} shape is wrong. Got {}".format(name, var.size()))
    unscaled = torch.cat([_rotation(ori.squeeze(-1)), xy.unsqueeze(-1)], dim=-1)
    return scale_laf(unscaled, scale)


def scale_laf(laf, scale_coef):
    """
        Multiplies the 2 x 2 part by scale_coef (a float or a tensor): centre, shape and orientation stay
    """
    if type(scale_coef) not in (float, torch.Tensor):   # exact types, like the reference: an int is refused
        raise TypeError("scale_coef should be float or torch.Tensor Got {}".format(type(scale_coef)))
    raise_error_if_laf_is_not_valid(laf)
    return torch.cat([scale_coef * laf[:, :, :2, :2], laf[:, :, :, 2:]], dim=3)


def make_upright(laf, eps=1e-9):
    """
        Removes the rotation of the 2 x 2 part (lower-triangular, same scale, shape and centre)
    """
    raise_error_if_laf_is_not_valid(laf)
    det = get_laf_scale(laf)
    a00, a01 = laf[..., 0:1, 0:1], laf[..., 0:1, 1:2]
    a10, a11 = laf[..., 1:2, 0:1], laf[..., 1:2, 1:2]
    b2a2 = torch.sqrt(a01 ** 2 + a00 ** 2) + eps
    row0 = torch.cat([b2a2 / det, torch.zeros_like(det)], dim=3)
    row1 = torch.cat([(a11 * a01 + a10 * a00) / (b2a2 * det), det / b2a2], dim=3)
    unit = torch.cat([torch.cat([row0, row1], dim=2), laf[..., :, 2:3]], dim=3)
    return scale_laf(unit, det)


def ellipse_to_laf(ells):
    """
        Ellipses (x, y, a, b, c) [B, N, 5] -> LAFs [B, N, 2, 3] (float32): the inverse of the
        lower-triangular square root [[sqrt|a|, 0], [b / (sqrt|a| + sqrt|c|), sqrt|c|]], centre (x, y)
    """
    if not torch.is_tensor(ells) or len(ells.size()) != 3 or ells.size(2) != 5:
        raise TypeError("ellipse shape should be must be [BxNx5]. Got {}"
                        .format(ells.size() if torch.is_tensor(ells) else type(ells)))
    return _ops.ellipse_to_laf(ells)


def _size_coef(LAF, images):
    n, ch, h, w = images.size()
    m = float(min(h, w))
    return torch.tensor([[m, m, float(w)], [m, m, float(h)]], dtype=LAF.dtype, device=LAF.device).view(1, 1, 2, 3)


def denormalize_laf(LAF, images):
    """
        Normalised LAFs -> pixels: the 2 x 2 part times min(h, w), the centre times (w, h)
    """
    raise_error_if_laf_is_not_valid(LAF)
    return _size_coef(LAF, images).expand_as(LAF) * LAF


def normalize_laf(LAF, images):
    """
        Pixel LAFs -> normalised: the 2 x 2 part over min(h, w), the centre over (w, h)
    """
    raise_error_if_laf_is_not_valid(LAF)
    return (1.0 / _size_coef(LAF, images)).expand_as(LAF) * LAF


def _pixel_lafs(img, laf, normalize_lafs_before_extraction):
    raise_error_if_laf_is_not_valid(laf)
    if not torch.is_tensor(img) or img.dim() != 4:
        raise ValueError("Invalid img shape, we expect BxCxHxW. Got: {}".format(getattr(img, "shape", type(img))))
    if laf.size(0) != img.size(0):
        raise ValueError("Batch size of laf and img should be the same. Got {}, {}".format(img.size(0), laf.size(0)))
    # normalize_lafs_before_extraction=False: the frames are normalised already
    return laf if normalize_lafs_before_extraction else denormalize_laf(laf, img)


def extract_patches_simple(img, laf, PS=32, normalize_lafs_before_extraction=True):
    """
        Patches [B, N, C, PS, PS] of the LAFs, sampled from the image itself (no smoothing)
    """
    return _ops.extract_patches(img, _pixel_lafs(img, laf, normalize_lafs_before_extraction), PS)


def extract_patches_from_pyramid(img, laf, PS=32, normalize_lafs_before_extraction=True, beyond="raise"):
    """
        Patches [B, N, C, PS, PS] of the LAFs, each sampled from the pyrdown level whose pixel pitch
        matches the patch's: level max(0, floor(log2(2 * scale / PS) + 0.5)).  Levels exist while
        their smaller side is at least PS.  A frame of a level past the last one raises
        NotImplementedError with beyond="raise" (one value is read from the device for that) and is
        sampled from the last level with beyond="clamp" (no synchronisation); the reference leaves
        a zero patch there.
    """
    if beyond not in ("raise", "clamp"):
        raise ValueError("beyond must be 'raise' or 'clamp'. Got {!r}".format(beyond))
    plaf = _pixel_lafs(img, laf, normalize_lafs_before_extraction)
    if beyond == "raise" and plaf.numel():
        last = len(_ops.pyramid_levels(img.size(2), img.size(3), int(PS))) - 1
        top = int(((2.0 * get_laf_scale(plaf.double()) / float(PS)).log2() + 0.5).floor().clamp(min=0).nan_to_num(0.0).max())
        if top > last:
            raise NotImplementedError("extract_patches_from_pyramid: a frame belongs to pyramid level {} but a {} x {} "
                                      "image has levels 0..{} at PS {} (pass beyond='clamp' to sample the last level)"
                                      .format(top, img.size(2), img.size(3), last, PS))
    return _ops.extract_patches_pyramid(img, plaf, PS)


def laf_to_boundary_points(LAF, n_pts=50):
    """
        [B, N, n_pts, 2]: the centre, then n_pts - 1 points of the frame's unit circle
    """
    raise_error_if_laf_is_not_valid(LAF)
    t = torch.linspace(0, 2 * math.pi, n_pts - 1, device=LAF.device, dtype=LAF.dtype)
    unit = torch.cat([torch.zeros(1, 2, device=LAF.device, dtype=LAF.dtype), torch.stack([torch.sin(t), torch.cos(t)], dim=1)])
    return torch.einsum("bnij,pj->bnpi", LAF[..., :2], unit) + LAF[..., 2].unsqueeze(2)


def laf_is_inside_image(laf, images, border=0):
    """
        Mask [B, N] of the LAFs whose boundary lies inside the image, `border` pixels from every edge
    """
    raise_error_if_laf_is_not_valid(laf)
    n, ch, h, w = images.size()
    pts = laf_to_boundary_points(laf, 12)
    good = (pts[..., 0] >= border) * (pts[..., 0] <= w - border) * (pts[..., 1] >= border) * (pts[..., 1] <= h - border)
    return good.min(dim=2)[0]
