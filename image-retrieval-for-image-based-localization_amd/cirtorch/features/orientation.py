"""The reference's patch orientation modules (``cirtorch/features/orientation.py``) on the engine's
kernels (rr_patch_orientation, rr_extract_patches).

Same names, arguments, shape checks and error types.  ``PatchDominantGradientOrientation`` is one
kernel (float32 patches; other floating dtypes are converted first): Sobel gradients, the
soft-binned orientation histogram (the mean over the patch, no Gaussian weight -- the reference
builds one and never applies it), circular smoothing and the argmax stay in LDS.  ``LAFOrienter``
extracts the patches of the frames it is given from their pyramid levels
(``laf.extract_patches_from_pyramid`` with ``beyond="clamp"``: a frame larger than the last level
allows is sampled from the last level), estimates the angles and returns
``make_upright(laf)`` rotated by them.  ``cirtorch.search.describe_keypoints`` does all of that and
the descriptor in one launch.
"""

import torch
import torch.nn as nn

from .. import _ops
from ..geometry.conversions import rad2deg
from .laf import _rotation, extract_patches_from_pyramid, make_upright, raise_error_if_laf_is_not_valid


class PassLAF(nn.Module):
    """
        The identity on LAFs: stands where an orientation or affine-shape estimator would, returns
        the frames it is given
    """

    def forward(self, laf, img):
        return laf


class PatchDominantGradientOrientation(nn.Module):
    """
        The angle, in radians, of the strongest bin of a patch's gradient-orientation histogram
        (rr_patch_orientation); an angle of zero is the +x direction.  Patches are [B, 1, PS, PS] on the
        GPU; float64 or half patches are converted to float32 first, the result is float32.
    """

    def __init__(self, patch_size=32, num_angular_bins=36, eps=1e-8):
        super(PatchDominantGradientOrientation, self).__init__()
        if eps != 1e-8:
            raise NotImplementedError("the orientation kernel has eps = 1e-8 built in")
        self.patch_size = patch_size
        self.num_ang_bins = num_angular_bins
        self.eps = eps

    def forward(self, patch):
        if not torch.is_tensor(patch):
            raise TypeError("Input type is not a torch.Tensor. Got {}".format(type(patch)))
        if not len(patch.shape) == 4:
            raise ValueError("Invalid input shape, we expect Bx1xHxW. Got: {}".format(patch.shape))
        B, CH, W, H = patch.size()
        if (W != self.patch_size) or (H != self.patch_size) or (CH != 1):
            raise TypeError("input shape should be must be [Bx1x{}x{}]. Got {}"
                            .format(self.patch_size, self.patch_size, patch.size()))
        return _ops.patch_orientation(patch[:, 0], self.num_ang_bins)


class LAFOrienter(nn.Module):
    """
        Gives every LAF its dominant gradient orientation: the patch of the frame (from its pyramid
        level) goes through :class:`PatchDominantGradientOrientation`, and ``make_upright(laf)`` turned by
        that angle is returned
    """

    def __init__(self, patch_size=32, num_angular_bins=36):
        super(LAFOrienter, self).__init__()
        self.patch_size = patch_size
        self.num_ang_bins = num_angular_bins
        self.angle_detector = PatchDominantGradientOrientation(self.patch_size, self.num_ang_bins)

    def forward(self, laf, img):
        raise_error_if_laf_is_not_valid(laf)
        if not torch.is_tensor(img):
            raise TypeError("img type is not a torch.Tensor. Got {}".format(type(img)))
        if len(img.shape) != 4:
            raise ValueError("Invalid img shape, we expect BxCxHxW. Got: {}".format(img.shape))
        if laf.size(0) != img.size(0):
            raise ValueError("Batch size of laf and img should be the same. Got {}, {}".format(img.size(0), laf.size(0)))
        B, N = laf.shape[:2]
        patches = extract_patches_from_pyramid(img, laf, self.patch_size, beyond="clamp").view(-1, 1, self.patch_size, self.patch_size)
        angles = self.angle_detector(patches).view(B, N)
        rot = _rotation(rad2deg(angles))
        return torch.cat([torch.matmul(make_upright(laf)[..., :2, :2], rot), laf[..., :2, 2:]], dim=3)
