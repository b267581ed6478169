"""The reference's affine shape modules (``cirtorch/features/affine_shape.py``) on the engine's
kernels (rr_patch_affine_shape, rr_laf_affine_shape).

Same names, arguments, shape checks, error types and ``__repr__``.  ``PatchAffineShapeEstimator`` is
one kernel (float32 patches; other floating dtypes are converted first): Sobel gradients weighted by
the Gaussian window of sigma = PS / sqrt(2), their second moments, the degenerate rule (two of the
three raw moments below ``eps`` give a circle -- decided before the normalisation) and the division
by the largest moment.  ``LAFAffineShapeEstimator`` is the pyramid build and one kernel per call:
the patch of ``make_upright(laf)`` from its pyramid level (a frame past the last level is sampled
from the last level, where the reference's zero patch would give a circle), its shape,
``ellipse_to_laf`` and the rescaling to the input frame's scale stay in LDS and registers.  The
orientation of the input frame is not kept: run ``LAFOrienter`` afterwards, as the reference advises.
"""

import torch
import torch.nn as nn

from .. import _ops
from .laf import raise_error_if_laf_is_not_valid


class PatchAffineShapeEstimator(nn.Module):
    """
        The second moment matrix (a, b, c) of the patch gradients, normalised by its largest entry
        (rr_patch_affine_shape).  Patches are [B, 1, PS, PS] on the GPU, the result is float32 [B, 1, 3].
    """

    def __init__(self, patch_size=19, eps=1e-10):
        super(PatchAffineShapeEstimator, self).__init__()
        self.patch_size = patch_size
        self.eps = eps

    def __repr__(self):
        return self.__class__.__name__ + '(' + 'patch_size=' + str(self.patch_size) + ', ' + 'eps=' + str(self.eps) + ')'

    def forward(self, patch):
        if not torch.is_tensor(patch):
            raise TypeError("Input type is not a torch.Tensor. Got {}".format(type(patch)))
        if not len(patch.shape) == 4:
            raise ValueError("Invalid input shape, we expect Bx1xHxW. Got: {}".format(patch.shape))
        B, CH, W, H = patch.size()
        if (W != self.patch_size) or (H != self.patch_size) or (CH != 1):
            raise TypeError("input shape should be must be [Bx1x{}x{}]. Got {}"
                            .format(self.patch_size, self.patch_size, patch.size()))
        return _ops.patch_affine_shape(patch, self.eps)


class LAFAffineShapeEstimator(nn.Module):
    """
        Replaces the shape of every LAF by the affine shape of its patch, keeping its scale and
        centre (rr_laf_affine_shape); the result is upright
    """

    def __init__(self, patch_size=32):
        super(LAFAffineShapeEstimator, self).__init__()
        self.patch_size = patch_size
        self.affine_shape_detector = PatchAffineShapeEstimator(self.patch_size)

    def __repr__(self):
        return self.__class__.__name__ + '(' + 'patch_size=' + str(self.patch_size) + ')'

    def forward(self, laf, img):
        raise_error_if_laf_is_not_valid(laf)
        if not torch.is_tensor(img):
            raise TypeError("img type is not a torch.Tensor. Got {}".format(type(img)))
        if len(img.shape) != 4:
            raise ValueError("Invalid img shape, we expect BxCxHxW. Got: {}".format(img.shape))
        if laf.size(0) != img.size(0):
            raise ValueError("Batch size of laf and img should be the same. Got {}, {}".format(img.size(0), laf.size(0)))
        return _ops.laf_affine_shape(img, laf, None, self.patch_size, self.affine_shape_detector.eps)
