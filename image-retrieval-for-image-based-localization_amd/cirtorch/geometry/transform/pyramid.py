"""The reference's ``ScalePyramid`` (``cirtorch/geometry/transform/pyramid.py:30-158``) on the engine's
pyramid entry (rr_scale_pyramid): every octave in one call, levels blurred from the float64 value of
the level before and rounded once to float32.

Same constructor and outputs.  The reference's ``forward`` reads ``self.init_sigma`` and its detector
``self.scale_pyr.n_levels``, which its constructor never sets; both are set here.
``double_image=True`` is not built.

``pyrdown`` / ``PyrDown`` (``pyramid.py:161-196``) are one kernel (rr_pyrdown): the 5 x 5 binomial blur
with reflect padding and the bilinear halving as a single separable 6-tap pass at stride 2.  Other
border types and ``align_corners=True`` are not built.
"""

import torch
import torch.nn as nn

from ... import _ops


class ScalePyramid(nn.Module):
    """
        Creates an scale pyramid of image, usually used for local feature detection.
        Images are consequently smoothed with Gaussian blur and downscaled.

    Returns:
        Tuple(List(Tensors), List(Tensors), List(Tensors)):
        1st output: images [B, 1, levels + 3, h_o, w_o] per octave (views of one buffer)
        2nd output: sigmas [B, levels + 3] per octave
        3rd output: pixelDists [B, levels + 3] per octave
    """

    def __init__(self, levels=3, sigma=1.6, min_size=15, double_image=False):
        super(ScalePyramid, self).__init__()
        if double_image:
            raise NotImplementedError("double_image=True is not built: the pyramid starts at the image's own size")
        self.levels = self.n_levels = levels
        self.sigma = self.init_sigma = sigma
        self.min_size = min_size
        self.double_image = double_image
        self.extra_levels = 3
        self.border = min_size // 2 - 1
        self.sigma_step = 2 ** (1. / float(self.levels))

    def forward(self, x):
        if not torch.is_tensor(x):
            raise TypeError("Input type is not a torch.Tensor. Got {}".format(type(x)))
        pyr, octs = _ops.scale_pyramid(x, self.levels, self.sigma, self.min_size)
        B = x.shape[0]
        sigmas = [torch.tensor(o["sigmas"], dtype=torch.float32).repeat(B, 1).to(x.device) for o in octs]
        pixel_dists = [torch.full((B, self.levels + self.extra_levels), float(2 ** i), dtype=torch.float32).to(x.device)
                       for i in range(len(octs))]
        return pyr, sigmas, pixel_dists


def pyrdown(input, border_type='reflect', align_corners=False):
    """
        Blurs a tensor and downsamples it.
    """
    return PyrDown(border_type, align_corners)(input)


class PyrDown(nn.Module):
    """
        Blurs a tensor and downsamples it: [B, C, H, W] -> [B, C, H // 2, W // 2], float32 on the GPU
    """

    def __init__(self, border_type='reflect', align_corners=False):
        super(PyrDown, self).__init__()
        if border_type != 'reflect':
            raise NotImplementedError("border_type {!r} is not built: the kernel pads by reflection".format(border_type))
        if align_corners:
            raise NotImplementedError("align_corners=True is not built")
        self.border_type = border_type
        self.align_corners = align_corners

    def forward(self, input):
        if not torch.is_tensor(input):
            raise TypeError("Input type is not a torch.Tensor. Got {}".format(type(input)))
        if not len(input.shape) == 4:
            raise ValueError("Invalid input shape, we expect BxCxHxW. Got: {}".format(input.shape))
        return _ops.pyrdown(input)
