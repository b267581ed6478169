"""The reference's ``conv_quad_interp3d`` / ``ConvQuadInterp3d``
(``cirtorch/geometry/subpix/spatial_soft_argmax.py:348-427``) on the engine's extrema kernel
(rr_scale_space_extrema): strict 3 x 3 x 3 maxima of a response volume and one SIFT-style quadratic
refinement of each, solved in float64.

Deviations, all stated in include/rr.h: the offsets sit on their own axes (the reference adds the x
offset to y and the y offset to x), no random ``eps`` term is added to the Hessian (``eps`` is
accepted and ignored; a singular system gives a zero offset), and ``torch.solve`` is not needed.
``ConvSoftArgmax3d`` exists so that code naming it imports, and raises in ``forward``.
"""

import torch
import torch.nn as nn

from ... import _ops


def conv_quad_interp3d(input, strict_maxima_bonus=10.0, eps=1e-7):
    """
        Function that computes the single iteration of quadratic interpolation of of the extremum (max or min) location
        and value per each 3x3x3 window which contains strict extremum, similar to one done is SIFT

        input [B, C, D, H, W] float32 on the GPU -> coords_max [B, C, 3, D, H, W] (level, x, y), y_max
        [B, C, D, H, W] (the refined value, plus strict_maxima_bonus at a strict maximum)
    """
    if not torch.is_tensor(input):
        raise TypeError("Input type is not a torch.Tensor. Got {}".format(type(input)))
    if not len(input.shape) == 5:
        raise ValueError("Invalid input shape, we expect BxCxDxHxW. Got: {}".format(input.shape))
    B, CH, D, H, W = input.shape
    mask, offs, vals = _ops.scale_space_extrema(input.reshape(B * CH, D, H, W), False)
    dev = input.device
    zs, ys, xs = torch.meshgrid(torch.arange(D, device=dev, dtype=torch.float32),
                                torch.arange(H, device=dev, dtype=torch.float32),
                                torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    coords_max = torch.stack([zs, xs, ys])[None, None] + offs.view(B, CH, 3, D, H, W)
    y_max = vals.view(B, CH, D, H, W)
    if strict_maxima_bonus > 0:
        y_max = y_max + strict_maxima_bonus * mask.view(B, CH, D, H, W).to(y_max.dtype)
    return coords_max, y_max


class ConvQuadInterp3d(nn.Module):
    """
        Module that calculates soft argmax 3d per window
        See :func:`geometry.subpix.conv_quad_interp3d` for details.
    """

    def __init__(self, strict_maxima_bonus=10.0, eps=1e-7):
        super(ConvQuadInterp3d, self).__init__()
        self.strict_maxima_bonus = strict_maxima_bonus
        self.eps = eps

    def forward(self, x):
        return conv_quad_interp3d(x, self.strict_maxima_bonus, self.eps)


class ConvSoftArgmax3d(nn.Module):
    """
        Not built.  As the suppression stage of a detector it keeps every voxel: the best responses
        of an image are one peak and its neighbours, with exactly tied scores whose order depends on
        the arithmetic.  Use :class:`ConvQuadInterp3d`.
    """

    def __init__(self, kernel_size=(3, 3, 3), stride=(1, 1, 1), padding=(1, 1, 1), temperature=torch.tensor(1.0),
                 normalized_coordinates=False, eps=1e-8, output_value=True, strict_maxima_bonus=0.0):
        super(ConvSoftArgmax3d, self).__init__()
        self.kernel_size, self.stride, self.padding = kernel_size, stride, padding
        self.temperature = temperature
        self.normalized_coordinates = normalized_coordinates
        self.eps = eps
        self.output_value = output_value
        self.strict_maxima_bonus = strict_maxima_bonus

    def forward(self, x):
        raise NotImplementedError("ConvSoftArgmax3d is not built: it keeps every voxel, so a detector's best responses "
                                  "are one peak and its exactly tied neighbours; use ConvQuadInterp3d")
