"""The reference's ``gaussian_blur2d`` / ``GaussianBlur2d`` (``cirtorch/filters/gaussian.py:8-42``) on
the engine's blur kernel (rr_gaussian_blur).

Same names and argument order.  The reference builds the 2-D kernel and runs ``filter2D``; here one
kernel blurs along x and along y through LDS in float64 and rounds once to float32.  Input
``[B, C, H, W]`` float32 on the GPU.  Built: square kernels of an odd size up to 63 with equal sigmas
and ``border_type='reflect'``; anything else raises.
"""

import torch
import torch.nn as nn

from .. import _ops


def _square(kernel_size, sigma, border_type):
    if border_type != 'reflect':
        raise NotImplementedError("border_type=%r is not built: the blur kernel has reflect borders only" % (border_type,))
    if not isinstance(kernel_size, tuple) or len(kernel_size) != 2 or not isinstance(sigma, tuple) or len(sigma) != 2:
        raise TypeError("kernel_size and sigma must be tuples of length two. Got {}, {}".format(kernel_size, sigma))
    if kernel_size[0] != kernel_size[1] or sigma[0] != sigma[1]:
        raise NotImplementedError("only square kernels with equal sigmas are built, got %r, %r" % (kernel_size, sigma))
    ks = kernel_size[0]
    if not isinstance(ks, int) or ks % 2 == 0 or ks <= 0:
        raise TypeError("kernel_size must be an odd positive integer. Got {}".format(ks))
    return ks, float(sigma[0])


def gaussian_blur2d(input, kernel_size, sigma, border_type='reflect'):
    """
        Creates an operator that blurs a tensor using a Gaussian filter.
    """
    if not torch.is_tensor(input):
        raise TypeError("Input type is not a torch.Tensor. Got {}".format(type(input)))
    if not len(input.shape) == 4:
        raise ValueError("Invalid input shape, we expect BxCxHxW. Got: {}".format(input.shape))
    ks, s = _square(kernel_size, sigma, border_type)
    return _ops.gaussian_blur(input, ks, s)


class GaussianBlur2d(nn.Module):
    """
        Creates an operator that blurs a tensor using a Gaussian filter.
        See :func:`gaussian_blur2d` for details.
    """

    def __init__(self, kernel_size, sigma, border_type='reflect'):
        super(GaussianBlur2d, self).__init__()
        _square(kernel_size, sigma, border_type)
        self.kernel_size = kernel_size
        self.sigma = sigma
        self.border_type = border_type

    def forward(self, input):
        return gaussian_blur2d(input, self.kernel_size, self.sigma, self.border_type)
