"""The reference's 2-D non-maxima suppression (``cirtorch/features/nms.py:29-67,111-116``) on the
engine's kernel (rr_nms2d).

The reference spreads the ``k*k`` window positions over ``k*k`` channels with a one-hot convolution
and takes their maximum; here one kernel compares a pixel with its window.  The results are the
reference's bit for bit on finite maps: a pixel is kept when it is greater than every other
position of the window (coordinates clamped, so no pixel on the map's edge is kept) and greater
than 0 -- the reference's centre filter is all zeros, so its "maximum of the others" includes 0.
Square windows of 3, 5, 7 or 9 (the reference's ``view`` raises on non-square ones; here that is a
ValueError).  ``nms3d`` belongs to the scale pyramid, which is out of scope.
"""

import torch.nn as nn

from .. import _ops


class NonMaximaSuppression2d(nn.Module):
    """
        Applies non maxima suppression to filter.
    """

    def __init__(self, kernel_size):
        super(NonMaximaSuppression2d, self).__init__()
        assert isinstance(kernel_size, tuple), type(kernel_size)
        assert len(kernel_size) == 2, kernel_size
        if kernel_size[0] != kernel_size[1]:
            raise ValueError("nms2d: the window must be square, got {}".format(kernel_size))
        if kernel_size[0] not in _ops.NMS_SIZES:
            raise ValueError("nms2d: window {} (sides of 3, 5, 7 or 9)".format(kernel_size))
        self.kernel_size = kernel_size

    def forward(self, x, mask_only=False):
        assert len(x.shape) == 4, x.shape
        return _ops.nms2d(x, self.kernel_size[0], mask_only)


def nms2d(input, kernel_size, mask_only=False):
    """
        Applies non maxima suppression to filter.
        See :class:`NonMaximaSuppression2d` for details.
    """
    return NonMaximaSuppression2d(kernel_size)(input, mask_only)


def nms3d(input, kernel_size, mask_only=False):
    raise NotImplementedError("nms3d is not built: the engine's detector is single-scale (responses, nms2d and "
                              "top-N selection); the scale pyramid and its 3-D suppression are out of scope")
