"""The reference's corner / blob response functions (``cirtorch/features/responses.py:8-103``) and
their modules (``:132-183``) on the engine's response kernel (rr_response).

Same names, argument order, shape checks and error types.  The reference composes
``spatial_gradient`` -> products -> ``gaussian_blur2d`` -> score in torch and materialises about ten
full-size planes on the way; here one kernel reads the image once and writes the score once, in
float64 rounded once to float32.  Input ``[B, C, H, W]`` float32 or uint8 (a uint8 pixel counts as
``v / 255``) on the GPU, output float32 ``[B, C, H, W]``: every plane is scored on its own.

Only ``grads_mode='sobel'`` exists (``'diff'`` raises NotImplementedError).  ``dog_response`` and
``BlobDoG`` (``:106-130``) work on the levels of a scale pyramid, ``[B, C, L, H, W]`` float32 ->
``[B, C, L - 1, H, W]`` (rr_dog_response).
"""

import torch
import torch.nn as nn

from .. import _ops


def _check_input(input):
    if not len(input.shape) == 4:
        raise ValueError("Invalid input shape, we expect BxCxHxW. Got: {}".format(input.shape))


def _check_sigmas(input, sigmas, need_tensor):
    if sigmas is None:
        return
    if need_tensor and not torch.is_tensor(sigmas):
        raise TypeError("sigmas type is not a torch.Tensor. Got {}".format(type(sigmas)))
    if (not len(sigmas.shape) == 1) or (sigmas.size(0) != input.size(0)):
        raise ValueError("Invalid sigmas shape, we expect B == input.size(0). Got: {}".format(sigmas.shape))


def _check_mode(grads_mode):
    if grads_mode not in ['sobel', 'diff']:
        raise TypeError("mode should be either sobel or diff. Got {}".format(grads_mode))
    if grads_mode == 'diff':
        raise NotImplementedError("grads_mode='diff' is not built: the response kernel has the sobel gradients only")


def harris_response(input, k=0.04, grads_mode='sobel', sigmas=None):
    """
        Computes the Harris cornerness function. Function does not do any normalization or nms.
        (A tensor k is read on the host.)
    """
    _check_input(input)
    _check_sigmas(input, sigmas, True)
    _check_mode(grads_mode)
    return _ops.response(input, "harris", float(k), sigmas)


def gftt_response(input, grads_mode='sobel', sigmas=None):
    """
        Computes the Shi-Tomasi cornerness function. Function does not do any normalization or nms.
    """
    _check_input(input)
    _check_mode(grads_mode)
    _check_sigmas(input, sigmas, False)
    return _ops.response(input, "gftt", 0.0, sigmas)


def hessian_response(input, grads_mode='sobel', sigmas=None):
    """
        Computes the determinant of the Hessian matrix. Function does not do any normalization or nms.
    """
    _check_input(input)
    _check_sigmas(input, sigmas, False)
    _check_mode(grads_mode)
    return _ops.response(input, "hessian", 0.0, sigmas)


class CornerHarris(nn.Module):
    """
        nn.Module that calculates Harris corners
        See :func:`harris_response` for details.  k (a float or a tensor) is registered as the
        buffer ``k`` like the reference's; its value is read once here, so forward never waits
        for the device.
    """

    def __init__(self, k, grads_mode='sobel'):
        super(CornerHarris, self).__init__()
        if type(k) is float:
            self.register_buffer('k', torch.tensor(k))
        else:
            self.register_buffer('k', k)
        self._k = float(k)
        self.grads_mode = grads_mode

    def forward(self, input, sigmas=None):
        return harris_response(input, self._k, self.grads_mode, sigmas)


class CornerGFTT(nn.Module):
    """
        nn.Module that calculates Shi-Tomasi corners
        See :func:`gftt_response` for details.
    """

    def __init__(self, grads_mode='sobel'):
        super(CornerGFTT, self).__init__()
        self.grads_mode = grads_mode

    def forward(self, input, sigmas=None):
        return gftt_response(input, self.grads_mode, sigmas)


class BlobHessian(nn.Module):
    """
        nn.Module that calculates Hessian blobs
        See :func:`hessian_response` for details.
    """

    def __init__(self, grads_mode='sobel'):
        super(BlobHessian, self).__init__()
        self.grads_mode = grads_mode

    def forward(self, input, sigmas=None):
        return hessian_response(input, self.grads_mode, sigmas)


def dog_response(input):
    """
        Computes the Difference-of-Gaussian response given the Gaussian 5d input: level l + 1 minus level l
    """
    if not len(input.shape) == 5:
        raise ValueError("Invalid input shape, we expect BxCxDxHxW. Got: {}".format(input.shape))
    B, C, L, H, W = input.shape
    return _ops.dog_response(input.reshape(B * C, L, H, W)).view(B, C, L - 1, H, W)


class BlobDoG(nn.Module):
    """
        nn.Module that calculates Difference-of-Gaussians blobs
        See :func:`dog_response` for details.
    """

    def forward(self, input, sigmas=None):
        return dog_response(input)
