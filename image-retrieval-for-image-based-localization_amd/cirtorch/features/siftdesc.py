"""The reference's SIFT patch descriptor (``cirtorch/features/siftdesc.py``) on the engine's kernel
(rr_sift_describe).

Same names, arguments, shape checks and error types.  The reference builds gradients, magnitude,
orientation, one masked plane per angular bin and a convolution per plane in torch -- about thirty
full-size temporaries; here one block per patch keeps all of that in LDS and writes the
``num_ang_bins * num_spatial_bins ** 2`` values, float64 arithmetic rounded once.  Patches are
``[B, 1, PS, PS]`` on the GPU, 8 <= PS <= 64; the kernel reads float32, so float64 or half patches are
converted first and the descriptors are float32 whatever the input was.  There is no backward pass.
"""

import math

import torch
import torch.nn as nn

from .. import _ops


def get_sift_pooling_kernel(ksize=25):
    """
        The triangular (bilinear) pooling kernel of a spatial bin, [ksize, ksize]
    """
    half = float(ksize) / 2.0
    tri = half - (torch.arange(ksize).float() + 0.5 - half).abs()
    return torch.outer(tri, tri) / (half ** 2)


def get_sift_bin_ksize_stride_pad(patch_size, num_spatial_bins):
    """
        (ksize, stride, pad) of the pooling of a patch into num_spatial_bins x num_spatial_bins cells
    """
    geo = _ops.sift_geometry(patch_size, num_spatial_bins)
    if geo is None:
        raise ValueError("Patch size {} is incompatible with requested number of spatial bins {} for SIFT descriptor. "
                         "Usually it happens when patch size is too small for num_spatial_bins specified"
                         .format(patch_size, num_spatial_bins))
    return geo


def _gaussian_window(patch_size):
    """float32 [PS, PS]: the reference's get_gaussian_kernel2d((PS, PS), sigma = PS / sqrt 2, force_even)"""
    sigma = float(patch_size) / math.sqrt(2.0)
    x = torch.arange(patch_size) - patch_size // 2
    if patch_size % 2 == 0:
        x = x + 0.5
    g = torch.exp(-x.pow(2.0) / (2 * sigma ** 2))
    g = g / g.sum()
    return torch.outer(g, g)


class SIFTDescriptor(nn.Module):
    """
        SIFT (RootSIFT by default) descriptors of a batch of patches, [B, 1, PS, PS] ->
        [B, num_ang_bins * num_spatial_bins ** 2]
    """

    def __init__(self, patch_size=41, num_ang_bins=8, num_spatial_bins=4, rootsift=True, clipval=0.2):
        super(SIFTDescriptor, self).__init__()
        self.eps = 1e-10
        self.num_ang_bins = num_ang_bins
        self.num_spatial_bins = num_spatial_bins
        self.clipval = clipval
        self.rootsift = rootsift
        self.patch_size = patch_size
        self.bin_ksize, self.bin_stride, self.pad = get_sift_bin_ksize_stride_pad(patch_size, num_spatial_bins)

    def get_pooling_kernel(self):
        return get_sift_pooling_kernel(ksize=self.bin_ksize).view(1, 1, self.bin_ksize, self.bin_ksize)

    def get_weighting_kernel(self):
        return _gaussian_window(self.patch_size)

    def forward(self, input):
        if not len(input.shape) == 4:
            raise ValueError("Invalid input shape, we expect Bx1xHxW. Got: {}".format(input.shape))
        B, CH, W, H = input.size()
        if (W != self.patch_size) or (H != self.patch_size) or (CH != 1):
            raise TypeError("input shape should be must be [Bx1x{}x{}]. Got {}"
                            .format(self.patch_size, self.patch_size, input.size()))
        return _ops.sift_describe(input[:, 0], self.num_ang_bins, self.num_spatial_bins, self.rootsift, float(self.clipval))


def sift_describe(input, patch_size=41, num_ang_bins=8, num_spatial_bins=4, rootsift=True, clipval=0.2):
    """
        The functional form of :class:`SIFTDescriptor`.
    """
    return SIFTDescriptor(patch_size, num_ang_bins, num_spatial_bins, rootsift, clipval)(input)
