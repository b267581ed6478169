"""Pixel <-> normalised coordinates (``cirtorch/geometry/conversions.py:456-492``): the step between
``detect_keypoints`` (pixels) and ``localHead.forward`` (grid coordinates in [-1, 1]), plain
elementwise torch on whatever device the coordinates live on.
"""

import torch


def _factor(pixel_coordinates, height, width, eps):
    if pixel_coordinates.shape[-1] != 2:
        raise ValueError("Input pixel_coordinates must be of shape (*, 2). Got {}".format(pixel_coordinates.shape))
    hw = torch.tensor([width, height], device=pixel_coordinates.device, dtype=pixel_coordinates.dtype)
    return torch.tensor(2., device=pixel_coordinates.device, dtype=pixel_coordinates.dtype) / (hw - 1).clamp(eps)


def normalize_pixel_coordinates(pixel_coordinates, height, width, eps=1e-8):
    """
        Normalize pixel coordinates between -1 and 1: -1 on the extreme left, 1 on the extreme right (x = w-1).
    """
    return _factor(pixel_coordinates, height, width, eps) * pixel_coordinates - 1


def denormalize_pixel_coordinates(pixel_coordinates, height, width, eps=1e-8):
    """
        Denormalize pixel coordinates: -1 is the extreme left, 1 the extreme right (x = w-1).
    """
    factor = _factor(pixel_coordinates, height, width, eps)
    return torch.tensor(1., device=factor.device, dtype=factor.dtype) / factor * (pixel_coordinates + 1)
