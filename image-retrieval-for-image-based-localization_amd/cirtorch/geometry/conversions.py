"""Pixel <-> normalised coordinates (``cirtorch/geometry/conversions.py:456-492``): the step between
``detect_keypoints`` (pixels) and ``localHead.forward`` (grid coordinates in [-1, 1]), plain
elementwise torch on whatever device the coordinates live on; and the reference's ``pi``, ``rad2deg``
and ``deg2rad`` (``:29-44``), which the LAF helpers use.
"""

import torch

# a float32 tensor, as the reference's (``conversions.py:29``): in a float64 computation it is still
# the float32 value of pi, which the describe kernels reproduce
pi = torch.tensor(3.14159265358979323846)


def rad2deg(tensor):
    """
        Radians -> degrees.
    """
    return 180. * tensor / pi.to(tensor.device).type(tensor.dtype)


def deg2rad(tensor):
    """
        Degrees -> radians.
    """
    return tensor * pi.to(tensor.device).type(tensor.dtype) / 180.


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
