"""The three small helpers of the reference's cirtorch/geometry/linalg.py that the epipolar modules
import, with its names and signatures; plain torch on any device."""

import torch


def cross_product_matrix(x):
    """x [B, 3] -> the skew-symmetric matrices [B, 3, 3] with ``[x]_x y = x x y``."""
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError("cross_product_matrix: x must be [B, 3], got %s" % (tuple(x.shape),))
    a, b, c = x.unbind(-1)
    o = torch.zeros_like(a)
    return torch.stack([o, -c, b, c, o, -a, -b, a, o], dim=-1).view(-1, 3, 3)


def eye_like(n, input):
    """n x n identities, one per batch element of `input`, on its device and in its dtype: [B, n, n]."""
    if n <= 0 or input.dim() < 1:
        raise ValueError("eye_like: n > 0 and a batched input, got %r and %s" % (n, tuple(input.shape)))
    return torch.eye(n, device=input.device, dtype=input.dtype).unsqueeze(0).repeat(input.shape[0], 1, 1)


def vec_like(n, tensor):
    """zero column vectors, one per batch element of `tensor`, on its device and in its dtype: [B, n, 1]."""
    if n <= 0 or tensor.dim() < 1:
        raise ValueError("vec_like: n > 0 and a batched tensor, got %r and %s" % (n, tuple(tensor.shape)))
    return torch.zeros(tensor.shape[0], n, 1, device=tensor.device, dtype=tensor.dtype)
