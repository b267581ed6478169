"""What HardNet and SOSNet share: the seven-convolution trunk on the engine's kernels
(rr_patchnet_pack, rr_patchnet_describe; ``include/rr.h`` states the arithmetic).

The modules keep the reference's submodules, so its checkpoints load with ``strict=True``; the
convolutions and BatchNorms are never called.  The packed weights are built on the first forward
and again whenever a weight or a running statistic was replaced, moved or written in place.
"""

import torch
import torch.nn as nn

from .. import _ops


def trunk_layers(dropout):
    """The reference's layer list after the input normalisation: conv, BatchNorm(affine=False), ReLU
    six times, Dropout, the 8 x 8 conv and its BatchNorm"""
    layers = []
    for cout, cin, k in _ops.PATCHNET_SHAPES[:6]:
        stride = 2 if cin != cout and cin != 1 else 1
        layers += [nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=1, bias=False), nn.BatchNorm2d(cout, affine=False),
                   nn.ReLU()]
    layers += [nn.Dropout(dropout), nn.Conv2d(128, 128, kernel_size=8, bias=False), nn.BatchNorm2d(128, affine=False)]
    return layers


class PatchNet(nn.Module):
    """forward([B, 1, 32, 32] on the GPU) -> [B, 128] float32, in eval mode only, without gradients"""

    variant = None      # "hardnet" / "sosnet"
    upstream = None     # where the pretrained file is published

    def _trunk(self):
        raise NotImplementedError

    def _refuse_pretrained(self):
        raise RuntimeError("%s(pretrained=True): nothing is downloaded here.  Fetch %s yourself and pass its state dict "
                           "to load_state_dict()" % (type(self).__name__, self.upstream))

    def _tensors(self):
        convs = [m for m in self._trunk() if isinstance(m, nn.Conv2d)]
        bns = [m for m in self._trunk() if isinstance(m, nn.BatchNorm2d)]
        return [c.weight for c in convs], [b.running_mean for b in bns], [b.running_var for b in bns]

    def refresh_engine(self):
        """Drop the packed weights (they are rebuilt on the next forward)"""
        self._packed = None

    def _apply(self, fn, *args, **kwargs):
        self._packed = None
        return super()._apply(fn, *args, **kwargs)

    def _load_from_state_dict(self, *args, **kwargs):
        self._packed = None
        return super()._load_from_state_dict(*args, **kwargs)

    def packed(self):
        """The packed blob of the current weights: rebuilt when a tensor was replaced or written to"""
        w, m, v = self._tensors()
        key = tuple((t.data_ptr(), t._version) for t in w + m + v)
        cached = getattr(self, "_packed", None)
        if cached is None or cached[0] != key:
            if w[0].device.type != "cuda":
                raise RuntimeError("the MI355X engine runs on the GPU: call .cuda() on the module first")
            cached = (key, _ops.patchnet_pack(w, m, v))
            self._packed = cached
        return cached[1]

    def describe(self, patches, out=None):
        """float32 patches [..., 32, 32] on the GPU -> [B, 128] (no shape checks of forward)"""
        if self.training:
            raise NotImplementedError("%s runs in eval mode only: batch statistics and dropout are not built; call .eval()"
                                      % type(self).__name__)
        return _ops.patchnet_describe(patches, self.packed(), self.variant, out)

    def forward(self, input):
        if not torch.is_tensor(input):
            raise TypeError("Input type is not a torch.Tensor. Got {}".format(type(input)))
        if input.dim() != 4 or tuple(input.shape[1:]) != (1, 32, 32):
            raise ValueError("Invalid input shape, we expect Bx1x32x32. Got: {}".format(tuple(input.shape)))
        _ops.E.require_gpu(input)
        return self.describe(input[:, 0])
