"""The reference's SOSNet (``cirtorch/features/sosnet.py``) on the engine's fused kernels.

Same name and submodule structure (``layers.0 .. layers.21``, ``desc_norm``), so an upstream
checkpoint loads with ``strict=True``.  The forward pass is rr_patchnet_describe: InstanceNorm2d of
the patch, the trunk in fp16 with float32 accumulation, and ``desc_norm`` of ``features + 1e-10``,
which over 128 channels is ``v / |v|``.
"""

import torch.nn as nn

from .patchnet import PatchNet, trunk_layers

urls = dict()
urls["lib"] = "https://github.com/yuruntian/SOSNet/raw/master/sosnet-weights/sosnet_32x32_liberty.pth"
urls["hp_a"] = "https://github.com/yuruntian/SOSNet/raw/master/sosnet-weights/sosnet_32x32_hpatches_a.pth"


class SOSNet(PatchNet):
    """
        128-dimensional SOSNet descriptors of 32 x 32 patches ("SOSNet: Second Order Similarity
        Regularization for Local Descriptor Learning").  Input (B, 1, 32, 32) on the GPU, output (B, 128)
        float32.  Eval mode only; ``pretrained=True`` raises (load sosnet_32x32_liberty.pth with
        ``load_state_dict``).
    """

    variant = "sosnet"
    upstream = urls["lib"]

    def __init__(self, pretrained=False):
        super(SOSNet, self).__init__()
        self.layers = nn.Sequential(nn.InstanceNorm2d(1, affine=False), *trunk_layers(0.1))
        self.desc_norm = nn.Sequential(nn.LocalResponseNorm(256, alpha=256, beta=0.5, k=0))
        if pretrained:
            self._refuse_pretrained()

    def _trunk(self):
        return self.layers

    def forward(self, input, eps=1e-10):
        if eps != 1e-10:
            raise NotImplementedError("the head kernel has eps = 1e-10 built in")
        return super(SOSNet, self).forward(input)
