"""The reference's HardNet (``cirtorch/features/hardnet.py``) on the engine's fused kernels.

Same name, constructor and submodule structure (``features.0 .. features.20``), so an upstream
checkpoint's ``state_dict`` loads with ``strict=True``.  The forward pass is rr_patchnet_describe:
per-patch ``(x - mean) / (std + 1e-6)``, the trunk in fp16 with float32 accumulation, ``F.normalize``.
"""

import torch.nn as nn

from .patchnet import PatchNet, trunk_layers

urls = dict()
urls["hardnet++"] = "https://github.com/DagnyT/hardnet/raw/master/pretrained/pretrained_all_datasets/HardNet++.pth"
urls["liberty_aug"] = "https://github.com/DagnyT/hardnet/raw/master/pretrained/train_liberty_with_aug/checkpoint_liberty_with_aug.pth"  # noqa


class HardNet(PatchNet):
    """
        HardNet descriptors of grayscale 32 x 32 patches ("Working hard to know your neighbor's margins:
        Local descriptor learning loss").  Input (B, 1, 32, 32) on the GPU, output (B, 128) float32,
        L2-normalised.  Eval mode only; ``pretrained=True`` raises (load the ``state_dict`` entry of
        checkpoint_liberty_with_aug.pth with ``load_state_dict``).
    """

    variant = "hardnet"
    upstream = urls["liberty_aug"]

    def __init__(self, pretrained=False):
        super(HardNet, self).__init__()
        self.features = nn.Sequential(*trunk_layers(0.3))
        if pretrained:
            self._refuse_pretrained()

    def _trunk(self):
        return self.features
