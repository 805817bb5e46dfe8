"""The UNet with a second 1x1 head for dual-task consistency training (DTC: Luo et al., AAAI 2021; `losses/dual_task.py`,
`training.semi.DTCEngine`).  The reference has no such model; this is the project's own addition on top of its drop-in `UNet`.
"""
from __future__ import annotations

import torch.nn as nn

from mia_hip import ops

from .unet import UNet, conv_dict


class DualTaskUNet(UNet):
    """`UNet` plus `decoder.ls_output = Conv2d(channels_list[0], output_classes - 1, 1)`: the level-set head, one channel per
    foreground class (channel c belongs to class c + 1), on the same last decoder activation as `decoder.seg_output`.

    The head is created AFTER `UNet.__init__`, so under one `torch.manual_seed` every shared parameter has the bits of a `UNet`
    built with the same arguments, and `UNet`'s `state_dict` keys are unchanged: a `UNet` loads this model's shared weights with
    `strict=False`, and this model loads a `UNet` checkpoint the same way.

    `forward(x)` is `UNet.forward`: the segmentation logits through the fused last-block + head node, bit-identical to a `UNet` with
    the same weights.  `forward(x, return_level_set=True)` returns `(z, r)`: both heads as `ops.HeadFn` on the last decoder
    activation (the un-fused decoder path), `z` `[B, K, H, W]` and `r` `[B, K - 1, H, W]` (the level-set LOGITS: the loss applies
    `tanh`), fp32 logical-NCHW views with channels-last strides.  2-D; no deep supervision together with `return_level_set`."""

    def __init__(self, dimension, input_channels, output_classes, channels_list, **kwargs):
        super().__init__(dimension, input_channels, output_classes, channels_list, **kwargs)
        if output_classes < 2:
            raise ValueError("DualTaskUNet: a level-set head needs at least one foreground class (output_classes >= 2)")
        self.decoder.ls_output = conv_dict[dimension](channels_list[0], output_classes - 1, kernel_size=1, stride=1)

    def forward(self, x, return_ds=False, upsample_ds=True, return_level_set=False):
        if not return_level_set:
            return super().forward(x, return_ds=return_ds, upsample_ds=upsample_ds)
        if return_ds:
            raise NotImplementedError("DualTaskUNet: return_level_set does not combine with return_ds")
        ops._COLSUM_HINT.clear()  # as UNet.forward: hints are only valid inside the backward pass of the forward that produced them
        ops._ACC_HINT.clear()
        ops._CR_HINT.clear()
        self._draw_dropout(x.shape[0], x.device)
        z, feat, _, _ = self.decoder._run(self._skips(x), False, fuse_head=False)
        head = self.decoder.ls_output
        return z, ops.HeadFn.apply(feat, head.weight, head.bias)
