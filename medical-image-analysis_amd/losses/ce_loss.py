"""Cross-entropy losses on the HIP kernels (reference `src/losses/ce_loss.py`): `RobustCrossEntropyLoss` and `TopKLoss`."""
from __future__ import annotations

import torch
from torch import Tensor, nn

from mia_hip import ops


class RobustCrossEntropyLoss(nn.CrossEntropyLoss):
    """Accepts a [B,1,H,W] (possibly float) target like the reference.  The default configuration is the mean over all pixels
    on the fused Dice/CE kernel; class weights and / or an `ignore_index` run on the fold-trainer kernel with torch's
    definition of the mean (sum of w[label] * nll over the kept pixels / sum of w[label]).  Label smoothing and other
    reductions are not implemented."""

    def forward(self, input: Tensor, target: Tensor) -> Tensor:
        if target.ndim == input.ndim:
            assert target.shape[1] == 1
            target = target[:, 0]
        if self.weight is None and self.ignore_index == -100:
            return hip_cross_entropy(self, input, target)
        _check_ce_config(self)
        ops._need_dev(input, target)
        return ops.SegLossFn.apply(input, target, self.weight, ops.seg_loss_flags(True, True, False), self.ignore_index, 1.0, 0.0,
                                   1.0, 0)


def _check_ce_config(module) -> None:
    if getattr(module, "label_smoothing", 0.0) != 0.0 or getattr(module, "reduction", "mean") != "mean":
        raise NotImplementedError("HIP cross-entropy: no label smoothing, reduction='mean'")


class TopKLoss(RobustCrossEntropyLoss):
    """Mean of the hardest k % of the per-pixel cross-entropy (reference `ce_loss.py:18-32`); ignored pixels count as zeros
    among the N pixels, as there.  The threshold comes from a radix select on the device instead of `torch.topk`'s sort.
    Where several pixels tie EXACTLY with the threshold, `torch.topk`'s choice among them is unspecified; here they share
    the remaining slots equally (value unchanged, gradient split evenly) -- this project's own deterministic rule."""

    def __init__(self, weight=None, ignore_index: int = -100, k: float = 10, label_smoothing: float = 0):
        self.k = k
        super().__init__(weight, ignore_index=ignore_index, reduction="none", label_smoothing=label_smoothing)

    def forward(self, input: Tensor, target: Tensor) -> Tensor:
        if self.label_smoothing != 0.0:
            raise NotImplementedError("HIP top-k cross-entropy: no label smoothing")
        if input.ndim != 4:
            raise NotImplementedError("the HIP segmentation losses implement 2-D inputs [B, K, H, W]")
        ops._need_dev(input, target)
        return ops.TopKCEFn.apply(input, target[:, 0], self.weight, self.ignore_index, self.k)


def hip_cross_entropy(module, input: Tensor, target: Tensor) -> Tensor:
    if getattr(module, "weight", None) is not None or getattr(module, "label_smoothing", 0.0) != 0.0 or \
            getattr(module, "reduction", "mean") != "mean":
        raise NotImplementedError("HIP cross-entropy implements the al_train configuration: no class weights, "
                                  "no label smoothing, reduction='mean'")
    ign = getattr(module, "ignore_index", -100)
    if 0 <= ign < input.shape[1]:
        raise NotImplementedError("HIP cross-entropy has no ignore_index: every label must be a class in [0, K1)")
    # the default ignore_index (-100) is not honoured either: such a label is out of range -> NaN loss, ops.check_labels() raises
    if target.shape != input.shape:
        target = target.long()
    return ops.DiceCEFn.apply(input, target, ops.loss_flags(True, True, False, False), 1e-5, 0.0, 1.0, 0)
