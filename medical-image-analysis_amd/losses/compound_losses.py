"""Dice + CE compound losses, one fused HIP pass each; drop-ins for the reference's ``DiceAndCELoss``
(`src/losses/compound_losses.py:17-65`) and for the fold trainers' ``DC_and_CE_loss`` (`compound_losses.py:129-196`)."""
from __future__ import annotations

from typing import Callable

import torch
from torch import nn

from mia_hip import ops

from .ce_loss import RobustCrossEntropyLoss, _check_ce_config, hip_cross_entropy
from .dice_loss import DiceLoss, MemoryEfficientSoftDiceLoss, _index_labels, softmax_helper_dim1  # noqa: F401  (re-exported)


class DiceAndCELoss(nn.Module):
    def __init__(self, dice_loss: Callable = DiceLoss, dice_kwargs: dict = {}, ce_loss: Callable = RobustCrossEntropyLoss,
                 ce_kwargs: dict = {}, default_dice_weight: float = 1.0, default_ce_weight: float = 1.0):
        super().__init__()
        self.dice_loss = dice_loss(**dice_kwargs)
        self.ce_loss = ce_loss(**ce_kwargs)
        self.default_dice_weight = default_dice_weight
        self.default_ce_weight = default_ce_weight

    def _fusable(self):
        return isinstance(self.dice_loss, DiceLoss) and isinstance(self.ce_loss, nn.CrossEntropyLoss)

    def forward(self, outputs: torch.Tensor, targets: torch.Tensor, dice_weight: float | None = None,
                ce_weight: float | None = None):
        if not dice_weight:  # reference quirk: 0.0 / None -> default (compound_losses.py:40-44)
            dice_weight = self.default_dice_weight
        if not ce_weight:
            ce_weight = self.default_ce_weight
        if self._fusable():
            d = self.dice_loss
            d._check(outputs, targets)
            if getattr(self.ce_loss, "weight", None) is not None or self.ce_loss.label_smoothing != 0.0 or \
                    self.ce_loss.reduction != "mean":
                raise NotImplementedError("HIP cross-entropy implements the al_train configuration only")
            return ops.DiceCEFn.apply(outputs, targets, d._flags(), float(d.smooth), float(dice_weight), float(ce_weight), 0)
        return ce_weight * self.get_ce_loss(outputs, targets) + dice_weight * self.dice_loss(outputs, targets)

    def get_dice_loss(self, outputs: torch.Tensor, targets: torch.Tensor):
        return self.dice_loss(outputs, targets)

    def get_ce_loss(self, outputs: torch.Tensor, targets: torch.Tensor):
        if isinstance(self.ce_loss, nn.CrossEntropyLoss):
            if targets.ndim == outputs.ndim and targets.shape[1] == 1 and outputs.shape[1] > 1:
                targets = targets[:, 0]
            return hip_cross_entropy(self.ce_loss, outputs, targets)
        return self.ce_loss(outputs, targets)


class DC_and_CE_loss(nn.Module):
    """weight_ce * RobustCrossEntropyLoss + weight_dice * MemoryEfficientSoftDiceLoss with an optional `ignore_label` that
    masks pixels out of both terms (reference `compound_losses.py:129-196`).  With the project's Dice class the whole loss is
    ONE forward pass and ONE backward pass over the logits; a weight of 0 drops that term as the reference does, and a batch
    with no valid pixel drops the CE term on the device (the reference tests `num_fg > 0` on the host).  By-products of the
    latest forward, device tensors: `last_ce`, `last_dc` (0-dim) and `last_hard_counts` (int64 [B,K1,3]: tp, fp, fn of the
    arg-max prediction over the valid pixels, the trainers' online Dice)."""

    def __init__(self, soft_dice_kwargs, ce_kwargs, weight_ce=1, weight_dice=1, ignore_label=None,
                 dice_class=MemoryEfficientSoftDiceLoss):
        super().__init__()
        if ignore_label is not None:
            ce_kwargs["ignore_index"] = ignore_label
        self.weight_dice = weight_dice
        self.weight_ce = weight_ce
        self.ignore_label = ignore_label
        self.ce = RobustCrossEntropyLoss(**ce_kwargs)
        self.dc = dice_class(apply_nonlin=softmax_helper_dim1, **soft_dice_kwargs)
        self.last_ce = self.last_dc = self.last_hard_counts = None

    def forward(self, net_output: torch.Tensor, target: torch.Tensor):
        if self.ignore_label is not None:
            assert target.ndim == net_output.ndim and target.shape[1] == 1, \
                "ignore label is not implemented for one hot encoded target variables (DC_and_CE_loss)"
        if type(self.dc) is MemoryEfficientSoftDiceLoss:
            _check_ce_config(self.ce)
            if self.ignore_label is None and self.ce.ignore_index != -100:
                raise NotImplementedError("DC_and_CE_loss: pass the ignore label as `ignore_label`, which masks both terms")
            labels = _index_labels(net_output, target)
            ops._need_dev(net_output, target)
            loss = ops.SegLossFn.apply(net_output, labels, self.ce.weight, self.dc._flags(),
                                       self.ignore_label, float(self.dc.smooth), float(self.weight_dice), float(self.weight_ce), 0)
            self.last_ce, self.last_dc = ops.SegLossFn.last_out[1], ops.SegLossFn.last_out[2]
            self.last_hard_counts = ops.SegLossFn.last_counts
            return loss
        # a foreign Dice class: the reference's composition, the CE term still on the kernel (0 when nothing is valid)
        mask = None
        target_dice = target
        if self.ignore_label is not None:
            mask = target != self.ignore_label
            target_dice = torch.where(mask, target, 0)
        dc_loss = self.dc(net_output, target_dice, loss_mask=mask) if self.weight_dice != 0 else 0
        ce_loss = self.ce(net_output, target[:, 0] if target.ndim == net_output.ndim else target) if self.weight_ce != 0 else 0
        return self.weight_ce * ce_loss + self.weight_dice * dc_loss
