"""Dice + CE compound losses, one fused HIP pass each; drop-ins for the reference's ``DiceAndCELoss``
(`src/losses/compound_losses.py:17-65`), for the fold trainers' ``DC_and_CE_loss`` (`compound_losses.py:129-196`), for the
region-based ``DC_and_BCE_loss`` (`compound_losses.py:178-233`) and for ``DC_and_topk_loss`` (`compound_losses.py:236-301`)."""
from __future__ import annotations

from typing import Callable

import torch
from torch import nn

from mia_hip import ops

from .ce_loss import RobustCrossEntropyLoss, TopKLoss, _check_ce_config, hip_cross_entropy
from .dice_loss import DiceLoss, MemoryEfficientSoftDiceLoss, _index_labels, softmax_helper_dim1  # noqa: F401  (re-exported)
from .regions import check_regions, expand_regions


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


class DC_and_BCE_loss(nn.Module):
    """weight_ce * BCEWithLogitsLoss + weight_dice * MemoryEfficientSoftDiceLoss(sigmoid): nnU-Net's *region-based* mode
    (reference `compound_losses.py:178-233`).  The network has one sigmoid output per region and regions may overlap; the target
    is a multi-label mask [B,C,H,W] in bool, uint8 or float (handed to the kernel as it is, never converted), or [B,C+1,H,W] with
    `use_ignore_label`, where the last channel marks the pixels that both terms leave out.  With the project's Dice class the
    whole loss is ONE forward pass and ONE backward pass over the logits.

    The BCE term keeps the reference's two normalisations: the mean over every element without the ignore channel; with it the
    sum over the valid pixels and all C channels divided by the number of valid *pixels* (the reference's mask broadcasts over the
    channels), clipped at 1e-8.  `bce_kwargs`: nothing, or a `pos_weight` of C values shaped [C,1,1] or [1,C,1,1].

    This build's addition (keyword-only): `regions=((1, 2), (1,))`, one tuple of labels per output channel, makes `forward` take
    index labels [B,1,H,W] or [B,H,W] (uint8 stays uint8) instead and run the kernel's index form, which reads one label per
    pixel instead of C (+1) mask values; `ignore_label=` names the label to leave out.  It computes, bit for bit, what the dense
    form computes on `losses.regions.expand_regions(labels, regions, ignore_label)`.

    By-products of the latest forward, device tensors: `last_ce`, `last_dc` (0-dim) and `last_hard_counts` (int64 [B,C,3]: tp, fp,
    fn of `logit > 0` against `target > 0.5` over the valid pixels, the online region Dice)."""

    def __init__(self, bce_kwargs, soft_dice_kwargs, weight_ce=1, weight_dice=1, use_ignore_label: bool = False,
                 dice_class=MemoryEfficientSoftDiceLoss, *, regions=None, ignore_label=None):
        super().__init__()
        if use_ignore_label:
            bce_kwargs["reduction"] = "none"
        self.weight_dice = weight_dice
        self.weight_ce = weight_ce
        self.use_ignore_label = use_ignore_label
        self.ce = nn.BCEWithLogitsLoss(**bce_kwargs)
        self.dc = dice_class(apply_nonlin=torch.sigmoid, **soft_dice_kwargs)
        self.regions = None if regions is None else check_regions(regions)
        self.ignore_label = ignore_label
        if ignore_label is not None and regions is None:
            raise ValueError("DC_and_BCE_loss: `ignore_label` belongs to the index form; pass `regions` too, or mark ignored pixels "
                             "in the last target channel with use_ignore_label=True")
        if regions is not None and use_ignore_label != (ignore_label is not None):
            raise ValueError("DC_and_BCE_loss: with `regions`, use_ignore_label and `ignore_label` go together")
        self._bits = None
        self.last_ce = self.last_dc = self.last_hard_counts = None

    def _check_bce(self, c: int):
        """The supported BCE configuration; returns pos_weight as C values or None."""
        if self.ce.weight is not None:
            raise NotImplementedError("DC_and_BCE_loss on the HIP kernel: BCE `weight` is not implemented")
        if self.ce.reduction != ("none" if self.use_ignore_label else "mean"):
            raise NotImplementedError("DC_and_BCE_loss on the HIP kernel: reduction='mean' only (the ignore channel sets 'none')")
        pw = self.ce.pos_weight
        if pw is None:
            return None
        if pw.numel() != c or tuple(pw.shape) not in ((c, 1, 1), (1, c, 1, 1)):
            raise NotImplementedError(f"DC_and_BCE_loss on the HIP kernel: pos_weight must hold one value per channel, shaped "
                                      f"[{c},1,1] or [1,{c},1,1]; got {tuple(pw.shape)}")
        return pw.reshape(c)

    def forward(self, net_output: torch.Tensor, target: torch.Tensor):
        if type(self.dc) is MemoryEfficientSoftDiceLoss:
            flags = self.dc._region_flags(net_output)
            pw = self._check_bce(net_output.shape[1])
            ops._need_dev(net_output, target)
            bits = None
            if self.regions is not None:
                if len(self.regions) != net_output.shape[1]:
                    raise ValueError(f"{len(self.regions)} regions for {net_output.shape[1]} output channels")
                if self._bits is None or self._bits.device != net_output.device:
                    self._bits = ops.region_bits(self.regions, net_output.device)
                bits = self._bits
                b, _, h, w = net_output.shape
                if target.numel() != b * h * w:
                    raise AssertionError("with `regions` the target is a label map [B,1,H,W] or [B,H,W]; got {} for inputs {}".format(
                        tuple(target.shape), tuple(net_output.shape)))
                target = target.reshape(b, h, w)
                if target.dtype != torch.uint8:
                    target = target.long()
            elif self.use_ignore_label:
                flags |= ops.REGLOSS_IGNORE
            loss = ops.RegionLossFn.apply(net_output, target, bits, pw, flags, self.ignore_label, float(self.dc.smooth),
                                          float(self.weight_dice), float(self.weight_ce), 0)
            self.last_ce, self.last_dc = ops.RegionLossFn.last_out[1], ops.RegionLossFn.last_out[2]
            self.last_hard_counts = ops.RegionLossFn.last_counts
            return loss
        # a foreign Dice class: the reference's composition in tensor ops
        if self.regions is not None:
            target = expand_regions(target, self.regions, self.ignore_label)
        if self.use_ignore_label:
            mask = ~target[:, -1:] if target.dtype == torch.bool else (1 - target[:, -1:]).bool()
            target_regions = target[:, :-1]
        else:
            target_regions, mask = target, None
        dc_loss = self.dc(net_output, target_regions, loss_mask=mask)
        target_regions = target_regions.to(net_output.dtype)  # `.float()` in the reference, whose logits are fp32
        if mask is not None:
            ce_loss = (self.ce(net_output, target_regions) * mask).sum() / torch.clip(mask.sum(), min=1e-8)
        else:
            ce_loss = self.ce(net_output, target_regions)
        return self.weight_ce * ce_loss + self.weight_dice * dc_loss


class DC_and_topk_loss(nn.Module):
    """weight_ce * TopKLoss + weight_dice * soft Dice on the soft-max, with an optional `ignore_label` that masks pixels out of
    the Dice term and counts as zero loss in the top-k term (reference `compound_losses.py:236-301`: same signature, same
    `forward`).  The reference's own class cannot be constructed -- it names a `SoftDiceLoss` that its module never defines and
    raises `NameError` -- so the Dice term here is `MemoryEfficientSoftDiceLoss`, which is algebraically nnU-Net's `SoftDiceLoss`
    (2 tp / (2 tp + fp + fn) with 2 tp + fp + fn = sum(p) + sum(t)).  A composition of the two existing kernels (`TopKCEFn`,
    `SegLossFn`): one top-k pass plus one Dice pass, no kernel of its own."""

    def __init__(self, soft_dice_kwargs, ce_kwargs, weight_ce=1, weight_dice=1, ignore_label=None):
        super().__init__()
        if ignore_label is not None:
            ce_kwargs["ignore_index"] = ignore_label
        self.weight_dice = weight_dice
        self.weight_ce = weight_ce
        self.ignore_label = ignore_label
        self.ce = TopKLoss(**ce_kwargs)
        self.dc = MemoryEfficientSoftDiceLoss(apply_nonlin=softmax_helper_dim1, **soft_dice_kwargs)

    def forward(self, net_output: torch.Tensor, target: torch.Tensor):
        mask = None
        target_dice = target
        if self.ignore_label is not None:
            assert target.shape[1] == 1, "ignore label is not implemented for one hot encoded target variables (DC_and_topk_loss)"
            mask = target != self.ignore_label
            target_dice = torch.where(mask, target, 0)
        dc_loss = self.dc(net_output, target_dice, loss_mask=mask) if self.weight_dice != 0 else 0
        # an all-ignored batch gives a top-k term of exactly 0 on the device, where the reference tests `num_fg > 0` on the host
        ce_loss = self.ce(net_output, target) if self.weight_ce != 0 else 0
        return self.weight_ce * ce_loss + self.weight_dice * dc_loss
