"""Dice losses on the fused HIP kernels; drop-ins for the reference's ``DiceLoss`` (`src/losses/dice_loss.py:7-76`: same
constructor, ``num_classes`` means FOREGROUND classes, ``self.num_classes = num_classes + 1``) and for the nnU-Net family the
fold trainers use: ``MemoryEfficientSoftDiceLoss`` (`dice_loss.py:100-165`) and ``get_tp_fp_fn_tn`` (`dice_loss.py:168-225`).
Every loss returns a 0-dim tensor with autograd."""
from __future__ import annotations

from typing import Callable

import torch
from torch import nn

from mia_hip import ops


class DiceLoss(nn.Module):
    def __init__(self, num_classes: int, smooth: float = 1e-5, do_bg: bool = False, softmax: bool = True,
                 batch: bool = False, squared: bool = False):
        super().__init__()
        self.num_classes = num_classes + 1  # include background (reference dice_loss.py:18)
        self.smooth = smooth
        self.do_bg = do_bg
        self.softmax = softmax
        self.batch = batch
        self.squared = squared

    def _flags(self):
        return ops.loss_flags(self.softmax, self.do_bg, self.batch, self.squared)

    def _check(self, outputs, targets):
        if outputs.ndim != 4:
            raise NotImplementedError("MI355X DiceLoss implements 2-D inputs [B, K, H, W]")
        if targets.shape == outputs.shape and outputs.shape[1] > 1:
            return  # dense (one-hot / soft) target, used as is (reference dice_loss.py:40-41)
        assert outputs.shape[1] == self.num_classes, "inputs {} & num_classes+1 {} do not match".format(
            tuple(outputs.shape), self.num_classes)
        assert targets.numel() == outputs.shape[0] * outputs.shape[2] * outputs.shape[3], \
            "inputs {} & target {} shape do not match".format(outputs.size(), targets.size())

    def forward(self, outputs: torch.Tensor, targets: torch.Tensor):
        self._check(outputs, targets)
        return ops.DiceCEFn.apply(outputs, targets, self._flags(), float(self.smooth), 1.0, 0.0, 0)


def softmax_helper_dim1(x: torch.Tensor) -> torch.Tensor:
    """The one `apply_nonlin` the kernels recognise (by identity): the soft-max then runs inside the fused pass."""
    return torch.softmax(x, 1)


_MASKED = -(1 << 62)  # stands for "loss_mask == 0" in the index labels handed to the kernel; no class and no user label


def _index_labels(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """[B,1,H,W] or [B,H,W] index labels of any integer / float dtype -> [B,H,W]; uint8 stays uint8, the rest becomes int64."""
    if x.ndim != 4:
        raise NotImplementedError("the HIP segmentation losses implement 2-D inputs [B, K, H, W]")
    if y.shape == x.shape and x.shape[1] > 1:
        raise NotImplementedError("one-hot targets are not implemented for the nnU-Net style losses: pass index labels")
    b, _, h, w = x.shape
    if y.numel() != b * h * w:
        raise AssertionError("inputs {} & target {} shape do not match".format(tuple(x.shape), tuple(y.shape)))
    y = y.reshape(b, h, w)
    return y if y.dtype == torch.uint8 else y.long()


class MemoryEfficientSoftDiceLoss(nn.Module):
    """-mean Dice with the denominator clipped at 1e-8 (reference `dice_loss.py:100-165`), on the fused kernel.
    `apply_nonlin` is `softmax_helper_dim1` (soft-max in the kernel) or None (logits used as they are), both with index labels;
    or `torch.sigmoid` with a dense (multi-label) target of the input's shape -- the region-based mode, on the region kernel."""

    def __init__(self, apply_nonlin: Callable | None = None, batch_dice: bool = False, do_bg: bool = True, smooth: float = 1.0):
        super().__init__()
        self.do_bg = do_bg
        self.batch_dice = batch_dice
        self.apply_nonlin = apply_nonlin
        self.smooth = smooth

    def _flags(self) -> int:
        if self.apply_nonlin is not None and self.apply_nonlin is not softmax_helper_dim1:
            raise NotImplementedError("MemoryEfficientSoftDiceLoss on the HIP kernel: apply_nonlin must be "
                                      "losses.compound_losses.softmax_helper_dim1 or None (index labels), or torch.sigmoid with a "
                                      "dense target of the input's shape")
        return ops.seg_loss_flags(self.apply_nonlin is not None, self.do_bg, self.batch_dice)

    def _region_flags(self, x: torch.Tensor) -> int:
        """Checks and kernel flags of the sigmoid (region) mode."""
        if x.ndim != 4:
            raise NotImplementedError("the HIP segmentation losses implement 2-D inputs [B, C, H, W]")
        if x.shape[1] > ops.REGLOSS_MAX_CHANNELS:
            raise NotImplementedError(f"the HIP region loss implements up to {ops.REGLOSS_MAX_CHANNELS} channels, got {x.shape[1]}")
        if x.shape[1] == 1 and not self.do_bg:
            raise ValueError("one output channel with do_bg=False leaves no Dice term")
        return ops.region_loss_flags(self.do_bg, self.batch_dice)

    def _forward_sigmoid(self, x: torch.Tensor, y: torch.Tensor, loss_mask):
        flags = self._region_flags(x)
        ops._need_dev(x, y, loss_mask)
        if loss_mask is not None:  # the kernel's ignore channel is the complement of the mask, in the target's own dtype
            b, _, h, w = x.shape
            if loss_mask.numel() != b * h * w:
                raise AssertionError("inputs {} & loss_mask {} shape do not match".format(tuple(x.shape), tuple(loss_mask.shape)))
            if y.dtype not in (torch.bool, torch.uint8, torch.float32):
                y = y.float()
            y = torch.cat((y, (loss_mask.reshape(b, 1, h, w) == 0).to(y.dtype)), 1)
            flags |= ops.REGLOSS_IGNORE
        return ops.RegionLossFn.apply(x, y, None, None, flags, None, float(self.smooth), 1.0, 0.0, 2)

    def forward(self, x: torch.Tensor, y: torch.Tensor, loss_mask: torch.Tensor | None = None):
        if self.apply_nonlin is torch.sigmoid and y.shape == x.shape:  # equal shapes = dense target, for one channel too
            return self._forward_sigmoid(x, y, loss_mask)
        flags = self._flags()
        lab = _index_labels(x, y)
        ops._need_dev(x, y, loss_mask)
        ign = None
        if loss_mask is not None:
            lab = torch.where(loss_mask.reshape(lab.shape) != 0, lab.long(), _MASKED)
            ign = _MASKED
        return ops.SegLossFn.apply(x, lab, None, flags, ign, float(self.smooth), 1.0, 0.0, 0)


def get_tp_fp_fn_tn(net_output, gt, axes=None, mask=None, square=False):
    """The reference's general function (`dice_loss.py:168-225`) in tensor ops, for CPU and GPU tensors: `net_output`
    [B,C,...] (probabilities or a one-hot prediction), `gt` a label map ([B,1,...] or [B,...]) or a one-hot tensor of
    `net_output`'s shape, `mask` [B,1,...] with 1 = valid.  For the trainers' per-step hard counts use `hard_tp_fp_fn`
    (or the `last_hard_counts` a fused `DC_and_CE_loss` leaves behind), which needs no one-hot tensors."""
    if axes is None:
        axes = tuple(range(2, net_output.ndim))
    with torch.no_grad():
        if net_output.ndim != gt.ndim:
            gt = gt.view((gt.shape[0], 1, *gt.shape[1:]))
        if net_output.shape == gt.shape:
            onehot = gt.bool()
        else:
            onehot = torch.zeros(net_output.shape, device=net_output.device, dtype=torch.bool)
            onehot.scatter_(1, gt.long(), 1)
    tp = net_output * onehot
    fp = net_output * (~onehot)
    fn = (1 - net_output) * onehot
    tn = (1 - net_output) * (~onehot)
    if mask is not None:
        tp, fp, fn, tn = tp * mask, fp * mask, fn * mask, tn * mask  # [B,1,...] broadcasts over the classes
    if square:
        tp, fp, fn, tn = tp ** 2, fp ** 2, fn ** 2, tn ** 2
    axes = tuple(axes)
    if len(axes) > 0:
        tp, fp, fn, tn = (t.sum(dim=axes, keepdim=False) for t in (tp, fp, fn, tn))
    return tp, fp, fn, tn


def hard_tp_fp_fn(logits: torch.Tensor, target: torch.Tensor, ignore_label=None) -> torch.Tensor:
    """int64 [B, K1, 3] = (tp, fp, fn) of `argmax(logits, 1)` against index labels, `ignore_label` pixels left out: what
    `get_tp_fp_fn_tn(onehot(argmax), target, axes=(2, 3), mask=target != ignore_label)` returns, from one kernel pass."""
    ops._need_dev(logits, target)
    return ops.hard_tp_fp_fn(logits, _index_labels(logits, target), ignore_label)
