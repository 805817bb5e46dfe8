"""Deep-supervision loss.  The reference builds the auxiliary heads (`UNet(deep_supervision=True, ds_layer=n)`, unet.py:193-197) but
never trains with them, so this is the project's own definition:

    forward(outputs, target) = sum_i w_i * loss(up_i(outputs[i]), target)

`outputs` is what `UNet.forward(x, return_ds=True, upsample_ds=False)` returns: the main logits followed by the auxiliary heads'
LOW-resolution logits, finest first.  `up_i` is the heads' own `Upsample(scale_factor, mode="bilinear", align_corners=False)`; every
output is supervised at the target's full resolution, so no output is dropped and the default weights are nnU-Net's halving rule
normalised over all of them: w_i = 2^-i / sum_j 2^-j.

An output at the target's resolution goes to `loss` as it is.  A lower-resolution one goes to the fused kernel
(`ops.UpsampleDiceCEFn`: interpolation in registers, the full-resolution logits and their gradient never exist) when `loss` is a
fusable `DiceAndCELoss`, the target holds index labels and the integer factor is one the kernel implements; otherwise it is
upsampled with `ResizeBilinearFn` and handed to `loss`, so `DC_and_CE_loss`, `DC_and_BCE_loss` and dense targets work too."""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import nn

from mia_hip import ops

from .compound_losses import DiceAndCELoss


def default_weights(n: int):
    raw = [2.0 ** -i for i in range(n)]
    return [r / sum(raw) for r in raw]


class DeepSupervisionLoss(nn.Module):
    """loss: any module `loss(logits, target)`.  weights: one per output (default: see the module text).
    fused: None = the fused kernel wherever it can serve, False = always upsample and call `loss`, True = raise where the fused
    kernel cannot serve.  `last_terms`: the per-output loss values of the latest forward, a device tensor (no host sync)."""

    def __init__(self, loss: nn.Module, weights: Optional[Sequence[float]] = None, fused: Optional[bool] = None):
        super().__init__()
        self.loss = loss
        self.weights = None if weights is None else [float(w) for w in weights]
        self.fused = fused
        self.last_terms = None

    def _why_not_fused(self, out: torch.Tensor, target: torch.Tensor, factor: int) -> Optional[str]:
        loss = self.loss
        if not (isinstance(loss, DiceAndCELoss) and loss._fusable()):
            return f"{type(loss).__name__} is not a DiceAndCELoss over DiceLoss + CrossEntropyLoss"
        ce = loss.ce_loss
        if getattr(ce, "weight", None) is not None or ce.label_smoothing != 0.0 or ce.reduction != "mean":
            return "the cross-entropy term has class weights, label smoothing or a reduction other than 'mean'"
        b, k1 = out.shape[0], out.shape[1]
        if target.numel() != b * target.shape[-2] * target.shape[-1]:
            return f"the target {tuple(target.shape)} is dense, the fused kernel takes index labels"
        if factor not in ops.DS_LOSS_FACTORS:
            return f"factor {factor} is not one of {ops.DS_LOSS_FACTORS}"
        if k1 > ops.DS_LOSS_MAX_CLASSES:
            return f"{k1} classes, the fused kernel implements up to {ops.DS_LOSS_MAX_CLASSES}"
        return None

    def _factor(self, out: torch.Tensor, target: torch.Tensor) -> int:
        """1 for an output at the target's resolution, else the integer upsampling factor; ValueError for anything else."""
        if out.ndim != 4 or target.ndim < 3:
            raise ValueError(f"DeepSupervisionLoss: outputs are [B,K,h,w] and the target ends in [H,W]; got {tuple(out.shape)} and "
                             f"{tuple(target.shape)}")
        (h, w), (H, W) = out.shape[-2:], target.shape[-2:]
        if H % h or W % w or H // h != W // w:
            raise ValueError(f"DeepSupervisionLoss: an output of {h}x{w} pixels does not divide the target's {H}x{W} by one integer "
                             f"factor (output {tuple(out.shape)}, target {tuple(target.shape)})")
        factor = H // h
        if factor > 1 and self.fused:
            why = self._why_not_fused(out, target, factor)
            if why is not None:
                raise ValueError(f"DeepSupervisionLoss(fused=True): {why}")
        return factor

    def _term(self, out: torch.Tensor, target: torch.Tensor, factor: int) -> torch.Tensor:
        if factor == 1:
            return self.loss(out, target)
        if self.fused is not False and self._why_not_fused(out, target, factor) is None:
            loss = self.loss
            d = loss.dice_loss
            assert out.shape[1] == d.num_classes, "inputs {} & num_classes+1 {} do not match".format(tuple(out.shape), d.num_classes)
            return ops.UpsampleDiceCEFn.apply(out, target, factor, d._flags(), float(d.smooth), float(loss.default_dice_weight),
                                              float(loss.default_ce_weight), 0)
        ops._need_dev(out, target)
        from transforms.hip.functional_hip import ResizeBilinearFn
        return self.loss(ResizeBilinearFn.apply(out, target.shape[-2], target.shape[-1]), target)

    def forward(self, outputs, target: torch.Tensor) -> torch.Tensor:
        if isinstance(outputs, torch.Tensor):
            return self.loss(outputs, target)
        outputs = list(outputs)
        weights = default_weights(len(outputs)) if self.weights is None else self.weights
        if len(weights) != len(outputs):
            raise ValueError(f"DeepSupervisionLoss: {len(weights)} weights for {len(outputs)} outputs")
        factors = [self._factor(o, target) for o in outputs]  # every shape is checked before anything runs
        terms = [self._term(o, target, f) for o, f in zip(outputs, factors)]
        total = terms[0] * weights[0]
        for t, w in zip(terms[1:], weights[1:]):
            total = total + t * w
        self.last_terms = torch.stack([t.detach() for t in terms])
        return total
