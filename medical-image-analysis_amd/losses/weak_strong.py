"""Weak-to-strong consistency (FixMatch: Sohn et al., NeurIPS 2020; UniMatch: Yang et al., CVPR 2023) and the CutMix form of cross
pseudo supervision (Chen et al., CVPR 2021) on the HIP kernels of `csrc/w2s.hip`: the pseudo-label code of a weak view, the CutMix
boxes, and the loss of a strong view whose pseudo-labels come from ANOTHER image of the batch wherever a CutMix box covers the pixel.
The reference has no such module; like `cross_pseudo.py` and `copy_paste.py` this is the project's own addition, and THIS TEXT is the
definition the kernels and the tests follow.

Code.  For weak logits `zw` `[B, K, H, W]` and a threshold `tau`, per pixel `y = argmax_k zw_k` on the logits as given (a tie goes to
the lowest class), `keep = [max_k softmax(zw)_k >= tau]`, `code = y | keep << 7`: one byte.  `mia_hip.ops.w2s_labels(zw, dyn)` reads
`tau = dyn[1]` on the device; `pseudo_label_code(zw, tau)` is the same in tensor ops.

Boxes.  `random_cutmix_boxes` draws, per image, whether CutMix fires (probability `p`), an area as a share of the image uniform in
`size`, an aspect `height / width` uniform in `ratio` (UniMatch's `obtain_cutmix_box`) and a position uniform over those that keep the
box inside the image; `box_masks` turns the boxes into a uint8 `[B, H, W]` mask with 1 inside.  Where the published code redraws until
the box fits, the aspect is drawn from the part of `ratio` for which a box of that area fits (the nearest fitting aspect if there is
none), so the number of draws is fixed: five per image, all on the host.

Mix.  `mia_hip.ops.cutmix_perm(x, perm, mask)` is `mask != 0 ? x[perm[n]] : x[n]` per pixel, every channel alike: a selection.

Loss.  Strong logits `zs` are `[B, K, H, W]`, `K = num_classes + 1 <= 8` for the kernels, `code` is the byte map above `[B, H, W]`,
`mask` uint8 `[H, W]` or `[B, H, W]`, `perm` `B` integers in `[0, B)`; `mask` or `perm` None means no mix (plain FixMatch).  For pixel
`(n, p)`: `src = mask[n][p] ? perm[n] : n`, `c = code[src][p]`, `y = c & 7`, `m = c >> 7` (a label `>= K` counts as not kept),
`q = softmax(zs)`, `N = B * H * W`, and over ALL images and pixels of the call

* `CE  = (1/N) sum m (logsumexp(zs) - zs[y])` -- the denominator is always N (the CPS convention here): no kept pixel gives 0;
* `I_k = sum m q_k [y = k]`, `Z_k = sum m q_k^2`, `Y_k = sum m [y = k]` (exact integers);
* `D   = (1/K) sum_k (1 - (2 I_k + s) / (Z_k + Y_k + s))`, `s = smooth`: the squared-denominator Dice of `copy_paste.py`, every class
  counts; no kept pixel gives 0;
* `L   = weight * (ce_weight * CE + dice_weight * D)`, `weight = dyn[0]` read on the device (`dyn` None: 1).

The gradient for a pixel is `dL/dzs_j = m [ cec (q_j - [j = y]) + q_j (g_j - sum_k g_k q_k) ]` with `cec = weight ce_weight / N`,
`g_k = al_k [y = k] + be_k q_k`, `al_k = -2 weight dice_weight / (K den_k)`, `be_k = 2 weight dice_weight (2 I_k + s) / (K den_k^2)`,
`den_k = Z_k + Y_k + s`; a pixel with `m = 0` gets exactly 0, and the code, the mask and `perm` carry no gradient.

By-products: `counts = {sum m over the mixed view, pixels whose mask byte is set}` as exact integers; the second is 0 without a mix
and counts a pixel also where `perm[n] = n`.

From tensor ops one strong view costs a soft-max, a max, an arg-max, two gathers by permutation, two `where`s, a masked CE map and a
masked Dice; the fused form is one streaming pass over the strong logits each way, reads one or two code bytes per pixel and keeps
nothing of the logits' size but the gradient.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import nn

from mia_hip import MiaError, ops


def pseudo_label_code(zw: torch.Tensor, tau=0.0) -> torch.Tensor:
    """uint8 `[B, H, W]`: `argmax_k zw_k | [max_k softmax(zw)_k >= tau] << 7` in tensor ops, in the dtype and on the device of `zw`
    (`torch.argmax` returns the first of equal maxima); at most 128 classes.  `tau` is a number or a 0-dim tensor."""
    if zw.ndim != 4 or zw.shape[1] > 128:
        raise ValueError(f"pseudo_label_code: logits [B, K <= 128, H, W] expected, got {tuple(zw.shape)}")
    zw = zw.detach()
    keep = torch.softmax(zw, 1).max(1).values >= tau
    return (zw.argmax(1) | (keep.to(torch.int64) << 7)).to(torch.uint8)


def random_cutmix_boxes(nb: int, h: int, w: int, p: float = 0.5, size=(0.02, 0.4), ratio=(0.3, 1 / 0.3),
                        generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """int64 `[nb, 4]` CPU tensor of boxes `(y0, x0, y1, x1)`, ends exclusive; `(0, 0, 0, 0)` is the empty box of an image where
    CutMix does not fire (or whose box rounds to no pixel).  One `torch.rand(nb, 5)` on the host (the CPU generator, `generator` or
    the default one): `torch.manual_seed` reproduces the boxes, nothing waits for the device, and `p` does not change the number of
    draws.  Per image: fire = `u0 < p`; area `a = (size[0] + u1 (size[1] - size[0])) h w`; aspect `r` uniform in the part of `ratio`
    where `a / w^2 <= r <= h^2 / a` (the box fits); height `int(sqrt(a r))`, width `int(sqrt(a / r))`; corner uniform over the
    positions that keep the box inside."""
    nb, h, w = int(nb), int(h), int(w)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"random_cutmix_boxes: p={p} not in [0, 1]")
    if not 0.0 < size[0] <= size[1] <= 1.0:
        raise ValueError(f"random_cutmix_boxes: size={tuple(size)} must satisfy 0 < size[0] <= size[1] <= 1")
    if not 0.0 < ratio[0] <= ratio[1]:
        raise ValueError(f"random_cutmix_boxes: ratio={tuple(ratio)} must satisfy 0 < ratio[0] <= ratio[1]")
    if nb < 0 or h < 1 or w < 1:
        raise ValueError(f"random_cutmix_boxes: nb={nb} h={h} w={w}")
    u = torch.rand(nb, 5, generator=generator, dtype=torch.float64).tolist()
    boxes = torch.zeros((nb, 4), dtype=torch.int64)
    for n, (u0, u1, u2, u3, u4) in enumerate(u):
        if not u0 < p:
            continue
        a = (size[0] + u1 * (size[1] - size[0])) * h * w
        fit_lo, fit_hi = a / (w * w), h * h / a  # the aspects at which a box of area a fits: fit_lo <= fit_hi since a <= h w
        lo, hi = max(ratio[0], fit_lo), min(ratio[1], fit_hi)
        if lo > hi:  # no aspect of the range fits: the nearest one that does
            lo = hi = fit_lo if ratio[1] < fit_lo else fit_hi
        r = lo + u2 * (hi - lo)
        bh, bw = min(int(math.sqrt(a * r)), h), min(int(math.sqrt(a / r)), w)
        if bh < 1 or bw < 1:
            continue
        y0, x0 = min(int(u3 * (h - bh + 1)), h - bh), min(int(u4 * (w - bw + 1)), w - bw)
        boxes[n] = torch.tensor([y0, x0, y0 + bh, x0 + bw])
    return boxes


def box_masks(boxes: torch.Tensor, h: int, w: int, device="cuda") -> torch.Tensor:
    """uint8 `[nb, h, w]` on `device`: 1 inside box n `(y0, x0, y1, x1)`, 0 outside.  The boxes are uploaded once and compared with
    the pixel coordinates there: no host sync."""
    b = torch.as_tensor(boxes).reshape(-1, 4).to(device=device, dtype=torch.int64, non_blocking=True)
    ys = torch.arange(int(h), device=device)[None, :, None]
    xs = torch.arange(int(w), device=device)[None, None, :]
    y0, x0, y1, x1 = (b[:, i, None, None] for i in range(4))
    return ((ys >= y0) & (ys < y1) & (xs >= x0) & (xs < x1)).to(torch.uint8)


def weak_to_strong_tensor_ops(logits, code, mask=None, perm=None, weight=1.0, ce_weight=1.0, dice_weight=0.0, smooth=1e-10):
    """The definition in tensor ops, in the logits' dtype and on their device (CPU included): `(L, terms [2] = {CE, D}, counts int64
    [2])`.  Differentiable in `logits`; any class count up to 128 (with more than 8 classes the label is the seven low bits of the
    code, as `pseudo_label_code` writes it).  `weight` is a number or a 0-dim tensor (`dyn[0]`)."""
    b, k, h, w = logits.shape
    dev = logits.device
    c = code.reshape(b, h, w).to(torch.int64)
    pasted = torch.zeros((), dtype=torch.int64, device=dev)
    if mask is not None and perm is not None:
        m = (mask != 0).expand(b, h, w) if mask.ndim == 3 else (mask != 0)[None].expand(b, h, w)
        c = torch.where(m, c[torch.as_tensor(perm, device=dev).to(torch.int64)], c)
        pasted = m.sum()
    y = c & 127 if k > 8 else c & 7
    keep = ((c >> 7) & 1).bool() & (y < k)
    mf = keep.to(logits.dtype)
    onehot = (y[:, None] == torch.arange(k, device=dev)[None, :, None, None]).to(logits.dtype)
    lse = torch.logsumexp(logits, 1)
    q = torch.exp(logits - lse[:, None])
    nll = lse - (logits * onehot).sum(1)
    ce = (mf * nll).sum() / float(b * h * w)
    mk = mf[:, None]
    inter = (mk * q * onehot).sum((0, 2, 3))
    z = (mk * q * q).sum((0, 2, 3))
    yk = (mk * onehot).sum((0, 2, 3))
    dice = (1.0 - (2.0 * inter + smooth) / (z + yk + smooth)).mean()
    dice = torch.where(keep.any(), dice, torch.zeros_like(dice))
    loss = weight * (ce_weight * ce + dice_weight * dice)
    return loss, torch.stack([ce.detach(), dice.detach()]), torch.stack([keep.sum(), pasted]).to(torch.int64)


class WeakToStrongLoss(nn.Module):
    """`forward(logits_strong, code, mask=None, perm=None, *, dyn=None)` -> `L` of the module text (0-dim tensor); only the logits
    receive a gradient.  `num_classes` counts foreground classes like `DiceLoss`; logits are `[B, num_classes + 1, H, W]` in any
    layout whose H and W collapse; `code` uint8 `[B, H, W]` (`mia_hip.ops.w2s_labels` or `pseudo_label_code`); `mask` uint8 `[H, W]`
    or `[B, H, W]`; `perm` B integers (host sequence, CPU tensor, or a device int32 tensor taken as it is); `dyn` None or the device
    fp32 `{weight, threshold}` of the engines, of which the loss reads the weight.  `fused=True`: the fp32 kernels of csrc/w2s.hip,
    at most 8 classes with background (more raise `MiaError`), device tensors only.  `fused=False`: the tensor-op form of the same
    definition, which also serves more classes, other dtypes and CPU tensors.  By-products of the latest forward, no host sync:
    `last_ce`, `last_dice` (unweighted), `last_kept`, `last_pasted` (int64).  2-D only."""

    def __init__(self, num_classes: int, ce_weight: float = 1.0, dice_weight: float = 0.0, smooth: float = 1e-10, fused: bool = True):
        super().__init__()
        self.num_classes = num_classes + 1  # include background, like DiceLoss
        self.ce_weight, self.dice_weight, self.smooth, self.fused = float(ce_weight), float(dice_weight), float(smooth), bool(fused)
        if self.num_classes < 1 or (self.fused and self.num_classes > ops.W2S_MAX_CLASSES):
            raise MiaError(f"weak-to-strong loss: {self.num_classes} classes not in [1, {ops.W2S_MAX_CLASSES}] (fused=False takes more)")
        if self.ce_weight < 0 or self.dice_weight < 0 or self.smooth < 0:
            raise ValueError("weak-to-strong loss: ce_weight, dice_weight and smooth must not be negative")
        self.last_ce = self.last_dice = self.last_kept = self.last_pasted = None

    def forward(self, logits_strong: torch.Tensor, code: torch.Tensor, mask: Optional[torch.Tensor] = None, perm=None, *,
                dyn: Optional[torch.Tensor] = None):
        if logits_strong.ndim != 4:
            raise NotImplementedError("the weak-to-strong loss implements 2-D inputs [B, K, H, W]")
        assert logits_strong.shape[1] == self.num_classes, \
            "inputs {} & num_classes+1 {} do not match".format(tuple(logits_strong.shape), self.num_classes)
        b, _, h, w = logits_strong.shape
        if self.fused:
            loss = ops.WeakToStrongFn.apply(logits_strong, code, mask, perm, dyn, self.ce_weight, self.dice_weight, self.smooth)
            out, counts = ops.WeakToStrongFn.last_out, ops.WeakToStrongFn.last_counts
            self.last_ce, self.last_dice, self.last_kept, self.last_pasted = out[1], out[2], counts[0], counts[1]
            return loss
        if code.dtype != torch.uint8 or tuple(code.shape) != (b, h, w):
            raise MiaError(f"weak-to-strong loss: the code map is uint8 [{b}, {h}, {w}], got {code.dtype} {tuple(code.shape)}")
        if mask is not None and perm is not None:
            ops._bcp_mask("weak-to-strong loss", mask, b, h, w)
            if isinstance(perm, torch.Tensor) and perm.is_cuda:
                perm = torch.where((perm >= 0) & (perm < b), perm, torch.arange(b, device=perm.device, dtype=perm.dtype))  # the kernels' guard
            else:
                perm = ops._perm_arg("weak-to-strong loss", perm, b, torch.device("cpu"))
        weight = 1.0 if dyn is None else ops._dyn_arg("weak-to-strong loss", dyn, 2, True)[0]
        loss, terms, counts = weak_to_strong_tensor_ops(logits_strong, code, mask, perm, weight, self.ce_weight, self.dice_weight,
                                                        self.smooth)
        self.last_ce, self.last_dice, self.last_kept, self.last_pasted = terms[0], terms[1], counts[0], counts[1]
        return loss
