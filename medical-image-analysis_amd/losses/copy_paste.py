"""Bidirectional copy-paste (BCP: Bai et al., CVPR 2023) on the HIP kernels of `csrc/bcp.hip`: the box mask, and the loss of a mixed
image whose pixels are supervised by one of two label maps.  The reference has no such module; like `consistency_loss.py` and
`cross_pseudo.py` this is the project's own addition, and THIS TEXT is the definition the kernels and the tests follow.

Mask.  `random_box_mask(h, w, ratio)` is a uint8 `[h, w]` device tensor of ones with one zero box of `int(h * ratio) x int(w * ratio)`
pixels whose top-left corner is uniform over the positions that keep the box inside the image.  One mask per step is shared by the
whole batch, as published.

Mix.  `mia_hip.ops.bcp_mix(fg, bg, mask)` is `mask != 0 ? fg : bg` per pixel, every channel alike.  It is a SELECTION, where the
published code forms `fg * m + bg * (1 - m)`: the bits of the chosen operand pass through (NaN payloads, -0.0), and a NaN or an
infinity in the operand NOT chosen does not reach the result (in the published form `inf * 0` does).

Loss.  Logits `z` are `[B, K, H, W]`, `K = num_classes + 1 <= 8` for the kernels, `label_a`, `label_b` are `[B, H, W]` index maps,
`mask` is uint8 `[H, W]` or `[B, H, W]`, `N = B * H * W`.  Region A is `mask != 0` and is supervised by `label_a`; region B is
`mask == 0` and is supervised by `label_b`.  With `p = softmax(z)`, and for each region r its indicator `m_r` and its label `y_r`:

* `I_rk = sum m_r p_k [y_r = k]`, `Z_rk = sum m_r p_k^2`, `Y_rk = sum m_r [y_r = k]`, `N_r = sum m_r` -- the sums run over ALL images
  and pixels of the call (the published "batch" Dice), and `Y`, `N` are exact integers;
* `D_r = (1/K) sum_k (1 - (2 I_rk + s) / (Z_rk + Y_rk + s))`: the squared-denominator Dice, every class counts, background included;
  `s = smooth = 1e-10`;
* `C_r = sum m_r (logsumexp(z) - z[y_r]) / (N_r + 1e-16)`: the masked mean cross-entropy;
* an empty region gives `D_r = C_r = 0`, not NaN (the published Dice of an empty region is 1 - s/s = 0 as well);
* `L = weight_a (D_A + C_A) / 2 + weight_b (D_B + C_B) / 2`.

The gradient for a pixel of region r is
`dL/dz_j = (w_r/2) [ (p_j - [j = y_r]) / (N_r + 1e-16) + sum_k g_rk p_k ([k = j] - p_j) ]` with
`g_rk = -(1/K) (2 [y_r = k] / den_rk - 2 p_k (2 I_rk + s) / den_rk^2)`, `den_rk = Z_rk + Y_rk + s`.

A pixel reads ONLY its own region's label: the other map may hold anything there, out-of-range values included.  An out-of-range
label that IS selected gives NaN results and raises the sticky verdict `mia_hip.ops.check_labels()` reads, as in the other losses.

The published code forms the same value with two soft-maxes, four masked Dice passes and two masked CE maps per mixed batch; the
fused form is one streaming pass over the logits each way and keeps nothing of the logits' size but the gradient.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from mia_hip import MiaError, ops


def random_box_mask(h: int, w: int, ratio: float = 2 / 3, generator: Optional[torch.Generator] = None,
                    device="cuda") -> torch.Tensor:
    """uint8 `[h, w]` on `device`: ones, except one zero box of `int(h * ratio) x int(w * ratio)` pixels.  The corner is drawn on the
    host (`torch.randint` with the CPU generator, `generator` or the default one), so `torch.manual_seed` reproduces it and nothing
    waits for the device; the box is written with a slice fill.  `ratio = 0` gives all ones (and draws the same two numbers)."""
    h, w = int(h), int(w)
    if not 0.0 <= ratio <= 1.0:
        raise ValueError(f"random_box_mask: ratio={ratio} not in [0, 1]")
    bh, bw = int(h * ratio), int(w * ratio)
    y0 = int(torch.randint(0, h - bh + 1, (1,), generator=generator).item())
    x0 = int(torch.randint(0, w - bw + 1, (1,), generator=generator).item())
    mask = torch.ones((h, w), device=device, dtype=torch.uint8)
    if bh > 0 and bw > 0:
        mask[y0:y0 + bh, x0:x0 + bw] = 0
    return mask


def copy_paste_loss_tensor_ops(logits, label_a, label_b, mask, weight_a=1.0, weight_b=1.0, smooth=1e-10):
    """The definition in tensor ops, in the logits' dtype: `(L, terms [4] = {D_A, C_A, D_B, C_B}, counts int64 [2])`.  Differentiable
    in `logits`; any class count.  An out-of-range selected label makes `L` and the terms NaN (no sticky verdict in this form)."""
    b, k, h, w = logits.shape
    m = (mask != 0).expand(b, h, w) if mask.ndim == 3 else (mask != 0)[None].expand(b, h, w)
    y = torch.where(m, label_a.reshape(b, h, w).long(), label_b.reshape(b, h, w).long())
    bad = ((y < 0) | (y >= k)).any()
    onehot = (y[:, None] == torch.arange(k, device=logits.device)[None, :, None, None]).to(logits.dtype)
    lse = torch.logsumexp(logits, 1)
    p = torch.exp(logits - lse[:, None])
    nll = lse - (logits * onehot).sum(1)
    terms, counts = [], []
    for mr in (m, ~m):
        mf = mr.to(logits.dtype)
        n = mr.sum()
        mk = mf[:, None]
        inter = (mk * p * onehot).sum((0, 2, 3))
        z = (mk * p * p).sum((0, 2, 3))
        yk = (mk * onehot).sum((0, 2, 3))
        dice = (1.0 - (2.0 * inter + smooth) / (z + yk + smooth)).mean()
        ce = (mf * nll).sum() / (n.to(logits.dtype) + 1e-16)
        live = (n > 0).to(logits.dtype)
        terms += [dice * live, ce * live]
        counts.append(n)
    loss = weight_a * (terms[0] + terms[1]) / 2 + weight_b * (terms[2] + terms[3]) / 2
    nan = torch.full_like(loss, float("nan"))
    terms = torch.stack([torch.where(bad, nan, t.detach()) for t in terms])
    return torch.where(bad, nan, loss), terms, torch.stack(counts).to(torch.int64)


class CopyPasteLoss(nn.Module):
    """`forward(logits, label_a, label_b, mask, weight_a=1.0, weight_b=1.0)` -> `L` of the module text (0-dim device tensor); only
    the logits receive a gradient.  `num_classes` counts foreground classes like `DiceLoss`; logits are `[B, num_classes + 1, H, W]`
    in any layout whose H and W collapse (planar, the head's channels-last view, a batch slice of either); labels `[B, H, W]` int64
    or uint8; mask uint8 `[H, W]` or `[B, H, W]`.  `fused=True` (fp32 kernels of csrc/bcp.hip, at most 8 classes with background;
    more raise `MiaError`); `fused=False` is the tensor-op form of the same definition, which also serves more classes and keeps
    non-fp32 logits in their dtype.  By-products of the latest forward, device tensors, no host sync: `last_terms` = `[D_A, C_A, D_B,
    C_B]` and `last_counts` = `[N_A, N_B]` (int64).  2-D only.  There is no CPU fallback: CPU tensors raise `MiaError`."""

    def __init__(self, num_classes: int, smooth: float = 1e-10, fused: bool = True):
        super().__init__()
        self.num_classes = num_classes + 1  # include background, like DiceLoss
        self.smooth, self.fused = float(smooth), bool(fused)
        if self.num_classes < 1 or (self.fused and self.num_classes > ops.BCP_MAX_CLASSES):
            raise MiaError(f"copy-paste loss: {self.num_classes} classes not in [1, {ops.BCP_MAX_CLASSES}] (fused=False takes more)")
        self.last_terms = self.last_counts = None

    def forward(self, logits: torch.Tensor, label_a: torch.Tensor, label_b: torch.Tensor, mask: torch.Tensor,
                weight_a: float = 1.0, weight_b: float = 1.0):
        ops._need_dev(logits, label_a, label_b, mask)
        if logits.ndim != 4:
            raise NotImplementedError("the HIP copy-paste loss implements 2-D inputs [B, K, H, W]")
        assert logits.shape[1] == self.num_classes, \
            "inputs {} & num_classes+1 {} do not match".format(tuple(logits.shape), self.num_classes)
        if self.fused:
            loss = ops.CopyPasteLossFn.apply(logits, label_a, label_b, mask, float(weight_a), float(weight_b), self.smooth)
            self.last_terms, self.last_counts = ops.CopyPasteLossFn.last_out[1:], ops.CopyPasteLossFn.last_counts
            return loss
        b, _, h, w = logits.shape
        ops._bcp_mask("copy-paste loss", mask, b, h, w)
        loss, self.last_terms, self.last_counts = copy_paste_loss_tensor_ops(logits, label_a, label_b, mask, float(weight_a),
                                                                             float(weight_b), self.smooth)
        return loss
