"""Cross pseudo supervision (CPS: Chen et al., CVPR 2021) on the HIP kernels of `csrc/cps.hip`.  The reference has no such module;
like `consistency_loss.py` and `pyramid_consistency.py` this is the project's own addition.

Logits `za`, `zb` are `[B, K, H, W]` fp32 from two networks with different initialisations, `N = B * H * W`, `K <= 8`:

* `ya = argmax_k za_k`, `yb` likewise -- compared on the fp32 logits themselves, a tie goes to the lowest index (`numpy.argmax`);
* `ca = [max_k softmax(za)_k >= tau]`, `cb` likewise: the confidence of the label SOURCE.  `tau = dyn[1]`, read on the device when
  the kernel runs; `tau = 0` keeps every pixel, which is the published CPS;
* `LA = (1/N) sum_p cb * (logsumexp(za) - za[yb])`, `LB = (1/N) sum_p ca * (logsumexp(zb) - zb[ya])`.  The denominator is always `N`
  (the FixMatch form): `tau = 0` is exactly `F.cross_entropy(za, yb) + F.cross_entropy(zb, ya)`, and an empty mask gives 0, not NaN.
  `-log p` is taken as `logsumexp(z) - z_y` without forming `p`, so a pixel whose label has soft-max 0 in fp32 still has a finite term;
* the result is `w * (LA + LB)` with `w = dyn[0]`; `dyn=None` means `w = 1`, `tau = 0`;
* gradients: `dLA/dza_j = (w/N) * cb * (pa_j - [j = yb])`, symmetric for `zb`.  Labels and flags carry no gradient, and a pixel whose
  flag is clear gets exactly `0.0`.

The forward takes one streaming pass over both logits tensors and keeps one byte per pixel (`ya | yb << 3 | ca << 6 | cb << 7`); the
backward reads that byte and writes both gradients in one pass, so both directions agree on every pixel by construction.  Counts of
confident pixels and of pixels where the two networks agree come out of the forward as exact integers, with no host sync.
"""
from __future__ import annotations

import torch
from torch import nn

from mia_hip import MiaError, ops


class CrossPseudoSupervisionLoss(nn.Module):
    """`forward(logits_a, logits_b, *, dyn=None)` -> `w * (LA + LB)` (0-dim device tensor); both inputs receive a gradient.
    `num_classes` counts foreground classes like `DiceLoss`; logits are `[B, num_classes + 1, H, W]` fp32 in any layout whose H and W
    collapse (planar, the head's channels-last view, a batch slice of either; the two networks may differ).  `dyn`: None or a device
    fp32 tensor `{weight, threshold}`.  By-products of the latest forward, device tensors, no host sync: `last_value_a`,
    `last_value_b` (the unweighted LA, LB), `last_confident` (int64 `[2]`: pixels of A and of B at or above the threshold) and
    `last_agree` (int64: pixels where the two arg-max labels agree).  2-D only.  There is no CPU fallback: CPU tensors raise
    `MiaError`."""

    def __init__(self, num_classes: int):
        super().__init__()
        self.num_classes = num_classes + 1  # include background, like DiceLoss
        if not 1 <= self.num_classes <= ops.CPS_MAX_CLASSES:
            raise MiaError(f"cross pseudo supervision: {self.num_classes} classes not in [1, {ops.CPS_MAX_CLASSES}]")
        self.last_value_a = self.last_value_b = self.last_confident = self.last_agree = None

    def forward(self, logits_a: torch.Tensor, logits_b: torch.Tensor, *, dyn: torch.Tensor | None = None):
        ops._need_dev(logits_a, logits_b, dyn)
        if logits_a.ndim != 4:
            raise NotImplementedError("the HIP cross pseudo supervision loss implements 2-D inputs [B, K, H, W]")
        assert logits_a.shape[1] == self.num_classes, \
            "inputs {} & num_classes+1 {} do not match".format(tuple(logits_a.shape), self.num_classes)
        loss = ops.CrossPseudoFn.apply(logits_a, logits_b, dyn)
        out, counts = ops.CrossPseudoFn.last_out, ops.CrossPseudoFn.last_counts
        self.last_value_a, self.last_value_b = out[1], out[2]
        self.last_confident, self.last_agree = counts[:2], counts[2]
        return loss
