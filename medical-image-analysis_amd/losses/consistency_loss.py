"""Mean-teacher consistency loss (Tarvainen & Valpola 2017) and its uncertainty-aware form (UA-MT: Yu et al., MICCAI 2019) on the
HIP kernels of `csrc/consistency.hip`.  The reference has no such module (its `adv_loss.py` / `contrastive_loss.py` belong to its
SAM path); this is the project's own addition.

With `ps = softmax(student_logits, 1)`, `pt = softmax(teacher_logits, 1)` and `dist = ((ps - pt) ** 2).sum(1)`:

* plain (`prob_mean=None`):  `torch.mean((ps - pt) ** 2)`, the Mean Teacher form;
* masked (`prob_mean` = the mean soft-max of the teacher's stochastic passes, e.g. what `inference.predictor.softmax_accum` leaves
  after T passes with `weight = 1 / T`):  `u = -(prob_mean * log(prob_mean + 1e-6)).sum(1)`, `mask = u < threshold`,
  `sum(mask * dist) / (den_scale * sum(mask) + 1e-16)` -- `den_scale = 2` is the published code's form.  An empty mask gives 0 and a
  zero gradient.

Only the student's logits receive a gradient.  The weight of the term and the entropy threshold live in a device buffer
`dyn = {weight, threshold}` that the kernels read when they run, so the ramps of a schedule never re-build anything (and a captured
step could follow them).
"""
from __future__ import annotations

import torch
from torch import nn

from mia_hip import MiaError, ops


class SoftmaxMSEConsistency(nn.Module):
    """`forward(student_logits, teacher_logits, prob_mean=None, *, dyn=None)` -> `weight * L` (0-dim device tensor), one fused HIP
    pass over the logits each way.  `num_classes` counts foreground classes like `DiceLoss`; logits are `[B, num_classes + 1, H, W]`
    fp32 in any layout whose H and W collapse (planar, the head's channels-last view, a batch slice of either; student and teacher
    may differ).  `dyn`: None (weight 1, plain form only) or a device fp32 tensor `{weight, threshold}`; `prob_mean` needs it.
    By-products of the latest forward, device tensors, no host sync: `last_value` (the unweighted L) and `last_kept` (int64: the
    pixels under the threshold; every pixel in the plain form).  There is no CPU fallback: CPU tensors raise `MiaError`."""

    def __init__(self, num_classes: int, den_scale: float = 2.0):
        super().__init__()
        self.num_classes = num_classes + 1  # include background, like DiceLoss
        if not 1 <= self.num_classes <= ops.CONSISTENCY_MAX_CLASSES:
            raise MiaError(f"consistency loss: {self.num_classes} classes not in [1, {ops.CONSISTENCY_MAX_CLASSES}]")
        self.den_scale = float(den_scale)
        if not 0.0 < self.den_scale < float("inf"):
            raise MiaError(f"consistency loss: den_scale={den_scale} must be finite and > 0")
        self.last_value = self.last_kept = None

    def forward(self, student_logits: torch.Tensor, teacher_logits: torch.Tensor, prob_mean: torch.Tensor | None = None, *,
                dyn: torch.Tensor | None = None):
        ops._need_dev(student_logits, teacher_logits, prob_mean, dyn)
        if student_logits.ndim != 4:
            raise NotImplementedError("the HIP consistency loss implements 2-D inputs [B, K, H, W]")
        assert student_logits.shape[1] == self.num_classes, \
            "inputs {} & num_classes+1 {} do not match".format(tuple(student_logits.shape), self.num_classes)
        loss = ops.ConsistencyFn.apply(student_logits, teacher_logits, prob_mean, dyn, self.den_scale)
        self.last_value = ops.ConsistencyFn.last_out[1]
        self.last_kept = ops.ConsistencyFn.last_kept[0]
        return loss
