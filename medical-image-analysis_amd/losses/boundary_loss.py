"""Boundary loss of Kervadec et al. (MIDL 2019: `one_hot2dist` + `SurfaceLoss` of their public code) on the HIP kernels of
`csrc/boundary.hip`.  The reference has no such module; this is the project's own addition.

The loss is the mean over (image, class, pixel) of `softmax(logits)_k * phi_k`, with `phi_k` the signed Euclidean distance map of
class k's ground truth.  Everywhere else `phi` is computed by scipy in the DataLoader; here the labels are augmented on the GPU
after collation (`transforms.gpu_pipeline.BatchedAugment`), so the map is computed on the GPU, every step, from the labels the loss
actually sees.

Definition of `phi` for `G = (labels[b] == k)`:  `phi = edt(~G) * ~G - (edt(G) - 1) * G`: outside the object the distance to the
nearest object pixel; inside, minus (the distance to the nearest non-object pixel, minus one), so inner border pixels get 0 at
unit spacing.  The `- 1` is literal whatever the spacing -- that is the published definition.  Pixels outside the array do not
exist: an object that touches the image edge has no boundary there (scipy's behaviour).  A class that is absent from an image has
`phi = 0` there (Kervadec); so has a class that fills the whole image, which is this project's own rule -- scipy's transform of an
all-true mask measures to an imaginary point, and Kervadec's code inherits those values.
"""
from __future__ import annotations

import torch
from torch import nn

from mia_hip import ops


def _spacing2(spacing):
    if spacing is None:
        return None
    sp = tuple(float(s) for s in spacing)
    if len(sp) != 2:
        raise NotImplementedError("the HIP boundary loss implements 2-D images: spacing is (sh, sw)")
    return sp


def signed_distance_map(labels: torch.Tensor, num_classes: int, classes=None, spacing=None) -> torch.Tensor:
    """fp32 `[B, len(classes), H, W]` signed distance maps of index labels `[B,H,W]` or `[B,1,H,W]` (uint8 stays uint8).
    `num_classes` counts FOREGROUND classes like `DiceLoss`; `classes` defaults to `1 .. num_classes` (Kervadec's `idc`), the
    channels follow the classes in ascending order; `spacing` is `(sh, sw)`, default `(1, 1)`.  No autograd.  Also the target for
    anyone regressing distance maps."""
    if labels.ndim == 4 and labels.shape[1] == 1:
        labels = labels[:, 0]
    if labels.ndim != 3:
        raise NotImplementedError(f"the HIP boundary loss implements 2-D label maps [B,H,W] or [B,1,H,W]; got {tuple(labels.shape)}")
    return ops.signed_distance_map(labels, num_classes + 1, classes, _spacing2(spacing))


class BoundaryLoss(nn.Module):
    """`mean(softmax(logits)[:, classes] * phi)` with `phi = signed_distance_map(labels, ...)`, one fused HIP pass over the logits
    each way.  `num_classes` counts foreground classes like `DiceLoss`; labels are `[B,H,W]` or `[B,1,H,W]`.  A precomputed
    `dist` (`[B, len(classes), H, W]` fp32, e.g. shared between several heads) skips the transform.  `weight`: None or a device
    fp32 tensor of one element that multiplies value and gradient inside the kernels (see `RegionAndBoundaryLoss`).  The
    unweighted value of the latest forward is `last_value` (0-dim device tensor).  A label outside `0 .. num_classes` makes the
    loss and every gradient NaN and `mia_hip.ops.check_labels()` raise, as in the other losses."""

    def __init__(self, num_classes: int, classes=None, spacing=None, dimension: int = 2):
        super().__init__()
        if dimension != 2:
            raise NotImplementedError("the HIP boundary loss implements 2-D images (the network is 2-D)")
        self.num_classes = num_classes + 1  # include background, like DiceLoss
        self.mask, self.classes = ops.class_mask(self.num_classes, classes)
        self.spacing = _spacing2(spacing)
        self.last_value = None

    def forward(self, logits: torch.Tensor, labels: torch.Tensor, dist: torch.Tensor | None = None, *, weight: torch.Tensor | None = None):
        ops._need_dev(logits, labels, dist, weight)
        if logits.ndim != 4:
            raise NotImplementedError("the HIP boundary loss implements 2-D inputs [B, K, H, W]")
        b, k1, h, w = logits.shape
        assert k1 == self.num_classes, "inputs {} & num_classes+1 {} do not match".format(tuple(logits.shape), self.num_classes)
        assert labels.numel() == b * h * w, "inputs {} & target {} shape do not match".format(tuple(logits.shape), tuple(labels.shape))
        labels = labels.reshape(b, h, w)
        if dist is None:
            dist = ops.signed_distance_map(labels, k1, self.classes, self.spacing)
        loss = ops.BoundaryLossFn.apply(logits, labels, dist, self.mask, weight)
        self.last_value = ops.BoundaryLossFn.last_out[1]
        return loss


class RegionAndBoundaryLoss(nn.Module):
    """A region loss mixed with the boundary loss under a weight `alpha` that moves during training (Kervadec schedules both):
      mode="rebalance":  (1 - alpha) * region + alpha * boundary
      mode="add":        region + alpha * boundary
    `alpha` lives in device fp32 buffers that the kernels and the mixing arithmetic read when they run, so a step captured into a
    graph (`TrainEngine(graph=True)`) follows `set_alpha(v)` without a re-capture; call `set_alpha` between steps, outside any
    capture.  The trainer feeds it from the ramps of `scheduler.ramps` (`SigmoidRampUp`, `LinearRampUp`), which this project does
    not redefine.  By-products of the latest forward, 0-dim device tensors: `last_region`, `last_boundary` (unweighted)."""

    def __init__(self, region_loss: nn.Module, boundary_loss: nn.Module, alpha: float = 0.01, mode: str = "rebalance"):
        super().__init__()
        if mode not in ("rebalance", "add"):
            raise ValueError(f"RegionAndBoundaryLoss: mode {mode!r} is not 'rebalance' or 'add'")
        self.region_loss = region_loss
        self.boundary_loss = boundary_loss
        self.mode = mode
        self._alpha = float(alpha)
        self._buf = None  # [2] fp32 on the logits' device: alpha | the region term's weight
        self.last_region = self.last_boundary = None

    @property
    def alpha(self) -> float:
        return self._alpha

    def region_weight(self) -> float:
        return 1.0 - self._alpha if self.mode == "rebalance" else 1.0

    def _values(self) -> torch.Tensor:
        return torch.tensor([self._alpha, self.region_weight()], dtype=torch.float32)

    def set_alpha(self, value: float) -> None:
        self._alpha = float(value)
        if self._buf is not None:
            self._buf.copy_(self._values())

    def _alpha_buffers(self, device) -> torch.Tensor:
        if self._buf is None or self._buf.device != device:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("RegionAndBoundaryLoss: the first forward on a device creates the alpha buffers and cannot run "
                                   "inside a graph capture; run one eager step first")
            self._buf = self._values().to(device)
        return self._buf

    def forward(self, logits: torch.Tensor, labels: torch.Tensor):
        buf = self._alpha_buffers(logits.device)
        region = self.region_loss(logits, labels)
        boundary = self.boundary_loss(logits, labels, weight=buf[0:1])
        self.last_region = region.detach()
        self.last_boundary = getattr(self.boundary_loss, "last_value", None)
        return region * buf[1] + boundary
