"""Dual-task consistency (DTC: Luo et al., AAAI 2021) on the HIP kernels of `csrc/dtc.hip`: one network predicts the segmentation and,
from a second 1x1 head, a level-set map -- `tanh` of a regression of the normalised signed distance to the object boundary -- and the
two predictions must agree on every image, labelled or not.  The reference has no such module; like `cross_pseudo.py`,
`copy_paste.py` and `weak_strong.py` this is the project's own addition, and THIS TEXT is the definition the kernels and the tests
follow.

Notation.  `K1 = num_classes + 1` classes with background, `C = K1 - 1` foreground classes; channel `c` of the level-set head belongs
to class `c + 1`.  `z` `[B, K1, H, W]` are the segmentation logits, `r` `[B, C, H, W]` the level-set logits; `s = softmax(z)`,
`t = tanh(r)`, `q = sigmoid(-k t)` with the published `k = 1500`.  The first `lb` images are labelled, and
`phi = signed_distance_map(label[:lb], num_classes)` `[lb, C, H, W]` at unit spacing: negative inside, positive outside, 0 on the inner
border, on a class absent from the image and on a class that fills it (`boundary_loss.py`).

Extents.  Per (image, class) `m_out = max(phi)` and `m_in = max(-phi)`, both >= 0 (`mia_hip.ops.sdm_extent`).

Normalised target `T`, the published `compute_sdf` restated on `phi` (inside the object the published `posdis` is `1 - phi`):

    phi > 0 :  T =  phi / m_out
    phi < 0 :  T = -(1 - phi) / (1 + m_in)
    phi = 0 :  T = 0

The last row is the published `sdf[boundary == 1] = 0`; it also covers an absent class (the published code leaves zeros there too).
`normalized_distance_map(labels, num_classes)` returns `T`; the kernels compute it per pixel from `phi` and the extents and never
store it.

Terms.

    L_sdf  = mean over n < lb, c, pixel of (t - T)^2                 0 when lb = 0, never NaN
    L_cons = mean over ALL n, c, pixel of (q_c - s_{c+1})^2          gradient into both heads, as published
    L      = dyn[0] L_cons + dyn[1] L_sdf

`dyn[0]` is the consistency weight, which follows a ramp, `dyn[1]` is beta (published 0.3); both are read from device memory when the
kernels run.  `dyn` None means both are 1.  `sigmoid(-k t)` is evaluated from `exp(-|k t|)`, so it stays finite for `|k t|` in the
thousands and `q (1 - q)` underflows to 0 there.

Gradients.  With `N = B C H W`, `Ns = lb C H W`, `d_c = q_c - s_{c+1}`, `e_0 = 0`, `e_{c+1} = -d_c`:

    dL/dz_j = (2 dyn[0] / N) s_j (e_j - sum_i s_i e_i)
    dL/dr_c = [ (2 dyn[0] / N) d_c (-k q_c (1 - q_c)) + [n < lb] (2 dyn[1] / Ns) (t_c - T_c) ] (1 - t_c^2)

`phi` and the labels carry no gradient.

Where this departs from the published code.  (1) The published LA code has ONE foreground class and compares `q` with
`sigmoid(z)`; here the segmentation head is the project's soft-max over `K1` classes and channel `c` is compared with `s_{c+1}`, which
for `K1 = 2` is `sigmoid(z_1 - z_0)`.  (2) A class that fills its image has `phi = 0` by this project's rule, so `T = 0` there; the
published code divides 0 by 0 in that case (`negdis` is all zero) and trains on NaN.  (3) The distance map is computed on the GPU from
the labels the step actually sees, after augmentation, not by scipy in the loader.  (4) The inner border is where the exact Euclidean
distance to the background is 1, which is skimage's `find_boundaries(mode="inner")` for 4-connectivity.

Not supported: a pixel spacing other than 1 (the `- 1` inside `phi` is literal, so `1 - phi` is the inside distance only at unit
spacing; asking for another spacing raises), 3-D volumes, a level-set head on a subset of the classes.

From tensor ops the loss is a `tanh`, a `sigmoid`, a soft-max, two squared differences and their autograd graph, about ten
logits-sized temporaries each way; the fused form is one streaming pass each way that keeps nothing of the logits' size but the two
gradients.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from mia_hip import MiaError, ops


def _unit_spacing(spacing) -> None:
    if spacing is not None and tuple(float(s) for s in spacing) != (1.0, 1.0):
        raise NotImplementedError("the dual-task target is defined at unit spacing: the `- 1` inside the signed distance map is "
                                  "literal, so `1 - phi` is the inside distance only there")


def normalize_distance_map(phi: torch.Tensor, extent: torch.Tensor) -> torch.Tensor:
    """`T` of the module text from `phi` [B, C, H, W] and its extents [B, C, 2] in tensor ops, in phi's dtype, on any device."""
    m_out, m_in = extent[..., 0, None, None].to(phi.dtype), extent[..., 1, None, None].to(phi.dtype)
    outside = phi / torch.where(m_out > 0, m_out, torch.ones_like(m_out))
    inside = -(1.0 - phi) / (1.0 + m_in)
    return torch.where(phi > 0, outside, torch.where(phi < 0, inside, torch.zeros_like(phi)))


def normalized_distance_map(labels: torch.Tensor, num_classes: int, spacing=None) -> torch.Tensor:
    """fp32 `T` `[B, num_classes, H, W]` of index labels `[B, H, W]` or `[B, 1, H, W]` on the device: `signed_distance_map`,
    `ops.sdm_extent` and tensor ops.  For users and tests; the loss computes `T` per pixel and does not call this.  No autograd."""
    from losses.boundary_loss import signed_distance_map
    _unit_spacing(spacing)
    phi = signed_distance_map(labels, num_classes)
    return normalize_distance_map(phi, ops.sdm_extent(phi))


def dual_task_tensor_ops(z, r, T, lb: int, k: float = 1500.0, w_cons=1.0, w_sdf=1.0):
    """The definition in tensor ops, in the logits' dtype and on their device (CPU included): `(L, L_cons, L_sdf)`, differentiable in
    `z` and `r`.  `T` is the normalised target of the first `lb` images (None when `lb = 0`); the weights are numbers or 0-dim
    tensors.  The sigmoid is `torch.sigmoid`, which is finite for any argument."""
    s = torch.softmax(z, 1)
    t = torch.tanh(r)
    q = torch.sigmoid(-k * t)
    cons = ((q - s[:, 1:]) ** 2).mean()
    sdf = ((t[:lb] - T.to(t.dtype)) ** 2).mean() if lb > 0 else torch.zeros((), dtype=cons.dtype, device=cons.device)
    return w_cons * cons + w_sdf * sdf, cons, sdf


class DualTaskConsistencyLoss(nn.Module):
    """`forward(z, r, labels, labeled_bs, dyn=None, *, phi=None)` -> `L` of the module text (0-dim tensor); `z` and `r` receive a
    gradient.  `num_classes` counts foreground classes like `DiceLoss`: `z` is `[B, num_classes + 1, H, W]`, `r` `[B, num_classes, H,
    W]`, in any layout whose H and W collapse; `labels` `[>= labeled_bs, H, W]` or `[.., 1, H, W]` index maps, of which the first
    `labeled_bs` are read (None with `labeled_bs = 0`); `dyn` None or the device fp32 `{consistency weight, beta}` of `DTCEngine`;
    `phi` a precomputed fp32 `signed_distance_map(labels[:labeled_bs], num_classes)` (e.g. shared with a boundary loss).
    `fused=True`: the fp32 kernels of csrc/dtc.hip, 2 to 8 classes with background, device tensors only.  `fused=False`: the
    tensor-op form of the same definition, which also serves more classes, other dtypes and CPU tensors (on CPU tensors `phi` is
    required, since the distance transform runs on the GPU); non-fp32 logits or more than 8 classes take it automatically.
    By-products of the latest forward, 0-dim device tensors, no host sync: `last_consistency`, `last_sdf` (both unweighted).  2-D
    only, unit spacing only."""

    def __init__(self, num_classes: int, k: float = 1500.0, fused: bool = True, spacing=None):
        super().__init__()
        _unit_spacing(spacing)
        self.num_classes = num_classes + 1  # include background, like DiceLoss
        if self.num_classes < 2:
            raise MiaError("dual-task loss: at least one foreground class is needed for a level-set head")
        self.k, self.fused = float(k), bool(fused)
        self.last_consistency = self.last_sdf = None

    def _phi(self, labels, lb: int, h: int, w: int, phi):
        if lb == 0:
            return None
        if phi is not None:
            if tuple(phi.shape) != (lb, self.num_classes - 1, h, w):
                raise MiaError(f"dual-task loss: phi {tuple(phi.shape)}, expected {(lb, self.num_classes - 1, h, w)}")
            return phi
        if labels is None or labels.shape[0] < lb:
            raise MiaError(f"dual-task loss: {0 if labels is None else labels.shape[0]} label maps for labeled_bs={lb}")
        from losses.boundary_loss import signed_distance_map
        return signed_distance_map(labels[:lb], self.num_classes - 1)

    def forward(self, z: torch.Tensor, r: torch.Tensor, labels: Optional[torch.Tensor], labeled_bs: int,
                dyn: Optional[torch.Tensor] = None, *, phi: Optional[torch.Tensor] = None):
        if z.ndim != 4 or r.ndim != 4:
            raise NotImplementedError("the dual-task loss implements 2-D inputs [B, K, H, W]")
        assert z.shape[1] == self.num_classes, "inputs {} & num_classes+1 {} do not match".format(tuple(z.shape), self.num_classes)
        b, k1, h, w = z.shape
        if tuple(r.shape) != (b, k1 - 1, h, w):
            raise MiaError(f"dual-task loss: level-set logits {tuple(r.shape)}, expected {(b, k1 - 1, h, w)} for logits {tuple(z.shape)}")
        lb = int(labeled_bs)
        if not 0 <= lb <= b:
            raise MiaError(f"dual-task loss: labeled_bs={lb} not in [0, {b}]")
        phi = self._phi(labels, lb, h, w, phi)
        fused = self.fused and k1 <= ops.DTC_MAX_CLASSES and z.dtype == torch.float32 and r.dtype == torch.float32
        if fused:
            loss = ops.DTCLossFn.apply(z, r, phi, None, lb, self.k, dyn)
            out = ops.DTCLossFn.last_out
            self.last_consistency, self.last_sdf = out[1], out[2]
            return loss
        T = None
        if lb > 0:
            ext = torch.stack([phi.amax((2, 3)), (-phi).amax((2, 3))], -1).clamp_min(0.0)
            T = normalize_distance_map(phi, ext).to(z.device)
        w_cons, w_sdf = (1.0, 1.0) if dyn is None else ops._dyn_arg("dual-task loss", dyn, 2, True)
        loss, cons, sdf = dual_task_tensor_ops(z, r, T, lb, self.k, w_cons, w_sdf)
        self.last_consistency, self.last_sdf = cons.detach(), sdf.detach()
        return loss
