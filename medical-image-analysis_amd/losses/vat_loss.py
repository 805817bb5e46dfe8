"""Virtual adversarial training (VAT: Miyato et al., TPAMI 2018) on the HIP kernels of `csrc/vat.hip` and the image gradient of
`csrc/stem_dgrad.hip`.  The reference ships `losses/adv_loss.py` (`VAT2d`, `xi=10, epi=6, ip=1`) for its SAM path; `losses.adv_loss`
still resolves to that file, and this module is the project's own form for the UNet path.

Definition.  With `p = softmax(z_target, 1)` (no gradient), `log q = log_softmax(z, 1)` and `log p = log_softmax(z_target, 1)`:

    KL(z_target || z) = sum over pixels and classes of p * (log p - log q) / den        (a term with p == 0 contributes 0)
    d KL / d z        = (softmax(z, 1) - p) / den

`reduction="batchmean"` divides by the batch size B: the scale of the published code (`F.kl_div(..., reduction="batchmean")`).
`reduction="mean"` divides by B * H * W, the per-pixel mean: ours, and the default.  The two differ by the factor H * W.

`VATLoss.adversarial(model, x, z_clean, d0=None, eps_dev=None)` is the power iteration:

    d = d0, or u / (||u||_2 + 1e-8) per image with u ~ U(-0.5, 0.5)                     (`ops.vat_noise`: torch's device generator)
    ip times:   x_hat = x + xi * d                                                       (a leaf that requires a gradient)
                D     = batchmean KL(z_clean || model(x_hat))
                g     = d D / d x_hat                                                    (under `ops.frozen_parameters`)
                d     = g / (||g||_2 + 1e-8) per image
    x_adv = x + eps * d

`g` is the gradient with respect to `x_hat`; the published code differentiates with respect to `d`, which is `xi * g`, so the
normalisation here is `xi * g / (xi * ||g|| + 1e-8)` (`ops.vat_perturb` with `gscale = xi`): the same direction bit for bit in exact
arithmetic.  Throughout `adversarial` the parameters are frozen (no weight-gradient kernel runs) and batch-norm layers normalise with
batch statistics while their running statistics and `num_batches_tracked` stay untouched (`ops.no_bn_tracking`).

`fused=False`, more than 8 classes or logits that are not fp32 take `kl_consistency_reference`, the tensor-op form of the same
definition.
"""
from __future__ import annotations

import torch
from torch import nn

from mia_hip import MiaError, ops

KL_MAX_CLASSES = 8
_REDUCTIONS = ("mean", "batchmean")


def _den(z: torch.Tensor, reduction: str) -> float:
    if reduction not in _REDUCTIONS:
        raise ValueError(f'KL consistency: reduction="{reduction}" is none of {_REDUCTIONS}')
    return float(z.shape[0]) if reduction == "batchmean" else float(z.shape[0] * z.shape[2] * z.shape[3])


def kl_consistency_reference(z: torch.Tensor, z_target: torch.Tensor, dyn=None, reduction: str = "mean") -> torch.Tensor:
    """The definition in tensor operations (any class count, any float dtype): weight * KL(z_target || z)."""
    lq = torch.log_softmax(z.float(), 1)
    lp = torch.log_softmax(z_target.detach().float(), 1)
    p = lp.exp()
    l = torch.where(p > 0, p * (lp - lq), torch.zeros_like(p)).sum() / _den(z, reduction)
    return l if dyn is None else dyn.detach()[0] * l


def kl_consistency(z: torch.Tensor, z_target: torch.Tensor, dyn=None, reduction: str = "mean") -> torch.Tensor:
    """weight * KL(softmax(z_target) || softmax(z)) as a 0-dim device tensor: one fused HIP pass over the two logits tensors each way
    (`ops.KLConsistencyFn`).  z, z_target: fp32 [B, K <= 8, H, W] in any layout whose H and W collapse; only `z` gets a gradient.
    `dyn`: None (weight 1) or a device fp32 tensor whose first element is the weight, read when the kernels run."""
    ops._need_dev(z, z_target, dyn)
    if z.ndim != 4:
        raise NotImplementedError("the HIP KL consistency implements 2-D inputs [B, K, H, W]")
    if not 1 <= z.shape[1] <= KL_MAX_CLASSES or z.dtype != torch.float32 or z_target.dtype != torch.float32:
        raise MiaError(f"kl_consistency: fp32 logits with 1..{KL_MAX_CLASSES} classes expected, got {z.dtype} {tuple(z.shape)}")
    return ops.KLConsistencyFn.apply(z, z_target, dyn, _den(z, reduction))


class VATLoss(nn.Module):
    """`adversarial(model, x, z_clean)` -> `x_adv` and `forward(z_adv, z_clean, dyn=None)` -> `weight * KL(z_clean || z_adv)` (see the
    module text).  xi: the length of the probe step, eps: the length of the adversarial step, ip: power iterations.  `last_value` is the
    unweighted KL of the latest forward (device tensor, no host sync)."""

    def __init__(self, xi: float = 10.0, eps: float = 6.0, ip: int = 1, reduction: str = "mean", fused: bool = True):
        super().__init__()
        if reduction not in _REDUCTIONS:
            raise ValueError(f'VATLoss: reduction="{reduction}" is none of {_REDUCTIONS}')
        if not (xi > 0 and ip >= 0):
            raise ValueError("VATLoss: xi must be positive and ip non-negative")
        self.xi, self.eps, self.ip, self.reduction, self.fused = float(xi), float(eps), int(ip), reduction, bool(fused)
        self.last_value = None

    def _kl(self, z, z_target, dyn, reduction):
        if self.fused and z.ndim == 4 and z.shape[1] <= KL_MAX_CLASSES and z.dtype == torch.float32 and z_target.dtype == torch.float32:
            out = kl_consistency(z, z_target, dyn, reduction)
            return out, ops.KLConsistencyFn.last_out[1]
        value = kl_consistency_reference(z, z_target, None, reduction)
        return (value if dyn is None else dyn.detach()[0] * value), value.detach()

    def forward(self, z_adv: torch.Tensor, z_clean: torch.Tensor, dyn=None) -> torch.Tensor:
        loss, self.last_value = self._kl(z_adv, z_clean, dyn, self.reduction)
        return loss

    def adversarial(self, model, x: torch.Tensor, z_clean: torch.Tensor, d0=None, eps_dev=None) -> torch.Tensor:
        """x: fp32 images [B, C, H, W] on the device; z_clean: the model's logits on x (no gradient).  d0: a start direction of x's
        shape (it is normalised per image), else noise from torch's device generator.  eps_dev: a device fp32 value that replaces
        `eps` (read when the kernel runs, so a ramp needs no host sync).  Returns x_adv (no gradient)."""
        ops._need_dev(x, z_clean, d0, eps_dev)
        if x.ndim != 4:
            raise NotImplementedError("VATLoss.adversarial implements 2-D inputs [B, C, H, W]")
        x = x.detach().float().contiguous()
        z_clean = z_clean.detach()
        u = ops.vat_noise(x.shape, x.device) if d0 is None else d0.detach().to(device=x.device, dtype=torch.float32).contiguous()
        if u.shape != x.shape:
            raise MiaError(f"VATLoss.adversarial: d0 {tuple(u.shape)} does not have the image's shape {tuple(x.shape)}")
        g, gscale = u, 1.0  # d = gscale * g / (gscale * ||g|| + 1e-8)
        with ops.frozen_parameters(model), ops.no_bn_tracking():
            for _ in range(self.ip):
                x_hat = ops.vat_perturb(x, g, ops.sample_sumsq(g), gscale, self.xi).requires_grad_(True)
                with torch.enable_grad():
                    dist, _ = self._kl(model(x_hat), z_clean, None, "batchmean")
                    g, = torch.autograd.grad(dist, x_hat)
                g, gscale = g.contiguous(), self.xi
        return ops.vat_perturb(x, g, ops.sample_sumsq(g), gscale, self.eps, eps_dev)
