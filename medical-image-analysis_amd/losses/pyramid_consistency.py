"""Uncertainty rectified pyramid consistency (URPC: Luo et al., MICCAI 2021 / MedIA 2022) between the outputs ONE network makes at
several decoder scales, for unlabelled images.  The reference has no such module; this is the project's own definition.  It follows
the published URPC code except that the scales are brought to full resolution by the heads' own bilinear `Upsample`.

`outputs` is what `UNet.forward(x, return_ds=True, upsample_ds=False)` returns (or batch slices of it): the main logits
`[N, K, H, W]` followed by the auxiliary heads' logits at their own resolution `[N, K, H / f, W / f]`.  With `up_f` =
`Upsample(scale_factor=f, mode="bilinear", align_corners=False)` (the identity for f = 1) and S outputs:

    u_s = up_{f_s}(z_s)       p_s = softmax(u_s, 1)       lp_s = log_softmax(u_s, 1)       m = (1/S) sum_s p_s
    v_s = sum_k [xlogy(m_k, m_k) - m_k * lp_sk]            KL(m || p_s) per pixel; a class with m_k == 0 adds 0
    w_s = exp(-v_s)           d_s = (m - p_s) ** 2
    L_s = mean(d_s * w_s) / (mean(w_s) + 1e-8) + mean(v_s)         the first mean over N K H W, the other two over N H W
    L   = (1/S) sum_s L_s

Gradients flow through everything, the mean `m` included (plain autograd of the expression, as in the published code).

The fused kernel (`ops.PyramidConsistencyFn`, csrc/urpc.hip) interpolates all S x K logits of a pixel in registers; none of the
full-resolution tensors above exists in either direction.  `fused=False` builds the expression from `ResizeBilinearFn` and torch
ops: the fallback for shapes the kernel does not implement, and what tools/microbench_urpc.py times the kernel against."""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from mia_hip import ops


def pyramid_factors(outputs):
    """The integer upsampling factor of every output against outputs[0]; ValueError for anything that is not such a pyramid."""
    outputs = list(outputs)
    if len(outputs) < 2:
        raise ValueError(f"PyramidConsistencyLoss: {len(outputs)} output(s); consistency needs at least two scales")
    if any(o.ndim != 4 for o in outputs):
        raise ValueError(f"PyramidConsistencyLoss: outputs are [N,K,h,w]; got {[tuple(o.shape) for o in outputs]}")
    n, k, hh, ww = outputs[0].shape
    factors = []
    for o in outputs:
        if o.shape[0] != n or o.shape[1] != k:
            raise ValueError(f"PyramidConsistencyLoss: output {tuple(o.shape)} differs from {tuple(outputs[0].shape)} in images or classes")
        h, w = o.shape[-2:]
        if h == 0 or w == 0 or hh % h or ww % w or hh // h != ww // w:
            raise ValueError(f"PyramidConsistencyLoss: an output of {h}x{w} pixels does not divide the main output's {hh}x{ww} by one "
                             f"integer factor")
        factors.append(hh // h)
    return factors


class PyramidConsistencyLoss(nn.Module):
    """`forward(outputs, *, dyn=None)` -> `weight * L`, a 0-dim device tensor; `weight` is `dyn[0]`, read on the device when the
    kernels run (None: 1), so a schedule's ramp never re-builds anything.
    fused: None = the fused kernel wherever it can serve, False = always the tensor-op form, True = raise where the kernel cannot
    serve.  By-products of the latest forward, device tensors, no host sync: `last_value` (the unweighted L) and `last_terms`
    (`[S]`, the per-scale L_s).  There is no CPU fallback: CPU tensors raise `MiaError`."""

    def __init__(self, fused: Optional[bool] = None):
        super().__init__()
        self.fused = fused
        self.last_value = self.last_terms = None

    @staticmethod
    def _why_not_fused(outputs, factors) -> Optional[str]:
        if len(outputs) > ops.URPC_MAX_SCALES:
            return f"{len(outputs)} outputs, the fused kernel implements up to {ops.URPC_MAX_SCALES}"
        if outputs[0].shape[1] > ops.DS_LOSS_MAX_CLASSES:
            return f"{outputs[0].shape[1]} classes, the fused kernel implements up to {ops.DS_LOSS_MAX_CLASSES}"
        for f in factors[1:]:
            if f not in ops.DS_LOSS_FACTORS:
                return f"factor {f} is not one of {ops.DS_LOSS_FACTORS}"
        if any(o.dtype != torch.float32 for o in outputs):
            return "the fused kernel takes fp32 logits"
        if outputs[0].shape[0] * outputs[0].shape[2] * outputs[0].shape[3] >= 1 << 31:
            return "the fused kernel indexes fewer than 2^31 full-resolution pixels"
        return None

    def forward(self, outputs, *, dyn: Optional[torch.Tensor] = None) -> torch.Tensor:
        outputs = list(outputs)
        factors = pyramid_factors(outputs)  # every shape is checked before anything runs
        why = None if self.fused is False else self._why_not_fused(outputs, factors)
        if self.fused and why is not None:
            raise ValueError(f"PyramidConsistencyLoss(fused=True): {why}")
        ops._need_dev(dyn, *outputs)
        if self.fused is not False and why is None:
            loss = ops.PyramidConsistencyFn.apply(dyn, *outputs)
            self.last_value = ops.PyramidConsistencyFn.last_out[1]
            self.last_terms = ops.PyramidConsistencyFn.last_terms
            return loss
        return self._composed(outputs, factors, dyn)

    def _composed(self, outputs, factors, dyn) -> torch.Tensor:
        """The definition, term by term, on full-resolution tensors."""
        from transforms.hip.functional_hip import ResizeBilinearFn
        hh, ww = outputs[0].shape[-2:]
        ups = [o.float() if f == 1 else ResizeBilinearFn.apply(o.float(), hh, ww) for o, f in zip(outputs, factors)]
        ps = [torch.softmax(u, 1) for u in ups]
        lps = [torch.log_softmax(u, 1) for u in ups]
        m = torch.stack(ps).mean(0)
        # xlogy(m, m) with a backward that stays finite where a saturated m_k rounds to 0 (0 / 0 otherwise); same values
        ent = torch.xlogy(m, m.clamp_min(torch.finfo(m.dtype).tiny))
        terms = []
        for p, lp in zip(ps, lps):
            v = (ent - m * lp).sum(1, keepdim=True)
            w = torch.exp(-v)
            terms.append(torch.mean((m - p) ** 2 * w) / (torch.mean(w) + 1e-8) + torch.mean(v))
        terms = torch.stack(terms)
        value = terms.mean()
        self.last_value, self.last_terms = value.detach(), terms.detach()
        return value if dyn is None else value * dyn.detach().reshape(-1)[0]
