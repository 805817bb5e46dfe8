#!/usr/bin/env python
"""Time the mean-teacher pieces on one GPU (csrc/consistency.hip, losses/consistency_loss.py, training/semi.py) on

  24 x 4 x 256 x 256 with 12 labelled images (ACDC) and 16 x 3 x 512 x 512 with 8 labelled,

against the torch expressions of the same definitions.  Arms, alternating inside every round on the same seeded data, in a new
seeded order each round (no arm always inherits the host state one predecessor leaves), every arm started on an idle device, device
events around each -- so an arm's time includes the host's path between its launches, which at these sizes is most of the loss
arms' time (kernel times: `rocprofv3 --kernel-trace --stats`):
  loss_plain / torch_plain     forward + backward of the consistency term on the unlabelled half of channels-last fp32 logits
                               (a batch slice z[lb:]), Mean Teacher form: `torch.mean((softmax(zs,1) - softmax(zt,1))**2)`
  loss_masked / torch_masked   the same with the UA-MT mask at 0.875 ln K: `sum(mask * dist) / (2 * sum(mask) + 1e-16)`
  ema / torch_ema              the EMA over the flat parameter buffer of the al_train-sized UNet: `t.mul_(a).add_(s, alpha=1-a)`
  step / torch_step            one whole `MeanTeacherEngine.train_step` (al_train-sized UNet, instance norm, Dice + CE, plain form)
                               against the same engine with the consistency term and the EMA as those tensor ops
Also recorded: on the first two unlabelled images the largest ratio of the value / gradient error to the bounds of
tests/test_gpu_consistency.py, and the bytes the kernels move per pixel.

    python tools/microbench_consistency.py [--rounds 7] [--warmup 2] [--out profiles/consistency.txt]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "medical-image-analysis_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

NOT_MEASURED = ("hipGraph capture of the mean-teacher step (it runs eagerly); more than one rank; bf16 compute; uncertainty passes "
                "inside the whole-step arm (their cost is T more teacher forwards plus one mia_softmax_accum each); batch-norm models; "
                "planar logits (the head writes channels-last); any shape other than the two above")


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()  # every arm starts on an idle device, whatever ran before it
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def stats(ts):
    return dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(float(min(ts)), 4), ms_max=round(float(max(ts)), 4), n=len(ts))


def torch_plain(zs, zt):
    return torch.mean((torch.softmax(zs, 1) - torch.softmax(zt, 1)) ** 2)


def torch_masked(zs, zt, pbar, thr):
    dist = ((torch.softmax(zs, 1) - torch.softmax(zt, 1)) ** 2).sum(1, keepdim=True)
    mask = (-(pbar * torch.log(pbar + 1e-6)).sum(1, keepdim=True) < thr).float()
    return torch.sum(mask * dist) / (2 * torch.sum(mask) + 1e-16)


class TorchConsistency(torch.nn.Module):
    """SoftmaxMSEConsistency's call signature on tensor ops (the whole-step comparator)."""

    def forward(self, zs, zt, pbar=None, *, dyn=None):
        loss = torch_plain(zs, zt) if pbar is None else torch_masked(zs, zt, pbar, dyn[1])
        self.last_value, self.last_kept = loss.detach(), None
        return loss * dyn[0]


def accuracy(zs, zt, pbar, thr, nimg=2):
    """Largest error / bound of value and gradient on the first `nimg` images (bounds of tests/test_gpu_consistency.py)."""
    import _consistency_ref as R
    from mia_hip import ops
    out = {}
    for name, pb in (("plain", None), ("masked", pbar)):
        zz = zs[:nimg].detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
        dyn = torch.tensor([1.0, thr], device=zs.device)
        ops.ConsistencyFn.apply(zz, zt[:nimg], None if pb is None else pb[:nimg].contiguous(), dyn, 2.0).backward()
        keep = None if pb is None else ops.ConsistencyFn.last_keep.cpu().numpy().astype(bool)
        ref = R.evaluate(zz.detach().cpu().numpy(), zt[:nimg].cpu().numpy(), keep)
        value = float(ops.ConsistencyFn.last_out[1].item())
        out[name + "_value_err_over_bound"] = round(abs(value - ref["value"]) / (2e-6 * ref["value_mag"]), 4)
        out[name + "_grad_err_over_bound"] = round(float((np.abs(zz.grad.cpu().numpy() - ref["grad"]) / (2e-6 * ref["grad_mag"] + 1e-12)).max()), 4)
    return out


def make_engine(k1, lb, torch_ops):
    from losses.compound_losses import DiceAndCELoss
    from models.unet import UNet
    from training.semi import MeanTeacherEngine

    class TorchEngine(MeanTeacherEngine):
        def _ema(self, alpha):
            self.teacher_flat.mul_(alpha).add_(self.optimizer.flat_param, alpha=1.0 - alpha)

    torch.manual_seed(0)
    nets = [UNet(2, 1, k1, [32, 64, 128, 256, 512], normalization="instance").cuda() for _ in range(2)]
    sup = DiceAndCELoss(dice_kwargs=dict(num_classes=k1 - 1, do_bg=True))
    cls = TorchEngine if torch_ops else MeanTeacherEngine
    return cls(nets[0], nets[1], sup, labeled_bs=lb, consistency=TorchConsistency() if torch_ops else None, consistency_weight=0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_consistency needs a GPU")
    from losses.consistency_loss import SoftmaxMSEConsistency
    from mia_hip import ops
    dev = torch.device("cuda:0")
    lines = [json.dumps(dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, warmup=a.warmup, torch=torch.__version__,
                             logits="fp32 channels-last, the unlabelled batch slice", not_measured=NOT_MEASURED))]
    print(lines[0], flush=True)
    for n, k1, h, w, lb in ((24, 4, 256, 256, 12), (16, 3, 512, 512, 8)):
        g = torch.Generator().manual_seed(n)
        full = (torch.randn(n, h, w, k1, generator=g) * 2).to(dev).permute(0, 3, 1, 2).requires_grad_(True)
        zt = (full.detach()[lb:] + torch.randn(n - lb, h, w, k1, generator=g).to(dev).permute(0, 3, 1, 2)).contiguous(memory_format=torch.channels_last)
        pbar = torch.stack([torch.softmax(zt + torch.randn(zt.shape, generator=g).to(dev), 1) for _ in range(4)]).mean(0).contiguous()
        thr = 0.875 * math.log(k1)
        dyn = torch.tensor([1.0, thr], device=dev)
        loss = SoftmaxMSEConsistency(k1 - 1)
        engines = {"step": make_engine(k1, lb, False), "torch_step": make_engine(k1, lb, True)}
        batch = {"image": torch.rand(n, 1, h, w, generator=g).to(dev), "label": torch.randint(0, k1, (lb, h, w), generator=g).to(dev)}
        nparam = engines["step"].optimizer.flat_param.numel()
        tflat = torch.randn(nparam, generator=g).to(dev)
        sflat = torch.randn(nparam, generator=g).to(dev)

        def fwd_bwd(fn):
            full.grad = None
            fn(full[lb:]).backward()
            return full.grad

        arms = {
            "loss_plain": lambda: fwd_bwd(lambda zs: loss(zs, zt)),
            "torch_plain": lambda: fwd_bwd(lambda zs: torch_plain(zs, zt)),
            "loss_masked": lambda: fwd_bwd(lambda zs: loss(zs, zt, pbar, dyn=dyn)),
            "torch_masked": lambda: fwd_bwd(lambda zs: torch_masked(zs, zt, pbar, thr)),
            "ema": lambda: ops.ema_update(tflat, sflat, 0.99),
            "torch_ema": lambda: tflat.mul_(0.99).add_(sflat, alpha=1.0 - 0.99),
            "step": lambda: engines["step"].train_step(batch),
            "torch_step": lambda: engines["torch_step"].train_step(batch),
        }
        times = {k: [] for k in arms}
        outs = {}
        order = np.random.default_rng(n)
        for r in range(a.warmup + a.rounds):  # the arms alternate inside every round, in a new seeded order each round
            for k in order.permutation(list(arms)):
                ms, out = event_ms(arms[k])
                if k.startswith(("loss_", "torch_plain", "torch_masked")):
                    outs[k] = out.clone()
                if r >= a.warmup:
                    times[k].append(ms)
        px = (n - lb) * h * w
        row = dict(workload=f"{n}x{k1}x{h}x{w}", labelled=lb, flat_params=nparam, **{k: stats(v) for k, v in times.items()})
        for kind in ("plain", "masked"):
            row[f"{kind}_grad_max_abs_diff_to_torch_expr"] = float((outs["loss_" + kind] - outs["torch_" + kind]).abs().max())
            row[f"{kind}_speedup_over_torch_expr"] = round(row["torch_" + kind]["ms_median"] / row["loss_" + kind]["ms_median"], 2)
        nbytes = px * ((3 * k1 * 4 + 1) + (3 * k1 * 4 + 1))  # forward: zs, zt, pbar in, keep out; backward: zs, zt, keep in, dzs out
        row["masked_bytes_moved"] = nbytes
        row["masked_gbytes_per_s"] = round(nbytes / (row["loss_masked"]["ms_median"] * 1e-3) / 1e9, 1)
        row["ema_speedup_over_torch"] = round(row["torch_ema"]["ms_median"] / row["ema"]["ms_median"], 2)
        row["ema_gbytes_per_s"] = round(12.0 * nparam / (row["ema"]["ms_median"] * 1e-3) / 1e9, 1)
        row["step_speedup_over_torch_ops"] = round(row["torch_step"]["ms_median"] / row["step"]["ms_median"], 3)
        row.update(accuracy(full[lb:], zt, pbar, thr))
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        del engines, outs, full, zt, pbar
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
