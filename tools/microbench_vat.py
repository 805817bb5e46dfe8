#!/usr/bin/env python
"""Time the virtual-adversarial-training pieces on one GPU and write the figures as JSON lines:
  (a) mia_stem_dgrad (csrc/stem_dgrad.hip) at 32 x 512^2 x 64 bf16, 16 x 768^2 x 96 bf16 and 32 x 256^2 x 64 fp32 against
      torch.nn.grad.conv2d_input on the same tensors; bytes moved (dy once + dx once) over time;
  (b) the KL consistency (csrc/vat.hip) forward + backward at 12 x 4 x 256^2 and 8 x 3 x 512^2 channels-last against
      F.kl_div(log_softmax, softmax) with autograd;
  (c) a VATEngine step against a MeanTeacherEngine step on the same network and batch;
  (d) the power pass (VATLoss.adversarial) with and without ops.frozen_parameters;
  (e) the distances of tests/test_gpu_vat_engine.py::test_adversarial_against_the_oracle (computed by that file's own functions).
Every time is the median of --rounds rounds, each the event-timed mean of --inner back-to-back calls, after --warmup rounds; the
variants of one comparison take turns inside every round.

    python tools/microbench_vat.py [--rounds 9] [--inner 10] [--warmup 2] [--out profiles/vat.txt]
"""
import argparse
import contextlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "medical-image-analysis_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def interleaved(fns, rounds, inner, warmup):
    ts = {k: [] for k in fns}
    for r in range(warmup + rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                ts[k].append(e0.elapsed_time(e1) / inner)
    return {k: dict(ms_median=round(float(np.median(v)), 4), ms_min=round(float(min(v)), 4), ms_max=round(float(max(v)), 4), n=len(v))
            for k, v in ts.items()}


def bench_stem_dgrad(a, dev, ops):
    out = []
    for n, hw, c0, dt in ((32, 512, 64, torch.bfloat16), (16, 768, 96, torch.bfloat16), (32, 256, 64, torch.float32)):
        g = torch.Generator().manual_seed(c0 + hw)
        w = (torch.rand(c0, 1, 3, 3, generator=g) - 0.5).to(dev)
        dy = torch.randn(n, hw, hw, c0, device=dev, dtype=dt)  # NHWC storage
        dy_nchw = dy.permute(0, 3, 1, 2)  # the same memory as a channels-last NCHW tensor
        w2 = w.reshape(c0, 9).contiguous()
        dx = torch.empty(n, hw, hw, device=dev)

        def ours():
            ops.call("mia_stem_dgrad", ops._p(dy), ops._dt(dy), ops._p(w2), ops._p(dx), n, hw, hw, c0, ops._stream())

        wt = w.to(dt)

        def theirs():
            return torch.nn.grad.conv2d_input((n, 1, hw, hw), wt, dy_nchw, padding=1)

        res = interleaved({"mia_stem_dgrad": ours, "torch_conv2d_input": theirs}, a.rounds, a.inner, a.warmup)
        ours()
        ref = theirs().float()[:, 0]
        nbytes = dy.numel() * dy.element_size() + dx.numel() * 4
        res.update(workload=f"{n}x{hw}x{hw}x{c0} {'bf16' if dt == torch.bfloat16 else 'fp32'}", bytes_moved=nbytes,
                   gbytes_per_s=round(nbytes / (res["mia_stem_dgrad"]["ms_median"] * 1e-3) / 1e9, 1),
                   speedup_over_torch=round(res["torch_conv2d_input"]["ms_median"] / res["mia_stem_dgrad"]["ms_median"], 2),
                   rel_l2_to_torch=float((dx - ref).norm() / ref.norm()))
        out.append(res)
        del dy, dx, ref
        torch.cuda.empty_cache()
    return out


def bench_kl(a, dev, ops):
    from losses.vat_loss import kl_consistency
    out = []
    for n, k1, hw in ((12, 4, 256), (8, 3, 512)):
        g = torch.Generator().manual_seed(hw)
        z = (torch.randn(n, hw, hw, k1, generator=g) * 2).to(dev).permute(0, 3, 1, 2).requires_grad_(True)
        zt = (torch.randn(n, hw, hw, k1, generator=g) * 2).to(dev).permute(0, 3, 1, 2)

        def ours():
            z.grad = None
            kl_consistency(z, zt, None, "batchmean").backward()

        def theirs():
            z.grad = None
            F.kl_div(F.log_softmax(z, 1), F.softmax(zt, 1), reduction="batchmean").backward()

        res = interleaved({"kl_consistency": ours, "torch_kl_div": theirs}, a.rounds, a.inner, a.warmup)
        ours()
        g1 = z.grad.clone()
        theirs()
        nbytes = z.numel() * 4 * 5  # both tensors in each direction + the gradient
        res.update(workload=f"{n}x{k1}x{hw}x{hw} channels-last", bytes_moved=nbytes,
                   speedup_over_torch=round(res["torch_kl_div"]["ms_median"] / res["kl_consistency"]["ms_median"], 2),
                   grad_max_abs_diff_to_torch=float((g1 - z.grad).abs().max()))
        out.append(res)
    return out


def bench_engines(a, dev, ops):
    from losses.compound_losses import DiceAndCELoss
    from losses.dice_loss import DiceLoss
    from losses.vat_loss import VATLoss
    from models.unet import UNet
    from training.semi import MeanTeacherEngine, VATEngine
    ch, n, lb, hw = [32, 64, 128, 256], 8, 4, 256

    def net(seed):
        torch.manual_seed(seed)
        return UNet(2, 1, 3, ch, normalization="instance", dropout_prob=None).to(dev).set_compute_dtype(torch.bfloat16)

    def sup():
        return DiceAndCELoss(dice_loss=DiceLoss, dice_kwargs=dict(num_classes=2, do_bg=True), ce_loss=torch.nn.CrossEntropyLoss, ce_kwargs={})

    g = torch.Generator().manual_seed(1)
    batch = {"image": torch.rand(n, 1, hw, hw, generator=g).to(dev), "label": torch.randint(0, 3, (lb, hw, hw), generator=g).to(dev)}
    kw = dict(labeled_bs=lb, start_lr=1e-3, lr_warmup_iter=0, num_iters=100000)
    vat_eng = VATEngine(net(1), sup(), **kw)
    mt_eng = MeanTeacherEngine(net(1), net(2), sup(), **kw)
    inner = max(1, a.inner // 3)
    res = interleaved({"VATEngine_step": lambda: vat_eng.train_step(batch), "MeanTeacherEngine_step": lambda: mt_eng.train_step(batch)},
                      a.rounds, inner, a.warmup)
    res.update(workload=f"UNet {ch} bf16, batch {n} ({lb} labelled) x 1 x {hw} x {hw}, ip=1")
    # the power pass alone, parameters frozen (as VATLoss.adversarial runs it) against the same pass with parameter gradients
    model, vat = vat_eng.model.train(), VATLoss()
    x = batch["image"][lb:]
    with torch.no_grad():
        z_clean = model(x)

    def frozen():
        vat.adversarial(model, x, z_clean)

    real = ops.frozen_parameters

    def unfrozen():
        ops.frozen_parameters = lambda m: contextlib.nullcontext(m)
        try:
            vat.adversarial(model, x, z_clean)
        finally:
            ops.frozen_parameters = real
            vat_eng.optimizer.zero_grad()  # drop the claims the parameter gradients left behind

    power = interleaved({"power_pass_frozen": frozen, "power_pass_with_parameter_gradients": unfrozen}, a.rounds, inner, a.warmup)
    power.update(workload=res["workload"] + f", {x.shape[0]} unlabelled images")
    return [res, power]


def distances(dev):
    import test_gpu_vat_engine as T
    from losses.vat_loss import VATLoss
    model = T._net().train()
    x = T._data()[0][:2]
    d0 = torch.rand(x.shape, generator=torch.Generator().manual_seed(4)) - 0.5
    vat = VATLoss(xi=10.0, eps=6.0, ip=1)
    xd = x.to(dev)
    with torch.no_grad():
        z_clean = model(xd)
    x_adv = vat.adversarial(model, xd, z_clean, d0=d0.to(dev))
    with torch.no_grad():
        vat(model(x_adv), z_clean)
    s64, k64 = T._oracle_adversarial(model, x, d0, "instance", torch.float64, 10.0, 6.0)
    s32, k32 = T._oracle_adversarial(model, x, d0, "instance", torch.float32, 10.0, 6.0)
    return dict(workload="test_adversarial_against_the_oracle", step_rel_l2=T._rel((x_adv - xd).cpu(), s64), step_rel_l2_fp32_oracle=T._rel(s32, s64),
                final_kl=float(vat.last_value), final_kl_fp64_oracle=k64, final_kl_rel=abs(float(vat.last_value) - k64) / k64,
                final_kl_rel_fp32_oracle=abs(k32 - k64) / k64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_vat needs a GPU")
    from mia_hip import ops
    dev = torch.device("cuda:0")
    lines = [dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, inner=a.inner, warmup=a.warmup, torch=torch.__version__,
                  timing="device events around `inner` back-to-back calls; the variants of a comparison alternate inside each round",
                  not_measured="kernel times by a profiler; hipGraph capture; more than one rank; ip > 1; any shape other than those below")]
    for part in (bench_stem_dgrad, bench_kl, bench_engines):
        for rec in part(a, dev, ops):
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    lines.append(distances(dev))
    print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(l) for l in lines) + "\n")


if __name__ == "__main__":
    main()
