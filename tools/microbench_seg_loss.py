#!/usr/bin/env python
"""Time the fold-trainer losses on one GPU (csrc/seg_loss.hip), forward + backward, at 32 x 3 x 512 x 512 channels-last (the head's
layout at the headline shape) and 16 x 3 x 768 x 768:
  (a) DiceCEFn          : the al_train loss (Dice + CE, no mask) -- the yardstick, timed in the same process;
  (b) SegLossFn         : DC_and_CE_loss({"smooth": 1e-5, "do_bg": False}, {}, ignore_label=255) without and with a 20 % ignore mask,
                          int64 and uint8 labels; (a) and (b) are timed in interleaved rounds;
  (c) tensor ops        : the same loss composed from torch tensor ops in fp32 on the GPU (the restatement's formulas);
  (d) TopKCEFn          : TopKLoss(k=10) against torch.topk on the per-pixel CE (F.cross_entropy(reduction="none")).
Every figure is the median of --rounds rounds, each the event-timed mean of --inner back-to-back forward + backward calls, after
--warmup rounds.

    python tools/microbench_seg_loss.py [--rounds 15] [--inner 10] [--warmup 3] [--out profiles/seg_loss.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "medical-image-analysis_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

IGN = 255


def interleaved(fns, rounds, inner, warmup):
    """{name: (median, min, max) ms per call}: the variants take turns inside every round, so clock drift hits all alike."""
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
    return {k: dict(ms_median=round(float(np.median(v)), 4), ms_min=round(float(min(v)), 4), ms_max=round(float(max(v)), 4))
            for k, v in ts.items()}


def tensor_dc_ce(x, y, smooth=1e-5):
    """DC_and_CE_loss(do_bg=False, ignore_label=255) from tensor ops, fp32: the composition a user would write without the kernel."""
    mask = y != IGN
    safe = torch.where(mask, y, 0)
    p = torch.softmax(x, 1)
    onehot = torch.zeros_like(x, dtype=torch.bool).scatter_(1, safe, 1)
    oh, pm = onehot[:, 1:] * mask, p[:, 1:] * mask
    inter, sp, sg = (pm * oh).sum((2, 3)), pm.sum((2, 3)), oh.sum((2, 3))
    dc = -((2 * inter + smooth) / torch.clip(sg + sp + smooth, 1e-8)).mean()
    ce = F.cross_entropy(x, y[:, 0], ignore_index=IGN)
    return ce + dc


def step(fn, x):
    def run():
        x.grad = None
        fn().backward()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_seg_loss needs a GPU")
    from losses.ce_loss import TopKLoss
    from losses.compound_losses import DC_and_CE_loss, DiceAndCELoss
    dev = torch.device("cuda:0")
    lines = [f"# {torch.cuda.get_device_name(0)}; forward + backward per call; median [min, max] ms over {a.rounds} interleaved rounds "
             f"of {a.inner} calls"]
    for n, k1, h, w in ((32, 3, 512, 512), (16, 3, 768, 768)):
        g = torch.Generator().manual_seed(h)
        x = (torch.randn(n, k1, h, w, generator=g) * 2).to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)
        y = torch.randint(0, k1, (n, 1, h, w), generator=g)
        ym = torch.where(torch.rand(n, 1, h, w, generator=g) < 0.2, torch.tensor(IGN), y)
        y, ym = y.to(dev), ym.to(dev)
        y8, ym8 = y.to(torch.uint8), ym.to(torch.uint8)
        old = DiceAndCELoss(dice_kwargs=dict(num_classes=k1 - 1, do_bg=False))
        new = DC_and_CE_loss({"smooth": 1e-5, "do_bg": False}, {}, ignore_label=IGN)
        topk = TopKLoss(ignore_index=IGN, k=10)
        n_top = int(n * h * w * 10 / 100)

        def torch_topk():
            res = F.cross_entropy(x, ym[:, 0], ignore_index=IGN, reduction="none")
            return torch.topk(res.view(-1), n_top, sorted=False)[0].mean()

        fns = {
            "a_DiceCEFn_int64": step(lambda: old(x, y[:, 0]), x),
            "b_SegLossFn_int64_nomask": step(lambda: new(x, y), x),
            "b_SegLossFn_uint8_nomask": step(lambda: new(x, y8), x),
            "b_SegLossFn_int64_mask20": step(lambda: new(x, ym), x),
            "b_SegLossFn_uint8_mask20": step(lambda: new(x, ym8), x),
        }
        res = interleaved(fns, a.rounds, a.inner, a.warmup)
        slow = {
            "c_tensor_ops_mask20": step(lambda: tensor_dc_ce(x, ym), x),
            "d_TopKCEFn_k10_uint8": step(lambda: topk(x, ym8), x),
            "d_torch_topk_k10": step(torch_topk, x),
        }
        res.update(interleaved(slow, max(3, a.rounds // 3), max(2, a.inner // 3), 1))
        # same numbers from both compositions (fp32 against fp32)
        v_new, v_ref = new(x, ym).item(), tensor_dc_ce(x, ym).item()
        t_new, t_ref = topk(x, ym8).item(), torch_topk().item()
        base = res["a_DiceCEFn_int64"]["ms_median"]
        nbytes = n * h * w * (3 * 4 * k1 + 2 * 8)  # logits twice + gradient once + int64 labels twice
        lines.append(f"## {n} x {k1} x {h} x {w} channels-last")
        for k, v in res.items():
            lines.append(f"{k:28s} {v['ms_median']:9.4f} [{v['ms_min']:.4f}, {v['ms_max']:.4f}] ms")
        for k in ("b_SegLossFn_int64_nomask", "b_SegLossFn_uint8_nomask", "b_SegLossFn_int64_mask20", "b_SegLossFn_uint8_mask20"):
            lines.append(f"ratio {k} / a = {res[k]['ms_median'] / base:.3f}")
        lines.append(f"(a) moves {nbytes / 1e6:.1f} MB per call: {nbytes / (base * 1e-3) / 1e12:.2f} TB/s")
        lines.append(f"speedup of (b int64 mask20) over (c) tensor ops: {res['c_tensor_ops_mask20']['ms_median'] / res['b_SegLossFn_int64_mask20']['ms_median']:.1f}x")
        lines.append(f"speedup of (d) TopKCEFn over torch.topk: {res['d_torch_topk_k10']['ms_median'] / res['d_TopKCEFn_k10_uint8']['ms_median']:.1f}x")
        lines.append(f"values: SegLossFn {v_new:.6f} tensor ops {v_ref:.6f}; TopKCEFn {t_new:.6f} torch.topk {t_ref:.6f}")
        print("\n".join(lines[-14:]), flush=True)
        del x, y, ym, y8, ym8
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
