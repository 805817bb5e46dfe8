#!/usr/bin/env python
"""Time the batched BADGE gradient embeddings on one GPU (csrc/badge_embed.hip, activelearning.scores.badge_embeddings,
BADGESelector(embed_batch_size=...)):
  kernel : mia_badge_embed alone (its four launches) on 32 x 3 x 512 x 512 logits with 64-channel bf16 features and on
           32 x 4 x 256 x 256 with 32-channel fp32 features, logits in the head's layout; bytes = features once + logits twice,
           over the median time, as a fraction of the achievable HBM rate;
  end2end: BADGESelector.cal_scores over a 64-image synthetic pool, the per-image autograd path (batch_size=1, the only path before
           this kernel) against the fused path at embed_batch_size=32, on cfg4's model (256 x 256, fp32) and cfg3's (512 x 512, bf16):
           images per second for both, their ratio, and the largest difference between the two sets of embeddings.
Kernel figures are medians of --iters event-timed calls after --warmup; end-to-end figures are medians of --repeats host-clock
timings of calls that end in the copy of the embeddings to the host, after one warm-up call of each path.

    python tools/microbench_badge.py [--iters 30] [--warmup 5] [--repeats 3] [--sections kernel,end2end] [--out out/badge.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "medical-image-analysis_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_ACHIEVABLE = 6.3e12  # bytes / s a streaming kernel reaches on this part


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def bench_kernel(a, dev):
    from activelearning.scores import badge_embeddings, badge_slabs
    from mia_hip import ops
    rows = []
    for b, k1, c0, size, dtype in ((32, 3, 64, 512, torch.bfloat16), (32, 4, 32, 256, torch.float32)):
        g = torch.Generator().manual_seed(1)
        feat = torch.randn(b, size, size, c0, generator=g).to(dev).to(dtype)
        weight = (torch.randn(k1, c0, 1, 1, generator=g) * (3.0 / c0 ** 0.5)).to(dev)
        with torch.no_grad():
            logits = ops.HeadFn.apply(feat, weight, torch.zeros(k1, device=dev))
        med, lo, hi = timed(lambda: badge_embeddings(logits, feat, 1e-5, True, False), a.iters, a.warmup)
        nbytes = feat.numel() * feat.element_size() + 2 * logits.numel() * 4
        rate = nbytes / (med * 1e-3)
        rows.append(dict(workload=f"{b}x{k1}x{size}x{size} logits, {c0}ch {str(dtype)[6:]} features",
                         slabs_per_image=badge_slabs(size * size, k1, c0, dtype), ms_median=round(med, 4), ms_min=round(lo, 4),
                         ms_max=round(hi, 4), bytes=nbytes, tb_per_s=round(rate / 1e12, 3), of_achievable=round(rate / HBM_ACHIEVABLE, 3)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


class _DS(torch.utils.data.Dataset):
    def __init__(self, images):
        self.images, self.image_idx = images, [f"case_{i:03d}" for i in range(len(images))]

    def __len__(self):
        return len(self.image_idx)

    def __getitem__(self, i):
        return {"image": self.images[i], "case_name": self.image_idx[i]}


class _Pool:
    def __init__(self, images):
        self.pool_dataset = _DS(images)

    def get_size(self):
        return 1, len(self.pool_dataset)

    def get_pool_dataset(self):
        return self.pool_dataset


def bench_end2end(a, dev):
    from activelearning import BADGESelector
    from losses.compound_losses import DiceAndCELoss
    from models.unet import UNet
    rows = []
    for name, channels, size, dt, norm in (("cfg4 model", [32, 64, 128, 256, 512], 256, torch.float32, "batch"),
                                           ("cfg3 model", [64, 128, 256, 512, 1024], 512, torch.bfloat16, "instance")):
        torch.manual_seed(0)
        model = UNet(2, 1, 3, channels, normalization=norm, dropout_prob=None).to(dev).set_compute_dtype(dt)
        g = torch.Generator().manual_seed(2)
        pool = _Pool(torch.rand(64, 1, size, size, generator=g))
        loss = DiceAndCELoss(dice_kwargs=dict(num_classes=2, do_bg=True), ce_loss=torch.nn.CrossEntropyLoss)
        kw = dict(dice_loss=loss.dice_loss, ce_loss=loss.ce_loss, batch_size=1, num_workers=0, pin_memory=False)
        sels = {"per_image": BADGESelector(**kw), "fused": BADGESelector(embed_batch_size=32, **kw)}
        assert sels["fused"].embed_path(model) == "fused", sels["fused"].embed_path_reason
        secs, embeds = {}, {}
        for key, sel in sels.items():
            sel.cal_scores(pool, model, dev)  # warm-up: code objects, allocator
            ts = []
            for _ in range(a.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, embeds[key] = sel.cal_scores(pool, model, dev)
                ts.append(time.perf_counter() - t0)
            secs[key] = float(np.median(ts))
        scale = float(np.abs(embeds["per_image"]).max())
        rows.append(dict(workload=f"{name} {channels} {size}x{size} {str(dt)[6:]} {norm} norm, 64-image pool",
                         per_image_images_per_s=round(64 / secs["per_image"], 1), fused_images_per_s=round(64 / secs["fused"], 1),
                         ratio=round(secs["per_image"] / secs["fused"], 2),
                         max_abs_diff_over_max_abs=float(np.abs(embeds["fused"] - embeds["per_image"]).max() / scale)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sections", default="kernel,end2end")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("microbench_badge.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0)}
    sections = a.sections.split(",")
    if "kernel" in sections:
        out["kernel"] = bench_kernel(a, dev)
    if "end2end" in sections:
        out["end2end"] = bench_end2end(a, dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
