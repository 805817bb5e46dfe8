#!/usr/bin/env python
"""Time the prediction path on one GPU (csrc/predict.hip, inference/predictor.py, UnetProcessor.denoise_masks):
  denoise : UnetProcessor.denoise_masks (5 / 5 / 7) on 32 x 336 x 544 and 88 x 576 x 576 label maps, the fused kernel against the
            tensor path on the same data (checked equal);
  ensemble: five mia_softmax_accum passes on 32 x 3 x 256 x 256 and 32 x 3 x 512 x 512 logits (planar and the head's layout)
            against the torch expression `sum(l.softmax(1) for l in logits).argmax(1)` in the same run, with the achieved bytes per
            second from the algorithmic byte count;
  end2end : EnsemblePredictor.predict_batch with five [32, 64, 128, 256, 512] networks on 32 x 3 x 336 x 544, and the five forwards
            alone.
  window  : sliding-window prediction, five models x four mirror combinations x every 512 x 512 window at overlap 0.5 -- 180
            mia_window_accum passes into a 1 x 3 x 1024 x 1024 canvas, 80 into 8 x 3 x 768 x 768 -- plus mia_window_finalize, planar
            and head layout, against the torch expression of the same definition in the same run, with the achieved bytes per second
            from the algorithmic byte count; and one EnsemblePredictor.predict_batch with five [32, 64, 128, 256, 512] networks on
            1 x 3 x 1024 x 1024 at patch size 512 with both mirror axes, next to the 180 forwards alone.
Every figure is the median of --iters calls after --warmup, each timed with device events.  The script times what the checkout
has: on a tree without the kernel it times the tensor path alone (the baseline), and it skips the sections whose code is absent.

    python tools/microbench_predict.py [--iters 30] [--warmup 5] [--sections denoise,ensemble,end2end,window] [--out out/predict.json]
"""
import argparse
import inspect
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "medical-image-analysis_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_ACHIEVABLE = 6.3e12  # bytes / s a streaming kernel reaches on this part


def timed(fn, iters, warmup):
    """(median, min, max) ms of fn() over `iters` event-timed calls after `warmup`, and the last result."""
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(float(min(ts)), 4), ms_max=round(float(max(ts)), 4)), out


def label_maps(n, h, w, seed, dev):
    """Two nested noisy ellipses per map with speckles and holes, built on the device: what a network's arg-max looks like."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    yy = torch.arange(h, dtype=torch.float32).view(1, h, 1)
    xx = torch.arange(w, dtype=torch.float32).view(1, 1, w)
    cy, cx = (0.3 + 0.4 * torch.rand(n, 1, 1, generator=g)) * h, (0.3 + 0.4 * torch.rand(n, 1, 1, generator=g)) * w
    a, b = (0.15 + 0.25 * torch.rand(n, 1, 1, generator=g)) * h, (0.15 + 0.25 * torch.rand(n, 1, 1, generator=g)) * w
    r = ((yy - cy) / a) ** 2 + ((xx - cx) / b) ** 2
    out = torch.zeros(n, h, w, dtype=torch.int64)
    out[r < 1.0] = 2
    out[r < 0.35] = 1
    noise = torch.rand(n, h, w, generator=g)
    out = torch.where(noise < 0.01, torch.randint(0, 3, (n, h, w), generator=g), out)
    return out.to(dev)


def bench_denoise(a, dev):
    from models.unet.unet_processor import UnetProcessor
    proc = UnetProcessor()
    has_kernel = "backend" in inspect.signature(proc.denoise_masks).parameters
    rows = []
    for n, h, w in ((32, 336, 544), (88, 576, 576)):
        m = label_maps(n, h, w, 1, dev)
        row = dict(section="denoise", workload=f"{n}x{h}x{w}", sizes=[proc.dilate_size, proc.erode_size, proc.smooth_kernel])
        if has_kernel:
            row["tensor"], ref = timed(lambda: proc.denoise_masks(m, backend="tensor"), a.iters, a.warmup)
            row["kernel"], got = timed(lambda: proc.denoise_masks(m, backend="kernel"), a.iters, a.warmup)
            assert torch.equal(ref, got), "kernel and tensor path differ"
            row["speedup"] = round(row["tensor"]["ms_median"] / row["kernel"]["ms_median"], 1)
            row["gate_5x"] = bool(row["speedup"] >= 5.0)
            row["changed_pixels"] = int((got != m).sum())
        else:
            row["tensor"], _ = timed(lambda: proc.denoise_masks(m), a.iters, a.warmup)
            row["kernel"] = None
        rows.append(row)
    return rows


def bench_ensemble(a, dev):
    try:
        from inference import softmax_accum
    except ImportError:
        return [dict(section="ensemble", absent=True)]
    rows, m_models, k1 = [], 5, 3
    for n, h, w in ((32, 256, 256), (32, 512, 512)):
        for layout in ("planar", "head"):
            g = torch.Generator().manual_seed(h)
            logits = []
            for _ in range(m_models):
                l = (torch.randn(n, k1, h, w, generator=g) * 4).to(dev)
                if layout == "head":
                    l = l.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
                logits.append(l)
            prob = torch.empty(n, k1, h, w, device=dev)
            pred = torch.empty(n, h, w, device=dev, dtype=torch.int64)

            def ours():
                for i, l in enumerate(logits):
                    softmax_accum(l, prob, pred if i == m_models - 1 else None, 1.0, first=i == 0)
                return pred

            row = dict(section="ensemble", workload=f"M{m_models}_{n}x{k1}x{h}x{w}_{layout}")
            row["kernel"], got = timed(ours, a.iters, a.warmup)
            got = got.clone()
            row["torch"], ref = timed(lambda: sum(l.softmax(1) for l in logits).argmax(1), a.iters, a.warmup)
            row["label_mismatch_share"] = float((got != ref).double().mean())  # fp32 against fp32: near-ties may differ
            px = n * h * w
            nbytes = px * (m_models * 4 * k1 + (m_models - 1) * 4 * k1 + m_models * 4 * k1 + 8)  # logits + sum read + sum written + labels
            row["bytes"] = nbytes
            row["tb_per_s"] = round(nbytes / (row["kernel"]["ms_median"] * 1e-3) / 1e12, 3)
            row["fraction_of_achievable_hbm"] = round(nbytes / (row["kernel"]["ms_median"] * 1e-3) / HBM_ACHIEVABLE, 3)
            row["speedup_over_torch"] = round(row["torch"]["ms_median"] / row["kernel"]["ms_median"], 2)
            rows.append(row)
            del logits, prob, pred
    return rows


def bench_end2end(a, dev):
    try:
        from inference import EnsemblePredictor
    except ImportError:
        return [dict(section="end2end", absent=True)]
    pred = EnsemblePredictor(None, device=dev)  # five [32, 64, 128, 256, 512] networks, no resize: 336 x 544 in and out
    for i, net in enumerate(pred.models):
        torch.manual_seed(i)
        net.load_state_dict(type(net)(2, 3, 3, [32, 64, 128, 256, 512]).state_dict())
    from mia_hip import ops
    ops.bump_param_epoch()
    X = (torch.rand(32, 3, 336, 544, generator=torch.Generator().manual_seed(0)) * 255).to(dev)
    x = pred.preprocess(X)

    def forwards():
        with torch.no_grad():
            for net in pred.models:
                out = net(x)
        return out

    iters, warmup = max(3, a.iters // 3), max(2, a.warmup // 2)
    row = dict(section="end2end", workload="5x[32,64,128,256,512]_32x3x336x544")
    row["predict_batch"], _ = timed(lambda: pred.predict_batch(X), iters, warmup)
    row["forwards_only"], _ = timed(forwards, iters, warmup)
    row["share_outside_forwards"] = round(1.0 - row["forwards_only"]["ms_median"] / row["predict_batch"]["ms_median"], 4)
    return [row]


def bench_window(a, dev):
    try:
        from inference import EnsemblePredictor, window_accum, window_finalize, window_starts, window_weights
        from inference.predictor import coverage_1d
    except ImportError:
        return [dict(section="window", absent=True)]
    rows, m_models, k1, ph, pw = [], 5, 3, 512, 512
    combos = [(), (2,), (3,), (2, 3)]
    gy, gx = (torch.from_numpy(window_weights(p)).to(dev) for p in (ph, pw))
    g2d = gy[:, None] * gx[None, :]
    for n, h, w in ((1, 1024, 1024), (8, 768, 768)):
        ys, xs = window_starts(h, ph, 0.5), window_starts(w, pw, 0.5)
        ry = torch.from_numpy((1.0 / coverage_1d(gy.cpu().numpy(), ys, h)).astype(np.float32)).to(dev)
        rx = torch.from_numpy((1.0 / coverage_1d(gx.cpu().numpy(), xs, w)).astype(np.float32)).to(dev)
        jobs = [(1.0 + 0.5 * mi, combo, y0, x0) for mi in range(m_models) for combo in combos for y0 in ys for x0 in xs]
        scale = 1.0 / (len(combos) * sum(1.0 + 0.5 * mi for mi in range(m_models)))
        for layout in ("planar", "head"):
            g = torch.Generator(device=dev).manual_seed(h)
            logits = []
            for _ in jobs:  # one logits tensor per pass, as in a real run: none of them is in cache when its pass starts
                l = torch.randn(n, k1, ph, pw, generator=g, device=dev) * 4
                if layout == "head":
                    l = l.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
                logits.append(l)
            canvas = torch.empty(n, k1, h, w, device=dev)
            pred = torch.empty(n, h, w, device=dev, dtype=torch.int64)

            def ours():
                canvas.zero_()
                for l, (wt, combo, y0, x0) in zip(logits, jobs):
                    window_accum(l, canvas, gy, gx, y0, x0, wt, 2 in combo, 3 in combo)
                window_finalize(canvas, pred, ry, rx, scale, normalise=True)
                return pred

            def tensor_ops():
                c = torch.zeros(n, k1, h, w, device=dev)
                for l, (wt, combo, y0, x0) in zip(logits, jobs):
                    p = wt * l.softmax(1)
                    c[:, :, y0:y0 + ph, x0:x0 + pw] += g2d * (p.flip(combo) if combo else p)
                labels = c.argmax(1)
                c *= (scale * ry)[:, None] * rx[None, :]
                return labels, c

            row = dict(section="window", workload=f"M{m_models}_mirror4_{len(ys) * len(xs)}win_{n}x{k1}x{h}x{w}_{layout}", passes=len(jobs))
            row["kernel"], got = timed(ours, a.iters, a.warmup)
            got, probs = got.clone(), canvas.clone()
            row["torch"], (ref, ref_probs) = timed(tensor_ops, a.iters, a.warmup)
            row["label_mismatch_share"] = float((got != ref).double().mean())  # fp32 against fp32: near-ties may differ
            row["max_prob_diff"] = float((probs - ref_probs).abs().max())
            nbytes = len(jobs) * n * ph * pw * 3 * 4 * k1 + n * h * w * (2 * 4 * k1 + 8)  # logits + canvas read + written; finalize
            row["bytes"] = nbytes
            row["tb_per_s"] = round(nbytes / (row["kernel"]["ms_median"] * 1e-3) / 1e12, 3)
            row["fraction_of_achievable_hbm"] = round(nbytes / (row["kernel"]["ms_median"] * 1e-3) / HBM_ACHIEVABLE, 3)
            row["speedup_over_torch"] = round(row["torch"]["ms_median"] / row["kernel"]["ms_median"], 2)
            rows.append(row)
            del logits, canvas, pred, probs, ref_probs
    pred = EnsemblePredictor(None, device=dev, patch_size=(ph, pw), mirror_axes=(2, 3), window_batch=3)
    for i, net in enumerate(pred.models):
        torch.manual_seed(i)
        net.load_state_dict(type(net)(2, 3, 3, [32, 64, 128, 256, 512]).state_dict())
    from mia_hip import ops
    ops.bump_param_epoch()
    X = (torch.rand(1, 3, 1024, 1024, generator=torch.Generator().manual_seed(0)) * 255).to(dev)
    patches = pred.preprocess(X)[:, :, :ph, :pw].repeat(3, 1, 1, 1).contiguous()

    def forwards():  # the same 60 forwards of three stacked windows, nothing else
        with torch.no_grad():
            for net in pred.models:
                for _ in range(4 * 3):
                    out = net(patches)
        return out

    iters, warmup = max(3, a.iters // 6), 2
    row = dict(section="window", workload="predict_batch_5x[32,64,128,256,512]_1x3x1024x1024_patch512_mirror4_wb3")
    row["predict_batch"], _ = timed(lambda: pred.predict_batch(X), iters, warmup)
    row["forwards_only"], _ = timed(forwards, iters, warmup)
    row["share_outside_forwards"] = round(1.0 - row["forwards_only"]["ms_median"] / row["predict_batch"]["ms_median"], 4)
    rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sections", default="denoise,ensemble,end2end,window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_predict needs a GPU")
    dev = torch.device("cuda:0")
    rows = []
    for name, fn in (("denoise", bench_denoise), ("ensemble", bench_ensemble), ("end2end", bench_end2end), ("window", bench_window)):
        if name in a.sections.split(","):
            for r in fn(a, dev):
                rows.append(r)
                print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), argv=sys.argv[1:], rows=rows), fh, indent=1)
    if any(r.get("gate_5x") is False for r in rows):
        raise SystemExit("the fused denoise is not 5x faster than the tensor path on every workload")


if __name__ == "__main__":
    main()
