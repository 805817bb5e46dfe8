#!/usr/bin/env python
"""Time the pyramid consistency loss (URPC; csrc/urpc.hip, losses/pyramid_consistency.py) on one GPU, forward + backward through
every scale's logits, in the same interleaved rounds:
  (a) composed : PyramidConsistencyLoss(fused=False) -- ResizeBilinearFn per low-resolution scale, then the definition from torch ops
                 on S full-resolution [N, K, H, W] tensors, with autograd keeping what its backward needs;
  (b) fused    : PyramidConsistencyLoss(fused=True) -- ops.PyramidConsistencyFn, the logits of every scale and 3 S sums only.
Shapes: 12 x 4-class unlabelled images at 256^2 with factors (1, 2, 4, 8) and 8 x 3-class at 512^2 with factors (1, 2, 4, 8, 16);
channels-last fp32 logits (the heads' layout), weight read from a device buffer.
Every figure is the median of --rounds rounds, each the event-timed mean of --inner back-to-back calls, after --warmup rounds: a call
is timed as a user times it, the host's path to the launches included.  Also recorded: the two values, the largest difference
between the two gradients relative to the largest gradient, and the peak of newly allocated device memory during one call.

    python tools/microbench_urpc.py [--rounds 15] [--inner 20] [--warmup 3] [--out profiles/urpc.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "medical-image-analysis_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from microbench_seg_loss import interleaved  # noqa: E402

SHAPES = ((12, 4, 256, (1, 2, 4, 8)), (8, 3, 512, (1, 2, 4, 8, 16)))  # unlabelled images, classes, full side, factors


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_urpc needs a GPU")
    from losses.pyramid_consistency import PyramidConsistencyLoss
    dev = torch.device("cuda:0")
    lines = [f"# {torch.cuda.get_device_name(0)}; forward + backward of the pyramid consistency term per call; median [min, max] ms over "
             f"{a.rounds} interleaved rounds of {a.inner} calls"]
    for n, k1, side, factors in SHAPES:
        g = torch.Generator().manual_seed(side + k1)
        base = torch.randn(n, k1, side // max(factors), side // max(factors), generator=g) * 3  # the scales agree roughly, as heads do
        zs = []
        for f in factors:
            z = torch.nn.functional.interpolate(base, size=(side // f, side // f), mode="bilinear", align_corners=False)
            z = z + torch.randn(z.shape, generator=g)
            zs.append(z.to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True))
        dyn = torch.tensor([0.1, 0.0], device=dev)
        losses = {"a_composed": PyramidConsistencyLoss(fused=False), "b_fused": PyramidConsistencyLoss(fused=True)}

        def step(fn):
            def run():
                for z in zs:
                    z.grad = None
                fn(zs, dyn=dyn).backward()
            return run

        res = interleaved({k: step(v) for k, v in losses.items()}, a.rounds, a.inner, a.warmup)
        values, grads, peaks = {}, {}, {}
        for k, fn in losses.items():
            for z in zs:
                z.grad = None  # so that the peak counts the gradients the call returns as well as its temporaries
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            step(fn)()
            torch.cuda.synchronize()
            peaks[k] = (torch.cuda.max_memory_allocated() - before) / 2 ** 20
            values[k] = fn.last_value.item()
            grads[k] = [z.grad.clone() for z in zs]
        top = max(gr.abs().max().item() for gr in grads["a_composed"])
        diff = max((x - y).abs().max().item() for x, y in zip(grads["a_composed"], grads["b_fused"]))
        lines.append(f"## {n} x {k1} x {side}^2, factors {factors}, channels-last fp32 logits")
        for k, v in res.items():
            lines.append(f"{k:12s} {v['ms_median']:9.4f} [{v['ms_min']:.4f}, {v['ms_max']:.4f}] ms   peak new memory {peaks[k]:8.1f} MiB")
        lines.append(f"ratio a / b = {res['a_composed']['ms_median'] / res['b_fused']['ms_median']:.2f}")
        lines.append(f"values: composed {values['a_composed']:.7f} fused {values['b_fused']:.7f}; largest gradient difference / largest "
                     f"gradient = {diff / top:.2e}")
        print("\n".join(lines[-5:]), flush=True)
        del zs, grads
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
