#!/usr/bin/env python
"""Time the deep-supervision loss of ONE auxiliary head (csrc/ds_loss.hip) on one GPU, forward + backward, against the composition
it replaces, in the same interleaved rounds:
  (a) composition      : DiceCEFn(ResizeBilinearFn(z)) -- the bilinear resize writes the full-resolution logits, the loss reads them
                         twice and writes their gradient, the resize's backward scatters it with float atomics;
  (b) UpsampleDiceCEFn : the fused op, low-resolution logits and full-resolution labels only;
  (c) DiceCEFn         : the loss alone on full-resolution logits of the same size (what the main output costs), as a yardstick.
Shapes: 32 x 3 logits at 128^2 -> 512^2 (factor 4) and 256^2 -> 512^2 (factor 2), 16 x 3 at 192^2 -> 768^2 and 384^2 -> 768^2, plus
factor 8 and 16 at 512^2; channels-last logits (the head's layout), int64 labels.
Every figure is the median of --rounds rounds, each the event-timed mean of --inner back-to-back calls, after --warmup rounds.

    python tools/microbench_ds_loss.py [--rounds 15] [--inner 10] [--warmup 3] [--out profiles/ds_loss.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "medical-image-analysis_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from microbench_seg_loss import interleaved, step  # noqa: E402

SHAPES = ((32, 3, 128, 4), (32, 3, 256, 2), (16, 3, 192, 4), (16, 3, 384, 2), (32, 3, 64, 8), (32, 3, 32, 16))  # images, classes, low side, factor


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_ds_loss needs a GPU")
    from mia_hip import ops
    from transforms.hip.functional_hip import ResizeBilinearFn
    dev = torch.device("cuda:0")
    flags = ops.loss_flags(True, True, False, False)
    lines = [f"# {torch.cuda.get_device_name(0)}; forward + backward of one auxiliary head's loss per call; median [min, max] ms over "
             f"{a.rounds} interleaved rounds of {a.inner} calls"]
    for n, k1, side, f in SHAPES:
        full = side * f
        g = torch.Generator().manual_seed(side * 100 + f)
        cl = lambda t: t.to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        z = cl(torch.randn(n, k1, side, side, generator=g) * 2).requires_grad_(True)
        big = cl(torch.randn(n, k1, full, full, generator=g) * 2).requires_grad_(True)
        y = torch.randint(0, k1, (n, full, full), generator=g).to(dev)
        fns = {
            "a_resize_then_DiceCEFn": step(lambda: ops.DiceCEFn.apply(ResizeBilinearFn.apply(z, full, full), y, flags, 1e-5, 1.0, 1.0, 0), z),
            "b_UpsampleDiceCEFn": step(lambda: ops.UpsampleDiceCEFn.apply(z, y, f, flags, 1e-5, 1.0, 1.0, 0), z),
            "c_DiceCEFn_full_resolution": step(lambda: ops.DiceCEFn.apply(big, y, flags, 1e-5, 1.0, 1.0, 0), big),
        }
        res = interleaved(fns, a.rounds, a.inner, a.warmup)
        va = ops.DiceCEFn.apply(ResizeBilinearFn.apply(z, full, full), y, flags, 1e-5, 1.0, 1.0, 0).item()
        vb = ops.UpsampleDiceCEFn.apply(z, y, f, flags, 1e-5, 1.0, 1.0, 0).item()
        lines.append(f"## {n} x {k1} x {side}^2 -> {full}^2 (factor {f}), channels-last, int64 labels")
        for k, v in res.items():
            lines.append(f"{k:28s} {v['ms_median']:9.4f} [{v['ms_min']:.4f}, {v['ms_max']:.4f}] ms")
        lines.append(f"ratio a / b = {res['a_resize_then_DiceCEFn']['ms_median'] / res['b_UpsampleDiceCEFn']['ms_median']:.2f}; "
                     f"b / c = {res['b_UpsampleDiceCEFn']['ms_median'] / res['c_DiceCEFn_full_resolution']['ms_median']:.2f}")
        lines.append(f"values: composition {va:.6f} fused {vb:.6f}")
        print("\n".join(lines[-6:]), flush=True)
        del z, big, y
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
