#!/usr/bin/env python
"""Time the cross-pseudo-supervision term on one GPU (csrc/cps.hip, losses/cross_pseudo.py) on the unlabelled halves that
profiles/consistency.txt uses,

  12 x 4 x 256 x 256 (of a batch of 24, ACDC) and 8 x 3 x 512 x 512 (of a batch of 16), channels-last fp32 logits of two networks,

against the torch expression of the same definition at tau = 0:

  ya = softmax(za, 1).argmax(1); yb = softmax(zb, 1).argmax(1); F.cross_entropy(za, yb) + F.cross_entropy(zb, ya)

Arms, alternating inside every round on the same seeded data, in a new seeded order each round, every arm started on an idle
device, device events around each -- so an arm's time includes the host's path between its launches, as a user times a call:
  loss_cps / torch_cps     forward + backward through autograd; both logits tensors are batch slices z[lb:] and get a gradient
  kernels                  mia_cps_fwd + mia_cps_bwd called back to back on preallocated buffers, CALLS times inside one pair of
                           events, divided by CALLS: the kernels alone (forward, finalize, backward), no autograd, no allocation
Also recorded: peak newly allocated device memory of one forward + backward of either arm, the largest difference between the two
arms' gradients, and on the first two images the largest ratio of the value / gradient error to the bounds of tests/test_gpu_cps.py.

    python tools/microbench_cps.py [--rounds 7] [--warmup 2] [--out profiles/cps.txt]
"""
import argparse
import ctypes
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

CALLS = 20
NOT_MEASURED = ("the whole CPSEngine step; tau > 0; planar logits (the head writes channels-last); hipGraph capture; more than one "
                "rank; any shape other than the two above; kernel times by a profiler (the `kernels` arm is timed by events)")


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


def torch_cps(za, zb):
    ya, yb = torch.softmax(za.detach(), 1).argmax(1), torch.softmax(zb.detach(), 1).argmax(1)
    return F.cross_entropy(za, yb) + F.cross_entropy(zb, ya)


def peak_new_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def accuracy(za, zb, nimg=2):
    """Largest error / bound of values and gradients on the first `nimg` images (bounds of tests/test_gpu_cps.py), tau = 0.6."""
    import _cps_ref as R
    from mia_hip import ops
    a = za[:nimg].detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    b = zb[:nimg].detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    tau = R.thresholds()[0]
    ops.CrossPseudoFn.apply(a, b, torch.tensor([1.0, tau], device=a.device)).backward()
    _, _, ca, cb = R.decode(ops.CrossPseudoFn.last_code.cpu().numpy())
    ref = R.evaluate(a.detach().cpu().numpy(), b.detach().cpu().numpy(), tau, 1.0, ca=ca, cb=cb)
    out = ops.CrossPseudoFn.last_out.cpu().numpy()
    res = {}
    for side, v, g in (("a", out[1], a.grad), ("b", out[2], b.grad)):
        res[f"value_{side}_err_over_bound"] = round(abs(float(v) - ref["value_" + side]) / (2e-6 * ref["value_mag_" + side]), 4)
        res[f"grad_{side}_err_over_bound"] = round(float((np.abs(g.cpu().numpy() - ref["grad_" + side]) /
                                                          (2e-6 * ref["grad_mag_" + side] + 1e-12)).max()), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_cps needs a GPU")
    import mia_hip
    from losses.cross_pseudo import CrossPseudoSupervisionLoss
    from mia_hip import ops
    dev = torch.device("cuda:0")
    lines = [json.dumps(dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, warmup=a.warmup, torch=torch.__version__,
                             logits="fp32 channels-last, the unlabelled batch slices of two networks", kernel_calls_per_timing=CALLS,
                             not_measured=NOT_MEASURED))]
    print(lines[0], flush=True)
    for n, k1, h, w, lb in ((24, 4, 256, 256, 12), (16, 3, 512, 512, 8)):
        g = torch.Generator().manual_seed(n)
        full_a = (torch.randn(n, h, w, k1, generator=g) * 2).to(dev).permute(0, 3, 1, 2).requires_grad_(True)
        full_b = (full_a.detach().permute(0, 2, 3, 1) + torch.randn(n, h, w, k1, generator=g).to(dev)).permute(0, 3, 1, 2).requires_grad_(True)
        loss = CrossPseudoSupervisionLoss(k1 - 1)
        nu, hw = n - lb, h * w
        # the kernels alone: preallocated buffers, the entry points called directly
        za, zb = full_a.detach()[lb:], full_b.detach()[lb:]
        sa, sb = ops._pix_strides(za), ops._pix_strides(zb)
        slabs = ops._two_logits_slabs(hw)
        ws = torch.empty(mia_hip.lib().mia_cps_workspace(nu, slabs), device=dev, dtype=torch.float32)
        out, counts = torch.empty(4, device=dev), torch.empty(3, device=dev, dtype=torch.int64)
        code = torch.empty((nu, h, w), device=dev, dtype=torch.uint8)
        dza, dzb = torch.empty_like(za), torch.empty_like(zb)
        i64, p = ctypes.c_int64, ops._p

        def kernels():
            for _ in range(CALLS):
                mia_hip.call("mia_cps_fwd", p(za), p(zb), None, nu, i64(hw), k1, *ops._strides_i64(sa), *ops._strides_i64(sb), slabs,
                             p(ws), p(code), p(out), p(counts), ops._stream())
                mia_hip.call("mia_cps_bwd", p(za), p(zb), p(code), None, None, p(dza), p(dzb), nu, i64(hw), k1,
                             *ops._strides_i64(sa), *ops._strides_i64(sb), *ops._strides_i64(ops._pix_strides(dza)),
                             *ops._strides_i64(ops._pix_strides(dzb)), ops._stream())

        def fwd_bwd(fn):
            full_a.grad = full_b.grad = None
            fn(full_a[lb:], full_b[lb:]).backward()
            return full_a.grad, full_b.grad

        arms = {"loss_cps": lambda: fwd_bwd(loss), "torch_cps": lambda: fwd_bwd(torch_cps), "kernels": kernels}
        times = {k: [] for k in arms}
        outs = {}
        order = np.random.default_rng(n)
        for r in range(a.warmup + a.rounds):  # the arms alternate inside every round, in a new seeded order each round
            for k in order.permutation(list(arms)):
                ms, res = event_ms(arms[k])
                if k != "kernels":
                    outs[k] = [t.clone() for t in res]
                if r >= a.warmup:
                    times[k].append(ms / CALLS if k == "kernels" else ms)
        row = dict(workload=f"{nu}x{k1}x{h}x{w}", batch=n, labelled=lb, **{k: stats(v) for k, v in times.items()})
        row["grad_max_abs_diff_to_torch_expr"] = max(float((x - y).abs().max()) for x, y in zip(outs["loss_cps"], outs["torch_cps"]))
        row["kernel_grads_equal_autograd_grads"] = bool(torch.equal(dza, outs["loss_cps"][0][lb:]) and torch.equal(dzb, outs["loss_cps"][1][lb:]))
        row["speedup_over_torch_expr"] = round(row["torch_cps"]["ms_median"] / row["loss_cps"]["ms_median"], 2)
        nbytes = nu * hw * ((2 * k1 * 4 + 1) + (4 * k1 * 4 + 1))  # forward: za, zb in, code out; backward: za, zb, code in, dza, dzb out
        row["bytes_moved"] = nbytes
        row["kernels_gbytes_per_s"] = round(nbytes / (row["kernels"]["ms_median"] * 1e-3) / 1e9, 1)
        full_a.grad = full_b.grad = None
        row["peak_new_bytes_loss_cps"] = peak_new_bytes(lambda: fwd_bwd(loss))
        full_a.grad = full_b.grad = None
        row["peak_new_bytes_torch_cps"] = peak_new_bytes(lambda: fwd_bwd(torch_cps))
        row["logits_bytes_one_network_full_batch"] = n * k1 * hw * 4
        row.update(accuracy(za, zb))
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        del outs, full_a, full_b, za, zb, dza, dzb
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
