#!/usr/bin/env python
"""Time the dual-task consistency term on one GPU (csrc/dtc.hip, losses/dual_task.py) on the sibling shapes,

  12 x 4 x 256 x 256 with 6 labelled (ACDC) and 8 x 3 x 512 x 512 with 4 labelled,

segmentation logits [B, K, H, W] and level-set logits [B, K - 1, H, W] as the heads write them: channels-last fp32, batch slices of
larger tensors.  The comparison is the tensor-op form of the same definition (`DualTaskConsistencyLoss(fused=False)`) in the same
rounds; there is no earlier path.  The signed distance map of the labelled images is computed once, outside the timed region, and given
to both forms (`phi=`): the transform itself is `signed_distance_map`, timed in profiles/boundary_loss.txt.

Arms, alternating inside every round on the same seeded data, in a new seeded order each round, every arm started on an idle
device, device events around each -- so an arm's time includes the host's path between its launches, as a user times a call:
  dtc / torch             forward + backward of the loss through autograd, the extents included (mia_sdm_extent / two amax)
  extent / extent_torch   `ops.sdm_extent(phi)` against `stack([phi.amax, (-phi).amax])`
  kernels                 mia_sdm_extent + mia_dtc_fwd + mia_dtc_finalize + mia_dtc_bwd called back to back on preallocated buffers,
                          CALLS times inside one pair of events, divided by CALLS: the kernels alone
Also recorded: peak newly allocated device memory of the two autograd arms, the bytes the kernels must move, the largest difference
between the two forms' gradients, and on the first two images the largest ratio of the value / gradient error to the bounds of
tests/test_gpu_dtc.py.

    python tools/microbench_dtc.py [--rounds 7] [--warmup 2] [--out profiles/dtc.txt]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "medical-image-analysis_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CALLS = 20
K, W_CONS, BETA = 1500.0, 0.1, 0.3
NOT_MEASURED = ("a whole DTCEngine step; the distance transform (profiles/boundary_loss.txt); planar logits (the heads write channels-last); "
                "kernel times by a profiler (the `kernels` arm is timed by events); the flagship shape; hipGraph capture; more than one "
                "rank; any shape other than the two above")


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


def peak_new_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def accuracy(z, r, phi, dyn, nimg=2, lb=1):
    """Largest error / bound of value and gradients on the first `nimg` images (bounds of tests/test_gpu_dtc.py)."""
    import _dtc_ref as R
    from losses.dual_task import DualTaskConsistencyLoss
    zz = z[:nimg].detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    rr = r[:nimg].detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    mod = DualTaskConsistencyLoss(z.shape[1] - 1, K)
    loss = mod(zz, rr, None, lb, dyn=dyn, phi=phi[:lb])
    loss.backward()
    w0, w1 = (float(v) for v in dyn.cpu())
    ref = R.evaluate(zz.detach().cpu().numpy(), rr.detach().cpu().numpy(), phi[:lb].cpu().numpy(), lb, K, w0, w1)
    gz = float((np.abs(zz.grad.cpu().numpy() - ref["dz"]) / (2e-6 * ref["dz_mag"] + 1e-12)).max())
    gr = float((np.abs(rr.grad.cpu().numpy() - ref["dr"]) / (2e-6 * ref["dr_mag"] + 1e-12)).max())
    return dict(value_err_over_bound=round(abs(float(loss.detach()) - ref["value"]) / (2e-6 * ref["value_mag"]), 4),
                grad_err_over_bound=round(max(gz, gr), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_dtc needs a GPU")
    import mia_hip
    from losses.boundary_loss import signed_distance_map
    from losses.dual_task import DualTaskConsistencyLoss
    from mia_hip import ops
    dev = torch.device("cuda:0")
    lines = [json.dumps(dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, warmup=a.warmup, torch=torch.__version__,
                             logits="fp32 channels-last, batch slices", k=K, consistency_weight=W_CONS, beta=BETA,
                             kernel_calls_per_timing=CALLS, not_measured=NOT_MEASURED))]
    print(lines[0], flush=True)
    for n, k1, h, w, lb in ((12, 4, 256, 256, 6), (8, 3, 512, 512, 4)):
        g = torch.Generator().manual_seed(n)
        hw, c = h * w, k1 - 1
        z = (torch.randn(n + 2, h, w, k1, generator=g) * 2).to(dev).permute(0, 3, 1, 2)[2:].requires_grad_(True)
        steep = torch.rand(n + 2, h, w, c, generator=g) < 0.5
        rv = torch.randn(n + 2, h, w, c, generator=g)
        r = torch.where(steep, 2e-3 * rv, torch.randn(n + 2, h, w, c, generator=g)).to(dev).permute(0, 3, 1, 2)[2:].requires_grad_(True)
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        label = torch.zeros(lb, h, w, dtype=torch.long)
        for i in range(lb):
            for cls in range(1, k1):
                cy, cx, rad = h * (cls + i % 2) // (k1 + 1), w * cls // k1, h // (5 + cls + i % 3)
                label[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad] = cls
        phi = signed_distance_map(label.to(dev), c)
        dyn = torch.tensor([W_CONS, BETA], device=dev)
        fused, soft = DualTaskConsistencyLoss(c, K), DualTaskConsistencyLoss(c, K, fused=False)

        def step(mod):
            z.grad = r.grad = None
            mod(z, r, None, lb, dyn=dyn, phi=phi).backward()
            return z.grad, r.grad

        # the kernels alone: preallocated buffers, the entry points called directly
        zd, rd = z.detach(), r.detach()
        sz, sr = ops._pix_strides(zd), ops._pix_strides(rd)
        slabs = ops._two_logits_slabs(hw)
        ws, coef, out = torch.empty(n * slabs * 4, device=dev), torch.empty(2, device=dev), torch.empty(3, device=dev)
        ext = torch.empty((lb, c, 2), device=dev)
        dz, dr = torch.empty_like(zd), torch.empty_like(rd)
        i64, f32, p = ctypes.c_int64, ctypes.c_float, ops._p

        def kernels():
            for _ in range(CALLS):
                mia_hip.call("mia_sdm_extent", p(phi), lb * c, i64(hw), p(ext), ops._stream())
                mia_hip.call("mia_dtc_fwd", p(zd), p(rd), p(phi), p(ext), n, lb, i64(hw), k1, f32(K), *ops._strides_i64(sz),
                             *ops._strides_i64(sr), slabs, p(ws), ops._stream())
                mia_hip.call("mia_dtc_finalize", p(ws), p(dyn), n, lb, i64(hw), k1, slabs, p(coef), p(out), ops._stream())
                mia_hip.call("mia_dtc_bwd", p(zd), p(rd), p(phi), p(ext), p(coef), None, p(dz), p(dr), n, lb, i64(hw), k1, f32(K),
                             *ops._strides_i64(sz), *ops._strides_i64(sr), *ops._strides_i64(ops._pix_strides(dz)),
                             *ops._strides_i64(ops._pix_strides(dr)), ops._stream())

        arms = {"dtc": lambda: step(fused), "torch": lambda: step(soft), "extent": lambda: (ops.sdm_extent(phi),),
                "extent_torch": lambda: (torch.stack([phi.amax((2, 3)), (-phi).amax((2, 3))], -1),), "kernels": kernels}
        times = {k: [] for k in arms}
        outs = {}
        order = np.random.default_rng(n)
        for rnd in range(a.warmup + a.rounds):  # the arms alternate inside every round, in a new seeded order each round
            for k in order.permutation(list(arms)):
                ms, res = event_ms(arms[k])
                if res is not None:
                    outs[k] = [t.clone() for t in res]
                if rnd >= a.warmup:
                    times[k].append(ms / CALLS if k == "kernels" else ms)
        row = dict(workload=f"{n}x{k1}x{h}x{w}", labelled=lb, **{k: stats(v) for k, v in times.items()})
        row["speedup_over_tensor_ops"] = round(row["torch"]["ms_median"] / row["dtc"]["ms_median"], 2)
        row["extent_over_extent_torch"] = round(row["extent"]["ms_median"] / row["extent_torch"]["ms_median"], 2)
        row["extent_bits_equal"] = bool(torch.equal(outs["extent"][0].view(torch.int32), (outs["extent_torch"][0] + 0.0).view(torch.int32)))
        row["dz_max_abs_diff_to_tensor_ops"] = float((outs["dtc"][0] - outs["torch"][0]).abs().max())
        row["dr_max_abs_diff_to_tensor_ops"] = float((outs["dtc"][1] - outs["torch"][1]).abs().max())
        row["kernel_grads_equal_autograd_grads"] = bool(torch.equal(dz, outs["dtc"][0]) and torch.equal(dr, outs["dtc"][1]))
        # extents: phi in; forward: z, r in, phi of the labelled images; backward: the same in, dz and dr out
        nbytes = lb * c * hw * 4 + 2 * (n * (k1 + c) * hw * 4 + lb * c * hw * 4) + n * (k1 + c) * hw * 4
        row["bytes_moved_extent_fwd_bwd"] = nbytes
        row["kernels_gbytes_per_s"] = round(nbytes / (row["kernels"]["ms_median"] * 1e-3) / 1e9, 1)
        for k in ("dtc", "torch"):
            z.grad = r.grad = None
            row[f"peak_new_bytes_{k}"] = peak_new_bytes(arms[k])
        row["logits_bytes_both_heads"] = n * (k1 + c) * hw * 4
        row.update(accuracy(z, r, phi, dyn))
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        del outs, z, r, phi, dz, dr
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
