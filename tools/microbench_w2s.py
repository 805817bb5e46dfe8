#!/usr/bin/env python
"""Time the weak-to-strong consistency term on one GPU (csrc/w2s.hip, losses/weak_strong.py) on the unlabelled halves that
profiles/consistency.txt and profiles/cps.txt use,

  12 x 4 x 256 x 256 (of a batch of 24, ACDC) and 8 x 3 x 512 x 512 (of a batch of 16), channels-last fp32 logits that are batch slices,

against the tensor-op form of the same definition (`pseudo_label_code`, `WeakToStrongLoss(fused=False)`, `torch.where(mask, x[perm],
x)`).  There is no earlier path: the tensor-op form in the same run is the comparison.

Arms, alternating inside every round on the same seeded data, in a new seeded order each round, every arm started on an idle
device, device events around each -- so an arm's time includes the host's path between its launches, as a user times a call:
  w2s_1view / torch_1view     pseudo-labels of the weak logits, then forward + backward of ONE strong view through autograd
  w2s_2views / torch_2views   the same labels, TWO strong views (rows of one logits tensor), (L1 + L2) / 2, one backward
  mix_hip / mix_torch         the CutMix of the unlabelled images with a permutation of themselves, written into the rows of a larger
                              input tensor: `ops.cutmix_perm(..., out=net_in[lb:])` against `net_in[lb:] = torch.where(m, x[perm], x)`
  kernels, mix_kernel         mia_w2s_labels + mia_w2s_loss_fwd + mia_w2s_loss_bwd, and mia_cutmix_perm, called back to back on
                              preallocated buffers, CALLS times inside one pair of events, divided by CALLS: the kernels alone
Also recorded: peak newly allocated device memory of every autograd arm and of the two mixes, the bytes the kernels must move, the
largest difference between the two forms' gradients, and on the first two images the largest ratio of the value / gradient error to
the bounds of tests/test_gpu_w2s.py.

    python tools/microbench_w2s.py [--rounds 7] [--warmup 2] [--out profiles/w2s.txt]
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
TAU, WEIGHT, CE_W, DICE_W = 0.9, 0.5, 1.0, 0.5
NOT_MEASURED = ("a whole FixMatchEngine step; planar logits (the head writes channels-last); kernel times by a profiler (the `kernels` "
                "arms are timed by events); the flagship shape; hipGraph capture; more than one rank; any shape other than the two above")


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


def accuracy(zw, zs, mask, perm, dyn, nimg=2):
    """Largest error / bound of value and gradient on the first `nimg` images (bounds of tests/test_gpu_w2s.py), the device's codes."""
    import _w2s_ref as R
    from losses.weak_strong import WeakToStrongLoss
    from mia_hip import ops
    w = zw[:nimg].detach()
    s = zs[:nimg].detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    pm = [int(i) % nimg for i in perm[:nimg]]
    code, _ = ops.w2s_labels(w, dyn)
    mod = WeakToStrongLoss(zw.shape[1] - 1, CE_W, DICE_W)
    loss = mod(s, code, mask[:nimg], pm, dyn=dyn)
    loss.backward()
    ref = R.evaluate(s.detach().cpu().numpy(), code.cpu().numpy(), mask[:nimg].cpu().numpy(), np.array(pm), WEIGHT, CE_W, DICE_W)
    return dict(value_err_over_bound=round(abs(float(loss.detach()) - ref["value"]) / (2e-6 * ref["value_mag"]), 4),
                grad_err_over_bound=round(float((np.abs(s.grad.cpu().numpy() - ref["grad"]) / (2e-6 * ref["grad_mag"] + 1e-12)).max()), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_w2s needs a GPU")
    import mia_hip
    from losses.weak_strong import WeakToStrongLoss, box_masks, pseudo_label_code, random_cutmix_boxes
    from mia_hip import ops
    dev = torch.device("cuda:0")
    lines = [json.dumps(dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, warmup=a.warmup, torch=torch.__version__,
                             logits="fp32 channels-last, batch slices", tau=TAU, weight=WEIGHT, ce_weight=CE_W, dice_weight=DICE_W,
                             kernel_calls_per_timing=CALLS, not_measured=NOT_MEASURED))]
    print(lines[0], flush=True)
    for n, k1, h, w, lb in ((24, 4, 256, 256, 12), (16, 3, 512, 512, 8)):
        g = torch.Generator().manual_seed(n)
        nu, hw = n - lb, h * w
        full_w = (torch.randn(n, h, w, k1, generator=g) * 3).to(dev).permute(0, 3, 1, 2)  # the weak logits of a whole batch
        noise = torch.randn(lb + 2 * nu, h, w, k1, generator=g).to(dev)
        full_s = (torch.cat([full_w[:lb], full_w[lb:], full_w[lb:]]).permute(0, 2, 3, 1) + noise).permute(0, 3, 1, 2).requires_grad_(True)
        del noise
        image = torch.rand(n, 1, h, w, generator=g).to(dev)
        torch.manual_seed(n)
        mask = box_masks(random_cutmix_boxes(nu, h, w, 1.0), h, w, dev)
        perm_host = torch.randperm(nu)
        perm = perm_host.to(torch.int32).to(dev)
        dyn = torch.tensor([WEIGHT, TAU], device=dev)
        fused, soft = WeakToStrongLoss(k1 - 1, CE_W, DICE_W), WeakToStrongLoss(k1 - 1, CE_W, DICE_W, fused=False)
        net_in = torch.empty((n, 1, h, w), device=dev)

        def views(mod, nviews, labels):
            full_s.grad = None
            code = labels(full_w[lb:])
            loss = sum(mod(full_s[lb + v * nu:lb + (v + 1) * nu], code, mask, perm, dyn=dyn) for v in range(nviews)) / nviews
            loss.backward()
            return (full_s.grad,)

        hip_labels = lambda z: ops.w2s_labels(z, dyn)[0]
        torch_labels = lambda z: pseudo_label_code(z, dyn[1])

        def mix_hip():
            return (ops.cutmix_perm(image[lb:], perm, mask, out=net_in[lb:]),)

        def mix_torch():
            net_in[lb:] = torch.where((mask != 0)[:, None], image[lb:][perm.long()], image[lb:])
            return (net_in[lb:],)

        # the kernels alone: preallocated buffers, the entry points called directly
        zw, zs = full_w[lb:], full_s.detach()[lb:lb + nu]
        sw, ss = ops._pix_strides(zw), ops._pix_strides(zs)
        slabs = ops._two_logits_slabs(hw)
        lws = torch.empty(nu * slabs, device=dev, dtype=torch.int32)
        words = mia_hip.lib().mia_w2s_loss_workspace(nu, k1, slabs)
        ws, coef, out = torch.empty(words, device=dev), torch.empty(2 * k1 + 1, device=dev), torch.empty(4, device=dev)
        counts, kept = torch.empty(2, device=dev, dtype=torch.int64), torch.empty(1, device=dev, dtype=torch.int64)
        code = torch.empty((nu, h, w), device=dev, dtype=torch.uint8)
        dz = torch.empty_like(zs)
        flags = ops._perm_flags(dev)
        x = image[lb:]
        i64, f32, p = ctypes.c_int64, ctypes.c_float, ops._p

        def kernels():
            for _ in range(CALLS):
                mia_hip.call("mia_w2s_labels", p(zw), p(dyn), nu, i64(hw), k1, *ops._strides_i64(sw), slabs, p(lws), p(code), p(kept),
                             ops._stream())
                mia_hip.call("mia_w2s_loss_fwd", p(zs), p(code), p(mask), p(perm), p(dyn), nu, i64(hw), k1, *ops._strides_i64(ss), i64(hw),
                             f32(1e-10), f32(CE_W), f32(DICE_W), slabs, p(ws), p(coef), p(out), p(counts), p(flags), ops._stream())
                mia_hip.call("mia_w2s_loss_bwd", p(zs), p(code), p(mask), p(perm), p(coef), None, p(dz), nu, i64(hw), k1,
                             *ops._strides_i64(ss), *ops._strides_i64(ops._pix_strides(dz)), i64(hw), ops._stream())

        def mix_kernel():
            for _ in range(CALLS):
                mia_hip.call("mia_cutmix_perm", p(x), p(perm), p(mask), p(net_in[lb:]), nu, 1, i64(hw), i64(hw), i64(hw), p(flags),
                             ops._stream())

        arms = {"w2s_1view": lambda: views(fused, 1, hip_labels), "torch_1view": lambda: views(soft, 1, torch_labels),
                "w2s_2views": lambda: views(fused, 2, hip_labels), "torch_2views": lambda: views(soft, 2, torch_labels),
                "mix_hip": mix_hip, "mix_torch": mix_torch, "kernels": kernels, "mix_kernel": mix_kernel}
        times = {k: [] for k in arms}
        outs = {}
        order = np.random.default_rng(n)
        for r in range(a.warmup + a.rounds):  # the arms alternate inside every round, in a new seeded order each round
            for k in order.permutation(list(arms)):
                ms, res = event_ms(arms[k])
                if res is not None:
                    outs[k] = [t.clone() for t in res]
                if r >= a.warmup:
                    times[k].append(ms / CALLS if k in ("kernels", "mix_kernel") else ms)
        row = dict(workload=f"{nu}x{k1}x{h}x{w}", batch=n, labelled=lb, **{k: stats(v) for k, v in times.items()})
        pasted = int((mask != 0).sum())
        row["pasted_share"] = round(pasted / (nu * hw), 4)
        row["kept_share_of_the_weak_view"] = round(int(ops.w2s_labels(zw, dyn)[1]) / (nu * hw), 4)
        for nv in (1, 2):
            row[f"grad_max_abs_diff_to_tensor_ops_{nv}view"] = float((outs[f"w2s_{nv}view{'s' if nv > 1 else ''}"][0] -
                                                                     outs[f"torch_{nv}view{'s' if nv > 1 else ''}"][0]).abs().max())
            row[f"speedup_over_tensor_ops_{nv}view"] = round(row[f"torch_{nv}view{'s' if nv > 1 else ''}"]["ms_median"] /
                                                             row[f"w2s_{nv}view{'s' if nv > 1 else ''}"]["ms_median"], 2)
        row["mix_bits_equal"] = bool(torch.equal(outs["mix_hip"][0].view(torch.int32), outs["mix_torch"][0].view(torch.int32)))
        row["mix_hip_over_mix_torch"] = round(row["mix_hip"]["ms_median"] / row["mix_torch"]["ms_median"], 2)
        row["kernel_grad_equals_autograd_grad"] = bool(torch.equal(dz, outs["w2s_1view"][0][lb:lb + nu]))
        # labels: zw in, code out; forward: zs, mask, code in (and the partner's code under a box); backward: the same in, dzs out
        nbytes = nu * hw * (k1 * 4 + 1) + 2 * (nu * hw * (k1 * 4 + 2) + pasted) + nu * hw * k1 * 4
        row["bytes_moved_labels_fwd_bwd"] = nbytes
        row["kernels_gbytes_per_s"] = round(nbytes / (row["kernels"]["ms_median"] * 1e-3) / 1e9, 1)
        mbytes = nu * hw * (4 + 1 + 4) + 4 * pasted  # x and mask in, out written, the partner under a box
        row["bytes_moved_mix"] = mbytes
        row["mix_kernel_gbytes_per_s"] = round(mbytes / (row["mix_kernel"]["ms_median"] * 1e-3) / 1e9, 1)
        for k in ("w2s_1view", "torch_1view", "w2s_2views", "torch_2views", "mix_hip", "mix_torch"):
            full_s.grad = None
            row[f"peak_new_bytes_{k}"] = peak_new_bytes(arms[k])
        row["logits_bytes_one_view"] = nu * k1 * hw * 4
        row.update(accuracy(zw, full_s[lb:lb + nu], mask, perm_host.tolist(), dyn))
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        del outs, full_w, full_s, image, net_in, dz
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
