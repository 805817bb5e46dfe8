"""Record tests/golden/region_losses.npz: inputs, loss values and logit gradients of the reference's own DC_and_BCE_loss
(sigmoid soft Dice + BCEWithLogitsLoss, nnU-Net's region-based mode) on the CPU in fp32, and for every case the reference's own
fp32 error against a float64 run of the same classes (every term in float64, see `_KeepsFloat64`).  Needs the reference checkout (oracle._refload); the tests only read the
recorded file.

    python tools/gen_region_loss_golden.py

File layout: `meta` = JSON list of cases {name, set, target, ignore, ...parameters}; `in/<set>/logits` fp32 [B,C,H,W];
`in/<set>/mask` uint8 [B,C,H,W] (the multi-label 0/1 target; regions overlap), `in/<set>/soft` fp32 [B,C,H,W] (a soft target in
[0,1]), `in/<set>/ign` uint8 [B,1,H,W] (1 = ignored pixel); `c/<name>/loss` fp32, `c/<name>/grad` fp32 like the logits,
`c/<name>/ref_dv` = |loss32 - loss64| and `c/<name>/ref_dg_rel` = max|grad32 - grad64| / max|grad64| (0 where grad64 is 0).
Case fields: target = "bool" (mask as bool), "float" (mask as fp32) or "soft"; ignore = null, "ign" (the recorded channel) or
"all" (every pixel ignored)."""
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle._refload import Ref  # noqa: E402

SHAPES = {"a": (2, 3, 20, 28), "b": (3, 1, 19, 21), "c": (1, 4, 24, 40)}
POS_WEIGHT = {1: [2.5], 3: [0.5, 2.0, 3.0], 4: [0.5, 2.0, 3.0, 1.25]}


def make_inputs():
    sets = {}
    for name, (b, c, h, w) in SHAPES.items():
        g = torch.Generator().manual_seed(2000 + 10 * c + h)
        logits = torch.randn(b, c, h, w, generator=g) * 2
        mask = (torch.rand(b, c, h, w, generator=g) < 0.4).to(torch.uint8)
        soft = torch.rand(b, c, h, w, generator=g)
        ign = (torch.rand(b, 1, h, w, generator=g) < 0.2).to(torch.uint8)
        sets[name] = dict(logits=logits, mask=mask, soft=soft, ign=ign)
    return sets


def cases():
    d = dict(target="bool", ignore=None, batch_dice=False, do_bg=True, smooth=1.0, pos_weight=False, pw_4d=False, weight_ce=1,
             weight_dice=1)

    def case(name, set_, **kw):
        return dict(d, name=name, set=set_, **kw)

    return [
        case("a_plain", "a"),
        case("a_ign", "a", ignore="ign"),
        case("a_ign_batch_nobg", "a", ignore="ign", batch_dice=True, do_bg=False, smooth=1e-5),
        case("a_float_ign", "a", target="float", ignore="ign"),
        case("a_soft_pw", "a", target="soft", pos_weight=True),
        case("a_pw_ign_w", "a", ignore="ign", pos_weight=True, pw_4d=True, weight_ce=0.7, weight_dice=0.4),
        case("a_all", "a", ignore="all"),
        case("a_nobg", "a", do_bg=False, smooth=1e-5),
        case("a_noce", "a", weight_ce=0, weight_dice=0.6),
        case("b_plain", "b"),
        case("b_ign_batch", "b", ignore="ign", batch_dice=True),
        case("b_float_pw", "b", target="float", pos_weight=True, weight_ce=0.3, weight_dice=1.5),
        case("c_plain_batch", "c", batch_dice=True),
        case("c_ign_nobg_pw", "c", ignore="ign", do_bg=False, pos_weight=True),
        case("c_float_ign_w", "c", target="float", ignore="ign", smooth=1e-5, weight_ce=2.0, weight_dice=0.5),
    ]


class _KeepsFloat64(torch.Tensor):
    """The reference's forward casts the target with `.float()` before the BCE term, and BCEWithLogitsLoss then computes in the
    target's precision -- a float64 run of the class would carry an fp32 BCE term and understate the fp32 error.  For the float64
    run the target is this subclass, whose `.float()` means float64, so every term of the reference's forward runs in float64."""

    def float(self):
        return torch.Tensor.double(self)


def build_target(c, s, dtype):
    """The target tensor of one case: bool stays bool; float targets in `dtype`; the ignore channel appended in the same dtype."""
    t = s["soft"].to(dtype) if c["target"] == "soft" else (s["mask"].bool() if c["target"] == "bool" else s["mask"].to(dtype))
    if c["ignore"] is not None:
        ign = s["ign"] if c["ignore"] == "ign" else torch.ones_like(s["ign"])
        t = torch.cat((t, ign.to(t.dtype)), 1)
    return t.as_subclass(_KeepsFloat64) if dtype == torch.float64 else t


def run_case(ref, c, s, dtype):
    x = s["logits"].to(dtype).clone().requires_grad_(True)
    k = x.shape[1]
    bce_kwargs = {}
    if c["pos_weight"]:
        pw = torch.tensor(POS_WEIGHT[k], dtype=dtype)
        bce_kwargs["pos_weight"] = pw.reshape(1, k, 1, 1) if c["pw_4d"] else pw.reshape(k, 1, 1)
    fn = ref.compound.DC_and_BCE_loss(bce_kwargs, dict(batch_dice=c["batch_dice"], do_bg=c["do_bg"], smooth=c["smooth"]),
                                      weight_ce=c["weight_ce"], weight_dice=c["weight_dice"], use_ignore_label=c["ignore"] is not None)
    loss = fn(x, build_target(c, s, dtype))
    assert loss.dtype == dtype
    loss.backward()
    return np.asarray(loss.item(), dtype=np.float64 if dtype == torch.float64 else np.float32), x.grad.numpy()


def main():
    warnings.simplefilter("ignore")
    ref = Ref()
    sets = make_inputs()
    arrays = {}
    for name, s in sets.items():
        for key, val in s.items():
            arrays[f"in/{name}/{key}"] = val.numpy()
    meta = cases()
    for c in meta:
        s = sets[c["set"]]
        v32, g32 = run_case(ref, c, s, torch.float32)
        v64, g64 = run_case(ref, c, s, torch.float64)
        gmax = np.abs(g64).max()
        arrays[f"c/{c['name']}/loss"] = v32.astype(np.float32)
        arrays[f"c/{c['name']}/grad"] = g32.astype(np.float32)
        dv = abs(float(v32) - float(v64))
        dg_rel = float(np.abs(g32.astype(np.float64) - g64).max() / gmax) if gmax > 0 else 0.0
        arrays[f"c/{c['name']}/ref_dv"] = np.float64(dv)
        arrays[f"c/{c['name']}/ref_dg_rel"] = np.float64(dg_rel)
        print(f"{c['name']}: loss {float(v32):.7f} ref_dv {dv:.2e} ref_dg_rel {dg_rel:.2e} max|g| {gmax:.3e}")
    arrays["meta"] = np.array(json.dumps(meta))
    out = os.path.join(ROOT, "tests", "golden", "region_losses.npz")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes,", len(meta), "cases")


if __name__ == "__main__":
    main()
