"""Record tests/golden/seg_losses.npz: inputs, loss values and logit gradients of the reference's own DC_and_CE_loss,
MemoryEfficientSoftDiceLoss, RobustCrossEntropyLoss(weight, ignore_index), TopKLoss and get_tp_fp_fn_tn, on the CPU in fp32.
Needs the reference checkout (oracle._refload); the tests only read the recorded file.

    python tools/gen_seg_loss_golden.py

File layout: `meta` = JSON list of cases {name, kind, set, labels, ...parameters}; `in/<set>/logits` fp32 [B,K1,H,W];
`in/<set>/<labels>` uint8 [B,1,H,W] (255 = ignore); `c/<name>/loss` fp32, `c/<name>/grad` fp32 like the logits;
`c/<name>/{tp,fp,fn,tn}` for the kind "tpfpfn"."""
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle._refload import Ref  # noqa: E402

IGN = 255
WEIGHTS = {2: [0.2, 1.0], 3: [0.2, 1.0, 3.0], 4: [0.2, 1.0, 3.0, 0.5]}


def make_inputs():
    sets = {}
    for name, (b, k1, h, w) in {"s2": (3, 2, 15, 12), "s3": (3, 3, 15, 12), "s4": (3, 4, 15, 12), "r3": (2, 3, 17, 11),
                                "l3": (2, 3, 48, 40)}.items():
        g = torch.Generator().manual_seed(1000 + 10 * k1 + h)
        logits = torch.randn(b, k1, h, w, generator=g) * 2
        lab = torch.randint(0, k1, (b, 1, h, w), generator=g).to(torch.uint8)
        drop = torch.rand(b, 1, h, w, generator=g) < 0.2
        lab_ign = torch.where(drop, torch.tensor(IGN, dtype=torch.uint8), lab)
        lab_img = lab_ign.clone()
        lab_img[1] = IGN  # one image fully ignored
        sets[name] = dict(logits=logits, lab=lab, lab_ign=lab_ign, lab_img=lab_img, lab_all=torch.full_like(lab, IGN))
    return sets


def cases():
    tr = dict(smooth=1e-5, do_bg=False, batch_dice=False)
    out = []
    for k1 in (2, 3, 4):
        out.append(dict(name=f"dcce_s{k1}_plain", kind="dcce", set=f"s{k1}", labels="lab", ignore=None, **tr))
        out.append(dict(name=f"dcce_s{k1}_ign", kind="dcce", set=f"s{k1}", labels="lab_ign", ignore=IGN, **tr))
    out += [
        dict(name="dcce_s3_img", kind="dcce", set="s3", labels="lab_img", ignore=IGN, **tr),
        dict(name="dcce_s3_all", kind="dcce", set="s3", labels="lab_all", ignore=IGN, **tr),
        dict(name="dcce_s3_bg_batch", kind="dcce", set="s3", labels="lab_ign", ignore=IGN, smooth=1.0, do_bg=True, batch_dice=True,
             weight_ce=0.9, weight_dice=0.6),
        dict(name="dcce_s3_batch_w", kind="dcce", set="s3", labels="lab_ign", ignore=IGN, smooth=1e-5, do_bg=False, batch_dice=True,
             class_weights=True),
        dict(name="dcce_s3_bg_s1", kind="dcce", set="s3", labels="lab_img", ignore=IGN, smooth=1.0, do_bg=True, batch_dice=False,
             weight_ce=0.9, weight_dice=0.6),
        dict(name="dcce_s3_nodice", kind="dcce", set="s3", labels="lab_ign", ignore=IGN, smooth=1.0, do_bg=True, batch_dice=False,
             weight_ce=0.9, weight_dice=0),
        dict(name="dcce_s3_noce", kind="dcce", set="s3", labels="lab", ignore=None, weight_ce=0, weight_dice=0.6, **tr),
        dict(name="dcce_r3_ign", kind="dcce", set="r3", labels="lab_ign", ignore=IGN, **tr),
        dict(name="dcce_l3_ign", kind="dcce", set="l3", labels="lab_ign", ignore=IGN, **tr),
        dict(name="dice_s3_raw_mask", kind="dice", set="s3", labels="lab", mask_from="lab_ign", softmax=False, smooth=1.0, do_bg=True,
             batch_dice=False),
        dict(name="dice_s4_batch", kind="dice", set="s4", labels="lab", mask_from=None, softmax=True, smooth=1e-5, do_bg=False,
             batch_dice=True),
        dict(name="rce_s3_w_ign", kind="rce", set="s3", labels="lab_ign", ignore=IGN, class_weights=True),
        dict(name="rce_s3_w", kind="rce", set="s3", labels="lab", ignore=None, class_weights=True),
        dict(name="rce_r3_ign", kind="rce", set="r3", labels="lab_ign", ignore=IGN, class_weights=False),
        dict(name="topk_s3_k10", kind="topk", set="s3", labels="lab", ignore=None, class_weights=False, k=10),
        dict(name="topk_s3_k25_w_ign", kind="topk", set="s3", labels="lab_ign", ignore=IGN, class_weights=True, k=25),
        dict(name="topk_s2_k25", kind="topk", set="s2", labels="lab", ignore=None, class_weights=False, k=25),
        dict(name="topk_r3_k10_ign", kind="topk", set="r3", labels="lab_ign", ignore=IGN, class_weights=False, k=10),
        dict(name="tpfpfn_s3_hard", kind="tpfpfn", set="s3", labels="lab", mask_from=None, hard=True, axes=[0, 2, 3], square=False),
        dict(name="tpfpfn_s3_hard_mask", kind="tpfpfn", set="s3", labels="lab", mask_from="lab_ign", hard=True, axes=[0, 2, 3],
             square=False),
        dict(name="tpfpfn_s4_soft_mask_sq", kind="tpfpfn", set="s4", labels="lab", mask_from="lab_ign", hard=False, axes=None,
             square=True),
    ]
    return out


def run_case(ref, c, sets):
    s = sets[c["set"]]
    x = s["logits"].clone().requires_grad_(True)
    k1 = x.shape[1]
    y = s[c["labels"]].long()
    w = torch.tensor(WEIGHTS[k1]) if c.get("class_weights") else None
    rec = {}
    if c["kind"] == "dcce":
        ce_kwargs = {} if w is None else {"weight": w}
        fn = ref.compound.DC_and_CE_loss(dict(smooth=c["smooth"], do_bg=c["do_bg"], batch_dice=c["batch_dice"]), ce_kwargs,
                                         weight_ce=c.get("weight_ce", 1), weight_dice=c.get("weight_dice", 1),
                                         ignore_label=c["ignore"])
        loss = fn(x, y)
    elif c["kind"] == "dice":
        fn = ref.dice_loss.MemoryEfficientSoftDiceLoss(ref.compound.softmax_helper_dim1 if c["softmax"] else None, c["batch_dice"],
                                                       c["do_bg"], c["smooth"])
        mask = None if c["mask_from"] is None else (s[c["mask_from"]] != IGN)
        loss = fn(x, y, loss_mask=mask)
    elif c["kind"] == "rce":
        kw = {} if c["ignore"] is None else {"ignore_index": c["ignore"]}
        loss = ref.ce_loss.RobustCrossEntropyLoss(weight=w, **kw)(x, y)
    elif c["kind"] == "topk":
        kw = {} if c["ignore"] is None else {"ignore_index": c["ignore"]}
        loss = ref.ce_loss.TopKLoss(weight=w, k=c["k"], **kw)(x, y)
    elif c["kind"] == "tpfpfn":
        with torch.no_grad():
            if c["hard"]:
                pred = torch.zeros_like(x).scatter_(1, x.argmax(1)[:, None], 1)
            else:
                pred = torch.softmax(x, 1)
            mask = None if c["mask_from"] is None else (s[c["mask_from"]] != IGN).float()
            tp, fp, fn_, tn = ref.dice_loss.get_tp_fp_fn_tn(pred, y, axes=c["axes"], mask=mask, square=c["square"])
        return dict(tp=tp.numpy(), fp=fp.numpy(), fn=fn_.numpy(), tn=tn.numpy())
    loss.backward()
    rec["loss"] = loss.detach().numpy().astype(np.float32)
    rec["grad"] = x.grad.numpy().astype(np.float32)
    return rec


def main():
    warnings.simplefilter("ignore")
    ref = Ref()
    sets = make_inputs()
    arrays = {}
    for name, s in sets.items():
        arrays[f"in/{name}/logits"] = s["logits"].numpy()
        for key in ("lab", "lab_ign", "lab_img", "lab_all"):
            arrays[f"in/{name}/{key}"] = s[key].numpy()
    meta = cases()
    for c in meta:
        for key, val in run_case(ref, c, sets).items():
            arrays[f"c/{c['name']}/{key}"] = val
    arrays["meta"] = np.array(json.dumps(meta))
    out = os.path.join(ROOT, "tests", "golden", "seg_losses.npz")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes,", len(meta), "cases")


if __name__ == "__main__":
    main()
