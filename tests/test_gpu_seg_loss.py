"""GPU checks of the fold-trainer losses (csrc/seg_loss.hip): masked soft Dice + CE with an ignore label, the hard tp / fp / fn,
and the radix-select top-k CE -- against the reference's recorded numbers (tests/golden/seg_losses.npz) and the float64
restatement (tests/_seg_loss_ref.py).  Tolerances are the project's for the fused loss against its golden (test_gpu_ops.py):
|dvalue| < 2e-6, gradient atol 2e-7.

These are the checks through the public classes, at one slab and k1 = 2, 3, 4.  The kernels' dispatch branches -- more than one
slab, k1 = 1 .. 8, every refusal of the fast route, the loop exits, every grid-stride wrap, the radix select with ties, label
decoding, grad_out -- are run through the C entry points by tests/test_gpu_seg_loss_branches.py, whose docstring opens with the
branch map (kernel -> branch -> test id)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import _seg_loss_ref as R
from test_seg_loss_host import IGN, WEIGHTS, load_golden, restate

pytestmark = pytest.mark.gpu
VAL_TOL, GRAD_ATOL = 2e-6, 2e-7


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _store(logits, layout, dev):
    """fp32 logits on the device as a logical [B,K,H,W] tensor in plain NCHW or channels-last storage, requiring grad."""
    t = torch.as_tensor(np.asarray(logits), dtype=torch.float32).to(dev)
    if layout == "nhwc":
        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return t.requires_grad_(True)


def _labels(lab, ltype, dev):
    """uint8 [B,1,H,W] labels (255 = ignore) as int64 or uint8 device tensors."""
    t = torch.as_tensor(np.asarray(lab)).to(dev)
    return t.long() if ltype == "int64" else t.to(torch.uint8)


def _build(c, k1, dev):
    """The project's loss object for one golden case, and whether it takes a loss_mask."""
    from losses.ce_loss import RobustCrossEntropyLoss, TopKLoss
    from losses.compound_losses import DC_and_CE_loss, softmax_helper_dim1
    from losses.dice_loss import MemoryEfficientSoftDiceLoss
    w = torch.tensor(WEIGHTS[k1], device=dev) if c.get("class_weights") else None
    if c["kind"] == "dcce":
        return DC_and_CE_loss(dict(smooth=c["smooth"], do_bg=c["do_bg"], batch_dice=c["batch_dice"]), {} if w is None else {"weight": w},
                              weight_ce=c.get("weight_ce", 1), weight_dice=c.get("weight_dice", 1), ignore_label=c["ignore"])
    if c["kind"] == "dice":
        return MemoryEfficientSoftDiceLoss(softmax_helper_dim1 if c["softmax"] else None, c["batch_dice"], c["do_bg"], c["smooth"])
    kw = {} if c["ignore"] is None else {"ignore_index": c["ignore"]}
    if c["kind"] == "rce":
        return RobustCrossEntropyLoss(weight=w, **kw)
    return TopKLoss(weight=w, k=c["k"], **kw)


@pytest.mark.parametrize("ltype", ["int64", "uint8"])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_every_golden_record(golden_dir, layout, ltype):
    """Value and logit gradient of every recorded case against the reference's own fp32 numbers."""
    from mia_hip import ops
    dev = _dev()
    d, meta = load_golden(golden_dir)
    n = 0
    for c in meta:
        if c["kind"] == "tpfpfn":
            continue
        x = _store(d[f"in/{c['set']}/logits"], layout, dev)
        y = _labels(d[f"in/{c['set']}/{c['labels']}"], ltype, dev)
        fn = _build(c, x.shape[1], dev)
        if c["kind"] == "dice":
            mask = None if c["mask_from"] is None else torch.from_numpy(d[f"in/{c['set']}/{c['mask_from']}"] != IGN).to(dev)
            v = fn(x, y, loss_mask=mask)
        else:
            v = fn(x, y)
        v.backward()
        dv = abs(v.item() - float(d[f"c/{c['name']}/loss"]))
        dg = np.abs(x.grad.cpu().numpy() - d[f"c/{c['name']}/grad"]).max()
        print(f"{c['name']} {layout} {ltype}: |dvalue| {dv:.2e} |dgrad| {dg:.2e}")
        assert dv < VAL_TOL, (c["name"], dv)
        assert dg < GRAD_ATOL, (c["name"], dg)
        assert x.grad.stride() == x.stride()
        ops.check_labels()  # 255 is the ignore label wherever it occurs: nothing flagged
        n += 1
    assert n == 24


def test_hard_counts_match_golden_tp_fp_fn(golden_dir):
    """`hard_tp_fp_fn` and the counts a fused DC_and_CE_loss leaves behind equal the reference's
    get_tp_fp_fn_tn(onehot(argmax), target, axes=[0,2,3], mask) as recorded."""
    from losses.compound_losses import DC_and_CE_loss
    from losses.dice_loss import hard_tp_fp_fn
    dev = _dev()
    d, meta = load_golden(golden_dir)
    for c in meta:
        if c["kind"] != "tpfpfn" or not c["hard"]:
            continue
        key = c["mask_from"] or c["labels"]
        ign = IGN if c["mask_from"] else None
        for layout in ("nchw", "nhwc"):
            for ltype in ("int64", "uint8"):
                x = _store(d[f"in/{c['set']}/logits"], layout, dev)
                y = _labels(d[f"in/{c['set']}/{key}"], ltype, dev)
                got = hard_tp_fp_fn(x, y, ign)
                assert got.dtype == torch.int64 and got.shape == (x.shape[0], x.shape[1], 3)
                fn = DC_and_CE_loss({"smooth": 1e-5, "do_bg": False}, {}, ignore_label=ign)
                fn(x, y)
                assert torch.equal(fn.last_hard_counts, got)
                tot = got.sum(0).cpu().numpy()
                for j, name in enumerate(("tp", "fp", "fn")):
                    assert tot[:, j].tolist() == d[f"c/{c['name']}/{name}"].astype(np.int64).tolist()


GRID = [(k1, hw) for k1 in (2, 3, 4) for hw in ((64, 64), (96, 136), (31, 20))]


def _grid_inputs(k1, hw, masked):
    g = torch.Generator().manual_seed(100 * k1 + hw[0])
    logits = torch.randn(3, k1, *hw, generator=g) * 2
    labels = torch.randint(0, k1, (3, 1, *hw), generator=g)
    if masked:
        labels[torch.rand(3, 1, *hw, generator=g) < 0.2] = IGN
    return logits, labels


@pytest.mark.parametrize("k1,hw", GRID)
@pytest.mark.parametrize("cfg", [dict(do_bg=False, batch_dice=False, smooth=1e-5, weighted=False),
                                 dict(do_bg=True, batch_dice=True, smooth=1.0, weighted=True)])
def test_masked_dice_ce_grid_vs_restatement(k1, hw, cfg):
    """The grid of test_dice_ce_vectorised_path_vs_oracle with a 20 % ignore mask against the float64 restatement, both storage
    orders and both label types: value, gradient (exactly 0 on ignored pixels), hard counts (exact integers)."""
    from losses.compound_losses import DC_and_CE_loss
    dev = _dev()
    logits, labels = _grid_inputs(k1, hw, True)
    w = WEIGHTS[k1] if cfg["weighted"] else None
    want = R.seg_loss(logits.numpy(), labels.numpy(), ignore=IGN, weight=w, do_bg=cfg["do_bg"], batch_dice=cfg["batch_dice"],
                      smooth=cfg["smooth"], w_ce=0.9, w_dice=0.6)
    ignored = (labels == IGN).expand(-1, k1, -1, -1)
    for layout in ("nhwc", "nchw"):
        for ltype in ("int64", "uint8"):
            x, y = _store(logits, layout, dev), _labels(labels, ltype, dev)
            fn = DC_and_CE_loss(dict(smooth=cfg["smooth"], do_bg=cfg["do_bg"], batch_dice=cfg["batch_dice"]),
                                {} if w is None else {"weight": torch.tensor(w, device=dev)}, weight_ce=0.9, weight_dice=0.6,
                                ignore_label=IGN)
            v = fn(x, y)
            v.backward()
            grad = x.grad.cpu()
            dv, dg = abs(v.item() - want["loss"]), np.abs(grad.numpy() - want["grad"]).max()
            print(f"k1={k1} hw={hw} {layout} {ltype}: |dvalue| {dv:.2e} |dgrad| {dg:.2e}")
            assert dv < VAL_TOL and dg < GRAD_ATOL
            assert abs(fn.last_ce.item() - want["ce"]) < VAL_TOL and abs(fn.last_dc.item() - want["dc"]) < VAL_TOL
            assert bool((grad[ignored] == 0).all())
            assert np.array_equal(fn.last_hard_counts.cpu().numpy(), want["counts"])


@pytest.mark.parametrize("k1,hw", GRID)
@pytest.mark.parametrize("k", [10, 25])
def test_topk_grid_vs_restatement(k1, hw, k):
    from losses.ce_loss import TopKLoss
    dev = _dev()
    logits, labels = _grid_inputs(k1, hw, True)
    want = R.topk_ce(logits.numpy(), labels.numpy(), k, ignore=IGN)
    assert want["n_eq"] == 1  # asserted on the CPU first: no exact tie, so torch.topk's selection is defined and no case is left out
    sel = want["grad"].any(axis=1)
    for layout in ("nhwc", "nchw"):
        for ltype in ("int64", "uint8"):
            x, y = _store(logits, layout, dev), _labels(labels, ltype, dev)
            v = TopKLoss(ignore_index=IGN, k=k)(x, y)
            v.backward()
            grad = x.grad.cpu().numpy()
            dv, dg = abs(v.item() - want["loss"]), np.abs(grad - want["grad"]).max()
            print(f"topk k1={k1} hw={hw} k={k} {layout} {ltype}: |dvalue| {dv:.2e} |dgrad| {dg:.2e}")
            assert dv < VAL_TOL and dg < GRAD_ATOL
            assert np.array_equal(grad.any(axis=1), sel)


def test_topk_tie_rule_and_empty_selection():
    """All-equal logits: every pixel ties with the threshold.  The value is that of any n pixels; the m tied pixels share the n
    slots, so the gradient sums to what n selected pixels would give (this project's rule; torch.topk leaves the choice open)."""
    from losses.ce_loss import TopKLoss
    dev = _dev()
    b, k1, h, w = 2, 3, 10, 10
    y = (torch.arange(b * h * w) % k1).reshape(b, 1, h, w)
    for layout in ("nchw", "nhwc"):
        x = _store(np.zeros((b, k1, h, w)), layout, dev)
        v = TopKLoss(k=30)(x, y.to(dev))
        v.backward()
        want = R.topk_ce(np.zeros((b, k1, h, w)), y.numpy(), 30)
        assert want["n"] == 60 and want["n_gt"] == 0 and want["n_eq"] == 200
        assert abs(v.item() - math.log(3.0)) < VAL_TOL
        g = x.grad.cpu().numpy()
        np.testing.assert_allclose(g, want["grad"], atol=GRAD_ATOL)
        # one selected pixel's gradient is (p - t) / n: its label entry is -(2/3) / 60; sixty selected pixels sum to -(2/3)
        lab_entries = np.take_along_axis(g, y.numpy(), axis=1)
        assert abs(lab_entries.sum() + 2.0 / 3.0) < 1e-6
    # n = int(N k / 100) = 0: the reference takes the mean of an empty tensor
    x = _store(np.random.RandomState(0).randn(1, 3, 3, 3), "nchw", dev)
    v = TopKLoss(k=1)(x, torch.zeros(1, 1, 3, 3, dtype=torch.long, device=dev))
    assert math.isnan(v.item())


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_ignore_label_against_the_bad_label_protocol(layout):
    """A 255-labelled pixel is still an error for DiceAndCELoss (NaN, check_labels raises) and an ignored pixel for
    DC_and_CE_loss(ignore_label=255) on the same tensors; a label of 7 with three classes poisons the new losses too."""
    import mia_hip
    from mia_hip import ops
    from losses.ce_loss import TopKLoss
    from losses.compound_losses import DC_and_CE_loss, DiceAndCELoss
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    logits = _store(torch.randn(2, 3, 16, 16, generator=g).numpy(), layout, dev)
    labels = torch.randint(0, 3, (2, 1, 16, 16), generator=g)
    labels[1, 0, 7, 9] = 255
    ops.check_labels()
    old = DiceAndCELoss(dice_kwargs=dict(num_classes=2, do_bg=True), ce_loss=torch.nn.CrossEntropyLoss)
    assert math.isnan(old(logits, labels[:, 0].to(dev)).item())
    with pytest.raises(mia_hip.MiaError):
        ops.check_labels()
    new = DC_and_CE_loss({"smooth": 1e-5, "do_bg": False}, {}, ignore_label=255)
    for lab in (labels.to(dev), labels.to(dev).to(torch.uint8)):
        logits.grad = None
        v = new(logits, lab)
        v.backward()
        assert math.isfinite(v.item()) and bool(torch.isfinite(logits.grad).all())
        assert bool((logits.grad[1, :, 7, 9] == 0).all())
        ops.check_labels()  # flag clear
    bad = labels.clone()
    bad[0, 0, 3, 3] = 7
    for fn in (new, TopKLoss(ignore_index=255, k=25)):
        for lab in (bad.to(dev), bad.to(dev).to(torch.uint8)):
            logits.grad = None
            v = fn(logits, lab)
            v.backward()
            assert math.isnan(v.item()) and bool(torch.isnan(logits.grad).any())
            with pytest.raises(mia_hip.MiaError):
                ops.check_labels()
            ops.check_labels()
    # without an ignore label 255 is an error for the new loss as well
    assert math.isnan(DC_and_CE_loss({}, {})(logits, labels.to(dev)).item())
    with pytest.raises(mia_hip.MiaError):
        ops.check_labels()


def test_run_to_run_bit_identity_and_retain_graph():
    from losses.ce_loss import TopKLoss
    from losses.compound_losses import DC_and_CE_loss
    dev = _dev()
    logits, labels = _grid_inputs(3, (96, 136), True)
    for fn in (DC_and_CE_loss({"smooth": 1e-5, "do_bg": False}, {}, ignore_label=IGN), TopKLoss(ignore_index=IGN, k=10)):
        for layout in ("nhwc", "nchw"):
            res = []
            for _ in range(2):
                x = _store(logits, layout, dev)
                v = fn(x, labels.to(dev))
                v.backward(retain_graph=True)
                g1 = x.grad.clone()
                v.backward()
                assert torch.equal(x.grad, 2 * g1)
                res.append((v.detach().clone(), g1))
            assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_fold_trainer_step_eager_and_graph():
    """The fold trainers' step (unet_trainer.py:438-447, semi_trainer.py:718-754: DC_and_CE_loss, SGD, clip at 12) on the engine:
    losses finite and falling, the captured-graph run bit-identical to the eager run."""
    from losses.compound_losses import DC_and_CE_loss
    from models.unet import UNet
    from training.engine import TrainEngine
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    batches = []
    for _ in range(20):
        x = torch.rand(4, 1, 64, 64, generator=g)
        y = (x[:, 0] * 3).long().clamp_(0, 2)[:, None]  # learnable: the class follows the intensity
        y[torch.rand(4, 1, 64, 64, generator=g) < 0.2] = IGN
        batches.append((x, y))

    def run(graph):
        torch.manual_seed(11)
        m = UNet(2, 1, 3, [16, 32, 64], normalization="instance", dropout_prob=None).to(dev)
        loss_fn = DC_and_CE_loss({"smooth": 1e-5, "do_bg": False}, {}, ignore_label=IGN)
        eng = TrainEngine(m, loss_fn, "sgd", {"weight_decay": 3e-5, "momentum": 0.9}, start_lr=1e-2,
                          num_iters=40, grad_norm=12, graph=graph)
        losses = [eng.train_step({"image": x.to(dev), "label": y.to(dev)}) for x, y in batches]
        torch.cuda.synchronize()
        return torch.stack(losses).cpu(), {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, len(eng._graphs)

    l0, s0, _ = run(False)
    l1, s1, ngraphs = run(True)
    print("fold step losses", l0.tolist())
    assert ngraphs == 1
    assert torch.isfinite(l0).all() and l0[-1] < l0[0]
    assert torch.equal(l0, l1), (l0 - l1).abs().max()
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
