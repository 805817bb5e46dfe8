"""CPU checks of the fold-trainer losses: the float64 restatement (tests/_seg_loss_ref.py) against hand-computed answers and
against every record of tests/golden/seg_losses.npz (the reference's own fp32 numbers), the tensor-op `get_tp_fp_fn_tn`, the
constructors and the error cases of the Python surface, and the C-ABI declarations -- none of it needs a GPU."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _seg_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGN = 255
WEIGHTS = {2: [0.2, 1.0], 3: [0.2, 1.0, 3.0], 4: [0.2, 1.0, 3.0, 0.5]}
ENTRY_POINTS = ("mia_seg_loss_workspace", "mia_seg_loss_fwd", "mia_seg_loss_bwd", "mia_topk_ce_workspace", "mia_topk_ce_fwd",
                "mia_topk_ce_bwd")
# fp32 reference against float64 formulas: the project's bounds for the fused loss against its golden (tests/test_gpu_ops.py)
VAL_TOL, GRAD_ATOL = 2e-6, 2e-7


def load_golden(golden_dir):
    d = np.load(os.path.join(golden_dir, "seg_losses.npz"))
    return d, json.loads(str(d["meta"]))


def restate(c, d):
    """The restatement's answer for one golden case (kinds dcce, dice, rce, topk)."""
    x = d[f"in/{c['set']}/logits"]
    y = d[f"in/{c['set']}/{c['labels']}"].astype(np.int64)
    w = WEIGHTS[x.shape[1]] if c.get("class_weights") else None
    if c["kind"] == "dcce":
        return R.seg_loss(x, y, ignore=c["ignore"], weight=w, softmax=True, do_bg=c["do_bg"], batch_dice=c["batch_dice"],
                          smooth=c["smooth"], w_ce=c.get("weight_ce", 1), w_dice=c.get("weight_dice", 1))
    if c["kind"] == "dice":
        if c["mask_from"] is not None:
            y = np.where(d[f"in/{c['set']}/{c['mask_from']}"] != IGN, y, -7)
        return R.seg_loss(x, y, ignore=-7 if c["mask_from"] is not None else None, softmax=c["softmax"], do_bg=c["do_bg"],
                          batch_dice=c["batch_dice"], smooth=c["smooth"], w_ce=0.0, w_dice=1.0)
    if c["kind"] == "rce":
        return R.seg_loss(x, y, ignore=c["ignore"], weight=w, w_ce=1.0, w_dice=0.0)
    if c["kind"] == "topk":
        return R.topk_ce(x, y, c["k"], ignore=c["ignore"], weight=w)
    raise AssertionError(c["kind"])


def test_restatement_hand_computed():
    # all-zero logits: p = 1/K1 everywhere, ce = ln K1, gradient of the CE term = (1/K1 - t) / N
    for k1 in (2, 3, 4):
        y = (np.arange(2 * 4 * 5) % k1).reshape(2, 4, 5)
        o = R.seg_loss(np.zeros((2, k1, 4, 5)), y, w_dice=0.0)
        assert abs(o["ce"] - np.log(k1)) < 1e-15 and abs(o["loss"] - np.log(k1)) < 1e-15
        t = np.eye(k1)[y].transpose(0, 3, 1, 2)
        np.testing.assert_allclose(o["grad"], (1.0 / k1 - t) / 40, atol=1e-16, rtol=0)
    # Dice by hand, one image, two classes, four pixels, raw "probabilities" (no soft-max), labels 0 0 1 1
    x = np.array([[[[0.5, 1.0, 0.25, 0.0]], [[0.5, 0.0, 0.75, 1.0]]]])
    y = np.array([[[0, 0, 1, 1]]])
    o = R.seg_loss(x, y, softmax=False, do_bg=True, smooth=1.0, w_ce=0.0)
    # class 0: I = 1.5, P = 1.75, G = 2; class 1: I = 1.75, P = 2.25, G = 2
    want = -0.5 * ((2 * 1.5 + 1) / (2 + 1.75 + 1) + (2 * 1.75 + 1) / (2 + 2.25 + 1))
    assert abs(o["dc"] - want) < 1e-15
    o = R.seg_loss(x, y, softmax=False, do_bg=False, smooth=1.0, w_ce=0.0)
    assert abs(o["dc"] + (2 * 1.75 + 1) / (2 + 2.25 + 1)) < 1e-15
    # the third pixel ignored: class 1 keeps I = 1, P = 0.5 + 0 + 1, G = 1
    o = R.seg_loss(x, np.array([[[0, 0, IGN, 1]]]), ignore=IGN, softmax=False, do_bg=False, smooth=1.0, w_ce=0.0)
    assert abs(o["dc"] + (2 * 1.0 + 1) / (1 + 1.5 + 1)) < 1e-15
    assert np.all(o["grad"][:, :, :, 2] == 0)
    # a fully ignored target: every Dice term is smooth / smooth, the CE term is dropped, no gradient
    o = R.seg_loss(np.random.RandomState(0).randn(2, 3, 4, 5), np.full((2, 1, 4, 5), IGN), ignore=IGN, do_bg=False, smooth=1e-5)
    assert o["dc"] == -1.0 and o["ce"] == 0.0 and o["loss"] == -1.0 and not o["grad"].any()
    # weighted CE by hand: two pixels, logits (0, ln 3): p = (1/4, 3/4); labels 0 and 1, weights 2 and 1
    o = R.seg_loss(np.array([[[[0.0, 0.0]], [[np.log(3.0), np.log(3.0)]]]]), np.array([[[0, 1]]]), weight=[2.0, 1.0], w_dice=0.0)
    assert abs(o["ce"] - (2 * np.log(4.0) + np.log(4.0 / 3.0)) / 3) < 1e-15


def test_restatement_hard_counts_and_topk_by_hand():
    x = np.array([[[[1.0, 0.0, 2.0, 2.0, 0.0]], [[0.0, 3.0, 2.0, 1.0, 0.0]]]])  # argmax: 0 1 0(tie) 0 0(tie)
    y = np.array([[[0, 0, 1, IGN, 1]]])
    c = R.hard_counts(x, y, ignore=IGN)
    assert c.tolist() == [[[1, 2, 1], [0, 1, 2]]]  # class 0: tp 1, fp 2 (pixels 2, 4), fn 1; class 1: tp 0, fp 1, fn 2
    assert R.hard_counts(x, np.array([[[0, 0, 1, 0, 1]]])).tolist() == [[[2, 2, 1], [0, 1, 2]]]
    # top-k: ten pixels, all-zero logits except known ones -> nll known; k = 30 % -> the 3 largest
    x = np.zeros((1, 2, 1, 10))
    x[0, 0, 0, :4] = [3.0, 2.0, 1.0, 0.5]  # label 1 everywhere: nll = log(1 + e^x)
    o = R.topk_ce(x, np.ones((1, 1, 1, 10), dtype=np.int64), 30)
    want = np.log1p(np.exp([3.0, 2.0, 1.0])).mean()
    assert o["n"] == 3 and o["n_gt"] == 2 and o["n_eq"] == 1 and abs(o["loss"] - want) < 1e-15
    assert (o["grad"][0, 0, 0] != 0).tolist() == [True] * 3 + [False] * 7
    # the tie rule: all ten pixels equal, n = 3 -> value ln 2, every pixel carries 3/10 of one pixel's gradient
    o = R.topk_ce(np.zeros((1, 2, 1, 10)), np.ones((1, 1, 1, 10), dtype=np.int64), 30)
    assert o["n_gt"] == 0 and o["n_eq"] == 10 and abs(o["loss"] - np.log(2.0)) < 1e-15
    np.testing.assert_allclose(o["grad"][0, 0, 0], np.full(10, 0.5 * 0.3 / 3), atol=1e-16, rtol=0)
    assert np.isnan(R.topk_ce(np.zeros((1, 2, 1, 5)), np.ones((1, 1, 1, 5), dtype=np.int64), 10)["loss"])  # n = int(0.5) = 0


def test_restatement_matches_every_golden_record(golden_dir):
    d, meta = load_golden(golden_dir)
    seen = set()
    for c in meta:
        if c["kind"] == "tpfpfn":
            continue
        o = restate(c, d)
        seen.add(c["kind"])
        dv = abs(o["loss"] - float(d[f"c/{c['name']}/loss"]))
        dg = np.abs(o["grad"] - d[f"c/{c['name']}/grad"]).max()
        print(f"{c['name']}: |dvalue| {dv:.2e} |dgrad| {dg:.2e}")
        assert dv < VAL_TOL and dg < GRAD_ATOL, (c["name"], dv, dg)
        if c["kind"] == "topk":
            assert o["n_eq"] == 1  # no exact tie: torch.topk's answer is defined
    assert seen == {"dcce", "dice", "rce", "topk"}


def test_tensor_op_tp_fp_fn_tn_matches_golden(golden_dir):
    from losses.dice_loss import get_tp_fp_fn_tn
    d, meta = load_golden(golden_dir)
    n = 0
    for c in meta:
        if c["kind"] != "tpfpfn":
            continue
        n += 1
        x = torch.from_numpy(d[f"in/{c['set']}/logits"])
        y = torch.from_numpy(d[f"in/{c['set']}/{c['labels']}"].astype(np.int64))
        pred = torch.zeros_like(x).scatter_(1, x.argmax(1)[:, None], 1) if c["hard"] else torch.softmax(x, 1)
        mask = None if c["mask_from"] is None else torch.from_numpy(d[f"in/{c['set']}/{c['mask_from']}"] != IGN).float()
        got = get_tp_fp_fn_tn(pred, y, axes=c["axes"], mask=mask, square=c["square"])
        for name, g in zip(("tp", "fp", "fn", "tn"), got):
            want = d[f"c/{c['name']}/{name}"]
            assert g.shape == want.shape
            np.testing.assert_allclose(g.numpy(), want, rtol=1e-6, atol=1e-6)
        if c["hard"]:  # the restatement's integer counts, summed over the batch, are the same numbers
            ign = None
            lab = y.numpy()
            if c["mask_from"] is not None:
                lab, ign = d[f"in/{c['set']}/{c['mask_from']}"].astype(np.int64), IGN
            cnt = R.hard_counts(x.numpy(), lab, ign).sum(0)
            for j, name in enumerate(("tp", "fp", "fn")):
                assert cnt[:, j].tolist() == d[f"c/{c['name']}/{name}"].astype(np.int64).tolist()
    assert n == 3
    # [B, H, W] labels and axes=() (no summation) keep the reference's shapes
    tp, fp, fn, tn = get_tp_fp_fn_tn(torch.rand(2, 3, 4, 5), torch.randint(0, 3, (2, 4, 5)), axes=())
    assert tp.shape == (2, 3, 4, 5) and torch.allclose(tp + fp + fn + tn, torch.ones(2, 3, 4, 5))


def test_constructors_follow_the_reference():
    from losses.ce_loss import RobustCrossEntropyLoss, TopKLoss
    from losses.compound_losses import DC_and_CE_loss, softmax_helper_dim1
    from losses.dice_loss import MemoryEfficientSoftDiceLoss
    from losses import dice_loss
    d = MemoryEfficientSoftDiceLoss()
    assert (d.apply_nonlin, d.batch_dice, d.do_bg, d.smooth) == (None, False, True, 1.0)
    d = MemoryEfficientSoftDiceLoss(softmax_helper_dim1, True, False, 1e-5)
    assert d.apply_nonlin is softmax_helper_dim1 and d.batch_dice and not d.do_bg and d.smooth == 1e-5
    assert dice_loss.softmax_helper_dim1 is softmax_helper_dim1
    assert torch.equal(softmax_helper_dim1(torch.ones(1, 4, 2, 2)), torch.full((1, 4, 2, 2), 0.25))
    ce_kwargs = {}
    l = DC_and_CE_loss({"smooth": 1e-5, "do_bg": False}, ce_kwargs, ignore_label=255)
    assert (l.weight_ce, l.weight_dice, l.ignore_label) == (1, 1, 255)
    assert isinstance(l.ce, RobustCrossEntropyLoss) and l.ce.ignore_index == 255 and ce_kwargs == {"ignore_index": 255}
    assert isinstance(l.dc, MemoryEfficientSoftDiceLoss) and l.dc.apply_nonlin is softmax_helper_dim1 and l.dc.smooth == 1e-5
    l = DC_and_CE_loss({}, {"weight": torch.tensor([0.2, 1.0, 3.0])}, weight_ce=0.9, weight_dice=0.6)
    assert l.ignore_label is None and l.ce.ignore_index == -100 and l.ce.weight.tolist() == pytest.approx([0.2, 1.0, 3.0])
    t = TopKLoss()
    assert (t.k, t.ignore_index, t.weight, t.label_smoothing, t.reduction) == (10, -100, None, 0, "none")
    t = TopKLoss(torch.tensor([1.0, 2.0]), 255, 25)
    assert t.k == 25 and t.ignore_index == 255 and isinstance(t, RobustCrossEntropyLoss)


def test_unsupported_and_cpu_cases_raise():
    import mia_hip
    from losses.ce_loss import RobustCrossEntropyLoss, TopKLoss
    from losses.compound_losses import DC_and_CE_loss, softmax_helper_dim1
    from losses.dice_loss import MemoryEfficientSoftDiceLoss, hard_tp_fp_fn
    x, y = torch.zeros(2, 3, 4, 4), torch.zeros(2, 1, 4, 4, dtype=torch.long)
    # no CPU fallback
    for fn in (DC_and_CE_loss({}, {}), DC_and_CE_loss({}, {}, ignore_label=255), MemoryEfficientSoftDiceLoss(softmax_helper_dim1),
               RobustCrossEntropyLoss(ignore_index=255), RobustCrossEntropyLoss(weight=torch.ones(3)), TopKLoss(k=25)):
        with pytest.raises(mia_hip.MiaError):
            fn(x, y)
    with pytest.raises(mia_hip.MiaError):
        hard_tp_fp_fn(x, y)
    # foreign non-linearity, one-hot targets, 3-D inputs, label smoothing, other reductions
    with pytest.raises(NotImplementedError):
        MemoryEfficientSoftDiceLoss(torch.sigmoid)(x, y)
    with pytest.raises(NotImplementedError):
        MemoryEfficientSoftDiceLoss()(x, torch.zeros(2, 3, 4, 4))
    with pytest.raises(NotImplementedError):
        DC_and_CE_loss({}, {})(x, torch.zeros(2, 3, 4, 4))
    x3, y3 = torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4, dtype=torch.long)
    for fn in (DC_and_CE_loss({}, {}), MemoryEfficientSoftDiceLoss(), TopKLoss()):
        with pytest.raises(NotImplementedError):
            fn(x3, y3)
    with pytest.raises(NotImplementedError):
        RobustCrossEntropyLoss(ignore_index=255, label_smoothing=0.1)(x, y)
    with pytest.raises(NotImplementedError):
        RobustCrossEntropyLoss(weight=torch.ones(3), reduction="sum")(x, y)
    with pytest.raises(NotImplementedError):
        TopKLoss(label_smoothing=0.1)(x, y)
    with pytest.raises(NotImplementedError):
        DC_and_CE_loss({}, {"label_smoothing": 0.1})(x, y)
    with pytest.raises(AssertionError):  # the reference asserts a [B,1,H,W] target when an ignore label is set
        DC_and_CE_loss({}, {}, ignore_label=255)(x, y[:, 0])


def test_header_declares_and_library_exports_the_entry_points():
    import __graft_entry__ as ge
    import mia_hip
    ge.build()
    protos = mia_hip.parse_header()
    l = ctypes.CDLL(mia_hip.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in protos, f"{name} missing from include/mia_hip.h"
        assert hasattr(l, name), f"{name} not exported by the built library"
    d = mia_hip.parse_defines()
    pairs = {"MIA_SEGLOSS_SOFTMAX": mia_hip.SEGLOSS_SOFTMAX, "MIA_SEGLOSS_DO_BG": mia_hip.SEGLOSS_DO_BG,
             "MIA_SEGLOSS_BATCH": mia_hip.SEGLOSS_BATCH, "MIA_SEGLOSS_LABEL_U8": mia_hip.SEGLOSS_LABEL_U8,
             "MIA_SEGLOSS_IGNORE": mia_hip.SEGLOSS_IGNORE}
    for name, val in pairs.items():
        assert d.get(name) == val, (name, d.get(name), val)
    # argument errors surface without a GPU
    lib = mia_hip.lib()
    assert lib.mia_seg_loss_fwd(None, None, None, 1, 16, 3, 48, 1, 3, 0, 0, 1.0, 1.0, 1.0, 1, None, None, None, None, None, None) < 0
    assert b"mia_seg_loss_fwd" in lib.mia_last_error()
    assert lib.mia_topk_ce_workspace(0) == 0 and lib.mia_topk_ce_workspace(100) > 100
    assert lib.mia_seg_loss_workspace(2, 3, 4) >= 2 * 4 * (5 * 3 + 2)
