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


# ------------------------------------------------------------------ what tests/test_gpu_seg_loss_branches.py builds on
def _torch_nll(c):
    """torch's own per-pixel weighted cross-entropy in float64, [B*HW]."""
    x = torch.from_numpy(c["logits"])
    w = None if c["weight"] is None else torch.tensor(c["weight"], dtype=torch.float64)
    lab = torch.from_numpy(c["labels"])
    ign = -100 if c["ignore"] is None else c["ignore"]
    return torch.nn.functional.cross_entropy(x, lab, weight=w, ignore_index=ign, reduction="none").reshape(-1).numpy()


def test_case_builders_and_pixel_nll_against_torch():
    """The per-pixel nll of the restatement equals torch.nn.functional.cross_entropy(reduction="none") in float64, and the
    builders' switches do what they say."""
    seen = 0
    for k1 in range(1, 9):
        for ltype, ignore in (("int64", IGN), ("int64", -100), ("uint8", IGN), ("uint8", -100), ("int64", None)):
            c = R.build_case(2, k1, 37, ignore=ignore, ltype=ltype, seed=k1, weighted=k1 % 2 == 0)
            assert c["logits"].shape == (2, k1, 37) and np.array_equal(c["logits"], R.fp32(c["logits"]))
            assert c["ignore"] == (None if (ltype == "uint8" and ignore == -100) else ignore)
            n_ign = 0 if c["ignore"] is None else int((c["labels"] == c["ignore"]).sum())
            assert (n_ign > 0) == (c["ignore"] is not None)
            if ltype == "uint8":
                assert c["labels"].min() >= 0 and c["labels"].max() <= 255
            nll = R.pixel_nll(c["logits"], c["labels"], c["ignore"], c["weight"])
            assert nll.shape == (2 * 37,)
            np.testing.assert_allclose(nll, _torch_nll(c), rtol=0, atol=1e-13)
            if c["ignore"] is not None:
                assert not nll[c["labels"].reshape(-1) == c["ignore"]].any()
            assert (R.pixel_nll_bound(c["logits"], c["labels"], c["ignore"], c["weight"]) >= 0).all()
            seen += 1
    assert seen == 40
    c = R.build_case(3, 4, 50, ignore=IGN, all_ignored_image=1, absent_class=2, zero_weight_class=3)
    assert (c["labels"][1] == IGN).all() and not (c["labels"] == 2).any() and (c["labels"] == 3).any()
    assert c["weight"][3] == 0.0 and c["weight"][:3] == [float(np.float32(v)) for v in R.CLASS_WEIGHTS[:3]]
    assert R.CLASS_WEIGHTS[:4] == tuple(WEIGHTS[4])
    # the same seed gives the same case; another seed another
    d = R.build_case(3, 4, 50, ignore=IGN, all_ignored_image=1, absent_class=2, zero_weight_class=3)
    assert np.array_equal(c["logits"], d["logits"]) and np.array_equal(c["labels"], d["labels"])
    assert not np.array_equal(c["logits"], R.build_case(3, 4, 50, ignore=IGN, seed=1)["logits"])


def test_select_check_and_topk_against_torch_topk():
    """select_check on the fp32 bit patterns of a tie-free nll picks torch.topk's n-th value with r = m = 1, the restatement's top-k
    value is the mean of torch.topk's values, and ties are counted as the definitions say."""
    for name, c in R.topk_free_cases().items():
        nll = R.pixel_nll(c["logits"], c["labels"], c["ignore"], c["weight"])
        n = c["n_top"]
        top = torch.topk(torch.from_numpy(nll), n).values
        want = R.topk_ce(c["logits"], c["labels"], 100.0 * (n + 0.5) / nll.size, ignore=c["ignore"], weight=c["weight"])
        assert want["n"] == n and want["n_eq"] == 1 and abs(want["loss"] - top.mean().item()) < 1e-12 * max(1.0, top.mean().item())
        assert want["tau"] == top[-1].item()
        n32 = nll.astype(np.float32)  # rounding to fp32 moves a value by less than its bound: still no tie at the threshold
        tau, r, m = R.select_check(n32.view(np.uint32), n)
        assert (r, m) == (1, 1), name
        assert tau == int(torch.topk(torch.from_numpy(n32), n).values[-1].numpy().view(np.uint32)), name
    bits = np.array([5, 9, 9, 9, 2, 0, 0, 7], dtype=np.uint32)
    assert R.select_check(bits, 1) == (9, 1, 3) and R.select_check(bits, 3) == (9, 3, 3)
    assert R.select_check(bits, 4) == (7, 1, 1) and R.select_check(bits, 7) == (0, 1, 2) and R.select_check(bits, 8) == (0, 2, 2)
    assert R.select_check(np.array([0x3F800000, 0x3F800001], dtype=np.uint32), 1) == (0x3F800001, 1, 1)


def test_rank_gap_of_every_tie_free_case():
    """Asserted from float64 alone: with every pixel's nll moved by its bound the selection stays the same, so the device's fp32
    selection must equal the restatement's -- no case needs to be filtered at run time."""
    cases = dict(R.topk_free_cases())
    for name, (nb, hw, n_above, frac) in {"wrap-fwd": (2, 524288 + 515, 150000, 0.2), "wrap-bwd": (2, 1048576 + 1029, 200000, 0.0)}.items():
        cases[name] = R.gap_case(nb, hw, n_above, frac_ignored=frac)
    for ltype in ("int64", "uint8"):
        cases[f"labels-{ltype}"] = dict(R.label_case(ltype), n_top=R.LABEL_CASE_N_TOP)
    cases["public-128x132"] = dict(R.build_case(3, 3, 128 * 132, ignore=IGN, seed=4), n_top=int(3 * 128 * 132 * 10 / 100))
    for name, c in cases.items():
        nll = R.pixel_nll(c["logits"], c["labels"], c["ignore"], c["weight"])
        bound = R.pixel_nll_bound(c["logits"], c["labels"], c["ignore"], c["weight"])
        margin = R.selection_margin(nll, bound, c["n_top"])
        print(f"{name}: n_top {c['n_top']} of {nll.size}, max bound {bound.max():.2e}, margin {margin:.2e}")
        assert margin > 0, name
        assert np.sort(nll)[nll.size - c["n_top"]] > 1e-3, name  # and the threshold is not a zero (an ignored pixel)
    # the span case does span many exponents, so that the first radix pass (sign + 7 exponent bits) already splits the values
    c = cases["span"]
    nll = R.pixel_nll(c["logits"], c["labels"], c["ignore"], c["weight"]).astype(np.float32)
    assert np.unique(nll[nll > 0].view(np.uint32) >> 24).size >= 8
    # weight0: the zero-weight class is present and none of its pixels is selected
    c = cases["weight0"]
    assert c["weight"][2] == 0.0 and (c["labels"] == 2).any()


def test_tie_builder_claims_against_a_sort():
    for (m, r), kw in R.TIE_CASES.items():
        for k1 in (2, 3, 8):
            c = R.tie_case(m, r, k1=k1, **kw)
            nll = R.pixel_nll(c["logits"], c["labels"])
            bound = R.pixel_nll_bound(c["logits"], c["labels"])
            n = c["n_top"]
            tau = np.sort(nll)[nll.size - n]
            n_gt, n_eq = int((nll > tau).sum()), int((nll == tau).sum())
            assert (n_gt, n_eq, n - n_gt) == (c["n_gt"], m, r) == (kw["n_a"], c["m"], c["r"])
            assert np.array_equal(nll == tau, c["tied"]) and abs(tau - np.log(np.exp(1.5) + k1 - 1)) < 1e-12
            # the tied pixels are copies of one pixel, bit for bit
            t = np.flatnonzero(c["tied"])
            flat = c["logits"].transpose(0, 2, 1).reshape(-1, k1)
            assert (flat[t] == flat[t[0]]).all() and (c["labels"].reshape(-1)[t] == 1).all()
            # A stays above T and B below it by more than the bounds; A's losses are distinct
            a, b = nll > tau, nll < tau
            assert (nll[a] - bound[a]).min() > tau + bound[t[0]] and (nll[b] + bound[b]).max() < tau - bound[t[0]]
            assert np.unique(nll[a]).size == n_gt and nll[a].min() > 2.9
            assert R.selection_margin(nll, bound, n, tied=c["tied"]) > 0
            # T is spread over the images and over the 256-pixel blocks
            hw = c["labels"].shape[1]
            assert np.unique(t // hw).size == min(m, c["labels"].shape[0])
            assert np.unique(t // 256).size >= min(m, nll.size // 256)
            want = R.topk_ce(c["logits"], c["labels"], 100.0 * (n + 0.5) / nll.size)
            assert (want["n"], want["n_gt"], want["n_eq"]) == (n, n_gt, m)


def test_dense_ramp_precondition():
    """Every valid pixel's float64 nll lies in [1 + 2^-10, 1 + 2^-7 - 2^-10]: 2^-10 inside the range [1, 1 + 2^-7) whose fp32
    patterns share their upper 16 bits, a margin of 9.8e-4 against a per-pixel bound below 1e-6; and the steps of the ramp exceed
    twice that bound, so the selection is defined."""
    c = R.dense_ramp()
    nll = R.pixel_nll(c["logits"], c["labels"], c["ignore"])
    bound = R.pixel_nll_bound(c["logits"], c["labels"], c["ignore"])
    valid = c["labels"].reshape(-1) != IGN
    assert valid.sum() == c["n_valid"] and 0.75 * nll.size < c["n_valid"] < 0.85 * nll.size
    tol = 1e-7  # the logits were rounded to fp32: d moves by 2^-25 relative, the nll by less than 4e-8
    assert nll[valid].min() >= R.RAMP_LO - tol and nll[valid].max() <= R.RAMP_HI + tol and bound.max() < 1e-6
    assert 2.0 ** -10 > 500 * bound.max()
    pat = nll[valid].astype(np.float32).view(np.uint32)
    assert np.unique(pat >> 16).tolist() == [0x3F80] and np.unique(pat).size == pat.size
    assert np.unique((pat >> 8) & 0xFF).size > 100  # pass 2 has work to do, and pass 3 after it
    assert np.diff(np.sort(nll[valid])).min() > 2 * bound.max()
    assert R.selection_margin(nll, bound, c["n_top"]) > 0 and c["n_top"] == c["n_valid"] // 2
    g = R.gap_case(2, 300, 40, frac_ignored=0.2)
    gn = R.pixel_nll(g["logits"], g["labels"], g["ignore"])
    assert (gn > 3.0).sum() == 40 and ((gn > 2.0) & (gn < 2.2)).sum() == 1 and (gn[(gn < 2.0)] < 0.98).all() and g["n_top"] == 41
    assert 0.1 * 600 < (g["labels"] == IGN).sum() < 0.25 * 600
