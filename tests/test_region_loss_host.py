"""CPU checks of the region-based mode (sigmoid soft Dice + BCE, and the region-to-label rule): the imports and constructors of
`DC_and_BCE_loss` / `DC_and_topk_loss`, the float64 restatement (tests/_region_loss_ref.py) against hand-computed answers and
against every record of tests/golden/region_losses.npz (the reference's own fp32 numbers with its own fp32 error),
`expand_regions`, the CPU branch of `ensemble_predict_regions`, the error cases and the C-ABI declarations -- no GPU needed."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _region_loss_ref as R

ENTRY_POINTS = ("mia_region_loss_workspace", "mia_region_loss_fwd", "mia_region_loss_bwd", "mia_sigmoid_accum")
POS_WEIGHT = {1: [2.5], 3: [0.5, 2.0, 3.0], 4: [0.5, 2.0, 3.0, 1.25]}  # tools/gen_region_loss_golden.py
LN2 = float(np.log(2.0))


def load_golden(golden_dir):
    d = np.load(os.path.join(golden_dir, "region_losses.npz"))
    return d, json.loads(str(d["meta"]))


def case_target(c, d):
    """The dense numpy target of one golden case as recorded: uint8 0/1 mask ("bool", "float") or the fp32 soft target, with the
    ignore channel (recorded, or all ones) appended in the same dtype."""
    t = d[f"in/{c['set']}/soft"] if c["target"] == "soft" else d[f"in/{c['set']}/mask"]
    if c["ignore"] is None:
        return t
    ign = d[f"in/{c['set']}/ign"]
    if c["ignore"] == "all":
        ign = np.ones_like(ign)
    return np.concatenate((t, ign.astype(t.dtype)), 1)


def case_kwargs(c, channels):
    return dict(pos_weight=POS_WEIGHT[channels] if c["pos_weight"] else None, smooth=c["smooth"], do_bg=c["do_bg"],
                batch_dice=c["batch_dice"], ce_w=c["weight_ce"], dice_w=c["weight_dice"])


def restate(c, d):
    x = d[f"in/{c['set']}/logits"]
    return R.region_loss_dense(x, case_target(c, d), c["ignore"] is not None, **case_kwargs(c, x.shape[1]))


class Fixed(torch.nn.Module):
    """A stand-in network: returns fixed logits, records the mode it was called in, optionally raises."""

    def __init__(self, logits, fail=False):
        super().__init__()
        self.logits, self.fail, self.seen = logits, fail, []

    def forward(self, x):
        self.seen.append(self.training)
        if self.fail:
            raise RuntimeError("boom")
        return self.logits


# ------------------------------------------------------------------------------------------------ imports and constructors
def test_imports_and_constructors():
    """Both names import from `losses.compound_losses` (an ImportError before this feature) and the constructors leave the
    reference's attributes and side effects behind (compound_losses.py:178-208, :236-265)."""
    from losses.ce_loss import TopKLoss
    from losses.compound_losses import DC_and_BCE_loss, DC_and_topk_loss, softmax_helper_dim1
    from losses.dice_loss import MemoryEfficientSoftDiceLoss
    kw = {}
    fn = DC_and_BCE_loss(kw, dict(batch_dice=True, do_bg=False, smooth=1e-5), weight_ce=0.5, weight_dice=2)
    assert kw == {} and (fn.weight_ce, fn.weight_dice, fn.use_ignore_label) == (0.5, 2, False)
    assert type(fn.ce) is torch.nn.BCEWithLogitsLoss and fn.ce.reduction == "mean"
    assert type(fn.dc) is MemoryEfficientSoftDiceLoss and fn.dc.apply_nonlin is torch.sigmoid
    assert (fn.dc.batch_dice, fn.dc.do_bg, fn.dc.smooth) == (True, False, 1e-5)
    kw = {"pos_weight": torch.ones(3, 1, 1)}
    fn = DC_and_BCE_loss(kw, {}, use_ignore_label=True)
    assert kw["reduction"] == "none" and fn.ce.reduction == "none" and fn.use_ignore_label is True  # the caller's dict is mutated
    assert (fn.weight_ce, fn.weight_dice) == (1, 1) and (fn.dc.batch_dice, fn.dc.do_bg, fn.dc.smooth) == (False, True, 1.0)
    assert fn.last_ce is None and fn.last_dc is None and fn.last_hard_counts is None

    class Other(torch.nn.Module):
        def __init__(self, apply_nonlin=None, **kw):
            super().__init__()
            self.apply_nonlin = apply_nonlin
    assert DC_and_BCE_loss({}, {}, dice_class=Other).dc.apply_nonlin is torch.sigmoid
    # the index form is keyword-only and wants regions and the ignore label together
    fn = DC_and_BCE_loss({}, {}, use_ignore_label=True, regions=((1, 2), (1,)), ignore_label=255)
    assert fn.regions == ((1, 2), (1,)) and fn.ignore_label == 255
    with pytest.raises(TypeError):
        DC_and_BCE_loss({}, {}, 1, 1, False, MemoryEfficientSoftDiceLoss, ((1,),))
    with pytest.raises(ValueError):
        DC_and_BCE_loss({}, {}, ignore_label=255)
    with pytest.raises(ValueError):
        DC_and_BCE_loss({}, {}, regions=((1,),), ignore_label=255)

    kw = {"k": 25}
    fn = DC_and_topk_loss(dict(batch_dice=True, do_bg=False, smooth=1e-5), kw, weight_ce=0.25, weight_dice=3, ignore_label=7)
    assert kw == {"k": 25, "ignore_index": 7}
    assert (fn.weight_ce, fn.weight_dice, fn.ignore_label) == (0.25, 3, 7)
    assert type(fn.ce) is TopKLoss and fn.ce.k == 25 and fn.ce.ignore_index == 7
    assert type(fn.dc) is MemoryEfficientSoftDiceLoss and fn.dc.apply_nonlin is softmax_helper_dim1
    assert (fn.dc.batch_dice, fn.dc.do_bg, fn.dc.smooth) == (True, False, 1e-5)
    fn = DC_and_topk_loss({}, {})
    assert fn.ignore_label is None and fn.ce.ignore_index == -100 and fn.ce.k == 10
    assert "SoftDiceLoss" in DC_and_topk_loss.__doc__ and "NameError" in DC_and_topk_loss.__doc__


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_hand_computed():
    ones = np.ones((2, 4, 5), bool)
    for c in (1, 2, 3):
        t = (np.arange(2 * c * 4 * 5) % 3 == 0).reshape(2, c, 4, 5).astype(np.float64)
        # all-zero logits: p = 1/2, every BCE element is ln 2 -> the mean is ln 2; gradient of the CE term (1/2 - t) / N
        o = R.region_loss(np.zeros((2, c, 4, 5)), t, ones, False, dice_w=0.0)
        assert abs(o["ce"] - LN2) < 1e-15 and abs(o["value"] - LN2) < 1e-15
        np.testing.assert_allclose(o["grad"], (0.5 - t) / (2 * c * 20), atol=1e-17, rtol=0)
        # ... and with an ignore channel that is empty the divisor counts pixels, not elements: C ln 2
        o = R.region_loss(np.zeros((2, c, 4, 5)), t, ones, True, dice_w=0.0)
        assert abs(o["ce"] - c * LN2) < 1e-14
        o = R.region_loss_dense(np.zeros((2, c, 4, 5)), np.concatenate((t, np.zeros((2, 1, 4, 5))), 1), True, dice_w=0.0)
        assert abs(o["ce"] - c * LN2) < 1e-14
    # Dice by hand: one image, two channels, four pixels; logits ln 3 / -ln 3 / 0 give p = 3/4, 1/4, 1/2
    l3 = np.log(3.0)
    z = np.array([[[[l3, -l3, 0.0, l3]], [[-l3, 0.0, l3, 0.0]]]])
    t = np.array([[[[1, 0, 1, 1]], [[0, 1, 1, 0]]]], np.float64)
    v = np.ones((1, 1, 4), bool)
    o = R.region_loss(z, t, v, False, smooth=1.0, ce_w=0.0)
    # channel 0: p = .75 .25 .5 .75 -> I = 2, P = 2.25, G = 3;  channel 1: p = .25 .5 .75 .5 -> I = 1.25, P = 2, G = 2
    want = -0.5 * ((2 * 2 + 1) / (3 + 2.25 + 1) + (2 * 1.25 + 1) / (2 + 2 + 1))
    assert abs(o["dc"] - want) < 1e-15 and abs(o["value"] - want) < 1e-15
    o = R.region_loss(z, t, v, False, smooth=1.0, do_bg=False, ce_w=0.0)
    assert abs(o["dc"] + (2 * 1.25 + 1) / (2 + 2 + 1)) < 1e-15 and not o["grad"][:, 0].any()
    # counts of (z > 0) against t: channel 0 predicts 1 0 0 1 -> tp 2, fp 0, fn 1; channel 1 predicts 0 0 1 0 -> tp 1, fp 0, fn 1
    assert o["counts"].tolist() == [[[2, 0, 1], [1, 0, 1]]]
    # the third pixel ignored: channel 1 keeps I = .5, P = 1.25, G = 1 and that pixel gets no gradient
    v3 = np.array([[[True, True, False, True]]])
    o = R.region_loss(z, t, v3, True, smooth=1.0, do_bg=False, ce_w=0.0)
    assert abs(o["dc"] + (2 * 0.5 + 1) / (1 + 1.25 + 1)) < 1e-15 and not o["grad"][:, :, :, 2].any()
    assert o["counts"].tolist() == [[[2, 0, 0], [0, 0, 1]]]
    # batch Dice: I, P, G of two copies of the image add up first
    o2 = R.region_loss(np.concatenate((z, z)), np.concatenate((t, t)), np.ones((2, 1, 4), bool), False, smooth=1.0, batch_dice=True, ce_w=0.0)
    want = -0.5 * ((2 * 4 + 1) / (6 + 4.5 + 1) + (2 * 2.5 + 1) / (4 + 4 + 1))
    assert abs(o2["dc"] - want) < 1e-15
    # pos_weight by hand: one pixel per channel, z = 0: t = 1 costs pw ln 2, t = 0 costs ln 2 whatever pw
    o = R.region_loss(np.zeros((1, 2, 1, 1)), np.array([[[[1.0]], [[0.0]]]]), np.ones((1, 1, 1), bool), False, pos_weight=[3.0, 5.0], dice_w=0.0)
    assert abs(o["ce"] - (3 * LN2 + LN2) / 2) < 1e-15
    np.testing.assert_allclose(o["grad"].ravel(), [(0.5 * 3 - 3) / 2, 0.5 / 2], atol=1e-16, rtol=0)
    # z = ln 3, t = 1, pw = 2: 2 softplus(-ln 3) = 2 ln(4/3)
    o = R.region_loss(np.full((1, 1, 1, 1), l3), np.ones((1, 1, 1, 1)), np.ones((1, 1, 1), bool), False, pos_weight=[2.0], dice_w=0.0)
    assert abs(o["ce"] - 2 * np.log(4.0 / 3.0)) < 1e-15
    # a fully ignored image: dc = -smooth / smooth, CE = 0 / 1e-8, no gradient
    rs = np.random.RandomState(0)
    o = R.region_loss(rs.randn(2, 3, 4, 5), (rs.rand(2, 3, 4, 5) < 0.5), np.zeros((2, 4, 5), bool), True, do_bg=False, smooth=1e-5)
    assert o["dc"] == -1.0 and o["ce"] == 0.0 and o["value"] == -1.0 and not o["grad"].any() and not o["counts"].any()
    # the gradient is the derivative: central differences on a small case with every option on
    z = rs.randn(2, 3, 2, 3)
    t = rs.rand(2, 3, 2, 3)
    v = rs.rand(2, 2, 3) < 0.7
    kw = dict(pos_weight=[0.5, 2.0, 3.0], smooth=1e-5, do_bg=False, batch_dice=True, ce_w=0.7, dice_w=0.4)
    o = R.region_loss(z, t, v, True, **kw)
    num = np.zeros_like(z)
    for i in np.ndindex(*z.shape):
        zp, zm = z.copy(), z.copy()
        zp[i] += 1e-6
        zm[i] -= 1e-6
        num[i] = (R.region_loss(zp, t, v, True, **kw)["value"] - R.region_loss(zm, t, v, True, **kw)["value"]) / 2e-6
    np.testing.assert_allclose(o["grad"], num, atol=1e-8, rtol=0)


def test_restatement_matches_every_golden_record(golden_dir):
    """fp64 restatement against the reference's fp32 record, within the record's own fp32 error (the reference's fp32 run against
    its float64 run) times 2: the comparison is fp32 against fp64 on both sides."""
    d, meta = load_golden(golden_dir)
    assert len(meta) == 15
    for c in meta:
        o = restate(c, d)
        v, g = float(d[f"c/{c['name']}/loss"]), d[f"c/{c['name']}/grad"].astype(np.float64)
        ref_dv, ref_dg_rel = float(d[f"c/{c['name']}/ref_dv"]), float(d[f"c/{c['name']}/ref_dg_rel"])
        dv, dg = abs(o["value"] - v), np.abs(o["grad"] - g).max()
        gmax = np.abs(o["grad"]).max()
        print(f"{c['name']}: |dvalue| {dv:.2e} (ref {ref_dv:.2e})  |dgrad|/max|g| {dg / gmax if gmax else 0:.2e} (ref {ref_dg_rel:.2e})")
        assert dv <= 2 * ref_dv, (c["name"], dv, ref_dv)
        assert dg <= 2 * ref_dg_rel * gmax, (c["name"], dg, ref_dg_rel, gmax)
        assert g.shape == o["grad"].shape
    o = restate(next(c for c in meta if c["name"] == "a_all"), d)
    assert o["value"] == -1.0 and not o["grad"].any()
    assert float(d["c/a_all/loss"]) == -1.0 and not d["c/a_all/grad"].any()


# ------------------------------------------------------------------------------------------------ regions
def test_expand_regions_by_hand():
    from losses.regions import expand_regions
    lab = torch.tensor([[[0, 1, 2], [3, 255, 1]]])
    got = expand_regions(lab, ((1, 2), (1,)))
    assert got.dtype == torch.bool and got.shape == (1, 2, 2, 3)
    assert got[0, 0].tolist() == [[False, True, True], [False, False, True]]   # object = label 1 or 2
    assert got[0, 1].tolist() == [[False, True, False], [False, False, True]]  # label 1 only: lies inside the object
    got = expand_regions(lab[:, None].to(torch.uint8), ((1, 2, 3), (2, 3), (3,)), ignore_label=255)
    assert got.shape == (1, 4, 2, 3)
    assert got[0, 0].tolist() == [[False, True, True], [True, False, True]]
    assert got[0, 1].tolist() == [[False, False, True], [True, False, False]]
    assert got[0, 2].tolist() == [[False, False, False], [True, False, False]]
    assert got[0, 3].tolist() == [[False, False, False], [False, True, False]]  # the ignore channel
    # the numpy restatement means the same thing
    t, valid = R.expand_regions(lab.numpy(), ((1, 2, 3), (2, 3), (3,)), 255)
    assert np.array_equal(t, got[:, :3].numpy().astype(np.float64)) and np.array_equal(valid, ~got[:, 3].numpy())
    with pytest.raises(ValueError):
        expand_regions(torch.zeros(1, 2, 4, 4, dtype=torch.long), ((1,),))
    with pytest.raises(ValueError):
        expand_regions(lab, ())


def test_region_bits_table():
    from mia_hip import ops
    assert ops.region_bits(((1, 2), (1,)), "cpu").tolist() == [0, 3, 1]
    assert ops.region_bits(((1, 2, 3), (2, 3), (3,)), "cpu").tolist() == [0, 1, 3, 7]
    assert ops.region_bits(((0,), ()), "cpu").tolist() == [1]
    with pytest.raises(NotImplementedError):
        ops.region_bits([(i,) for i in range(9)], "cpu")


# ------------------------------------------------------------------------------------------------ prediction, CPU branch
def test_ensemble_predict_regions_cpu_branch():
    from inference import ensemble_predict_regions, regions_to_labels
    g = torch.Generator().manual_seed(0)
    logits = [3 * torch.randn(2, 3, 9, 11, generator=g) for _ in range(3)]
    weights = [0.5, 1.0, 2.0]
    order = [1, 2, 3]
    models = [Fixed(l) for l in logits]
    models[1].eval()
    pred, prob = ensemble_predict_regions(models, torch.zeros(1), order, weights, return_probs=True)
    want_sum = R.sigmoid_sum([l.numpy() for l in logits], weights)
    assert pred.dtype == torch.int64 and pred.shape == (2, 9, 11) and prob.dtype == torch.float32
    assert np.abs(prob.numpy() - want_sum).max() < 1e-6 * sum(weights)
    want = R.regions_to_labels(want_sum, order, 0.5 * sum(weights))
    far = (np.abs(want_sum / sum(weights) - 0.5) > 1e-5).all(1)
    assert far.mean() > 0.999 and np.array_equal(pred.numpy()[far], want[far])
    assert np.array_equal(pred.numpy(), R.regions_to_labels(prob.numpy(), order, np.float32(0.5 * sum(weights))))
    assert [m.seen for m in models] == [[False]] * 3 and [m.training for m in models] == [True, False, True]
    # the rule: a later region overwrites an earlier one, nothing above the threshold is background
    p = torch.tensor([[[[0.9, 0.9, 0.1, 0.9]], [[0.1, 0.9, 0.9, 0.9]], [[0.1, 0.1, 0.1, 0.9]]]])
    assert regions_to_labels(p, [5, 6, 7], 0.5).tolist() == [[[5, 6, 6, 7]]]
    assert regions_to_labels(p, [7, 6, 5], 0.5).tolist() == [[[7, 6, 6, 5]]]
    assert regions_to_labels(torch.full((1, 2, 1, 2), 0.5), [1, 2], 0.5).tolist() == [[[0, 0]]]  # strictly above
    # one model: the plain thresholded map of its logits
    assert torch.equal(ensemble_predict_regions([Fixed(logits[0])], torch.zeros(1), order),
                       regions_to_labels(logits[0].sigmoid(), order, 0.5))
    # every model gets its mode back after an exception
    models = [Fixed(logits[0]), Fixed(logits[1], fail=True), Fixed(logits[2])]
    models[2].eval()
    with pytest.raises(RuntimeError):
        ensemble_predict_regions(models, torch.zeros(1), order)
    assert [m.training for m in models] == [True, True, False]
    with pytest.raises(ValueError):
        ensemble_predict_regions([], torch.zeros(1), order)
    with pytest.raises(ValueError):
        ensemble_predict_regions([Fixed(logits[0])], torch.zeros(1), [1, 2])
    with pytest.raises(ValueError):
        ensemble_predict_regions([Fixed(logits[0])], torch.zeros(1), order, weights=[1.0, 2.0])


# ------------------------------------------------------------------------------------------------ error cases
def test_error_cases():
    import mia_hip
    from inference import sigmoid_accum
    from losses.compound_losses import DC_and_BCE_loss, DC_and_CE_loss, DC_and_topk_loss
    from losses.dice_loss import MemoryEfficientSoftDiceLoss
    from mia_hip import ops
    x = torch.zeros(2, 3, 4, 4)
    dense = torch.zeros(2, 3, 4, 4, dtype=torch.bool)
    # no CPU fallback anywhere
    for fn, t in ((DC_and_BCE_loss({}, {}), dense), (DC_and_BCE_loss({}, {}, use_ignore_label=True), torch.zeros(2, 4, 4, 4)),
                  (DC_and_BCE_loss({}, {}, regions=((1, 2), (1,), (2,))), torch.zeros(2, 1, 4, 4, dtype=torch.uint8)),
                  (MemoryEfficientSoftDiceLoss(torch.sigmoid), dense.float()),
                  (DC_and_topk_loss({}, {}), torch.zeros(2, 1, 4, 4, dtype=torch.long))):
        with pytest.raises(mia_hip.MiaError):
            fn(x, t)
    with pytest.raises(mia_hip.MiaError):
        MemoryEfficientSoftDiceLoss(torch.sigmoid)(x, dense, loss_mask=torch.ones(2, 1, 4, 4))
    with pytest.raises(mia_hip.MiaError):
        ops.RegionLossFn.apply(x, dense, None, None, 1, None, 1.0, 1.0, 1.0, 0)
    with pytest.raises(mia_hip.MiaError):
        sigmoid_accum(x, torch.zeros(2, 3, 4, 4), None, None, 1.0, 0.5, True)
    # what the kernel does not implement
    with pytest.raises(NotImplementedError):
        DC_and_BCE_loss({"weight": torch.ones(3, 1, 1)}, {})(x, dense)
    for red in ("sum", "none"):
        with pytest.raises(NotImplementedError):
            DC_and_BCE_loss({"reduction": red}, {})(x, dense)
    with pytest.raises(NotImplementedError):
        DC_and_BCE_loss({"pos_weight": torch.ones(3)}, {})(x, dense)  # would broadcast over W, not over the channels
    with pytest.raises(NotImplementedError):
        DC_and_BCE_loss({"pos_weight": torch.ones(1, 1, 1)}, {})(x, dense)
    with pytest.raises(NotImplementedError):
        DC_and_BCE_loss({}, {})(torch.zeros(2, 3, 4, 4, 4), torch.zeros(2, 3, 4, 4, 4))
    with pytest.raises(NotImplementedError):
        DC_and_BCE_loss({}, {})(torch.zeros(2, 9, 4, 4), torch.zeros(2, 9, 4, 4))
    with pytest.raises(NotImplementedError):
        MemoryEfficientSoftDiceLoss(torch.sigmoid)(torch.zeros(2, 9, 4, 4), torch.zeros(2, 9, 4, 4))
    with pytest.raises(ValueError):
        DC_and_BCE_loss({}, {"do_bg": False})(torch.zeros(2, 1, 4, 4), torch.zeros(2, 1, 4, 4))
    with pytest.raises(ValueError):
        MemoryEfficientSoftDiceLoss(torch.sigmoid, do_bg=False)(torch.zeros(2, 1, 4, 4), torch.zeros(2, 1, 4, 4))
    # the two cases tests/test_seg_loss_host.py pins keep raising, and so does everything else that raised before
    y = torch.zeros(2, 1, 4, 4, dtype=torch.long)
    with pytest.raises(NotImplementedError):
        MemoryEfficientSoftDiceLoss(torch.sigmoid)(x, y)
    with pytest.raises(NotImplementedError):
        MemoryEfficientSoftDiceLoss()(x, torch.zeros(2, 3, 4, 4))
    with pytest.raises(NotImplementedError):
        MemoryEfficientSoftDiceLoss(torch.tanh)(x, torch.zeros(2, 3, 4, 4))
    with pytest.raises(NotImplementedError):
        DC_and_CE_loss({}, {})(x, torch.zeros(2, 3, 4, 4))


def test_foreign_dice_class_falls_back_to_the_reference_composition():
    """A Dice class that is not the project's runs the reference's forward in tensor ops (on any device) -- checked against the
    restatement with a plain-torch sigmoid Dice, dense and through `regions`."""
    from losses.compound_losses import DC_and_BCE_loss

    class TorchDice(torch.nn.Module):
        def __init__(self, apply_nonlin=None, smooth=1.0):
            super().__init__()
            self.apply_nonlin, self.smooth = apply_nonlin, smooth

        def forward(self, x, y, loss_mask=None):
            p = self.apply_nonlin(x)
            m = 1.0 if loss_mask is None else loss_mask
            i, s, g = (p * y * m).sum((2, 3)), (p * m).sum((2, 3)), (y * m).sum((2, 3))
            return -((2 * i + self.smooth) / torch.clip(g + s + self.smooth, 1e-8)).mean()

    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 2, 5, 6, generator=g, dtype=torch.float64)
    lab = torch.randint(0, 4, (2, 1, 5, 6), generator=g)
    lab[0, 0, 0, :3] = 255
    fn = DC_and_BCE_loss({}, {}, weight_ce=0.5, use_ignore_label=True, dice_class=TorchDice, regions=((1, 2), (1,)), ignore_label=255)
    want = R.region_loss_index(x.numpy(), lab.numpy(), ((1, 2), (1,)), 255, ce_w=0.5)
    assert abs(float(fn(x, lab)) - want["value"]) < 1e-12
    dense = (torch.rand(2, 2, 5, 6, generator=g) < 0.5)
    want = R.region_loss_dense(x.numpy(), dense.numpy(), False)
    assert abs(float(DC_and_BCE_loss({}, {}, dice_class=TorchDice)(x, dense)) - want["value"]) < 1e-12


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_declares_and_exports_the_region_entry_points():
    import mia_hip
    import __graft_entry__ as ge
    ge.build()
    protos = mia_hip.parse_header()
    l = ctypes.CDLL(mia_hip.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in protos, f"{name} is not declared in include/mia_hip.h"
        assert hasattr(l, name), f"{name} is not exported"
    assert len(protos["mia_region_loss_fwd"][1]) == 23 and len(protos["mia_region_loss_bwd"][1]) == 20
    assert len(protos["mia_sigmoid_accum"][1]) == 14 and len(protos["mia_region_loss_workspace"][1]) == 3
    d = mia_hip.parse_defines()
    pairs = {"MIA_REGLOSS_DO_BG": mia_hip.REGLOSS_DO_BG, "MIA_REGLOSS_BATCH": mia_hip.REGLOSS_BATCH,
             "MIA_REGLOSS_IGNORE": mia_hip.REGLOSS_IGNORE, "MIA_REGLOSS_INDEX": mia_hip.REGLOSS_INDEX,
             "MIA_REGLOSS_TARGET_U8": mia_hip.REGLOSS_TARGET_U8}
    for name, val in pairs.items():
        assert d.get(name) == val, (name, d.get(name), val)
    assert len(set(pairs.values())) == 5 and all(v & (v - 1) == 0 for v in pairs.values())  # distinct single bits


def test_argument_errors_are_reported_without_a_gpu():
    """The host-side checks of the new entry points return MIA_EARG before anything is launched."""
    import mia_hip
    l = mia_hip.lib()
    i64, f32 = ctypes.c_int64, ctypes.c_float
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16)

    def fwd(c=3, flags=1, bits=None, n_labels=0, hw=16, slabs=1, logits=p):
        return l.mia_region_loss_fwd(logits, p, bits, n_labels, None, 1, i64(hw), c, i64(c * hw), i64(hw), i64(1), flags, i64(0), f32(1.0),
                                     f32(1.0), f32(1.0), slabs, p, p, p, p, p, None)

    assert fwd(c=9) < 0 and b"not in [1,8]" in l.mia_last_error()
    assert fwd(c=0) < 0
    assert fwd(c=1, flags=0) < 0 and b"no Dice term" in l.mia_last_error()
    assert fwd(flags=8) < 0 and b"region_bits" in l.mia_last_error()
    assert fwd(flags=64) < 0 and b"unknown flag" in l.mia_last_error()
    assert fwd(hw=0) < 0 and fwd(slabs=0) < 0 and fwd(logits=None) < 0
    assert l.mia_region_loss_bwd(p, p, None, 0, None, None, None, p, 1, i64(16), 3, i64(48), i64(16), i64(1), i64(48), i64(16), i64(1), 1,
                                 i64(0), None) < 0
    assert l.mia_region_loss_workspace(0, 3, 1) == 0 and l.mia_region_loss_workspace(2, 3, 2) == 2 * 2 * 20 + 2 * 3 * 6
    assert l.mia_sigmoid_accum(p, None, None, None, 1, i64(16), 3, i64(48), i64(16), i64(1), f32(1.0), f32(0.5), 1, None) < 0
    assert b"prob_sum may be NULL only" in l.mia_last_error()
    assert l.mia_sigmoid_accum(p, p, p, None, 1, i64(16), 3, i64(48), i64(16), i64(1), f32(1.0), f32(0.5), 1, None) < 0
    assert b"class_order" in l.mia_last_error()
    assert l.mia_sigmoid_accum(p, p, None, None, 1, i64(16), 9, i64(48), i64(16), i64(1), f32(1.0), f32(0.5), 1, None) < 0
