"""GPU checks of the region-based loss (csrc/region_loss.hip: sigmoid soft Dice + BCE with an ignore channel, dense and index
targets) against the reference's recorded numbers (tests/golden/region_losses.npz) and the float64 restatement
(tests/_region_loss_ref.py), and of `DC_and_topk_loss` against the two losses it composes.

Bounds.  Value and absolute gradient bound are the project's for a fused loss against its golden (test_gpu_seg_loss.py):
|dvalue| < 2e-6 * max(1, |value|), max|dgrad| < 2e-7.  The relative gradient bound is max|dgrad| / max|grad| < max(32 * ref_dg_rel,
2^-20) with ref_dg_rel the record's own fp32 error (the reference's fp32 run against its float64 run, about 2e-7: summation
only); the factor 32 covers the kernel's few-ulp exp / log1p and its fp32 coefficient table.  Against the float64 restatement
there is no record, and ref_dg_rel is replaced by one fp32 ulp, 2^-23 -- the least an fp32 evaluation can be off: 32 * 2^-23 = 2^-18."""
import numpy as np
import pytest
import torch

import _region_loss_ref as R
from test_region_loss_host import case_kwargs, case_target, load_golden

pytestmark = pytest.mark.gpu
VAL_TOL, GRAD_ATOL = 2e-6, 2e-7
GRID_REL = 2.0 ** -18


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _store(logits, layout, dev):
    """fp32 logits on the device as a logical [B,C,H,W] tensor in plain NCHW or channels-last storage, requiring grad."""
    t = torch.as_tensor(np.asarray(logits), dtype=torch.float32).to(dev)
    if layout == "nhwc":
        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return t.requires_grad_(True)


def _loss(dev, channels, pos_weight=None, pw_4d=False, smooth=1.0, do_bg=True, batch_dice=False, ce_w=1, dice_w=1, ignore=False, **kw):
    from losses.compound_losses import DC_and_BCE_loss
    bce = {}
    if pos_weight is not None:
        pw = torch.tensor(pos_weight, device=dev)
        bce["pos_weight"] = pw.reshape(1, channels, 1, 1) if pw_4d else pw.reshape(channels, 1, 1)
    return DC_and_BCE_loss(bce, dict(batch_dice=batch_dice, do_bg=do_bg, smooth=smooth), weight_ce=ce_w, weight_dice=dice_w,
                           use_ignore_label=ignore, **kw)


def _check(name, v, g, want_v, want_g, rel_bound):
    dv, dg, gmax = abs(v - want_v), float(np.abs(g - want_g).max()), float(np.abs(want_g).max())
    rel = dg / gmax if gmax > 0 else (0.0 if dg == 0 else float("inf"))
    print(f"{name}: |dvalue| {dv:.2e} |dgrad| {dg:.2e} |dgrad|/max|g| {rel:.2e} (bound {rel_bound:.2e})")
    assert dv < VAL_TOL * max(1.0, abs(want_v)), (name, dv)
    assert dg < GRAD_ATOL, (name, dg)
    assert rel < rel_bound, (name, rel, rel_bound)


@pytest.mark.parametrize("ttype", ["bool", "uint8", "float"])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_every_golden_record(golden_dir, layout, ttype):
    """Value and logit gradient of every recorded case against the reference's own fp32 numbers; a 0/1 record runs with bool, uint8
    and float targets, a soft record with float only."""
    from mia_hip import ops
    dev = _dev()
    d, meta = load_golden(golden_dir)
    n = 0
    for c in meta:
        if c["target"] == "soft" and ttype != "float":
            continue
        x = _store(d[f"in/{c['set']}/logits"], layout, dev)
        t = torch.from_numpy(case_target(c, d)).to(dev)
        t = t.bool() if ttype == "bool" else (t.float() if ttype == "float" else t)
        assert t.dtype == {"bool": torch.bool, "uint8": torch.uint8, "float": torch.float32}[ttype]
        kw = case_kwargs(c, x.shape[1])
        fn = _loss(dev, x.shape[1], pw_4d=c["pw_4d"], ignore=c["ignore"] is not None, **kw)
        v = fn(x, t)
        v.backward()
        ref_dg_rel = float(d[f"c/{c['name']}/ref_dg_rel"])
        _check(f"{c['name']} {layout} {ttype}", v.item(), x.grad.cpu().numpy(), float(d[f"c/{c['name']}/loss"]), d[f"c/{c['name']}/grad"],
               max(32 * ref_dg_rel, 2.0 ** -20))
        assert x.grad.stride() == x.stride()
        ops.check_labels()
        n += 1
    assert n == (15 if ttype == "float" else 14)


SHAPES = [(37, 52), (19, 21), (128, 132), (130, 131)]  # vector path, scalar path, two slabs on either


def _grid_inputs(b, c, hw, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(b, c, *hw, generator=g) * 2
    mask = torch.rand(b, c, *hw, generator=g) < 0.4
    soft = torch.rand(b, c, *hw, generator=g)
    ign = torch.rand(b, 1, *hw, generator=g) < 0.2
    return logits, mask, soft, ign


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("c", [1, 2, 3, 8])
def test_grid_against_restatement(c, hw):
    """B in {1, 3} x ignore x batch_dice x do_bg x pos_weight at one (channels, size): value, gradient, CE, dc against float64 and the
    hard counts as exact integers.  Target dtype (bool, uint8, float 0/1, soft float) and logits layout rotate over the
    combinations, so every loader meets every path."""
    dev = _dev()
    pos_w = [0.5, 2.0, 3.0, 1.25, 0.75, 1.5, 2.5, 0.25][:c]
    k = 0
    for b in (1, 3):
        logits, mask, soft, ign = _grid_inputs(b, c, hw, 100 * c + hw[0] + b)
        for ignore in (False, True):
            for batch_dice in (False, True):
                for do_bg in (True, False):
                    for pw in (None, pos_w):
                        if c == 1 and not do_bg:
                            continue
                        ttype = ("bool", "uint8", "float", "soft")[k % 4]
                        layout = ("nchw", "nhwc")[(k // 4) % 2]
                        k += 1
                        t = soft if ttype == "soft" else (mask if ttype == "bool" else mask.to(torch.uint8 if ttype == "uint8" else torch.float32))
                        if ignore:
                            t = torch.cat((t, ign.to(t.dtype)), 1)
                        kw = dict(pos_weight=pw, smooth=1e-5 if batch_dice else 1.0, do_bg=do_bg, batch_dice=batch_dice, ce_w=0.7, dice_w=1.3)
                        want = R.region_loss_dense(logits.numpy(), t.numpy(), ignore, **kw)
                        x = _store(logits, layout, dev)
                        fn = _loss(dev, c, ignore=ignore, **kw)
                        v = fn(x, t.to(dev))
                        v.backward()
                        name = f"b{b} c{c} {hw} ign{int(ignore)} batch{int(batch_dice)} bg{int(do_bg)} pw{int(pw is not None)} {ttype} {layout}"
                        _check(name, v.item(), x.grad.cpu().numpy(), want["value"], want["grad"], GRID_REL)
                        assert abs(fn.last_ce.item() - want["ce"]) < VAL_TOL * max(1.0, abs(want["ce"])), name
                        assert abs(fn.last_dc.item() - want["dc"]) < VAL_TOL, name
                        assert fn.last_hard_counts.dtype == torch.int64
                        assert np.array_equal(fn.last_hard_counts.cpu().numpy(), want["counts"]), name
                        assert x.grad.stride() == x.stride()
    assert k == (16 if c == 1 else 32)


def _run(fn, x, t):
    """(out [3], counts, gradient) of one forward + backward, as device tensors."""
    from mia_hip import ops
    x = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    v = fn(x, t)
    out, counts = ops.RegionLossFn.last_out.clone(), ops.RegionLossFn.last_counts.clone()
    assert torch.equal(v.detach(), out[0]) or bool(torch.isnan(out[0]))
    v.backward()
    return out, counts, x.grad


@pytest.mark.parametrize("hw", [(37, 52), (19, 21), (128, 132)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_index_and_dense_forms_are_bit_identical(layout, hw):
    """The label map through `regions=` (uint8 and int64) and the dense bool / uint8 / float target `expand_regions` makes of it:
    torch.equal values, counts and gradients.  A label outside the table sets the sticky verdict (and NaN results); nothing else
    does."""
    import mia_hip
    from losses.regions import expand_regions
    from mia_hip import ops
    dev = _dev()
    g = torch.Generator().manual_seed(hw[0])
    for regions, ign, n_lab in ((((1, 2), (1,)), None, 3), (((1, 2, 3), (2, 3), (3,)), 255, 4)):
        c = len(regions)
        x = _store(torch.randn(3, c, *hw, generator=g) * 2, layout, dev)
        lab = torch.randint(0, n_lab, (3, 1, *hw), generator=g).to(torch.uint8)
        if ign is not None:
            lab[torch.rand(3, 1, *hw, generator=g) < 0.2] = ign
            lab[1] = ign  # one image fully ignored
        lab = lab.to(dev)
        kw = dict(pos_weight=[0.5, 2.0, 3.0][:c], smooth=1e-5, do_bg=False, batch_dice=False, ce_w=0.7, dice_w=1.3)
        dense_fn = _loss(dev, c, ignore=ign is not None, **kw)
        dense = expand_regions(lab, regions, ign)
        assert dense.dtype == torch.bool and dense.shape == (3, c + (ign is not None), *hw)
        want = _run(dense_fn, x, dense)
        ops.check_labels()
        assert torch.isfinite(want[0]).all() and want[2].abs().max() > 0
        for t in (dense.to(torch.uint8), dense.float()):
            got = _run(dense_fn, x, t)
            assert all(torch.equal(a, b) for a, b in zip(got, want))
        index_fn = _loss(dev, c, ignore=ign is not None, regions=regions, ignore_label=ign, **kw)
        for labels in (lab, lab.long(), lab[:, 0].long()):
            got = _run(index_fn, x, labels)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (regions, labels.dtype)
            assert got[2].stride() == x.stride()
            ops.check_labels()  # nothing flagged: 255 is the ignore label where it occurs
        if ign is not None:
            assert not want[2][1].any()  # the fully ignored image gets exact zeros
        for labels in (lab, lab.long()):
            bad = labels.clone()
            bad[0, 0, 3, 5] = n_lab + 3  # neither a label of the table nor the ignore label
            out, _, grad = _run(index_fn, x, bad)
            assert torch.isnan(out).all() and torch.isnan(grad[0]).any()
            with pytest.raises(mia_hip.MiaError):
                ops.check_labels()
            ops.check_labels()  # read and cleared


def test_repeatable_and_byproducts():
    from mia_hip import ops
    dev = _dev()
    logits, mask, soft, ign = _grid_inputs(3, 3, (128, 132), 7)
    x = _store(logits, "nhwc", dev)
    t = torch.cat((mask, ign), 1).to(dev)
    kw = dict(pos_weight=[0.5, 2.0, 3.0], smooth=1.0, do_bg=True, batch_dice=False)
    fn = _loss(dev, 3, ignore=True, ce_w=0.7, dice_w=1.3, **kw)
    a, b = _run(fn, x, t), _run(fn, x, t)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    out, counts, grad = a
    assert torch.equal(fn.last_ce, out[1]) and torch.equal(fn.last_dc, out[2]) and torch.equal(fn.last_hard_counts, counts)
    assert fn.last_ce.dim() == 0 and counts.shape == (3, 3, 3)
    assert abs(out[0].item() - (0.7 * out[1].item() + 1.3 * out[2].item())) < 1e-6
    # the counts are the region Dice of the thresholded prediction
    hp, ht, valid = (x.detach() > 0), t[:, :3], ~t[:, 3:]
    assert torch.equal(counts[..., 0], (hp & ht & valid).sum((2, 3)))
    assert torch.equal(counts[..., 1], (hp & ~ht & valid).sum((2, 3)))
    assert torch.equal(counts[..., 2], (~hp & ht & valid).sum((2, 3)))
    # a weight of 0 drops that term: the value is the other term alone and the gradients of the two halves add up
    only_dc = _run(_loss(dev, 3, ignore=True, ce_w=0, dice_w=1, **kw), x, t)
    only_ce = _run(_loss(dev, 3, ignore=True, ce_w=1, dice_w=0, **kw), x, t)
    assert torch.equal(only_dc[0][0], only_dc[0][2]) and torch.equal(only_dc[0][2], out[2])
    assert torch.equal(only_ce[0][0], only_ce[0][1]) and torch.equal(only_ce[0][1], out[1])
    assert (0.7 * only_ce[2] + 1.3 * only_dc[2] - grad).abs().max().item() < 1e-9
    # inside a no_grad block the forward alone runs
    with torch.no_grad():
        assert torch.equal(fn(x, t), out[0])
    assert ops.RegionLossFn.last_out is not None


@pytest.mark.parametrize("hw", [(37, 52), (19, 21)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sigmoid_dice_with_loss_mask_is_the_compound_loss_dice_term(hw):
    """MemoryEfficientSoftDiceLoss(torch.sigmoid)(x, y, loss_mask) == the Dice term of DC_and_BCE_loss(weight_ce=0) whose ignore
    channel is the complement of the mask: value and gradient bit for bit; and it matches the restatement."""
    from losses.dice_loss import MemoryEfficientSoftDiceLoss
    dev = _dev()
    for c, do_bg, batch in ((3, True, False), (3, False, True), (1, True, False)):
        logits, mask, soft, ign = _grid_inputs(2, c, hw, 11 + c)
        for y in (mask, mask.to(torch.uint8), soft):
            x1, x2 = _store(logits, "nchw", dev), _store(logits, "nchw", dev)
            v1 = MemoryEfficientSoftDiceLoss(torch.sigmoid, batch_dice=batch, do_bg=do_bg, smooth=1e-5)(x1, y.to(dev), loss_mask=(~ign).to(dev))
            fn = _loss(dev, c, smooth=1e-5, do_bg=do_bg, batch_dice=batch, ce_w=0, dice_w=1, ignore=True)
            v2 = fn(x2, torch.cat((y, ign.to(y.dtype)), 1).to(dev))
            v1.backward()
            v2.backward()
            assert torch.equal(v1.detach(), fn.last_dc) and torch.equal(v1.detach(), v2.detach()) and torch.equal(x1.grad, x2.grad)
            want = R.region_loss_dense(logits.numpy(), torch.cat((y, ign.to(y.dtype)), 1).numpy(), True, smooth=1e-5, do_bg=do_bg,
                                       batch_dice=batch, ce_w=0.0)
            _check(f"dice c{c} {y.dtype}", v1.item(), x1.grad.cpu().numpy(), want["dc"], want["grad"], GRID_REL)
        # without a mask: the plain sigmoid Dice
        x = _store(logits, "nhwc", dev)
        v = MemoryEfficientSoftDiceLoss(torch.sigmoid, batch_dice=batch, do_bg=do_bg, smooth=1.0)(x, mask.to(dev))
        v.backward()
        want = R.region_loss_dense(logits.numpy(), mask.numpy(), False, smooth=1.0, do_bg=do_bg, batch_dice=batch, ce_w=0.0)
        _check(f"dice c{c} no mask", v.item(), x.grad.cpu().numpy(), want["dc"], want["grad"], GRID_REL)


def test_dc_and_topk_loss_is_the_composition_of_the_two_kernels():
    """weight_ce * TopKLoss + weight_dice * MemoryEfficientSoftDiceLoss(softmax) from the existing classes on the same inputs,
    exactly -- it is that composition."""
    from losses.ce_loss import TopKLoss
    from losses.compound_losses import DC_and_topk_loss, softmax_helper_dim1
    from losses.dice_loss import MemoryEfficientSoftDiceLoss
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(2, 3, 37, 52, generator=g) * 2
    lab = torch.randint(0, 3, (2, 1, 37, 52), generator=g)
    lab_ign = torch.where(torch.rand(2, 1, 37, 52, generator=g) < 0.2, 255, lab)
    cw = torch.tensor([0.2, 1.0, 3.0], device=dev)
    for y, ign, w_ce, w_dc in ((lab, None, 1, 1), (lab_ign, 255, 0.3, 1.7), (lab_ign.to(torch.uint8), 255, 2.0, 0.5)):
        y = y.to(dev)
        dice_kw = dict(batch_dice=True, do_bg=False, smooth=1e-5)
        fn = DC_and_topk_loss(dict(dice_kw), {"k": 25, "weight": cw}, weight_ce=w_ce, weight_dice=w_dc, ignore_label=ign)
        x1, x2 = _store(logits, "nhwc", dev), _store(logits, "nhwc", dev)
        v1 = fn(x1, y)
        v1.backward()
        topk = TopKLoss(weight=cw, k=25, **({} if ign is None else {"ignore_index": ign}))
        dice = MemoryEfficientSoftDiceLoss(softmax_helper_dim1, **dice_kw)
        mask = None if ign is None else y != ign
        y_dice = y if ign is None else torch.where(mask, y, 0)
        v2 = w_ce * topk(x2, y) + w_dc * dice(x2, y_dice, loss_mask=mask)
        v2.backward()
        assert torch.isfinite(v1) and torch.equal(v1.detach(), v2.detach()) and torch.equal(x1.grad, x2.grad)
    # a weight of 0 drops the term, as in the reference
    x = _store(logits, "nchw", dev)
    only = DC_and_topk_loss({}, {"k": 10}, weight_ce=1, weight_dice=0)(x, lab.to(dev))
    assert torch.equal(only.detach(), TopKLoss(k=10)(x, lab.to(dev)).detach())
