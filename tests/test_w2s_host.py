"""Host-side tests of weak-to-strong consistency (no GPU): the float64 restatement against torch's autograd on the tensor-op form,
hand-made identities, the CutMix box generator, the argument checks of the new entry points, and the ambiguity cap of the inputs that
tests/test_gpu_w2s.py feeds the kernels -- checked here on the reference alone, so the GPU comparison cannot hide behind it."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _w2s_ref as R
import mia_hip
from losses.weak_strong import (WeakToStrongLoss, box_masks, pseudo_label_code, random_cutmix_boxes,
                                weak_to_strong_tensor_ops)
from mia_hip import ops


def _t(a, **kw):
    return None if a is None else torch.tensor(a, **kw)


# ---------------------------------------------------------------- the restatement against autograd on the tensor-op form
@pytest.mark.parametrize("perm_kind", ["none", "identity", "reverse", "fixed"])
@pytest.mark.parametrize("mask_kind", ["none", "hw", "bhw"])
@pytest.mark.parametrize("k1", [2, 3, 8])
def test_restatement_equals_tensor_op_form_under_autograd(k1, mask_kind, perm_kind):
    nb, h, w = 4, 9, 11
    zw, zs = R.make_case(nb, k1, h, w, absent=k1 == 3)
    mask, perm = R.make_mask(nb, h, w, mask_kind), R.make_perm(nb, perm_kind)
    for tau, weight, cw, dw in ((0.0, 1.0, 1.0, 0.0), (0.6, 0.3, 1.0, 0.5), (0.6, 2.0, 0.0, 1.0)):
        code = R.code_of(zw, tau)
        ref = R.evaluate(zs, code, mask, perm, weight, cw, dw)
        assert np.array_equal(pseudo_label_code(torch.tensor(zw, dtype=torch.float64), tau).numpy(), code)
        t = torch.tensor(zs, dtype=torch.float64, requires_grad=True)
        loss, terms, counts = weak_to_strong_tensor_ops(t, _t(code), _t(mask), _t(perm), weight, cw, dw)
        loss.backward()
        assert tuple(int(c) for c in counts) == ref["counts"] and 0 < ref["counts"][0] <= nb * h * w
        assert abs(loss.item() - ref["value"]) <= 1e-12 * max(abs(ref["value"]), 1e-30)
        assert abs(terms[0].item() - ref["ce"]) <= 1e-12 * ref["ce_mag"] and abs(terms[1].item() - ref["dice"]) <= 1e-12
        g = t.grad.numpy()
        assert np.abs(g - ref["grad"]).max() <= 1e-12 * max(np.abs(g).max(), 1e-30)
        assert (np.abs(ref["grad"]) <= ref["grad_mag"] * (1 + 1e-12)).all()
        if mask is not None and perm is not None:
            assert ref["counts"][1] == int(np.broadcast_to(mask != 0, (nb, h, w)).sum()) > 0


def test_restatement_gradient_against_central_differences():
    nb, k1, h, w = 3, 3, 2, 3
    zw, zs = R.make_case(nb, k1, h, w)
    mask, perm, code = R.make_mask(nb, h, w, "bhw"), R.make_perm(nb, "reverse"), R.code_of(zw, 0.5)
    ref = R.evaluate(zs, code, mask, perm, 0.7, 1.0, 0.5)
    z = zs.astype(np.float64)
    eps = 1e-6
    for idx in np.ndindex(z.shape):
        zp, zm = z.copy(), z.copy()
        zp[idx] += eps
        zm[idx] -= eps
        num = (R.evaluate(zp, code, mask, perm, 0.7, 1.0, 0.5)["value"] - R.evaluate(zm, code, mask, perm, 0.7, 1.0, 0.5)["value"]) / (2 * eps)
        assert abs(num - ref["grad"][idx]) <= 1e-8


# ---------------------------------------------------------------- hand-made checks
@pytest.mark.parametrize("how", ["no_mix", "identity", "zero_mask"])
def test_no_mix_at_tau_zero_is_cross_entropy_on_the_weak_argmax(how):
    nb, k1, h, w = 3, 4, 5, 6
    zw, zs = R.make_case(nb, k1, h, w)
    code = R.code_of(zw, 0.0)
    mask = {"no_mix": None, "identity": R.make_mask(nb, h, w, "bhw"), "zero_mask": np.zeros((h, w), np.uint8)}[how]
    perm = {"no_mix": None, "identity": np.arange(nb), "zero_mask": R.make_perm(nb, "reverse")}[how]
    want = F.cross_entropy(torch.tensor(zs, dtype=torch.float64), torch.tensor(zw).argmax(1)).item()
    ref = R.evaluate(zs, code, mask, perm, 1.0, 1.0, 0.0)
    assert abs(ref["value"] - want) <= 1e-13 * want and ref["counts"][0] == nb * h * w
    loss, _, _ = weak_to_strong_tensor_ops(torch.tensor(zs, dtype=torch.float64), _t(code), _t(mask), _t(perm))
    assert abs(loss.item() - want) <= 1e-13 * want


def test_full_mask_with_reverse_perm_is_the_weak_batch_reversed():
    nb, k1, h, w = 4, 3, 5, 6
    zw, zs = R.make_case(nb, k1, h, w)
    code = R.code_of(zw, 0.6)
    full = np.ones((h, w), np.uint8)
    a = R.evaluate(zs, code, full, R.make_perm(nb, "reverse"), 1.0, 1.0, 0.5)
    b = R.evaluate(zs, R.code_of(zw[::-1], 0.6), None, None, 1.0, 1.0, 0.5)
    assert a["value"] == b["value"] and np.array_equal(a["grad"], b["grad"]) and a["counts"][0] == b["counts"][0]
    assert a["counts"][1] == nb * h * w and b["counts"][1] == 0
    t = torch.tensor(zs, dtype=torch.float64)
    la = weak_to_strong_tensor_ops(t, _t(code), _t(full), [3, 2, 1, 0], 1.0, 1.0, 0.5)[0]
    lb = weak_to_strong_tensor_ops(t, _t(np.ascontiguousarray(code[::-1])), None, None, 1.0, 1.0, 0.5)[0]
    assert la.item() == lb.item()


def test_threshold_above_one_gives_zero_and_a_zero_gradient():
    nb, k1, h, w = 2, 3, 4, 5
    zw, zs = R.make_case(nb, k1, h, w)
    code = R.code_of(zw, 1.5)
    assert not R.decode(code)[1].any()
    ref = R.evaluate(zs, code, R.make_mask(nb, h, w, "hw"), R.make_perm(nb, "reverse"), 1.0, 1.0, 1.0)
    assert ref["value"] == 0.0 and ref["dice"] == 0.0 and not ref["grad"].any() and ref["counts"][0] == 0
    t = torch.tensor(zs, dtype=torch.float64, requires_grad=True)
    loss, terms, counts = weak_to_strong_tensor_ops(t, _t(code), None, None, 1.0, 1.0, 1.0)
    loss.backward()
    assert loss.item() == 0.0 and not t.grad.numpy().any() and int(counts[0]) == 0


def test_ties_go_to_the_lowest_class_and_the_mix_is_a_selection():
    zw = np.zeros((1, 3, 1, 2), np.float32)
    zw[0, :, 0, 1] = [1.0, 2.0, 2.0]
    assert R.labels(zw).tolist() == [[[0, 1]]]
    assert (pseudo_label_code(torch.tensor(zw), 0.0).numpy() & 7).tolist() == [[[0, 1]]]
    x = np.arange(2 * 1 * 2 * 2, dtype=np.float32).reshape(2, 1, 2, 2)
    m = np.array([[1, 0], [0, 7]], np.uint8)
    assert R.mix(x, [1, 0], m)[0, 0].tolist() == [[4.0, 1.0], [2.0, 7.0]]


# ---------------------------------------------------------------- the box generator
def test_cutmix_boxes_are_reproducible_and_stay_in_range():
    nb, h, w = 64, 48, 80
    size, ratio = (0.02, 0.4), (0.3, 1 / 0.3)
    torch.manual_seed(11)
    a = random_cutmix_boxes(nb, h, w, p=0.7)
    torch.manual_seed(11)
    b = random_cutmix_boxes(nb, h, w, p=0.7)
    g = torch.Generator().manual_seed(5)
    c = random_cutmix_boxes(nb, h, w, p=0.7, generator=g)
    assert torch.equal(a, b) and not torch.equal(a, c) and a.dtype == torch.int64 and tuple(a.shape) == (nb, 4)
    fired = 0
    for y0, x0, y1, x1 in a.tolist():
        if (y0, x0, y1, x1) == (0, 0, 0, 0):
            continue
        fired += 1
        bh, bw = y1 - y0, x1 - x0
        assert 0 <= y0 < y1 <= h and 0 <= x0 < x1 <= w  # inside the image
        # the drawn height and width are real numbers in [bh, bh + 1) x [bw, bw + 1): area and aspect with that rounding
        assert bh * bw <= size[1] * h * w and (bh + 1) * (bw + 1) > size[0] * h * w
        assert bh / (bw + 1) < ratio[1] and (bh + 1) / bw > ratio[0]
    assert 0.45 * nb < fired < 0.95 * nb  # p = 0.7 of 64 draws
    assert not random_cutmix_boxes(nb, h, w, p=0.0).any()
    assert (random_cutmix_boxes(nb, h, w, p=1.0)[:, 2] > 0).all()
    # p does not change the draws: what fires at p = 0.7 has the same box at p = 1
    torch.manual_seed(11)
    full = random_cutmix_boxes(nb, h, w, p=1.0)
    assert all(torch.equal(a[n], full[n]) for n in range(nb) if a[n].any())
    m = box_masks(a, h, w, device="cpu")
    assert m.dtype == torch.uint8 and tuple(m.shape) == (nb, h, w)
    for n, (y0, x0, y1, x1) in enumerate(a.tolist()):
        want = torch.zeros(h, w, dtype=torch.uint8)
        want[y0:y1, x0:x1] = 1
        assert torch.equal(m[n], want)


def test_cutmix_boxes_fit_extreme_images_and_reject_bad_arguments():
    for h, w in ((1, 1), (1, 40), (40, 1), (3, 200)):
        b = random_cutmix_boxes(32, h, w, p=1.0)
        assert ((b[:, 0] >= 0) & (b[:, 2] <= h) & (b[:, 1] >= 0) & (b[:, 3] <= w) & (b[:, 0] <= b[:, 2]) & (b[:, 1] <= b[:, 3])).all()
    for kw in (dict(p=1.5), dict(size=(0.0, 0.4)), dict(size=(0.5, 0.4)), dict(ratio=(0.0, 1.0)), dict(ratio=(2.0, 1.0))):
        with pytest.raises(ValueError):
            random_cutmix_boxes(2, 8, 8, **kw)


# ---------------------------------------------------------------- constructor and argument errors
def test_constants_constructor_and_argument_errors():
    assert ops.W2S_MAX_CLASSES == 8 == mia_hip.parse_defines()["MIA_W2S_MAX_CLASSES"]
    assert WeakToStrongLoss(7).num_classes == 8
    with pytest.raises(mia_hip.MiaError):
        WeakToStrongLoss(8)
    assert WeakToStrongLoss(8, fused=False).num_classes == 9
    with pytest.raises(ValueError):
        WeakToStrongLoss(2, ce_weight=-1.0)
    z, code = torch.zeros(2, 3, 4, 4), torch.zeros(2, 4, 4, dtype=torch.uint8)
    with pytest.raises(mia_hip.MiaError):  # no CPU fallback of the fused form
        WeakToStrongLoss(2)(z, code)
    with pytest.raises(mia_hip.MiaError):
        ops.w2s_labels(z)
    with pytest.raises(mia_hip.MiaError):
        ops.cutmix_perm(z, [1, 0], torch.ones(4, 4, dtype=torch.uint8))
    soft = WeakToStrongLoss(2, fused=False)
    assert soft(z, code).item() == 0.0 and int(soft.last_kept) == 0  # no confidence bit set
    with pytest.raises(AssertionError):
        soft(torch.zeros(2, 4, 4, 4), code)
    with pytest.raises(NotImplementedError):
        soft(torch.zeros(2, 3, 4, 4, 4), code)
    with pytest.raises(mia_hip.MiaError):
        soft(z, code.long())
    with pytest.raises(mia_hip.MiaError):
        soft(z, code, torch.ones(4, 4, dtype=torch.uint8), [0, 2])  # an entry outside the batch
    with pytest.raises(mia_hip.MiaError):
        soft(z, code, torch.ones(4, 4, dtype=torch.uint8), [0.0, 1.0])
    with pytest.raises(mia_hip.MiaError):
        soft(z, code, torch.ones(4, 4), [1, 0])  # a float mask
    with pytest.raises(ValueError):
        pseudo_label_code(torch.zeros(2, 3, 4))


def test_abi_argument_checks_happen_before_any_launch():
    l = mia_hip.lib()
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    p = lambda off=0: ctypes.c_void_p(base + off)
    i64 = ctypes.c_int64
    f = ctypes.c_float
    assert l.mia_w2s_loss_workspace(2, 3, 4) == 2 * 4 * (2 * 7 + 5) and l.mia_w2s_loss_workspace(2, 9, 4) < 0
    assert l.mia_w2s_loss_workspace(0, 3, 4) < 0
    assert l.mia_w2s_labels(p(), None, 2, i64(16), 9, i64(48), i64(16), i64(1), 1, p(), p(), p(), None) < 0
    assert b"k1=9" in l.mia_last_error()
    assert l.mia_w2s_labels(p(), None, 2, i64(16), 3, i64(48), i64(16), i64(1), 1, None, p(), p(), None) < 0
    assert l.mia_w2s_labels(p(), None, 1 << 20, i64(1 << 20), 3, i64(48), i64(16), i64(1), 1, p(), p(), p(), None) < 0  # nb * hw >= 2^31
    # out overlaps x: [0, 2 * 32) floats against out at float 40 is fine by address, at float 60 of x [0, 2 * 32) it is not
    assert l.mia_cutmix_perm(p(), p(), p(), p(4 * 60), 2, 2, i64(16), i64(16), i64(32), p(), None) < 0
    assert b"overlaps" in l.mia_last_error()
    assert l.mia_cutmix_perm(p(4 * 8), p(), p(), p(), 2, 2, i64(16), i64(16), i64(32), p(), None) < 0  # x starts inside out
    assert l.mia_cutmix_perm(p(), p(), p(), p(4 * 64), 2, 2, i64(16), i64(8), i64(32), p(), None) < 0  # mask stride
    assert l.mia_cutmix_perm(p(), p(), p(), p(4 * 64), 2, 2, i64(16), i64(16), i64(31), p(), None) < 0  # out stride below c * hw
    assert l.mia_cutmix_perm(p(), None, p(), p(4 * 64), 2, 2, i64(16), i64(16), i64(32), p(), None) < 0
    args = (2, i64(16), 3, i64(48), i64(16), i64(1))
    assert l.mia_w2s_loss_fwd(p(), p(), None, None, None, *args, i64(5), f(1e-10), f(1), f(0), 1, p(), p(), p(), p(), p(), None) < 0
    assert b"strides" in l.mia_last_error()
    assert l.mia_w2s_loss_fwd(p(), None, None, None, None, *args, i64(0), f(1e-10), f(1), f(0), 1, p(), p(), p(), p(), p(), None) < 0
    assert l.mia_w2s_loss_bwd(p(), p(), None, None, p(), None, p(), 2, i64(16), 0, i64(48), i64(16), i64(1), i64(48), i64(16), i64(1),
                              i64(0), None) < 0


# ---------------------------------------------------------------- the ambiguity cap of the GPU file's inputs
def test_the_gpu_cases_keep_few_pixels_on_the_threshold():
    """For every case and threshold tests/test_gpu_w2s.py uses, the share of pixels with |max softmax - tau| < 1e-6 in float64 is at
    most 5e-4 (the cap of tests/test_gpu_cps.py)."""
    shapes = R.SHAPES + [(4, 36, 60), (4, 8, 12)]  # the grid, the path test, the perm-guard test
    cases = [R.make_case(nb, k1, h, w, absent=absent)[0] for nb, h, w in shapes for k1 in R.K1S for absent in (False, True)]
    cases += [R.tie_case(4, k1, 37, 61)[0] for k1 in R.K1S] + [R.tie_case(2, k1, 336, 544)[0] for k1 in R.K1S]
    cases += [R.saturated_case(nb, 3, h, w)[0] for nb, h, w in ((1, 3, 5), (2, 8, 16))]
    worst = 0.0
    for zw in cases:
        for tau in R.thresholds() + [0.0]:
            share = float(R.ambiguous(zw, tau).mean())
            worst = max(worst, share)
            assert share <= 5e-4, (zw.shape, tau, share)
    print(f"largest ambiguous share {worst:.2e}")
