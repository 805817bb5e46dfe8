"""Host side of the batched BADGE embeddings (CPU): the closed form the HIP kernel implements against autograd through the
oracle's restatement of the reference losses (fp64), the pure-Python eligibility test of `BADGESelector`'s fused path, the
precedence of `embed_batch_size` over `MIA_BADGE_BATCH`, and the argument errors of the C entry point."""
import ctypes
import itertools

import pytest
import torch

import _badge_ref as R
import mia_hip
from oracle import losses_ref

SMOOTH = 1e-5


def _case(k1, c0, h, w, seed, single_class=False):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(1, h, w, c0, generator=g, dtype=torch.float64)
    weight = torch.randn(k1, c0, generator=g, dtype=torch.float64)
    bias = torch.randn(k1, generator=g, dtype=torch.float64)
    if single_class:
        weight = weight * 1e-2
        bias[k1 - 1] += 5.0  # the last class wins every pixel
    return feat, weight, bias


def _close(got, want, what):
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= 1e-10 * scale, (what, float((got - want).abs().max()), scale)


GRID = [(k1, c0, hw, do_bg, False) for k1, c0, hw, do_bg in
        itertools.product((2, 3, 5), (4, 7), ((1, 1), (6, 5), (9, 7)), (True, False))] + \
       [(3, 4, (6, 5), True, True), (3, 7, (9, 7), False, True)]


@pytest.mark.parametrize("k1,c0,hw,do_bg,single", GRID)
def test_closed_form_equals_autograd_through_the_reference_losses(k1, c0, hw, do_bg, single):
    feat, weight, bias = _case(k1, c0, hw[0], hw[1], seed=100 * k1 + 10 * c0 + hw[0], single_class=single)
    logits = torch.nn.functional.conv2d(feat.permute(0, 3, 1, 2), weight.reshape(k1, c0, 1, 1), bias)
    if single:
        assert (logits.argmax(1) == k1 - 1).all()
    want, want_loss = R.embed_autograd(
        feat, weight, bias, SMOOTH, do_bg, False, ce=losses_ref.ce_loss,
        dice=lambda o, t: losses_ref.dice_loss(o, t, k1 - 1, smooth=SMOOTH, do_bg=do_bg, softmax=True, batch=False))
    got, got_loss, unit = R.embed_closed_form(logits, feat, SMOOTH, do_bg, False)
    _close(got, want, "embed")
    _close(got_loss, want_loss, "loss")
    assert (got.abs() <= unit * (1 + 1e-12)).all()
    # `batch` makes no difference at one image per loss
    want_b, _ = R.embed_autograd(
        feat, weight, bias, SMOOTH, do_bg, False, ce=losses_ref.ce_loss,
        dice=lambda o, t: losses_ref.dice_loss(o, t, k1 - 1, smooth=SMOOTH, do_bg=do_bg, softmax=True, batch=True))
    _close(want_b, want, "batch")


@pytest.mark.parametrize("k1,c0,hw,do_bg", [(2, 4, (1, 1), True), (3, 7, (6, 5), False), (5, 4, (9, 7), True), (3, 4, (9, 7), False)])
def test_closed_form_squared_equals_autograd_through_the_restated_reference_formula(k1, c0, hw, do_bg):
    feat, weight, bias = _case(k1, c0, hw[0], hw[1], seed=7 * k1 + c0)
    logits = torch.nn.functional.conv2d(feat.permute(0, 3, 1, 2), weight.reshape(k1, c0, 1, 1), bias)
    want, want_loss = R.embed_autograd(feat, weight, bias, SMOOTH, do_bg, True)
    got, got_loss, _ = R.embed_closed_form(logits, feat, SMOOTH, do_bg, True)
    _close(got, want, "embed")
    _close(got_loss, want_loss, "loss")
    # the restatement itself against the oracle's
    pred = logits.argmax(1)
    for sq in (False, True):
        a = R.dice_loss_restated(logits, pred, k1, SMOOTH, do_bg, sq)
        b = losses_ref.dice_loss(logits, pred, k1 - 1, smooth=SMOOTH, do_bg=do_bg, squared=sq)
        assert abs(float(a) - float(b)) <= 1e-12


def test_closed_form_handles_a_batch_image_by_image():
    g = torch.Generator().manual_seed(3)
    feat = torch.randn(3, 6, 5, 4, generator=g, dtype=torch.float64)
    weight = torch.randn(3, 4, generator=g, dtype=torch.float64)
    bias = torch.zeros(3, dtype=torch.float64)
    logits = torch.nn.functional.conv2d(feat.permute(0, 3, 1, 2), weight.reshape(3, 4, 1, 1), bias)
    want, _ = R.embed_autograd(feat, weight, bias, SMOOTH, True, False)
    got, _, _ = R.embed_closed_form(logits, feat, SMOOTH, True, False)
    _close(got, want, "batch of 3")


# ------------------------------------------------------------------ eligibility and precedence
def _al_train_parts():
    from losses.compound_losses import DiceAndCELoss
    from models.unet import UNet
    loss = DiceAndCELoss(dice_kwargs=dict(num_classes=2, do_bg=True), ce_loss=torch.nn.CrossEntropyLoss)
    model = UNet(2, 1, 3, [8, 16, 32], normalization="instance", dropout_prob=None)
    return loss, model


def _selector(dice, ce, **kw):
    from activelearning import BADGESelector
    return BADGESelector(dice_loss=dice, ce_loss=ce, batch_size=1, num_workers=0, pin_memory=False, **kw)


def test_al_train_construction_is_eligible_and_each_deviation_is_not(monkeypatch):
    from activelearning.selectors import badge_closed_form_reason
    from losses.dice_loss import DiceLoss
    monkeypatch.delenv("MIA_BADGE_BATCH", raising=False)
    loss, model = _al_train_parts()
    assert badge_closed_form_reason(loss.dice_loss, loss.ce_loss, "add", model) is None
    sel = _selector(loss.dice_loss, loss.ce_loss, embed_batch_size=8)
    assert sel.embed_path(model) == "fused" and sel.embed_path_reason is None
    # DiceLoss.batch may be either value
    assert _selector(DiceLoss(2, do_bg=True, batch=True), loss.ce_loss, embed_batch_size=8).embed_path(model) == "fused"
    assert _selector(DiceLoss(2, do_bg=False, squared=True), loss.ce_loss, embed_batch_size=8).embed_path(model) == "fused"

    class NoPixelFeature(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.encoder, self.decoder = inner.encoder, inner.decoder

    deviations = {
        "weighted CE": dict(ce=torch.nn.CrossEntropyLoss(weight=torch.ones(3))),
        "label smoothing": dict(ce=torch.nn.CrossEntropyLoss(label_smoothing=0.1)),
        "sum reduction": dict(ce=torch.nn.CrossEntropyLoss(reduction="sum")),
        "softmax=False": dict(dice=DiceLoss(2, do_bg=True, softmax=False)),
        "sep": dict(multiple_loss="sep"),
        "no get_pixel_feature": dict(model=NoPixelFeature(model)),
        "class count": dict(dice=DiceLoss(3, do_bg=True)),
    }
    for what, d in deviations.items():
        dice, ce, m = d.get("dice", loss.dice_loss), d.get("ce", loss.ce_loss), d.get("model", model)
        ml = d.get("multiple_loss", "add")
        assert isinstance(badge_closed_form_reason(dice, ce, ml, m), str), what
        sel = _selector(dice, ce, multiple_loss=ml, embed_batch_size=8)
        assert sel.embed_path(m) == "autograd" and sel.embed_path_reason, what
    # a head outside the kernel's range: 6 channels
    from models.unet import UNet
    odd = UNet(2, 1, 3, [6, 12], normalization="instance", dropout_prob=None)
    assert "range" in badge_closed_form_reason(loss.dice_loss, loss.ce_loss, "add", odd)


def test_explicit_batch_size_beats_the_environment_and_both_unset_means_off(monkeypatch):
    loss, model = _al_train_parts()
    monkeypatch.delenv("MIA_BADGE_BATCH", raising=False)
    sel = _selector(loss.dice_loss, loss.ce_loss)
    assert sel.resolved_embed_batch_size() is None and sel.embed_path(model) == "autograd"
    monkeypatch.setenv("MIA_BADGE_BATCH", "4")
    assert sel.resolved_embed_batch_size() == 4 and sel.embed_path(model) == "fused"
    assert _selector(loss.dice_loss, loss.ce_loss, embed_batch_size=16).resolved_embed_batch_size() == 16
    off = _selector(loss.dice_loss, loss.ce_loss, embed_batch_size=0)  # an explicit 0 switches it off whatever the environment says
    assert off.resolved_embed_batch_size() is None and off.embed_path(model) == "autograd"
    monkeypatch.setenv("MIA_BADGE_BATCH", "")
    assert sel.resolved_embed_batch_size() is None


# ------------------------------------------------------------------ C entry point without a GPU
def _embed_rc(k1=3, c0=8, logits=4096, feat=4096, dtype=mia_hip.F32, hw=16, do_bg=1, sk=1, ws=4096):
    l = mia_hip.lib()
    v = ctypes.c_void_p
    rc = l.mia_badge_embed(v(logits), v(feat), dtype, 2, hw, k1, c0, hw * k1, sk, k1, ctypes.c_float(1e-5), do_bg, 0, v(ws), v(4096),
                           v(4096), None)
    return rc, l.mia_last_error()


def test_argument_errors_are_reported_without_a_gpu():
    rc, msg = _embed_rc(k1=9)
    assert rc < 0 and b"k1=9" in msg
    rc, msg = _embed_rc(c0=6)
    assert rc < 0 and b"c0=6" in msg
    rc, msg = _embed_rc(feat=None)
    assert rc < 0 and b"null pointer" in msg
    rc, msg = _embed_rc(logits=None)
    assert rc < 0 and b"null pointer" in msg
    rc, msg = _embed_rc(dtype=7)
    assert rc < 0 and b"dtype" in msg
    rc, msg = _embed_rc(k1=1, do_bg=0)
    assert rc < 0 and b"do_bg" in msg
    rc, msg = _embed_rc(sk=0)
    assert rc < 0 and b"strides" in msg
    rc, msg = _embed_rc(feat=4100)
    assert rc < 0 and b"misaligned" in msg
    with pytest.raises(mia_hip.MiaError):
        from activelearning.scores import badge_embeddings
        badge_embeddings(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, 8))  # CPU tensors: no fallback


def test_slab_rule_depends_on_the_image_size_alone():
    l = mia_hip.lib()
    from activelearning.scores import badge_slabs

    def query(nb, hw, k1, c0, dt):
        s = ctypes.c_int(-1)
        return l.mia_badge_embed_workspace(nb, hw, k1, c0, dt, ctypes.byref(s)), s.value

    for hw, want in ((1, 1), (4096, 1), (4097, 2), (97 * 97, 3), (512 * 512, 64), (1024 * 1024, 256), (2048 * 2048, 256)):
        for nb, k1, c0, dt in ((1, 3, 64, mia_hip.BF16), (32, 3, 64, mia_hip.BF16), (5, 8, 128, mia_hip.F32), (2, 2, 4, mia_hip.F32)):
            words, slabs = query(nb, hw, k1, c0, dt)
            assert slabs == want, (hw, nb, k1, c0, dt)
            assert words == nb * (slabs * (3 * k1 + 1) + 2 * k1 + slabs * k1 * c0)
    assert badge_slabs(97 * 97, 3, 64, torch.bfloat16) == 3
    for bad in ((1, 16, 9, 8, 0), (1, 16, 3, 6, 0), (1, 16, 3, 132, 0), (0, 16, 3, 8, 0), (1, 0, 3, 8, 0), (1, 16, 3, 8, 5)):
        assert query(*bad) == (0, 0)
    assert l.mia_badge_embed_workspace(1, 16, 3, 8, 0, None) > 0  # the slab count is optional
