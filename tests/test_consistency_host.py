"""Host-side tests of the mean-teacher work (no GPU): the float64 restatement against torch's autograd of the literal expressions,
the argument checks of the three new entry points, the no-CPU-fallback rule, the layout of MeanTeacherEngine's teacher buffer and
the two schedules."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _consistency_ref as R
import mia_hip


# ---------------------------------------------------------------- the restatement against the literal torch expressions
def _torch_plain(zs, zt):
    return torch.mean((torch.softmax(zs, 1) - torch.softmax(zt, 1)) ** 2)


def _torch_masked(zs, zt, pbar, thr):
    dist = ((torch.softmax(zs, 1) - torch.softmax(zt, 1)) ** 2).sum(1, keepdim=True)
    mask = (-(pbar * torch.log(pbar + 1e-6)).sum(1, keepdim=True) < thr).double()
    return torch.sum(mask * dist) / (2 * torch.sum(mask) + 1e-16), mask


@pytest.mark.parametrize("k1", [2, 3, 8])
def test_restatement_equals_torch_autograd(k1):
    zs, zt, pbar = R.make_case(2, k1, 9, 11)
    tz = torch.tensor(zs, dtype=torch.float64, requires_grad=True)
    tt, tp = torch.tensor(zt, dtype=torch.float64), torch.tensor(pbar, dtype=torch.float64)
    ref = R.evaluate(zs, zt)
    loss = _torch_plain(tz, tt)
    loss.backward()
    assert abs(loss.item() - ref["value"]) <= 1e-12
    assert np.abs(tz.grad.numpy() - ref["grad"]).max() <= 1e-12
    assert ref["n_keep"] == 2 * 9 * 11
    for thr in R.thresholds(k1) + [0.0]:  # 0: the all-dropped mask
        tz.grad = None
        loss, mask = _torch_masked(tz, tt, tp, thr)
        loss.backward()
        keep = R.keep_mask(pbar, thr)
        assert np.array_equal(keep, mask.numpy()[:, 0] > 0)
        ref = R.evaluate(zs, zt, keep)
        assert ref["n_keep"] == int(mask.sum().item())
        assert abs(loss.item() - ref["value"]) <= 1e-12
        assert np.abs(tz.grad.numpy() - ref["grad"]).max() <= 1e-12
        if thr == 0.0:
            assert ref["n_keep"] == 0 and ref["value"] == 0.0 and not ref["grad"].any() and np.isfinite(ref["grad"]).all()
        else:
            assert 0 < ref["n_keep"] < keep.size  # both branches


def test_bounds_dominate_the_terms_they_bound():
    zs, zt, pbar = R.make_case(2, 3, 9, 11)
    ref = R.evaluate(zs, zt, R.keep_mask(pbar, R.thresholds(3)[1]))
    assert ref["value"] <= ref["value_mag"]
    assert (np.abs(ref["grad"]) <= ref["grad_mag"]).all()


def test_ema_restatement_and_schedules():
    rng = np.random.default_rng(5)
    t, s = rng.standard_normal(100), rng.standard_normal(100)
    assert np.array_equal(R.ema(t, s, 0.0), s)
    assert np.array_equal(R.ema(t, s, 1.0), t)
    assert np.allclose(R.ema(t, s, 0.25), 0.25 * t + 0.75 * s, rtol=0, atol=1e-15)
    from training.semi import ema_alpha, entropy_threshold
    want = [0.0, 0.5, 2.0 / 3.0, 0.75]
    for i, a in enumerate(want):
        assert ema_alpha(i, 0.99) == pytest.approx(a, abs=1e-15) and R.ema_alpha(i, 0.99) == ema_alpha(i, 0.99)
    assert ema_alpha(98, 0.99) == pytest.approx(1.0 - 1.0 / 99.0, abs=1e-15)
    assert ema_alpha(99, 0.99) == 0.99 and ema_alpha(10 ** 6, 0.99) == 0.99
    assert ema_alpha(5, 0.0) == 0.0
    for k in (2, 3, 4):
        assert entropy_threshold(0.0, k) == pytest.approx(0.75 * math.log(k), abs=1e-15)
        assert entropy_threshold(1.0, k) == pytest.approx(math.log(k), abs=1e-15)
        assert entropy_threshold(0.5, k) == pytest.approx(0.875 * math.log(k), abs=1e-15)
        assert R.entropy_threshold(0.3, k) == entropy_threshold(0.3, k)


# ---------------------------------------------------------------- C ABI: argument errors without a device
def _ptr(v):
    return None if v is None else ctypes.c_void_p(16 * v)  # never dereferenced: the checks fail before any launch


def _fwd(**kw):
    a = dict(zs=1, zt=1, pbar=None, dyn=None, nb=1, hw=64, k1=3, den=2.0, slabs=1, ws=1, keep=None, coef=1, out=1, nk=1, st=(192, 64, 1))
    a.update(kw)
    i64 = ctypes.c_int64
    mia_hip.call("mia_consistency_fwd", _ptr(a["zs"]), _ptr(a["zt"]), _ptr(a["pbar"]), _ptr(a["dyn"]), a["nb"], i64(a["hw"]), a["k1"],
                 *(i64(s) for s in a["st"]), i64(192), i64(64), i64(1), ctypes.c_float(a["den"]), a["slabs"], _ptr(a["ws"]),
                 _ptr(a["keep"]), _ptr(a["coef"]), _ptr(a["out"]), _ptr(a["nk"]), None)


def _bwd(**kw):
    a = dict(zs=1, zt=1, keep=None, coef=1, dyn=None, gout=None, dl=1, nb=1, hw=64, k1=3, gst=(192, 64, 1))
    a.update(kw)
    i64 = ctypes.c_int64
    mia_hip.call("mia_consistency_bwd", _ptr(a["zs"]), _ptr(a["zt"]), _ptr(a["keep"]), _ptr(a["coef"]), _ptr(a["dyn"]), _ptr(a["gout"]),
                 _ptr(a["dl"]), a["nb"], i64(a["hw"]), a["k1"], i64(192), i64(64), i64(1), i64(192), i64(64), i64(1),
                 *(i64(s) for s in a["gst"]), None)


def _ema(**kw):
    a = dict(t=1, s=2, n=8, alpha=0.5, adev=None)
    a.update(kw)
    mia_hip.call("mia_ema_update", _ptr(a["t"]), _ptr(a["s"]), ctypes.c_int64(a["n"]), ctypes.c_float(a["alpha"]), _ptr(a["adev"]), None)


def test_consistency_argument_errors():
    for name in ("zs", "zt", "ws", "coef", "out", "nk"):
        with pytest.raises(mia_hip.MiaError, match="null pointer"):
            _fwd(**{name: None})
    for kw in (dict(nb=0), dict(hw=0), dict(slabs=0), dict(nb=1 << 16, hw=1 << 16)):
        with pytest.raises(mia_hip.MiaError, match="bad shape"):
            _fwd(**kw)
    with pytest.raises(mia_hip.MiaError, match="k1=0"):
        _fwd(k1=0)
    with pytest.raises(mia_hip.MiaError, match="k1=9"):
        _fwd(k1=9)
    with pytest.raises(mia_hip.MiaError, match="negative strides"):
        _fwd(st=(192, -64, 1))
    with pytest.raises(mia_hip.MiaError, match="prob_mean needs dyn_dev"):
        _fwd(pbar=1, keep=1)
    with pytest.raises(mia_hip.MiaError, match="keep map"):
        _fwd(pbar=1, dyn=1)
    for den in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(mia_hip.MiaError, match="den_scale"):
            _fwd(pbar=1, dyn=1, keep=1, den=den)
    for name in ("zs", "zt", "coef", "dl"):
        with pytest.raises(mia_hip.MiaError, match="null pointer"):
            _bwd(**{name: None})
    for kw in (dict(nb=0), dict(hw=0)):
        with pytest.raises(mia_hip.MiaError, match="bad shape"):
            _bwd(**kw)
    with pytest.raises(mia_hip.MiaError, match="k1=0"):
        _bwd(k1=0)
    with pytest.raises(mia_hip.MiaError, match="k1=9"):
        _bwd(k1=9)
    with pytest.raises(mia_hip.MiaError, match="negative strides"):
        _bwd(gst=(-1, 64, 1))
    lib = mia_hip.lib()
    assert lib.mia_consistency_workspace(3, 4) == 36
    assert lib.mia_consistency_workspace(0, 4) < 0 and lib.mia_consistency_workspace(3, 0) < 0
    assert lib.mia_consistency_workspace(1 << 20, 1 << 10) < 0


def test_ema_argument_errors():
    for name in ("t", "s"):
        with pytest.raises(mia_hip.MiaError, match="null pointer"):
            _ema(**{name: None})
    for n in (0, -4):
        with pytest.raises(mia_hip.MiaError, match="must be positive"):
            _ema(n=n)
    for alpha in (-0.1, 1.5, float("nan")):
        with pytest.raises(mia_hip.MiaError, match="alpha"):
            _ema(alpha=alpha)
    with pytest.raises(mia_hip.MiaError, match="4-byte aligned"):
        mia_hip.call("mia_ema_update", ctypes.c_void_p(18), ctypes.c_void_p(32), ctypes.c_int64(8), ctypes.c_float(0.5), None, None)


# ---------------------------------------------------------------- Python layer
def test_no_cpu_fallback():
    from losses.consistency_loss import SoftmaxMSEConsistency
    from mia_hip import ops
    z, t = torch.randn(1, 3, 8, 8), torch.randn(1, 3, 8, 8)
    with pytest.raises(mia_hip.MiaError):
        SoftmaxMSEConsistency(2)(z, t)
    with pytest.raises(mia_hip.MiaError):
        SoftmaxMSEConsistency(2)(z, t, torch.full((1, 3, 8, 8), 1 / 3), dyn=torch.tensor([1.0, 0.8]))
    with pytest.raises(mia_hip.MiaError):
        ops.ema_update(torch.zeros(8), torch.ones(8), 0.5)
    with pytest.raises(mia_hip.MiaError):
        SoftmaxMSEConsistency(8)       # nine classes
    with pytest.raises(mia_hip.MiaError):
        SoftmaxMSEConsistency(2, den_scale=0.0)


def _tiny(seed):
    from models.unet import UNet
    torch.manual_seed(seed)
    return UNet(2, 1, 3, [4, 8, 16], normalization="instance")


def test_mean_teacher_engine_layout_on_the_host():
    from losses.compound_losses import DiceAndCELoss
    from losses.dice_loss import DiceLoss
    from training.semi import MeanTeacherEngine
    model, teacher = _tiny(1), _tiny(2)
    loss = DiceAndCELoss(dice_loss=DiceLoss, dice_kwargs=dict(num_classes=2, do_bg=True), ce_loss=torch.nn.CrossEntropyLoss, ce_kwargs={})
    eng = MeanTeacherEngine(model, teacher, loss, labeled_bs=2)
    opt = eng.optimizer
    assert eng.teacher_flat.shape == opt.flat_param.shape and eng.teacher_flat.data_ptr() != opt.flat_param.data_ptr()
    assert torch.equal(eng.teacher_flat.view(torch.int32), opt.flat_param.view(torch.int32))  # bit-equal at construction
    names = {id(p): n for n, p in model.named_parameters()}
    tparams = dict(teacher.named_parameters())
    assert len(eng.teacher_params) == len(opt.params) == len(tparams)
    for p, o, t in zip(opt.params, opt.offsets, eng.teacher_params):
        assert t is tparams[names[id(p)]]
        assert t.data_ptr() == eng.teacher_flat.data_ptr() + 4 * o and t.shape == p.shape and t.is_contiguous()
        assert p.data_ptr() == opt.flat_param.data_ptr() + 4 * o
        assert not t.requires_grad and t.grad is None and p.requires_grad
        assert torch.equal(t, p.detach())
    # a write to the buffer is a write to the teacher, and not to the student
    before = opt.flat_param.clone()
    eng.teacher_flat.add_(1.0)
    assert all(torch.equal(t, p.detach() + 1.0) for p, t in zip(opt.params, eng.teacher_params))
    assert torch.equal(opt.flat_param, before)
    assert eng.num_classes == 3 and eng.consistency.num_classes == 3 and eng.ema_step == 0
    assert tuple(eng.dyn.shape) == (2,) and eng.dyn.dtype == torch.float32
    eng.consistency_weight, eng.threshold_ramp, eng.current_iter = type("R", (), {"step": staticmethod(lambda i: 0.1 * i)})(), 0.5, 3
    eng._write_dyn()
    assert eng.dyn[0].item() == pytest.approx(0.3, rel=1e-6) and eng.dyn[1].item() == pytest.approx(0.875 * math.log(3), rel=1e-6)


def test_mean_teacher_engine_rejects_a_different_teacher():
    from models.unet import UNet
    from training.semi import MeanTeacherEngine
    with pytest.raises(ValueError):
        MeanTeacherEngine(_tiny(1), UNet(2, 1, 3, [4, 8], normalization="instance"), None, labeled_bs=2)
    with pytest.raises(ValueError):
        MeanTeacherEngine(_tiny(1), _tiny(2), None, labeled_bs=0)


def _engine(name, **kw):
    """One of the three semi-supervised engines on tiny CPU networks."""
    from models.unet import UNet
    from training import semi
    if name == "MeanTeacherEngine":
        return semi.MeanTeacherEngine(_tiny(1), _tiny(2), None, **kw)
    if name == "URPCEngine":
        torch.manual_seed(1)
        return semi.URPCEngine(UNet(2, 1, 3, [4, 8, 16], deep_supervision=True, ds_layer=2, normalization="instance"), None, **kw)
    return semi.CPSEngine(_tiny(1), _tiny(2), None, **kw)


@pytest.mark.parametrize("name", ["MeanTeacherEngine", "URPCEngine", "CPSEngine"])
def test_semi_engines_share_one_batch_and_schedule_contract(name):
    with pytest.raises(ValueError, match=f"{name}: labeled_bs"):
        _engine(name, labeled_bs=0)
    with pytest.raises(ValueError, match="not supported"):
        _engine(name, labeled_bs=2, lr_scheduler_name="cosine")
    eng = _engine(name, labeled_bs=2, lr_scheduler_name="none")
    assert eng.lr_scheduler is None
    if name == "CPSEngine":
        assert eng.lr_scheduler_b is None
    assert _engine(name, labeled_bs=2).lr_scheduler is not None
    with pytest.raises(NotImplementedError, match=f"{name} implements 2-D"):
        eng.train_step({"image": torch.zeros(4, 1, 16, 16, 16), "label": torch.zeros(2, 16, 16, 16, dtype=torch.long)})
    with pytest.raises(ValueError, match=f"{name}: 1 label maps / 4 images for labeled_bs=2"):
        eng.train_step({"image": torch.zeros(4, 1, 16, 16), "label": torch.zeros(1, 16, 16, dtype=torch.long)})
    assert eng.current_iter == 0
