"""Host-side tests of cross pseudo supervision (no GPU): the float64 restatement against torch's autograd of the literal expressions,
the argument checks of the new entry points, the exported symbols, the no-CPU-fallback rule, `cps_decode`, and `CPSEngine`'s
constructor."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _cps_ref as R
import mia_hip


# ---------------------------------------------------------------- the restatement against the literal torch expressions
@pytest.mark.parametrize("k1", [2, 3, 8])
def test_restatement_equals_torch_autograd(k1):
    za, zb = R.make_case(2, k1, 9, 11)
    ta = torch.tensor(za, dtype=torch.float64, requires_grad=True)
    tb = torch.tensor(zb, dtype=torch.float64, requires_grad=True)
    ya, yb = torch.tensor(za).argmax(1), torch.tensor(zb).argmax(1)
    ref = R.evaluate(za, zb)  # tau = 0: the published CPS
    la, lb = F.cross_entropy(ta, yb), F.cross_entropy(tb, ya)
    (la + lb).backward()
    assert np.array_equal(ref["ya"], ya.numpy()) and np.array_equal(ref["yb"], yb.numpy())
    assert abs(la.item() - ref["value_a"]) <= 1e-12 and abs(lb.item() - ref["value_b"]) <= 1e-12
    assert abs((la + lb).item() - ref["value"]) <= 1e-12
    assert np.abs(ta.grad.numpy() - ref["grad_a"]).max() <= 1e-12 and np.abs(tb.grad.numpy() - ref["grad_b"]).max() <= 1e-12
    assert ref["counts"] == (198, 198, int((ya == yb).sum()))
    assert ref["ca"].all() and ref["cb"].all()
    for tau, w in ((R.thresholds()[0], 1.0), (R.thresholds()[1], 0.25), (2.0, 1.0)):  # 2: the empty mask
        ta.grad = tb.grad = None
        ca = (torch.softmax(ta.detach(), 1).max(1).values >= tau)
        cb = (torch.softmax(tb.detach(), 1).max(1).values >= tau)
        n = ya.numel()
        la = (F.cross_entropy(ta, yb, reduction="none") * cb.double()).sum() / n
        lb = (F.cross_entropy(tb, ya, reduction="none") * ca.double()).sum() / n
        (w * (la + lb)).backward()
        ref = R.evaluate(za, zb, tau, w)
        assert np.array_equal(ref["ca"], ca.numpy()) and np.array_equal(ref["cb"], cb.numpy())
        assert ref["counts"][:2] == (int(ca.sum()), int(cb.sum()))
        assert abs(la.item() - ref["value_a"]) <= 1e-12 and abs(lb.item() - ref["value_b"]) <= 1e-12
        assert abs(w * (la + lb).item() - ref["value"]) <= 1e-12
        assert np.abs(ta.grad.numpy() - ref["grad_a"]).max() <= 1e-12 and np.abs(tb.grad.numpy() - ref["grad_b"]).max() <= 1e-12
        if tau == 2.0:
            assert ref["counts"][:2] == (0, 0) and ref["value"] == 0.0
            assert not ref["grad_a"].any() and not ref["grad_b"].any() and np.isfinite(ref["grad_a"]).all()
        else:
            assert 0 < ref["counts"][0] < n and 0 < ref["counts"][1] < n  # both branches
        assert np.array_equal(ref["code"], R.encode(ref["ya"], ref["yb"], ref["ca"], ref["cb"]))
        for got, want in zip(R.decode(ref["code"]), (ref["ya"], ref["yb"], ref["ca"], ref["cb"])):
            assert np.array_equal(got, want)


def test_restatement_takes_given_flags_and_ties_go_to_the_lowest_index():
    za, zb = R.tie_case(2, 3, 9, 11)
    ref = R.evaluate(za, zb)
    top2 = np.sort(za, axis=1)[:, -2:]
    assert (top2[:, 0] == top2[:, 1]).mean() > 0.15  # ties are common
    assert np.array_equal(ref["ya"], torch.tensor(za).argmax(1).numpy())
    first_max = (za == za.max(1, keepdims=True)).argmax(1)
    assert np.array_equal(ref["ya"], first_max)
    ca = np.zeros((2, 9, 11), bool)
    ca[0] = True
    got = R.evaluate(za, zb, ca=ca, cb=~ca)
    assert got["counts"][:2] == (99, 99)
    assert not got["grad_b"][1].any() and not got["grad_a"][0].any() and got["grad_b"][0].any() and got["grad_a"][1].any()


def test_bounds_dominate_the_terms_they_bound():
    za, zb = R.make_case(2, 3, 9, 11)
    ref = R.evaluate(za, zb, R.thresholds()[0], 0.5)
    # term = log sum exp(z - max) + (max - z_y) <= ln K + |z_y - max| <= ln K * (1 + |z_y - max|)
    assert 0.0 <= ref["value_a"] <= np.log(3) * ref["value_mag_a"] and 0.0 <= ref["value_b"] <= np.log(3) * ref["value_mag_b"]
    assert (np.abs(ref["grad_a"]) <= ref["grad_mag_a"]).all() and (np.abs(ref["grad_b"]) <= ref["grad_mag_b"]).all()


# ---------------------------------------------------------------- C ABI: argument errors without a device
def _ptr(v):
    return None if v is None else ctypes.c_void_p(16 * v)  # never dereferenced: the checks fail before any launch


def _fwd(**kw):
    a = dict(za=1, zb=1, dyn=None, nb=1, hw=64, k1=3, slabs=1, ws=1, code=1, out=1, counts=1, sa=(192, 64, 1), sb=(192, 64, 1))
    a.update(kw)
    i64 = ctypes.c_int64
    mia_hip.call("mia_cps_fwd", _ptr(a["za"]), _ptr(a["zb"]), _ptr(a["dyn"]), a["nb"], i64(a["hw"]), a["k1"],
                 *(i64(s) for s in a["sa"]), *(i64(s) for s in a["sb"]), a["slabs"], _ptr(a["ws"]), _ptr(a["code"]), _ptr(a["out"]),
                 _ptr(a["counts"]), None)


def _bwd(**kw):
    a = dict(za=1, zb=1, code=1, dyn=None, gout=None, dza=1, dzb=1, nb=1, hw=64, k1=3, sa=(192, 64, 1), sb=(192, 64, 1),
             ga=(192, 64, 1), gb=(192, 64, 1))
    a.update(kw)
    i64 = ctypes.c_int64
    mia_hip.call("mia_cps_bwd", _ptr(a["za"]), _ptr(a["zb"]), _ptr(a["code"]), _ptr(a["dyn"]), _ptr(a["gout"]), _ptr(a["dza"]),
                 _ptr(a["dzb"]), a["nb"], i64(a["hw"]), a["k1"], *(i64(s) for n in ("sa", "sb", "ga", "gb") for s in a[n]), None)


def test_cps_argument_errors():
    for name in ("za", "zb", "ws", "code", "out", "counts"):
        with pytest.raises(mia_hip.MiaError, match="mia_cps_fwd: null pointer"):
            _fwd(**{name: None})
    for kw in (dict(nb=0), dict(nb=-1), dict(hw=0), dict(hw=-4), dict(slabs=0), dict(nb=1 << 16, hw=1 << 16), dict(hw=1 << 31),
               dict(nb=1 << 20, slabs=1 << 10)):
        with pytest.raises(mia_hip.MiaError, match="mia_cps_fwd: bad shape"):
            _fwd(**kw)
    with pytest.raises(mia_hip.MiaError, match="k1=0"):
        _fwd(k1=0)
    with pytest.raises(mia_hip.MiaError, match="k1=9"):
        _fwd(k1=9)
    for kw in (dict(sa=(192, -64, 1)), dict(sa=(-1, 64, 1)), dict(sb=(192, 64, -1))):
        with pytest.raises(mia_hip.MiaError, match="mia_cps_fwd: negative strides"):
            _fwd(**kw)
    for name in ("za", "zb", "code", "dza", "dzb"):
        with pytest.raises(mia_hip.MiaError, match="mia_cps_bwd: null pointer"):
            _bwd(**{name: None})
    for kw in (dict(nb=0), dict(hw=0), dict(nb=1 << 16, hw=1 << 16)):
        with pytest.raises(mia_hip.MiaError, match="mia_cps_bwd: bad shape"):
            _bwd(**kw)
    with pytest.raises(mia_hip.MiaError, match="k1=0"):
        _bwd(k1=0)
    with pytest.raises(mia_hip.MiaError, match="k1=9"):
        _bwd(k1=9)
    for name in ("sa", "sb", "ga", "gb"):
        with pytest.raises(mia_hip.MiaError, match="mia_cps_bwd: negative strides"):
            _bwd(**{name: (192, 64, -1)})
    lib = mia_hip.lib()
    assert lib.mia_cps_workspace(3, 4) == 84  # seven 4-byte words per block
    assert lib.mia_cps_workspace(0, 4) < 0 and lib.mia_cps_workspace(3, 0) < 0
    assert lib.mia_cps_workspace(1 << 20, 1 << 10) < 0


def test_new_symbols_are_declared_and_exported():
    protos = mia_hip.parse_header()
    l = ctypes.CDLL(mia_hip.LIB_PATH)
    for name, nargs in (("mia_cps_workspace", 2), ("mia_cps_fwd", 18), ("mia_cps_bwd", 23)):
        assert name in protos and len(protos[name][1]) == nargs, name
        assert hasattr(l, name), f"{name} declared in include/mia_hip.h but not exported"
    for name in ("mia_consistency_fwd", "mia_consistency_bwd", "mia_ema_update"):  # the header move kept the older entry points
        assert hasattr(l, name)


# ---------------------------------------------------------------- Python layer
def test_no_cpu_fallback():
    from losses.cross_pseudo import CrossPseudoSupervisionLoss
    from mia_hip import ops
    za, zb = torch.randn(1, 3, 8, 8, requires_grad=True), torch.randn(1, 3, 8, 8, requires_grad=True)
    with pytest.raises(mia_hip.MiaError):
        CrossPseudoSupervisionLoss(2)(za, zb)
    with pytest.raises(mia_hip.MiaError):
        CrossPseudoSupervisionLoss(2)(za, zb, dyn=torch.tensor([1.0, 0.6]))
    with pytest.raises(mia_hip.MiaError):
        ops.CrossPseudoFn.apply(za, zb, None)
    with pytest.raises(mia_hip.MiaError):
        CrossPseudoSupervisionLoss(8)  # nine classes
    assert ops.CPS_MAX_CLASSES == 8 and CrossPseudoSupervisionLoss(7).num_classes == 8


def test_cps_decode_round_trips():
    from mia_hip import ops
    rng = np.random.default_rng(3)
    ya, yb = rng.integers(0, 8, (2, 5, 7)), rng.integers(0, 8, (2, 5, 7))
    ca, cb = rng.random((2, 5, 7)) < 0.5, rng.random((2, 5, 7)) < 0.5
    code = R.encode(ya, yb, ca, cb)
    assert code.dtype == np.uint8
    got = ops.cps_decode(torch.from_numpy(code))
    assert got[0].dtype == got[1].dtype == torch.int64 and got[2].dtype == got[3].dtype == torch.bool
    for g, want in zip(got, (ya, yb, ca, cb)):
        assert np.array_equal(g.numpy(), want)
    every = torch.arange(256, dtype=torch.uint8)  # every byte value
    y0, y1, c0, c1 = ops.cps_decode(every)
    assert torch.equal((y0 | (y1 << 3) | (c0.long() << 6) | (c1.long() << 7)).to(torch.uint8), every)


def _tiny(seed, classes=3):
    from models.unet import UNet
    torch.manual_seed(seed)
    return UNet(2, 1, classes, [4, 8, 16], normalization="instance")


def test_cps_engine_constructor():
    from training.semi import CPSEngine
    a, b = _tiny(1), _tiny(2)
    eng = CPSEngine(a, b, None, labeled_bs=2, cps_weight=0.5)
    assert eng.model is a and eng.model_b is b and eng.optimizer is not eng.optimizer_b
    assert eng.lr_scheduler is not None and eng.lr_scheduler_b is not None and eng.lr_scheduler is not eng.lr_scheduler_b
    assert eng.optimizer.flat_param.data_ptr() != eng.optimizer_b.flat_param.data_ptr()
    assert not torch.equal(eng.optimizer.flat_param, eng.optimizer_b.flat_param)  # different initialisations
    for opt, net in ((eng.optimizer, a), (eng.optimizer_b, b)):  # each optimizer owns its own network's parameters
        own = {id(p) for p in net.parameters()}
        assert {id(p) for p in opt.params} == own
        for p, o in zip(opt.params, opt.offsets):
            assert p.data_ptr() == opt.flat_param.data_ptr() + 4 * o
    assert eng.num_classes == 3 and eng.cps.num_classes == 3 and not eng.cps_on_labeled
    assert tuple(eng.dyn.shape) == (2,) and eng.dyn.dtype == torch.float32
    eng.cps_weight, eng.confidence_threshold, eng.current_iter = type("R", (), {"step": staticmethod(lambda i: 0.1 * i)})(), 0.75, 3
    eng._write_dyn()
    assert eng.dyn[0].item() == pytest.approx(0.3, rel=1e-6) and eng.dyn[1].item() == 0.75
    with pytest.raises(ValueError, match="same object"):
        CPSEngine(a, a, None, labeled_bs=2)
    with pytest.raises(ValueError, match="classes"):
        CPSEngine(_tiny(1), _tiny(2, classes=4), None, labeled_bs=2)
    with pytest.raises(ValueError, match="labeled_bs"):
        CPSEngine(_tiny(1), _tiny(2), None, labeled_bs=0)
    with pytest.raises(ValueError, match="not supported"):
        CPSEngine(_tiny(1), _tiny(2), None, labeled_bs=2, lr_scheduler_name="cosine")
    with pytest.raises(ValueError):
        eng.predict(torch.zeros(1, 1, 8, 8), use="both")
