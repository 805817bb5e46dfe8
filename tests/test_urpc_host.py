"""Host-side tests of the pyramid consistency work (no GPU): the float64 restatement in tests/_urpc_ref.py against torch's autograd of
the literal expression, the argument checks of the three entry points through ctypes, the no-CPU-fallback rule, the shape errors of
PyramidConsistencyLoss, and what URPCEngine decides before a kernel runs."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _urpc_ref as R
import mia_hip


# ---------------------------------------------------------------- the restatement against the literal torch expression
def _literal(zs, factors):
    """zs: float64 leaves [N, K, h, w]."""
    us = [z if f == 1 else F.interpolate(z, scale_factor=f, mode="bilinear", align_corners=False) for z, f in zip(zs, factors)]
    ps = [torch.softmax(u, 1) for u in us]
    lps = [torch.log_softmax(u, 1) for u in us]
    m = sum(ps) / len(ps)
    terms = []
    for p, lp in zip(ps, lps):
        v = (torch.xlogy(m, m) - m * lp).sum(1, keepdim=True)
        w = torch.exp(-v)
        d = (m - p) ** 2
        terms.append(torch.mean(d * w) / (torch.mean(w) + 1e-8) + torch.mean(v))
    return torch.stack(terms)


@pytest.mark.parametrize("factors", [(1, 2), (1, 4, 16), (1, 2, 4, 8, 16)], ids=str)
@pytest.mark.parametrize("k1", [2, 3, 8])
def test_restatement_equals_torch_autograd(k1, factors):
    zs = R.make_case(2, k1, 2, 3, factors, seed=1)
    weight, gout = 0.37, 0.625
    ref = R.evaluate(zs, factors, weight, gout)
    leaves = [torch.tensor(z).permute(0, 3, 1, 2).contiguous().requires_grad_(True) for z in zs]
    terms = _literal(leaves, factors)
    loss = terms.mean()
    (gout * weight * loss).backward()
    assert np.abs(terms.detach().numpy() - ref["terms"]).max() <= 1e-12
    assert abs(loss.item() - ref["out"][1]) <= 1e-12 and abs(weight * loss.item() - ref["out"][0]) <= 1e-12
    for leaf, dz in zip(leaves, ref["dz"]):
        assert np.abs(leaf.grad.permute(0, 2, 3, 1).numpy() - dz).max() <= 1e-12
    assert max(np.abs(dz).max() for dz in ref["dz"]) > 1e-6, "the comparison is not one of zeros"


def test_one_class_and_equal_scales_give_zero():
    zs = R.make_case(2, 1, 1, 2, (1, 2, 4))
    ref = R.evaluate(zs, (1, 2, 4))
    assert ref["out"].tolist() == [0.0, 0.0] and all(not dz.any() for dz in ref["dz"])
    flat = [np.full((1, 8 // f, 8 // f, 3), 1.5) * np.arange(3) for f in (1, 2, 8)]  # every scale upsamples to the same image
    ref = R.evaluate(flat, (1, 2, 8))
    assert abs(ref["out"][1]) <= 1e-14 and max(np.abs(dz).max() for dz in ref["dz"]) <= 1e-14


def test_case_tables():
    cases = R.shape_cases()
    assert len(set(cases)) == len(cases)
    for fs in R.FACTOR_SETS:
        mine = [c for c in cases if c[4] == fs]
        assert {(c[2], c[3]) for c in mine} == set(R.COARSE_HW)
        assert {c[5] for c in mine} == {1, 2, 3}
    assert {c[1] for c in cases} == set(R.ALL_K1) and {c[0] for c in cases} == {1, 3}
    assert max(nb * ch * cw * max(fs) ** 2 * k1 * 4 for nb, k1, ch, cw, fs, _ in cases) <= 1 << 20, "the largest tensor stays under 1 MiB"
    a, b = R.make_case(3, 3, 5, 7, (1, 4, 16)), R.make_case(3, 3, 5, 7, (1, 4, 16))
    assert all(np.array_equal(x, y) and np.array_equal(x.astype(np.float32).astype(np.float64), x) for x, y in zip(a, b))
    assert [z.shape for z in a] == [(3, 80, 112, 3), (3, 20, 28, 3), (3, 5, 7, 3)]


# ---------------------------------------------------------------- C ABI: argument errors without a device
def _ptr(v):
    return None if v is None else ctypes.c_void_p(16 * v)  # never dereferenced: the checks fail before any launch


def _host(ns, z=1, factors=(1, 2, 4, 8, 16, 16), strides=None):
    zp = (ctypes.c_void_p * ns)(*[None if z is None else 16 * (i + 1) for i in range(ns)])
    fac = (ctypes.c_int * ns)(*factors[:ns])
    st = (ctypes.c_int64 * (3 * ns))(*(strides or [192, 64, 1] * ns))
    return zp, fac, st


def _fwd(**kw):
    a = dict(ns=3, nb=1, H=16, W=16, k1=3, dyn=None, slabs=1, ws=1, sums=1, terms=1, out=1, z=1, factors=(1, 2, 4, 8, 16, 16),
             strides=None, arrays=True)
    a.update(kw)
    zp, fac, st = _host(max(a["ns"], 1), a["z"], a["factors"], a["strides"]) if a["arrays"] else (None, None, None)
    mia_hip.call("mia_urpc_fwd", zp, fac, st, a["ns"], a["nb"], a["H"], a["W"], a["k1"], _ptr(a["dyn"]), a["slabs"], _ptr(a["ws"]),
                 _ptr(a["sums"]), _ptr(a["terms"]), _ptr(a["out"]), None)


def _bwd(**kw):
    a = dict(ns=3, nb=1, H=16, W=16, k1=3, dyn=None, gout=None, sums=1, z=1, dz=1, factors=(1, 2, 4, 8, 16, 16), strides=None,
             gstrides=None, arrays=True)
    a.update(kw)
    zp, fac, st = _host(max(a["ns"], 1), a["z"], a["factors"], a["strides"]) if a["arrays"] else (None, None, None)
    dp, _, gst = _host(max(a["ns"], 1), a["dz"], a["factors"], a["gstrides"]) if a["arrays"] else (None, None, None)
    mia_hip.call("mia_urpc_bwd", zp, fac, st, dp, gst, a["ns"], a["nb"], a["H"], a["W"], a["k1"], _ptr(a["sums"]), _ptr(a["dyn"]),
                 _ptr(a["gout"]), None)


@pytest.mark.parametrize("entry", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_urpc_argument_errors(entry):
    with pytest.raises(mia_hip.MiaError, match="null pointer"):
        entry(arrays=False)
    with pytest.raises(mia_hip.MiaError, match="null pointer"):
        entry(z=None)
    for ns in (1, 6, 0, -3):
        with pytest.raises(mia_hip.MiaError, match="scales, not in"):
            entry(ns=ns)
    with pytest.raises(mia_hip.MiaError, match="factor 3"):
        entry(factors=(1, 3, 4))
    with pytest.raises(mia_hip.MiaError, match="factor 32"):
        entry(factors=(1, 2, 32), H=64, W=64)
    with pytest.raises(mia_hip.MiaError, match="factor 1 of scale 2"):
        entry(factors=(1, 2, 1))
    with pytest.raises(mia_hip.MiaError, match="the first scale"):
        entry(factors=(2, 1, 4))
    for k1 in (0, 9):
        with pytest.raises(mia_hip.MiaError, match=f"k1={k1}"):
            entry(k1=k1)
    with pytest.raises(mia_hip.MiaError, match="does not divide"):
        entry(H=18)  # a 16 x 16 pyramid handed an 18-row main output: factor 4 does not divide it
    with pytest.raises(mia_hip.MiaError, match="does not divide"):
        entry(W=8, ns=5)
    for kw in (dict(nb=0), dict(H=0), dict(W=-16), dict(nb=1 << 12, H=1 << 10, W=1 << 10)):
        with pytest.raises(mia_hip.MiaError, match="bad shape"):
            entry(**kw)
    with pytest.raises(mia_hip.MiaError, match="negative strides"):
        entry(strides=[192, 64, 1, 192, -64, 1, 192, 64, 1])
    with pytest.raises(mia_hip.MiaError, match="beyond 2\\^31"):
        entry(strides=[192, 64, 1, 192, 1 << 31, 1, 192, 64, 1])


def test_urpc_argument_errors_of_one_direction():
    for name in ("ws", "sums", "terms", "out"):
        with pytest.raises(mia_hip.MiaError, match="null pointer"):
            _fwd(**{name: None})
    for slabs in (0, -1, 1 << 30):
        with pytest.raises(mia_hip.MiaError, match="slab count"):
            _fwd(slabs=slabs)
    with pytest.raises(mia_hip.MiaError, match="null pointer"):
        _bwd(sums=None)
    with pytest.raises(mia_hip.MiaError, match="null pointer"):
        _bwd(dz=None)
    with pytest.raises(mia_hip.MiaError, match="negative strides"):
        _bwd(gstrides=[-1, 64, 1] * 3)
    lib = mia_hip.lib()
    assert lib.mia_urpc_workspace(3, 4, 5) == 3 * 5 * 4 * 6
    for bad in ((0, 4, 5), (3, 1, 5), (3, 6, 5), (3, 4, 0), (1 << 20, 5, 1 << 10)):
        assert lib.mia_urpc_workspace(*bad) < 0


# ---------------------------------------------------------------- Python layers
def _outs(n=2, k=3, side=32, factors=(1, 2, 4)):
    return [torch.zeros(n, k, side // f, side // f) for f in factors]


@pytest.mark.parametrize("fused", [None, False, True])
def test_no_cpu_fallback(fused):
    from losses.pyramid_consistency import PyramidConsistencyLoss
    with pytest.raises(mia_hip.MiaError, match="no CPU fallback"):
        PyramidConsistencyLoss(fused=fused)(_outs())
    from mia_hip import ops
    with pytest.raises(mia_hip.MiaError, match="no CPU fallback"):
        ops.PyramidConsistencyFn.apply(None, *_outs())
    assert ops.URPC_MAX_SCALES == 5


def test_shape_errors_come_before_anything_runs():
    """CPU tensors: a shape error must win over the no-CPU-fallback error, i.e. it is raised before the device is looked at."""
    from losses.pyramid_consistency import PyramidConsistencyLoss, pyramid_factors
    loss = PyramidConsistencyLoss()
    with pytest.raises(ValueError, match="at least two"):
        loss(_outs(factors=(1,)))
    with pytest.raises(ValueError, match="at least two"):
        loss([])
    with pytest.raises(ValueError, match="12x12.*32x32"):
        loss([torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 12, 12)])
    with pytest.raises(ValueError, match="16x8.*32x32"):
        loss([torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 16, 8)])
    with pytest.raises(ValueError, match="64x64.*32x32"):
        loss([torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 64, 64)])
    with pytest.raises(ValueError, match="images or classes"):
        loss([torch.zeros(2, 3, 32, 32), torch.zeros(1, 3, 16, 16)])
    with pytest.raises(ValueError, match="images or classes"):
        loss([torch.zeros(2, 3, 32, 32), torch.zeros(2, 4, 16, 16)])
    with pytest.raises(ValueError, match=r"\[N,K,h,w\]"):
        loss([torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 16)])
    assert pyramid_factors(_outs(factors=(1, 8, 2))) == [1, 8, 2]


def test_fused_true_names_what_the_kernel_cannot_serve():
    from losses.pyramid_consistency import PyramidConsistencyLoss
    loss = PyramidConsistencyLoss(fused=True)
    with pytest.raises(ValueError, match="factor 32"):
        loss(_outs(side=64, factors=(1, 32)))
    with pytest.raises(ValueError, match="6 outputs"):
        loss(_outs(factors=(1, 2, 4, 8, 16, 2)))
    with pytest.raises(ValueError, match="9 classes"):
        loss(_outs(k=9))
    with pytest.raises(ValueError, match="fp32"):
        loss([o.double() for o in _outs()])


def _sup():
    from losses.compound_losses import DiceAndCELoss
    return DiceAndCELoss(dice_kwargs=dict(num_classes=2, do_bg=True))


def test_engine_needs_auxiliary_heads():
    from models.unet import UNet
    from training.semi import URPCEngine
    with pytest.raises(ValueError, match="auxiliary heads"):
        URPCEngine(UNet(2, 1, 3, [4, 8, 16], normalization="instance", dropout_prob=None), _sup(), labeled_bs=2)
    with pytest.raises(ValueError, match="auxiliary heads"):
        URPCEngine(UNet(2, 1, 3, [4, 8, 16], deep_supervision=True, ds_layer=1, normalization="instance", dropout_prob=None), _sup(),
                   labeled_bs=2)
    with pytest.raises(ValueError, match="labeled_bs"):
        URPCEngine(UNet(2, 1, 3, [4, 8, 16], deep_supervision=True, ds_layer=2, normalization="instance"), _sup(), labeled_bs=0)


def test_engine_layout_and_schedule_on_the_host():
    from losses.deep_supervision import DeepSupervisionLoss
    from losses.pyramid_consistency import PyramidConsistencyLoss
    from models.unet import UNet
    from training.semi import URPCEngine
    model = UNet(2, 1, 3, [4, 8, 16, 32], deep_supervision=True, ds_layer=3, normalization="instance", dropout_prob=None)
    eng = URPCEngine(model, _sup(), labeled_bs=2, consistency_weight=0.25)
    assert eng.num_outputs == 3
    assert isinstance(eng.supervised_loss, DeepSupervisionLoss) and eng.supervised_loss.weights == pytest.approx([1 / 3] * 3, abs=1e-15)
    assert isinstance(eng.consistency, PyramidConsistencyLoss) and eng.consistency.fused is None
    assert tuple(eng.dyn.shape) == (2,) and eng.dyn.dtype == torch.float32 and eng.dyn.tolist() == [0.0, 0.0]
    eng._write_dyn()
    assert eng.dyn.tolist() == [0.25, 0.0]
    eng.consistency_weight, eng.current_iter = type("Ramp", (), {"step": staticmethod(lambda i: 0.1 * i)})(), 3
    eng._write_dyn()
    assert eng.dyn[0].item() == pytest.approx(0.3, rel=1e-6)
    assert URPCEngine(model, _sup(), labeled_bs=2, consistency=False).consistency is None
    with pytest.raises(NotImplementedError, match="2-D"):
        eng.train_step({"image": torch.zeros(4, 1, 8, 8, 8), "label": torch.zeros(2, 8, 8, 8, dtype=torch.long)})
    with pytest.raises(ValueError, match="labeled_bs=2"):
        eng.train_step({"image": torch.zeros(4, 1, 8, 8), "label": torch.zeros(1, 8, 8, dtype=torch.long)})
