"""csrc/vat.hip on the GPU against the float64 restatement (tests/_vat_ref.py): value and gradient of the KL consistency in every layout
class, the run-time `dyn` weight, determinism, and the noise / sum-of-squares / perturbation kernels of the power iteration.

Bounds, in the form tests/test_gpu_consistency.py derives (32 roundings x 2^-24 ~ 2e-6 of the magnitudes being rounded):
    |L - ref| <= 2e-6 * coef * sum_pix sum_k p_k (|log p_k| + |log q_k|)
    |g - ref| <= 2e-6 * coef * (p_j + q_j) + 1e-12                                  per element
mia_sample_sumsq: 2^-23 relative (double accumulation, one rounding, and the fp32 rounding of the comparison itself);
mia_vat_perturb: 4 fp32 roundings of the larger of |x| and |step| (the kernel computes in double and rounds once)."""
import ctypes
import functools

import pytest
import torch

import _vat_ref as V
from mia_hip import MiaError, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(16, 20), (15, 17)]  # hw % 4 == 0: four pixels per thread; hw odd: the scalar class
K1S = [2, 3, 4, 8]
LAYOUTS = ["planar", "clast", "mixed", "slice"]
NB = 3


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _case(k1, h, w):
    """Inputs and float64 references of one case, computed once and never modified."""
    g = torch.Generator().manual_seed(31 * k1 + h)
    z = torch.randn(NB, k1, h, w, generator=g) * 3
    zt = torch.randn(NB, k1, h, w, generator=g) * 3
    refs = {red: V.kl(z, zt, den) for red, den in (("mean", NB * h * w), ("batchmean", NB))}
    return z, zt, refs


def _planar(a):
    return a.clone().to(DEV)


def _clast(a, lead=0):
    """The head's layout: memory [B][H][W][K] viewed as [B, K, H, W]; with `lead`, a batch slice z[lead:] of a larger tensor."""
    t = a.to(DEV).permute(0, 2, 3, 1)
    big = torch.full((lead + t.shape[0],) + tuple(t.shape[1:]), 7.0, device=DEV)
    big[lead:] = t
    return big.permute(0, 3, 1, 2)[lead:]


def _inputs(z, zt, layout):
    a = {"planar": _planar, "clast": _clast, "mixed": _clast, "slice": lambda t: _clast(t, 2)}[layout](z)
    b = {"planar": _planar, "clast": _clast, "mixed": _planar, "slice": _clast}[layout](zt)
    return a.detach().requires_grad_(True), b


def _run(z, zt, dyn, den, gout=None):
    z.grad = None
    loss = ops.KLConsistencyFn.apply(z, zt, dyn, den)
    out = ops.KLConsistencyFn.last_out
    (loss if gout is None else loss * gout).backward()
    return out.clone(), z.grad.clone()


def _check(out, grad, ref, what):
    value, g, mag, gmag = ref
    vb, gb = 2e-6 * float(mag), 2e-6 * gmag + 1e-12
    verr, gerr = abs(float(out[1].double()) - float(value)), (grad.cpu().double() - g).abs()
    print(f"{what}: L={float(out[1]):.9g} ref={float(value):.9g}  value err/bound={verr / max(vb, 1e-300):.3f}  "
          f"gradient max err/bound={float((gerr / gb).max()):.3f}")
    assert torch.isfinite(out).all() and torch.isfinite(grad).all()
    assert verr <= vb, (what, verr, vb)
    assert bool((gerr <= gb).all()), (what, float((gerr / gb).max()))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k1", K1S)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_kl_value_and_gradient_against_restatement(size, k1, layout):
    _need_gpu()
    h, w = size
    z, zt, refs = _case(k1, h, w)
    a, b = _inputs(z, zt, layout)
    for red, den in (("mean", NB * h * w), ("batchmean", NB)):
        out, grad = _run(a, b, None, float(den))
        assert float(out[2]) == 1.0 and float(out[0]) == float(out[1])
        _check(out, grad, refs[red], f"{red} {size} k1={k1} {layout}")
    again, grad2 = _run(a, b, None, float(NB))
    assert torch.equal(again, out) and torch.equal(grad2, grad)  # run to run: equal bits


def test_kl_module_paths_agree():
    _need_gpu()
    from losses.vat_loss import VATLoss, kl_consistency
    z, zt, refs = _case(3, 16, 20)
    a, b = _inputs(z, zt, "clast")
    for red in ("mean", "batchmean"):
        fused = float(kl_consistency(a, b, None, red).detach())
        slow = float(VATLoss(reduction=red, fused=False)(a, b).detach())
        ref = float(refs[red][0])
        assert abs(fused - ref) <= 2e-6 * float(refs[red][2]) and abs(slow - ref) <= 1e-4 * float(refs[red][2])
    # more than 8 classes: the tensor-op form, silently
    z9 = torch.randn(2, 9, 4, 4, device=DEV)
    assert torch.isfinite(VATLoss()(z9, z9 + 1))
    with pytest.raises(MiaError):
        kl_consistency(z9, z9)


def test_kl_saturated_and_equal_inputs():
    _need_gpu()
    z = torch.zeros(2, 3, 4, 4, device=DEV)
    z[:, 0], z[:, 1] = 80.0, -80.0
    zt = torch.zeros(2, 3, 4, 4, device=DEV)
    zt[:, 0], zt[:, 1], zt[:, 2] = -80.0, 80.0, -80.0  # a one-hot target on the class the prediction excludes
    z.requires_grad_(True)
    out, grad = _run(z, zt, None, 32.0)
    ref = V.kl(z.detach().cpu(), zt.cpu(), 32.0)
    assert torch.isfinite(out).all() and torch.isfinite(grad).all()
    _check(out, grad, ref, "saturated")
    same = torch.randn(2, 4, 6, 6, device=DEV)
    out, grad = _run(same.clone().requires_grad_(True), same, None, 72.0)
    assert float(out[1]) == 0.0 and float(grad.abs().max()) == 0.0


def test_kl_weight_from_dyn_and_grad_out():
    _need_gpu()
    z, zt, _ = _case(4, 16, 20)
    a, b = _inputs(z, zt, "planar")
    base, g1 = _run(a, b, None, 960.0)
    d1, d2 = torch.tensor([0.75, 9.0], device=DEV), torch.tensor([1.5, 9.0], device=DEV)
    o1, ga = _run(a, b, d1, 960.0)
    o2, gb = _run(a, b, d2, 960.0)
    assert float(o1[2]) == 0.75 and float(o2[2]) == 1.5 and torch.equal(o1[1], base[1]) and torch.equal(o2[1], base[1])
    assert float(o2[0]) == 2.0 * float(o1[0])  # doubling the weight doubles the bits
    assert torch.equal(gb, 2.0 * ga)
    _, g4 = _run(a, b, None, 960.0, gout=4.0)
    assert torch.equal(g4, 4.0 * g1)


def test_kl_gradient_slice_leaves_the_rest_alone():
    """The backward writes by its own strides: a gradient buffer that is a batch slice of a larger channels-last tensor."""
    _need_gpu()
    z, zt, refs = _case(3, 16, 20)
    a, b = _inputs(z, zt, "clast")
    big = torch.full((NB + 2, 16, 20, 3), 5.0, device=DEV)
    dz = big.permute(0, 3, 1, 2)[1:1 + NB]
    ws = torch.empty(ops.lib().mia_kl_workspace(NB, 1), device=DEV)
    coef, out = torch.empty(1, device=DEV), torch.empty(3, device=DEV)
    st, tt, gt = ops._pix_strides(a), ops._pix_strides(b), ops._pix_strides(dz)
    ops.call("mia_kl_fwd", ops._p(a), ops._p(b), None, NB, ctypes.c_int64(320), 3, *ops._strides_i64(st), *ops._strides_i64(tt),
             ctypes.c_double(960.0), 1, ops._p(ws), ops._p(coef), ops._p(out), ops._stream())
    ops.call("mia_kl_bwd", ops._p(a), ops._p(b), ops._p(coef), None, None, ops._p(dz), NB, ctypes.c_int64(320), 3, *ops._strides_i64(st),
             *ops._strides_i64(tt), *ops._strides_i64(gt), ops._stream())
    _check(out, dz, refs["mean"], "gradient slice")
    assert bool((big[0] == 5.0).all()) and bool((big[1 + NB:] == 5.0).all())
    with pytest.raises(MiaError):  # k1 = 9
        ops.call("mia_kl_fwd", ops._p(a), ops._p(b), None, NB, ctypes.c_int64(320), 9, *ops._strides_i64(st), *ops._strides_i64(tt),
                 ctypes.c_double(960.0), 1, ops._p(ws), ops._p(coef), ops._p(out), ops._stream())


@pytest.mark.parametrize("per", [1, 7, 4096, 16 * 20, 3 * 4096 + 5])
def test_sample_sumsq(per):
    _need_gpu()
    g = torch.Generator().manual_seed(per)
    x = torch.randn(NB, per, generator=g)
    got = ops.sample_sumsq(x.to(DEV)).cpu().double()
    ref = V.sumsq(x)
    assert bool(((got - ref).abs() <= 2.0 ** -23 * ref).all()), (got, ref)
    assert torch.equal(ops.sample_sumsq(x.to(DEV)).cpu().double(), got)


@pytest.mark.parametrize("per", [1, 7, 4096, 16 * 20])
def test_vat_perturb(per):
    _need_gpu()
    g = torch.Generator().manual_seed(100 + per)
    x, gr = torch.randn(NB, per, generator=g), torch.randn(NB, per, generator=g) * 1e-3
    ss = ops.sample_sumsq(gr.to(DEV))
    for gscale, s in ((1.0, 10.0), (10.0, 6.0)):
        got = ops.vat_perturb(x.to(DEV), gr.to(DEV), ss, gscale, s).cpu().double()
        ref = V.perturb(x, gr, gscale, s)
        bound = 4 * 2.0 ** -24 * torch.maximum(x.double().abs(), (ref - x.double()).abs()) + 1e-30
        assert bool(((got - ref).abs() <= bound).all()), float(((got - ref).abs() / bound).max())
    # the scale read from the device wins over the argument
    sd = torch.tensor([0.0, 6.0], device=DEV)
    a = ops.vat_perturb(x.to(DEV), gr.to(DEV), ss, 10.0, 123.0, sd[1:2])
    assert torch.equal(a.cpu().double(), got)
    # a zero gradient returns x, not NaN
    zero = torch.zeros(NB, per, device=DEV)
    assert torch.equal(ops.vat_perturb(x.to(DEV), zero, ops.sample_sumsq(zero), 10.0, 6.0).cpu(), x)


def test_vat_noise():
    _need_gpu()
    per = 1 << 14

    def noise(nb, seed, off):
        u = torch.empty(nb, per, device=DEV)
        ops.call("mia_vat_noise", ops._p(u), nb, ctypes.c_int64(per), ctypes.c_uint64(seed), ctypes.c_uint64(off), ops._stream())
        return u

    u = noise(4, 1234, 8)
    assert float(u.min()) >= -0.5 and float(u.max()) < 0.5
    assert torch.equal(noise(4, 1234, 8), u)
    assert not torch.equal(noise(4, 1235, 8), u) and not torch.equal(noise(4, 1234, 12), u)
    assert torch.equal(noise(2, 1234, 8), u[:2])  # a sample's values do not depend on nb
    mean, sigma = float(u.double().mean()), (1.0 / 12.0 / u.numel()) ** 0.5  # 2^16 values of variance 1/12
    assert abs(mean) < 5 * sigma, (mean, sigma)
    # through torch's generator: the same seed reproduces, and the offset moves on
    torch.manual_seed(7)
    a = ops.vat_noise((2, 1, 8, 9), DEV)
    b = ops.vat_noise((2, 1, 8, 9), DEV)
    torch.manual_seed(7)
    assert torch.equal(ops.vat_noise((2, 1, 8, 9), DEV), a) and not torch.equal(a, b)
