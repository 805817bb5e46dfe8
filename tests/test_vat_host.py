"""CPU checks of the virtual-adversarial-training reference (tests/_vat_ref.py) against closed forms, of the integer probes'
preconditions, and of the C header."""
import pytest
import torch

import _conv_ref as R
import _vat_ref as V
import mia_hip


def _logits(seed, shape=(3, 4, 5, 7), scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


def test_kl_is_non_negative_and_zero_for_equal_logits():
    for seed in range(4):
        z, zt = _logits(seed), _logits(100 + seed)
        value, grad, mag, gmag = V.kl(z, zt, 3 * 35)
        assert float(value) >= 0.0 and float(mag) >= float(value)
        assert bool((gmag >= grad.abs()).all())
    value, grad, _, _ = V.kl(zt, zt, 3 * 35)
    assert float(value) == 0.0 and float(grad.abs().max()) == 0.0


def test_kl_gradient_matches_central_differences():
    z, zt = _logits(7, (2, 3, 3, 4), 1.5), _logits(8, (2, 3, 3, 4), 1.5)
    den = 2.0
    _, grad, _, _ = V.kl(z, zt, den)
    h = 1e-6
    fd = torch.zeros_like(z)
    flat = z.reshape(-1)
    for i in range(flat.numel()):
        zp, zm = flat.clone(), flat.clone()
        zp[i] += h
        zm[i] -= h
        fd.reshape(-1)[i] = (V.kl(zp.reshape(z.shape), zt, den)[0] - V.kl(zm.reshape(z.shape), zt, den)[0]) / (2 * h)
    assert float((fd - grad).abs().max()) < 1e-8
    # a softmax gradient sums to zero over the classes
    assert float(grad.sum(1).abs().max()) < 1e-15


def test_kl_saturated_logits_stay_finite():
    z = torch.tensor([80.0, -80.0, 0.0]).reshape(1, 3, 1, 1).double()
    zt = torch.tensor([-80.0, 80.0, -80.0]).reshape(1, 3, 1, 1).double()
    value, grad, mag, _ = V.kl(z, zt, 1)
    assert torch.isfinite(value) and torch.isfinite(grad).all() and torch.isfinite(mag)
    assert abs(float(value) - 160.0) < 1e-9


def test_perturb_and_normalize():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 1, 5, 6, generator=g)
    assert torch.equal(V.perturb(x, torch.zeros_like(x), 10.0, 6.0), x.double())
    u = torch.rand(3, 1, 5, 6, generator=g) - 0.5
    d = V.normalize(u)
    assert float((d.reshape(3, -1).norm(dim=1) - 1).abs().max()) < 1e-7
    # perturb with gscale = xi is the normalised direction times s, for any xi
    for xi in (1.0, 10.0):
        out = V.perturb(x, u, xi, 6.0)
        assert float((out - (x.double() + 6.0 * d)).abs().max()) < 1e-6
    assert torch.allclose(V.sumsq(u), (u.double() ** 2).sum((1, 2, 3)))


@pytest.mark.parametrize("row", range(len(V.PROBES)))
def test_integer_probes_are_exact(row):
    """Every probe of tests/test_gpu_stem_dgrad.py: integer operands, every fp32 partial sum below 2^24 -- and the stem input gradient
    is the 3x3 conv of dy with the flipped kernel (tests/_conv_ref.py)."""
    _, c0, shape = V.PROBES[row]
    dy, w = V.probe_operands(c0, shape, 1000 + row)
    assert int(dy.abs().max()) <= 3 and int(w.abs().max()) <= 2
    w_nk = w.reshape(c0, 3, 3)[None]  # [n = 1][k = C0][3][3]
    ok = R.exact_ok(R.G3S1, dy, None, w_nk, flip=True)
    assert all(ok.values()), ok
    ref = V.stem_dgrad(dy, w)
    assert torch.equal(ref, R.conv_ref(R.G3S1, dy, None, w_nk, flip=True)[:, 0])
    assert torch.equal(ref, ref.round())


def test_new_prototypes_are_in_the_header():
    protos = mia_hip.parse_header()
    for name, nargs in (("mia_stem_dgrad", 9), ("mia_kl_workspace", 2), ("mia_kl_fwd", 18), ("mia_kl_bwd", 19), ("mia_vat_noise", 6),
                        ("mia_sample_sumsq_workspace", 2), ("mia_sample_sumsq", 6), ("mia_vat_perturb", 10)):
        assert name in protos, name
        assert len(protos[name][1]) == nargs, (name, len(protos[name][1]))


def test_python_surface():
    from losses import vat_loss
    from mia_hip import ops
    from training.semi import VATEngine  # noqa: F401
    assert hasattr(ops, "KLConsistencyFn") and hasattr(ops, "frozen_parameters") and hasattr(ops, "no_bn_tracking")
    m = torch.nn.Linear(2, 2)
    m.bias.requires_grad_(False)
    with pytest.raises(RuntimeError):
        with ops.frozen_parameters(m):
            assert not any(p.requires_grad for p in m.parameters())
            raise RuntimeError("leave by an exception")
    assert m.weight.requires_grad and not m.bias.requires_grad
    # the tensor-op form of the definition against the reference
    z, zt = _logits(1).float(), _logits(2).float()
    for red, den in (("mean", 3 * 35), ("batchmean", 3)):
        got = vat_loss.kl_consistency_reference(z, zt, None, red)
        assert abs(float(got) - float(V.kl(z, zt, den)[0])) < 1e-5 * max(1.0, float(V.kl(z, zt, den)[2]))
    with pytest.raises(ValueError):
        vat_loss.VATLoss(reduction="sum")
