"""CPU-side checks of dual-task consistency training (no GPU): the float64 restatement (tests/_dtc_ref.py) against float64 autograd of
the plain formula; the normalised target against the published `compute_sdf` steps written out with scipy; the condition on the
generator that the GPU test relies on (a share of pixels in the steep zone of sigmoid(-1500 t)); the tensor-op form of
`DualTaskConsistencyLoss` on CPU tensors; the parameters of `DualTaskUNet`; the engine's refusals; and the C ABI."""
import numpy as np
import pytest
import torch

import _dtc_ref as R

CASES = [((2, 1, 7), 2, 1), ((4, 9, 13), 3, 2), ((4, 12, 10), 8, 4), ((2, 6, 5), 3, 0)]


def _case(shape, k1, lb, seed=0):
    nb, h, w = shape
    z, r = R.make_case(nb, k1, h, w, seed)
    labels = R.make_labels(nb, k1, h, w, seed)
    phi = R.phi_scipy(labels[:lb], k1) if lb else None
    return z, r, labels, phi


@pytest.mark.parametrize("shape,k1,lb", CASES)
@pytest.mark.parametrize("k", [1500.0, 8.0])
def test_restatement_gradients_equal_float64_autograd(shape, k1, lb, k):
    z, r, _, phi = _case(shape, k1, lb)
    ref = R.evaluate(z, r, phi, lb, k, 0.7, 0.3)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    rt = torch.tensor(r, dtype=torch.float64, requires_grad=True)
    loss, cons, sdf = R.torch_loss(zt, rt, ref["T"], lb, k, 0.7, 0.3)
    loss.backward()
    for name, got, want in (("value", ref["value"], loss.item()), ("cons", ref["cons"], cons.item()), ("sdf", ref["sdf"], sdf.item())):
        assert abs(got - want) <= 1e-10 * max(abs(want), 1e-300), (name, got, want)
    for name, got, want in (("dz", ref["dz"], zt.grad.numpy()), ("dr", ref["dr"], rt.grad.numpy())):
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max(), (name, np.abs(got - want).max(), np.abs(want).max())
        assert (np.abs(got) <= ref[name + "_mag"] * (1 + 1e-12)).all()  # a magnitude bounds its expression
    assert np.abs(ref["dr"]).max() > 0 and np.abs(ref["dz"]).max() > 0


def test_saturated_logits_stay_finite_in_the_restatement():
    z, r = R.saturated_case(2, 3, 5, 7)
    labels = R.make_labels(2, 3, 5, 7)
    ref = R.evaluate(z, r, R.phi_scipy(labels[:1], 3), 1, 1500.0, 0.1, 0.3)
    for key in ("value", "cons", "sdf", "dz", "dr", "dz_mag", "dr_mag"):
        assert np.isfinite(ref[key]).all(), key


@pytest.mark.parametrize("shape,k1", [((4, 37, 61), 2), ((4, 37, 61), 3), ((4, 20, 24), 8), ((2, 1, 7), 3)])
def test_target_equals_the_published_compute_sdf_steps(shape, k1):
    nb, h, w = shape
    labels = R.make_labels(nb, k1, h, w)
    T = R.target(R.phi_scipy(labels, k1))
    compared = 0
    for n in range(nb):
        for c in range(1, k1):
            pub = R.published_sdf(labels[n] == c)
            if pub is None:  # the published code leaves zeros for a class that is absent
                assert not T[n, c - 1].any()
                continue
            ok = np.isfinite(pub)
            if (labels[n] == c).all():  # published: 0 / 0 nearly everywhere (scipy's edt of an all-true mask leaves a few `boundary` zeros)
                assert not ok.all() and not T[n, c - 1].any()  # here: phi = 0, so T = 0
            else:
                assert ok.all()
                compared += 1
            assert np.abs(T[n, c - 1] - pub)[ok].max(initial=0.0) <= 1e-12  # wherever the published value is finite
    assert compared > 0 or k1 == 2
    # the generator's promises: an image without class 1, an image filled by one class, a line with m_in = 0, an object on the edge
    if nb >= 4 and h > 4:
        ext = R.extents(R.phi_scipy(labels, k1))
        assert not (labels[3] == 1).any() and (labels[2] == 1).all()
        assert ext[1, min(2, k1 - 1) - 1, 1] == 0.0 and ext[1, min(2, k1 - 1) - 1, 0] > 0.0
        assert labels[0, 0, 0] == 1


def test_make_case_puts_a_share_of_pixels_in_the_steep_zone():
    for (nb, h, w) in R.SHAPES[2:]:
        for k1 in R.K1S:
            _, r = R.make_case(nb, k1, h, w)
            q, _ = R.sigmoid_parts(-R.K_PUBLISHED * np.tanh(r.astype(np.float64)))
            share = ((q > 0.01) & (q < 0.99)).mean()
            assert share >= 0.05, (nb, h, w, k1, share)
            assert ((q <= 0.01) | (q >= 0.99)).mean() >= 0.05  # and the saturated zone is there too


@pytest.mark.parametrize("shape,k1,lb", CASES)
def test_tensor_op_form_on_cpu_matches_restatement(shape, k1, lb):
    from losses.dual_task import DualTaskConsistencyLoss
    z, r, labels, phi = _case(shape, k1, lb, seed=1)
    ref = R.evaluate(z, r, phi, lb, 1500.0, 0.7, 0.3)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    rt = torch.tensor(r, dtype=torch.float64, requires_grad=True)
    mod = DualTaskConsistencyLoss(k1 - 1, fused=False)
    dyn = torch.tensor([0.7, 0.3], dtype=torch.float32)
    loss = mod(zt, rt, torch.tensor(labels), lb, dyn=dyn, phi=None if phi is None else torch.tensor(phi))
    loss.backward()
    w0, w1 = float(np.float32(0.7)), float(np.float32(0.3))
    want = w0 * ref["cons"] + w1 * ref["sdf"]
    assert abs(loss.item() - want) <= 1e-10 * abs(want)
    assert abs(mod.last_consistency.item() - ref["cons"]) <= 1e-10 * ref["cons"]
    assert abs(mod.last_sdf.item() - ref["sdf"]) <= 1e-10 * max(ref["sdf"], 1e-300)
    ref = R.evaluate(z, r, phi, lb, 1500.0, w0, w1)
    assert np.abs(zt.grad.numpy() - ref["dz"]).max() <= 1e-10 * np.abs(ref["dz"]).max()
    assert np.abs(rt.grad.numpy() - ref["dr"]).max() <= 1e-10 * np.abs(ref["dr"]).max()
    if lb == 0:
        assert mod.last_sdf.item() == 0.0


def test_tensor_op_form_takes_more_than_eight_classes_and_bf16():
    from losses.dual_task import DualTaskConsistencyLoss
    z = torch.randn(2, 10, 4, 5, dtype=torch.bfloat16, requires_grad=True)
    r = torch.randn(2, 9, 4, 5, dtype=torch.bfloat16, requires_grad=True)
    loss = DualTaskConsistencyLoss(9)(z, r, None, 0)  # fused=True falls back by itself: 10 classes, bf16
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(z.grad).all() and torch.isfinite(r.grad).all()


def test_spacing_other_than_unit_is_refused():
    from losses.dual_task import DualTaskConsistencyLoss, normalized_distance_map
    with pytest.raises(NotImplementedError):
        DualTaskConsistencyLoss(2, spacing=(1.0, 2.0))
    with pytest.raises(NotImplementedError):
        normalized_distance_map(torch.zeros(1, 4, 4, dtype=torch.long), 2, spacing=(0.5, 0.5))
    DualTaskConsistencyLoss(2, spacing=(1, 1))


def test_dual_task_unet_adds_one_head_and_shares_every_other_bit():
    from models.unet import DualTaskUNet, UNet
    for norm in ("instance", "batch"):
        torch.manual_seed(1337)
        a = UNet(2, 1, 3, [4, 8, 16], normalization=norm, dropout_prob=None)
        torch.manual_seed(1337)
        b = DualTaskUNet(2, 1, 3, [4, 8, 16], normalization=norm, dropout_prob=None)
        sa, sb = a.state_dict(), b.state_dict()
        assert set(sb) - set(sa) == {"decoder.ls_output.weight", "decoder.ls_output.bias"} and set(sa) <= set(sb)
        for key, v in sa.items():
            assert torch.equal(v, sb[key]), key
        assert tuple(sb["decoder.ls_output.weight"].shape) == (2, 4, 1, 1) and tuple(sb["decoder.ls_output.bias"].shape) == (2,)
        missing, unexpected = a.load_state_dict(sb, strict=False)
        assert not missing and sorted(unexpected) == ["decoder.ls_output.bias", "decoder.ls_output.weight"]
    with pytest.raises(ValueError):
        DualTaskUNet(2, 1, 1, [4, 8])


def test_engine_refuses_a_plain_unet_and_dtc_false_before_touching_a_device():
    from models.unet import DualTaskUNet, UNet
    from training.semi import DTCEngine
    with pytest.raises(ValueError, match="level-set head"):
        DTCEngine(UNet(2, 1, 3, [4, 8], dropout_prob=None), torch.nn.CrossEntropyLoss(), labeled_bs=1)
    with pytest.raises(ValueError, match="dtc=False"):
        DTCEngine(DualTaskUNet(2, 1, 3, [4, 8], dropout_prob=None), torch.nn.CrossEntropyLoss(), labeled_bs=1, dtc=False)


def test_header_declares_the_new_symbols_and_errors_come_back():
    import ctypes

    import mia_hip
    protos = mia_hip.parse_header()
    for name in ("mia_sdm_extent", "mia_dtc_fwd", "mia_dtc_finalize", "mia_dtc_bwd"):
        assert name in protos, name
    assert len(protos["mia_dtc_bwd"][1]) == 26 and len(protos["mia_dtc_fwd"][1]) == 18
    l = mia_hip.lib()
    i64, f32 = ctypes.c_int64, ctypes.c_float
    one = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)  # never dereferenced: every check precedes any launch
    strides = [i64(4), i64(1), i64(1)]
    for k1, nb, lb, hw, text in ((1, 1, 0, 4, b"k1=1"), (9, 1, 0, 4, b"k1=9"), (3, 1, 2, 4, b"lb=2"), (3, 2, 0, 1 << 30, b"2^31"),
                                 (3, 1, 1, 4, b"need phi")):
        rc = l.mia_dtc_fwd(one, one, None, None, nb, lb, i64(hw), k1, f32(1500.0), *strides, *strides, 1, one, None)
        assert rc < 0 and text in l.mia_last_error(), (k1, nb, lb, hw, l.mia_last_error())
        rc = l.mia_dtc_bwd(one, one, None, None, one, None, one, one, nb, lb, i64(hw), k1, f32(1500.0), *strides, *strides, *strides,
                           *strides, None)
        assert rc < 0 and text in l.mia_last_error()
    assert l.mia_sdm_extent(one, 2, i64(1 << 30), one, None) < 0 and b"2^31" in l.mia_last_error()
    assert l.mia_dtc_finalize(one, None, 1, 2, i64(4), 3, 1, one, one, None) < 0 and b"lb=2" in l.mia_last_error()
