"""Host-side tests of the feature-perturbation stream (no GPU): the tensor-op form of `ops.feature_dropout_cat` against a plain numpy
loop and under gradcheck, the mask helper, the argument checks of the new entry points, and the new arguments of `FixMatchEngine` and
`UNet.forward`."""
import ctypes

import numpy as np
import pytest
import torch

import _featdrop_ref as R
import mia_hip
from mia_hip import ops


def test_mask_helper_rows():
    m = R.make_mask(5, 6, seed=3)
    assert m.dtype == torch.float32 and tuple(m.shape) == (5, 6)
    assert not m[1].any() and (m[2] == 1).all()
    for u in (0, 3, 4):
        assert set(m[u].tolist()) == {0.0, R.SCALE}
    assert set(R.make_mask(1, 4)[0].tolist()) == {0.0, R.SCALE}
    two = R.make_mask(2, 8)
    assert set(two[0].tolist()) == {0.0, R.SCALE} and not two[1].any()


@pytest.mark.parametrize("n,h,w,c,row0,nu", [(3, 5, 7, 4, 1, 2), (4, 3, 3, 8, 1, 3), (2, 1, 1, 5, 0, 2), (3, 2, 2, 3, 2, 1)])
def test_tensor_op_form_against_a_numpy_loop(n, h, w, c, row0, nu):
    g = torch.Generator().manual_seed(n * 100 + c)
    x = torch.randn(n, h, w, c, generator=g)
    mask = R.make_mask(nu, c, seed=c)
    got = ops.feature_dropout_cat(x, mask, row0, fused=False)
    want = R.numpy_loop(x.numpy(), mask.numpy(), row0)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n + nu, h, w, c)
    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32))
    assert torch.equal(got.view(torch.int32), R.tensor_ops(x, mask, row0).view(torch.int32))
    # bf16: the product is formed in fp32 and rounded once
    xb = x.to(torch.bfloat16)
    gb = ops.feature_dropout_cat(xb, mask, row0, fused=False)
    wb = torch.from_numpy(R.numpy_loop(xb.float().numpy(), mask.numpy(), row0)).to(torch.bfloat16)
    assert gb.dtype == torch.bfloat16 and torch.equal(gb.view(torch.int16), wb.view(torch.int16))


def test_a_dropped_channel_is_a_selection_on_the_host():
    x = torch.tensor([float("inf"), float("-inf"), float("nan"), -1.0]).view(1, 1, 1, 4)
    out = ops.feature_dropout_cat(x, torch.zeros(1, 4), 0, fused=False)
    assert out[1].view(torch.int32).flatten().tolist() == [0, 0, 0, 0]  # +0.0: sign bit clear, nothing non-finite


def test_gradcheck_in_float64():
    x = torch.randn(3, 2, 2, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    mask = R.make_mask(2, 3, seed=2)
    assert torch.autograd.gradcheck(lambda t: ops.feature_dropout_cat(t, mask, 1, fused=False), (x,))


def test_wrapper_argument_errors_and_no_cpu_fallback_of_the_fused_form():
    x, mask = torch.zeros(3, 2, 2, 4), torch.ones(2, 4)
    with pytest.raises(mia_hip.MiaError):
        ops.feature_dropout_cat(x, mask, 0)  # fused: device tensors only
    for bad in (dict(row0=2), dict(row0=-1), dict(mask=torch.ones(2, 3)), dict(mask=torch.ones(2, 4, dtype=torch.float64)),
                dict(mask=torch.ones(0, 4)), dict(x=torch.zeros(3, 2, 4))):
        args = dict(x=x, mask=mask, row0=0)
        args.update(bad)
        with pytest.raises(mia_hip.MiaError):
            ops.feature_dropout_cat(args["x"], args["mask"], args["row0"], fused=False)


@pytest.mark.parametrize("name", ["mia_feat_drop_cat_fwd", "mia_feat_drop_cat_bwd"])
def test_abi_argument_checks_happen_before_any_launch(name):
    l = mia_hip.lib()
    fn = getattr(l, name)
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    p = lambda off=0: ctypes.c_void_p(base + 4 * off)
    i64 = ctypes.c_int64
    # n = 3 images of hw = 4 pixels of c = 4 channels: the [n] tensor takes 48 floats, the [n + nu] one 80; the mask sits past both
    big, small, mask = p(0), p(1024), p(2048)
    src, dst = (big, small) if name.endswith("bwd") else (small, big)
    ok = dict(dtype=mia_hip.F32, src=src, mask=mask, dst=dst, n=3, hw=i64(4), c=4, row0=1, nu=2)

    def rc(**kw):
        a = dict(ok)
        a.update(kw)
        return fn(a["dtype"], a["src"], a["mask"], a["dst"], a["n"], a["hw"], a["c"], a["row0"], a["nu"], None, None)

    for bad, word in ((dict(nu=0), b"rows"), (dict(row0=-1), b"rows"), (dict(row0=2), b"rows"), (dict(nu=4, row0=0), b"rows"),
                      (dict(c=0), b"shape"), (dict(hw=i64(0)), b"shape"), (dict(dtype=2), b"dtype"), (dict(dtype=-1), b"dtype"),
                      (dict(src=None), b"null"), (dict(mask=None), b"null"), (dict(dst=None), b"null")):
        assert rc(**bad) < 0, bad
        assert word in l.mia_last_error(), (bad, l.mia_last_error())
    # overlap: the destination starts inside the source, the source inside the destination, and the same pointer
    n_src = 80 if name.endswith("bwd") else 48
    n_dst = 48 if name.endswith("bwd") else 80
    for s, d in ((p(0), p(n_src - 1)), (p(n_dst - 1), p(0)), (p(0), p(0))):
        assert rc(src=s, dst=d) < 0 and b"overlaps" in l.mia_last_error()


def test_launch_shape_query():
    l = mia_hip.lib()
    px = ctypes.c_int(0)
    cap = l.mia_feat_drop_cat_sweep(mia_hip.F32, 4, 1, ctypes.byref(px))
    assert cap > 0 and px.value >= 1
    one = ctypes.c_int(0)
    assert l.mia_feat_drop_cat_sweep(mia_hip.F32, 4, 0, ctypes.byref(one)) == cap and one.value * 4 == px.value
    wide = ctypes.c_int(0)
    assert l.mia_feat_drop_cat_sweep(mia_hip.BF16, 1 << 20, 1, ctypes.byref(wide)) == cap and wide.value == 1
    assert l.mia_feat_drop_cat_sweep(7, 4, 1, ctypes.byref(px)) < 0 and l.mia_feat_drop_cat_sweep(mia_hip.F32, 2, 1, ctypes.byref(px)) < 0
    assert l.mia_feat_drop_cat_sweep(mia_hip.F32, 4, 1, None) < 0


def _tiny(seed=1):
    from models.unet import UNet
    torch.manual_seed(seed)
    return UNet(2, 1, 3, [4, 8], normalization="instance", dropout_prob=None)


def test_fixmatch_engine_validates_the_new_arguments():
    from training.semi import FixMatchEngine
    for kw in (dict(fp_weight=-0.1), dict(fp_weight=1.5), dict(fp_weight=float("nan")), dict(fp_drop=-0.1), dict(fp_drop=1.0),
               dict(fp_drop=float("nan"))):
        for flag in (False, True):
            with pytest.raises(ValueError, match="fp_"):
                FixMatchEngine(_tiny(), None, labeled_bs=2, feature_perturbation=flag, **kw)
    eng = FixMatchEngine(_tiny(), None, labeled_bs=2)
    assert eng.feature_perturbation is False and eng.fp_drop == 0.5 and eng.fp_weight == 0.5 and eng.last_fp is None
    eng = FixMatchEngine(_tiny(), None, labeled_bs=2, feature_perturbation=True, fp_drop=0.0, fp_weight=1.0)
    assert eng.feature_perturbation is True and eng.fp_drop == 0.0 and eng.fp_weight == 1.0


def test_unet_forward_rejects_deep_supervision_outputs_and_bad_rows_with_the_stream():
    net = _tiny()
    x = torch.zeros(2, 1, 8, 8)
    with pytest.raises(NotImplementedError):
        net(x, fp_rows=(0, 1), return_ds=True)
    for rows in ((0, 0), (-1, 1), (1, 2)):
        with pytest.raises(ValueError):
            net(x, fp_rows=rows)
