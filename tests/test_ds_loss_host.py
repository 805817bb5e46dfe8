"""CPU checks around the deep-supervision loss: the float64 restatement in tests/_ds_loss_ref.py against torch's interpolate and
autograd through the loss oracle (oracle/losses_ref.py), the default weights of losses.DeepSupervisionLoss, and every argument error
that is decided before a kernel runs.  None of it needs a GPU."""
import pytest
import torch
import torch.nn.functional as F

import _ds_loss_ref as D
import _head_loss_ref as R
from oracle import losses_ref


def nchw(t):  # [B, h, w, K] -> [B, K, h, w]
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("h,w,f", D.interp_shapes(), ids=lambda v: str(v))
def test_upsample_is_torch_interpolate(h, w, f):
    """Value and adjoint of Uy . Ux^T against F.interpolate(scale_factor=f, mode="bilinear", align_corners=False) in float64."""
    g = torch.Generator().manual_seed(h * 100 + w * 10 + f)
    z = torch.randn(2, h, w, 3, generator=g, dtype=torch.float64)
    v = nchw(z).clone().requires_grad_(True)
    ref = F.interpolate(v, scale_factor=f, mode="bilinear", align_corners=False)
    got = D.upsample(z, f)
    assert tuple(got.shape) == (2, h * f, w * f, 3)
    assert (nchw(got) - ref.detach()).abs().max().item() <= 1e-12
    du = torch.randn(2, h * f, w * f, 3, generator=g, dtype=torch.float64)
    ref.backward(nchw(du))
    adj = torch.einsum("Yy,bYXk,Xx->byxk", D.upsample_matrix(h, f), du, D.upsample_matrix(w, f))
    assert (nchw(adj) - v.grad).abs().max().item() <= 1e-12
    rows = D.upsample_matrix(h, f).sum(1)
    assert (rows - 1).abs().max().item() <= 1e-15, "every full-resolution row is a convex combination"


def test_footprint_of_a_low_resolution_pixel():
    """What the gather kernel relies on: pixel i is touched by the rows [(i - 1) f + f / 2, (i + 1) f + f / 2) only (clipped)."""
    for f in D.FACTORS:
        for n in (1, 2, 5):
            u = D.upsample_matrix(n, f)
            for i in range(n):
                rows = torch.nonzero(u[:, i]).flatten()
                assert rows.min().item() >= max(0, (i - 1) * f + f // 2) and rows.max().item() < min(n * f, (i + 1) * f + f // 2)


ONE_PER_BIT = [D.DEFAULT_FLAGS, (False, True, False, False), (True, False, False, False), (True, True, True, False),
               (True, True, False, True)]


@pytest.mark.parametrize("flags", ONE_PER_BIT, ids=lambda f: "".join("SDBQ"[j] if v else "-" for j, v in enumerate(f)))
@pytest.mark.parametrize("factor", D.FACTORS)
def test_loss_and_dz_match_autograd_through_interpolate(factor, flags):
    nb, h, w, k1 = 4, 3, 2, 3  # four images: the oracle keeps its one-hot target in fp32, where a batch mean over 4 is exact
    z, labels = D.ds_inputs(nb, h, w, factor, k1, softmax=flags[0])
    got = D.ds_dice_ce(z, labels, factor, *flags, dice_w=0.6, ce_w=0.9, gout=R.LOSS_GOUT)
    v = nchw(z.double()).clone().requires_grad_(True)
    up = F.interpolate(v, scale_factor=factor, mode="bilinear", align_corners=False)
    s, d, b, q = flags
    ref = losses_ref.dice_and_ce(up, labels, k1 - 1, 0.6, 0.9, smooth=D.SMOOTH, do_bg=d, softmax=s, batch=b, squared=q)
    (R.LOSS_GOUT * ref).backward()
    assert abs(got["out"][0].item() - ref.item()) <= 1e-10
    assert (nchw(got["dz"]) - v.grad).abs().max().item() <= 1e-10


def test_case_tables():
    cases = D.shape_cases()
    assert len(set(cases)) == len(cases)
    for f in D.FACTORS:
        mine = [c for c in cases if c[3] == f]
        assert {(h, w) for _, h, w, _, _, _ in mine} == set(D.SMALL_HW) | {D.MULTI_TILE[f]}
        assert {c[4] for c in mine} == set(D.FAST_K1 + D.GENERIC_K1)
    assert {c[0] for c in cases} == {1, 3}
    assert max(nb * h * f * w * f * 8 for nb, h, w, f, _, _ in cases) <= 1 << 20, "labels of the largest case stay under 1 MiB"
    z, labels = D.ds_inputs(3, 5, 7, 4, 3)
    z2, labels2 = D.ds_inputs(3, 5, 7, 4, 3)
    assert torch.equal(z, z2) and torch.equal(labels, labels2) and torch.equal(z.float().double(), z)
    assert labels.dtype == torch.int64 and tuple(labels.shape) == (3, 20, 28)


# ------------------------------------------------------------------ the Python layers, without a GPU
def _loss():
    from losses.compound_losses import DiceAndCELoss
    return DiceAndCELoss(dice_kwargs=dict(num_classes=2, do_bg=True))


def test_default_weights():
    from losses.deep_supervision import DeepSupervisionLoss, default_weights
    assert default_weights(3) == pytest.approx([4 / 7, 2 / 7, 1 / 7], abs=1e-15)
    assert default_weights(1) == [1.0]

    class Const(torch.nn.Module):
        def forward(self, out, target):
            return out.mean()

    ds = DeepSupervisionLoss(Const())
    outs = [torch.full((1, 3, 8, 8), v) for v in (1.0, 10.0, 100.0)]  # all at the target's resolution: handed over as they are
    total = ds(outs, torch.zeros(1, 8, 8, dtype=torch.long))
    assert total.item() == pytest.approx((4 * 1 + 2 * 10 + 1 * 100) / 7, rel=1e-6)
    assert ds.last_terms.tolist() == [1.0, 10.0, 100.0]
    assert ds(outs[1], torch.zeros(1, 8, 8, dtype=torch.long)).item() == 10.0, "a single tensor behaves like the loss itself"
    assert DeepSupervisionLoss(Const(), weights=[1, 0, 0])(outs, torch.zeros(1, 8, 8)).item() == 1.0
    with pytest.raises(ValueError, match="2 weights for 3 outputs"):
        DeepSupervisionLoss(Const(), weights=[1, 2])(outs, torch.zeros(1, 8, 8))


def test_mismatched_factors_name_the_shapes():
    from losses.deep_supervision import DeepSupervisionLoss
    ds = DeepSupervisionLoss(_loss())
    target = torch.zeros(2, 32, 32, dtype=torch.long)
    for shape in ((2, 3, 16, 8), (2, 3, 12, 12), (2, 3, 64, 64)):
        with pytest.raises(ValueError, match=r"%dx%d.*32x32" % shape[2:]):
            ds([torch.zeros(2, 3, 32, 32), torch.zeros(shape)], target)


def test_fused_true_refuses_what_the_kernel_cannot_serve():
    from losses.deep_supervision import DeepSupervisionLoss
    ds = DeepSupervisionLoss(_loss(), fused=True)
    low = torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError, match="dense"):
        ds([low], torch.zeros(2, 3, 32, 32))
    with pytest.raises(ValueError, match="factor 32"):
        ds([torch.zeros(2, 3, 1, 1)], torch.zeros(2, 32, 32, dtype=torch.long))
    with pytest.raises(ValueError, match="not a DiceAndCELoss"):
        DeepSupervisionLoss(torch.nn.CrossEntropyLoss(), fused=True)([low], torch.zeros(2, 32, 32, dtype=torch.long))


@pytest.mark.parametrize("fused", [None, False])
def test_no_cpu_fallback(fused):
    from losses.deep_supervision import DeepSupervisionLoss
    from mia_hip import MiaError
    ds = DeepSupervisionLoss(_loss(), fused=fused)
    with pytest.raises(MiaError, match="no CPU fallback"):
        ds([torch.zeros(2, 3, 8, 8)], torch.zeros(2, 32, 32, dtype=torch.long))


def test_engine_needs_auxiliary_heads():
    from models.unet import UNet
    from training.engine import TrainEngine
    plain = UNet(2, 1, 3, [4, 8, 16], normalization="instance", dropout_prob=None)
    with pytest.raises(ValueError, match="auxiliary heads"):
        TrainEngine(plain, _loss(), deep_supervision=True)
    # ds_layer = 1 builds no head either (the reference's `ds_layer > 1`)
    with pytest.raises(ValueError, match="auxiliary heads"):
        TrainEngine(UNet(2, 1, 3, [4, 8, 16], deep_supervision=True, ds_layer=1, normalization="instance", dropout_prob=None), _loss(),
                    deep_supervision=True)


def test_upsample_ds_keyword_exists_with_todays_default():
    import inspect
    from models.unet import UNet
    from models.unet.unet import UNetDecoder
    for fn in (UNet.forward, UNetDecoder.forward, UNetDecoder.forward_nhwc):
        assert inspect.signature(fn).parameters["upsample_ds"].default is True
