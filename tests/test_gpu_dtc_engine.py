"""`DualTaskUNet` and `DTCEngine` on the GPU.  The model is DualTaskUNet(2, 1, 3, [8, 16, 32], dropout_prob=None) on 4 x 1 x 32 x 48
images with labeled_bs = 2, the scale of tests/test_gpu_vat_engine.py.  Everything here is an exact property (bits) or a finiteness
check; the loss itself is held against the float64 restatement in tests/test_gpu_dtc.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LB, B, H, W = 2, 4, 32, 48
CH = [8, 16, 32]
HEAD = ("decoder.ls_output.weight", "decoder.ls_output.bias")


def _net(seed=5, dtype=torch.float32, cls=None):
    from models.unet import DualTaskUNet
    torch.manual_seed(seed)
    m = (cls or DualTaskUNet)(2, 1, 3, CH, normalization="instance", dropout_prob=None).to(DEV)
    return m.set_compute_dtype(dtype)


def _sup():
    from losses.compound_losses import DiceAndCELoss
    from losses.dice_loss import DiceLoss
    return DiceAndCELoss(dice_loss=DiceLoss, dice_kwargs=dict(num_classes=2, do_bg=True), ce_loss=torch.nn.CrossEntropyLoss, ce_kwargs={})


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 1, H, W, generator=g)
    y = torch.zeros(B, H, W, dtype=torch.long)
    y[:, 6:20, 8:30] = 1  # two objects with an inside, so the distance map has both signs
    y[:, 22:30, 20:44] = 2
    y[1, :4] = torch.randint(0, 3, (4, W), generator=g)
    return {"image": x.to(DEV), "label": y[:LB].to(DEV)}


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _engine(seed=3, dtype=torch.float32, **kw):
    from training.semi import DTCEngine
    args = dict(labeled_bs=LB, consistency_weight=0.1, beta=0.3, start_lr=1e-2, lr_warmup_iter=0, num_iters=100)
    args.update(kw)
    return DTCEngine(_net(seed, dtype=dtype), _sup(), **args)


def test_forward_equals_a_unet_with_the_shared_weights_bit_for_bit():
    from models.unet import UNet
    dual = _net().train()
    plain = _net(seed=9, cls=UNet).train()
    missing, unexpected = plain.load_state_dict(dual.state_dict(), strict=False)
    assert not missing and sorted(unexpected) == sorted(HEAD)
    x = _batch(0)["image"]
    assert torch.equal(_bits(dual(x)), _bits(plain(x)))
    z, r = dual(x, return_level_set=True)
    assert z.shape == (B, 3, H, W) and r.shape == (B, 2, H, W) and z.dtype == r.dtype == torch.float32
    assert z.requires_grad and r.requires_grad
    assert (z - dual(x)).abs().max() <= 1e-4  # the un-fused head path computes the same logits (other kernels, not the same bits)
    with pytest.raises(NotImplementedError):
        dual(x, return_ds=True, return_level_set=True)


def test_two_engines_from_one_seed_agree_after_two_steps():
    runs = []
    for _ in range(2):
        eng = _engine()
        for i in range(2):
            loss = eng.train_step(_batch(i))
            assert isinstance(loss, torch.Tensor) and loss.is_cuda and not loss.requires_grad
        assert bool(torch.isfinite(loss)) and float(eng.last_consistency) > 0.0 and float(eng.last_sdf) > 0.0
        assert bool(torch.isfinite(eng.last_supervised))
        assert all(p.grad is not None for p in eng.model.parameters())
        assert eng.current_iter == 2 and float(eng.dyn[0]) == pytest.approx(0.1) and float(eng.dyn[1]) == pytest.approx(0.3)
        runs.append((eng.optimizer.flat_param.clone(), loss.clone()))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))


def test_the_level_set_head_learns_and_ramps_are_followed():
    class Ramp:
        def step(self, i):
            return 0.05 * (i + 1)

    eng = _engine(consistency_weight=Ramp())
    before = {k: v.clone() for k, v in eng.model.state_dict().items() if k in HEAD}
    eng.train_step(_batch(0))
    assert float(eng.dyn[0]) == pytest.approx(0.05)
    eng.train_step(_batch(1))
    assert float(eng.dyn[0]) == pytest.approx(0.10)
    after = eng.model.state_dict()
    assert all(not torch.equal(before[k], after[k]) for k in HEAD)


def test_zero_weights_step_like_a_supervised_step_and_leave_the_head_alone():
    """consistency_weight = beta = 0: both gradients of the term are exact zeros, so the shared parameters take the step of a
    supervised `SemiEngine` on the same forward (every image through the un-fused head path, the loss on the labelled ones), and
    the level-set head, whose gradient is zero, does not move under Adam."""
    from training.semi import SemiEngine

    class Supervised(SemiEngine):
        def __init__(self, model, sup, **kw):
            super().__init__(model, LB, 10.0, None, "adam", None, kw["start_lr"], kw["num_iters"], kw["lr_warmup_iter"], 1, "poly")
            self.sup = sup

        def _loss(self, image, label):
            z, _ = self.model(image, return_level_set=True)
            return self.sup(z[:LB], label[:LB])

    kw = dict(start_lr=1e-2, lr_warmup_iter=0, num_iters=100)
    eng = _engine(consistency_weight=0.0, beta=0.0)
    ref = Supervised(_net(3), _sup(), **kw)
    head0 = {k: v.clone() for k, v in eng.model.state_dict().items() if k in HEAD}
    for i in range(2):
        a, b = eng.train_step(_batch(i)), ref.train_step(_batch(i))
        assert torch.equal(_bits(a), _bits(b))  # sup + 0 * L_cons + 0 * L_sdf
    sa, sb = eng.model.state_dict(), ref.model.state_dict()
    for k in sa:
        assert torch.equal(_bits(sa[k]), _bits(sb[k])), k
    assert all(torch.equal(_bits(head0[k]), _bits(sa[k])) for k in HEAD)
    assert float(eng.last_consistency) > 0.0 and float(eng.last_sdf) > 0.0  # the by-products are unweighted


def test_checkpoint_round_trip_restores_the_level_set_head(tmp_path):
    eng = _engine()
    for i in range(2):
        eng.train_step(_batch(i))
    eng.save_state_dict(tmp_path, save_training_state=True)
    assert (tmp_path / "model.pth").is_file()
    other = _engine(seed=11)
    assert not torch.equal(other.optimizer.flat_param, eng.optimizer.flat_param)
    other.load_state_dict(tmp_path)
    sa, sb = eng.model.state_dict(), other.model.state_dict()
    for k in HEAD:
        assert torch.equal(_bits(sa[k]), _bits(sb[k])), k
    assert torch.equal(_bits(other.optimizer.flat_param), _bits(eng.optimizer.flat_param))
    x = _batch(60)["image"]
    assert torch.equal(eng.predict(x), other.predict(x))
    eng.train_step(_batch(2))  # and training goes on after a prediction
    assert eng.model.training and eng.current_iter == 3


def test_a_plain_unet_and_dtc_false_are_refused():
    from models.unet import UNet
    from training.semi import DTCEngine
    with pytest.raises(ValueError, match="level-set head"):
        DTCEngine(_net(cls=UNet), _sup(), labeled_bs=LB)
    with pytest.raises(ValueError, match="dtc=False"):
        DTCEngine(_net(), _sup(), labeled_bs=LB, dtc=False)
    eng = _engine()
    bad = _batch(0)
    bad["image"] = bad["image"][:, :, :, :, None]
    with pytest.raises(NotImplementedError):
        eng.train_step(bad)


def test_bf16_step_is_finite_and_deterministic():
    runs = []
    for _ in range(2):
        eng = _engine(dtype=torch.bfloat16)
        loss = eng.train_step(_batch(0))
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(eng.last_consistency)) and bool(torch.isfinite(eng.last_sdf))
        assert bool(torch.isfinite(eng.optimizer.flat_param).all())
        runs.append(eng.optimizer.flat_param.clone())
    assert torch.equal(_bits(runs[0]), _bits(runs[1]))
