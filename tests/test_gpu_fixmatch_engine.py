"""training/semi.py: `FixMatchEngine` on the GPU, on a tiny net -- UNet(2, 1, 3, [8, 16], instance norm, no dropout), 2 labelled and 3
unlabelled images of 32 x 32: steps with one and two strong views, reproducibility, the unsupervised term recomposed from the step's
by-products with the float64 restatement (tests/_w2s_ref.py) within the bounds of tests/test_gpu_w2s.py, the plain cross-entropy
case, the checkpoint, and the shape and rank errors."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _w2s_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LB, NU, HW = 2, 3, 32
OPT = dict(start_lr=1e-2, lr_warmup_iter=0, num_iters=100)
TAU = 0.4  # a freshly initialised three-class net is not confident: a low threshold keeps a fair share of the pixels


def _net(seed):
    from models.unet import UNet
    torch.manual_seed(seed)
    return UNet(2, 1, 3, [8, 16], normalization="instance", dropout_prob=None).to(DEV)


def _sup():
    from losses.compound_losses import DiceAndCELoss
    from losses.dice_loss import DiceLoss
    return DiceAndCELoss(dice_loss=DiceLoss, dice_kwargs=dict(num_classes=2, do_bg=True), ce_loss=torch.nn.CrossEntropyLoss, ce_kwargs={})


def _strong():
    from transforms.gpu_pipeline import BatchedAugment, strong_intensity_transforms
    return BatchedAugment(strong_intensity_transforms())


def _batch(seed, nu=NU):
    g = torch.Generator().manual_seed(seed)
    return {"image": torch.rand(LB + nu, 1, HW, HW, generator=g).to(DEV), "label": torch.randint(0, 3, (LB, HW, HW), generator=g).to(DEV)}


def _engine(seed=3, **kw):
    from training.semi import FixMatchEngine
    args = dict(labeled_bs=LB, u_weight=0.5, confidence_threshold=TAU, dice_weight=0.5, **OPT)
    args.update(kw)
    return FixMatchEngine(_net(seed), _sup(), **args)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


class _Spy(torch.nn.Module):
    """Records the inputs a network is called with."""

    def __init__(self, net):
        super().__init__()
        self.net, self.seen = net, []

    def forward(self, x, *a, **k):
        self.seen.append(x.detach().clone())
        return self.net(x, *a, **k)


@pytest.mark.parametrize("views", [1, 2])
def test_two_steps_give_finite_losses_and_move_the_parameters(views):
    eng = _engine(strong_views=views, strong_transform=_strong())
    eng.model = spy = _Spy(eng.model)
    start = eng.optimizer.flat_param.clone()
    torch.manual_seed(7)
    for i in range(2):
        before = eng.optimizer.flat_param.clone()
        loss = eng.train_step(_batch(i))
        assert torch.isfinite(loss).item() and not torch.equal(eng.optimizer.flat_param, before)
    assert torch.isfinite(eng.optimizer.flat_param).all() and not torch.equal(eng.optimizer.flat_param, start)
    assert eng.current_iter == 2 and len(spy.seen) == 4  # per step the weak pass and ONE student forward
    assert tuple(spy.seen[2].shape) == (NU, 1, HW, HW) and tuple(spy.seen[3].shape) == (LB + views * NU, 1, HW, HW)
    image = _batch(1)["image"]
    assert torch.equal(_bits(spy.seen[2]), _bits(image[LB:])) and torch.equal(_bits(spy.seen[3][:LB]), _bits(image[:LB]))
    assert torch.equal(_bits(spy.seen[3]), _bits(eng.last_net_in))
    assert len(eng.last_masks) == len(eng.last_perms) == views
    for m, p in zip(eng.last_masks, eng.last_perms):
        assert m.dtype == torch.uint8 and tuple(m.shape) == (NU, HW, HW) and sorted(p.tolist()) == list(range(NU))
    assert 0 < int(eng.last_kept) <= NU * HW * HW and eng.last_code.dtype == torch.uint8
    assert torch.isfinite(eng.last_supervised).item() and torch.isfinite(eng.last_unsup).item() and eng.last_unsup.item() > 0
    assert torch.equal(_bits(loss), _bits(eng.last_supervised + eng.last_unsup))
    if views == 2:  # the two views have their own draws
        assert not torch.equal(eng.last_net_in[LB:LB + NU], eng.last_net_in[LB + NU:])


@pytest.mark.parametrize("views", [1, 2])
def test_same_seed_same_bits(views):
    runs = []
    for _ in range(2):
        eng = _engine(strong_views=views, strong_transform=_strong())
        torch.manual_seed(5)
        losses = [eng.train_step(_batch(i)).clone() for i in range(3)]
        runs.append((torch.stack(losses), eng.optimizer.flat_param.clone(), eng.last_net_in.clone(), eng.last_code.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a if a.dtype == torch.uint8 else _bits(a), b if b.dtype == torch.uint8 else _bits(b))
    assert torch.isfinite(runs[0][0]).all()


@pytest.mark.parametrize("views", [1, 2])
def test_unsupervised_term_recomposed_from_the_by_products(views):
    """`last_unsup` against the float64 restatement on `last_net_in`, `last_masks`, `last_perms` and a fresh no-grad weak forward of
    a network with the engine's initial weights: the codes EXACTLY outside ambiguous pixels, the value within 2e-6 of the mean of
    the views' magnitudes."""
    batch = _batch(0)
    eng = _engine(strong_views=views, strong_transform=_strong(), cutmix_prob=1.0)
    torch.manual_seed(11)
    eng.train_step(batch)
    fresh = _net(3)
    fresh.train()
    with torch.no_grad():
        zw = fresh(batch["image"][LB:]).float().cpu().numpy()
        out = fresh(eng.last_net_in).float().cpu().numpy()
    tau = float(np.float32(TAU))
    got = eng.last_code.cpu().numpy()
    amb = R.ambiguous(zw, tau)
    assert amb.mean() <= 5e-4 and np.array_equal(got[~amb], R.code_of(zw, tau)[~amb])
    assert int(eng.last_kept) == int((got >> 7).sum()) and 0 < int(eng.last_kept) < NU * HW * HW
    value = mag = 0.0
    for v in range(views):
        mask, perm = eng.last_masks[v].cpu().numpy(), eng.last_perms[v].cpu().numpy()
        assert mask.any() and not mask.all()  # cutmix_prob = 1: every image has a box
        rows = slice(LB + v * NU, LB + (v + 1) * NU)
        m4 = torch.tensor(mask != 0)[:, None].to(DEV)
        unmixed = torch.where(m4, torch.zeros_like(eng.last_net_in[rows]), eng.last_net_in[rows])
        assert unmixed.abs().sum().item() > 0  # and pixels outside it
        ref = R.evaluate(out[rows], got, mask, perm, 0.5, 1.0, 0.5)
        value += ref["value"] / views
        mag += ref["value_mag"] / views
    err = abs(float(eng.last_unsup) - value)
    print(f"views={views}: last_unsup {float(eng.last_unsup):.6f} restatement {value:.6f} err/bound {err / (2e-6 * mag):.3f}")
    assert err <= 2e-6 * mag and value > 0


def test_without_cutmix_and_strong_transform_at_tau_zero_it_is_cross_entropy_on_the_weak_argmax():
    batch = _batch(2)
    eng = _engine(cutmix_prob=0.0, strong_transform=None, confidence_threshold=0.0, u_weight=1.0, dice_weight=0.0)
    eng.train_step(batch)
    assert not eng.last_masks[0].any() and int(eng.last_kept) == NU * HW * HW
    assert torch.equal(_bits(eng.last_net_in), _bits(batch["image"]))  # no box, identity transform: the batch itself
    fresh = _net(3)
    fresh.train()
    with torch.no_grad():
        zw = fresh(batch["image"][LB:]).float()
        out = fresh(batch["image"])[LB:].float()
    want = F.cross_entropy(out.double(), zw.argmax(1)).item()
    ref = R.evaluate(out.cpu().numpy(), R.code_of(zw.cpu().numpy(), 0.0))
    assert abs(ref["value"] - want) <= 1e-12 * want
    assert abs(float(eng.last_unsup) - want) <= 2e-6 * ref["ce_mag"]


def test_supervised_only_paths_and_schedules():
    class Ramp:
        def step(self, i):
            return 0.1 * (i + 1)

    eng = _engine(u_weight=Ramp(), confidence_threshold=Ramp())
    eng.train_step(_batch(0))
    eng.train_step(_batch(1))
    assert eng.dyn.tolist() == [np.float32(0.2).item(), np.float32(0.2).item()]
    only = _engine(loss=False)
    loss = only.train_step(_batch(0))
    assert torch.isfinite(loss).item() and only.last_unsup is None and torch.equal(_bits(loss), _bits(only.last_supervised))
    none = _engine()
    loss = none.train_step(_batch(0, nu=0))  # no unlabelled image
    assert torch.isfinite(loss).item() and none.last_unsup is None


def test_checkpoint_round_trip(tmp_path):
    eng = _engine(strong_views=2)
    torch.manual_seed(1)
    for i in range(2):
        eng.train_step(_batch(i))
    eng.save_state_dict(tmp_path, save_training_state=True)
    assert (tmp_path / "model.pth").is_file()
    other = _engine(seed=11, strong_views=2)
    assert not torch.equal(other.optimizer.flat_param, eng.optimizer.flat_param)
    other.load_state_dict(tmp_path)
    assert torch.equal(_bits(other.optimizer.flat_param), _bits(eng.optimizer.flat_param))
    x = _batch(60)["image"]
    assert torch.equal(eng.predict(x), other.predict(x))
    eng.train_step(_batch(2))  # and training goes on after a prediction
    assert eng.model.training and eng.current_iter == 3


def test_shape_rank_and_argument_errors(monkeypatch):
    import torch.distributed as dist
    from training.semi import FixMatchEngine
    eng = _engine()
    with pytest.raises(NotImplementedError):
        eng.train_step({"image": torch.rand(5, 1, 8, HW, HW), "label": torch.zeros(2, 8, HW, HW, dtype=torch.long)})  # 3-D
    with pytest.raises(ValueError):
        eng.train_step({"image": torch.rand(5, 1, HW, HW), "label": torch.zeros(1, HW, HW, dtype=torch.long)})  # fewer labels than lb
    with pytest.raises(ValueError):
        _engine(strong_views=0)
    with pytest.raises(ValueError):
        _engine(cutmix_prob=1.5)
    with pytest.raises(ValueError):
        _engine(labeled_bs=0)
    from transforms.gpu_pipeline import BatchedAugment, strong_intensity_transforms
    with pytest.raises(ValueError):
        _engine(strong_transform=BatchedAugment(strong_intensity_transforms(), inplace=True))
    resized = _engine(strong_transform=BatchedAugment(strong_intensity_transforms(), image_size=16))
    with pytest.raises(ValueError):
        resized.train_step(_batch(0))
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError):
        FixMatchEngine(_net(3), _sup(), labeled_bs=LB)
