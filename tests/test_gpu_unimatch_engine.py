"""training/semi.py: `FixMatchEngine(feature_perturbation=True)`, UniMatch's three unlabelled streams, on the GPU -- the tiny setup
of tests/test_gpu_fixmatch_engine.py: UNet(2, 1, 3, [8, 16], instance norm, no dropout), 2 labelled and 3 unlabelled images of 32 x
32, tau = 0.4.  One model call per step with the weak rows inside it, reproducibility, the composition of the loss, the
feature-perturbation term recomposed with the float64 restatement (tests/_w2s_ref.py) from the logits the step saw, and the flag-off
step unchanged."""
import numpy as np
import pytest
import torch

import _w2s_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LB, NU, HW = 2, 3, 32
OPT = dict(start_lr=1e-2, lr_warmup_iter=0, num_iters=100)
TAU = 0.4


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


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    return {"image": torch.rand(LB + NU, 1, HW, HW, generator=g).to(DEV), "label": torch.randint(0, 3, (LB, HW, HW), generator=g).to(DEV)}


def _engine(seed=3, **kw):
    from training.semi import FixMatchEngine
    args = dict(labeled_bs=LB, u_weight=0.5, confidence_threshold=TAU, dice_weight=0.5, feature_perturbation=True, **OPT)
    args.update(kw)
    return FixMatchEngine(_net(seed), _sup(), **args)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


class _Spy(torch.nn.Module):
    """Records the inputs a network is called with, its keyword arguments and what it returned."""

    def __init__(self, net):
        super().__init__()
        self.net, self.seen, self.kwargs, self.outs = net, [], [], []

    def forward(self, x, *a, **k):
        self.seen.append(x.detach().clone())
        self.kwargs.append(dict(k))
        out = self.net(x, *a, **k)
        self.outs.append(out.detach().clone())
        return out


@pytest.mark.parametrize("views", [1, 2])
def test_two_steps_with_one_model_call_each(views):
    eng = _engine(strong_views=views, strong_transform=_strong())
    eng.model = spy = _Spy(eng.model)
    start = eng.optimizer.flat_param.clone()
    torch.manual_seed(7)
    for i in range(2):
        before = eng.optimizer.flat_param.clone()
        loss = eng.train_step(_batch(i))
        assert torch.isfinite(loss).item() and not torch.equal(eng.optimizer.flat_param, before)
    assert torch.isfinite(eng.optimizer.flat_param).all() and not torch.equal(eng.optimizer.flat_param, start)
    rows = LB + NU + views * NU
    assert eng.current_iter == 2 and len(spy.seen) == 2  # ONE model call per step: no separate weak pass
    for x, k, out in zip(spy.seen, spy.kwargs, spy.outs):
        assert tuple(x.shape) == (rows, 1, HW, HW) and tuple(k["fp_rows"]) == (LB, NU) and k["fp_drop"] == 0.5
        assert tuple(out.shape) == (rows + NU, 3, HW, HW)
    image = _batch(1)["image"]
    assert torch.equal(_bits(spy.seen[1][:LB + NU]), _bits(image))  # the labelled rows, then the weak view as it is
    assert torch.equal(_bits(spy.seen[1]), _bits(eng.last_net_in))
    assert len(eng.last_masks) == len(eng.last_perms) == views
    assert 0 < int(eng.last_kept) <= NU * HW * HW and eng.last_code.dtype == torch.uint8 and tuple(eng.last_code.shape) == (NU, HW, HW)
    for t in (eng.last_supervised, eng.last_unsup, eng.last_fp):
        assert torch.isfinite(t).item()
    assert eng.last_fp.item() > 0 and eng.last_unsup.item() > eng.last_fp.item()
    assert torch.equal(_bits(loss), _bits(eng.last_supervised + eng.last_unsup))


@pytest.mark.parametrize("views", [1, 2])
def test_same_seed_same_bits(views):
    runs = []
    for _ in range(2):
        eng = _engine(strong_views=views, strong_transform=_strong())
        torch.manual_seed(5)
        losses = [eng.train_step(_batch(i)).clone() for i in range(3)]
        runs.append((torch.stack(losses), eng.optimizer.flat_param.clone(), eng.last_net_in.clone(), eng.last_code.clone(),
                     eng.last_fp.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a if a.dtype == torch.uint8 else _bits(a), b if b.dtype == torch.uint8 else _bits(b))
    assert torch.isfinite(runs[0][0]).all()


@pytest.mark.parametrize("views", [1, 2])
def test_the_weights_of_the_streams(views):
    batch = _batch(0)
    eng = _engine(strong_views=views, fp_weight=0.0)
    torch.manual_seed(2)
    loss = eng.train_step(batch)
    assert eng.last_fp.item() == 0.0 and eng.last_unsup.item() > 0
    assert torch.equal(_bits(loss), _bits(eng.last_supervised + eng.last_unsup))
    eng = _engine(strong_views=views, fp_weight=1.0)
    torch.manual_seed(2)
    loss = eng.train_step(batch)
    assert eng.last_fp.item() > 0 and torch.equal(_bits(eng.last_unsup), _bits(eng.last_fp))
    assert torch.equal(_bits(loss), _bits(eng.last_supervised + eng.last_unsup))


@pytest.mark.parametrize("views", [1, 2])
def test_feature_perturbation_term_recomposed_from_the_logits_the_step_saw(views):
    """`last_fp` against the float64 restatement on the perturbed rows' logits with the code of the weak rows' logits, both as the
    one forward returned them: the codes EXACTLY outside ambiguous pixels, the value within 2e-6 of the term's magnitude (the bound
    of tests/test_gpu_fixmatch_engine.py for the same recomposition)."""
    fp_weight = 0.5
    eng = _engine(strong_views=views, strong_transform=_strong(), cutmix_prob=1.0, fp_weight=fp_weight)
    eng.model = spy = _Spy(eng.model)
    torch.manual_seed(11)
    eng.train_step(_batch(0))
    assert len(spy.outs) == 1
    out = spy.outs[0].float().cpu().numpy()
    rows = LB + NU + views * NU
    zw, zp = out[LB:LB + NU], out[rows:rows + NU]
    tau = float(np.float32(TAU))
    got = eng.last_code.cpu().numpy()
    amb = R.ambiguous(zw, tau)
    assert amb.mean() <= 5e-4 and np.array_equal(got[~amb], R.code_of(zw, tau)[~amb])
    assert int(eng.last_kept) == int((got >> 7).sum()) and 0 < int(eng.last_kept) < NU * HW * HW
    assert not np.array_equal(zp, zw)  # the perturbed rows are not the weak rows
    ref = R.evaluate(zp, got, None, None, 0.5, 1.0, 0.5)
    value, mag = fp_weight * ref["value"], fp_weight * ref["value_mag"]
    err = abs(float(eng.last_fp) - value)
    print(f"views={views}: last_fp {float(eng.last_fp):.6f} restatement {value:.6f} err/bound {err / (2e-6 * mag):.3f}")
    assert err <= 2e-6 * mag and value > 0
    # and the whole unlabelled term from its parts
    strong = mags = 0.0
    for v in range(views):
        sl = slice(LB + NU + v * NU, LB + NU + (v + 1) * NU)
        r = R.evaluate(out[sl], got, eng.last_masks[v].cpu().numpy(), eng.last_perms[v].cpu().numpy(), 0.5, 1.0, 0.5)
        strong += r["value"] / views
        mags += r["value_mag"] / views
    whole, whole_mag = (1 - fp_weight) * strong + value, (1 - fp_weight) * mags + mag
    assert abs(float(eng.last_unsup) - whole) <= 2e-6 * whole_mag


def test_flag_off_is_the_old_step():
    eng = _engine(feature_perturbation=False, strong_views=2, strong_transform=_strong())
    eng.model = spy = _Spy(eng.model)
    torch.manual_seed(7)
    eng.train_step(_batch(0))
    assert len(spy.seen) == 2 and eng.last_fp is None  # the weak pass and ONE student forward
    assert tuple(spy.seen[0].shape) == (NU, 1, HW, HW) and tuple(spy.seen[1].shape) == (LB + 2 * NU, 1, HW, HW)
    assert spy.kwargs == [{}, {}]
    assert tuple(spy.outs[1].shape) == (LB + 2 * NU, 3, HW, HW)


def test_supervised_only_paths_do_not_use_the_stream():
    only = _engine(loss=False)
    only.model = spy = _Spy(only.model)
    loss = only.train_step(_batch(0))
    assert torch.isfinite(loss).item() and only.last_unsup is None and only.last_fp is None and spy.kwargs == [{}]
