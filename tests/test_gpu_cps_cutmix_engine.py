"""training/semi.py: `CPSEngine(cutmix=True)` on the GPU, on two tiny nets -- UNet(2, 1, 3, [4, 8, 16], instance norm), 2 labelled
and 3 unlabelled images of 32 x 32: reproducibility, the rows of the one network input, and the cross term recomposed from the step's
by-products with the float64 restatement (tests/_w2s_ref.py) within the bounds of tests/test_gpu_w2s.py."""
import numpy as np
import pytest
import torch

import _w2s_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LB, NU, HW = 2, 3, 32
LR = dict(start_lr=1e-2, lr_warmup_iter=0, num_iters=100)
TAU, WEIGHT = 0.4, 0.5


def _net(seed):
    from models.unet import UNet
    torch.manual_seed(seed)
    return UNet(2, 1, 3, [4, 8, 16], normalization="instance", dropout_prob=None).to(DEV)


def _sup():
    from losses.compound_losses import DiceAndCELoss
    from losses.dice_loss import DiceLoss
    return DiceAndCELoss(dice_loss=DiceLoss, dice_kwargs=dict(num_classes=2, do_bg=True), ce_loss=torch.nn.CrossEntropyLoss, ce_kwargs={})


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    return {"image": torch.rand(LB + NU, 1, HW, HW, generator=g).to(DEV), "label": torch.randint(0, 3, (LB, HW, HW), generator=g).to(DEV)}


def _engine(seed=3, **kw):
    from training.semi import CPSEngine
    args = dict(labeled_bs=LB, cps_weight=WEIGHT, confidence_threshold=TAU, cutmix=True, **LR)
    args.update(kw)
    return CPSEngine(_net(seed), _net(seed + 100), _sup(), **args)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def test_same_seed_same_bits_and_both_networks_move():
    runs = []
    for _ in range(2):
        eng = _engine()
        start = eng.optimizer.flat_param.clone(), eng.optimizer_b.flat_param.clone()
        torch.manual_seed(5)
        losses = [eng.train_step(_batch(i)).clone() for i in range(3)]
        assert not torch.equal(start[0], eng.optimizer.flat_param) and not torch.equal(start[1], eng.optimizer_b.flat_param)
        runs.append((torch.stack(losses), eng.optimizer.flat_param.clone(), eng.optimizer_b.flat_param.clone(), eng.last_net_in.clone()))
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.isfinite(runs[0][0]).all() and torch.isfinite(runs[0][1]).all() and torch.isfinite(runs[0][2]).all()


def test_cross_term_recomposed_from_the_by_products():
    """The unweighted `last_cps` and the loss against the float64 restatement on `last_net_in`, `last_mask`, `last_perm` and fresh
    no-grad forwards of two networks with the engine's initial weights: network A learns from B's codes and the other way round."""
    batch = _batch(0)
    eng = _engine()
    torch.manual_seed(11)
    loss = eng.train_step(batch)
    image = batch["image"]
    mask, perm = eng.last_mask.cpu().numpy(), eng.last_perm.cpu().numpy()
    assert mask.dtype == np.uint8 and mask.shape == (NU, HW, HW) and sorted(perm.tolist()) == list(range(NU))
    assert all(m.any() and not m.all() for m in mask)  # cutmix_prob = 1 by default: every image has a box
    m4 = torch.tensor(mask != 0)[:, None].to(DEV)
    assert torch.equal(_bits(eng.last_net_in[:LB]), _bits(image[:LB]))
    assert torch.equal(_bits(eng.last_net_in[LB:]), _bits(torch.where(m4, image[LB:][torch.tensor(perm).to(DEV).long()], image[LB:])))
    tau = float(np.float32(TAU))
    nets = _net(3), _net(103)
    z, out, codes = [], [], []
    for net in nets:
        net.train()
        with torch.no_grad():
            z.append(net(image[LB:]).float().cpu().numpy())
            out.append(net(eng.last_net_in)[LB:].float().cpu().numpy())
        amb = R.ambiguous(z[-1], tau)
        assert amb.mean() <= 5e-4
        codes.append((R.code_of(z[-1], tau), amb))
    kept = eng.last_confident.cpu().numpy()
    got = [c.cpu().numpy() for c in eng.last_codes]
    for k, g, (code, amb) in zip(kept, got, codes):  # the device's codes: EXACTLY the restatement's outside ambiguous pixels
        assert np.array_equal(g[~amb], code[~amb]) and int(k) == int((g >> 7).sum()) and 0 < int(k) < NU * HW * HW
    ra = R.evaluate(out[0], got[1], mask, perm, WEIGHT)  # A learns from B
    rb = R.evaluate(out[1], got[0], mask, perm, WEIGHT)
    cps, mag = ra["ce"] + rb["ce"], ra["ce_mag"] + rb["ce_mag"]
    err = abs(float(eng.last_cps) - cps)
    print(f"last_cps {float(eng.last_cps):.6f} restatement {cps:.6f} err/bound {err / (2e-6 * mag):.3f}")
    assert err <= 2e-6 * mag and cps > 0
    assert eng.last_agree is None
    sup = float(eng.last_supervised)
    # loss = sup + w LA + w LB: the restatement's bound on the cross terms plus the fp32 roundings of the two additions
    assert abs(float(loss) - (sup + WEIGHT * cps)) <= 2e-6 * WEIGHT * mag + 3 * 2.0 ** -24 * abs(float(loss))


def test_plain_form_is_untouched_and_argument_errors():
    from training.semi import CPSEngine
    plain = _engine(cutmix=False)
    torch.manual_seed(1)
    state = torch.random.get_rng_state()
    loss = plain.train_step(_batch(0))
    assert torch.isfinite(loss).item() and plain.last_agree is not None and plain.last_mask is None
    assert torch.equal(state, torch.random.get_rng_state())  # no box and no permutation is drawn
    with pytest.raises(ValueError):
        _engine(cps_on_labeled=True)
    with pytest.raises(ValueError):
        _engine(cutmix_prob=-0.1)
    only = _engine()
    g = torch.Generator().manual_seed(0)
    loss = only.train_step({"image": torch.rand(LB, 1, HW, HW, generator=g).to(DEV), "label": torch.randint(0, 3, (LB, HW, HW), generator=g).to(DEV)})
    assert torch.isfinite(loss).item() and only.last_mask is None  # no unlabelled image: the supervised terms alone
