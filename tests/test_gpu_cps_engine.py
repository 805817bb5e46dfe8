"""training/semi.py CPSEngine on the GPU: the cross-pseudo-supervision step on two tiny nets, UNet(2, 1, 3, [4, 8, 16], instance norm),
B = 4 with 2 labelled images of 32 x 32, Dice + CE as the supervised loss.  Two networks receive gradients from ONE backward here:
the first two tests are the ones that notice a producer -> consumer hint or a gradient-destination claim (mia_hip/ops.py) clobbered
by the peer's forward or backward."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mia_hip import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LB, B, HW = 2, 4, 32
SEED_A, SEED_B = 3, 103
LR = dict(start_lr=1e-2, lr_warmup_iter=0, num_iters=100)


def _net(seed, dropout=None):
    from models.unet import UNet
    torch.manual_seed(seed)
    return UNet(2, 1, 3, [4, 8, 16], normalization="instance", dropout_prob=dropout).to(DEV)


def _sup():
    from losses.compound_losses import DiceAndCELoss
    from losses.dice_loss import DiceLoss
    return DiceAndCELoss(dice_loss=DiceLoss, dice_kwargs=dict(num_classes=2, do_bg=True), ce_loss=torch.nn.CrossEntropyLoss, ce_kwargs={})


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    return {"image": torch.rand(B, 1, HW, HW, generator=g).to(DEV), "label": torch.randint(0, 3, (LB, HW, HW), generator=g).to(DEV)}


def _engine(seed=SEED_A, dropout=None, **kw):
    from training.semi import CPSEngine
    args = dict(labeled_bs=LB, cps_weight=0.5, **LR)
    args.update(kw)
    eng = CPSEngine(_net(seed, dropout), _net(seed + 100, dropout), _sup(), **args)
    torch.manual_seed(seed + 7)  # the Dropout2d masks
    return eng


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _hand_step(seed, batch, peer_labels=None, weight=0.0, double=False, step=False):
    """One hand-assembled step of ONE network alone (a FlatOptimizer of its own, the engine's schedule): the supervised term, plus
    `weight` x cross-entropy against fixed index labels `peer_labels` on the unlabelled images, in fp32 or in fp64.
    Returns (optimizer, {name: gradient})."""
    from scheduler.lr_scheduler import PolyLRScheduler
    from training.engine import FlatOptimizer
    model = _net(seed)
    opt = FlatOptimizer(model, "adam")
    PolyLRScheduler(opt, initial_lr=LR["start_lr"], max_steps=LR["num_iters"], warmup_steps=LR["lr_warmup_iter"], interval=1).step(0)
    model.train()
    out = model(batch["image"])
    loss = _sup()(out[:LB], batch["label"][:LB])
    if peer_labels is not None:
        z = out[LB:]
        loss = loss.double() + weight * F.cross_entropy(z.double(), peer_labels) if double else loss + weight * F.cross_entropy(z, peer_labels)
    opt.zero_grad()
    loss.backward(torch.ones_like(loss))
    names = {id(p): n for n, p in model.named_parameters()}
    grads = {names[id(p)]: opt.flat_grad[o:o + p.numel()].clone() for p, o in zip(opt.params, opt.offsets)}
    if step:
        opt.step(max_grad_norm=10.0)
    return opt, grads


def _train_logits(seed, image):
    """The logits network `seed` makes in the engine's own forward (train mode, autograd on)."""
    net = _net(seed)
    net.train()
    return net(image).detach().clone()


def test_weight_zero_leaves_each_network_its_own_supervised_step():
    batch = _batch(0)
    eng = _engine(cps_weight=0.0)
    loss = eng.train_step(batch)
    assert torch.isfinite(loss).item() and eng.last_cps.item() > 0  # the term ran, with weight 0
    for seed, opt in ((SEED_A, eng.optimizer), (SEED_B, eng.optimizer_b)):
        alone, _ = _hand_step(seed, batch, step=True)
        assert alone.flat_grad.abs().max().item() > 0
        assert torch.equal(_bits(opt.flat_grad), _bits(alone.flat_grad)), f"network {seed}: gradient bits differ from the step alone"
        assert torch.equal(_bits(opt.flat_param), _bits(alone.flat_param)), f"network {seed}: parameter bits differ from the step alone"
        assert opt.step_count == 1


def test_step_gradients_against_the_hand_assembled_steps():
    """cps_weight = 0.5, tau = 0, no dropout.  Each network's gradients against a hand-assembled step of that network alone, in which
    the peer's pseudo-labels are fixed index labels and the term is F.cross_entropy in fp32.  Tolerance: 10 x the largest per-tensor
    difference between that hand step in fp32 and in fp64 -- a noise floor taken from the reference side, computed here each run (the
    rule of test_step_gradient_against_the_hand_assembled_step in tests/test_gpu_mean_teacher.py).
    Measured on an MI355X: network A floor 1.5e-8 (tolerance 1.5e-7) beside a largest gradient of 0.10, the engine's step differs from
    the fp32 hand step by 1.5e-8; network B floor 8.8e-9 (tolerance 8.8e-8), largest gradient 0.16, difference 1.5e-8."""
    batch, weight = _batch(0), 0.5
    eng = _engine(cps_weight=weight)
    eng.train_step(batch)
    assert eng.last_cps.item() > 0
    labels = {SEED_A: _train_logits(SEED_B, batch["image"])[LB:].argmax(1), SEED_B: _train_logits(SEED_A, batch["image"])[LB:].argmax(1)}
    ya, yb, _, _ = ops.cps_decode(ops.CrossPseudoFn.last_code)
    assert torch.equal(yb, labels[SEED_A]) and torch.equal(ya, labels[SEED_B])  # the engine saw the same pseudo-labels
    for seed, opt, net in ((SEED_A, eng.optimizer, eng.model), (SEED_B, eng.optimizer_b, eng.model_b)):
        _, g32 = _hand_step(seed, batch, labels[seed], weight, False)
        _, g64 = _hand_step(seed, batch, labels[seed], weight, True)
        floor = max((g32[n] - g64[n]).abs().max().item() for n in g32)
        names = {id(p): n for n, p in net.named_parameters()}
        diff = max((opt.flat_grad[o:o + p.numel()] - g32[names[id(p)]]).abs().max().item() for p, o in zip(opt.params, opt.offsets))
        scale = max(g.abs().max().item() for g in g32.values())
        print(f"network {seed}: fp32-vs-fp64 floor of the hand-assembled step {floor:.3e}, engine vs fp32 hand step {diff:.3e}, "
              f"largest gradient {scale:.3e}")
        assert scale > 0 and floor > 0
        assert diff <= 10 * floor


def test_same_seed_same_bits():
    runs = []
    for _ in range(2):
        eng = _engine(dropout=0.2, confidence_threshold=0.4)
        losses = []
        for i in range(3):
            losses.append(eng.train_step(_batch(i)).clone())
            n = (B - LB) * HW * HW
            conf = eng.last_confident.cpu()
            assert 0 <= int(conf[0]) <= n and 0 <= int(conf[1]) <= n and 0 <= int(eng.last_agree.item()) <= n
            assert torch.isfinite(eng.last_supervised).item() and torch.isfinite(eng.last_cps).item()
        assert eng.dyn[0].item() == 0.5 and eng.dyn[1].item() == pytest.approx(0.4, rel=1e-6)
        assert eng.current_iter == 3 and eng.optimizer.step_count == 3 and eng.optimizer_b.step_count == 3
        runs.append((torch.stack(losses), eng.optimizer.flat_param.clone(), eng.optimizer_b.flat_param.clone()))
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.isfinite(runs[0][0]).all()
    assert not torch.equal(runs[0][1], runs[0][2])


@pytest.mark.parametrize("on_labeled", [False, True])
def test_agreement_and_confident_counts(on_labeled):
    eng = _engine(cps_on_labeled=on_labeled)
    batch = _batch(1)
    s = 0 if on_labeled else LB
    logits = []
    for net in (eng.model, eng.model_b):  # eval logits of the two networks on the CPS slice, before the step changes the weights
        net.eval()
        with torch.no_grad():
            logits.append(net(batch["image"])[s:].clone())
    want = int((logits[0].argmax(1) == logits[1].argmax(1)).sum().item())
    # a pixel whose two largest logits lie within 1e-5 may flip between the eval forward and the train forward of the step
    tops = [z.topk(2, dim=1).values for z in logits]
    near = sum(int((t[:, 0] - t[:, 1] < 1e-5).sum().item()) for t in tops)
    eng.train_step(batch)
    n = (B - s) * HW * HW
    print(f"agreement {int(eng.last_agree.item())} of {n} (eval logits: {want}, near-tied pixels: {near})")
    assert abs(int(eng.last_agree.item()) - want) <= near and 0 < want < n
    assert int(eng.last_confident.sum().item()) == 2 * n  # tau = 0: every pixel of the slice, in both directions


def test_checkpoint_round_trip(tmp_path):
    eng = _engine()
    for i in range(2):
        eng.train_step(_batch(i))
    eng.save_state_dict(tmp_path, save_training_state=True)
    assert (tmp_path / "model.pth").is_file() and (tmp_path / "training_state.pth").is_file() and (tmp_path / "cps_peer.pth").is_file()
    other = _engine(seed=11)
    assert not torch.equal(other.optimizer_b.flat_param, eng.optimizer_b.flat_param)
    epoch = ops.PARAM_EPOCH
    other.load_state_dict(tmp_path)
    assert ops.PARAM_EPOCH > epoch
    for mine, theirs in ((other.optimizer, eng.optimizer), (other.optimizer_b, eng.optimizer_b)):
        assert torch.equal(_bits(mine.flat_param), _bits(theirs.flat_param))
        assert torch.equal(_bits(mine.m), _bits(theirs.m)) and torch.equal(_bits(mine.v), _bits(theirs.v))
        assert mine.step_count == theirs.step_count == 2
    assert other.current_iter == eng.current_iter + 1  # the reference's resume rule (training/checkpoint.py)
    other.current_iter = eng.current_iter  # same schedule position on both sides for the comparison below
    la, lb = eng.train_step(_batch(2)), other.train_step(_batch(2))
    assert torch.equal(_bits(la), _bits(lb))
    assert torch.equal(_bits(other.optimizer.flat_param), _bits(eng.optimizer.flat_param))
    assert torch.equal(_bits(other.optimizer_b.flat_param), _bits(eng.optimizer_b.flat_param))
    # without the training state the peer file holds the model alone, and loading it leaves B's optimizer as it is
    eng.save_state_dict(tmp_path / "bare")
    assert set(torch.load(tmp_path / "bare" / "cps_peer.pth", weights_only=True)) == {"model"}
    third = _engine(seed=21)
    third.load_state_dict(tmp_path / "bare")
    assert torch.equal(_bits(third.optimizer_b.flat_param), _bits(eng.optimizer_b.flat_param)) and third.optimizer_b.step_count == 0


def test_predict_uses_either_network_or_the_mean_soft_max():
    eng = _engine()
    eng.train_step(_batch(0))
    x = _batch(60)["image"]
    eng.model.eval()
    eng.model_b.eval()
    with torch.no_grad():
        za, zb = eng.model(x).clone(), eng.model_b(x).clone()
    assert torch.equal(eng.predict(x, use="a"), za.softmax(1).argmax(1)) and torch.equal(eng.predict(x, use="b"), zb.softmax(1).argmax(1))
    assert torch.equal(eng.predict(x), eng.predict(x, use="a"))
    mean = 0.5 * za.double().softmax(1) + 0.5 * zb.double().softmax(1)
    got, want = eng.predict(x, use="mean"), mean.argmax(1)
    top = mean.topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) > 1e-6  # fp32 soft-maxes on the device: a closer call may go either way
    assert got.dtype == torch.int64 and got.shape == want.shape and clear.float().mean().item() > 0.99
    assert torch.equal(got[clear], want[clear])
    assert not eng.model.training and not eng.model_b.training
    eng.train_step(_batch(1))  # and training goes on after a prediction
    assert eng.model.training and eng.model_b.training
    with pytest.raises(ValueError):
        eng.predict(x, use="teacher")
