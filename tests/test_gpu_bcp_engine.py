"""training/semi.py: `BCPEngine` on the GPU, on a tiny net -- UNet(2, 1, 3, [4, 8], instance norm), B = 8 with 4 labelled images of
32 x 32: a self-training step against the same step composed by hand from the public pieces, the EMA, reproducibility, the rows of
the network input, pre-training and the checkpoint."""
import pytest
import torch

from mia_hip import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LB, B, HW = 4, 8, 32
H = LB // 2
OPT = dict(start_lr=1e-2, lr_warmup_iter=0, num_iters=100)


def _net(seed):
    from models.unet import UNet
    torch.manual_seed(seed)
    return UNet(2, 1, 3, [4, 8], normalization="instance", dropout_prob=None).to(DEV)


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    return {"image": torch.rand(B, 1, HW, HW, generator=g).to(DEV), "label": torch.randint(0, 3, (LB, HW, HW), generator=g).to(DEV)}


def _engine(seed=3, **kw):
    from training.semi import BCPEngine
    args = dict(labeled_bs=LB, **OPT)
    args.update(kw)
    return BCPEngine(_net(seed), _net(seed + 100), **args)


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


def _hand_step(batch, seed, mask_seed, u_weight=0.5):
    """The self-training step from the public pieces; returns (loss, flat_grad, flat_param, mask, teacher parameters before the EMA)."""
    from inference.components import filter_components
    from inference.predictor import softmax_accum
    from losses.copy_paste import CopyPasteLoss, random_box_mask
    from training.engine import EngineBase
    model, teacher = _net(seed), _net(seed + 100)
    opt, sched = EngineBase._make_optimizer(model, "adam", None, OPT["start_lr"], OPT["num_iters"], OPT["lr_warmup_iter"], 1, "poly")
    teacher.load_state_dict(model.state_dict())  # the engine's teacher starts as the student
    model.train()
    teacher.train()
    sched.step(0)
    image, label = batch["image"], batch["label"]
    torch.manual_seed(mask_seed)
    with torch.no_grad():
        zt = teacher(image[LB:])
        pseudo = torch.empty((LB, HW, HW), device=DEV, dtype=torch.int64)
        softmax_accum(zt, None, pseudo, first=True)
        pseudo = filter_components(pseudo, keep_largest=True, n_classes=3)
    mask = random_box_mask(HW, HW, 2 / 3, device=DEV)
    net_in = torch.empty((LB, 1, HW, HW), device=DEV)
    ops.bcp_mix(image[LB:LB + H], image[:H], mask, out=net_in[:H])
    ops.bcp_mix(image[H:LB], image[LB + H:], mask, out=net_in[H:])
    out = model(net_in)
    crit = CopyPasteLoss(2)
    loss = crit(out[:H], pseudo[:H], label[:H], mask, u_weight, 1.0) + crit(out[H:], label[H:LB], pseudo[H:], mask, 1.0, u_weight)
    opt.zero_grad()
    loss.backward(torch.ones_like(loss))
    grad = opt.flat_grad.clone()
    opt.step(max_grad_norm=10.0)
    return loss.detach(), grad, opt.flat_param.clone(), mask, net_in


def test_step_equals_the_hand_composed_step_bit_for_bit():
    batch = _batch(0)
    eng = _engine()
    torch.manual_seed(21)
    loss = eng.train_step(batch)
    grad, param = eng.optimizer.flat_grad.clone(), eng.optimizer.flat_param.clone()
    want_loss, want_grad, want_param, mask, _ = _hand_step(batch, 3, 21)
    assert torch.isfinite(loss).item() and grad.abs().max().item() > 0
    assert torch.equal(_bits(loss), _bits(want_loss))
    assert torch.equal(eng.last_mask, mask) and 0 < int(mask.sum()) < HW * HW
    assert torch.equal(_bits(grad), _bits(want_grad))
    assert torch.equal(_bits(param), _bits(want_param))
    assert torch.equal(_bits(eng.last_inward + eng.last_outward), _bits(loss))
    # after it the teacher is ema_update of the student: the first update (alpha = 0) copies the student's bits
    assert eng.ema_step == 1 and eng.current_iter == 1
    assert torch.equal(_bits(eng.teacher_flat), _bits(param))


def test_teacher_follows_ema_update_of_the_student():
    from training.semi import ema_alpha
    eng = _engine(ema_decay=0.9)
    for i in range(3):
        before = eng.teacher_flat.clone()
        eng.train_step(_batch(i))
        want = before.clone()
        ops.ema_update(want, eng.optimizer.flat_param, ema_alpha(i, 0.9))
        assert torch.equal(_bits(eng.teacher_flat), _bits(want))
        assert i == 0 or not torch.equal(eng.teacher_flat, eng.optimizer.flat_param)
    for p, o, t in zip(eng.optimizer.params, eng.optimizer.offsets, eng.teacher_params):  # the modules see the buffer
        assert t.data_ptr() == eng.teacher_flat.data_ptr() + 4 * o and not t.requires_grad and t.grad is None
    assert eng.ema_step == 3


def test_same_seed_same_bits():
    runs = []
    for _ in range(2):
        eng = _engine()
        torch.manual_seed(5)
        losses = [eng.train_step(_batch(i)).clone() for i in range(3)]
        runs.append((torch.stack(losses), eng.optimizer.flat_param.clone(), eng.teacher_flat.clone(), eng.last_mask.clone()))
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(runs[0][3], runs[1][3]) and torch.isfinite(runs[0][0]).all()


def test_mask_ratio_zero_feeds_the_unlabelled_and_the_labelled_rows():
    batch = _batch(1)
    eng = _engine(mask_ratio=0.0)
    eng.model = spy = _Spy(eng.model)
    loss = eng.train_step(batch)
    assert torch.isfinite(loss).item() and eng.last_mask.all()
    assert len(spy.seen) == 1  # ONE student forward
    net_in = spy.seen[0]
    image = batch["image"]
    assert torch.equal(_bits(net_in[:H]), _bits(image[LB:LB + H]))  # inward rows: U_a
    assert torch.equal(_bits(net_in[H:]), _bits(image[H:LB]))       # outward rows: X_b
    # and with a box the rows are the mix
    eng2 = _engine()
    eng2.model = spy2 = _Spy(eng2.model)
    torch.manual_seed(9)
    eng2.train_step(batch)
    m = (eng2.last_mask != 0)[None, None]
    assert torch.equal(_bits(spy2.seen[0][:H]), _bits(torch.where(m, image[LB:LB + H], image[:H])))
    assert torch.equal(_bits(spy2.seen[0][H:]), _bits(torch.where(m, image[H:LB], image[LB + H:])))


def test_pretrain_leaves_the_teacher_alone_and_begin_self_training_adopts_the_student():
    from losses.copy_paste import CopyPasteLoss
    batch = _batch(2)
    eng = _engine(pretrain=True)
    eng.teacher = spy = _Spy(eng.teacher)
    eng.model = mspy = _Spy(eng.model)
    start = eng.optimizer.flat_param.clone()
    with torch.no_grad():
        eng.teacher_flat.mul_(1.25)  # make the teacher differ from the student, to see that nothing touches it
    ops.bump_param_epoch()
    frozen = eng.teacher_flat.clone()
    torch.manual_seed(13)
    loss = eng.train_step(batch)
    assert torch.isfinite(loss).item() and not spy.seen  # the teacher never ran
    assert torch.equal(_bits(eng.teacher_flat), _bits(frozen)) and eng.ema_step == 0
    assert not torch.equal(eng.optimizer.flat_param, start) and eng.current_iter == 1
    # the input is M ? X_a : X_b (h rows), the loss CopyPasteLoss(out, Y_a, Y_b, M, 1, 1)
    image, label = batch["image"], batch["label"]
    m = (eng.last_mask != 0)[None, None]
    assert len(mspy.seen) == 1 and torch.equal(_bits(mspy.seen[0]), _bits(torch.where(m, image[:H], image[H:LB])))
    fresh = _net(3)
    fresh.train()
    want = CopyPasteLoss(2)(fresh(mspy.seen[0]), label[:H], label[H:LB], eng.last_mask, 1.0, 1.0)
    assert torch.equal(_bits(loss), _bits(want))
    eng.teacher, eng.model = spy.net, mspy.net
    eng.begin_self_training()
    assert not eng.pretrain and torch.equal(_bits(eng.teacher_flat), _bits(eng.optimizer.flat_param))
    for (n, a), (_, b) in zip(eng.model.state_dict().items(), eng.teacher.state_dict().items()):
        assert torch.equal(a, b), n
    eng.train_step(_batch(3))  # and self-training goes on from there
    assert eng.ema_step == 1 and eng.last_outward is not None


def test_two_teacher_engines_alternate_in_one_process(monkeypatch):
    """A `BCPEngine` and a `MeanTeacherEngine` stepped in turn (what tools/microbench_bcp.py does), on the fp32 split-f16 conv path
    (forced here for a small net).  Each optimizer step moves the parameter epoch on, so the OTHER engine's packed weights miss and
    re-pack themselves one by one after their `PackPlan` was planted; the per-tensor split descriptor then has to name the slot the
    plan hung on the buffer (ops.PackPlan.plant) -- with the buffer's first slot, since freed, the weights were scaled by whatever
    that memory held and both engines went to NaN at their third step.  Each engine must take the steps it takes alone: the two paths
    pack the same bits, and a wrong power-of-two scale would move the loss by far more than the 1e-5 allowed here for fp32 noise."""
    from losses.compound_losses import DiceAndCELoss
    from losses.dice_loss import DiceLoss
    from models.unet import UNet
    from training.semi import BCPEngine, MeanTeacherEngine
    monkeypatch.setattr(ops, "F32_SPLIT_MIN_MACS", 0)
    size = 64

    def net(seed):
        torch.manual_seed(seed)
        return UNet(2, 1, 3, [16, 32], normalization="instance", dropout_prob=None).to(DEV)

    def engines():
        sup = DiceAndCELoss(dice_loss=DiceLoss, dice_kwargs=dict(num_classes=2, do_bg=True), ce_loss=torch.nn.CrossEntropyLoss, ce_kwargs={})
        return (BCPEngine(net(1), net(2), labeled_bs=LB, **OPT),
                MeanTeacherEngine(net(1), net(2), sup, labeled_bs=LB, noise_std=0.0, **OPT))

    g = torch.Generator().manual_seed(4)
    batch = {"image": torch.rand(B, 1, size, size, generator=g).to(DEV), "label": torch.randint(0, 3, (LB, size, size), generator=g).to(DEV)}
    alone = []
    for k in range(2):
        eng = engines()[k]
        torch.manual_seed(17)
        alone.append(torch.stack([eng.train_step(batch).clone() for _ in range(5)]))
    pair = engines()
    torch.manual_seed(17)
    state = [torch.random.get_rng_state(), torch.random.get_rng_state()]
    turns = [[], []]
    for _ in range(5):
        for k in (0, 1):
            torch.random.set_rng_state(state[k])  # each engine draws its masks from its own stream, as when it runs alone
            turns[k].append(pair[k].train_step(batch).clone())
            state[k] = torch.random.get_rng_state()
    for k in range(2):
        got = torch.stack(turns[k])
        assert torch.isfinite(got).all() and torch.isfinite(pair[k].optimizer.flat_param).all() and torch.isfinite(pair[k].teacher_flat).all()
        assert torch.allclose(got, alone[k], rtol=1e-5, atol=0.0), (k, got, alone[k])


def test_checkpoint_round_trip(tmp_path):
    eng = _engine(ema_decay=0.9)
    for i in range(2):
        eng.train_step(_batch(i))
    eng.save_state_dict(tmp_path, save_training_state=True)
    assert (tmp_path / "model.pth").is_file() and (tmp_path / "mean_teacher.pth").is_file()
    other = _engine(seed=11)
    assert not torch.equal(other.teacher_flat, eng.teacher_flat)
    other.load_state_dict(tmp_path)
    assert torch.equal(_bits(other.optimizer.flat_param), _bits(eng.optimizer.flat_param))
    assert torch.equal(_bits(other.teacher_flat), _bits(eng.teacher_flat))
    assert not torch.equal(eng.teacher_flat, eng.optimizer.flat_param)
    assert other.ema_step == eng.ema_step == 2
    x = _batch(60)["image"]
    assert torch.equal(eng.predict(x, use_teacher=True), other.predict(x, use_teacher=True))
    assert torch.equal(eng.predict(x), other.predict(x))
    eng.train_step(_batch(2))  # and training goes on after a prediction
    assert eng.teacher.training and eng.ema_step == 3
