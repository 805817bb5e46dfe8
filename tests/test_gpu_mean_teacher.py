"""training/semi.py on the GPU: the mean-teacher step on a tiny net, UNet(2, 1, 3, [4, 8, 16], instance norm), B = 4 with 2 labelled
images of 32 x 32, Dice + CE as the supervised loss."""
import numpy as np
import pytest
import torch

import _consistency_ref as R
from mia_hip import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LB, B, HW = 2, 4, 32


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


def _engine(seed=3, dropout=None, **kw):
    from training.semi import MeanTeacherEngine
    args = dict(labeled_bs=LB, consistency_weight=0.5, start_lr=1e-2, lr_warmup_iter=0, num_iters=100)
    args.update(kw)
    eng = MeanTeacherEngine(_net(seed, dropout), _net(seed + 100, dropout), _sup(), **args)
    torch.manual_seed(seed + 7)  # the teacher's input noise and the Dropout2d masks
    return eng


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _fresh_logits(state_dict, x):
    net = _net(999)
    net.load_state_dict(state_dict)
    net.eval()
    with torch.no_grad():
        return net(x).clone()


def test_no_packed_teacher_weight_survives_the_ema():
    eng = _engine()
    x = _batch(50)["image"][:2]
    for i in range(3):
        loss = eng.train_step(_batch(i))
        assert torch.isfinite(loss).item()
        eng.teacher.eval()
        with torch.no_grad():
            got = eng.teacher(x).clone()
        want = _fresh_logits({k: v.detach().clone() for k, v in eng.teacher.state_dict().items()}, x)
        assert torch.equal(_bits(got), _bits(want)), f"step {i}: the teacher ran with stale packed weights"
        assert not torch.equal(eng.teacher_flat, eng.optimizer.flat_param) or i == 0
    assert eng._teacher_plan is not None  # the one-launch re-pack took over, and the check above held with it


@pytest.mark.parametrize("decay", [0.99, 0.0])
def test_teacher_parameters_follow_the_ema_of_the_student(decay):
    eng = _engine(ema_decay=decay)
    opt = eng.optimizer
    for i in range(3):
        before = eng.teacher_flat.cpu().numpy().copy()
        eng.train_step(_batch(i))
        student = opt.flat_param.cpu().numpy()
        got = eng.teacher_flat.cpu().numpy()
        alpha = float(np.float32(R.ema_alpha(i, decay)))
        if alpha == 0.0:
            assert np.array_equal(got.view(np.int32), student.view(np.int32))  # the student's bits
        else:
            err = np.abs(got.astype(np.float64) - R.ema(before, student, alpha))
            assert (err <= R.ema_bound(before, student, alpha)).all()
            assert not np.array_equal(got, student)
        for p, o, t in zip(opt.params, opt.offsets, eng.teacher_params):  # the modules see the buffer
            assert t.data_ptr() == eng.teacher_flat.data_ptr() + 4 * o and not t.requires_grad and t.grad is None
    assert eng.ema_step == 3 and eng.current_iter == 3


def test_teacher_passes_clobber_no_hint_of_the_students_backward():
    batch = _batch(0)
    with_teacher = _engine(noise_std=0.0, consistency_weight=0.0)
    without = _engine(noise_std=0.0, consistency=False)
    assert torch.equal(_bits(with_teacher.optimizer.flat_param), _bits(without.optimizer.flat_param))
    la, lb = with_teacher.train_step(batch), without.train_step(batch)
    assert torch.equal(_bits(la), _bits(lb))
    ga, gb = with_teacher.optimizer.flat_grad, without.optimizer.flat_grad
    assert ga.abs().max().item() > 0
    assert torch.equal(_bits(ga), _bits(gb))
    assert torch.equal(_bits(with_teacher.optimizer.flat_param), _bits(without.optimizer.flat_param))


TEACHER_SCALE = 1.05  # at step 0 the teacher IS the student and the consistency term vanishes: both sides scale the teacher's weights


def _hand_step(batch, weight, double):
    """One hand-assembled step on an identical model: the teacher is the student with every parameter times TEACHER_SCALE and sees
    the clean images; the consistency term is the torch expression, in fp32 or in fp64.  Returns {name: gradient}."""
    from training.engine import FlatOptimizer
    model, teacher = _net(3), _net(3)
    opt = FlatOptimizer(model, "adam")
    with torch.no_grad():
        for p in teacher.parameters():
            p.mul_(TEACHER_SCALE)
    model.train()
    teacher.train()
    image, label = batch["image"], batch["label"]
    with torch.no_grad():
        zt = teacher(image[LB:])
    out = model(image)
    sup = _sup()(out[:LB], label[:LB])
    zs = out[LB:]
    if double:
        cons = torch.mean((torch.softmax(zs.double(), 1) - torch.softmax(zt.double(), 1)) ** 2)
        loss = sup.double() + weight * cons
    else:
        cons = torch.mean((torch.softmax(zs, 1) - torch.softmax(zt, 1)) ** 2)
        loss = sup + weight * cons
    opt.zero_grad()
    loss.backward()
    names = {id(p): n for n, p in model.named_parameters()}
    return {names[id(p)]: opt.flat_grad[o:o + p.numel()].clone() for p, o in zip(opt.params, opt.offsets)}


def test_step_gradient_against_the_hand_assembled_step():
    """Tolerance: 10 x the largest per-tensor difference between two hand-assembled steps that evaluate the torch expression of the
    consistency term in fp32 and in fp64 -- a noise floor taken from the reference side, computed here each run.
    Measured on an MI355X: floor 7.5e-9 (tolerance 7.5e-8) beside a largest gradient of 0.13; the engine's step differs from the fp32
    hand step by 3.7e-9."""
    batch, weight = _batch(0), 0.5
    g32, g64 = _hand_step(batch, weight, False), _hand_step(batch, weight, True)
    floor = max((g32[n] - g64[n]).abs().max().item() for n in g32)
    eng = _engine(noise_std=0.0, consistency_weight=weight)
    eng.teacher_flat.mul_(TEACHER_SCALE)
    ops.bump_param_epoch()
    eng.train_step(batch)
    assert eng.last_consistency.item() > 0
    opt = eng.optimizer
    names = {id(p): n for n, p in eng.model.named_parameters()}
    diff = max((opt.flat_grad[o:o + p.numel()] - g32[names[id(p)]]).abs().max().item() for p, o in zip(opt.params, opt.offsets))
    scale = max(g.abs().max().item() for g in g32.values())
    print(f"fp32-vs-fp64 floor of the hand-assembled step {floor:.3e}, engine vs fp32 hand step {diff:.3e}, largest gradient {scale:.3e}")
    assert scale > 0 and floor > 0
    assert diff <= 10 * floor


def test_same_seed_same_bits_and_uncertainty_passes():
    runs = []
    for _ in range(2):
        eng = _engine(dropout=0.2, uncertainty_passes=2, threshold_ramp=0.5)
        losses = []
        for i in range(3):
            losses.append(eng.train_step(_batch(i)).clone())
            kept = int(eng.last_kept.item())
            assert 0 <= kept <= (B - LB) * HW * HW
            assert torch.isfinite(eng.last_supervised).item() and torch.isfinite(eng.last_consistency).item()
        assert eng.dyn[1].item() == pytest.approx(R.entropy_threshold(0.5, 3), rel=1e-6) and eng.dyn[0].item() == 0.5
        runs.append((torch.stack(losses), eng.optimizer.flat_param.clone(), eng.teacher_flat.clone()))
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.isfinite(runs[0][0]).all()


def test_checkpoint_round_trip_and_teacher_prediction(tmp_path):
    eng = _engine()
    for i in range(2):
        eng.train_step(_batch(i))
    eng.save_state_dict(tmp_path, save_training_state=True)
    assert (tmp_path / "model.pth").is_file() and (tmp_path / "mean_teacher.pth").is_file()
    other = _engine(seed=11)
    assert not torch.equal(other.teacher_flat, eng.teacher_flat)
    other.load_state_dict(tmp_path)
    assert torch.equal(_bits(other.optimizer.flat_param), _bits(eng.optimizer.flat_param))
    assert torch.equal(_bits(other.teacher_flat), _bits(eng.teacher_flat))
    assert other.ema_step == eng.ema_step == 2
    assert other.current_iter == eng.current_iter + 1  # the reference's resume rule (training/checkpoint.py)
    x = _batch(60)["image"]
    # the teacher's prediction path is the student's with other weights
    want_t = _fresh_logits({k: v.detach().clone() for k, v in eng.teacher.state_dict().items()}, x).softmax(1).argmax(1)
    want_s = _fresh_logits({k: v.detach().clone() for k, v in eng.model.state_dict().items()}, x).softmax(1).argmax(1)
    assert torch.equal(eng.predict(x, use_teacher=True), want_t) and torch.equal(other.predict(x, use_teacher=True), want_t)
    assert torch.equal(eng.predict(x), want_s) and torch.equal(other.predict(x), want_s)
    assert not eng.teacher.training and not eng.model.training
    eng.train_step(_batch(2))  # and training goes on after a prediction
    assert eng.teacher.training and eng.ema_step == 3
