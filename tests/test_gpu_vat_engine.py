"""The image gradient through the network, the backward without parameter gradients, `VATLoss.adversarial` and `VATEngine` on the
GPU.  The model is UNet(2, 1, 3, [8, 16, 32], dropout_prob=None) on 4 x 1 x 32 x 48 images with labeled_bs = 2 unless a test says
otherwise.

Bars.  An image gradient is judged like the parameter gradients of tests/test_gpu_configs.py: relative L2 distance from the EXACT
gradient (the CPU oracle in fp64) <= max(1e-2, 2 x the fp32 oracle's own distance from it).  The adversarial step x_adv - x has the
same bar; the final KL is held to relative 1e-2 (the gradient bar: it is a function of that direction) or twice the fp32 oracle's
distance, whichever is larger."""

import pytest
import torch

import _vat_ref as V
from mia_hip import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LB, B, H, W = 2, 4, 32, 48
CH = [8, 16, 32]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _net(seed=5, norm="instance", cin=1, channels=CH, dtype=torch.float32):
    from models.unet import UNet
    torch.manual_seed(seed)
    m = UNet(2, cin, 3, channels, normalization=norm, dropout_prob=None).to(DEV)
    return m.set_compute_dtype(dtype)


def _sup():
    from losses.compound_losses import DiceAndCELoss
    from losses.dice_loss import DiceLoss
    return DiceAndCELoss(dice_loss=DiceLoss, dice_kwargs=dict(num_classes=2, do_bg=True), ce_loss=torch.nn.CrossEntropyLoss, ce_kwargs={})


def _data(seed=11, cin=1):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, cin, H, W, generator=g), torch.randint(0, 3, (B, H, W), generator=g)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _rel(a, ref64):
    return float((a.double() - ref64).norm() / ref64.norm())


def _oracle_params(model, dtype):
    return {k: (v.detach().cpu().to(dtype).clone() if v.is_floating_point() else v.detach().cpu().clone())
            for k, v in model.state_dict().items()}


def _oracle_image_grad(model, x, y, norm, dtype):
    from oracle import losses_ref, unet_ref
    xi = x.to(dtype).clone().requires_grad_(True)
    out = unet_ref.unet_forward(_oracle_params(model, dtype), xi, norm, True)
    losses_ref.dice_and_ce(out, y.long(), 2).backward()
    return xi.grad.detach()


def _image_grad(model, x, y, need_grad=True):
    """(logits, image gradient or None, {name: parameter gradient}) of Dice + CE, from a clean slate."""
    for p in model.parameters():
        p.grad = None
    x = x.detach().requires_grad_(need_grad)
    out = model(x)
    _sup()(out, y).backward()
    return out.detach(), x.grad, {k: p.grad.clone() for k, p in model.named_parameters()}


# ------------------------------------------------------------------ (a) the forward does not depend on requires_grad
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_logits_do_not_depend_on_the_image_requiring_a_gradient(dtype):
    _need_gpu()
    model = _net(dtype=dtype).train()
    x = _data()[0].to(DEV)
    plain = model(x).detach().clone()
    with_grad = model(x.clone().requires_grad_(True))
    assert with_grad.requires_grad
    assert torch.equal(_bits(plain), _bits(with_grad))


# ------------------------------------------------------------------ (b) the image gradient against the oracle
@pytest.mark.parametrize("norm,cin,layout", [("instance", 1, "nchw"), ("batch", 1, "nchw"), ("instance", 3, "nchw"),
                                             ("instance", 3, "clast")])
def test_image_gradient_against_the_oracle(norm, cin, layout):
    _need_gpu()
    model = _net(norm=norm, cin=cin).train()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    x, y = _data(cin=cin)
    xd = x.to(DEV)
    if layout == "clast":
        xd = xd.contiguous(memory_format=torch.channels_last)
    _, gx, grads = _image_grad(model, xd, y.to(DEV))
    assert gx is not None and gx.shape == xd.shape and gx.dtype == torch.float32
    model.load_state_dict(state)  # (batch norm: the running statistics moved)
    g64 = _oracle_image_grad(model, x, y, norm, torch.float64)
    g32 = _oracle_image_grad(model, x, y, norm, torch.float32)
    rel, rel_cpu = _rel(gx.cpu(), g64), _rel(g32, g64)
    print(f"image gradient {norm} cin={cin} {layout}: rel L2 {rel:.3e} (fp32 oracle {rel_cpu:.3e})")
    assert rel <= max(1e-2, 2.0 * rel_cpu), (rel, rel_cpu)
    # the parameter gradients of that backward have the bits of a run whose image asks for no gradient
    model.load_state_dict(state)
    _, none, grads0 = _image_grad(model, xd, y.to(DEV), need_grad=False)
    assert none is None
    for k in grads0:
        assert torch.equal(_bits(grads[k]), _bits(grads0[k])), k


def test_image_gradient_bf16_compute_is_close_to_fp32():
    """bf16 activations: the bf16 path of mia_stem_dgrad inside the network.  The image sits behind the FIRST encoder conv, so its
    gradient has travelled the whole backward pass; it is held to the bars tests/test_gpu_configs.py sets for the deepest bf16 parameter
    gradients (why they are that wide is written there): relative L2 BF16_DEEP_REL_L2 = 0.60 and cosine BF16_DEEP_COS = 0.80.  A
    structural fault in the stem kernel is not judged here but bit for bit in tests/test_gpu_stem_dgrad.py."""
    _need_gpu()
    x, y = _data()
    g = {}
    for dt in (torch.float32, torch.bfloat16):
        model = _net(dtype=dt).train()
        g[dt] = _image_grad(model, x.to(DEV), y.to(DEV))[1]
        assert g[dt].dtype == torch.float32 and torch.isfinite(g[dt]).all()
    a, b = g[torch.bfloat16].cpu().double().reshape(-1), g[torch.float32].cpu().double().reshape(-1)
    rel, cos = _rel(a, b), float(torch.dot(a, b) / (a.norm() * b.norm()))
    print(f"image gradient bf16 vs fp32 compute: rel L2 {rel:.3e} cos {cos:.4f}")
    assert rel <= 0.60 and cos >= 0.80


# ------------------------------------------------------------------ (c) a backward without parameter gradients
@pytest.mark.parametrize("channels", [CH, [64, 128]], ids=["8-16-32", "64-128"])
def test_frozen_backward_touches_no_parameter_gradient(channels, monkeypatch):
    _need_gpu()
    from training.engine import FlatOptimizer
    model = _net(channels=channels).train()
    opt = FlatOptimizer(model, "adam")
    x, y = _data()
    xd, yd = x.to(DEV), y.to(DEV)
    _, gx_ref, _ = _image_grad(model, xd, yd)
    opt.zero_grad()
    assert not ops._GRAD_CLAIMED
    opt.flat_grad.fill_(-123.0)
    names = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    with ops.frozen_parameters(model):
        assert not any(p.requires_grad for p in model.parameters())
        xg = xd.detach().clone().requires_grad_(True)
        gx, = torch.autograd.grad(_sup()(model(xg), yd), xg)
    assert all(p.requires_grad for p in model.parameters())
    torch.cuda.synchronize()
    assert bool((opt.flat_grad == -123.0).all())
    assert all(p.grad is None for p in model.parameters())
    assert not ops._GRAD_CLAIMED
    assert "mia_stem_dgrad" in names and not [n for n in names if "wgrad" in n], names
    assert torch.equal(_bits(gx), _bits(gx_ref))


# ------------------------------------------------------------------ (d) the power iteration against the oracle
def _oracle_adversarial(model, x, d0, norm, dtype, xi, eps):
    from oracle import unet_ref

    def fwd(inp):
        return unet_ref.unet_forward(_oracle_params(model, dtype), inp, norm, True)

    n = x.shape[0]
    x = x.to(dtype)
    with torch.no_grad():
        z_clean = fwd(x)
    d = V.normalize(d0).to(dtype)
    x_hat = (x + xi * d).requires_grad_(True)
    lq, lp = torch.log_softmax(fwd(x_hat), 1), torch.log_softmax(z_clean, 1)
    dist = (lp.exp() * (lp - lq)).sum() / n
    g, = torch.autograd.grad(dist, x_hat)
    x_adv = x + eps * V.normalize(g).to(dtype)
    with torch.no_grad():
        final = V.kl(fwd(x_adv), z_clean, n * H * W)[0]
    return (x_adv - x).double(), float(final)


def test_adversarial_against_the_oracle():
    _need_gpu()
    from losses.vat_loss import VATLoss
    model = _net().train()
    x = _data()[0][:2]
    d0 = torch.rand(x.shape, generator=torch.Generator().manual_seed(4)) - 0.5
    vat = VATLoss(xi=10.0, eps=6.0, ip=1)
    xd = x.to(DEV)
    with torch.no_grad():
        z_clean = model(xd)
    x_adv = vat.adversarial(model, xd, z_clean, d0=d0.to(DEV))
    assert not x_adv.requires_grad
    with torch.no_grad():
        vat(model(x_adv), z_clean)
    got_step, got_kl = (x_adv - xd).cpu(), float(vat.last_value)
    s64, k64 = _oracle_adversarial(model, x, d0, "instance", torch.float64, 10.0, 6.0)
    s32, k32 = _oracle_adversarial(model, x, d0, "instance", torch.float32, 10.0, 6.0)
    rel, rel_cpu = _rel(got_step, s64), _rel(s32, s64)
    krel, krel_cpu = abs(got_kl - k64) / k64, abs(k32 - k64) / k64
    print(f"adversarial step: rel L2 {rel:.3e} (fp32 oracle {rel_cpu:.3e}); final KL {got_kl:.6e} vs {k64:.6e}: rel {krel:.3e} "
          f"(fp32 oracle {krel_cpu:.3e})")
    assert abs(float(got_step.double().reshape(2, -1).norm(dim=1)[0]) - 6.0) < 1e-3
    assert rel <= max(1e-2, 2.0 * rel_cpu), (rel, rel_cpu)
    assert krel <= max(1e-2, 2.0 * krel_cpu), (krel, krel_cpu)


# ------------------------------------------------------------------ (e) batch-norm buffers
def test_adversarial_leaves_batch_norm_buffers_alone():
    _need_gpu()
    from losses.vat_loss import VATLoss
    model = _net(norm="batch").train()
    xd = _data()[0].to(DEV)
    model(xd)  # one tracked pass, so the buffers are not at their initial values
    before = {k: v.clone() for k, v in model.named_buffers()}
    assert before and int(before["encoder.levels.0.0.all.2.num_batches_tracked"]) == 1
    with torch.no_grad(), ops.no_bn_tracking():
        z_clean = model(xd)
    for k, v in model.named_buffers():
        assert torch.equal(v, before[k]), k
    x_adv = VATLoss(ip=2).adversarial(model, xd, z_clean)
    assert torch.isfinite(x_adv).all()
    for k, v in model.named_buffers():
        assert torch.equal(v, before[k]), k
    model(xd)  # and tracking is back
    assert int(dict(model.named_buffers())["encoder.levels.0.0.all.2.num_batches_tracked"]) == 2


# ------------------------------------------------------------------ (f) - (h) the engine
def _batch(seed):
    x, y = _data(seed)
    return {"image": x.to(DEV), "label": y[:LB].to(DEV)}


def _engine(seed=3, dtype=torch.float32, **kw):
    from training.semi import VATEngine
    args = dict(labeled_bs=LB, vat_weight=0.5, start_lr=1e-2, lr_warmup_iter=0, num_iters=100)
    args.update(kw)
    eng = VATEngine(_net(seed, dtype=dtype), _sup(), **args)
    torch.manual_seed(seed + 7)  # the power iteration's start noise
    return eng


def test_engine_two_steps_are_reproducible():
    _need_gpu()
    runs = []
    for _ in range(2):
        eng = _engine()
        for i in range(2):
            loss = eng.train_step(_batch(i))
            assert isinstance(loss, torch.Tensor) and loss.is_cuda and not loss.requires_grad
        assert bool(torch.isfinite(loss)) and float(eng.last_vat) >= 0.0 and bool(torch.isfinite(eng.last_supervised))
        assert all(p.grad is not None for p in eng.model.parameters())
        assert eng.current_iter == 2 and float(eng.dyn[0]) == 0.5 and float(eng.dyn[1]) == 6.0
        runs.append((eng.optimizer.flat_param.clone(), loss.clone()))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))


def test_engine_without_vat_forwards_the_labelled_images_only(monkeypatch):
    _need_gpu()
    eng = _engine(vat=False)
    monkeypatch.setattr(ops, "vat_noise", lambda *a, **k: pytest.fail("the engine drew noise"))
    seen = []
    eng.model.register_forward_pre_hook(lambda m, args: seen.append(args[0].shape[0]))
    gen = torch.cuda.default_generators[0]
    off = gen.get_offset()
    loss = eng.train_step(_batch(0))
    assert bool(torch.isfinite(loss)) and seen == [LB] and eng.last_vat is None and gen.get_offset() == off
    assert torch.equal(loss, eng.last_supervised)
    # a batch without unlabelled images, with the term switched on: the same route
    eng2 = _engine()
    b = _batch(0)
    b["image"] = b["image"][:LB]
    seen2 = []
    eng2.model.register_forward_pre_hook(lambda m, args: seen2.append(args[0].shape[0]))
    assert bool(torch.isfinite(eng2.train_step(b))) and seen2 == [LB]


def test_engine_bf16_step_is_finite_and_deterministic():
    _need_gpu()
    runs = []
    for _ in range(2):
        eng = _engine(dtype=torch.bfloat16)
        loss = eng.train_step(_batch(0))
        assert bool(torch.isfinite(loss)) and float(eng.last_vat) >= 0.0
        runs.append(eng.optimizer.flat_param.clone())
    assert torch.equal(_bits(runs[0]), _bits(runs[1]))
