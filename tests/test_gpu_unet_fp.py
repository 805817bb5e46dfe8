"""models/unet/unet.py: `UNet.forward(fp_rows=...)`, UniMatch's feature-perturbation stream, on the GPU.  UNet(2, 1, 3, [8, 16],
instance norm, no dropout) in fp32 on 5 images of 32 x 32: instance norm normalises per image, so a row's logits do not depend on the
other rows and the clean rows, all-one masks and all-zero masks have exact consequences; the fused kernels against their tensor-op
form through the whole network, logits and parameter gradients bit for bit; and a three-level bf16 batch-norm network with its own
dropout on the default random masks."""
import pytest
import torch

import _featdrop_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, HW, ROWS = 5, 32, (2, 3)
CHANS = [8, 16]


def _net(seed=3):
    from models.unet import UNet
    torch.manual_seed(seed)
    return UNet(2, 1, 3, CHANS, normalization="instance", dropout_prob=None).to(DEV).train()


def _x(seed=0):
    return torch.rand(N, 1, HW, HW, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _bits(t):
    return t.detach().float().contiguous().view(torch.int32)


def _masks(kind):
    nu = ROWS[1]
    if kind == "ref":
        return [R.make_mask(nu, c, seed=c).to(DEV) for c in CHANS]
    return [torch.full((nu, c), 1.0 if kind == "ones" else 0.0, device=DEV) for c in CHANS]


@pytest.fixture(scope="module")
def plain():
    """model(x) of the seed-3 network: the reference of the tests below, computed once."""
    with torch.no_grad():
        return _net()(_x()).clone()


def test_the_keyword_path_without_the_stream_is_the_old_forward(plain):
    net = _net()
    with torch.no_grad():
        got = net(_x(), False, True, fp_rows=None, fp_drop=0.3, fp_masks=None, fp_fused=False)
    assert tuple(plain.shape) == (N, 3, HW, HW) and torch.equal(_bits(got), _bits(plain))


@pytest.mark.parametrize("fused", [True, False])
def test_clean_rows_all_one_and_all_zero_masks(plain, fused):
    net = _net()
    row0, nu = ROWS
    with torch.no_grad():
        ones = net(_x(), fp_rows=ROWS, fp_masks=_masks("ones"), fp_fused=fused)
        zeros = net(_x(), fp_rows=ROWS, fp_masks=_masks("zeros"), fp_fused=fused)
        rand = net(_x(), fp_rows=ROWS, fp_drop=0.5, fp_fused=fused)
    for out in (ones, zeros, rand):
        assert tuple(out.shape) == (N + nu, 3, HW, HW) and torch.isfinite(out).all()
        assert torch.equal(_bits(out[:N]), _bits(plain))  # per-image normalisation: the clean rows are model(x)
    assert torch.equal(_bits(ones[N:]), _bits(plain[row0:row0 + nu]))  # a multiplier of one changes nothing
    assert torch.equal(_bits(zeros[N]), _bits(zeros[N + 1])) and torch.equal(_bits(zeros[N]), _bits(zeros[N + 2]))
    assert not torch.equal(_bits(zeros[N:]), _bits(plain[row0:row0 + nu]))
    assert not torch.equal(_bits(rand[N:]), _bits(plain[row0:row0 + nu]))


def test_fused_and_tensor_op_form_agree_bit_for_bit_through_the_network():
    runs = []
    for fused in (True, False):
        net = _net()
        out = net(_x(), fp_rows=ROWS, fp_masks=_masks("ref"), fp_fused=fused)
        out.square().mean().backward()
        grad = torch.cat([p.grad.flatten() for p in net.parameters()])
        runs.append((out.detach().clone(), grad.clone()))
    (out_f, grad_f), (out_t, grad_t) = runs
    assert torch.isfinite(out_f).all() and torch.isfinite(grad_f).all() and grad_f.abs().max().item() > 0
    assert torch.equal(_bits(out_f), _bits(out_t))
    assert torch.equal(_bits(grad_f), _bits(grad_t))


def test_masks_argument_is_checked():
    net = _net()
    with pytest.raises(ValueError):
        net(_x(), fp_rows=ROWS, fp_masks=_masks("ones")[:1])
    with pytest.raises(ValueError):
        net(_x(), fp_rows=ROWS, fp_masks=[m[:2] for m in _masks("ones")])
    with pytest.raises(ValueError):
        net(_x(), fp_rows=ROWS, fp_drop=1.0)
    with pytest.raises(NotImplementedError):
        net(_x(), fp_rows=ROWS, return_ds=True)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_bf16_batch_norm_network_with_random_masks_is_reproducible(mode):
    from models.unet import UNet
    torch.manual_seed(9)
    net = UNet(2, 1, 3, [8, 16, 32], normalization="batch", dropout_prob=0.1).to(DEV).set_compute_dtype(torch.bfloat16)
    net.train(mode == "train")
    x = _x(1)
    runs = []
    for _ in range(2):
        torch.manual_seed(21)
        with torch.no_grad():
            runs.append(net(x, fp_rows=(1, 2), fp_drop=0.5).clone())
    torch.manual_seed(22)
    with torch.no_grad():
        other = net(x, fp_rows=(1, 2), fp_drop=0.5)
    assert tuple(runs[0].shape) == (N + 2, 3, HW, HW) and torch.isfinite(runs[0]).all()
    assert torch.equal(_bits(runs[0]), _bits(runs[1]))
    assert not torch.equal(_bits(runs[0][N:]), _bits(other[N:]))  # other draws, other perturbed rows
    # the stream is an argument, not a module: it perturbs in eval() as in train()
    assert not torch.equal(_bits(runs[0][N:]), _bits(runs[0][1:3]))


def test_residual_block_network_goes_through_the_same_call():
    from models.unet import UNet
    runs = []
    for fused in (True, False):
        torch.manual_seed(5)
        net = UNet(2, 1, 3, CHANS, block_type="res", norm_key="instance", dropout_prob=None).to(DEV).train()
        out = net(_x(), fp_rows=ROWS, fp_masks=_masks("ref"), fp_fused=fused)
        out.square().mean().backward()
        runs.append((out.detach().clone(), torch.cat([p.grad.flatten() for p in net.parameters()])))
    assert tuple(runs[0][0].shape) == (N + ROWS[1], 3, HW, HW) and torch.isfinite(runs[0][1]).all()
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))


def test_bf16_batch_norm_network_trains_through_the_stream():
    from models.unet import UNet
    torch.manual_seed(9)
    net = UNet(2, 1, 3, [8, 16, 32], normalization="batch", dropout_prob=0.1).to(DEV).set_compute_dtype(torch.bfloat16).train()
    torch.manual_seed(4)
    out = net(_x(1), fp_rows=(1, 2))
    out[N:].square().mean().backward()  # only the perturbed rows carry a gradient: it reaches the encoder through the new kernels
    g = net.encoder.levels[0][0].all[0].weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().max().item() > 0
