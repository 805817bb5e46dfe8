"""csrc/feat_drop.hip on the GPU: `ops.feature_dropout_cat` and the two entry points behind it against the tensor-op form under
autograd (tests/_featdrop_ref.py), BIT FOR BIT, forward output and dx -- no tolerance is involved.  The fp32 cases use masks of
{0, 1 / 0.7} on standard-normal data: a fused multiply-add in the backward would change the bits of about 30 % of the elements, so
these cases also pin the two separately rounded operations (bf16 would not: about 0.04 %)."""
import ctypes

import pytest
import torch

import _featdrop_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16

# (dtype, N, H, W, C, row0, nu)
CASES = [
    (F32, 3, 5, 7, 4, 1, 2),      # one 16-byte unit per pixel, odd pixel count, perturbed rows last
    (F32, 3, 5, 7, 6, 0, 1),      # 24-byte pixels: the one-element path, first row perturbed
    (BF16, 4, 3, 3, 8, 1, 2),     # perturbed rows in the middle; row 3 is a pure copy both ways
    (BF16, 2, 4, 4, 12, 0, 2),    # one-element bf16, every row perturbed
    (F32, 2, 1, 1, 1024, 0, 2),   # one pixel, wide channel axis
    (F32, 4, 3, 3, 4, 1, 3),      # an all-zero and an all-one mask row beside a mixed one
    (BF16, 5, 2, 3, 8, 1, 3),
    (F32, 3, 3, 5, 12, 1, 2),     # three units per pixel: not a power of two
    (BF16, 2, 3, 3, 4104, 0, 1),  # 513 units per pixel: more than a tile holds, one pixel per tile
]


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _data(dtype, n, h, w, c, nu, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, c, generator=g).to(dtype).to(DEV)
    dy = torch.randn(n + nu, h, w, c, generator=g).to(dtype).to(DEV)
    return x, dy, R.make_mask(nu, c, seed=seed + 1).to(DEV)


def _fused(x, mask, row0, dy):
    from mia_hip import ops
    leaf = x.detach().clone().requires_grad_(True)
    out = ops.feature_dropout_cat(leaf, mask, row0)
    out.backward(dy)
    return out.detach(), leaf.grad


def _raw(name, src, mask, dst, n, row0, nu, slot=None):
    """The entry point itself, on tensors as they are (no `.contiguous()`, no alignment repair)."""
    import mia_hip
    from mia_hip import ops
    h, w, c = src.shape[1:]
    mia_hip.call(name, ops._dt(src), ops._p(src), ops._p(mask), ops._p(dst), n, ctypes.c_int64(h * w), c, row0, nu, ops._p(slot),
                 ops._stream())
    return dst


@pytest.mark.parametrize("dtype,n,h,w,c,row0,nu", CASES)
def test_forward_and_dx_have_the_bits_of_the_tensor_op_form(dtype, n, h, w, c, row0, nu):
    x, dy, mask = _data(dtype, n, h, w, c, nu)
    want_out, want_dx = R.tensor_ops_grad(x, mask, row0, dy)
    out, dx = _fused(x, mask, row0, dy)
    assert _same(out, want_out) and _same(dx, want_dx)
    assert _same(out[:n], x)  # the clean rows are a copy
    outside = [i for i in range(n) if not row0 <= i < row0 + nu]
    assert _same(dx[outside], dy[outside])  # and so is the gradient of a row that has no twin
    out2, dx2 = _fused(x, mask, row0, dy)  # the same bits from a second call
    assert _same(out2, out) and _same(dx2, dx)
    if dtype == F32 and (mask == R.SCALE).any():
        # what this case would not notice must not be what it is there for: a fused multiply-add differs from the two roundings
        a, b, m = dy[row0:row0 + nu].double(), dy[n:].double(), mask[:, None, None, :].double()
        fma = torch.where(m == 0, a, a + b * m).float()
        assert not torch.equal(fma, dx[row0:row0 + nu])


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_more_tiles_than_one_sweep_of_the_grid(dtype):
    """The launch code caps the grid and a block strides over tiles of whole pixels: two tiles per image (one full, one of three
    pixels) and more images than half the cap, so some blocks take a second tile -- perturbed and plain rows among them."""
    import mia_hip
    c = 4 if dtype == F32 else 16
    px = ctypes.c_int(0)
    cap = mia_hip.lib().mia_feat_drop_cat_sweep(mia_hip.F32 if dtype == F32 else mia_hip.BF16, c, 1, ctypes.byref(px))
    assert cap > 0 and px.value >= 1
    hw, n = px.value + 3, cap // 2 + 5
    assert 2 * n > cap and n * hw * c * x_bytes(dtype) <= 16 << 20
    row0, nu = n - 40, 38  # the last two rows stay plain
    x, dy, mask = _data(dtype, n, 1, hw, c, nu, seed=5)
    want_out, want_dx = R.tensor_ops_grad(x, mask, row0, dy)
    out, dx = _fused(x, mask, row0, dy)
    assert _same(out, want_out) and _same(dx, want_dx)


def x_bytes(dtype):
    return 4 if dtype == F32 else 2


def _shifted(t):
    """The same values at an address 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def test_misaligned_pointers_fall_back_to_the_same_bits():
    n, h, w, c, row0, nu = 3, 5, 7, 4, 1, 2
    x, dy, mask = _data(F32, n, h, w, c, nu, seed=2)
    want_out, want_dx = R.tensor_ops_grad(x, mask, row0, dy)
    out = _raw("mia_feat_drop_cat_fwd", _shifted(x), mask, torch.empty_like(want_out), n, row0, nu)
    dx = _raw("mia_feat_drop_cat_bwd", _shifted(dy), mask, torch.empty_like(want_dx), n, row0, nu)
    assert _same(out, want_out) and _same(dx, want_dx)
    # ... and a shifted destination or mask
    out = _raw("mia_feat_drop_cat_fwd", x, mask, _shifted(torch.empty_like(want_out)), n, row0, nu)
    dx = _raw("mia_feat_drop_cat_bwd", dy, _shifted(mask), torch.empty_like(want_dx), n, row0, nu)
    assert _same(out, want_out) and _same(dx, want_dx)
    # the aligned call takes the 16-byte path
    assert _same(_raw("mia_feat_drop_cat_fwd", x, mask, torch.empty_like(want_out), n, row0, nu), want_out)


@pytest.mark.parametrize("dtype,c", [(F32, 4), (F32, 6), (BF16, 8), (BF16, 12)])
def test_a_dropped_channel_is_a_selection(dtype, c):
    n, h, w, row0, nu = 3, 2, 3, 1, 2
    x, dy, mask = _data(dtype, n, h, w, c, nu, seed=3)
    mask[0, :4] = 0.0
    mask[1] = 0.0
    bad = torch.tensor([float("inf"), float("-inf"), float("nan"), -1.0], device=DEV).to(dtype)
    x[row0:row0 + nu, :, :, :4] = bad
    out, _ = _fused(x, mask, row0, dy)
    pert = out[n:]
    assert torch.isfinite(pert.float()).all()
    assert not _bits(pert[0, :, :, :4]).any() and not _bits(pert[1]).any()  # +0.0: every bit clear, the sign included
    assert _same(out, R.tensor_ops(x, mask, row0))
    # backward: a NaN (or anything else) in the twin's gradient under a dropped channel leaves dy[n]'s bits
    dy[n:, :, :, :4] = bad
    dy[n + 1] = float("nan")
    _, dx = _fused(x, mask, row0, dy)
    assert _same(dx[row0, :, :, :4], dy[row0, :, :, :4]) and _same(dx[row0 + 1], dy[row0 + 1])
    assert torch.isfinite(dx.float()).all()


@pytest.mark.parametrize("n,h,w,c,row0,nu", [(3, 5, 7, 4, 1, 2), (3, 5, 7, 6, 0, 1), (2, 9, 33, 64, 0, 2)])
def test_amax_slot_holds_the_bits_of_the_maximum(n, h, w, c, row0, nu):
    from mia_hip import ops
    x, dy, mask = _data(F32, n, h, w, c, nu, seed=4)
    leaf = x.clone().requires_grad_(True)
    out = ops.feature_dropout_cat(leaf, mask, row0)
    slot, version = out._mia_amax
    assert version == out._version and slot.item() == out.detach().abs().max().view(torch.int32).item()
    assert not hasattr(out, "_mia_dup")
    for name, src, shape in (("mia_feat_drop_cat_fwd", x, out.shape), ("mia_feat_drop_cat_bwd", dy, x.shape)):
        slot = torch.zeros(1, device=DEV, dtype=torch.int32)
        got = _raw(name, src, mask, torch.empty(tuple(shape), device=DEV), n, row0, nu, slot)
        assert slot.item() == got.abs().max().view(torch.int32).item() > 0
    # a bf16 call leaves the slot alone
    slot = torch.zeros(1, device=DEV, dtype=torch.int32)
    _raw("mia_feat_drop_cat_fwd", x.to(BF16), mask, torch.empty(tuple(out.shape), device=DEV, dtype=BF16), n, row0, nu, slot)
    assert slot.item() == 0


def test_wrapper_by_products_and_none_gradient():
    from mia_hip import ops
    x, dy, mask = _data(BF16, 3, 2, 2, 8, 2, seed=6)
    x._mia_dup = True
    leaf = x.requires_grad_(True)
    out = ops.feature_dropout_cat(leaf, mask, 1)
    assert not hasattr(out, "_mia_dup") and not hasattr(out, "_mia_amax")  # an ordinary tensor; the maximum serves fp32 only
    assert ops.FeatDropCatFn.backward(type("Ctx", (), {})(), None) == (None, None, None)
    with torch.no_grad():
        assert _same(ops.feature_dropout_cat(x, mask, 1), out)
    with pytest.raises(Exception):
        ops.feature_dropout_cat(x.detach().double(), mask, 1)  # the fused form serves fp32 and bf16
    assert ops.feature_dropout_cat(x.detach().double(), mask, 1, fused=False).dtype == torch.float64
