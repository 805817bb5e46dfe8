"""csrc/bcp.hip on the GPU against the float64 restatement (tests/_bcp_ref.py): the mix bit for bit against `torch.where`; counts,
the four terms, the value and the gradient of the two-source loss in every layout, on the 16-byte and the scalar path, with int64 and
uint8 labels and both mask shapes; empty regions, zero weights, an absent class, saturated logits, the label-range protocol,
determinism, and the tensor-op form (`fused=False`).

Counts are compared EXACTLY.  Bounds, with the project's constant 2e-6 (32 roundings x 2^-24, tests/test_gpu_consistency.py,
tests/test_gpu_cps.py) times the magnitudes the restatement returns:
    |C_r - ref| <= 2e-6 * sum m_r (1 + |z_y - max z|) / N_r                         the CPS magnitude: the term is log sum exp(z - max)
                                                                                   + (max - z_y), the second part exact in double
    |D_r - ref| <= 2e-6 * (1/K) sum_k (2 I_rk / den + (2 I_rk + s) Z_rk / den^2)    a 2e-6 relative error of I and Z through the quotient
    |L - ref|   <= 2e-6 * (wa (magD_A + magC_A) / 2 + wb (magD_B + magC_B) / 2)
    |g - ref|   <= 2e-6 * (sum of the absolute values of the gradient's terms) + 1e-12       per element
The kernels evaluate the soft-max in double from fp32 expf, add per thread and per wave in double, and round a block's sum to a
(hi, lo) float pair whose four wave parts are added in fp32: a few 2^-24 relative on I, Z and the CE sum; the gradient is one fp32
rounding of a double expression of that soft-max and of coefficients rounded once to fp32.
Measured on an MI355X over every case below: the error of the value and of the four terms is at most 0.28 of its bound, the gradient
error at most 0.072; for the tensor-op form (`fused=False`, fp32 torch ops) 0.22 and 0.27."""
import functools

import numpy as np
import pytest
import torch

import _bcp_ref as R
import mia_hip
from mia_hip import ops

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 1, 7), (4, 37, 61), (2, 336, 544)]  # hw odd: the one-pixel loads; the last: 16-byte units, several slabs
K1S = [2, 4, 8]
LAYOUTS = ["planar", "clast", "slice", "offset"]
LABELS = ["int64", "uint8"]
MASKS = ["hw", "bhw"]
DEV = "cuda:0"
WA, WB = 0.5, 1.0


@functools.lru_cache(maxsize=None)
def _case(nb, h, w, k1, per_image, absent=False):
    """Inputs and their float64 reference at weights (WA, WB), computed once and never modified."""
    z, ya, yb = R.make_case(nb, k1, h, w, absent=absent)
    mask = R.make_mask(nb, h, w, per_image)
    out = dict(z=z, ya=ya, yb=yb, mask=mask)
    for a in out.values():
        a.setflags(write=False)
    out["ref"] = R.evaluate(z, ya, yb, mask, WA, WB)
    return out


def _planar(a):
    return torch.tensor(a).to(DEV)


def _clast(a, lead=0):
    """The head's layout: memory [B][H][W][K] viewed as [B, K, H, W]; with `lead`, a batch slice z[lead:] of a larger tensor."""
    t = torch.tensor(a).to(DEV).permute(0, 2, 3, 1)
    big = torch.full((lead + t.shape[0],) + tuple(t.shape[1:]), 7.0, device=DEV)
    big[lead:] = t
    return big.permute(0, 3, 1, 2)[lead:]


def _offset(a):
    """Planar at a 4-byte offset from a 16-byte boundary: never the 16-byte path."""
    flat = torch.empty(a.size + 1, device=DEV, dtype=torch.float32)[1:]
    flat.copy_(torch.tensor(a).reshape(-1))
    return flat.view(a.shape)


def _logits(z, layout):
    t = {"planar": _planar, "clast": _clast, "slice": lambda a: _clast(a, 2), "offset": _offset}[layout](z)
    return t.detach().requires_grad_(True)


def _labels(y, kind):
    return torch.tensor(y.astype(np.uint8) if kind == "uint8" else y).to(DEV)


def _run(z, ya, yb, mask, wa=WA, wb=WB, fused=True):
    """(out [5] = L and the four terms, counts [2], gradient) as numpy, from one forward + backward of the module."""
    from losses.copy_paste import CopyPasteLoss
    mod = CopyPasteLoss(z.shape[1] - 1, fused=fused)
    z.grad = None
    loss = mod(z, ya, yb, mask, wa, wb)
    loss.backward()
    out = torch.cat([loss.detach().reshape(1), mod.last_terms.reshape(4)])
    return out.cpu().numpy(), mod.last_counts.cpu().numpy(), z.grad.cpu().numpy().astype(np.float64)


def _check(res, ref, what):
    out, counts, g = res
    assert tuple(int(c) for c in counts) == ref["counts"], (what, counts, ref["counts"])  # exactly
    assert np.isfinite(out).all() and np.isfinite(g).all(), what
    ratios = []
    for name, got, want, mag in [("L", out[0], ref["value"], ref["value_mag"])] + \
            [(n, out[1 + i], ref["terms"][i], ref["term_mags"][i]) for i, n in enumerate(("D_A", "C_A", "D_B", "C_B"))]:
        err, bound = abs(float(got) - want), 2e-6 * mag
        ratios.append(f"{name} {err / max(bound, 1e-300):.3f}")
        assert err <= bound, (what, name, float(got), want, err, bound)
    gbound = 2e-6 * ref["grad_mag"] + 1e-12
    gerr = np.abs(g - ref["grad"])
    print(f"{what}: err/bound  {'  '.join(ratios)}  gradient {(gerr / gbound).max():.3f}")
    assert (gerr <= gbound).all(), (what, (gerr / gbound).max())


# ---------------------------------------------------------------- the loss against the restatement
@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("label_kind", LABELS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k1", K1S)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_counts_terms_value_and_gradient_against_restatement(shape, k1, layout, label_kind, mask_kind):
    nb, h, w = shape
    c = _case(nb, h, w, k1, mask_kind == "bhw")
    res = _run(_logits(c["z"], layout), _labels(c["ya"], label_kind), _labels(c["yb"], label_kind), torch.tensor(c["mask"]).to(DEV))
    _check(res, c["ref"], f"{shape} k1={k1} {layout} {label_kind} mask {mask_kind}")
    if nb * h * w > 1:
        assert min(c["ref"]["counts"]) > 0  # both regions populated


@pytest.mark.parametrize("shape,k1", [((4, 37, 61), 4), ((2, 336, 544), 8)], ids=["scalar", "quad"])
def test_tensor_op_form_within_the_same_bounds(shape, k1):
    nb, h, w = shape
    c = _case(nb, h, w, k1, False)
    res = _run(_logits(c["z"], "clast"), _labels(c["ya"], "int64"), _labels(c["yb"], "uint8"), torch.tensor(c["mask"]).to(DEV),
               fused=False)
    _check(res, c["ref"], f"fused=False {shape} k1={k1}")


def test_tensor_op_form_serves_more_than_eight_classes():
    nb, k1, h, w = 2, 11, 12, 20
    z, ya, yb = R.make_case(nb, k1, h, w)
    mask = R.make_mask(nb, h, w)
    _check(_run(_logits(z, "planar"), _labels(ya, "int64"), _labels(yb, "int64"), torch.tensor(mask).to(DEV), fused=False),
           R.evaluate(z, ya, yb, mask, WA, WB), "fused=False, 11 classes")
    with pytest.raises(mia_hip.MiaError):
        ops.CopyPasteLossFn.apply(_logits(z, "planar"), _labels(ya, "int64"), _labels(yb, "int64"), torch.tensor(mask).to(DEV), 1.0, 1.0,
                                  1e-10)


# ---------------------------------------------------------------- edge cases
@pytest.mark.parametrize("shape", [(4, 37, 61), (2, 336, 544)], ids=["scalar", "quad"])
@pytest.mark.parametrize("fill", [1, 0], ids=["all_ones", "all_zeros"])
def test_empty_region_gives_zero_terms_and_no_gradient(shape, fill):
    nb, h, w = shape
    c = _case(nb, h, w, 4, False)
    mask = np.full((h, w), fill, np.uint8)
    z, ya, yb, mk = _logits(c["z"], "clast"), _labels(c["ya"], "int64"), _labels(c["yb"], "int64"), torch.tensor(mask).to(DEV)
    res = _run(z, ya, yb, mk, 1.0, 1.0)
    _check(res, R.evaluate(c["z"], c["ya"], c["yb"], mask, 1.0, 1.0), f"mask all {fill} {shape}")
    empty = 3 if fill else 1  # out = {L, D_A, C_A, D_B, C_B}: the empty region's two terms
    assert res[0][empty] == 0.0 and res[0][empty + 1] == 0.0 and int(res[1][1 if fill else 0]) == 0
    # the empty region contributes exactly nothing: its weight and its label map do not change a bit of the gradient, and the
    # gradient is that of the single-source case (one label map, one weight)
    wa2, wb2 = (1.0, 0.0) if fill else (0.0, 1.0)
    other = _run(z, ya, yb, mk, wa2, wb2)
    single = _run(z, ya if fill else yb, ya if fill else yb, mk, wa2, wb2)
    assert np.array_equal(res[2], other[2]) and np.array_equal(res[2], single[2]) and res[2].any()
    assert np.array_equal(res[0], other[0]) and np.array_equal(res[0], single[0])


@pytest.mark.parametrize("shape", [(4, 37, 61), (2, 336, 544)], ids=["scalar", "quad"])
def test_zero_weights_give_exactly_zero_gradients(shape):
    nb, h, w = shape
    c = _case(nb, h, w, 4, True)
    out, counts, g = _run(_logits(c["z"], "planar"), _labels(c["ya"], "uint8"), _labels(c["yb"], "uint8"),
                          torch.tensor(c["mask"]).to(DEV), 0.0, 0.0)
    assert out[0] == 0.0 and not g.any() and np.isfinite(g).all()
    ref = R.evaluate(c["z"], c["ya"], c["yb"], c["mask"], 0.0, 0.0)
    for i in range(4):  # the unweighted terms are still reported
        assert abs(float(out[1 + i]) - ref["terms"][i]) <= 2e-6 * ref["term_mags"][i] and out[1 + i] > 0


@pytest.mark.parametrize("shape", [(4, 37, 61), (2, 336, 544)], ids=["scalar", "quad"])
def test_class_absent_from_a_region(shape):
    nb, h, w = shape
    for k1 in (2, 8):
        c = _case(nb, h, w, k1, False, True)
        assert not (c["ya"] == 0).any() and not (c["yb"] == k1 - 1).any()
        _check(_run(_logits(c["z"], "clast"), _labels(c["ya"], "int64"), _labels(c["yb"], "int64"), torch.tensor(c["mask"]).to(DEV)),
               c["ref"], f"absent class {shape} k1={k1}")


@pytest.mark.parametrize("shape", [(1, 3, 5), (2, 8, 16)], ids=["scalar", "quad"])
def test_saturated_logits_stay_finite(shape):
    nb, h, w = shape
    z, ya, yb = R.saturated_case(nb, 3, h, w)
    mask = R.make_mask(nb, h, w)
    ref = R.evaluate(z, ya, yb, mask, WA, WB)
    assert ref["terms"][1] > 10 and ref["terms"][3] > 10  # labels that disagree with a one-hot soft-max: terms of 160
    _check(_run(_logits(z, "planar"), _labels(ya, "int64"), _labels(yb, "int64"), torch.tensor(mask).to(DEV)), ref, f"saturated {shape}")


# ---------------------------------------------------------------- label range
@pytest.mark.parametrize("label_kind", LABELS)
@pytest.mark.parametrize("shape", [(4, 37, 61), (2, 336, 544)], ids=["scalar", "quad"])
def test_only_the_selected_label_is_read(shape, label_kind):
    nb, h, w = shape
    k1 = 4
    c = _case(nb, h, w, k1, False)
    m = np.broadcast_to(c["mask"] != 0, (nb, h, w))
    junk = 255 if label_kind == "uint8" else -(1 << 40)
    z, mk = _logits(c["z"], "clast"), torch.tensor(c["mask"]).to(DEV)
    ops.check_labels()  # nothing pending
    clean = _run(z, _labels(c["ya"], label_kind), _labels(c["yb"], label_kind), mk)
    # out-of-range values wherever a map is NOT selected: no bit of any output changes, and no verdict
    ya_j, yb_j = np.where(m, c["ya"], junk), np.where(m, junk, c["yb"])
    if label_kind == "uint8":
        ta, tb = torch.tensor(ya_j.astype(np.uint8)).to(DEV), torch.tensor(yb_j.astype(np.uint8)).to(DEV)
    else:
        ta, tb = torch.tensor(ya_j).to(DEV), torch.tensor(yb_j).to(DEV)
    dirty = _run(z, ta, tb, mk)
    assert np.array_equal(clean[0].view(np.int32), dirty[0].view(np.int32)) and np.array_equal(clean[1], dirty[1])
    assert np.array_equal(clean[2], dirty[2])
    ops.check_labels()
    # one such value in a SELECTED position: NaN results and the sticky verdict
    pos = np.argwhere(m)[len(np.argwhere(m)) // 2]
    bad_a = c["ya"].copy()
    bad_a[tuple(pos)] = k1 if label_kind == "uint8" else (1 << 32)  # the low word alone would be class 0
    out, counts, g = _run(z, _labels(bad_a, label_kind), _labels(c["yb"], label_kind), mk)
    assert np.isnan(out).all() and np.isnan(g).all()
    _run(z, _labels(c["ya"], label_kind), _labels(c["yb"], label_kind), mk)  # a clean call in between does not erase it
    with pytest.raises(mia_hip.MiaError):
        ops.check_labels()
    ops.check_labels()  # read and cleared
    again = _run(z, _labels(c["ya"], label_kind), _labels(c["yb"], label_kind), mk)
    assert np.array_equal(clean[0].view(np.int32), again[0].view(np.int32)) and np.array_equal(clean[2], again[2])


# ---------------------------------------------------------------- determinism and paths
@pytest.mark.parametrize("k1", [3, 8])
@pytest.mark.parametrize("shape", [(4, 36, 60), (2, 336, 544)], ids=["small", "full"])
def test_runs_and_paths_give_the_same_bits(shape, k1):
    """hw % 4 == 0 in both shapes: `planar` takes the 16-byte path, `offset` (and misaligned labels or mask) the scalar one."""
    nb, h, w = shape
    c = _case(nb, h, w, k1, True)
    ya, yb, mk = _labels(c["ya"], "int64"), _labels(c["yb"], "int64"), torch.tensor(c["mask"]).to(DEV)
    zp = _logits(c["z"], "planar")
    first = _run(zp, ya, yb, mk)
    _check(first, c["ref"], f"paths {shape} k1={k1}")
    for _ in range(2):
        again = _run(zp, ya, yb, mk)
        assert np.array_equal(first[0].view(np.int32), again[0].view(np.int32)) and np.array_equal(first[2], again[2])
    scalar = _run(_logits(c["z"], "offset"), ya, yb, mk)
    assert np.array_equal(first[0].view(np.int32), scalar[0].view(np.int32)) and np.array_equal(first[1], scalar[1])
    assert np.array_equal(first[2], scalar[2])
    # a mask at an odd address sends aligned logits down the scalar path too
    odd = torch.empty(mk.numel() + 1, device=DEV, dtype=torch.uint8)[1:].view(mk.shape)
    odd.copy_(mk)
    assert odd.data_ptr() % 4 != 0
    via_mask = _run(zp, ya, yb, odd)
    assert np.array_equal(first[0].view(np.int32), via_mask[0].view(np.int32)) and np.array_equal(first[2], via_mask[2])
    # channels-last: the same pixels per thread and the same sums
    cl = _run(_logits(c["z"], "clast"), ya, yb, mk)
    assert np.array_equal(first[0].view(np.int32), cl[0].view(np.int32)) and np.array_equal(first[2], cl[2])


def test_gradient_scales_with_grad_out_and_by_products_are_device_tensors():
    from losses.copy_paste import CopyPasteLoss
    c = _case(4, 37, 61, 4, False)
    z = _logits(c["z"], "clast")
    mod = CopyPasteLoss(3)
    loss = mod(z, _labels(c["ya"], "int64"), _labels(c["yb"], "int64"), torch.tensor(c["mask"]).to(DEV), WA, WB)
    assert loss.is_cuda and mod.last_terms.is_cuda and tuple(mod.last_terms.shape) == (4,) and mod.last_counts.dtype == torch.int64
    (3.0 * loss).backward()
    g3 = z.grad.cpu().numpy().astype(np.float64)
    assert (np.abs(g3 - 3.0 * c["ref"]["grad"]) <= 3.0 * (2e-6 * c["ref"]["grad_mag"] + 1e-12)).all()


# ---------------------------------------------------------------- the mix
def _payloads(shape, seed):
    """fp32 tensors of random BIT PATTERNS (NaNs of every payload, infinities, denormals) with quiet / signalling NaNs and -0.0 planted."""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g, dtype=torch.int64).to(torch.int32)
    flat = bits.view(-1)
    special = torch.tensor([0x7FC00001, 0x7F800001, -0x7FFFFFFF - 1, 0x7FFFFFFF, -1, 0x7F800000], dtype=torch.int64).to(torch.int32)
    flat[:min(len(special), flat.numel())] = special[:flat.numel()]
    return bits.view(torch.float32).to(DEV)


@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 5, 7), (3, 2, 8, 12), (2, 4, 64, 96)], ids=lambda s: "x".join(map(str, s)))
def test_mix_equals_torch_where_bit_for_bit(shape, mask_kind):
    nb, ch, h, w = shape
    fg, bg = _payloads(shape, 1), _payloads(shape, 2)
    assert torch.isnan(fg).any() and (fg.numel() < 6 or (fg.view(torch.int32) == -0x7FFFFFFF - 1).any())  # NaN payloads, -0.0
    mask = torch.tensor(R.make_mask(nb, h, w, mask_kind == "bhw")).to(DEV)
    m4 = (mask != 0)[None, None] if mask.ndim == 2 else (mask != 0)[:, None]
    want = torch.where(m4, fg, bg).view(torch.int32)
    assert np.array_equal(want.cpu().numpy(), R.mix(fg.cpu().numpy().view(np.int32), bg.cpu().numpy().view(np.int32), mask.cpu().numpy()))
    got = ops.bcp_mix(fg, bg, mask)
    assert torch.equal(got.view(torch.int32), want)
    # into a batch slice of a larger tensor: the rows around it keep their bits
    big = torch.full((nb + 3, ch, h, w), 5.0, device=DEV)
    ret = ops.bcp_mix(fg, bg, mask, out=big[2:2 + nb])
    assert ret.data_ptr() == big[2:].data_ptr() and torch.equal(big[2:2 + nb].view(torch.int32), want)
    assert (big[:2] == 5.0).all() and (big[2 + nb:] == 5.0).all()
    # an unaligned base (inputs and output 4 bytes off a 16-byte boundary): the scalar path, the same bits
    def off(t):
        flat = torch.empty(t.numel() + 1, device=DEV, dtype=torch.float32)[1:]
        flat.view(torch.int32).copy_(t.reshape(-1).view(torch.int32))
        return flat.view(t.shape)
    out = off(torch.zeros_like(fg))
    ops.bcp_mix(off(fg), off(bg), mask, out=out)
    assert out.data_ptr() % 16 == 4 and torch.equal(out.view(torch.int32), want)


def test_mix_argument_checks():
    fg, bg = torch.zeros(2, 1, 4, 4, device=DEV), torch.ones(2, 1, 4, 4, device=DEV)
    with pytest.raises(mia_hip.MiaError):
        ops.bcp_mix(fg, bg, torch.ones(4, 4, device=DEV))  # a float mask
    with pytest.raises(mia_hip.MiaError):
        ops.bcp_mix(fg, bg, torch.ones(3, 4, 4, device=DEV, dtype=torch.uint8))
    with pytest.raises(mia_hip.MiaError):
        ops.bcp_mix(fg, bg[:1], torch.ones(4, 4, device=DEV, dtype=torch.uint8))
    with pytest.raises(mia_hip.MiaError):
        ops.bcp_mix(fg, bg, torch.ones(4, 4, device=DEV, dtype=torch.uint8), out=torch.zeros(2, 1, 4, 8, device=DEV)[..., ::2])
