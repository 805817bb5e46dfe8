"""csrc/w2s.hip on the GPU against the float64 restatement (tests/_w2s_ref.py): the pseudo-label code of the weak view, the CutMix of
a batch with itself bit for bit against `torch.where`, and counts, CE, Dice, value and gradient of the weak-to-strong loss in every
layout, on the 16-byte and the scalar path, with every mask shape and permutation; ties, saturated logits, the empty mask, tau = 0,
single-term weights, an absent class, the run-time `dyn` buffer, determinism, batch independence, the perm guard, and the tensor-op
form (`fused=False`).

Codes are compared EXACTLY outside ambiguous pixels (|max p - tau| < 1e-6 in float64; tests/test_w2s_host.py caps their share at 5e-4
on the reference alone) and counts EXACTLY; values and gradients are checked against the restatement evaluated with the device's own
codes.  Bounds, with the project's constant 2e-6 (32 roundings x 2^-24, tests/test_gpu_consistency.py, tests/test_gpu_cps.py,
tests/test_gpu_bcp.py) times the magnitudes the restatement returns:
    |CE - ref| <= 2e-6 * (1/N) sum m (1 + |zs_y - max zs|)                          the CPS magnitude
    |D - ref|  <= 2e-6 * (1/K) sum_k (2 I_k / den + (2 I_k + s) Z_k / den^2)        the BCP quotient magnitude
    |L - ref|  <= 2e-6 * weight (ce_w magCE + dice_w magD)
    |g - ref|  <= 2e-6 * (sum of the absolute values of the gradient's terms) + 1e-12      per element
The kernels evaluate the soft-max in double from fp32 expf, add per thread and per wave in double and round a block's sum to a
(hi, lo) float pair, as csrc/bcp.hip does; the gradient is one fp32 rounding of a double expression of that soft-max and of
coefficients rounded once to fp32.
Measured on an MI355X over every case below: the error of L, CE and D is at most 0.033 of its bound, the gradient error at most
0.059; for the tensor-op form (`fused=False`, fp32 torch ops) 0.034 and 0.20.
What the D bound does not cover is the fp32 rounding of D itself, 2^-25 |D|: a call whose kept pixels nearly all contradict their
labels has D near 1 and a magnitude near 0.  A one-pixel input of that kind was met while this file was written ((1, 1, 1), k1 = 8,
strong logits that did not follow the weak ones: |D - ref| = 2.1e-8, a correctly rounded fp32 D, against a bound of 7.3e-9).  The
generator (`_w2s_ref.make_case`) derives the strong logits from the weak ones, strong = weak + 1.5 N(0, 1), as its text says; there
the magnitude is a few tenths."""
import functools
import itertools

import numpy as np
import pytest
import torch

import _w2s_ref as R
import mia_hip
from mia_hip import ops

pytestmark = pytest.mark.gpu

SHAPES = R.SHAPES  # hw odd: the one-pixel loads; the last: 16-byte units, several slabs
K1S = R.K1S
LAYOUTS = ["planar", "clast", "slice", "offset"]
# (mask, perm): no mix; every mask shape with every permutation; and one operand alone, which is no mix either
MIXES = [("none", "none")] + list(itertools.product(["hw", "bhw"], ["identity", "reverse", "fixed"])) + [("hw", "none"), ("none", "reverse")]
DEV = "cuda:0"
TAU = R.thresholds()[0]
WEIGHT, CE_W, DICE_W = 0.7, 1.0, 0.5
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) and isinstance(v[0], int) else ("+".join(v) if isinstance(v, tuple) else str(v))


@functools.lru_cache(maxsize=4)
def _inputs(nb, h, w, k1, kind="normal"):
    """(zw, zs), read-only."""
    zw, zs = {"normal": lambda: R.make_case(nb, k1, h, w), "absent": lambda: R.make_case(nb, k1, h, w, absent=True),
              "tie": lambda: R.tie_case(nb, k1, h, w), "saturated": lambda: R.saturated_case(nb, k1, h, w)}[kind]()
    zw.setflags(write=False)
    zs.setflags(write=False)
    return zw, zs


@functools.lru_cache(maxsize=2)
def _ref(nb, h, w, k1, mask_kind, perm_kind, kind="normal", tau=TAU, weight=WEIGHT, cw=CE_W, dw=DICE_W):
    """The float64 reference with the float64 codes, computed once per case and never modified."""
    zw, zs = _inputs(nb, h, w, k1, kind)
    code = R.code_of(zw, tau)
    return code, R.evaluate(zs, code, R.make_mask(nb, h, w, mask_kind), R.make_perm(nb, perm_kind), weight, cw, dw)


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


def _logits(z, layout, grad=True):
    t = {"planar": _planar, "clast": _clast, "slice": lambda a: _clast(a, 2), "offset": _offset}[layout](z)
    return t.detach().requires_grad_(grad)


def _dyn(weight, tau):
    return torch.tensor([weight, tau], device=DEV, dtype=torch.float32)


def _dev(a):
    return None if a is None else torch.tensor(a).to(DEV)


def _device_code(zw, tau, layout="planar", dyn=None):
    """The device's code map (tensor) and its kept count, after the EXACT comparison with the restatement outside ambiguous pixels."""
    code, kept = ops.w2s_labels(_logits(zw, layout, grad=False), _dyn(1.0, tau) if dyn is None else dyn)
    got = code.cpu().numpy()
    y, keep = R.decode(got)
    assert np.array_equal(y, R.labels(zw)) and not (got & 0x78).any()  # labels exactly, no stray bit
    amb = R.ambiguous(zw, tau)
    assert amb.mean() <= 5e-4, "the inputs put too many pixels on the threshold"
    assert np.array_equal(keep[~amb], (R.max_prob(zw) >= tau)[~amb])
    assert int(kept) == int(keep.sum())  # exactly the device map's own sum
    return code, got


def _run(zs, code, mask, perm, dyn, cw=CE_W, dw=DICE_W, fused=True):
    """(out [4] = L, CE, D, weight; counts [2]; gradient) as numpy, from one forward + backward of the module."""
    from losses.weak_strong import WeakToStrongLoss
    mod = WeakToStrongLoss(zs.shape[1] - 1, cw, dw, fused=fused)
    zs.grad = None
    loss = mod(zs, code, mask, perm, dyn=dyn)
    loss.backward()
    out = torch.stack([loss.detach(), mod.last_ce, mod.last_dice, dyn[0] if dyn is not None else torch.ones((), device=DEV)])
    counts = torch.stack([mod.last_kept, mod.last_pasted])
    return out.cpu().numpy(), counts.cpu().numpy(), zs.grad.cpu().numpy().astype(np.float64)


RATIOS = {"value": 0.0, "grad": 0.0}       # the largest error / bound ratios of the kernels so far in this session
RATIOS_SOFT = {"value": 0.0, "grad": 0.0}  # and of the tensor-op form


def _check(res, ref, what, RATIOS=RATIOS):
    out, counts, g = res
    assert tuple(int(c) for c in counts) == ref["counts"], (what, counts, ref["counts"])  # exactly
    assert np.isfinite(out).all() and np.isfinite(g).all(), what
    ratios = []
    for name, got, want, mag in (("L", out[0], ref["value"], ref["value_mag"]), ("CE", out[1], ref["ce"], ref["ce_mag"]),
                                 ("D", out[2], ref["dice"], ref["dice_mag"])):
        err, bound = abs(float(got) - want), 2e-6 * mag
        r = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        ratios.append(f"{name} {r:.3f}")
        RATIOS["value"] = max(RATIOS["value"], r)
        assert err <= bound, (what, name, float(got), want, err, bound)
    gbound = 2e-6 * ref["grad_mag"] + 1e-12
    gerr = np.abs(g - ref["grad"])
    RATIOS["grad"] = max(RATIOS["grad"], float((gerr / gbound).max()))
    print(f"{what}: err/bound  {'  '.join(ratios)}  gradient {(gerr / gbound).max():.3f}   largest so far {RATIOS}")
    assert (gerr <= gbound).all(), (what, (gerr / gbound).max())
    assert not g[np.broadcast_to(ref["grad_mag"].sum(1, keepdims=True) == 0, g.shape)].any()  # a dropped pixel: exactly zero


def _case_ref(nb, h, w, k1, mask_kind, perm_kind, got_code, kind="normal", tau=TAU, weight=WEIGHT, cw=CE_W, dw=DICE_W):
    """The reference evaluated with the device's own codes (the cached one when they are the float64 codes)."""
    code, ref = _ref(nb, h, w, k1, mask_kind, perm_kind, kind, tau, weight, cw, dw)
    if np.array_equal(code, got_code):
        return ref
    zs = _inputs(nb, h, w, k1, kind)[1]
    return R.evaluate(zs, got_code, R.make_mask(nb, h, w, mask_kind), R.make_perm(nb, perm_kind), weight, cw, dw)


def _perm_arg(nb, perm_kind):
    p = R.make_perm(nb, perm_kind)
    return None if p is None else p.tolist()


# ---------------------------------------------------------------- the labels against the restatement
@pytest.mark.parametrize("shape,k1,tau,layout", list(itertools.product(SHAPES, K1S, [0.0] + R.thresholds(), LAYOUTS)), ids=_ids)
def test_codes_and_kept_count_against_restatement(shape, k1, tau, layout):
    nb, h, w = shape
    zw = _inputs(nb, h, w, k1)[0]
    _, got = _device_code(zw, tau, layout)
    if tau == 0.0:
        assert (got >> 7).all()  # tau = 0 keeps every pixel


# ---------------------------------------------------------------- the loss against the restatement
@pytest.mark.parametrize("shape,k1,mix,layout", list(itertools.product(SHAPES, K1S, MIXES, LAYOUTS)), ids=_ids)
def test_counts_terms_value_and_gradient_against_restatement(shape, k1, mix, layout):
    nb, h, w = shape
    zw, zs = _inputs(nb, h, w, k1)
    code, got = _device_code(zw, TAU)
    ref = _case_ref(nb, h, w, k1, mix[0], mix[1], got)
    res = _run(_logits(zs, layout), code, _dev(R.make_mask(nb, h, w, mix[0])), _perm_arg(nb, mix[1]), _dyn(WEIGHT, TAU))
    _check(res, ref, f"{shape} k1={k1} {layout} mask {mix[0]} perm {mix[1]}")
    assert res[0][3] == np.float32(WEIGHT) and 0 < ref["counts"][0] <= nb * h * w  # some pixel is kept in every case
    if "none" in mix:
        assert ref["counts"][1] == 0
    elif nb * h * w > 1:
        assert 0 < ref["counts"][1] < nb * h * w


@pytest.mark.parametrize("shape,k1", [((4, 37, 61), 3), ((2, 336, 544), 8)], ids=["scalar", "quad"])
def test_tensor_op_form_within_the_same_bounds(shape, k1):
    nb, h, w = shape
    zw, zs = _inputs(nb, h, w, k1)
    code, got = _device_code(zw, TAU)
    ref = _case_ref(nb, h, w, k1, "bhw", "fixed", got)
    res = _run(_logits(zs, "clast"), code, _dev(R.make_mask(nb, h, w, "bhw")), _perm_arg(nb, "fixed"), _dyn(WEIGHT, TAU), fused=False)
    _check(res, ref, f"fused=False {shape} k1={k1}", RATIOS_SOFT)
    from losses.weak_strong import pseudo_label_code
    soft = pseudo_label_code(_planar(zw), TAU).cpu().numpy()
    amb = R.ambiguous(zw, TAU)
    assert np.array_equal(soft[~amb], R.code_of(zw, TAU)[~amb])


def test_tensor_op_form_serves_more_than_eight_classes():
    from losses.weak_strong import pseudo_label_code
    nb, k1, h, w = 2, 11, 12, 20
    zw, zs = R.make_case(nb, k1, h, w)
    code = pseudo_label_code(_planar(zw), 0.0)
    z = _logits(zs, "planar")
    with pytest.raises(mia_hip.MiaError):
        ops.WeakToStrongFn.apply(z, code, None, None, None, 1.0, 0.0, 1e-10)
    with pytest.raises(mia_hip.MiaError):
        ops.w2s_labels(_planar(zw))
    out, counts, g = _run(z, code, None, None, None, 1.0, 0.0, fused=False)
    want = torch.nn.functional.cross_entropy(torch.tensor(zs, dtype=torch.float64), torch.tensor(zw).argmax(1)).item()
    assert abs(float(out[0]) - want) <= 2e-5 * want and int(counts[0]) == nb * h * w


# ---------------------------------------------------------------- edge cases
@pytest.mark.parametrize("shape", [(4, 37, 61), (2, 336, 544)], ids=["scalar", "quad"])
@pytest.mark.parametrize("k1", K1S)
def test_tied_logits(shape, k1):
    nb, h, w = shape
    zw, zs = _inputs(nb, h, w, k1, "tie")
    top2 = np.sort(zw, 1)[:, -2:]
    assert k1 == 1 or (top2[:, 0] == top2[:, 1]).mean() > 0.1  # many tied arg-maxes
    for tau in [0.0] + R.thresholds():
        code, got = _device_code(zw, tau, "clast")
        ref = _case_ref(nb, h, w, k1, "bhw", "fixed", got, "tie", tau)
        _check(_run(_logits(zs, "clast"), code, _dev(R.make_mask(nb, h, w, "bhw")), _perm_arg(nb, "fixed"), _dyn(WEIGHT, tau)), ref,
               f"ties {shape} k1={k1} tau={tau}")


@pytest.mark.parametrize("shape", [(1, 3, 5), (2, 8, 16)], ids=["scalar", "quad"])
def test_saturated_logits_stay_finite(shape):
    nb, h, w = shape
    zw, zs = _inputs(nb, h, w, 3, "saturated")
    code, got = _device_code(zw, TAU)
    assert (got >> 7).all()
    ref = _case_ref(nb, h, w, 3, "hw", "reverse", got, "saturated")
    assert ref["ce"] > 10  # labels whose soft-max is 0 in fp32: terms of 160
    _check(_run(_logits(zs, "planar"), code, _dev(R.make_mask(nb, h, w, "hw")), _perm_arg(nb, "reverse"), _dyn(WEIGHT, TAU)), ref,
           f"saturated {shape}")


@pytest.mark.parametrize("shape", [(4, 37, 61), (2, 336, 544)], ids=["scalar", "quad"])
def test_empty_mask_gives_zero_and_no_gradient(shape):
    nb, h, w = shape
    zw, zs = _inputs(nb, h, w, 3)
    code, got = _device_code(zw, 1.5)  # no soft-max reaches 1.5
    assert not (got >> 7).any()
    out, counts, g = _run(_logits(zs, "clast"), code, _dev(R.make_mask(nb, h, w, "bhw")), _perm_arg(nb, "reverse"), _dyn(WEIGHT, 1.5),
                          1.0, 1.0)
    assert out[0] == 0.0 and out[1] == 0.0 and out[2] == 0.0 and int(counts[0]) == 0 and int(counts[1]) > 0
    assert not g.any() and np.isfinite(g).all()


@pytest.mark.parametrize("shape", [(4, 37, 61), (2, 336, 544)], ids=["scalar", "quad"])
@pytest.mark.parametrize("cw,dw", [(1.0, 0.0), (0.0, 1.0)], ids=["ce_only", "dice_only"])
def test_single_term_weights_at_tau_zero(shape, cw, dw):
    nb, h, w = shape
    zw, zs = _inputs(nb, h, w, 3)
    code, got = _device_code(zw, 0.0)
    ref = _case_ref(nb, h, w, 3, "hw", "fixed", got, "normal", 0.0, WEIGHT, cw, dw)
    assert ref["counts"][0] == nb * h * w
    res = _run(_logits(zs, "clast"), code, _dev(R.make_mask(nb, h, w, "hw")), _perm_arg(nb, "fixed"), _dyn(WEIGHT, 0.0), cw, dw)
    _check(res, ref, f"cw={cw} dw={dw} {shape}")
    assert res[0][1] > 0 and res[0][2] > 0  # the unweighted terms are both reported
    if dw == 0.0:  # identity perm at tau = 0: F.cross_entropy on the weak arg-max
        plain = _run(_logits(zs, "clast"), code, None, None, None, 1.0, 0.0)
        want = torch.nn.functional.cross_entropy(torch.tensor(zs, dtype=torch.float64), torch.tensor(zw).argmax(1)).item()
        assert abs(float(plain[0][0]) - want) <= 2e-6 * R.evaluate(zs, got)["ce_mag"]


@pytest.mark.parametrize("shape", [(4, 37, 61), (2, 336, 544)], ids=["scalar", "quad"])
def test_class_absent_from_the_kept_pixels(shape):
    nb, h, w = shape
    for k1 in (2, 8):
        zw, zs = _inputs(nb, h, w, k1, "absent")
        code, got = _device_code(zw, TAU)
        assert not ((got & 7) == k1 - 1).any()
        ref = _case_ref(nb, h, w, k1, "bhw", "reverse", got, "absent")
        _check(_run(_logits(zs, "clast"), code, _dev(R.make_mask(nb, h, w, "bhw")), _perm_arg(nb, "reverse"), _dyn(WEIGHT, TAU)), ref,
               f"absent class {shape} k1={k1}")


def test_dyn_is_read_when_the_kernels_run():
    nb, h, w, k1 = 4, 37, 61, 3
    zw, zs = _inputs(nb, h, w, k1)
    dyn = _dyn(WEIGHT, TAU)
    z, mask, perm = _logits(zs, "clast"), _dev(R.make_mask(nb, h, w, "bhw")), _perm_arg(nb, "fixed")
    code, got = _device_code(zw, TAU, dyn=dyn)
    first = _run(z, code, mask, perm, dyn)
    _check(first, _case_ref(nb, h, w, k1, "bhw", "fixed", got), "dyn, first values")
    tau2 = R.thresholds()[1]
    dyn.copy_(torch.tensor([0.25, tau2]))  # the same buffer, new values: nothing is rebuilt
    code2, got2 = _device_code(zw, tau2, dyn=dyn)
    assert (got2 >> 7).sum() < (got >> 7).sum()
    second = _run(z, code2, mask, perm, dyn)
    _check(second, _case_ref(nb, h, w, k1, "bhw", "fixed", got2, "normal", tau2, 0.25), "dyn, second values")
    assert second[0][3] == np.float32(0.25)


# ---------------------------------------------------------------- determinism, paths, batch independence
@pytest.mark.parametrize("k1", [3, 8])
@pytest.mark.parametrize("shape", [(4, 36, 60), (2, 336, 544)], ids=["small", "full"])
def test_runs_and_paths_give_the_same_bits(shape, k1):
    """hw % 4 == 0 in both shapes: `planar` takes the 16-byte path, `offset` (and a misaligned mask or code map) the scalar one."""
    nb, h, w = shape
    zw, zs = _inputs(nb, h, w, k1)
    code, got = _device_code(zw, TAU)
    for layout in LAYOUTS[1:]:  # the code does not depend on the layout or the path
        assert np.array_equal(_device_code(zw, TAU, layout)[1], got)
    mask, perm, dyn = _dev(R.make_mask(nb, h, w, "bhw")), _perm_arg(nb, "fixed"), _dyn(WEIGHT, TAU)
    zp = _logits(zs, "planar")
    first = _run(zp, code, mask, perm, dyn)
    _check(first, _case_ref(nb, h, w, k1, "bhw", "fixed", got), f"paths {shape} k1={k1}")
    same = lambda a, b: np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1]) and \
        np.array_equal(a[2], b[2])
    for _ in range(2):
        assert same(first, _run(zp, code, mask, perm, dyn))
    assert same(first, _run(_logits(zs, "offset"), code, mask, perm, dyn))
    odd = lambda t: torch.empty(t.numel() + 1, device=DEV, dtype=torch.uint8)[1:].view(t.shape).copy_(t)
    assert odd(mask).data_ptr() % 4 != 0
    assert same(first, _run(zp, code, odd(mask), perm, dyn))  # a mask at an odd address: aligned logits down the scalar path
    assert same(first, _run(zp, odd(code), mask, perm, dyn))  # likewise the code map
    assert same(first, _run(_logits(zs, "clast"), code, mask, perm, dyn))  # channels-last: the same pixels per thread, the same sums
    assert same(first, _run(zp, code, mask, torch.tensor(perm, dtype=torch.int32, device=DEV), dyn))  # a device perm, as it is


def test_code_of_an_image_does_not_depend_on_its_batch():
    nb, h, w, k1 = 4, 37, 61, 3
    zw = _inputs(nb, h, w, k1)[0]
    z = _planar(zw)
    dyn = _dyn(1.0, TAU)
    whole, kept = ops.w2s_labels(z, dyn)
    total = 0
    for n in range(nb):
        one, k = ops.w2s_labels(z[n:n + 1], dyn)
        assert torch.equal(one[0], whole[n])
        total += int(k)
    assert total == int(kept)
    none, kept0 = ops.w2s_labels(z)  # dyn None: tau = 0
    assert int(kept0) == nb * h * w and (none >> 7).all()


def test_gradient_scales_with_grad_out_and_by_products_are_device_tensors():
    from losses.weak_strong import WeakToStrongLoss
    nb, h, w, k1 = 4, 37, 61, 3
    zw, zs = _inputs(nb, h, w, k1)
    code, got = _device_code(zw, TAU)
    ref = _case_ref(nb, h, w, k1, "hw", "reverse", got)
    z = _logits(zs, "clast")
    mod = WeakToStrongLoss(k1 - 1, CE_W, DICE_W)
    loss = mod(z, code, _dev(R.make_mask(nb, h, w, "hw")), _perm_arg(nb, "reverse"), dyn=_dyn(WEIGHT, TAU))
    assert loss.is_cuda and mod.last_ce.is_cuda and mod.last_dice.is_cuda and mod.last_kept.dtype == torch.int64
    assert mod.last_pasted.is_cuda and tuple(ops.WeakToStrongFn.last_out.shape) == (4,)
    (3.0 * loss).backward()
    g3 = z.grad.cpu().numpy().astype(np.float64)
    assert (np.abs(g3 - 3.0 * ref["grad"]) <= 3.0 * (2e-6 * ref["grad_mag"] + 1e-12)).all()


# ---------------------------------------------------------------- the mix
def _payloads(shape, seed):
    """fp32 tensors of random BIT PATTERNS (NaNs of every payload, infinities, denormals) with quiet / signalling NaNs and -0.0 planted."""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g, dtype=torch.int64).to(torch.int32)
    flat = bits.view(-1)
    special = torch.tensor([0x7FC00001, 0x7F800001, -0x7FFFFFFF - 1, 0x7FFFFFFF, -1, 0x7F800000], dtype=torch.int64).to(torch.int32)
    flat[:min(len(special), flat.numel())] = special[:flat.numel()]
    return bits.view(torch.float32).to(DEV)


@pytest.mark.parametrize("perm_kind", ["identity", "reverse", "fixed"])
@pytest.mark.parametrize("mask_kind", ["hw", "bhw"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 5, 7), (3, 2, 8, 12), (4, 4, 64, 96)], ids=_ids)
def test_cutmix_equals_torch_where_bit_for_bit(shape, mask_kind, perm_kind):
    nb, ch, h, w = shape
    x = _payloads(shape, 1)
    assert torch.isnan(x).any() and (x.numel() < 6 or (x.view(torch.int32) == -0x7FFFFFFF - 1).any())  # NaN payloads, -0.0
    mask = _dev(R.make_mask(nb, h, w, mask_kind))
    perm = R.make_perm(nb, perm_kind)
    m4 = (mask != 0)[None, None] if mask.ndim == 2 else (mask != 0)[:, None]
    want = torch.where(m4, x[torch.tensor(perm).to(DEV)], x).view(torch.int32)
    assert np.array_equal(want.cpu().numpy(), R.mix(x.cpu().numpy().view(np.int32), perm, mask.cpu().numpy()))
    got = ops.cutmix_perm(x, perm.tolist(), mask)
    assert torch.equal(got.view(torch.int32), want)
    assert torch.equal(ops.cutmix_perm(x, torch.tensor(perm), mask).view(torch.int32), want)  # a CPU tensor
    assert torch.equal(ops.cutmix_perm(x, torch.tensor(perm, dtype=torch.int32).to(DEV), mask).view(torch.int32), want)
    # into a batch slice of a larger tensor: the rows around it keep their bits
    big = torch.full((nb + 3, ch, h, w), 5.0, device=DEV)
    ret = ops.cutmix_perm(x, perm.tolist(), mask, out=big[2:2 + nb])
    assert ret.data_ptr() == big[2:].data_ptr() and torch.equal(big[2:2 + nb].view(torch.int32), want)
    assert (big[:2] == 5.0).all() and (big[2 + nb:] == 5.0).all()
    # an unaligned base (input and output 4 bytes off a 16-byte boundary): the scalar path, the same bits
    def off(t):
        flat = torch.empty(t.numel() + 1, device=DEV, dtype=torch.float32)[1:]
        flat.view(torch.int32).copy_(t.reshape(-1).view(torch.int32))
        return flat.view(t.shape)
    out = off(torch.zeros_like(x))
    ops.cutmix_perm(off(x), perm.tolist(), mask, out=out)
    assert out.data_ptr() % 16 == 4 and torch.equal(out.view(torch.int32), want)
    ops.check_perm()  # nothing raised


def test_out_of_range_device_perm_pairs_the_image_with_itself_and_raises_the_verdict():
    nb, ch, h, w, k1 = 4, 2, 8, 12, 3
    ops.check_perm()  # nothing pending
    x = _payloads((nb, ch, h, w), 3)
    mask = _dev(R.make_mask(nb, h, w, "bhw"))
    bad = torch.tensor([1, nb, -1, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    fixed = [1, 1, 2, 3]  # what the guard makes of it: perm[n] = n for the three bad entries
    want = ops.cutmix_perm(x, fixed, mask)
    ops.check_perm()
    got = ops.cutmix_perm(x, bad, mask)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    ops.cutmix_perm(x, fixed, mask)  # a clean call in between does not erase the verdict
    with pytest.raises(mia_hip.MiaError):
        ops.check_perm()
    ops.check_perm()  # read and cleared
    # the loss: the same guard, forward and backward
    zw, zs = R.make_case(nb, k1, h, w)
    code, got_code = _device_code(zw, TAU)
    dyn = _dyn(WEIGHT, TAU)
    clean = _run(_logits(zs, "planar"), code, mask, fixed, dyn)
    _check(clean, R.evaluate(zs, got_code, mask.cpu().numpy(), np.array(fixed), WEIGHT, CE_W, DICE_W), "guarded perm")
    ops.check_perm()
    dirty = _run(_logits(zs, "planar"), code, mask, bad, dyn)
    assert np.array_equal(clean[0].view(np.int32), dirty[0].view(np.int32)) and np.array_equal(clean[2], dirty[2])
    assert np.array_equal(clean[1], dirty[1])
    with pytest.raises(mia_hip.MiaError):
        ops.check_perm()
    ops.check_perm()
    with pytest.raises(mia_hip.MiaError):  # a HOST perm is checked when it is given
        ops.cutmix_perm(x, [1, nb, 0, 2], mask)


def test_argument_checks():
    x = torch.zeros(2, 1, 4, 4, device=DEV)
    m = torch.ones(4, 4, device=DEV, dtype=torch.uint8)
    with pytest.raises(mia_hip.MiaError):
        ops.cutmix_perm(x, [1, 0], torch.ones(4, 4, device=DEV))  # a float mask
    with pytest.raises(mia_hip.MiaError):
        ops.cutmix_perm(x, [1, 0], torch.ones(3, 4, 4, device=DEV, dtype=torch.uint8))
    with pytest.raises(mia_hip.MiaError):
        ops.cutmix_perm(x, [1, 0, 1], m)
    with pytest.raises(mia_hip.MiaError):
        ops.cutmix_perm(x, torch.tensor([1, 0], device=DEV), m)  # a device perm must be int32
    with pytest.raises(mia_hip.MiaError):
        ops.cutmix_perm(x, [1, 0], m, out=x)  # out overlaps x
    big = torch.zeros(3, 1, 4, 4, device=DEV)
    with pytest.raises(mia_hip.MiaError):
        ops.cutmix_perm(big[:2], [1, 0], m, out=big[1:])  # one shared image
    with pytest.raises(mia_hip.MiaError):
        ops.cutmix_perm(x, [1, 0], m, out=torch.zeros(2, 1, 4, 8, device=DEV)[..., ::2])
    z = torch.zeros(2, 3, 4, 4, device=DEV)
    with pytest.raises(mia_hip.MiaError):
        ops.WeakToStrongFn.apply(z, torch.zeros(2, 4, 4, device=DEV, dtype=torch.int64), None, None, None, 1.0, 0.0, 1e-10)
    with pytest.raises(mia_hip.MiaError):
        ops.WeakToStrongFn.apply(z, torch.zeros(1, 4, 4, device=DEV, dtype=torch.uint8), None, None, None, 1.0, 0.0, 1e-10)
    with pytest.raises(mia_hip.MiaError):
        ops.w2s_labels(z, torch.zeros(3, device=DEV))  # dyn holds two values
    with pytest.raises(NotImplementedError):
        ops.w2s_labels(torch.zeros(2, 3, 4, 4, 4, device=DEV))
