"""csrc/cps.hip on the GPU against the float64 restatement (tests/_cps_ref.py): labels, flags, counts, the code map, values and both
gradients of cross pseudo supervision in every layout and on both the four-pixel and the one-pixel path; ties, saturated logits,
the empty mask, the run-time `dyn` buffer, determinism and batch independence.

Labels, the agreement count and (outside ambiguous pixels) the flags are compared EXACTLY.  The device's flags may differ from the
float64 ones only at ambiguous pixels, |max p - tau| < 1e-6 in float64, which are at most 5e-4 of any case; values and gradients are
checked against the restatement evaluated with the device's own flags.  Bounds (32 roundings x 2^-24 ~ 2e-6 of the magnitudes being
rounded, the constant of tests/test_gpu_consistency.py):
    |LA - ref| <= 2e-6 * (1/N) sum cb (1 + |za[yb] - max za|)                    likewise LB
    |g - ref|  <= 2e-6 * (w/N) flag (p_j + [j = y]) + 1e-12                       per element
The term is log sum_k exp(z_k - max) + (max - z_y): the second part is exact in double, the first carries expf's error (a few
2^-24 of a value <= ln K) and one double log; the gradient is one fp32 rounding of a double product of a soft-max with that error.
Measured on an MI355X over every case below: the value error is at most 0.025 of its bound, the gradient error at most 0.057."""
import functools

import numpy as np
import pytest
import torch

import _cps_ref as R
import mia_hip
from mia_hip import ops

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 1, 7), (4, 37, 61), (2, 336, 544)]  # hw odd: one pixel per thread; the last: four per thread, several slabs
K1S = [2, 3, 8]
LAYOUTS = ["planar", "clast", "mixed", "slice", "offset"]
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _case(nb, h, w, k1, ties=False):
    """Inputs and the float64 references that do not depend on the flags, computed once and never modified."""
    za, zb = R.tie_case(nb, k1, h, w) if ties else R.make_case(nb, k1, h, w)
    out = dict(za=za, zb=zb, ya=R.labels(za), yb=R.labels(zb), qa=R.max_prob(za), qb=R.max_prob(zb))
    for a in out.values():
        a.setflags(write=False)
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
    """Planar at a 4-byte offset from a 16-byte boundary: never the four-pixel path."""
    flat = torch.empty(a.size + 1, device=DEV, dtype=torch.float32)[1:]
    flat.copy_(torch.tensor(a).reshape(-1))
    return flat.view(a.shape)


def _inputs(c, layout):
    za = {"planar": _planar, "clast": _clast, "mixed": _clast, "slice": lambda a: _clast(a, 2), "offset": _offset}[layout](c["za"])
    zb = {"planar": _planar, "clast": _clast, "mixed": _planar, "slice": _clast, "offset": _planar}[layout](c["zb"])
    return za.detach().requires_grad_(True), zb.detach().requires_grad_(True)


def _run(za, zb, dyn):
    """(out [4], counts [3], code, gradient of za, gradient of zb) as numpy, from one forward + backward."""
    za.grad = zb.grad = None
    loss = ops.CrossPseudoFn.apply(za, zb, dyn)
    out, counts, code = ops.CrossPseudoFn.last_out, ops.CrossPseudoFn.last_counts, ops.CrossPseudoFn.last_code
    loss.backward()
    return (out.cpu().numpy(), counts.cpu().numpy(), code.cpu().numpy(), za.grad.cpu().numpy().astype(np.float64),
            zb.grad.cpu().numpy().astype(np.float64))


def _check(out, ga, gb, ref, what):
    assert np.isfinite(out).all() and np.isfinite(ga).all() and np.isfinite(gb).all(), what
    for side, got, g in (("a", out[1], ga), ("b", out[2], gb)):
        vb = 2e-6 * ref["value_mag_" + side]
        gbound = 2e-6 * ref["grad_mag_" + side] + 1e-12
        verr, gerr = abs(float(got) - ref["value_" + side]), np.abs(g - ref["grad_" + side])
        print(f"{what} L{side.upper()}={got:.9g} ref={ref['value_' + side]:.9g}  value err/bound={verr / max(vb, 1e-300):.3f}  "
              f"gradient max err/bound={(gerr / gbound).max():.3f}")
        assert verr <= vb, (what, side, verr, vb)
        assert (gerr <= gbound).all(), (what, side, (gerr / gbound).max())
    w = float(out[3])
    assert abs(float(out[0]) - w * (float(out[1]) + float(out[2]))) <= 4 * 2.0 ** -24 * abs(w) * (abs(out[1]) + abs(out[2])) + 1e-45


def _check_run(c, res, tau, w, what):
    """Everything one forward + backward must satisfy for flags at threshold `tau` and weight `w`."""
    out, counts, code, ga, gb = res
    ya, yb, ca, cb = R.decode(code)
    assert np.array_equal(ya, c["ya"]) and np.array_equal(yb, c["yb"]), what  # exactly
    assert int(counts[2]) == int((c["ya"] == c["yb"]).sum())
    for flag, q in ((ca, c["qa"]), (cb, c["qb"])):
        ambiguous = np.abs(q - tau) < 1e-6
        assert ambiguous.mean() <= 5e-4, "the inputs put too many pixels on the threshold"
        assert np.array_equal(flag[~ambiguous], (q >= tau)[~ambiguous]), what
    assert int(counts[0]) == int(ca.sum()) and int(counts[1]) == int(cb.sum())  # exactly the device map's own sums
    assert out[3] == np.float32(w)
    ref = R.evaluate(c["za"], c["zb"], tau, w, ca=ca, cb=cb)
    _check(out, ga, gb, ref, what)
    assert not ga[np.broadcast_to(~cb[:, None], ga.shape)].any()  # a dropped pixel: exactly zero
    assert not gb[np.broadcast_to(~ca[:, None], gb.shape)].any()
    return ca, cb


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k1", K1S)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_labels_flags_value_and_gradients_against_restatement(shape, k1, layout):
    nb, h, w = shape
    c = _case(nb, h, w, k1)
    za, zb = _inputs(c, layout)
    res = _run(za, zb, None)  # tau = 0, weight 1: the published CPS
    ca, cb = _check_run(c, res, 0.0, 1.0, f"plain {shape} k1={k1} {layout}")
    assert ca.all() and cb.all()
    assert int(res[1][0]) == int(res[1][1]) == nb * h * w
    for tau in R.thresholds():
        dyn = torch.tensor([1.0, tau], device=DEV)
        res = _run(za, zb, dyn)
        ca, cb = _check_run(c, res, tau, 1.0, f"masked {shape} k1={k1} {layout} tau={tau:.2f}")
        print(f"    kept: A {ca.mean():.3f}  B {cb.mean():.3f}")


def test_both_branches_of_the_mask_run():
    shares = []
    for k1 in K1S:
        c = _case(2, 336, 544, k1)
        for tau in R.thresholds():
            shares += [float((c["qa"] >= tau).mean()), float((c["qb"] >= tau).mean())]
    print("kept shares:", " ".join(f"{s:.3f}" for s in shares))
    assert 0.03 < min(shares) and max(shares) < 0.95, shares


@pytest.mark.parametrize("shape", [(4, 37, 61), (2, 336, 544)], ids=["scalar", "quad"])
def test_ties_go_to_the_lowest_index(shape):
    nb, h, w = shape
    c = _case(nb, h, w, 3, True)
    top2 = np.sort(c["za"], axis=1)[:, -2:]
    assert (top2[:, 0] == top2[:, 1]).mean() > 0.2  # 28 % of the pixels have a tied top-2
    assert np.array_equal(c["ya"], np.argmax(c["za"], axis=1)) and np.array_equal(c["yb"], np.argmax(c["zb"], axis=1))
    for layout in ("clast", "mixed"):
        za, zb = _inputs(c, layout)
        _check_run(c, _run(za, zb, None), 0.0, 1.0, f"ties {shape} {layout}")


@pytest.mark.parametrize("shape", [(1, 3, 5), (1, 4, 8)], ids=["scalar", "quad"])
def test_saturated_logits_stay_finite(shape):
    """One class ahead by 200, the other network votes for a trailing class: its soft-max is 0 in fp32, the term is 200."""
    nb, h, w = shape
    za = np.zeros((nb, 3, h, w), np.float32)
    zb = np.zeros((nb, 3, h, w), np.float32)
    za[:, 0] = 200.0  # A is sure of class 0 ...
    zb[:, 2] = 1.0    # ... B votes for class 2, and is itself taught class 0
    ta, tb = _planar(za).requires_grad_(True), _planar(zb).requires_grad_(True)
    out, counts, code, ga, gb = _run(ta, tb, None)
    ref = R.evaluate(za, zb)
    assert (ref["ya"] == 0).all() and (ref["yb"] == 2).all() and abs(ref["value_a"] - 200.0) < 1e-12
    assert np.array_equal(code, ref["code"]) and int(counts[2]) == 0
    _check(out, ga, gb, ref, f"saturated {shape}")
    assert abs(float(out[1]) - 200.0) <= 2e-6 * 201.0
    assert np.isfinite(ga).all() and np.isfinite(gb).all() and ga.any() and gb.any()


@pytest.mark.parametrize("shape", [(4, 37, 61), (2, 336, 544)], ids=["scalar", "quad"])
def test_empty_mask_gives_zero_not_nan(shape):
    nb, h, w = shape
    za, zb = _inputs(_case(nb, h, w, 3), "clast")
    out, counts, code, ga, gb = _run(za, zb, torch.tensor([1.0, 2.0], device=DEV))
    ya, yb, ca, cb = R.decode(code)
    assert not ca.any() and not cb.any() and int(counts[0]) == 0 and int(counts[1]) == 0
    assert np.isfinite(out).all() and out[0] == 0.0 and out[1] == 0.0 and out[2] == 0.0 and out[3] == 1.0
    assert np.isfinite(ga).all() and np.isfinite(gb).all() and not ga.any() and not gb.any()


def test_dyn_is_read_at_run_time():
    from losses.cross_pseudo import CrossPseudoSupervisionLoss
    nb, h, w, k1 = 2, 336, 544, 3
    c = _case(nb, h, w, k1)
    za, zb = _inputs(c, "clast")
    t0, t1 = R.thresholds()
    mod = CrossPseudoSupervisionLoss(k1 - 1)
    dyn = torch.tensor([1.0, t1], device=DEV)

    def step(d):
        za.grad = zb.grad = None
        loss = mod(za, zb, dyn=d)
        loss.backward()
        return (loss.item(), mod.last_value_a.item(), mod.last_value_b.item(), mod.last_confident.cpu().numpy().copy(),
                int(mod.last_agree.item()), za.grad.clone(), zb.grad.clone(), ops.CrossPseudoFn.last_code.clone())

    l1, a1, b1, n1, agree1, ga1, gb1, code1 = step(dyn)
    assert abs(l1 - (a1 + b1)) <= 2.0 ** -22 * (a1 + b1)  # weight 1
    assert agree1 == int((c["ya"] == c["yb"]).sum())
    dyn.copy_(torch.tensor([0.0, t1]))  # weight 0: the weighted value is 0, the unweighted ones keep their bits
    l0, a0, b0, n0, agree0, ga0, gb0, code0 = step(dyn)
    assert l0 == 0.0 and a0 == a1 and b0 == b1 and np.array_equal(n0, n1) and not ga0.any() and not gb0.any()
    assert torch.equal(code0, code1)
    dyn.copy_(torch.tensor([0.25, t0]))  # a later write changes the next call of the same module
    l2, a2, b2, n2, agree2, ga2, gb2, code2 = step(dyn)
    ya, yb, ca, cb = R.decode(code2.cpu().numpy())
    ref = R.evaluate(c["za"], c["zb"], t0, 0.25, ca=ca, cb=cb)
    assert n2[0] > n1[0] and n2[1] > n1[1] and tuple(int(v) for v in n2) == ref["counts"][:2] and agree2 == agree1
    assert abs(a2 - ref["value_a"]) <= 2e-6 * ref["value_mag_a"] and abs(b2 - ref["value_b"]) <= 2e-6 * ref["value_mag_b"]
    assert abs(l2 - ref["value"]) <= 0.25 * 2e-6 * (ref["value_mag_a"] + ref["value_mag_b"])
    assert (np.abs(ga2.cpu().numpy() - ref["grad_a"]) <= 2e-6 * ref["grad_mag_a"] + 1e-12).all()
    assert (np.abs(gb2.cpu().numpy() - ref["grad_b"]) <= 2e-6 * ref["grad_mag_b"] + 1e-12).all()
    # dyn=None is {1, 0} bit for bit
    none = _run(za, zb, None)
    ones = _run(za, zb, torch.tensor([1.0, 0.0], device=DEV))
    assert np.array_equal(none[0].view(np.int32), ones[0].view(np.int32)) and np.array_equal(none[1], ones[1])
    assert np.array_equal(none[2], ones[2]) and np.array_equal(none[3], ones[3]) and np.array_equal(none[4], ones[4])
    with pytest.raises(mia_hip.MiaError):
        mod(za, zb[:1])
    with pytest.raises(mia_hip.MiaError):
        mod(za, zb, dyn=torch.tensor([1.0, 0.5, 0.0], device=DEV))


@pytest.mark.parametrize("shape", [(4, 37, 61), (2, 336, 544)], ids=["scalar", "quad"])
def test_bit_identical_runs_and_batch_independence(shape):
    nb, h, w = shape
    c = _case(nb, h, w, 3)
    za, zb = _inputs(c, "mixed")
    dyn = torch.tensor([0.5, R.thresholds()[0]], device=DEV)
    a, b = _run(za, zb, dyn), _run(za, zb, dyn)
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    # the first image alone: its code is the same; its gradients are the batch's times nb (N is the only thing that changes)
    za1 = za.detach()[:1].contiguous().requires_grad_(True)
    zb1 = zb.detach()[:1].contiguous().requires_grad_(True)
    one = _run(za1, zb1, dyn)
    assert np.array_equal(one[2][0], a[2][0])
    for g1, gall in ((one[3][0], a[3][0]), (one[4][0], a[4][0])):
        assert (np.abs(g1 - nb * gall) <= 2.0 ** -22 * np.abs(g1) + 1e-30).all()  # one fp32 rounding on each side


def test_five_classes_planar_against_channels_last():
    """The instantiation <5, planar, channels-last> of the backward (tools/store_hazard_allow.json): per element against the
    restatement at full size, and bit for bit across runs."""
    nb, h, w, k1 = 2, 336, 544, 5
    c = _case(nb, h, w, k1)
    za = _planar(c["za"]).requires_grad_(True)
    zb = _clast(c["zb"]).detach().requires_grad_(True)
    dyn = torch.tensor([1.0, R.thresholds()[0]], device=DEV)
    first = _run(za, zb, dyn)
    _check_run(c, first, R.thresholds()[0], 1.0, "five classes, planar against channels-last")
    for _ in range(3):
        again = _run(za, zb, dyn)
        assert np.array_equal(again[3], first[3]) and np.array_equal(again[4], first[4]) and np.array_equal(again[2], first[2])
