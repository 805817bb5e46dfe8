"""csrc/dtc.hip on the GPU against the float64 restatement (tests/_dtc_ref.py): the extents of a signed distance map bit for bit, the
normalised target, and value, both terms and both gradients of the dual-task consistency loss in every layout of either tensor, on the
16-byte and the scalar path, for lb in {0, 1, B/2, B} and k in {1500, 8}; zero weights, lb = 0, saturated logits, the run-time `dyn`
buffer, determinism, batch independence, the two paths' bits, and the tensor-op form (`fused=False`).

The distance map is the device's own (`signed_distance_map`, pinned against scipy by tests/test_gpu_boundary.py); the restatement is
evaluated on it, so what is compared is the loss alone.  Bounds, with the project's constant 2e-6 (32 roundings x 2^-24,
tests/test_gpu_consistency.py, tests/test_gpu_cps.py, tests/test_gpu_bcp.py) times the magnitudes the restatement returns (its module
text lists them; everything that passes through q carries the first-order sensitivity k q (1 - q) |t| to one fp32 rounding of t):
    |L_cons - ref| <= 2e-6 * cons_mag,  |L_sdf - ref| <= 2e-6 * sdf_mag,  |L - ref| <= 2e-6 * (w0 cons_mag + w1 sdf_mag)
    |g - ref|      <= 2e-6 * (the gradient's magnitude) + 1e-12                                      per element of dz and of dr
The kernels are held to dr_mag, in which q (1 - q) and 1 - t^2 are one term each -- they form both without a subtraction.  The tensor-op
form computes `q * (1 - q)` and `1 - t * t` in fp32 as the definition writes them, so its dr is held to dr_mag_ops, where those
differences have the magnitude of their terms (q + q^2, 1 + t^2); against dr_mag it misses by three orders of magnitude wherever q is
within 1e-4 of 0 or 1, which is a property of fp32 autograd of a sigmoid, not of the definition.  Everything else is the same bound.
    |T - ref|      <= 4 * 2^-24 |T|     (fp32 tensor ops on the device's fp32 phi: 1 - phi, 1 + m_in and the quotient, three roundings)
The kernels evaluate soft-max, tanh and sigmoid in double from the fp32 logits, add per thread, per wave and per block in double and
round a block's sum once to a (hi, lo) float pair; a gradient is one fp32 rounding of a double expression of coefficients rounded once
to fp32.
Measured on an MI355X over every case below: the error of L, L_cons and L_sdf is at most 0.0079 of its bound, the gradient error at
most 0.070; for the tensor-op form (`fused=False`, fp32 torch ops) 0.0059 and 0.20 against dr_mag_ops, and 1.7e3 against dr_mag
((4, 37, 61), k1 = 3: the figure that made dr_mag_ops necessary; the kernels were never near either)."""
import functools
import itertools

import numpy as np
import pytest
import torch

import _dtc_ref as R
import mia_hip
from mia_hip import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LAYOUTS = ["planar", "clast", "slice", "offset"]
W0, W1 = 0.7, 0.3
W0F, W1F = float(np.float32(W0)), float(np.float32(W1))  # what the device reads
CROSS = (4, 37, 61)   # odd: a tail after full quads, the lb boundary inside a block's range; the full layout cross product runs here
BIG = (2, 336, 544)   # 16-byte units, several blocks per image
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) and isinstance(v[0], int) else ("+".join(v) if isinstance(v, tuple) else str(v))


# ---------------------------------------------------------------- inputs and references, computed once and never modified
@functools.lru_cache(maxsize=None)
def _inputs(shape, k1, kind="normal"):
    nb, h, w = shape
    z, r = (R.saturated_case if kind == "saturated" else R.make_case)(nb, k1, h, w)
    z.setflags(write=False)
    r.setflags(write=False)
    return z, r


@functools.lru_cache(maxsize=None)
def _phi(shape, k1):
    """(labels on the device, the device's phi [nb, C, H, W], phi as float64 numpy)."""
    from losses.boundary_loss import signed_distance_map
    nb, h, w = shape
    labels = torch.tensor(R.make_labels(nb, k1, h, w)).to(DEV)
    phi = signed_distance_map(labels, k1 - 1)
    host = phi.cpu().numpy().astype(np.float64)
    host.setflags(write=False)
    return labels, phi, host


@functools.lru_cache(maxsize=8)
def _ref(shape, k1, lb, k, kind="normal", w0=W0F, w1=W1F):
    z, r = _inputs(shape, k1, kind)
    return R.evaluate(z, r, _phi(shape, k1)[2][:lb], lb, k, w0, w1)


def _planar(a):
    return torch.tensor(a).to(DEV)


def _clast(a, lead=0):
    """The head's layout: memory [B][H][W][K] viewed as [B, K, H, W]; with `lead`, a batch slice of a larger tensor."""
    t = torch.tensor(a).to(DEV).permute(0, 2, 3, 1)
    big = torch.full((lead + t.shape[0],) + tuple(t.shape[1:]), 7.0, device=DEV)
    big[lead:] = t
    return big.permute(0, 3, 1, 2)[lead:]


def _offset(a):
    """Planar at a 4-byte offset from a 16-byte boundary: never the 16-byte path."""
    flat = torch.empty(a.size + 1, device=DEV, dtype=torch.float32)[1:]
    flat.copy_(torch.tensor(a).reshape(-1))
    return flat.view(a.shape)


def _logits(a, layout):
    t = {"planar": _planar, "clast": _clast, "slice": lambda x: _clast(x, 2), "offset": _offset}[layout](np.ascontiguousarray(a))
    return t.detach().requires_grad_(True)


def _dyn(w0=W0, w1=W1):
    return torch.tensor([w0, w1], device=DEV, dtype=torch.float32)


def _run(z, r, phi, lb, dyn, k=1500.0, fused=True):
    """(out [3] = L, L_cons, L_sdf; dz; dr) as numpy from one forward + backward of the module."""
    from losses.dual_task import DualTaskConsistencyLoss
    mod = DualTaskConsistencyLoss(z.shape[1] - 1, k, fused=fused)
    z.grad = r.grad = None
    loss = mod(z, r, None, lb, dyn=dyn, phi=None if lb == 0 else phi[:lb])
    loss.backward()
    out = torch.stack([loss.detach(), mod.last_consistency, mod.last_sdf])
    return out.cpu().numpy().astype(np.float64), z.grad.cpu().numpy().astype(np.float64), r.grad.cpu().numpy().astype(np.float64)


RATIOS = {"value": 0.0, "grad": 0.0}       # the largest error / bound ratios of the kernels so far in this session
RATIOS_SOFT = {"value": 0.0, "grad": 0.0}  # and of the tensor-op form


def _check(res, ref, what, RATIOS=RATIOS, ops_form=False):
    out, dz, dr = res
    assert np.isfinite(out).all() and np.isfinite(dz).all() and np.isfinite(dr).all(), what
    ratios = []
    for name, got, want, mag in (("L", out[0], ref["value"], ref["value_mag"]), ("cons", out[1], ref["cons"], ref["cons_mag"]),
                                 ("sdf", out[2], ref["sdf"], ref["sdf_mag"])):
        err, bound = abs(float(got) - want), 2e-6 * mag
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        ratios.append(f"{name} {ratio:.3f}")
        RATIOS["value"] = max(RATIOS["value"], ratio)
        assert err <= bound, (what, name, float(got), want, err, bound)
    for name, g in (("dz", dz), ("dr", dr)):
        bound = 2e-6 * ref["dr_mag_ops" if ops_form and name == "dr" else name + "_mag"] + 1e-12
        ratio = float((np.abs(g - ref[name]) / bound).max())
        ratios.append(f"{name} {ratio:.3f}")
        RATIOS["grad"] = max(RATIOS["grad"], ratio)
        assert ratio <= 1.0, (what, name, ratio)
    print(f"{what}: err/bound  {'  '.join(ratios)}   largest so far {RATIOS}")


def _case(shape, k1, lz, lr, lb, k, kind="normal", fused=True, RATIOS=RATIOS):
    z, r = _inputs(shape, k1, kind)
    res = _run(_logits(z, lz), _logits(r, lr), _phi(shape, k1)[1], lb, _dyn(), k, fused)
    _check(res, _ref(shape, k1, lb, k, kind), f"{shape} k1={k1} z {lz} r {lr} lb={lb} k={k} {kind} fused={fused}", RATIOS, not fused)
    return res


# ---------------------------------------------------------------- extents and target
@pytest.mark.parametrize("shape,k1", list(itertools.product(R.SHAPES, R.K1S)), ids=_ids)
def test_extents_bit_for_bit_and_target_to_fp32_rounding(shape, k1):
    from losses.dual_task import normalized_distance_map
    labels, phi, host = _phi(shape, k1)
    want = torch.stack([phi.amax((2, 3)), (-phi).amax((2, 3))], -1) + 0.0  # + 0.0: -0.0 (a class with phi = 0) becomes +0.0
    for name, p in (("aligned", phi), ("offset", _offset(phi.cpu().numpy()))):  # the 16-byte and the one-element loads
        ext = ops.sdm_extent(p)
        assert ext.shape == (shape[0], k1 - 1, 2) and torch.equal(ext.view(torch.int32), want.view(torch.int32)), name
    assert (ext >= 0).all()
    T = normalized_distance_map(labels, k1 - 1).cpu().numpy().astype(np.float64)
    ref = R.target(host)
    assert (np.abs(T - ref) <= 4 * 2.0 ** -24 * np.abs(ref)).all()
    assert (T[host == 0] == 0).all() and np.abs(T).max() <= 1.0 + 1e-6


# ---------------------------------------------------------------- value and gradients against the restatement
@pytest.mark.parametrize("k1,lz,lr", list(itertools.product(R.K1S, LAYOUTS, LAYOUTS)), ids=_ids)
def test_every_layout_pair_against_restatement(k1, lz, lr):
    _case(CROSS, k1, lz, lr, CROSS[0] // 2, 1500.0)


@pytest.mark.parametrize("k1,lb,k,layouts", list(itertools.product(R.K1S, [0, 1, 2, 4], [1500.0, 8.0], [("clast", "clast"), ("planar", "offset")])),
                         ids=_ids)
def test_every_labelled_count_and_both_slopes(k1, lb, k, layouts):
    res = _case(CROSS, k1, layouts[0], layouts[1], lb, k)
    if lb == 0:
        assert res[0][2] == 0.0  # L_sdf exactly 0, not 0 / 0


@pytest.mark.parametrize("shape,k1,layouts", list(itertools.product(R.SHAPES[:2], R.K1S, [("planar", "planar"), ("clast", "clast"),
                                                                                          ("slice", "slice"), ("offset", "planar")])),
                         ids=_ids)
def test_tiny_shapes(shape, k1, layouts):
    for lb in sorted({0, 1, shape[0] // 2, shape[0]}):
        _case(shape, k1, layouts[0], layouts[1], lb, 1500.0)


@pytest.mark.parametrize("k1,layouts", [(2, ("clast", "clast")), (3, ("clast", "clast")), (8, ("clast", "clast")), (3, ("planar", "slice")),
                                        (8, ("slice", "planar")), (2, ("planar", "planar")), (3, ("offset", "clast"))], ids=_ids)
def test_several_blocks_per_image(k1, layouts):
    _case(BIG, k1, layouts[0], layouts[1], 1, 1500.0)  # one reference per class count: the other lb and k run on the odd shape


@pytest.mark.parametrize("shape,k1,lb", [(CROSS, 3, 2), (BIG, 2, 1)], ids=_ids)
def test_tensor_op_form_within_the_same_bounds(shape, k1, lb):
    _case(shape, k1, "clast", "clast", lb, 1500.0, fused=False, RATIOS=RATIOS_SOFT)


@pytest.mark.parametrize("shape,k1,layouts", [(CROSS, 3, ("clast", "planar")), (BIG, 3, ("clast", "clast")), ((1, 1, 1), 2, ("planar", "planar"))], ids=_ids)
def test_saturated_logits_give_finite_values_and_gradients(shape, k1, layouts):
    _case(shape, k1, layouts[0], layouts[1], max(shape[0] // 2, 1), 1500.0, kind="saturated")


# ---------------------------------------------------------------- exact properties
def _raw(shape, k1, lz, lr, lb, dyn, k=1500.0, rows=slice(None)):
    """(out, dz, dr) as device-side bits (torch tensors on the host) for the images `rows` of the case."""
    z, r = _inputs(shape, k1)
    zt, rt = _logits(z[rows], lz), _logits(r[rows], lr)
    from losses.dual_task import DualTaskConsistencyLoss
    mod = DualTaskConsistencyLoss(k1 - 1, k)
    phi = _phi(shape, k1)[1][rows]
    loss = mod(zt, rt, None, lb, dyn=dyn, phi=None if lb == 0 else phi[:lb])
    loss.backward()
    return torch.stack([loss.detach(), mod.last_consistency, mod.last_sdf]).cpu(), zt.grad.cpu(), rt.grad.cpu()


@pytest.mark.parametrize("shape,layouts", [(CROSS, ("clast", "planar")), (BIG, ("clast", "clast"))], ids=_ids)
def test_zero_weights_are_exact(shape, layouts):
    k1, lb = 3, shape[0] // 2
    out, dz, dr = _raw(shape, k1, *layouts, lb, _dyn(0.0, W1))
    assert not dz.any() and not dr[lb:].any() and dr[:lb].any()  # no consistency: dz == 0 everywhere, dr == 0 on unlabelled images
    assert abs(float(out[0]) - W1F * float(out[2])) <= 3e-7 * float(out[0])  # L = beta L_sdf, each rounded once to fp32
    base = _raw(shape, k1, *layouts, 0, _dyn(W0, W1))            # no labelled image: no L_sdf part anywhere
    out, dz, dr = _raw(shape, k1, *layouts, lb, _dyn(W0, 0.0))   # beta = 0 removes it exactly
    assert torch.equal(dz, base[1]) and torch.equal(dr, base[2])
    assert out[1] == base[0][1] and out[2] > 0 and base[0][2] == 0 and not torch.isnan(base[0]).any()


def test_a_later_write_to_dyn_changes_the_next_call():
    shape, k1, lb = CROSS, 3, 2
    dyn = _dyn(W0, W1)
    first = _raw(shape, k1, "clast", "clast", lb, dyn)
    dyn.copy_(torch.tensor([0.25, 1.5]))
    second = _raw(shape, k1, "clast", "clast", lb, dyn)
    assert not torch.equal(first[0], second[0])
    ref = _ref(shape, k1, lb, 1500.0, "normal", 0.25, 1.5)
    _check(tuple(t.numpy().astype(np.float64) for t in second), ref, "dyn rewritten")
    assert torch.equal(first[0][1:], second[0][1:])  # the unweighted terms do not move


@pytest.mark.parametrize("shape,k1,layouts", [(CROSS, 8, ("slice", "planar")), (BIG, 3, ("clast", "clast"))], ids=_ids)
def test_two_runs_give_identical_bits(shape, k1, layouts):
    a = _raw(shape, k1, *layouts, shape[0] // 2, _dyn())
    b = _raw(shape, k1, *layouts, shape[0] // 2, _dyn())
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("layouts", [("clast", "clast"), ("planar", "offset")], ids=_ids)
def test_an_image_gradient_depends_on_the_batch_through_the_denominator_alone(layouts):
    """A batch of 4 with 2 labelled against its two halves with the consistency weight halved: 2 w0 / N is the same number, and so is
    2 w1 / Ns of the labelled half."""
    shape, k1 = CROSS, 3
    full = _raw(shape, k1, *layouts, 2, _dyn(W0, W1))
    lo = _raw(shape, k1, *layouts, 2, _dyn(W0 / 2, W1), rows=slice(0, 2))
    hi = _raw(shape, k1, *layouts, 0, _dyn(W0 / 2, W1), rows=slice(2, 4))
    assert torch.equal(full[1], torch.cat([lo[1], hi[1]])) and torch.equal(full[2], torch.cat([lo[2], hi[2]]))


@pytest.mark.parametrize("k1", R.K1S)
def test_the_16_byte_and_the_scalar_path_give_identical_bits(k1):
    wide = _raw(BIG, k1, "planar", "clast", 1, _dyn())
    scalar = _raw(BIG, k1, "offset", "clast", 1, _dyn())   # one misaligned tensor sends both to the scalar path
    assert all(torch.equal(x, y) for x, y in zip(wide, scalar))
    scalar = _raw(BIG, k1, "planar", "offset", 1, _dyn())
    assert all(torch.equal(x, y) for x, y in zip(wide[:2], scalar[:2])) and torch.equal(wide[2], scalar[2])


def test_argument_errors():
    z = torch.zeros(2, 9, 4, 4, device=DEV)
    r = torch.zeros(2, 8, 4, 4, device=DEV)
    with pytest.raises(mia_hip.MiaError, match="classes"):
        ops.DTCLossFn.apply(z, r, None, None, 0, 1500.0, None)
    with pytest.raises(mia_hip.MiaError, match="labeled_bs"):
        ops.DTCLossFn.apply(z[:, :3], r[:, :2], None, None, 3, 1500.0, None)
    with pytest.raises(mia_hip.MiaError, match="distance map"):
        ops.DTCLossFn.apply(z[:, :3], r[:, :2], None, None, 1, 1500.0, None)
    with pytest.raises(mia_hip.MiaError, match="level-set"):
        ops.DTCLossFn.apply(z[:, :3], r[:, :3], None, None, 0, 1500.0, None)
