"""csrc/consistency.hip on the GPU against the float64 restatement (tests/_consistency_ref.py): the keep map, n_keep, value and
gradient of the softmax-MSE consistency loss in every layout and on both the four-pixel and the one-pixel path, the run-time `dyn`
buffer, determinism, and the exponential moving average.

Bounds (32 roundings x 2^-24 ~ 2e-6 of the magnitudes being rounded; the cancellation in ps - pt is allowed for):
    |L - ref| <= 2e-6 * coef * sum keep * sum_k |e_k| (ps_k + pt_k)
    |g - ref| <= 2e-6 * 2 * coef * keep * ps_j * ((ps_j + pt_j) + sum_k ps_k (ps_k + pt_k)) + 1e-12        per element
The device's keep map may differ from the float64 mask only at ambiguous pixels, |u - threshold| < 1e-5 in float64, which are at most
5e-4 of any case (the float64 reference alone gives at most 1.2e-4 with this generator and these seeds); value and gradient are
checked against the restatement evaluated with the device's own map."""
import functools

import numpy as np
import pytest
import torch

import _consistency_ref as R
import mia_hip
from mia_hip import ops

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 1, 7), (4, 37, 61), (2, 336, 544)]  # hw odd: one pixel per thread; the last: four per thread, several slabs
K1S = [2, 3, 8]
LAYOUTS = ["planar", "clast", "mixed", "slice", "offset"]
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _case(nb, h, w, k1):
    """Inputs and every float64 reference of one case, computed once and never modified."""
    zs, zt, pbar = R.make_case(nb, k1, h, w)
    for a in (zs, zt, pbar):
        a.setflags(write=False)
    return dict(zs=zs, zt=zt, pbar=pbar, u=R.entropy(pbar), plain=R.evaluate(zs, zt))


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
    zs = {"planar": _planar, "clast": _clast, "mixed": _clast, "slice": lambda a: _clast(a, 2), "offset": _offset}[layout](c["zs"])
    zt = {"planar": _planar, "clast": _clast, "mixed": _planar, "slice": _clast, "offset": _planar}[layout](c["zt"])
    return zs.detach().requires_grad_(True), zt, _planar(c["pbar"])


def _run(zs, zt, pbar, dyn, den_scale=2.0):
    """(out [3], n_keep, keep map or None, gradient) as numpy, from one forward + backward."""
    zs.grad = None
    loss = ops.ConsistencyFn.apply(zs, zt, pbar, dyn, den_scale)
    out, kept, keep = ops.ConsistencyFn.last_out, ops.ConsistencyFn.last_kept, ops.ConsistencyFn.last_keep
    loss.backward()
    return (out.cpu().numpy(), int(kept.item()), None if keep is None else keep.cpu().numpy().astype(bool),
            zs.grad.cpu().numpy().astype(np.float64))


def _check(out, grad, ref, what):
    vb = 2e-6 * ref["value_mag"]
    gb = 2e-6 * ref["grad_mag"] + 1e-12
    verr, gerr = abs(float(out[1]) - ref["value"]), np.abs(grad - ref["grad"])
    print(f"{what}: L={out[1]:.9g} ref={ref['value']:.9g}  value err/bound={verr / max(vb, 1e-300):.3f}  "
          f"gradient max err/bound={(gerr / gb).max():.3f}")
    assert np.isfinite(out).all() and np.isfinite(grad).all()
    assert verr <= vb, (what, verr, vb)
    assert (gerr <= gb).all(), (what, (gerr / gb).max())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k1", K1S)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_value_gradient_and_mask_against_restatement(shape, k1, layout):
    nb, h, w = shape
    c = _case(nb, h, w, k1)
    zs, zt, pbar = _inputs(c, layout)
    out, n_keep, keep, grad = _run(zs, zt, None, None)  # the plain form
    assert keep is None and n_keep == nb * h * w and out[2] == 1.0 and out[0] == out[1]
    _check(out, grad, c["plain"], f"plain {shape} k1={k1} {layout}")
    for thr in R.thresholds(k1):
        dyn = torch.tensor([1.0, thr], device=DEV)
        out, n_keep, keep, grad = _run(zs, zt, pbar, dyn)
        want = c["u"] < thr
        ambiguous = np.abs(c["u"] - thr) < 1e-5
        assert ambiguous.mean() <= 5e-4, "the inputs put too many pixels on the threshold"
        assert np.array_equal(keep[~ambiguous], want[~ambiguous])
        assert n_keep == int(keep.sum())  # exactly the device map's own count
        assert out[2] == 1.0 and out[0] == out[1]
        _check(out, grad, R.evaluate(c["zs"], c["zt"], keep), f"masked {shape} k1={k1} {layout} thr={thr:.4f} kept={keep.mean():.3f}")
        assert not grad[np.broadcast_to(~keep[:, None], grad.shape)].any()  # a dropped pixel: exactly zero


def test_both_branches_of_the_mask_run():
    shares = []
    for k1 in K1S:
        c = _case(2, 336, 544, k1)
        shares += [float((c["u"] < thr).mean()) for thr in R.thresholds(k1)]
    assert 0.5 < min(shares) and max(shares) < 0.995, shares


@pytest.mark.parametrize("shape", [(4, 37, 61), (2, 336, 544)], ids=["scalar", "quad"])
def test_all_dropped_mask_gives_zero_not_nan(shape):
    nb, h, w = shape
    zs, zt, pbar = _inputs(_case(nb, h, w, 3), "clast")
    out, n_keep, keep, grad = _run(zs, zt, pbar, torch.tensor([1.0, 0.0], device=DEV))
    assert n_keep == 0 and not keep.any()
    assert out[0] == 0.0 and out[1] == 0.0 and np.isfinite(out).all()
    assert np.isfinite(grad).all() and not grad.any()


def test_dyn_is_read_at_run_time():
    from losses.consistency_loss import SoftmaxMSEConsistency
    nb, h, w, k1 = 2, 336, 544, 3
    c = _case(nb, h, w, k1)
    zs, zt, pbar = _inputs(c, "clast")
    t0, t1 = R.thresholds(k1)
    mod = SoftmaxMSEConsistency(k1 - 1)
    dyn = torch.tensor([1.0, t0], device=DEV)

    def step():
        zs.grad = None
        loss = mod(zs, zt, pbar, dyn=dyn)
        loss.backward()
        return loss.item(), mod.last_value.item(), int(mod.last_kept.item()), zs.grad.clone()

    l1, v1, n1, g1 = step()
    assert l1 == v1
    dyn.copy_(torch.tensor([0.0, t0]))  # weight 0: the weighted value is 0, the unweighted one keeps its bits
    l0, v0, n0, g0 = step()
    assert l0 == 0.0 and v0 == v1 and n0 == n1 and not g0.any()
    dyn.copy_(torch.tensor([0.25, t1]))  # a later write changes the next call of the same module
    l2, v2, n2, g2 = step()
    ref = R.evaluate(c["zs"], c["zt"], ops.ConsistencyFn.last_keep.cpu().numpy().astype(bool))
    assert n2 > n1 and n2 == ref["n_keep"]
    assert abs(v2 - ref["value"]) <= 2e-6 * ref["value_mag"]
    assert abs(l2 - 0.25 * ref["value"]) <= 0.25 * 2e-6 * ref["value_mag"]
    assert (np.abs(g2.cpu().numpy() - 0.25 * ref["grad"]) <= 0.25 * 2e-6 * ref["grad_mag"] + 1e-12).all()
    with pytest.raises(mia_hip.MiaError):  # prob_mean without dyn
        mod(zs, zt, pbar)
    with pytest.raises(mia_hip.MiaError):
        mod(zs, zt[:1])


@pytest.mark.parametrize("shape", [(4, 37, 61), (2, 336, 544)], ids=["scalar", "quad"])
def test_bit_identical_runs_and_batch_independence(shape):
    nb, h, w = shape
    k1 = 3
    c = _case(nb, h, w, k1)
    zs, zt, pbar = _inputs(c, "clast")
    dyn = torch.tensor([1.0, R.thresholds(k1)[1]], device=DEV)
    a = _run(zs, zt, pbar, dyn)
    b = _run(zs, zt, pbar, dyn)
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and a[1] == b[1]
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    p1, p2 = _run(zs, zt, None, None), _run(zs, zt, None, None)
    assert np.array_equal(p1[0].view(np.int32), p2[0].view(np.int32)) and np.array_equal(p1[3], p2[3])
    # the first image alone: its keep map is the same; its gradient is the same up to the denominators (coef is one fp32 value)
    zs1 = zs.detach()[:1].contiguous().requires_grad_(True)
    one = _run(zs1, zt[:1].contiguous(), pbar[:1].contiguous(), dyn)
    assert np.array_equal(one[2][0], a[2][0])
    den_all, den_one = 2.0 * a[1] + 1e-16, 2.0 * one[1] + 1e-16
    ga, g1 = a[3][0] * den_all, one[3][0] * den_one
    assert (np.abs(ga - g1) <= 2.0 ** -21 * np.abs(ga) + 1e-30).all()  # two fp32 roundings each: coef and the gradient itself
    po = _run(zs1, zt[:1].contiguous(), None, None)
    assert (np.abs(po[3][0] - nb * p1[3][0]) <= 2.0 ** -21 * np.abs(po[3][0]) + 1e-30).all()


# ---------------------------------------------------------------- exponential moving average
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, 2 ** 20 + 3])
def test_ema_update(n):
    rng = np.random.default_rng(n)
    t0 = rng.standard_normal(n + 8).astype(np.float32)
    s0 = rng.standard_normal(n + 8).astype(np.float32)
    s0[:: 7] = -0.0  # alpha == 0 must copy the sign of a zero too
    sbuf = torch.from_numpy(s0).to(DEV)
    for toff, soff in ((0, 0), (1, 1), (4, 0), (0, 1), (3, 2)):  # aligned, co-aligned at a 4-byte offset, differently aligned
        for alpha in (0.99, 0.5, 0.0):
            a32 = float(np.float32(alpha))
            tbuf = torch.from_numpy(t0).to(DEV)
            ops.ema_update(tbuf[toff:toff + n], sbuf[soff:soff + n], alpha)
            got = tbuf.cpu().numpy()
            assert np.array_equal(got[:toff].view(np.int32), t0[:toff].view(np.int32))  # nothing outside the slice is touched
            assert np.array_equal(got[toff + n:].view(np.int32), t0[toff + n:].view(np.int32))
            t, s = t0[toff:toff + n], s0[soff:soff + n]
            if alpha == 0.0:
                assert np.array_equal(got[toff:toff + n].view(np.int32), s.view(np.int32))
            else:
                err = np.abs(got[toff:toff + n].astype(np.float64) - R.ema(t, s, a32))
                assert (err <= R.ema_bound(t, s, a32)).all(), (toff, soff, alpha, (err / R.ema_bound(t, s, a32)).max())
            tdev = torch.from_numpy(t0).to(DEV)
            ops.ema_update(tdev[toff:toff + n], sbuf[soff:soff + n], torch.tensor([alpha], device=DEV))  # alpha from the device
            assert torch.equal(tdev.view(torch.int32), tbuf.view(torch.int32))
    assert torch.equal(sbuf.cpu().view(torch.int32), torch.from_numpy(s0).view(torch.int32))  # the student is only read
