"""CPU-side checks behind tests/test_gpu_step.py: the float64 restatement of the optimizer step (tests/_step_ref.py) against
torch.optim, the bounds it returns against a plain float32 evaluation (inside HALF of every bound) and against a list of subtly
wrong updates (each outside a bound at every step), the Philox restatement against Random123's known answers, the packing and
fp16-split restatements against element-by-element definitions, the host-side refusals of the C ABI, and the two host helpers of
the feed (`mia_host_narrow_labels`, `mia_host_copy`), which need no GPU at all."""
import ctypes

import numpy as np
import pytest
import torch

import _step_ref as R

BETAS, WD, MAX_NORM = (0.9, 0.999), 0.1, 10.0
KIND_IDS = ["adam", "adamw", "sgd"]


# ================================================================== optimizer restatement
@pytest.mark.parametrize("kind", KIND_IDS)
def test_restatement_matches_torch_optim(kind):
    """Three chained steps of torch.optim in float64 with clip_grad_norm_(10) (step 2 is clipped, steps 1 and 3 are not), weight
    decay 0.1, lr = 1e-2 t: p, m and v of the restatement agree to 1e-12 of their largest element."""
    rng = np.random.default_rng(3)
    n = 257
    p = rng.standard_normal(n)
    pr = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    if kind == "sgd":
        opt = torch.optim.SGD([pr], lr=1e-2, momentum=0.9, weight_decay=WD)
    else:
        opt = (torch.optim.Adam if kind == "adam" else torch.optim.AdamW)([pr], lr=1e-2, betas=BETAS, eps=1e-3, weight_decay=WD)
    m, v = np.zeros(n), np.zeros(n)
    clipped = []
    for t in (1, 2, 3):
        g = rng.standard_normal(n) * (3.0 if t == 2 else 0.1)
        pr.grad = torch.tensor(g)
        tn = float(torch.nn.utils.clip_grad_norm_([pr], MAX_NORM))
        coef = min(1.0, MAX_NORM / (tn + 1e-6))
        clipped.append(coef < 1.0)
        for gp in opt.param_groups:
            gp["lr"] = 1e-2 * t
        opt.step()
        s = dict(lr=1e-2 * t, beta1=0.9, beta2=0.999, eps=1e-3, wd=WD, bc1=1.0 - 0.9 ** t, bc2=1.0 - 0.999 ** t, cs=coef)
        r = R.step(R.KINDS[kind], p, g, m, v, s, first=(t == 1))
        st = opt.state[pr]
        want = [("p", pr.detach().numpy()), ("m", (st["momentum_buffer"] if kind == "sgd" else st["exp_avg"]).numpy())]
        if kind != "sgd":
            want.append(("v", st["exp_avg_sq"].numpy()))
        for name, w in want:
            assert np.abs(r[name] - w).max() <= 1e-12 * np.abs(w).max(), (kind, t, name)
        p, m = r["p"], r["m"]
        v = r["v"] if kind != "sgd" else v
    assert clipped == [False, True, False]


def _chain(kind, eps, n=1024, steps=3):
    """(t, p, g, m, v, scalars, reference answer) of three chained steps from optim_case: lr = 1e-2 t, wd 0.1, clip coefficient 0.37 and
    grad_scale 1/3 (so that ignoring either, or applying one twice, changes g'), state advanced with the float32 evaluation."""
    k = R.KINDS[kind]
    p, m, v, sc = R.optim_case(n, seed=11 + k)
    for t in range(1, steps + 1):
        g = R.optim_grad(sc, seed=100 * k + t)
        s = R.kernel_scalars(1e-2 * t, 0.9, 0.0 if k == R.SGD else 0.999, eps, WD, t, clip1=0.37, grad_scale=1.0 / 3.0)
        yield t, p, g, m, v, s
        p, m, v2 = R.step_f32(k, p, g, m, v, s, first=(t == 1))
        v = v if v2 is None else v2


@pytest.mark.parametrize("eps", [1e-3, 1e-8])
@pytest.mark.parametrize("kind", KIND_IDS)
def test_float32_evaluation_stays_inside_half_of_every_bound(kind, eps):
    """A plain float32 evaluation (no fused multiply-adds, textbook order) of 1024 elements over three chained steps.  The bounds
    are worst cases -- every rounding of a path at its largest and in the same direction -- so independent roundings sit well
    inside them: the largest error / bound here is 0.49 (Adam's v, whose g' enters twice with the same error), 0.46 for m, 0.38
    for p.  An evaluation outside HALF of a bound would mean a rounding that the count k next to the formula missed."""
    k = R.KINDS[kind]
    for t, p, g, m, v, s in _chain(kind, eps):
        for first in ((True, False) if k == R.SGD else (t == 1,)):
            r = R.step(k, p, g, m, v, s, first)
            got = dict(zip("pmv", R.step_f32(k, p, g, m, v, s, first)))
            for name in "pm" if k == R.SGD else "pmv":
                bound = r["bound_" + name]
                assert np.isfinite(bound).all() and (bound > 0).all()
                ratio = (np.abs(got[name].astype(np.float64) - r[name]) / bound).max()
                assert ratio <= 0.5, (kind, eps, t, first, name, ratio)
            # the bounds are about the update, not about |p|: the p bound is a small fraction of the step taken
            moved = np.abs(r["p"] - p.astype(np.float64))
            assert np.median(r["bound_p"] / moved) < 1e-3, (kind, eps, t)


@pytest.mark.parametrize("eps", [1e-3, 1e-8])
@pytest.mark.parametrize("kind", KIND_IDS)
def test_every_wrong_variant_violates_a_bound_at_every_step(kind, eps):
    k = R.KINDS[kind]
    seen = set()
    for t, p, g, m, v, s in _chain(kind, eps):
        for name, kinds, needs_first in R.VARIANTS:
            if k not in kinds:
                continue
            first = (t == 1) if needs_first is None else needs_first
            r = R.step(k, p, g, m, v, s, first)
            bad = dict(zip("pmv", R.step_f32(k, p, g, m, v, s, first, variant=name)))
            worst = max((np.abs(bad[o].astype(np.float64) - r[o]) / r["bound_" + o]).max() for o in ("pm" if k == R.SGD else "pmv"))
            assert worst > 1.0, (kind, eps, t, name, worst)
            seen.add(name)
    assert seen == {name for name, kinds, _ in R.VARIANTS if k in kinds}


def test_grad_norm_bound_counts():
    assert [R.grad_norm_blocks(n) for n in (1, 4, 1027, 4 * 256 * 1023, 4 * 256 * 1023 + 4, 3 * 2 ** 20 + 3)] == [1, 2, 2, 1024, 1024, 1024]
    assert R.grad_norm_bound(3 * 2 ** 20 + 3, 1.0) == pytest.approx(R.U * (20 / 2 + 2) + 2.0 ** -23)
    assert R.clip_coef_f32(np.float32(5.0), 10.0) == 1 and R.clip_coef_f32(np.float32(5.0), 0.0) == 1
    assert R.clip_coef_f32(np.float32(40.0), 10.0) == np.float32(10.0) / (np.float32(40.0) + np.float32(1e-6))
    assert np.isnan(R.clip_coef_f32(np.float32("nan"), 10.0))


# ================================================================== Philox
def test_philox_known_answers():
    """The three known-answer vectors of Random123's kat_vectors for philox4x32-10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(w) for w in R.philox4x32_10(ctr, key)) == want
    # vectorised over counters: the same words as one counter at a time
    q = np.array([0, 1, 2 ** 32 - 1], np.uint64)
    many = R.philox4x32_10((q, q * 0 + 7, q * 0 + 9, q * 0 + 11), (5, 6))
    for i, qi in enumerate(q):
        assert tuple(int(w[i]) for w in many) == tuple(int(w) for w in R.philox4x32_10((int(qi), 7, 9, 11), (5, 6)))


def test_dropout_restatement_values_and_frequency():
    seed, off = 2 ** 63 + 12345, 2 ** 40 + 8
    a = R.dropout_mask(40001, 0.9, seed, off)
    assert a.dtype == np.float32 and set(np.unique(a).tolist()) == {0.0, float(np.float32(1) / np.float32(0.9))}
    assert abs((a > 0).mean() - 0.9) < 0.01
    assert (R.dropout_mask(5, 1.0, seed, off) == 1.0).all()
    assert np.array_equal(R.dropout_mask(40001, 0.9, seed, off)[:4001], R.dropout_mask(4001, 0.9, seed, off))  # counter = quad index
    assert not np.array_equal(a[:4000], R.dropout_mask(4000, 0.9, seed, off + 4))
    assert not np.array_equal(a[:4000], R.dropout_mask(4000, 0.9, seed + 2 ** 32, off))  # the key's high word matters


# ================================================================== packing and splitting
def test_pack_restatement_is_the_definition():
    g = torch.Generator().manual_seed(2)
    w = torch.randn(5, 7, 3, 3, generator=g)
    for n_from_d0 in (True, False):
        nn, kk = (5, 7) if n_from_d0 else (7, 5)
        out = R.pack_weight(w, n_from_d0, 64, 16)
        assert out.shape == (9, 64, 16)
        w3 = w.reshape(5, 7, 9)
        for t in range(9):
            for n in range(64):
                for k in range(16):
                    want = 0.0 if n >= nn or k >= kk else float(w3[n, k, t] if n_from_d0 else w3[k, n, t])
                    assert float(out[t, n, k]) == want


def test_split_restatement_keeps_22_bits_and_subnormal_low_parts():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(4096).astype(np.float32)
    x[:64] *= np.float32(2.0 ** -20)
    x[100] = -0.0
    pat = R.amax_bits(x)
    e = R.split_exponent(pat)
    assert 2.0 ** 14 <= np.abs(x).max() * 2.0 ** e < 2.0 ** 15
    w = R.split_f16(x, pat)
    h = (w & np.uint32(0xFFFF)).astype(np.uint16).view(np.float16).astype(np.float64)
    l = (w >> np.uint32(16)).astype(np.uint16).view(np.float16).astype(np.float64)
    xs = x.astype(np.float64) * 2.0 ** e
    assert (np.abs(h + l - xs) <= np.maximum(np.abs(xs) * 2.0 ** -22, 2.0 ** -25)).all()
    lo = (w[:64] >> np.uint32(16)) & np.uint32(0x7FFF)
    assert ((lo > 0) & (lo < 0x0400)).any(), "no subnormal low part in the case that is meant to have them"
    assert w[100] == 0x8000
    # torch's conversions give the same words
    ts = torch.from_numpy(x) * float(2.0 ** e)
    th = ts.half()
    tl = (ts - th.float()).half()
    tw = th.view(torch.int16).numpy().view(np.uint16).astype(np.uint32) | (tl.view(torch.int16).numpy().view(np.uint16).astype(np.uint32) << 16)
    assert np.array_equal(w, tw)
    assert R.split_exponent(0) == 120 and (R.split_f16(np.zeros(8, np.float32), 0) == 0).all()


def test_colsum_addition_counts():
    assert [R.colsum_blocks(p) for p in (1, 63, 64, 65, 1000, 16384 + 37)] == [1, 1, 1, 1, 15, 256]
    assert R.colsum_k(1000, 64, False, True, 0) == 5 + 16 + 1 + 16    # per = 67 rows over 16 lanes
    assert R.colsum_k(16421, 128, True, True, 1) == 3 + 32 + 16 + 16 + 1
    assert R.colsum_k(16421, 300, False, False, 0) == 65 + 1 + 16 + 16
    assert R.colsum_k(1, 3, False, False, 0) == 1 + 85 + 1 + 16


# ================================================================== refusals of the C ABI (argument checks run before any launch)
def test_host_side_refusals():
    import mia_hip
    l = mia_hip.lib()
    P = ctypes.c_void_p
    i64, cf = ctypes.c_int64, ctypes.c_float
    ok16 = 1 << 20
    assert l.mia_grad_norm(P(ok16 + 4), i64(64), cf(10.0), cf(1.0), P(ok16), P(ok16), None) == -1
    assert b"16-byte aligned" in l.mia_last_error()
    for a, b, o in ((4, 0, 0), (0, 8, 0), (0, 0, 4)):
        assert l.mia_add(P(ok16 + a), P(ok16 + b), P(ok16 + o), mia_hip.F32, i64(16), None) == -1
        assert b"alignment" in l.mia_last_error()
    # mia_pack_weight: padding smaller than the tensor in either direction and orientation, and a dtype that is neither
    for d0, d1, npad, kpad, nd0 in ((65, 17, 64, 32, 1), (65, 17, 128, 16, 1), (65, 17, 64, 64, 0), (65, 17, 16, 128, 0)):
        assert l.mia_pack_weight(P(ok16), P(ok16), mia_hip.F32, d0, d1, 4, npad, kpad, nd0, None) == -1
        assert b"padding too small" in l.mia_last_error()
    assert l.mia_pack_weight(P(ok16), P(ok16), 2, 65, 17, 4, 128, 32, 1, None) == -1 and b"bad dtype" in l.mia_last_error()
    assert l.mia_pack_weight_batch(P(ok16), 1, 1, 17, mia_hip.F32, None) == -1  # more than 16 taps
    assert l.mia_pack_weight_batch(P(ok16), 1, 1, 9, 2, None) == -1 and b"bad dtype" in l.mia_last_error()
    assert l.mia_step_dyn_set(P(ok16 + 8), cf(1), cf(1), cf(1), 0, ctypes.c_uint64(0), ctypes.c_uint64(0), None) == -1
    assert l.mia_zero(P(ok16), i64(24), None) == -1 and l.mia_zero(P(ok16 + 4), i64(32), None) == -1
    assert l.mia_dropout_mask(P(ok16), i64(4), cf(0.0), ctypes.c_uint64(0), ctypes.c_uint64(0), None) == -1
    assert l.mia_optim_step(P(ok16), P(ok16), P(ok16), None, i64(4), mia_hip.OPT_ADAM, cf(1), cf(.9), cf(.999), cf(1e-8), cf(0), cf(1), cf(1), 1,
                            None, cf(1), None) == -1 and b"second-moment" in l.mia_last_error()


# ================================================================== host helpers of the feed
def _narrow(lab, dst, threads):
    import mia_hip
    return mia_hip.lib().mia_host_narrow_labels(ctypes.c_void_p(lab.data_ptr()), ctypes.c_void_p(dst.data_ptr()), ctypes.c_int64(lab.numel()), threads)


@pytest.mark.parametrize("n", [1, 65535, 65536, 1000003])
def test_host_narrow_labels(n):
    from training.feed import HostFeed
    g = torch.Generator().manual_seed(n)
    lab = torch.randint(0, 256, (n,), generator=g, dtype=torch.int64)
    lab[: min(n, 256)] = torch.arange(256)[: min(n, 256)]
    for threads in (1, 3, 7, 16):
        buf = torch.full((n + 32,), 0xA5, dtype=torch.uint8)
        dst = buf[16:16 + n]
        assert _narrow(lab, dst, threads) == 1 and HostFeed.labels_fit_a_byte(lab)
        assert torch.equal(dst, lab.to(torch.uint8)) and bool((buf[:16] == 0xA5).all()) and bool((buf[16 + n:] == 0xA5).all())
        per = ((n + threads - 1) // threads + 63) & ~63  # first element of the second thread's chunk
        spots = sorted({0, n - 1} | ({per - 1, per} if per < n else set()))
        for spot in spots:
            for bad in (-1, 256, 2 ** 40, -2 ** 63):
                keep = int(lab[spot])
                lab[spot] = bad
                assert _narrow(lab, dst, threads) == 0, (n, threads, spot, bad)
                if threads == 1:
                    assert not HostFeed.labels_fit_a_byte(lab)
                lab[spot] = keep
        assert _narrow(lab, dst, threads) == 1


@pytest.mark.parametrize("nbytes", [1, 2 ** 20 - 1, 2 ** 20, 5 * 2 ** 20 + 123])
def test_host_copy(nbytes):
    import mia_hip
    g = torch.Generator().manual_seed(7)
    src = torch.randint(0, 256, (nbytes,), generator=g, dtype=torch.uint8)
    for threads in (1, 3, 16):
        buf = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8)
        dst = buf[32:32 + nbytes]
        rc = mia_hip.lib().mia_host_copy(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()), ctypes.c_int64(nbytes), threads)
        assert rc == 0 and torch.equal(dst, src)
        assert bool((buf[:32] == 0x5A).all()) and bool((buf[32 + nbytes:] == 0x5A).all())
