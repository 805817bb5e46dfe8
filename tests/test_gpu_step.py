"""GPU checks of what every training step runs besides the convs, norms and losses: csrc/optim.hip (clip-by-global-norm, Adam / AdamW /
SGD over the flat buffers) and csrc/pack.hip (weight packing, the batched re-pack, fp16 splitting, maxima, relayout, column sums,
residual add, Dropout2d masks, zero / gather, label widening) against the restatements in tests/_step_ref.py, called through the C
ABI (mia_hip.call / ops).  Every output lives inside a buffer filled with NaN (or a sentinel bit pattern) with guard elements in
front of and behind it: the guards must be bit-identical afterwards and every element a kernel owns must have been written.  The
host-side refusals and the two host helpers (mia_host_narrow_labels, mia_host_copy) are in tests/test_step_host.py.

Launch -> kernel / branch -> case (test[parameters]):
  mia_grad_norm
    sumsq_partial_kernel
      tail loop only (n < 4) ....................... test_grad_norm[1 | 2 | 3]
      quad loop, with and without tail ............. test_grad_norm[4 | 5 | 1027]
      blocks = quads / 256 + 1 = 1024, and the cap . test_grad_norm[1047552 | 1047556]
      quad loop wraps the 1024-block grid (3 trips)  test_grad_norm[3145731]
    norm_final_kernel
      coefficient < 1, >= 1 (exactly 1.0f) ......... test_grad_norm[*] (scales 1 and 1e-3), max_norm <= 0: [*] (max_norm 0 and -1)
      norm 0, NaN .................................. test_grad_norm_zero_and_nan
  mia_optim_step: optim_step_kernel, dyn = NULL
    kind Adam / AdamW / SGD, first step and later .. test_optim_step[*] (steps 1 .. 3 chained)
    clip NULL / coefficient < 1 / = 1 / max_norm 0 . test_optim_step[*-none | *-clip | *-zero]; grad_scale 1 and 1/3: [*-1 | *-3]
    wd != 0 (coupled and decoupled) ................ every case; wd = 0: test_optim_step_dyn_is_bit_identical (kernel against kernel)
    one block .. 40 blocks ......................... test_optim_step sizes 1, 3, 4, 5, 1027, 10007
    grid-stride loop wraps 8192 x 256, ragged tail . test_optim_step_wraps_the_grid[*] (3 * 2^20 + 3)
    slice 4 elements into a larger buffer .......... test_optim_step_on_a_slice
    through FlatOptimizer.step, two live runs ...... test_flat_optimizer_skips_a_parameter_without_gradient[*]
  mia_step_dyn_set: step_dyn_set_kernel ............ test_step_dyn_set_bytes
  mia_optim_step_dyn: optim_step_kernel, dyn != NULL test_optim_step_dyn_is_bit_identical[3 kinds x first 0 / 1]
  mia_scale_by_clip: scale_by_dev_kernel
    c != 1, loop wraps 8192 x 256 .................. test_scale_by_clip[1 | 1027 | 3145731]
    c == 1 (early return) .......................... test_scale_by_clip[*] second half
  mia_pack_weight
    pack_weight_kernel<float / bf16_t> (naive) ..... test_pack_weight[(1,1,1,1) | (3,16,1,1) | (5,7,3,3) | (16,130,5,5: 25 taps)] x orientation
    pack_weight_tiled_kernel<T, 16, 64> / <T, 64, 16> test_pack_weight[(64,64,3,3) | (96,40,3,3) | (65,17,2,2) | (130,96,3,3)], n_from_d0 1 / 0
    padding one brick larger than the minimum ...... test_pack_weight_extra_padding (tiled and naive)
  mia_pack_weight_batch: pack_weight_batch_kernel<float / bf16_t>
    pack_brick<T, 9 | 4 | 1 | 0> ................... test_pack_weight_batch[*]: 3x3, 2x2, 1x1 and 1x3 tensors, both orientations
    ballot loop 2 and 3 iterations ................. test_pack_weight_batch[bf16-38 | f32-38] (76 descriptors), [f32-68] (136)
  mia_split_f16_batch: split_f16_batch_kernel
    count 1; count 5 ............................... test_split_f16_batch
    n / 4 < 256 (blocks 1 .. 63 return) ............ tensors of 64 and 1024 words
    stride wraps 64 x 256 quads .................... tensor of 200704 words
    amax 0 (e = 120), subnormal low parts .......... the all-zero tensor, the tensor with elements at 2^-20 of its maximum
    through ops.PackPlan ........................... test_pack_weight_batch[f32-*]
  mia_amax_batch: amax_slots_zero_kernel + amax_batch_kernel (amax_span head / body / tail, amax_block)
    sizes 1, 3, 1023, 70001 (> 64 blocks x 1024) ... test_amax_batch
    NaN stays visible; start not 16-byte aligned ... test_amax_batch (tensors 4 and 5)
    (mia_amax, the one-tensor form, shares amax_span / amax_block: tests/test_gpu_ops.py and PackCache.get in test_pack_weight_batch)
  mia_relayout: relayout_kernel<TS, TD>, 4 dtype pairs
    dst_c_fast = 1 (NCHW -> NHWC, cast_nhwc) ....... test_relayout[*-to_nhwc], test_relayout_through_ops
    dst_c_fast = 0 (NHWC -> NCHW) .................. test_relayout[*-to_nchw], test_to_nhwc_gradient[contiguous]
    channel slice as source ........................ test_relayout_through_ops
    loop wraps 16384 x 256 ......................... test_relayout_wraps_the_grid
  mia_colsum
    colsum_vec_kernel<float / bf16_t> .............. test_colsum[*] c = 64, 128, 320
    colsum_partial_kernel<float / bf16_t> .......... test_colsum[*] c = 1, 3, 96, 300 (two channel blocks); x 4 bytes off: test_colsum_misaligned
    colsum_final_kernel, accumulate 0 / 1 .......... every case
  mia_add: add_kernel<float / bf16_t>
    tail only, units + tail, wrap of 8192 x 256 .... test_add[*]
  mia_dropout_mask / mia_dropout_mask_dyn: dropout_mask_kernel, dyn NULL / non-NULL
    ragged last quad, wrap of 1024 x 256 quads ..... test_dropout_mask[*]
    carry of base + rel_offset across 2^32 ......... test_dropout_mask_dyn
  mia_zero: zero_kernel, 1 unit and past 2048 blocks test_zero
  mia_gather_f32: gather_f32_kernel ................ test_gather
  mia_widen_u8_i64: widen_u8_i64_kernel, odd tail .. test_widen_u8_i64
Not mapped: mia_version / mia_last_error / the *_desc_bytes and *_workspace getters (no kernel; asserted where used).

Bounds: tests/_step_ref.py states each one as (roundings on the path) * 2^-24 * magnitude + 1 ulp; everything else is bit-exact.  Every
bounded test prints its error / bound ratios (pytest -s) and asserts only that they are below 1.  Largest seen on an MI355X:
optimizer p 0.40, m 0.50, v 0.52; through FlatOptimizer 0.32; mia_grad_norm 0.10; mia_colsum 0.05 (the docstrings of test_optim_step,
test_flat_optimizer_skips_a_parameter_without_gradient, test_grad_norm and test_colsum repeat them).  Finding recorded here:
mia_split_f16_batch keeps subnormal low parts on the device, as csrc/common.h says (test_split_f16_batch compares them bit for bit)."""
import ctypes

import numpy as np
import pytest
import torch

import _step_ref as R
import test_gpu_norm as G

pytestmark = pytest.mark.gpu

_dev, _abi = G._dev, G._abi
NAN = float("nan")
GUARD = 16
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
WD = 0.1


def raw(t):
    return t if not t.dtype.is_floating_point else t.view(_INT[t.element_size()])


class Guarded:
    """`n` elements of `dtype` inside a buffer filled with `fill`, GUARD elements in front (plus `offset`) and GUARD behind."""

    def __init__(self, n, dtype, dev, fill=NAN, offset=0):
        self.lo, self.n = GUARD + offset, n
        self.base = torch.full((self.lo + n + GUARD,), fill, dtype=dtype, device=dev)
        self.view = self.base[self.lo:self.lo + n]
        self.before = raw(self.base).clone()

    def set(self, values):
        self.view.copy_(torch.as_tensor(values).to(self.view.dtype))
        self.before = raw(self.base).clone()
        return self

    def guards_ok(self):
        now = raw(self.base)
        return torch.equal(now[:self.lo], self.before[:self.lo]) and torch.equal(now[self.lo + self.n:], self.before[self.lo + self.n:])

    def untouched(self):
        return torch.equal(raw(self.base), self.before)

    def np(self):
        return self.view.detach().cpu().numpy()


def bits1(x):
    return int(R.bits32(x).reshape(-1)[0])


def note(tag, ratio):
    print(f"RATIO {tag} {ratio:.4f}")


def same_bits(got, ref):
    """Bit-identical, where a NaN may be any NaN."""
    got, ref = got.detach().cpu().contiguous(), ref.detach().cpu().contiguous()
    assert got.shape == ref.shape and got.dtype == ref.dtype
    if got.dtype.is_floating_point:
        gn, rn = torch.isnan(got), torch.isnan(ref)
        return torch.equal(gn, rn) and torch.equal(raw(got)[~gn], raw(ref)[~rn])
    return torch.equal(got, ref)


# ================================================================== mia_grad_norm
def run_grad_norm(g, max_norm, grad_scale, dev):
    mia_hip, ops = _abi()
    gd = Guarded(g.size, torch.float32, dev).set(g)
    ws = Guarded(mia_hip.lib().mia_grad_norm_workspace(), torch.float32, dev)
    out = Guarded(2, torch.float32, dev)
    mia_hip.call("mia_grad_norm", ops._p(gd.view), ops._c_i64(g.size), ops._c_float(max_norm), ops._c_float(grad_scale), ops._p(ws.view),
                 ops._p(out.view), ops._stream())
    torch.cuda.synchronize()
    assert gd.untouched() and ws.guards_ok() and out.guards_ok()
    if np.isfinite(g).all():
        assert int(torch.isnan(ws.view).sum()) == ws.n - R.grad_norm_blocks(g.size), "one partial sum per block, the rest untouched"
    return out.np().copy()


def mixed_grad(n, seed):
    rng = np.random.default_rng(seed)
    return (np.where(rng.random(n) < 0.5, 1e-3, 10.0) * rng.standard_normal(n)).astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1027, 4 * 256 * 1023, 4 * 256 * 1023 + 4, 3 * 2 ** 20 + 3])
def test_grad_norm(n):
    """out[0] against float64 grad_scale sqrt(sum g^2) within _step_ref.grad_norm_bound; out[1] within 1 ulp of the float32
    min(1, max_norm / (out[0] + 1e-6)), exactly 1.0f when that is >= 1 or max_norm <= 0.  Largest error / bound on an MI355X: 0.10."""
    dev = _dev()
    g0 = mixed_grad(n, n)
    seen = set()
    for scale, max_norm, gs in ((1.0, 10.0, 1.0), (1.0, 10.0, 1.0 / 3.0), (1e-3, 10.0, 1.0), (1.0, 0.0, 1.0 / 3.0), (1.0, -1.0, 1.0)):
        g = (g0 * np.float32(scale)).astype(np.float32)
        out = run_grad_norm(g, max_norm, gs, dev)
        ref = R.grad_norm(g, gs)
        ratio = abs(float(out[0]) - ref) / R.grad_norm_bound(n, ref)
        note(f"grad_norm n={n} scale={scale} gs={gs:.3f}", ratio)
        assert ratio < 1.0, (n, scale, max_norm, gs, out, ref)
        want = R.clip_coef_f32(out[0], max_norm)
        if want >= 1 or max_norm <= 0:
            assert bits1(out[1]) == 0x3F800000
        else:
            assert abs(bits1(out[1]) - bits1(want)) <= 1, (out, want)
        seen.add("one" if want >= 1 else "clipped")
    assert "one" in seen and (n < 1027 or "clipped" in seen)


def test_grad_norm_zero_and_nan():
    dev = _dev()
    for n in (5, 1027):
        out = run_grad_norm(np.zeros(n, np.float32), 10.0, 1.0, dev)
        assert R.bits32(out).tolist() == [0, 0x3F800000]  # norm +0, coefficient exactly 1
        g = mixed_grad(n, 3)
        g[n - 2] = np.nan
        out = run_grad_norm(g, 10.0, 1.0, dev)
        assert np.isnan(out).all()  # torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False)


# ================================================================== mia_optim_step
class State:
    """p, g, m, v of one optimizer case on the device, each inside its own guarded buffer."""

    def __init__(self, n, seed, dev, offset=0):
        p, m, v, self.sc = R.optim_case(n, seed)
        self.n = n
        self.p, self.m, self.v = (Guarded(n, torch.float32, dev, offset=offset).set(a) for a in (p, m, v))
        self.g = Guarded(n, torch.float32, dev, offset=offset)

    def host(self):
        return self.p.np().copy(), self.m.np().copy(), self.v.np().copy()

    def guards_ok(self):
        return self.p.guards_ok() and self.m.guards_ok() and self.v.guards_ok() and self.g.untouched()


def launch_step(kind, st, s, first, clip, grad_scale, dyn=None):
    mia_hip, ops = _abi()
    _p, cf = ops._p, ops._c_float
    v = None if kind == R.SGD else _p(st.v.view)
    if dyn is None:
        mia_hip.call("mia_optim_step", _p(st.p.view), _p(st.g.view), _p(st.m.view), v, ops._c_i64(st.n), kind, cf(s["lr"]), cf(s["beta1"]),
                     cf(s["beta2"]), cf(s["eps"]), cf(s["wd"]), cf(s["bc1"]), cf(s["bc2"]), int(first), _p(clip), cf(grad_scale), ops._stream())
    else:
        mia_hip.call("mia_optim_step_dyn", _p(st.p.view), _p(st.g.view), _p(st.m.view), v, ops._c_i64(st.n), kind, cf(s["beta1"]),
                     cf(s["beta2"]), cf(s["eps"]), cf(s["wd"]), dyn, _p(clip), cf(grad_scale), ops._stream())


def check_step(kind, before, g, after, s, first, tag):
    r = R.step(kind, before[0], g, before[1], before[2], s, first)
    worst = 0.0
    for name, got in zip("pmv" if kind != R.SGD else "pm", after):
        assert np.isfinite(got).all(), (tag, name)
        ratio = float((np.abs(got.astype(np.float64) - r[name]) / r["bound_" + name]).max())
        note(f"{tag} {name}", ratio)
        assert ratio < 1.0, (tag, name, ratio)
        worst = max(worst, ratio)
    if kind == R.SGD:
        assert np.array_equal(R.bits32(after[2]), R.bits32(before[2])), "SGD touched v"
    return worst


def run_chain(kind_name, n, gs, clip_mode, dev, offset=0, steps=3):
    """Three chained steps.  Before each one the device's own p, m, v are read back and fed to the restatement, so every bound is
    per step.  lr = 1e-2 t, wd = 0.1, eps = 1e-3 without a clip buffer and 1e-8 with one; the gradient is rescaled so that
    grad_scale ||g|| is 25 at step 2 (clipped at max_norm 10) and 2.5 at steps 1 and 3 (not clipped)."""
    mia_hip, ops = _abi()
    kind = R.KINDS[kind_name]
    st = State(n, 1000 * kind + n, dev, offset)
    eps = 1e-3 if clip_mode == "none" else 1e-8
    coefs = []
    for t in (1, 2, 3)[:steps]:
        g = R.optim_grad(st.sc, seed=7 * n + t)
        g = (g * ((25.0 if t == 2 else 2.5) / max(R.grad_norm(g, gs), 1e-30))).astype(np.float32)
        st.g.set(g)
        clip, c1 = None, 1.0
        if clip_mode != "none":
            out = Guarded(2, torch.float32, dev)
            ws = torch.full((mia_hip.lib().mia_grad_norm_workspace(),), NAN, device=dev)
            mia_hip.call("mia_grad_norm", ops._p(st.g.view), ops._c_i64(n), ops._c_float(10.0 if clip_mode == "clip" else 0.0), ops._c_float(gs),
                         ops._p(ws), ops._p(out.view), ops._stream())
            clip, c1 = out.view, float(out.np()[1])
            coefs.append(c1)
        s = R.kernel_scalars(1e-2 * t, 0.9, 0.0 if kind == R.SGD else 0.999, eps, WD, t, clip1=c1, grad_scale=gs)
        before = st.host()
        launch_step(kind, st, s, t == 1, clip, gs)
        torch.cuda.synchronize()
        assert st.guards_ok(), "wrote outside p / m / v, or into g"
        check_step(kind, before, g, st.host(), s, t == 1, f"optim {kind_name} n={n} gs={gs:.3f} {clip_mode} t={t}")
    if clip_mode == "clip" and steps == 3:
        assert coefs[0] == 1.0 and coefs[2] == 1.0 and 0.39 < coefs[1] < 0.41, coefs
    if clip_mode == "zero":
        assert coefs == [1.0] * len(coefs)


@pytest.mark.parametrize("clip_mode", ["none", "clip", "zero"])
@pytest.mark.parametrize("gs", [1.0, 1.0 / 3.0], ids=["1", "3"])
@pytest.mark.parametrize("kind", ["adam", "adamw", "sgd"])
def test_optim_step(kind, gs, clip_mode):
    """p, m and v after each of three chained steps, inside the bounds of _step_ref.step at every element, for 1, 3, 4, 5, 1027 and
    10007 elements.  Largest error / bound on an MI355X: p 0.40, m 0.50, v 0.52
    (test_optim_step_dyn_is_bit_identical: 0.41)."""
    dev = _dev()
    for n in (1, 3, 4, 5, 1027, 10007):
        run_chain(kind, n, gs, clip_mode, dev)


@pytest.mark.parametrize("kind", ["adam", "adamw", "sgd"])
def test_optim_step_wraps_the_grid(kind):
    """3 * 2^20 + 3 elements: the grid-stride loop wraps the 8192 x 256 grid and ends in a ragged tail."""
    run_chain(kind, 3 * 2 ** 20 + 3, 1.0 / 3.0, "clip", _dev(), steps=2)


def test_optim_step_on_a_slice():
    """A slice that starts 4 elements into a larger buffer (a FlatOptimizer live run)."""
    run_chain("adamw", 1027, 1.0, "clip", _dev(), offset=4)


def test_step_dyn_set_bytes():
    mia_hip, ops = _abi()
    dev = _dev()
    for lr, bc1, bc2, first, seed, off in ((0.0123, 0.1, 0.001, True, 2 ** 63 + 0x1234567, 2 ** 32 + 5), (3e-4, 0.271, 0.002997, False, 2 ** 64 - 1, 2 ** 40 + 3)):
        buf = Guarded(32, torch.uint8, dev, fill=0xA5)
        mia_hip.call("mia_step_dyn_set", ops._p(buf.view), ops._c_float(lr), ops._c_float(bc1), ops._c_float(bc2), int(first),
                     ctypes.c_uint64(seed), ctypes.c_uint64(off), ops._stream())
        torch.cuda.synchronize()
        assert bytes(buf.np().tolist()) == R.dyn_bytes(lr, bc1, bc2, first, seed, off) and buf.guards_ok()
    sd = ops.StepDyn(dev)  # the wrapper the engine uses writes the same bytes
    sd.set(0.0123, 0.1, 0.001, True, 2 ** 63 + 0x1234567, 2 ** 32 + 5)
    assert bytes(sd.dev.cpu().numpy().tolist()) == R.dyn_bytes(0.0123, 0.1, 0.001, True, 2 ** 63 + 0x1234567, 2 ** 32 + 5)


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("kind", ["adam", "adamw", "sgd"])
def test_optim_step_dyn_is_bit_identical(kind, first):
    """mia_optim_step_dyn, its scalars read from the 32 bytes mia_step_dyn_set wrote, against mia_optim_step with the same scalars
    as arguments: p, m, v bit for bit (wd 0.1 and wd 0, the branch the bounded cases do not take)."""
    mia_hip, ops = _abi()
    dev = _dev()
    k, n = R.KINDS[kind], 1027
    for wd in (WD, 0.0):
        s = R.kernel_scalars(0.0123, 0.9, 0.0 if k == R.SGD else 0.999, 1e-8, wd, 3)
        a, b = State(n, 5, dev), State(n, 5, dev)
        g = R.optim_grad(a.sc, 9)
        a.g.set(g), b.g.set(g)
        clip = torch.tensor([NAN, 0.37], device=dev)
        sd = ops.StepDyn(dev)
        sd.set(s["lr"], s["bc1"], s["bc2"], bool(first), 1, 2)
        launch_step(k, a, s, first, clip, 1.0 / 3.0)
        launch_step(k, b, s, first, clip, 1.0 / 3.0, dyn=sd.f32_ptr)
        torch.cuda.synchronize()
        assert a.guards_ok() and b.guards_ok()
        for x, y in zip(a.host(), b.host()):
            assert np.array_equal(R.bits32(x), R.bits32(y))
        check_step(k, State(n, 5, dev).host(), g, a.host(), dict(s, cs=float(np.float32(0.37) * np.float32(1.0 / 3.0))), bool(first),
                   f"optim_dyn {kind} first={first} wd={wd}")


@pytest.mark.parametrize("kind", ["adam", "adamw", "sgd"])
def test_flat_optimizer_skips_a_parameter_without_gradient(kind):
    """Three parameters of 5, 7 and 64 elements, the middle one without a gradient (autograd never reaches it): after step() its
    p, m, v and every padding element of the flat buffers are bit-unchanged, the live parameters are inside the bounds.  Largest error /
    bound on an MI355X: 0.32."""
    from training.engine import FlatOptimizer
    mia_hip, ops = _abi()
    dev = _dev()
    g = torch.Generator().manual_seed(4)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b, self.c = (torch.nn.Parameter(torch.randn(k, generator=g)) for k in (5, 7, 64))

    net = Net().to(dev)
    opt = FlatOptimizer(net, kind, lr=1e-2, weight_decay=WD, eps=1e-8)
    assert opt.offsets == [0, 64, 72] and opt.flat_param.numel() == 80
    live, dead, pads = [(0, 64), (72, 77)], (64, 71), [71, 77, 78, 79]
    bufs = [opt.m] + ([opt.v] if opt.v is not None else [])
    for i, buf in enumerate(bufs):
        buf.copy_((torch.rand(80, generator=g) * 0.1 + 0.01 * i).to(dev))
        buf[pads[1]:] = 0.0
    for buf in [opt.flat_param] + bufs:
        buf[pads[0]] = 7.0  # the dead parameter's padding: outside every live run, so even a sentinel must survive
    x = torch.randn(64, generator=g).to(dev)
    opt.zero_grad()
    loss = 0.5 * (net.a * net.a).sum() + (net.c * x).sum()
    loss.backward()
    assert net.b.grad is None and net.a.grad is not None
    before = [opt.flat_param.cpu().numpy().copy(), opt.m.cpu().numpy().copy(), opt.v.cpu().numpy().copy() if opt.v is not None else np.zeros(80, np.float32)]
    gh = opt.flat_grad.cpu().numpy().copy()
    assert not gh[64:72].any() and gh[72:77].all() and gh[:64].all() and not gh[77:].any()
    opt.step(max_grad_norm=10.0, grad_scale=1.0)
    torch.cuda.synchronize()
    after = [opt.flat_param.cpu().numpy(), opt.m.cpu().numpy(), opt.v.cpu().numpy() if opt.v is not None else np.zeros(80, np.float32)]
    keep = list(range(dead[0], dead[1] + 1)) + pads[1:]
    for b4, af in zip(before, after):
        assert np.array_equal(R.bits32(b4[keep]), R.bits32(af[keep])), "a gradient-less parameter or a padding element changed"
    c1 = float(opt.last_norm.cpu().numpy()[1])
    k = R.KINDS[kind]
    s = R.kernel_scalars(1e-2, 0.9, 0.0 if k == R.SGD else 0.999, 1e-8, WD, 1, clip1=c1, grad_scale=1.0)
    for lo, hi in live:
        check_step(k, [b[lo:hi] for b in before], gh[lo:hi], [a[lo:hi] for a in after], s, True, f"flat {kind} [{lo}:{hi}]")
    assert torch.equal(net.a.data, opt.flat_param[72:77]) and net.a.data.data_ptr() == opt.flat_param.data_ptr() + 4 * 72


# ================================================================== mia_scale_by_clip
@pytest.mark.parametrize("n", [1, 1027, 3 * 2 ** 20 + 3])
def test_scale_by_clip(n):
    mia_hip, ops = _abi()
    dev = _dev()
    x = mixed_grad(n, n + 1)
    x[0] = -0.0
    for c in (0.37, 1.0):
        buf = Guarded(n, torch.float32, dev).set(x)
        clip = torch.tensor([NAN, c], device=dev)
        mia_hip.call("mia_scale_by_clip", ops._p(buf.view), ops._c_i64(n), ops._p(clip), ops._stream())
        torch.cuda.synchronize()
        assert buf.guards_ok()
        want = x if c == 1.0 else x * np.float32(c)
        assert want.dtype == np.float32 and np.array_equal(R.bits32(buf.np()), R.bits32(want)), c
        if c == 1.0:
            assert buf.untouched() and R.bits32(buf.np())[0] == 0x80000000


# ================================================================== mia_pack_weight
NAIVE = [(1, 1, 1, 1), (3, 16, 1, 1), (5, 7, 3, 3), (16, 130, 5, 5)]
TILED = [(64, 64, 3, 3), (96, 40, 3, 3), (65, 17, 2, 2), (130, 96, 3, 3)]
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}


def run_pack(w, dt, n_from_d0, extra, dev):
    mia_hip, ops = _abi()
    d0, d1, taps = w.shape[0], w.shape[1], w.shape[2] * w.shape[3]
    nn, kk = (d0, d1) if n_from_d0 else (d1, d0)
    kb = 32 if dt == "bf16" else 16
    npad, kpad = R.pad_to(nn, 64) + 64 * extra, R.pad_to(kk, kb) + kb * extra
    naive = npad * kpad < 4096 or taps > 16
    dst, wd = Guarded(taps * npad * kpad, TDT[dt], dev), w.to(dev)
    mia_hip.call("mia_pack_weight", ops._p(wd), ops._p(dst.view), G.dt_id(dt), d0, d1, taps, npad, kpad, int(n_from_d0), ops._stream())
    torch.cuda.synchronize()
    ref = R.pack_weight(w, n_from_d0, npad, kpad).to(TDT[dt])
    assert dst.guards_ok(), "wrote outside the packed buffer"
    assert torch.equal(raw(dst.view.cpu()), raw(ref.reshape(-1))), (tuple(w.shape), dt, n_from_d0, extra)
    return naive


@pytest.mark.parametrize("n_from_d0", [1, 0])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", NAIVE + TILED, ids=lambda s: "x".join(map(str, s)))
def test_pack_weight(shape, dt, n_from_d0):
    """dst[t][n][k] = w[n][k][t] (n_from_d0) or w[k][n][t], zero padded, bit for bit (bf16: `.to(torch.bfloat16)`)."""
    g = torch.Generator().manual_seed(sum(shape))
    assert run_pack(torch.randn(*shape, generator=g), dt, n_from_d0, 0, _dev()) == (shape in NAIVE)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_pack_weight_extra_padding(dt):
    """npad and kpad one brick larger than the minimum: the extra rows and columns are written as zeros."""
    g = torch.Generator().manual_seed(8)
    for shape in ((96, 40, 3, 3), (5, 7, 3, 3), (65, 17, 2, 2)):
        for n_from_d0 in (1, 0):
            run_pack(torch.randn(*shape, generator=g), dt, n_from_d0, 1, _dev())


@pytest.mark.parametrize("dt,small", [("bf16", 30), ("f32", 30), ("f32", 60)], ids=["bf16-38", "f32-38", "f32-68"])
def test_pack_weight_batch(dt, small):
    """ops.PackPlan.repack (one mia_pack_weight_batch launch; fp32 also mia_amax_batch and mia_split_f16_batch) against the DEFINITION of
    the packed layout, of the maximum and of the split words: 8 + `small` tensors in both orientations make 76 / 136 descriptors, so
    a block's descriptor search takes two / three ballot rounds; taps 9, 4, 1 and 3 (1 x 3)."""
    mia_hip, ops = _abi()
    dev = _dev()
    g = torch.Generator().manual_seed(small)
    tiny = [(2, 3, 1, 1), (3, 2, 2, 2), (2, 2, 3, 3), (2, 5, 1, 3)]
    shapes = NAIVE[:3] + TILED + [(4, 6, 1, 3)] + [tiny[i % 4] for i in range(small)]
    ws = [torch.nn.Parameter(torch.randn(*s, generator=g).to(dev)) for s in shapes]
    dtid = G.dt_id(dt)
    for w in ws:
        for orient in (True, False):
            ops.pack_cache(w).get(w, dtid, n_from_d0=orient)
    plan = ops.PackPlan(ws, dtid)
    assert len(plan.entries) == 2 * len(ws) > (128 if small == 60 else 64)
    with torch.no_grad():
        for i, w in enumerate(ws):
            w.mul_(1.7).add_(0.01)
            if i == 5:
                w.mul_(2.0 ** -30)  # a tensor whose maximum sits far from the others'
    for e in plan.entries:
        e[3].fill_(NAN)  # the packed copies: all of it, zero padding included, must be rewritten
    if dt == "f32":
        plan.amax_slots.fill_(0x7FFFFFFF)
        for sp in plan.split_bufs:
            sp.fill_(-1)
    ops.bump_param_epoch()
    plan.repack()
    torch.cuda.synchronize()
    for i, (w, pc, key, buf, npad, kpad, _) in enumerate(plan.entries):
        got, npad2, kpad2 = ops.pack_cache(w).get(w, dtid, n_from_d0=key[1])  # planted by the plan: no launch
        assert got.data_ptr() == buf.data_ptr() and (npad, kpad) == (npad2, kpad2)
        ref = R.pack_weight(w, key[1], npad, kpad).to(TDT[dt])
        assert torch.equal(raw(got.cpu()), raw(ref)), (tuple(w.shape), key)
        if dt == "f32":
            pat = R.amax_bits(w.detach().cpu().numpy())
            assert int(plan.amax_slots[i].item()) == pat, (tuple(w.shape), key)
            words = plan.split_bufs[i].cpu().numpy().view(np.uint32)
            assert np.array_equal(words, R.split_f16(ref.numpy(), pat)), (tuple(w.shape), key)


# ================================================================== mia_split_f16_batch, mia_amax_batch
def test_split_f16_batch():
    """Words h | l << 16 of x 2^e, bit for bit.  common.h says subnormal low parts are kept: the fourth tensor has them."""
    mia_hip, ops = _abi()
    dev = _dev()
    rng = np.random.default_rng(12)
    xs = [rng.standard_normal(64), rng.standard_normal(1024) * 37.0, rng.standard_normal(200704) * 1e-3, rng.standard_normal(4096), np.zeros(256)]
    xs = [x.astype(np.float32) for x in xs]
    xs[3][::2] *= np.float32(2.0 ** -20)
    xs[1][5] = -0.0
    refs = [R.split_f16(x, R.amax_bits(x)) for x in xs]
    lo = (refs[3][::2] >> np.uint32(16)) & np.uint32(0x7FFF)
    assert ((lo > 0) & (lo < 0x400)).any()
    for pick in ([1], [0, 1, 2, 3, 4]):
        src = [torch.from_numpy(xs[i]).to(dev) for i in pick]
        dst = [Guarded(xs[i].size, torch.int32, dev, fill=-1) for i in pick]
        slots = torch.tensor([R.amax_bits(xs[i]) for i in pick], dtype=torch.int32, device=dev)
        descs = ops._split_descs([(s, d.view, slots[j:j + 1]) for j, (s, d) in enumerate(zip(src, dst))], dev)
        mia_hip.call("mia_split_f16_batch", ops._p(descs), len(pick), ops._stream())
        torch.cuda.synchronize()
        for j, i in enumerate(pick):
            assert dst[j].guards_ok()
            got = dst[j].np().view(np.uint32)
            bad = np.flatnonzero(got != refs[i])
            assert bad.size == 0, (i, bad[:5], [hex(v) for v in got[bad[:5]]], [hex(v) for v in refs[i][bad[:5]]])


def test_amax_batch():
    """Each slot holds the bit pattern of max |x| of its tensor; the slots start as garbage (the launch zeroes them itself)."""
    mia_hip, ops = _abi()
    dev = _dev()
    rng = np.random.default_rng(13)
    xs = [rng.standard_normal(n).astype(np.float32) for n in (1, 3, 1023, 70001, 1000, 1027, 1027)]
    xs[3][-1] = -77.0   # the maximum in the scalar tail, negative
    xs[4][77] = np.nan
    xs[5][0] = 55.0     # the maximum in the scalar head of a start that is not 16-byte aligned
    xs[6][-2] = -66.0
    front = [5 if i >= 5 else 4 for i in range(len(xs))]  # 1e9 on both sides: reading outside the tensor shows
    bufs = [torch.from_numpy(np.concatenate([np.full(f, 1e9, np.float32), x, np.full(4, 1e9, np.float32)])).to(dev) for f, x in zip(front, xs)]
    views = [b[f:f + x.size] for f, b, x in zip(front, bufs, xs)]
    assert views[0].data_ptr() % 16 == 0 and views[5].data_ptr() % 16 == 4

    class ADesc(ctypes.Structure):
        _fields_ = [("src", ctypes.c_void_p), ("n", ctypes.c_int64)]

    assert ctypes.sizeof(ADesc) == mia_hip.lib().mia_amax_desc_bytes()
    arr = (ADesc * len(xs))(*[ADesc(v.data_ptr(), v.numel()) for v in views])
    descs = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    slots = Guarded(len(xs), torch.int32, dev, fill=0x7FFFFFFF)
    mia_hip.call("mia_amax_batch", ops._p(descs), len(xs), ops._p(slots.view), ops._stream())
    torch.cuda.synchronize()
    assert slots.guards_ok()
    got = slots.np().view(np.uint32).tolist()
    assert got == [R.amax_bits(x) for x in xs]
    assert np.isnan(np.array(got[4], np.uint32).view(np.float32)) and got[5] == bits1(np.float32(55.0)) and got[3] == bits1(np.float32(77.0))


# ================================================================== mia_relayout
def special(t):
    """NaN, +-inf and -0.0 at fixed places of a tensor with at least four elements."""
    f = t.view(-1)
    if f.numel() >= 4:
        f[0], f[1], f[2], f[3] = NAN, float("inf"), float("-inf"), -0.0
    return t


def run_relayout(src_view, dst_dtype, n, c, hw, sstr, dstr_of, dev):
    """dst: contiguous tensor whose logical (n, c, p) strides are dstr_of; returns it as [n, c, hw] logical view."""
    mia_hip, ops = _abi()
    i64 = ops._c_i64
    dst = Guarded(n * c * hw, dst_dtype, dev)
    mia_hip.call("mia_relayout", ops._p(src_view), ops._dt(src_view), ops._p(dst.view), ops._dt(dst.view), n, c, i64(hw), i64(sstr[0]), i64(sstr[1]),
                 i64(sstr[2]), i64(dstr_of[0]), i64(dstr_of[1]), i64(dstr_of[2]), ops._stream())
    torch.cuda.synchronize()
    assert dst.guards_ok()
    return torch.as_strided(dst.view, (n, c, hw), dstr_of)


@pytest.mark.parametrize("direction", ["to_nhwc", "to_nchw"])
@pytest.mark.parametrize("sd,dd", [("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16")])
def test_relayout(sd, dd, direction):
    """Bit-exact against permute / .to(), c = 1, 3, 5, 64 x hw = 1, 7, 1961, two images; NaN, +-inf and -0.0 survive."""
    dev = _dev()
    g = torch.Generator().manual_seed(6)
    n = 2
    for c in (1, 3, 5, 64):
        for hw in (1, 7, 1961):
            nchw, nhwc = (c * hw, hw, 1), (c * hw, 1, c)  # strides of (image, channel, pixel)
            sstr, dstr = (nchw, nhwc) if direction == "to_nhwc" else (nhwc, nchw)
            logical = special(torch.randn(n, c, hw, generator=g).to(TDT[sd]))
            src = torch.empty(n * c * hw, dtype=TDT[sd])
            torch.as_strided(src, (n, c, hw), sstr).copy_(logical)
            got = run_relayout(src.to(dev), TDT[dd], n, c, hw, sstr, dstr, dev)
            assert same_bits(got, logical.to(TDT[dd])), (sd, dd, direction, c, hw)
            assert int(torch.isnan(got).sum()) == int(torch.isnan(logical).sum()), "an element was never written"


def test_relayout_wraps_the_grid():
    dev = _dev()
    n, c, hw = 1, 5, 1024 * 820  # 4,198,400 elements > 16384 x 256
    g = torch.Generator().manual_seed(7)
    x = torch.randn(n, c, hw, generator=g)
    got = run_relayout(x.to(dev), torch.bfloat16, n, c, hw, (c * hw, hw, 1), (c * hw, 1, c), dev)
    assert same_bits(got, x.to(torch.bfloat16))


def test_relayout_through_ops():
    """ops.to_nhwc of a channel slice of a larger NCHW tensor, and ops.cast_nhwc."""
    mia_hip, ops = _abi()
    dev = _dev()
    g = torch.Generator().manual_seed(8)
    big = special(torch.randn(2, 9, 7, 11, generator=g))
    for dt in (torch.float32, torch.bfloat16):
        for src_dt in (torch.float32, torch.bfloat16):
            bd = big.to(src_dt).to(dev)
            sl = bd[:, 2:7]
            assert not sl.is_contiguous()
            got = ops.to_nhwc(sl, dt)
            assert got.shape == (2, 7, 11, 5) and got.is_contiguous()
            assert same_bits(got, big.to(src_dt)[:, 2:7].permute(0, 2, 3, 1).contiguous().to(dt))
            if src_dt != dt:
                x = special(torch.randn(2, 7, 11, 5, generator=g)).to(src_dt)
                assert same_bits(ops.cast_nhwc(x.to(dev), dt), x.to(dt))


@pytest.mark.parametrize("layout", ["channels_last", "contiguous"])
def test_to_nhwc_gradient(layout):
    """The gradient of ops.to_nhwc for an image that requires one: the same kernel backwards, into the image's own layout and dtype."""
    mia_hip, ops = _abi()
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 5, 7, 11, generator=g).to(dev)
    if layout == "channels_last":
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    out_dt = torch.bfloat16 if layout == "channels_last" else torch.float32
    y = ops.to_nhwc(x, out_dt)
    assert y.requires_grad and same_bits(y, x.detach().cpu().permute(0, 2, 3, 1).contiguous().to(out_dt))
    gout = torch.randn(2, 7, 11, 5, generator=g).to(out_dt)
    y.backward(gout.to(dev))
    torch.cuda.synchronize()
    assert x.grad.shape == x.shape and x.grad.dtype == torch.float32 and x.grad.stride() == x.stride()
    assert same_bits(x.grad.cpu().contiguous(), gout.permute(0, 3, 1, 2).contiguous().float())


# ================================================================== mia_colsum
def run_colsum(x_np, dt, c, accumulate, dev, byte_offset=0):
    """Returns (device sums, float64 sums, bound).  x sits in a NaN-filled buffer, so a read outside it shows in the sums."""
    mia_hip, ops = _abi()
    p = x_np.shape[0]
    eoff = byte_offset // (2 if dt == "bf16" else 4)
    x = Guarded(p * c, TDT[dt], dev, offset=eoff).set(torch.from_numpy(x_np).reshape(-1))
    aligned = x.view.data_ptr() % 16 == 0
    assert aligned == (byte_offset == 0)
    xs = x.view.float().cpu().double().view(p, c)  # the stored values
    nws = mia_hip.lib().mia_colsum_workspace(ops._c_i64(p), c)
    assert nws == R.colsum_blocks(p) * c
    ws = Guarded(nws, torch.float32, dev)
    prev = np.linspace(-3.0, 5.0, c).astype(np.float32)
    out = Guarded(c, torch.float32, dev)
    if accumulate:
        out.set(prev)
    mia_hip.call("mia_colsum", ops._p(x.view), G.dt_id(dt), ops._c_i64(p), c, ops._p(ws.view), ops._p(out.view), accumulate, ops._stream())
    torch.cuda.synchronize()
    assert x.untouched() and ws.guards_ok() and out.guards_ok()
    assert bool(torch.isfinite(ws.view).all()) and bool(torch.isfinite(out.view).all())
    ref = xs.sum(0).numpy() + (prev.astype(np.float64) if accumulate else 0.0)
    mag = xs.abs().sum(0).numpy() + (np.abs(prev).astype(np.float64) if accumulate else 0.0)
    k = R.colsum_k(p, c, dt == "bf16", c % 64 == 0 and aligned, accumulate)
    return out.np().astype(np.float64), ref, k * R.U * mag + R.ulp32(ref)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_colsum(dt, accumulate):
    """out[c] (+)= sum_p x[p][c] against float64 sums of the stored values, within (additions on the path, _step_ref.colsum_k) * 2^-24 *
    sum |x| + 1 ulp per channel.  Largest error / bound on an MI355X: 0.05 (test_colsum_misaligned: 0.03)."""
    dev = _dev()
    rng = np.random.default_rng(14)
    worst = 0.0
    for c in (1, 3, 64, 96, 128, 300, 320):
        for p in (1, 63, 64, 65, 1000, 16384 + 37):
            x = (rng.standard_normal((p, c)) + 0.25).astype(np.float32)
            got, ref, bound = run_colsum(x, dt, c, accumulate, dev)
            ratio = float((np.abs(got - ref) / bound).max())
            assert ratio < 1.0, (dt, c, p, accumulate, ratio)
            worst = max(worst, ratio)
    note(f"colsum {dt} acc={accumulate}", worst)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_colsum_misaligned(dt):
    """x 4 bytes past a 16-byte boundary with c % 64 == 0: the vector kernel is refused, the generic one answers."""
    dev = _dev()
    rng = np.random.default_rng(15)
    for c in (64, 128):
        for p in (65, 1000):
            for accumulate in (0, 1):
                got, ref, bound = run_colsum((rng.standard_normal((p, c)) + 0.25).astype(np.float32), dt, c, accumulate, dev, byte_offset=4)
                ratio = float((np.abs(got - ref) / bound).max())
                note(f"colsum_misaligned {dt} c={c} p={p}", ratio)
                assert ratio < 1.0, (dt, c, p, accumulate, ratio)


# ================================================================== mia_add
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_add(dt):
    """fp32: numpy float32 a + b; bf16: (a.float() + b.float()).to(bfloat16); bit for bit, one size past 8192 x 256 units."""
    mia_hip, ops = _abi()
    dev = _dev()
    g = torch.Generator().manual_seed(16)
    epu = 8 if dt == "bf16" else 4
    for n in (1, 7, 8, 9, 1027, 8192 * 256 * epu + 300 * epu + 3):
        a, b = (special(torch.randn(n, generator=g) * 3.0).to(TDT[dt]) for _ in range(2))
        out = Guarded(n, TDT[dt], dev)
        ad, bd = a.to(dev), b.to(dev)
        mia_hip.call("mia_add", ops._p(ad), ops._p(bd), ops._p(out.view), G.dt_id(dt), ops._c_i64(n), ops._stream())
        torch.cuda.synchronize()
        assert out.guards_ok()
        if dt == "f32":
            with np.errstate(invalid="ignore"):
                ref = torch.from_numpy(a.numpy() + b.numpy())
        else:
            ref = (a.float() + b.float()).to(torch.bfloat16)
        assert same_bits(out.view, ref), (dt, n)
        assert int(torch.isnan(out.view).sum()) == int(torch.isnan(ref).sum()), "an element was never written"


# ================================================================== Dropout2d masks
SEED, OFFSET = 2 ** 63 + 0x9E3779B97F4A7C15 % 2 ** 62, 2 ** 40 + 12


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1001, 2 ** 20 + 4 * 256 + 1])
def test_dropout_mask(n):
    """Bit-exact against the Philox4x32-10 restatement; survivors carry the bits of float32(1) / float32(keep)."""
    mia_hip, ops = _abi()
    dev = _dev()
    for keep in (1.0, 0.5, 0.9):
        out = Guarded(n, torch.float32, dev)
        mia_hip.call("mia_dropout_mask", ops._p(out.view), ops._c_i64(n), ops._c_float(keep), ctypes.c_uint64(SEED), ctypes.c_uint64(OFFSET), ops._stream())
        torch.cuda.synchronize()
        assert out.guards_ok()
        ref = R.dropout_mask(n, keep, SEED, OFFSET)
        assert np.array_equal(R.bits32(out.np()), R.bits32(ref)), (n, keep)
        assert set(R.bits32(out.np()).tolist()) <= {0, bits1(np.float32(1) / np.float32(keep))}


def test_dropout_mask_dyn():
    """(seed, base) in device memory plus rel_offset = the plain form at base + rel_offset; one case carries across 2^32."""
    mia_hip, ops = _abi()
    dev = _dev()
    n = 1001
    for base, rel in ((OFFSET, 4 * 251), (2 ** 32 - 8, 16), (2 ** 33 - 4, 2 ** 32 + 8)):
        sd = ops.StepDyn(dev)
        sd.set(1e-3, 0.1, 0.001, False, SEED, base)
        a, b = Guarded(n, torch.float32, dev), Guarded(n, torch.float32, dev)
        mia_hip.call("mia_dropout_mask_dyn", ops._p(a.view), ops._c_i64(n), ops._c_float(0.9), sd.u64_ptr, ctypes.c_uint64(rel), ops._stream())
        mia_hip.call("mia_dropout_mask", ops._p(b.view), ops._c_i64(n), ops._c_float(0.9), ctypes.c_uint64(SEED), ctypes.c_uint64(base + rel), ops._stream())
        torch.cuda.synchronize()
        assert a.guards_ok() and b.guards_ok()
        ref = R.dropout_mask(n, 0.9, SEED, base + rel)
        assert np.array_equal(R.bits32(a.np()), R.bits32(ref)) and np.array_equal(R.bits32(b.np()), R.bits32(ref)), (base, rel)


# ================================================================== mia_zero, mia_gather_f32, mia_widen_u8_i64
def test_zero():
    mia_hip, ops = _abi()
    dev = _dev()
    for nbytes in (16, 8 * 2 ** 20 + 48):
        buf = Guarded(nbytes // 4, torch.int32, dev, fill=0x5A5A5A5A)
        mia_hip.call("mia_zero", ops._p(buf.view), ops._c_i64(nbytes), ops._stream())
        torch.cuda.synchronize()
        assert buf.guards_ok() and int(buf.view.count_nonzero()) == 0


def test_gather():
    mia_hip, ops = _abi()
    dev = _dev()
    for n in (257, 1000):
        for stride in (1, 3):
            src = torch.arange(5 + n * stride, dtype=torch.float32) * 0.5 - 7.0
            dst = Guarded(n, torch.float32, dev)
            sd = src.to(dev)
            mia_hip.call("mia_gather_f32", ops._p(sd[5:]), ops._c_i64(stride), ops._p(dst.view), n, ops._stream())
            torch.cuda.synchronize()
            assert dst.guards_ok() and torch.equal(dst.view.cpu(), src[5::stride][:n])


def test_widen_u8_i64():
    mia_hip, ops = _abi()
    dev = _dev()
    g = torch.Generator().manual_seed(17)
    for n in (1, 2, 3, 255, 2049, 1000001):
        lab = torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8)
        if n >= 255:
            lab[:255] = torch.arange(255, dtype=torch.uint8)
            lab[-1] = 255
        src = Guarded(n, torch.uint8, dev, fill=0xEE).set(lab)
        dst = Guarded(n, torch.int64, dev, fill=-1)
        assert src.view.data_ptr() % 8 == 0 and dst.view.data_ptr() % 16 == 0
        mia_hip.call("mia_widen_u8_i64", ops._p(src.view), ops._p(dst.view), ops._c_i64(n), ops._stream())
        torch.cuda.synchronize()
        assert src.untouched() and dst.guards_ok()
        assert torch.equal(dst.view.cpu(), lab.to(torch.int64)), n
        if n >= 2049:
            assert len(torch.unique(dst.view)) == 256
