"""GPU checks of csrc/norm.hip at kernel level: every dispatch branch of the finalize, forward-apply, backward reduce / finalize /
apply, statistics and synchronised-batch-norm entry points against the float64 restatement in tests/_norm_ref.py, called through
the C ABI (mia_hip.call / ops._p).  Inputs are seeded and exactly representable in the storage dtype on both sides.

Branch -> case (test, parameters):
  mia_norm_finalize
    inline sums (n * tiles <= 1024) ................ test_finalize_routes[(2,1)], [(3,300)]
    norm_fwd_sum_kernel<true> (long, instance) ..... test_finalize_routes[instance-(4,300) | (4,517) | (2,1025) | (5,250)]
    norm_fwd_sum_kernel<false> + finalize (batch) .. test_finalize_routes[batch-(4,300) | (4,517) | (2,1025) | (5,250)]
      a tile lane tl = 0..63 starts at t = tl, takes 256 tiles per unrolled pass while t + 192 < tiles, then strides of 64:
      tiles = 300, 517, 1025 (44, 5, 1 mod 256): 1, 2, 4 unrolled passes, then ONE remainder stride on lanes tl < 44, 5, 1;
      tiles = 250: lanes tl < 58 take one unrolled pass and no remainder, lanes tl >= 58 take no unrolled pass and THREE
      remainder strides (lane 58 sits on the guard's boundary, t + 192 == tiles, lane 57 reads the last tile in its pass);
      `ch < c` edge of the 16-channel groups at C = 20
    eval mode (partials = NULL, running stats) ..... test_finalize_routes[batch_eval-*]
    drop_scale with an exact 0 and 1/keep; ysum .... test_finalize_routes[drop=1 / ysum=1]
    E[y^2] - mean^2 at mean = r std ................ test_finalize_offset_mean[r = 0, 2, 8]
  mia_norm_act_fwd
    non-vector kernel (C % EPU != 0) ............... test_forward_apply[C=7; C=12 bf16; C=20 bf16]
    stream kernel, 3 units per pixel ............... test_forward_apply[C=12 f32; C=24 bf16]
    stream kernel, units per pixel not 2^k ......... test_forward_apply[C=20 f32 (5); C=24 f32 (6); C=96 (24 / 12); C=160 (40 / 20)]
    misaligned y, z -> scalar kernel ............... test_forward_apply_misaligned
    amax by-product, stream and separate pass ...... test_forward_amax_is_the_bit_pattern_of_the_maximum
  mia_norm_act_bwd
    colreduce_vec_kernel CG = 64 ................... test_backward[C=32*2=64]        (two pieces: TWO = true)
    CG = 32 ........................................ test_backward[C=32, 160, 224]
    CG = 96 (252 / 240 live threads) ............... test_backward[C=96, 288]
    norm_act_bwd_reduce_kernel (generic) ........... test_backward[C=7, 12, 20, 24], test_backward_long_slab_sums[C=40]
    ragged last slab ............................... test_backward[slabs=3, 7]  (1961 = 2 * 654 + 653 = 6 * 281 + 275)
    norm_bwd_sum_kernel (n * slabs > 1024) ......... test_backward_long_slab_sums[n=3, slabs=400]
    stream apply / scalar apply .................... test_backward[C % EPU == 0 / else]
    TWO = false vector kernels ..................... test_backward_accumulates, test_backward_sums_only_is_bit_identical
    accumulate = 1 ................................. test_backward_accumulates
    fixed_stats = 1, ysum = NULL ................... test_backward_frozen_statistics
    ScaleLReLUFn call shape, dbias = NULL .......... test_backward_scale_lrelu_call_shape
    slope = 1.0 .................................... test_backward_slope_one
    misaligned dy only (vector reduce, scalar apply) test_backward_misaligned[dy]
    misaligned dz only (scalar reduce and apply) ... test_backward_misaligned[dz]
    misaligned dz2 ................................. test_backward_two_pieces_need_aligned_tensors
  mia_norm_bwd_sums ................................ test_backward_sums_only_is_bit_identical[C=64, 96, 160, 20]
  mia_norm_stats
    vector route CG = 64 / 96 / 32, slabs 1 and 5 .. test_stats[C=256 / 96 / 32, 160]
    generic route .................................. test_stats[C=20], test_stats_misaligned
    ops.global_avg_pool ............................ test_stats[slabs=1]
  sync batch norm .................................. test_sync_batch_norm_in_one_process[(1,3), (2,2)]

Tolerances (relerr = max |error| / max |reference|, in float64): fp32 tensors 2e-5 (TOL of test_gpu_ops.py); bf16 z 1.5 * 2^-8 and dy
2.5 * 2^-8, dgamma / dbeta (and the group means c1 / c2, which are the same sums over a pixel count) 1e-3, dbias absolutely within
1e-3 * max sum|dy| + 1e-4 (test_norm_streams_wide_bf16_vs_fp32_cpu); finalize coefficients: the derived bound of
test_finalize_offset_mean.  The dy comparison skips only elements whose REFERENCE pre-activation is within rounding of the
LeakyReLU kink (_norm_ref.near_zero; at most 1 % of a case, asserted on the CPU by tests/test_norm_host.py for this whole grid)."""

import pytest
import torch

import _norm_ref as R

pytestmark = pytest.mark.gpu

TOL32 = 2e-5
STEP = 2.0 ** -8
Z_TOL = {"f32": TOL32, "bf16": 1.5 * STEP}
DY_TOL = {"f32": TOL32, "bf16": 2.5 * STEP}
SUM_TOL = 1e-3
NAN = float("nan")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _abi():
    import mia_hip
    from mia_hip import ops
    return mia_hip, ops


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape
    assert bool(torch.isfinite(got).all()), "an output element was never written (or is not finite)"
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def act(t, dt, dev, misalign=False):
    """[N, P, C] float64 -> device tensor in the storage dtype; misalign: a view one element into its buffer (not 16-byte aligned)."""
    flat = torch.full((t.numel() + 8,), NAN, dtype=R.DT[dt], device=dev)
    off = 1 if misalign else 0
    v = flat[off:off + t.numel()].view(t.shape)
    v.copy_(t.to(R.DT[dt]))
    assert (v.data_ptr() % 16 != 0) == misalign
    return v


def f32(t, dev):
    return None if t is None else t.float().contiguous().to(dev)


def rows(r, dev):
    """[5, N, C] fp32 coefficient table (xa, xb, scale, shift, ysum) of a reference answer."""
    return torch.stack([r[k] for k in ("xa", "xb", "scale", "shift", "ysum")]).float().contiguous().to(dev)


def dt_id(dt):
    mia_hip, _ = _abi()
    return mia_hip.F32 if dt == "f32" else mia_hip.BF16


def mode_id(mode):
    mia_hip, _ = _abi()
    return mia_hip.NORM_INSTANCE if mode == "instance" else mia_hip.NORM_BATCH


# ================================================================== a / b: finalize
def run_finalize(part, n, tiles, c, hw, mode, training, drop, i, want_ysum, dev):
    mia_hip, ops = _abi()
    _p, cf = ops._p, ops._c_float
    coefs = torch.full((5, n, c), NAN, device=dev, dtype=torch.float32)
    batch = mode == "batch"
    rm, rv = (f32(i["running"][0], dev), f32(i["running"][1], dev)) if batch else (None, None)
    nbt = torch.zeros((), device=dev, dtype=torch.long) if batch else None
    gd, bd, dd, pd = f32(i["gamma"], dev), f32(i["beta"], dev), f32(drop, dev), (part.to(dev) if part is not None else None)
    mia_hip.call("mia_norm_finalize", _p(pd), n, tiles, c, ops._c_i64(hw), mode_id(mode), int(training), _p(dd), _p(gd), _p(bd),
                 cf(R.EPS), cf(R.MOM), _p(rm), _p(rv), _p(nbt), _p(coefs[0]), _p(coefs[1]), _p(coefs[2]), _p(coefs[3]),
                 _p(coefs[4]) if want_ysum else None, ops._stream())
    torch.cuda.synchronize()
    return coefs, rm, rv, nbt


def check_finalize(n, tiles, c, mode, training, drop, want_ysum, r, seed, dev):
    """One mia_norm_finalize call against R.coefficients on the SAME fp32 partials; bound = 2^-22 (1 + r^2), see
    test_finalize_offset_mean."""
    i = R.finalize_inputs(n, c, r, seed)
    hw = R.FINALIZE_P
    part = R.epilogue_partials(i["y"], tiles, seed=seed) if training else None
    m = i["m"] if drop else None
    got, rm, rv, nbt = run_finalize(part, n, tiles, c, hw, mode, training, m, i, want_ysum, dev)
    if training:
        s1, s2 = part[..., 0].double().sum(1), part[..., 1].double().sum(1)
    else:
        s1 = s2 = torch.zeros(n, c, dtype=torch.float64)  # eval mode reads no sums
    ref = R.coefficients(s1, s2, hw, i["gamma"], i["beta"], mode, m, training, i["running"] if mode == "batch" else None)
    bound = 2.0 ** -22 * (1.0 + r * r)
    errs = {k: rel(got[j], ref[k]) for j, k in enumerate(("xa", "xb", "scale", "shift"))}
    if want_ysum and training:
        errs["ysum"] = rel(got[4], ref["ysum"])
    if mode == "batch":
        errs["running_mean"], errs["running_var"] = rel(rm, ref["running"][0]), rel(rv, ref["running"][1])
        assert nbt.item() == (1 if training else 0)
        if not training:
            assert torch.equal(rm.cpu(), i["running"][0].float()) and torch.equal(rv.cpu(), i["running"][1].float())
    print(f"finalize n={n} tiles={tiles} c={c} {mode} train={training} drop={drop} r={r}: "
          + " ".join(f"{k}={v / bound:.3f}" for k, v in errs.items()) + f" (fractions of the bound {bound:.3e})")
    for k, v in errs.items():
        assert v <= bound, f"{k}: {v:.3e} > {bound:.3e}"
    if drop and training:  # a dropped channel: xa = scale = 0 exactly
        dead = (i["m"] == 0)
        assert bool(dead.any()) and not got[0].cpu()[dead].any() and not got[2].cpu()[dead].any()


@pytest.mark.parametrize("want_ysum", [0, 1])
@pytest.mark.parametrize("drop", [0, 1])
@pytest.mark.parametrize("c", [20, 64])
@pytest.mark.parametrize("n,tiles", R.FINALIZE_NT)
@pytest.mark.parametrize("mode", ["instance", "batch", "batch_eval"])
def test_finalize_routes(mode, n, tiles, c, drop, want_ysum):
    """The three routes of mia_norm_finalize (inline sums; the 1024-thread sum kernel finishing instance norm itself; sum kernel +
    finalize for batch norm) on synthetic ragged partials with per-channel mean = +-1 std, so xb and shift are not trivial: all
    five coefficient rows, and in batch mode the running statistics and the batch counter.  Eval mode passes partials = NULL and
    must ignore the Dropout2d mask.  Bound: 2^-22 (1 + r^2) at r = 1 (derivation: test_finalize_offset_mean; the Dropout2d mask
    only lowers the batch's |mean'| / std', r'^2 = f r^2 / (1 + (1 - f) r^2) for a kept fraction f)."""
    dev = _dev()
    training = mode != "batch_eval"
    check_finalize(n, tiles, c, "instance" if mode == "instance" else "batch", training, bool(drop), bool(want_ysum), 1.0,
                   seed=17 * tiles + c + n, dev=dev)


@pytest.mark.parametrize("r", [0.0, 2.0, 8.0])
@pytest.mark.parametrize("c", [20, 64])
@pytest.mark.parametrize("n,tiles", R.FINALIZE_NT)
@pytest.mark.parametrize("mode", ["instance", "batch"])
def test_finalize_offset_mean(mode, n, tiles, c, r):
    """var = E[y^2] - mean^2 "must not cancel" (csrc/norm.hip): per-channel mean = r std, r in {0, 2, 8}.

    Derived bound, not a tuned one.  The kernel and the reference read the same fp32 partials; the kernel adds them in double and
    rounds the per-(n, c) sums S1, S2 once to fp32 (relative error <= 2^-24 each) before forming the variance in double.  With
    E[y^2] = var (1 + r^2) and mean^2 = var r^2, the rounding of S2 moves the variance by at most 2^-24 (1 + r^2) var and the
    rounding of S1 (squared) by 2^-23 r^2 var: together at most 2^-23 (1 + r^2) var for r <= 1 and 2^-24 (1 + 3 r^2) var beyond.
    rstd = (var + eps)^-1/2 sees half of that: <= 2^-25 (1 + 3 r^2) < 2^-23 (1 + r^2).  xa and xb are cast to fp32 (2^-24) and
    scale = gamma xa, shift = gamma xb + beta are formed in fp32 (another 2^-24 of the row's maximum).  The assertion is
    relerr <= 2^-22 (1 + r^2) on every row: the statistics' share plus room for the final roundings.  The sampled mean / std of
    1153 pixels is within 3 % of r, which moves the bound by less than 0.2 %.  The running variance sees the variance error in
    full, 2^-24 (1 + 3 r^2) + 2^-24 <= 2^-22 (1 + r^2).  Sums ACCUMULATED in fp32 over the tile table (an error that grows with
    the tile count, times 1 + r^2) would miss this at r = 8; each figure is printed as a fraction of the bound before it is
    asserted."""
    dev = _dev()
    check_finalize(n, tiles, c, mode, True, False, True, r, seed=31 * tiles + c + n + int(r), dev=dev)


# ================================================================== c: forward apply
def fwd_inputs(n, hw, c, dt, seed):
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(n, hw, c, generator=g).double() * 1.5 + torch.randn(c, generator=g).double()).to(R.DT[dt]).double()
    scale = (torch.randn(n, c, generator=g) * 0.8).double()
    scale[0, 0] = 0.0  # a dropped channel
    shift = (torch.randn(n, c, generator=g) * 0.5).double()
    return y, scale, shift


def run_fwd(y, scale, shift, dt, dev, slope=R.SLOPE, misalign=False, amax=False):
    mia_hip, ops = _abi()
    _p = ops._p
    n, hw, c = y.shape
    yd = act(y, dt, dev, misalign)
    zd = act(torch.full_like(y, NAN), dt, dev, misalign)
    sc, sf = f32(scale, dev), f32(shift, dev)
    slot = torch.zeros(1, dtype=torch.int32, device=dev) if amax else None
    mia_hip.call("mia_norm_act_fwd", _p(yd), _p(zd), dt_id(dt), _p(sc), _p(sf), n, ops._c_i64(hw), c, ops._c_float(slope), _p(slot),
                 ops._stream())
    torch.cuda.synchronize()
    return zd, slot


@pytest.mark.parametrize("hw", R.FWD_HW)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", R.FWD_CHANNELS)
def test_forward_apply(c, dt, hw):
    """z = lrelu(scale y + shift) with per-(n, c) rows (one scale is an exact 0): the non-vector kernel (C = 7; 12 and 20 in bf16) and the
    stream kernel at 3 units per pixel (C = 12 fp32, 24 bf16) and at unit counts that are no power of two (5, 6, 12, 20, 24, 40), on
    15, 256 and 1961 pixels (fewer pixels than pixel lanes, and a ragged tail behind the four-way unrolled loop)."""
    dev = _dev()
    y, scale, shift = fwd_inputs(2, hw, c, dt, seed=c * 7 + hw)
    z, _ = run_fwd(y, scale, shift, dt, dev)
    ref = R.lrelu(scale.float().double()[:, None] * y + shift.float().double()[:, None], R.SLOPE)
    assert rel(z, ref) < Z_TOL[dt]


@pytest.mark.parametrize("dt,c", [("f32", 32), ("bf16", 96)])
def test_forward_apply_misaligned(dt, c):
    """y and z one element into their buffers: a vector-eligible C must take the scalar kernel and touch nothing outside z."""
    dev = _dev()
    y, scale, shift = fwd_inputs(2, 16 * 16, c, dt, seed=c)
    z, _ = run_fwd(y, scale, shift, dt, dev, misalign=True)
    ref = R.lrelu(scale.float().double()[:, None] * y + shift.float().double()[:, None], R.SLOPE)
    assert rel(z, ref) < Z_TOL[dt]
    flat = z._base  # the buffer the view sits in, NaN wherever the kernel did not write
    assert z.storage_offset() == 1 and bool(torch.isnan(flat[0])) and bool(torch.isnan(flat[1 + z.numel():]).all()), "wrote outside z"


@pytest.mark.parametrize("c,misalign", [(32, False), (160, False), (32, True), (7, False)])
def test_forward_amax_is_the_bit_pattern_of_the_maximum(c, misalign):
    """fp32 with amax_out: the zeroed slot ends as the bit pattern of max |z| exactly -- folded into the stream kernel (C = 32, 160)
    and as a separate pass behind the scalar kernel (misaligned C = 32, C = 7)."""
    dev = _dev()
    y, scale, shift = fwd_inputs(2, 37 * 53, c, "f32", seed=c + 100)
    z, slot = run_fwd(y, scale, shift, "f32", dev, misalign=misalign, amax=True)
    assert slot.item() == z.abs().max().view(torch.int32).item()
    assert slot.item() != 0


# ================================================================== d: backward
def run_bwd(i, co, dt, mode, slabs, dev, *, pieces=1, fixed=0, slope=R.SLOPE, ysum=True, dbias=True, accumulate=0, sums=None,
            misalign=(), entry="mia_norm_act_bwd"):
    """One mia_norm_act_bwd (or mia_norm_bwd_sums) call; every output buffer starts as NaN so an unwritten element shows."""
    mia_hip, ops = _abi()
    _p = ops._p
    n, hw, c = i["y"].shape
    yd = act(i["y"], dt, dev)
    dzd = act(i["dz"], dt, dev, "dz" in misalign)
    dz2d = act(i["dz2"], dt, dev, "dz2" in misalign) if pieces == 2 else None
    dyd = act(torch.full_like(i["y"], NAN), dt, dev, "dy" in misalign)
    part = torch.full((n, slabs, c, 2), NAN, device=dev, dtype=torch.float32)
    cc = torch.full((2, n, c), NAN, device=dev, dtype=torch.float32)
    dgb = torch.full((3, c), NAN, device=dev, dtype=torch.float32) if sums is None else sums
    args = [_p(dzd), _p(dz2d), _p(yd)] + ([_p(dyd)] if entry == "mia_norm_act_bwd" else []) + [
        dt_id(dt), _p(co[2]), _p(co[3]), _p(co[0]), _p(co[1]), _p(co[4]) if ysum else None, n, ops._c_i64(hw), c, mode_id(mode),
        int(fixed), ops._c_float(slope), slabs, _p(part), _p(cc[0]), _p(cc[1]), _p(dgb[0]), _p(dgb[1]), _p(dgb[2]) if dbias else None,
        int(accumulate)] + ([None] if entry == "mia_norm_act_bwd" else []) + [ops._stream()]
    mia_hip.call(entry, *args)
    torch.cuda.synchronize()
    return dict(dy=dyd, c1=cc[0], c2=cc[1], dgamma=dgb[0], dbeta=dgb[1], dbias=dgb[2], part=part)


def check_dy(got_dy, r, dt, what="dy"):
    skip = R.near_zero(r["v"], dt)
    assert skip.double().mean().item() <= R.MAX_EXCLUDED
    got = got_dy.detach().double().cpu()
    assert bool(torch.isfinite(got).all()), "a dy element was never written"
    err = ((got - r["dy"]).abs() * (~skip)).max().item() / r["dy"].abs().max().item()
    assert err < DY_TOL[dt], f"{what}: {err:.3e}"


def check_bwd(got, r, dt, dbias=True):
    check_dy(got["dy"], r, dt)
    assert rel(got["dgamma"], r["dgamma"]) < SUM_TOL and rel(got["dbeta"], r["dbeta"]) < SUM_TOL
    if r["c1"].any():
        assert rel(got["c1"], r["c1"]) < SUM_TOL and rel(got["c2"], r["c2"]) < SUM_TOL
    else:  # frozen statistics: no statistic terms at all
        assert not got["c1"].any() and not got["c2"].any()
    if dbias:
        bound = 1e-3 * r["dy"].abs().sum((0, 1)).max().item() + 1e-4
        assert (got["dbias"].double().cpu() - r["dbias"]).abs().max().item() < bound


@pytest.mark.parametrize("slabs", [1, 3, 7])
@pytest.mark.parametrize("mode", ["instance", "batch"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", R.BWD_CHANNELS)
def test_backward(c, dt, mode, slabs):
    """mia_norm_act_bwd on 3 images of 37 * 53 pixels with Dropout2d masks: every reduction layout (CG = 64 / 96 / 32 / generic), the
    slab sums folded into the finalize launch, stream and scalar apply; the gradient comes in two pieces wherever
    mia_norm_two_piece_ok holds.  Compared: dy, dgamma, dbeta, dbias and the group means c1 / c2.  A wrong lane count, a dropped
    ragged slab or a missed channel group changes the sums by tens of percent."""
    dev = _dev()
    mia_hip, _ = _abi()
    key = R._key(c, dt, mode)
    i, r = R.reference(key)
    pieces = 2 if mia_hip.lib().mia_norm_two_piece_ok(dt_id(dt), c) else 1
    assert (pieces == 2) == (i["dz2"] is not None)
    got = run_bwd(i, rows(r, dev), dt, mode, slabs, dev, pieces=pieces)
    check_bwd(got, r, dt)


@pytest.mark.parametrize("mode", ["instance", "batch"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", R.LONG_SLAB["channels"])
def test_backward_long_slab_sums(c, dt, mode):
    """n * slabs = 3 * 400 > 1024: the slab sums run in norm_bwd_sum_kernel (16 lanes per channel over 400 slabs of 4 pixels)
    instead of inside the finalize launch."""
    dev = _dev()
    key = R._key(c, dt, mode, R.LONG_SLAB["n"], R.LONG_SLAB["hw"])
    i, r = R.reference(key)
    got = run_bwd(i, rows(r, dev), dt, mode, R.LONG_SLAB["slabs"], dev, pieces=2 if i["dz2"] is not None else 1)
    check_bwd(got, r, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", [20, 64])
def test_backward_accumulates(c, dt):
    """accumulate = 1 adds into dgamma / dbeta / dbias: two calls into buffers that start at b0 give b0 + 2 x, where x is the
    accumulate = 0 answer.  Each of the two additions rounds once, so the bound is 2 * 2^-24 (|b0| + 2 |x|) per element."""
    dev = _dev()
    i, r = R.reference(R._key(c, dt, "batch"), 1)
    co = rows(r, dev)
    single = run_bwd(i, co, dt, "batch", 3, dev)
    check_bwd(single, r, dt)
    b0 = torch.randn(3, c, generator=torch.Generator().manual_seed(c)).to(dev)
    acc = b0.clone()
    run_bwd(i, co, dt, "batch", 3, dev, accumulate=1, sums=acc)
    run_bwd(i, co, dt, "batch", 3, dev, accumulate=1, sums=acc)
    x = torch.stack([single["dgamma"], single["dbeta"], single["dbias"]]).double()
    want = b0.double() + 2 * x
    bound = 2.0 ** -23 * (b0.double().abs() + 2 * x.abs())
    assert bool(((acc.double() - want).abs() <= bound).all())
    assert bool(((acc.double() - x).abs() > 0.5 * x.abs()).any()), "the test's own inputs: accumulation must be visible"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", [20, 64])
def test_backward_frozen_statistics(c, dt):
    """fixed_stats = 1 (eval-mode BatchNorm backward), ysum = NULL, running statistics that differ from the batch's own: no
    statistic terms (c1 = c2 = 0), dbias = sum dy = sum scale g."""
    dev = _dev()
    i, r = R.reference(R._key(c, dt, "batch", frozen=True), 1)
    live = R.norm_act(i["y"], i["gamma"], i["beta"], i["dz"], "batch", m=None, running=i["running"])
    assert rel(live["dy"], r["dy"]) > 0.05, "the test's own inputs: batch statistics must give another answer"
    got = run_bwd(i, rows(r, dev), dt, "batch", 3, dev, fixed=1, ysum=False)
    check_bwd(got, r, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", [20, 64])
def test_backward_scale_lrelu_call_shape(c, dt):
    """ScaleLReLUFn's call: xa = scale = m (a Dropout2d mask with exact zeros), xb = shift = 0, instance mode with fixed_stats = 1,
    ysum = NULL, dbias = NULL -> dv = m dz lrelu'(m v).  m v is a product with no addend, so its sign is exact in fp32 and every
    element is compared."""
    dev = _dev()
    i = R.make_inputs(R._key(c, dt, "instance"))
    n = i["y"].shape[0]
    ref = R.scale_lrelu(i["y"], i["m"], i["dz"])
    zero = torch.zeros(n, c, dtype=torch.float64)
    co = torch.stack([i["m"], zero, i["m"], zero, zero]).float().to(dev)
    got = run_bwd(i, co, dt, "instance", 1, dev, fixed=1, ysum=False, dbias=False)
    assert rel(got["dy"], ref["dv"]) < DY_TOL[dt]
    assert not got["dy"].double().cpu()[:, :, i["m"][0] == 0][0].any()
    assert bool(torch.isnan(got["dbias"]).all()), "dbias = NULL: nothing may be written"


@pytest.mark.parametrize("mode", ["instance", "batch"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", [20, 64])
def test_backward_slope_one(c, dt, mode):
    """slope = 1.0 (PointwiseNormFn: a norm without activation): g = dz on both branches, so every element is compared."""
    dev = _dev()
    i = R.make_inputs(R._key(c, dt, mode))
    r = R.norm_act(i["y"], i["gamma"], i["beta"], i["dz"], mode, m=i["m"], slope=1.0, running=i["running"])
    r["v"] = torch.ones_like(r["v"])  # no kink: nothing is skipped
    got = run_bwd(i, rows(r, dev), dt, mode, 3, dev, slope=1.0)
    check_bwd(got, r, dt)


@pytest.mark.parametrize("which", ["dy", "dz"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_backward_misaligned(dt, which):
    """C = 64 with one pointer one element off 16-byte alignment.  dy only: the reduce pass looks at (dz, y) and stays on the vector
    kernel, the apply pass looks at (dz, y, dy) and falls to the scalar kernel.  dz only: scalar reduce and scalar apply.  Same
    answer as the aligned call, nothing written outside dy."""
    dev = _dev()
    i, r = R.reference(R._key(64, dt, "instance"), 1)
    got = run_bwd(i, rows(r, dev), dt, "instance", 3, dev, misalign=(which,))
    check_bwd(got, r, dt)
    if which == "dy":
        dy = got["dy"]
        flat = dy._base
        assert bool(torch.isnan(flat[0])) and bool(torch.isnan(flat[1 + dy.numel():]).all()), "wrote outside dy"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_backward_two_pieces_need_aligned_tensors(dt):
    dev = _dev()
    mia_hip, _ = _abi()
    i, r = R.reference(R._key(64, dt, "instance"))
    with pytest.raises(mia_hip.MiaError, match="two-piece"):
        run_bwd(i, rows(r, dev), dt, "instance", 3, dev, pieces=2, misalign=("dz2",))


# ================================================================== e: reduce-only variant
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c,mode", [(64, "instance"), (96, "batch"), (160, "instance"), (20, "batch")])
def test_backward_sums_only_is_bit_identical(c, mode, dt):
    """mia_norm_bwd_sums (the stem's variant without the apply pass) launches the same reduction and finalize with the same
    arguments as mia_norm_act_bwd: c1, c2, dgamma, dbeta and dbias are bit-identical, one case per reduction layout."""
    dev = _dev()
    i, r = R.reference(R._key(c, dt, mode), 1)
    co = rows(r, dev)
    full = run_bwd(i, co, dt, mode, 7, dev)
    only = run_bwd(i, co, dt, mode, 7, dev, entry="mia_norm_bwd_sums")
    check_bwd(full, r, dt)
    for k in ("part", "c1", "c2", "dgamma", "dbeta", "dbias"):
        assert torch.equal(full[k], only[k]), k


# ================================================================== f: stand-alone statistics
def run_stats(y, dt, slabs, dev, misalign=False):
    mia_hip, ops = _abi()
    n, hw, c = y.shape
    yd = act(y, dt, dev, misalign)
    part = torch.full((n, slabs, c, 2), NAN, device=dev, dtype=torch.float32)
    mia_hip.call("mia_norm_stats", ops._p(yd), dt_id(dt), n, ops._c_i64(hw), c, slabs, ops._p(part), ops._stream())
    torch.cuda.synchronize()
    return yd, part


def check_stats(part, y):
    got = part.double().sum(1).cpu()
    assert rel(got[..., 0], y.sum(1)) < TOL32 and rel(got[..., 1], (y * y).sum(1)) < TOL32


@pytest.mark.parametrize("slabs", [1, 5])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", [20, 32, 96, 160, 256])
def test_stats(c, dt, slabs):
    """mia_norm_stats on 2 x 1961 pixels: the generic kernel (C = 20) and the vector reduction at CG = 32 (C = 32, 160), 96 and 64
    (C = 256), one slab and five (the last one ragged: 4 * 393 + 389).  partials.sum(1) against float64 sums and sums of squares
    of the same quantised y; fp32 accumulation, so the fp32 bound holds for both dtypes.  ops.global_avg_pool is the mean."""
    dev = _dev()
    _, ops = _abi()
    y = R.finalize_inputs(2, c, 1.0, seed=c + slabs, p=R.HW_RAGGED)["y"].to(R.DT[dt]).double()
    yd, part = run_stats(y, dt, slabs, dev)
    check_stats(part, y)
    if slabs == 1:
        pool = ops.global_avg_pool(yd.view(2, 37, 53, c))
        assert rel(pool, y.mean(1)) < TOL32


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_stats_misaligned(dt):
    """A vector-eligible C = 64 whose pointer is one element off: the generic kernel, same sums."""
    dev = _dev()
    y = R.finalize_inputs(2, 64, 1.0, seed=5, p=R.HW_RAGGED)["y"].to(R.DT[dt]).double()
    _, part = run_stats(y, dt, 5, dev, misalign=True)
    check_stats(part, y)


# ================================================================== g: synchronised batch norm, both ranks in one process
@pytest.mark.parametrize("split", R.SYNC_SPLITS)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", R.SYNC_CHANNELS)
def test_sync_batch_norm_in_one_process(c, dt, split):
    """A batch of 4 images (1961 pixels, Dropout2d masks) as two shards of unequal or equal size, the collectives done by hand:
    mia_bn_sync_local_stats per shard -> stack (all-gather) -> mia_norm_finalize_sync per shard -> mia_norm_act_bwd_reduce per
    shard -> add `tot` (all-reduce) -> mia_norm_act_bwd_apply_sync per shard.  Against the restatement's world view (one batch
    holding every shard), and against the one-process mia_norm_finalize + mia_norm_act_bwd on the whole batch.

    Bounds on the coefficient rows and running statistics.  Both routes start from the same fp32 partials and round the per-(n, c)
    sums to fp32; R.coefficients on those partials is the exact answer for them.  The one-process route is within
    2^-22 (1 + r^2) of it (test_finalize_offset_mean).  The sync route additionally sends each shard's (mean, M2) as fp32: the
    combined variance moves by at most 2^-24 (1 + 2 r^2) var (M2 by 2^-24, each squared mean difference by 2^-23), rstd by half
    of that, 2^-25 (1 + 2 r^2) < 2^-22 (1 + r^2): the sync route is held to twice the one-process bound, 2^-21 (1 + r^2), and
    the two routes to the sum, 3 * 2^-22 (1 + r^2) -- with r = 1, a cap: these inputs have |mean| <= 0.3 std and the Dropout2d
    masks only lower it.  The restatement's world view is computed from y itself, not from the fp32 partials (three tiles per
    image, each rounded once), so it is compared at the project's fp32 figure 2e-5 only as a check of the whole chain."""
    dev = _dev()
    mia_hip, ops = _abi()
    _p, cf, ci = ops._p, ops._c_float, ops._c_i64
    key = R._key(c, dt, "batch", 4)
    i, r = R.reference(key)
    hw, tiles, slabs = R.HW_RAGGED, 3, 3
    pieces = 2 if i["dz2"] is not None else 1
    edges = [0, split[0], 4]
    gd, bd = f32(i["gamma"], dev), f32(i["beta"], dev)
    part_all = R.epilogue_partials(i["y"], tiles, seed=c)
    ranks = []
    for a, b in zip(edges[:-1], edges[1:]):  # forward, local statistics
        k = dict(n=b - a, y=act(i["y"][a:b], dt, dev), dz=act(i["dz"][a:b], dt, dev),
                 dz2=act(i["dz2"][a:b], dt, dev) if pieces == 2 else None, drop=f32(i["m"][a:b], dev), part=part_all[a:b].contiguous().to(dev),
                 coefs=torch.full((5, b - a, c), NAN, device=dev), local=torch.full((3, c), NAN, device=dev),
                 rm=f32(i["running"][0], dev), rv=f32(i["running"][1], dev), nbt=torch.zeros((), device=dev, dtype=torch.long))
        mia_hip.call("mia_bn_sync_local_stats", _p(k["part"]), k["n"], tiles, c, ci(hw), _p(k["drop"]), _p(k["coefs"][0]),
                     _p(k["coefs"][1]), _p(k["local"]), ops._stream())
        ranks.append(k)
    gathered = torch.stack([k["local"] for k in ranks]).contiguous()
    assert gathered[:, 2].cpu().tolist() == [[float(k["n"] * hw)] * c for k in ranks]
    for k in ranks:
        co = k["coefs"]
        mia_hip.call("mia_norm_finalize_sync", _p(gathered), 2, k["n"], c, ci(hw), _p(k["drop"]), _p(gd), _p(bd), cf(R.EPS), cf(R.MOM),
                     _p(k["rm"]), _p(k["rv"]), _p(k["nbt"]), _p(co[0]), _p(co[1]), _p(co[2]), _p(co[3]), _p(co[4]), ops._stream())
    for k in ranks:  # backward
        k["slab_part"] = torch.full((k["n"], slabs, c, 2), NAN, device=dev)
        k["cc"] = torch.full((2, k["n"], c), NAN, device=dev)
        k["tot"] = torch.full((3, c), NAN, device=dev)
        co = k["coefs"]
        mia_hip.call("mia_norm_act_bwd_reduce", _p(k["dz"]), _p(k["dz2"]), _p(k["y"]), dt_id(dt), _p(co[2]), _p(co[3]), _p(co[0]), _p(co[1]),
                     k["n"], ci(hw), c, cf(R.SLOPE), slabs, _p(k["slab_part"]), _p(k["cc"][0]), _p(k["cc"][1]), _p(k["tot"]), ops._stream())
    tot = (ranks[0]["tot"] + ranks[1]["tot"]).contiguous()
    for k in ranks:
        k["dy"] = act(torch.full((k["n"], hw, c), NAN, dtype=torch.float64), dt, dev)
        k["dgb"] = torch.full((3, c), NAN, device=dev)
        co = k["coefs"]
        mia_hip.call("mia_norm_act_bwd_apply_sync", _p(k["dz"]), _p(k["dz2"]), _p(k["y"]), _p(k["dy"]), dt_id(dt), _p(co[2]), _p(co[3]),
                     _p(co[0]), _p(co[1]), _p(co[4]), k["n"], ci(hw), c, cf(R.SLOPE), _p(k["cc"][0]), _p(k["cc"][1]), _p(tot),
                     _p(k["dgb"][0]), _p(k["dgb"][1]), _p(k["dgb"][2]), 0, None, ops._stream())
    torch.cuda.synchronize()
    # ---- against the world view
    world = R.norm_act_world([dict(y=i["y"][a:b], dz=i["dz"][a:b], dz2=i["dz2"][a:b] if pieces == 2 else None, m=i["m"][a:b])
                              for a, b in zip(edges[:-1], edges[1:])], i["gamma"], i["beta"], running=i["running"])
    assert torch.equal(world["dy"], r["dy"])
    coefs = torch.cat([k["coefs"] for k in ranks], 1)
    exact = R.coefficients(part_all[..., 0].double().sum(1), part_all[..., 1].double().sum(1), hw, i["gamma"], i["beta"], "batch",
                           i["m"], True, i["running"])
    one_bound = 2.0 ** -22 * (1.0 + 1.0)
    errs = {name: rel(coefs[j], exact[name]) for j, name in enumerate(("xa", "xb", "scale", "shift", "ysum"))}
    errs["running_mean"], errs["running_var"] = rel(ranks[0]["rm"], exact["running"][0]), rel(ranks[0]["rv"], exact["running"][1])
    print(f"sync c={c} {dt} {split}: " + " ".join(f"{k}={v / (2 * one_bound):.3f}" for k, v in errs.items())
          + f" (fractions of the bound {2 * one_bound:.3e})")
    for name, v in errs.items():
        assert v <= 2 * one_bound, f"{name}: {v:.3e}"
    for j, name in enumerate(("xa", "xb", "scale", "shift", "ysum")):
        assert rel(coefs[j], world[name]) < TOL32, name
    for k in ranks:
        assert rel(k["rm"], world["running_mean"]) < TOL32 and rel(k["rv"], world["running_var"]) < TOL32 and k["nbt"].item() == 1
    assert torch.equal(ranks[0]["rm"], ranks[1]["rm"]) and torch.equal(ranks[0]["rv"], ranks[1]["rv"])
    dy = torch.cat([k["dy"] for k in ranks], 0)
    sums = sum(k["dgb"].double() for k in ranks)
    cc = torch.cat([k["cc"] for k in ranks], 1)
    shards = dict(dy=dy, dgamma=sums[0], dbeta=sums[1], dbias=sums[2], c1=cc[0], c2=cc[1])
    check_bwd(shards, world, dt)
    # ---- against one process holding the whole batch
    whole, rm1, rv1, _ = run_finalize(part_all, 4, tiles, c, hw, "batch", True, i["m"], i, True, dev)
    for j in range(5):
        assert rel(coefs[j], whole[j]) <= 3 * one_bound
    assert rel(ranks[0]["rm"], rm1) <= 3 * one_bound and rel(ranks[0]["rv"], rv1) <= 3 * one_bound
    one = run_bwd(i, whole, dt, "batch", slabs, dev, pieces=pieces)
    skip = R.near_zero(r["v"], dt)
    diff = ((dy.double().cpu() - one["dy"].double().cpu()).abs() * (~skip)).max().item() / r["dy"].abs().max().item()
    assert diff < DY_TOL[dt]
    assert rel(sums[0], one["dgamma"]) < SUM_TOL and rel(sums[1], one["dbeta"]) < SUM_TOL
    bound = 1e-3 * r["dy"].abs().sum((0, 1)).max().item() + 1e-4
    assert (sums[2].cpu() - one["dbias"].double().cpu()).abs().max().item() < bound
