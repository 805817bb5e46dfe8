"""GPU checks of the tail of a training step at kernel level: the 1x1 head, the head fused with the last block's norm + LeakyReLU
(csrc/head.hip), the Dice + CE loss (csrc/dice_ce.hip) and the norm backward fed by the head (csrc/norm.hip, mia_norm_act_bwd_head[_w]) against the
float64 restatement in tests/_head_loss_ref.py, called through the C ABI (mia_hip.call / ops._p).  Inputs are seeded and exactly
representable in their storage types on both sides; every output buffer (the gaps of padded layouts included) starts as NaN, the
gaps must still be NaN afterwards and every element a kernel owns finite.

Launch -> template arguments reached -> case (test[parameters]):
  mia_head_fwd
    head_fwd_fast_kernel<T, K1, UPP> ............... all 18: T = float C0 = 16 / 32 / 64, bf16 C0 = 32 / 64 / 128 (UPP = 4 / 8 / 16), K1 = 2, 3, 4
      paired loop once + single-pixel tail ......... test_head_forward[*-2-1961-cl-False] (npix = 3922)
      npix < 2 * LANES (tail only) ................. test_head_forward[f32-64-3-1-15, bf16-32-2-1-15]
      grid capped at 16384, paired loop twice ...... test_head_forward_capped_grid (float, 3, 16; npix = 887^2 > 3 * 16384 * 16)
      padded pixel stride osp = k1 + 1 ............. test_head_forward[f32-32-3-*-pad, bf16-128-4-*-pad]
    head_fwd_kernel<float / bf16_t>
      16-byte branch, idle lanes (3 units) ......... test_head_forward[f32-12-{1,5,8}]
      16-byte branch, two units on some lanes ...... test_head_forward[f32-40-{1,5,8}], 2 units: [bf16-16-{1,5,8}]
      scalar branch (c0 % EPU != 0) ................ test_head_forward[f32-7, bf16-7, bf16-12, bf16-20]
      scalar branch (x misaligned, c0 % EPU == 0) .. test_head_forward[f32-32, f32-12, bf16-64, bf16-16 -True]; c0 % EPU != 0: [f32-7, bf16-20 -True]
      grid capped at 8192 blocks ................... test_head_forward[f32-12-3-2-131406]
      NCHW logits, two-level address (n = 3) ....... test_head_forward[*-nchw] (also what refuses the fast kernel for C0 = 32 / 128)
      padded pixel stride .......................... test_head_forward[f32-12-5-*-pad, bf16-20-2-*-pad]
  mia_head_bwd
    head_bwd_input_fast_kernel / head_bwd_weight_fast_kernel<T, K1, UPP>: all 18, channels-last dl
                                                     test_head_backward[*-cl-None] (61 weight blocks of 65 rows, the last ragged)
      one weight block (npix < 64) ................. test_head_backward[f32-32-3-1-37]
      2048-block cap ............................... test_head_backward[bf16-32-2-2-90300]
    head_bwd_input_vec_kernel / head_bwd_weight_vec_kernel<float / bf16_t>
      the 18 fast shapes with NCHW dl .............. test_head_backward[*-nchw-None]
      3 / 10 / 32 / 63 units (fp32), 2 / 31 (bf16) . test_head_backward[f32-12 | 40 | 128 | 252, bf16-16 | 248; k1 = 1, 3, 5, 8]
    head_bwd_input_kernel / head_bwd_weight_kernel<float / bf16_t> (scalar)
      c0 % EPU != 0 ................................ test_head_backward[f32-7, bf16-7, bf16-12, bf16-20]
      one unit (256 lanes refused by the vec rule) . test_head_backward[f32-4]
      c0 = 256, and two cb passes (44 live) ........ test_head_backward[f32-256, f32-300]; NCHW dl: [f32-300-2-3-1961-nchw]
      misaligned x / misaligned dx ................. test_head_backward[*-x, *-dx]
    dx = NULL, accumulate = 1 (head_bwd_final_kernel) test_head_backward_options[no_dx | accumulate] on the fast, vec and scalar routes
  mia_head_norm_eligible ........................... test_head_norm_eligibility (truth table)
  mia_head_norm_fwd: head_norm_fwd_kernel<T, K1, UPP[, CU]>: all 24 (UPP = 4, 8, 16 and <16, 12>; K1 = 2, 3, 4; both T)
      tail only (hw = 195, one slab) ............... test_head_norm_forward[*-195-cl]
      bulk only (hw = 1024, two slabs of 512) ...... test_head_norm_forward[*-1024-cl]
      bulk 512 + tail, slabs 654 / 654 / 653 ....... test_head_norm_forward[*-1961-cl], NCHW logits: [*-1961-nchw]; slope = 1: [*-1.0]
  mia_head_norm_wgrad: head_norm_wgrad_kernel<...>: the same 24 x sizes x dl layouts
                                                     test_head_norm_wgrad[*]
    head_bwd_final_kernel over n * slabs = 3, 6, 9 partial blocks, accumulate = 0 then 1: every case of test_head_norm_wgrad
  mia_norm_act_bwd_head / mia_norm_act_bwd_head_w (csrc/norm.hip)
    colreduce_head_kernel<T, K1, 64, false> ........ test_head_fed_backward[64 | 128 -*-head]
    colreduce_head_kernel<T, K1, 32, false> ........ test_head_fed_backward[32 | 96 | 160 -*-head], C = 288: test_head_fed_stream_geometry
    colreduce_head_kernel<T, K1, 64, true> + head_w_final_kernel: test_head_fed_backward[64-*-head_w]
      each with K1 = 2, 3, 4 and both T; slabs = 1, 3, 7 (ragged: 2 * 654 + 653, 6 * 281 + 275); dl channels-last and NCHW
    norm_act_bwd_stream_head_kernel<T, K1>
      unit count 2^k ............................... C = 32, 64, 128 fp32 and bf16
      fp32 C = 96 (24 of 32 lanes live), amax NULL (dead lanes return) and non-NULL (dead lanes stay for the publish)
                                                     test_head_fed_stream_geometry[f32-96-False | True]
      fp32 C = 288, gy = 2; bf16 C = 288 (36 / 64) . test_head_fed_stream_geometry[f32-288, bf16-288]
    norm_bwd_sum_kernel (n * slabs = 1200 > 1024) .. test_head_fed_long_slabs[head | head_w]
    norm_bwd_finalize_kernel
      slab partials added inline (n * slabs <= 1024) every test_head_fed_* case but the next
      partials = NULL (sums already in c1 / c2) .... test_head_fed_long_slabs
      mode instance / batch ........................ test_head_fed_backward[*-instance-* | *-batch-*]
      fixed_stats = 1, ysum = NULL ................. test_head_fed_frozen_statistics
      accumulate = 0 / 1 (dgamma, dbeta, dbias) .... test_head_fed_accumulates
    head_w_final_kernel, accumulate_head = 0 / 1 ... test_head_fed_accumulates
    amax_out = bit pattern of max |dy| ............. every fp32 case with K1 != 2, and test_head_fed_stream_geometry
    _w against the two-call route .................. test_head_fed_routes_agree
  mia_dice_ce_fwd / mia_dice_ce_bwd
    dice_ce_fwd_fast_kernel<K1> / dice_ce_bwd_fast_kernel<K1>, K1 = 2, 3, 4
      491 quads, slabs 1 / 3 / 7 (last ragged) ..... test_loss_fast[*-1964-*]
      paired loop three times (1500 quads) ......... test_loss_fast[*-6000-1]
      empty last slab (9 quads on 4 slabs) ......... test_loss_fast[*-36-4]
    dice_ce_fwd_kernel / dice_ce_bwd_kernel (every refusal of the fast route), slabs 1 and 3
                                                     test_loss_generic[hw1961 | nchw | k1_1 | k1_5 | k1_8 | dense | logits_off | labels_off]
    backward only: other dl strides, misaligned dl . test_loss_backward_refusals[nchw_dl | dl_off] (fast forward, generic backward)
    all 16 flag sets, both routes; LF_DENSE ........ test_loss_flags[fast | generic | dense]
    weights, grad_out NULL / device scalar ......... test_loss_weights_and_upstream
    dice_ce_finalize_kernel loops .................. test_loss_finalize_loops[nb * k1 = 320, nb * slabs = 280 on both routes]
    absent / never predicted / single class ........ test_loss_hand_built
    labels k1, -1, 2^32 + 1 ........................ test_loss_bad_labels[fast | generic]

Tolerances (relerr = max |error| / max |reference|, float64): fp32 outputs 2e-5; bf16 dx of the head 1.5 * 2^-8; bf16 dy of the head-fed
backward 2.5 * 2^-8; dgamma, dbeta, c1, c2 1e-3; dbias test_gpu_norm's absolute rule; head dW, db 1e-4; loss scalars absolutely 2e-6;
label counts exact; dlogits of the loss atol 2e-7 and relerr < 2e-5.  The dy comparison skips only elements whose REFERENCE
pre-activation is within rounding of the LeakyReLU kink (at most 1 %, asserted on the CPU by tests/test_head_loss_host.py); the fused
head's forward and weight gradient are continuous in the pre-activation, so nothing is skipped there.

Coefficient rows.  W, b, dl and the fused head's scale / shift are rounded to fp32 when the inputs are made, so both sides consume the
same numbers.  The head-fed cases follow tests/test_gpu_norm.py instead: the restatement derives xa, xb, scale, shift from y in float64
(_norm_ref.norm_act) and the kernels get those rows rounded once to fp32 (test_gpu_norm.rows), a relative difference of 2^-24 per
coefficient -- 300 times below the fp32 bound, and far inside the near-zero band that the dy comparison may skip."""
import pytest
import torch

import _head_loss_ref as R
import _norm_ref as N
import test_gpu_norm as G

pytestmark = pytest.mark.gpu

TOL32, Z_TOL, SUM_TOL = G.TOL32, G.Z_TOL, G.SUM_TOL
HEAD_W_TOL = 1e-4
LOSS_ATOL, DL_ATOL = 2e-6, 2e-7
NAN = float("nan")
_dev, _abi, rel, act, f32, dt_id, mode_id = G._dev, G._abi, G.rel, G.act, G.f32, G.dt_id, G.mode_id
_id = lambda k: "-".join(str(x) for x in k)


class Buf:
    """An fp32 [N, P, K] tensor of logits (or their gradient) in one of the layouts the kernels take, inside a NaN-filled buffer:
    cl [N][P][K], nchw [N][K][P], pad [N][P][K + 1] (one float of gap per pixel); misalign puts it one float into the buffer."""

    def __init__(self, shape, layout, dev, values=None, misalign=False):
        n, p, k = shape
        store = {"cl": (n, p, k), "nchw": (n, k, p), "pad": (n, p, k + 1)}[layout]
        numel = store[0] * store[1] * store[2]
        self.flat = torch.full((numel + 8,), NAN, dtype=torch.float32, device=dev)
        off = 1 if misalign else 0
        st = self.flat[off:off + numel].view(store)
        self.view = {"cl": st, "nchw": st.permute(0, 2, 1), "pad": st[..., :k]}[layout]
        assert tuple(self.view.shape) == (n, p, k) and (self.view.data_ptr() % 16 != 0) == misalign
        if values is not None:
            self.view.copy_(values.float())
        self.sn, self.sp, self.sk = self.view.stride()

    def strides(self, ops):  # in the ABI's order: image, class, pixel
        return ops._c_i64(self.sn), ops._c_i64(self.sk), ops._c_i64(self.sp)

    def check_written(self):
        assert bool(torch.isfinite(self.view).all()), "an element was never written (or is not finite)"
        assert int(torch.isnan(self.flat).sum()) == self.flat.numel() - self.view.numel(), "wrote outside the tensor (a gap or a guard)"


def nan_f32(shape, dev):
    return torch.full(shape, NAN, dtype=torch.float32, device=dev)


def guard_ok(t):
    """t: a G.act view; the buffer around it is still NaN."""
    off = t.storage_offset()
    return bool(torch.isnan(t._base[:off]).all()) and bool(torch.isnan(t._base[off + t.numel():]).all())


# ================================================================== mia_head_fwd
def run_head_fwd(i, dt, layout, misalign, dev):
    mia_hip, ops = _abi()
    n, hw, c0 = i["x"].shape
    k1 = i["w"].shape[0]
    xd = act(i["x"], dt, dev, misalign)
    out = Buf((n, hw, k1), layout, dev)
    wd, bd = f32(i["w"], dev), f32(i["b"], dev)
    mia_hip.call("mia_head_fwd", ops._p(xd), dt_id(dt), ops._p(wd), ops._p(bd), ops._p(out.view), n, ops._c_i64(hw), c0, k1,
                 *out.strides(ops), ops._stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", R.head_fwd_cases(), ids=_id)
def test_head_forward(case):
    """logits = x W^T + b on every route of mia_head_fwd (see the table above).  A wrong lane sum, a dropped tail pixel or a
    16-byte load from a misaligned row changes logits by their own size; the bound is the fp32 figure for both dtypes (the
    products of bf16 inputs are exact in fp32, accumulation is fp32)."""
    dev = _dev()
    dt, c0, k1, n, hw, layout, misalign = case
    i = R.head_inputs(dt, c0, k1, n, hw)
    out = run_head_fwd(i, dt, layout, misalign, dev)
    out.check_written()
    assert rel(out.view, R.head(i["x"], i["w"], i["b"])["logits"]) < TOL32


def test_head_forward_capped_grid():
    """The one large case: fp32 C0 = 64, K1 = 3 on 887 x 887 pixels (201 MB).  16 lanes per block and 16384 blocks cover
    2 * 262144 pixels per paired round, so pixels beyond 524288 are a second round and those beyond 786432 its single-pixel tail.
    Input from a seeded integer grid on the device, the float64 reference evaluated there in chunks."""
    dev = _dev()
    mia_hip, ops = _abi()
    dt, c0, k1, n, hw = R.CAPPED
    small = R.head_inputs(dt, c0, k1, 1, 1)
    x = torch.randint(-24, 25, (n, hw, c0), device=dev, generator=torch.Generator(device=dev).manual_seed(7), dtype=torch.float32) / 8
    out = Buf((n, hw, k1), "cl", dev)
    wd, bd = f32(small["w"], dev), f32(small["b"], dev)
    mia_hip.call("mia_head_fwd", ops._p(x), dt_id(dt), ops._p(wd), ops._p(bd), ops._p(out.view), n, ops._c_i64(hw), c0, k1,
                 *out.strides(ops), ops._stream())
    torch.cuda.synchronize()
    out.check_written()
    w64, b64 = small["w"].to(dev), small["b"].to(dev)
    err = top = 0.0
    for a in range(0, hw, 1 << 16):
        ref = (x[0, a:a + (1 << 16)].double()[:, None, :] * w64[None]).sum(-1) + b64
        err = max(err, (out.view[0, a:a + (1 << 16)].double() - ref).abs().max().item())
        top = max(top, ref.abs().max().item())
    assert err / top < TOL32


# ================================================================== mia_head_bwd
def run_head_bwd(i, dt, layout, mis, dev, want_dx=True, into=None):
    mia_hip, ops = _abi()
    _p = ops._p
    n, hw, c0 = i["x"].shape
    k1 = i["w"].shape[0]
    xd = act(i["x"], dt, dev, mis == "x")
    dl = Buf((n, hw, k1), layout, dev, values=i["dl"])
    dxd = act(torch.full_like(i["x"], NAN), dt, dev, mis == "dx") if want_dx else None
    dw, db = (nan_f32((k1, c0), dev), nan_f32((k1,), dev)) if into is None else into
    ws = nan_f32((mia_hip.lib().mia_head_bwd_workspace(c0, k1),), dev)
    wd = f32(i["w"], dev)
    mia_hip.call("mia_head_bwd", _p(dl.view), _p(xd), dt_id(dt), _p(wd), _p(dxd), _p(dw), _p(db), _p(ws), n, ops._c_i64(hw), c0, k1,
                 *dl.strides(ops), 0 if into is None else 1, ops._stream())
    torch.cuda.synchronize()
    return dxd, dw, db


@pytest.mark.parametrize("case", R.head_bwd_cases(), ids=_id)
def test_head_backward(case):
    """dx = dl W, dW = dl^T x, db = sum dl on every route of mia_head_bwd.  Channels-last dl is what DiceCEFn.backward hands the
    head in training (the fast kernels); NCHW dl takes the vector kernels."""
    dev = _dev()
    dt, c0, k1, n, hw, layout, mis = case
    i = R.head_inputs(dt, c0, k1, n, hw)
    ref = R.head(i["x"], i["w"], i["b"], i["dl"])
    dx, dw, db = run_head_bwd(i, dt, layout, mis, dev)
    assert rel(dx, ref["dx"]) < Z_TOL[dt]
    assert guard_ok(dx), "wrote outside dx"
    assert rel(dw, ref["dw"]) < HEAD_W_TOL and rel(db, ref["db"]) < HEAD_W_TOL


@pytest.mark.parametrize("what", ["no_dx", "accumulate"])
@pytest.mark.parametrize("dt,c0,k1", R.HEAD_OPTION_CASES)
def test_head_backward_options(dt, c0, k1, what):
    """dx = NULL: dW and db are still right.  accumulate = 1: dW and db preloaded with non-zero values end as preload + gradient
    (one more fp32 addition: the 1e-4 bound of dW / db, relative to the sum)."""
    dev = _dev()
    i = R.head_inputs(dt, c0, k1, 2, R.HW)
    ref = R.head(i["x"], i["w"], i["b"], i["dl"])
    if what == "no_dx":
        dx, dw, db = run_head_bwd(i, dt, "cl", None, dev, want_dx=False)
        assert dx is None
        assert rel(dw, ref["dw"]) < HEAD_W_TOL and rel(db, ref["db"]) < HEAD_W_TOL
        return
    g = torch.Generator().manual_seed(c0)
    w0, b0 = 20 * torch.randn(k1, c0, generator=g), 20 * torch.randn(k1, generator=g)
    _, dw, db = run_head_bwd(i, dt, "cl", None, dev, into=(w0.to(dev), b0.to(dev)))
    assert rel(dw, w0.double() + ref["dw"]) < HEAD_W_TOL and rel(db, b0.double() + ref["db"]) < HEAD_W_TOL
    assert rel(dw, ref["dw"]) > 0.05 and rel(dw, w0.double()) > 0.05, "the test's own inputs: both terms must be visible"


# ================================================================== mia_head_norm_eligible / _fwd / _wgrad
def test_head_norm_eligibility():
    _dev()
    mia_hip, ops = _abi()
    lib = mia_hip.lib()
    for dt, epu in (("f32", 4), ("bf16", 8)):
        for c0 in (8, 16, 24, 32, 48, 64, 96, 128, 160):
            for k1 in range(1, 6):
                for n in (3, 2048, 2049):
                    upp = c0 // epu
                    want = upp if (c0 % epu == 0 and upp in (4, 8, 12, 16) and 2 <= k1 <= 4 and n <= 2048) else 0
                    assert lib.mia_head_norm_eligible(dt_id(dt), n, ops._c_i64(R.HW), c0, k1) == want, (dt, c0, k1, n)
    assert lib.mia_head_norm_eligible(2, 3, ops._c_i64(R.HW), 32, 3) == 0, "an unknown dtype"
    assert lib.mia_head_norm_eligible(dt_id("f32"), 3, ops._c_i64(2 ** 31), 32, 3) == 0, "hw does not fit the kernels' int"


@pytest.mark.parametrize("case", R.fused_cases(), ids=_id)
def test_head_norm_forward(case):
    """logits = W lrelu(scale y + shift) + b with per-(n, c) rows (one scale exactly 0): every instantiation, the bulk rounds
    (wave-private transpose) and the per-pixel tail, both logits layouts.  The LeakyReLU is continuous: every element compared."""
    dev = _dev()
    mia_hip, ops = _abi()
    dt, c0, k1, n, hw, layout, slope = case
    i = R.fused_inputs(dt, c0, k1, n, hw)
    yd = act(i["y"], dt, dev)
    out = Buf((n, hw, k1), layout, dev)
    sc, sf, wd, bd = f32(i["scale"], dev), f32(i["shift"], dev), f32(i["w"], dev), f32(i["b"], dev)
    mia_hip.call("mia_head_norm_fwd", ops._p(yd), dt_id(dt), ops._p(sc), ops._p(sf), ops._c_float(slope), ops._p(wd), ops._p(bd),
                 ops._p(out.view), n, ops._c_i64(hw), c0, k1, *out.strides(ops), ops._stream())
    torch.cuda.synchronize()
    out.check_written()
    assert rel(out.view, R.head_norm(i["y"], i["scale"], i["shift"], slope, i["w"], i["b"])["logits"]) < TOL32


def run_head_norm_wgrad(i, dt, layout, slope, dev, into=None):
    mia_hip, ops = _abi()
    _p = ops._p
    n, hw, c0 = i["y"].shape
    k1 = i["w"].shape[0]
    yd = act(i["y"], dt, dev)
    dl = Buf((n, hw, k1), layout, dev, values=i["dl"])
    sc, sf = f32(i["scale"], dev), f32(i["shift"], dev)
    dw, db = (nan_f32((k1, c0), dev), nan_f32((k1,), dev)) if into is None else into
    ws = nan_f32((mia_hip.lib().mia_head_bwd_workspace(c0, k1),), dev)
    mia_hip.call("mia_head_norm_wgrad", _p(dl.view), _p(yd), dt_id(dt), _p(sc), _p(sf), ops._c_float(slope), _p(dw), _p(db), _p(ws),
                 n, ops._c_i64(hw), c0, k1, *dl.strides(ops), 0 if into is None else 1, ops._stream())
    torch.cuda.synchronize()
    return dw, db


@pytest.mark.parametrize("case", R.fused_cases(), ids=_id)
def test_head_norm_wgrad(case):
    """dW = dl^T lrelu(scale y + shift), db = sum dl: accumulate = 0 into NaN buffers, then accumulate = 1 into preloaded ones."""
    dev = _dev()
    dt, c0, k1, n, hw, layout, slope = case
    i = R.fused_inputs(dt, c0, k1, n, hw)
    ref = R.head_norm(i["y"], i["scale"], i["shift"], slope, i["w"], i["b"], i["dl"])
    dw, db = run_head_norm_wgrad(i, dt, layout, slope, dev)
    assert rel(dw, ref["dw"]) < HEAD_W_TOL and rel(db, ref["db"]) < HEAD_W_TOL
    g = torch.Generator().manual_seed(c0 + k1)
    w0, b0 = 20 * torch.randn(k1, c0, generator=g), 20 * torch.randn(k1, generator=g)
    dw, db = run_head_norm_wgrad(i, dt, layout, slope, dev, into=(w0.to(dev), b0.to(dev)))
    assert rel(dw, w0.double() + ref["dw"]) < HEAD_W_TOL and rel(db, b0.double() + ref["db"]) < HEAD_W_TOL
    assert rel(dw, w0.double()) > 0.05, "the test's own inputs: the gradient must be visible next to the preload"


# ================================================================== mia_norm_act_bwd_head / _head_w
def run_fed(i, r, dt, mode, slabs, dev, entry="head", layout="cl", fixed=0, amax=False, into=None, head_into=None):
    """One mia_norm_act_bwd_head (entry "head") or mia_norm_act_bwd_head_w ("head_w") call; into = (dgb [3, C]) and head_into =
    (dW, db) switch accumulate / accumulate_head on."""
    mia_hip, ops = _abi()
    _p = ops._p
    n, hw, c = i["y"].shape
    k1 = i["w"].shape[0]
    co = G.rows(r, dev)
    yd = act(i["y"], dt, dev)
    dyd = act(torch.full_like(i["y"], NAN), dt, dev)
    dl = Buf((n, hw, k1), layout, dev, values=i["dl"])
    wd = f32(i["w"], dev)
    part, cc = nan_f32((n, slabs, c, 2), dev), nan_f32((2, n, c), dev)
    dgb = nan_f32((3, c), dev) if into is None else into
    slot = torch.zeros(1, dtype=torch.int32, device=dev) if amax else None
    args = [_p(dl.view), _p(wd), k1, *dl.strides(ops), _p(yd), _p(dyd), dt_id(dt), _p(co[2]), _p(co[3]), _p(co[0]), _p(co[1]),
            None if fixed else _p(co[4]), n, ops._c_i64(hw), c, mode_id(mode), int(fixed), ops._c_float(N.SLOPE), slabs, _p(part), _p(cc[0]),
            _p(cc[1]), _p(dgb[0]), _p(dgb[1]), _p(dgb[2]), 0 if into is None else 1]
    got = dict(dy=dyd, c1=cc[0], c2=cc[1], dgamma=dgb[0], dbeta=dgb[1], dbias=dgb[2], part=part, slot=slot)
    if entry == "head_w":
        ws = nan_f32((n * slabs * k1 * (c + 1),), dev)
        dw, db = (nan_f32((k1, c), dev), nan_f32((k1,), dev)) if head_into is None else head_into
        args += [_p(ws), _p(dw), _p(db), 0 if head_into is None else 1]
        got.update(dw=dw, db=db)
    mia_hip.call("mia_norm_act_bwd_head" if entry == "head" else "mia_norm_act_bwd_head_w", *args, _p(slot), ops._stream())
    torch.cuda.synchronize()
    return got


def check_fed(got, r, dt):
    G.check_bwd(got, r, dt)
    assert guard_ok(got["dy"]), "wrote outside dy"
    assert bool(torch.isfinite(got["part"]).all()), "a slab partial was never written"
    if "dw" in got:
        assert rel(got["dw"], r["dw"]) < HEAD_W_TOL and rel(got["db"], r["db"]) < HEAD_W_TOL
    if got["slot"] is not None:
        assert dt == "f32"
        assert got["slot"].item() == got["dy"].abs().max().view(torch.int32).item() and got["slot"].item() != 0


def _fed_grid():
    out = []
    for key in R.fed_cases():
        c, dt, mode, k1, n, hw, frozen = key
        if frozen or hw != R.HW or c == 288:
            continue
        entries = ("head", "head_w") if c == 64 else ("head",)
        for entry in entries:
            out.append((key, 3, "cl", entry))
            if k1 == 3 and mode == "instance":
                out += [(key, 1, "cl", entry), (key, 7, "nchw", entry)]
    return out


@pytest.mark.parametrize("key,slabs,layout,entry", _fed_grid(), ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_head_fed_backward(key, slabs, layout, entry):
    """The norm backward with dz = dl W recomputed, on 3 images of 1961 pixels with Dropout2d masks: the reduce kernel at CG = 64
    and 32 (and, with the head's dW / db riding along, HWG), K1 = 2, 3, 4, both dtypes, instance and batch statistics, one, three
    and seven slabs, dl channels-last and NCHW.  Compared: dy, dgamma, dbeta, dbias, c1, c2, for _w the head's dW and db, and
    for fp32 with K1 != 2 the amax slot."""
    dev = _dev()
    c, dt, mode, k1, n, hw, frozen = key
    i, r = R.fed_reference(key)
    got = run_fed(i, r, dt, mode, slabs, dev, entry=entry, layout=layout, amax=(dt == "f32" and k1 != 2))
    check_fed(got, r, dt)


@pytest.mark.parametrize("amax", [False, True])
@pytest.mark.parametrize("dt,c", [("f32", 96), ("f32", 288), ("bf16", 288)])
def test_head_fed_stream_geometry(dt, c, amax):
    """The stream kernel with dead lanes: fp32 C = 96 is 24 units on blocks of 32 (dead lanes return early without an amax slot and
    stay for the block-wide publish with one), fp32 C = 288 is 72 units on two block columns of 64, bf16 C = 288 is 36 of 64."""
    dev = _dev()
    key = R.fed_key(c, dt, "instance", 3)
    i, r = R.fed_reference(key)
    got = run_fed(i, r, dt, "instance", 3, dev, amax=amax and dt == "f32")
    check_fed(got, r, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_head_fed_frozen_statistics(dt):
    """fixed_stats = 1 (eval-mode BatchNorm backward), ysum = NULL: no statistic terms, c1 = c2 = 0."""
    dev = _dev()
    i, r = R.fed_reference(R.fed_key(64, dt, "batch", 3, frozen=True))
    assert not r["c1"].any()
    for entry in ("head", "head_w"):
        check_fed(run_fed(i, r, dt, "batch", 3, dev, entry=entry, fixed=1), r, dt)


@pytest.mark.parametrize("entry", ["head", "head_w"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_head_fed_long_slabs(dt, entry):
    """n * slabs = 3 * 400 > 1024: the slab sums run in norm_bwd_sum_kernel; for _w, 1200 partial blocks in head_w_final_kernel."""
    dev = _dev()
    L = R.LONG_SLAB
    i, r = R.fed_reference(R.fed_key(64, dt, "instance", 3, L["n"], L["hw"]))
    check_fed(run_fed(i, r, dt, "instance", L["slabs"], dev, entry=entry, amax=dt == "f32"), r, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_head_fed_accumulates(dt):
    """accumulate = 1 adds into dgamma / dbeta / dbias and accumulate_head = 1 into the head's dW / db, independently: bound
    2^-23 (|b0| + |x|) per element against the accumulate = 0 answer x of the same kernels (one more rounded addition)."""
    dev = _dev()
    i, r = R.fed_reference(R.fed_key(64, dt, "batch", 3))
    single = run_fed(i, r, dt, "batch", 3, dev, entry="head_w")
    check_fed(single, r, dt)
    g = torch.Generator().manual_seed(64)
    b0, w0, hb0 = torch.randn(3, 64, generator=g).to(dev), 20 * torch.randn(3, 64, generator=g).to(dev), 20 * torch.randn(3, generator=g).to(dev)
    x = torch.stack([single["dgamma"], single["dbeta"], single["dbias"]]).double()
    for acc, acc_head in ((1, 0), (0, 1), (1, 1)):
        got = run_fed(i, r, dt, "batch", 3, dev, entry="head_w", into=b0.clone() if acc else None,
                      head_into=(w0.clone(), hb0.clone()) if acc_head else None)
        sums = torch.stack([got["dgamma"], got["dbeta"], got["dbias"]]).double()
        for have, base, add in ((sums, b0 if acc else None, x), (got["dw"].double(), w0 if acc_head else None, single["dw"].double()),
                                (got["db"].double(), hb0 if acc_head else None, single["db"].double())):
            if base is None:
                assert torch.equal(have, add)
            else:
                assert bool(((have - (base.double() + add)).abs() <= 2.0 ** -23 * (base.double().abs() + add.abs())).all())
                assert bool(((have - add).abs() > 0.5 * add.abs()).any()), "the test's own inputs: accumulation must be visible"
        assert torch.equal(got["dy"], single["dy"])


@pytest.mark.parametrize("k1", [2, 3, 4])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_head_fed_routes_agree(dt, k1):
    """mia_norm_act_bwd_head_w against mia_norm_act_bwd_head + mia_head_norm_wgrad on C = 64: dy, the slab partials, c1, c2, dgamma,
    dbeta and dbias bit for bit (the same arithmetic in the same order).  So are the head's dW / db at this size: with n = 3 and
    1961 pixels mia_head_norm_wgrad picks three slabs of ceil(1961 / 3) pixels too, both kernels deal the pixels to the same 16
    (fp32) or 32 (bf16) lanes in the same four-way unrolled order, form x = lrelu(scale y + shift) and acc += dl x alike, add the
    lanes through LDS in the same order and finish in final kernels of the same text over n * slabs = 9 partial blocks."""
    dev = _dev()
    i, r = R.fed_reference(R.fed_key(64, dt, "instance", k1))
    one = run_fed(i, r, dt, "instance", 3, dev, entry="head_w", amax=dt == "f32")
    two = run_fed(i, r, dt, "instance", 3, dev, entry="head", amax=dt == "f32")
    for k in ("dy", "part", "c1", "c2", "dgamma", "dbeta", "dbias"):
        assert torch.equal(one[k], two[k]), k
    if dt == "f32":
        assert torch.equal(one["slot"], two["slot"])
    fi = dict(y=i["y"], scale=r["scale"], shift=r["shift"], w=i["w"], dl=i["dl"])
    dw, db = run_head_norm_wgrad(fi, dt, "cl", N.SLOPE, dev)
    assert torch.equal(one["dw"], dw) and torch.equal(one["db"], db)
    assert rel(dw, r["dw"]) < HEAD_W_TOL and rel(db, r["db"]) < HEAD_W_TOL


# ================================================================== mia_dice_ce_fwd / mia_dice_ce_bwd
DEFAULT_FLAGS = (True, True, False, False)


def flag_bits(flags, dense=False):
    mia_hip, _ = _abi()
    s, d, b, q = flags
    return ((mia_hip.LOSS_SOFTMAX if s else 0) | (mia_hip.LOSS_DO_BG if d else 0) | (mia_hip.LOSS_BATCH if b else 0)
            | (mia_hip.LOSS_SQUARED if q else 0) | (mia_hip.LOSS_DENSE if dense else 0))


def place_labels(labels, dev, misalign=False):
    flat = torch.full((labels.numel() + 3,), -7, dtype=torch.int64, device=dev)
    off = 1 if misalign else 0
    v = flat[off:off + labels.numel()].view(labels.shape)
    v.copy_(labels)
    assert (v.data_ptr() % 16 != 0) == misalign
    return v


def run_loss(logits, target, dev, *, slabs=1, flags=DEFAULT_FLAGS, layout="cl", dl_layout=None, weights=(0.6, 0.9), gout=None,
             off=(), bad=None, backward=True):
    """mia_dice_ce_fwd, then mia_dice_ce_bwd.  target: int64 labels [B, P] or a dense [B, P, K] target (stored [B][K][P], fp32).
    off: which of "logits", "labels", "dl" sit one element into their buffers.  bad: the int32[2] label flags to reuse."""
    mia_hip, ops = _abi()
    _p, cf, ci = ops._p, ops._c_float, ops._c_i64
    nb, hw, k1 = logits.shape
    assert (nb, hw, k1) in R.LOSS_SHAPES, "a loss test may only use shapes of the shared (size-checked) table"
    dense = target.dtype.is_floating_point
    lg = Buf((nb, hw, k1), layout, dev, values=logits, misalign="logits" in off)
    tg = target.permute(0, 2, 1).float().contiguous().to(dev) if dense else place_labels(target, dev, "labels" in off)
    bits = flag_bits(flags, dense)
    ws = nan_f32((mia_hip.lib().mia_dice_ce_workspace(nb, k1, slabs),), dev)
    sums, coef, out = nan_f32((nb, k1, 3), dev), nan_f32((nb, k1, 2), dev), nan_f32((3,), dev)
    bad = torch.zeros(2, dtype=torch.int32, device=dev) if bad is None else bad
    mia_hip.call("mia_dice_ce_fwd", _p(lg.view), _p(tg), nb, ci(hw), k1, *lg.strides(ops), bits, cf(R.SMOOTH), cf(weights[0]), cf(weights[1]),
                 slabs, _p(ws), _p(sums), _p(coef), _p(out), _p(bad), ops._stream())
    got = dict(sums=sums, coef=coef, out=out, bad=bad, dl=None)
    if backward:
        dl = Buf((nb, hw, k1), dl_layout or layout, dev, misalign="dl" in off)
        gd = None if gout is None else torch.tensor([gout], dtype=torch.float32, device=dev)
        mia_hip.call("mia_dice_ce_bwd", _p(lg.view), _p(tg), _p(coef), _p(gd), _p(dl.view), nb, ci(hw), k1, *lg.strides(ops), *dl.strides(ops),
                     bits, cf(weights[0]), cf(weights[1]), ops._stream())
        got["dl"] = dl
    torch.cuda.synchronize()
    return got


def reference_loss(logits, target, flags=DEFAULT_FLAGS, weights=(0.6, 0.9), gout=None):
    w0, w1 = (float(torch.tensor(w, dtype=torch.float32)) for w in weights)  # the kernels take the weights as C floats
    return R.dice_ce(logits, target, *flags, dice_w=w0, ce_w=w1, gout=1.0 if gout is None else gout)


def check_loss(got, ref, index_labels, what=""):
    """out absolutely within 2e-6; sums and coef per column within 2e-5 (label counts exact, the background's coef exactly 0 when
    it is left out); dlogits elementwise within 2e-7 AND relerr < 2e-5.  Each figure is printed before it is asserted."""
    out_err = (got["out"].double().cpu() - ref["out"]).abs().max().item()
    figs = {"out": out_err}
    for j, name in enumerate(("I", "S", "T")):
        figs[name] = rel(got["sums"][..., j], ref["sums"][..., j])
    for j, name in enumerate(("alpha", "beta")):
        figs[name] = rel(got["coef"][..., j], ref["coef"][..., j])
    dl = got["dl"]
    if dl is not None:
        dl.check_written()
        d = (dl.view.double().cpu() - ref["dlogits"]).abs().max().item()
        top = ref["dlogits"].abs().max().item()
        figs["dl_abs"], figs["dl_rel"] = d, (d / top if top > 0 else 0.0)
        if top == 0:  # one class: softmax = 1 = t, every term of the gradient cancels exactly; relerr says nothing, so ask for zeros
            assert not dl.view.any(), "the gradient of a one-class loss is exactly 0"
    print(f"loss {what}: " + " ".join(f"{k}={v:.3e}" for k, v in figs.items()))
    assert bool(torch.isfinite(got["out"]).all()) and figs["out"] < LOSS_ATOL
    assert figs["I"] < TOL32 and figs["S"] < TOL32 and figs["alpha"] < TOL32 and figs["beta"] < TOL32
    if index_labels:
        assert torch.equal(got["sums"][..., 2].double().cpu(), ref["sums"][..., 2]), "label counts are integers"
    else:
        assert figs["T"] < TOL32
    zero = ref["coef"] == 0
    assert not got["coef"].cpu()[zero].any()
    if dl is not None:
        assert figs["dl_abs"] <= DL_ATOL and figs["dl_rel"] < TOL32
    assert got["bad"].tolist() == [0, 0]


@pytest.mark.parametrize("hw,slabs", R.LOSS_FAST_HW)
@pytest.mark.parametrize("k1", [2, 3, 4])
def test_loss_fast(k1, hw, slabs):
    """Channels-last logits on the four-pixels-per-thread kernels: the slab partition of the forward (per = ceil(quads / slabs), a
    ragged or an empty last slab) at sizes far below the 8192 pixels per slab of training, and three rounds of the paired loop."""
    dev = _dev()
    logits, labels = R.loss_inputs(3, hw, k1)
    got = run_loss(logits, labels, dev, slabs=slabs)
    check_loss(got, reference_loss(logits, labels), True, f"fast k1={k1} hw={hw} slabs={slabs}")


GENERIC_WHY = ("hw1961", "nchw", "k1_1", "k1_5", "k1_8", "dense", "logits_off", "labels_off")


@pytest.mark.parametrize("slabs", [1, 3])
@pytest.mark.parametrize("why", GENERIC_WHY)
def test_loss_generic(why, slabs):
    """Every reason for which dice_ce_fast_ok refuses a call: the generic kernels, on one slab and on three (the last ragged)."""
    dev = _dev()
    k1 = int(why[3:]) if why.startswith("k1_") else 3
    hw = 1961 if why == "hw1961" else 1964
    logits, target = R.loss_inputs(3, hw, k1, dense=why == "dense")
    got = run_loss(logits, target, dev, slabs=slabs, layout="nchw" if why == "nchw" else "cl",
                   off=("logits", "dl") if why == "logits_off" else ("labels",) if why == "labels_off" else ())
    check_loss(got, reference_loss(logits, target), why != "dense", f"generic {why} slabs={slabs}")


@pytest.mark.parametrize("why", ["nchw_dl", "dl_off"])
def test_loss_backward_refusals(why):
    """The forward takes the fast kernel, the backward must not: dl with other strides than the logits, or misaligned."""
    dev = _dev()
    logits, labels = R.loss_inputs(3, 1964, 3)
    got = run_loss(logits, labels, dev, slabs=3, dl_layout="nchw" if why == "nchw_dl" else "cl", off=("dl",) if why == "dl_off" else (),
                   gout=R.LOSS_GOUT)
    check_loss(got, reference_loss(logits, labels, gout=R.LOSS_GOUT), True, why)


@pytest.mark.parametrize("flags", R.LOSS_FLAGS, ids=lambda f: "".join("SDBQ"[j] if v else "-" for j, v in enumerate(f)))
@pytest.mark.parametrize("route", ["fast", "generic", "dense"])
def test_loss_flags(route, flags):
    """All 16 sets of softmax / do_bg / batch / squared on 3 x 144 pixels, two slabs: the fast kernels, the generic ones (NCHW logits)
    and the generic ones with a dense target.  Softmax off: the inputs are probabilities in (0, 1), as that flag expects."""
    dev = _dev()
    logits, target = R.loss_inputs(3, 144, 3, softmax=flags[0], dense=route == "dense")
    got = run_loss(logits, target, dev, slabs=2, flags=flags, layout="cl" if route == "fast" else "nchw", gout=R.LOSS_GOUT)
    check_loss(got, reference_loss(logits, target, flags, gout=R.LOSS_GOUT), route != "dense", f"{route} {flags}")


@pytest.mark.parametrize("gout", [None, R.LOSS_GOUT])
@pytest.mark.parametrize("weights", R.LOSS_WEIGHTS, ids=_id)
@pytest.mark.parametrize("route", ["fast", "generic"])
def test_loss_weights_and_upstream(route, weights, gout):
    """(dice_w, ce_w) = (0.6, 0.9), Dice alone, CE alone; grad_out NULL (1) and a device scalar that is neither 0 nor 1."""
    dev = _dev()
    logits, labels = R.loss_inputs(3, 1964, 4, seed=2)
    got = run_loss(logits, labels, dev, slabs=3, flags=(True, False, False, False), layout="cl" if route == "fast" else "nchw",
                   weights=weights, gout=gout)
    check_loss(got, reference_loss(logits, labels, (True, False, False, False), weights, gout), True, f"{route} {weights} gout={gout}")


@pytest.mark.parametrize("nb,k1,slabs", [(40, 8, 7), (70, 4, 4)])
@pytest.mark.parametrize("batch", [False, True])
def test_loss_finalize_loops(nb, k1, slabs, batch):
    """The single-block finalize with more (image, class) pairs than threads (nb * k1 = 320, 280) and more slab partials than
    threads (nb * slabs = 280): K1 = 8 on the generic route, K1 = 4 on the fast one, 16 pixels per image (slabs beyond the data
    are empty)."""
    dev = _dev()
    logits, labels = R.loss_inputs(nb, 16, k1)
    flags = (True, True, batch, False)
    got = run_loss(logits, labels, dev, slabs=slabs, flags=flags)
    check_loss(got, reference_loss(logits, labels, flags), True, f"finalize nb={nb} k1={k1} slabs={slabs} batch={batch}")


@pytest.mark.parametrize("route", ["fast", "generic"])
@pytest.mark.parametrize("do_bg", [False, True])
@pytest.mark.parametrize("special", ["absent", "unpredicted", "one_class"])
def test_loss_hand_built(special, do_bg, route):
    """A class absent from one image's labels (T = 0, I = 0: the smooth term alone), a class that is never the arg-max, an image of
    a single class."""
    dev = _dev()
    logits, labels = R.loss_inputs(3, 1964, 3, special=special)
    flags = (True, do_bg, False, False)
    got = run_loss(logits, labels, dev, slabs=3, flags=flags, layout="cl" if route == "fast" else "nchw")
    check_loss(got, reference_loss(logits, labels, flags), True, f"{route} {special} do_bg={do_bg}")


@pytest.mark.parametrize("flags", [DEFAULT_FLAGS, (False, False, False, True)], ids=["softmax", "plain_squared"])
@pytest.mark.parametrize("which", R.BAD_LABELS, ids=str)
@pytest.mark.parametrize("route", ["fast", "generic"])
def test_loss_bad_labels(route, which, flags):
    """One label equal to k1, negative, or with its high word set over a valid low word (what the fast kernels' `hi[j] == 0u` test is
    for): out and coef all NaN, the working flag re-armed and the sticky verdict set, no finite gradient anywhere.  A clean call
    afterwards on the same flags returns the correct finite loss and leaves the verdict standing."""
    dev = _dev()
    k1 = 3
    logits, labels = R.loss_inputs(3, 1964, k1, softmax=flags[0])
    layout = "cl" if route == "fast" else "nchw"
    got = run_loss(logits, R.bad_labels(labels, k1, which), dev, slabs=3, flags=flags, layout=layout)
    assert bool(torch.isnan(got["out"]).all()) and bool(torch.isnan(got["coef"]).all())
    assert got["bad"].tolist() == [0, 1]
    dl = got["dl"]
    assert not bool(torch.isfinite(dl.view).any()), "a finite gradient after a bad label"
    assert bool(torch.isnan(dl.flat[dl.view.numel():]).all()), "wrote outside dlogits"
    clean = run_loss(logits, labels, dev, slabs=3, flags=flags, layout=layout, bad=got["bad"])
    assert clean["bad"].tolist() == [0, 1], "the verdict is sticky"
    clean["bad"] = torch.zeros(2, dtype=torch.int32)
    check_loss(clean, reference_loss(logits, labels, flags), True, f"clean after bad {route} {which}")
