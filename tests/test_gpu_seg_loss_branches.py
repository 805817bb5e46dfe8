"""GPU checks of every dispatch branch of the fold-trainer losses (csrc/seg_loss.hip) against the float64 restatement in
tests/_seg_loss_ref.py, called through the C ABI (mia_seg_loss_fwd / bwd, mia_topk_ce_fwd / bwd) with a chosen `slabs`.  Inputs are
seeded and exactly representable in fp32.  Every buffer a kernel writes starts as NaN (floats) or a sentinel (counts, the logits
gradient); afterwards every word the kernels own must have been written -- all 5 k1 + 2 words of every workspace slice, the doubles
behind them, every coef entry, every count, every gradient element -- and every word they do not own must still hold its fill.
Which route a call takes cannot be observed from outside; each case asserts on its own pointers and strides, with `expect_fast`
(a restatement of sl_fast_ok and of the backward's extra condition), that it takes the route it is listed under.

Launch -> branch -> case (test[parameters]):
  mia_seg_loss_fwd
    seg_loss_fwd_fast_kernel<K1, LT>, two-in-flight loop `q + 256 < q1; q += 512` and its single tail step, by quads per slab
      <2,int64> quads 1 (tail on one lane), 769 (pair twice on lane 0, pair + tail elsewhere) test_seg_fast_quads[1 | 769]
      <3,uint8> 255 (tail only, one idle lane), ragged 4 + 4 + 2 .......... test_seg_fast_quads[255 | ragged]
      <4,int64> 256 (tail only, every lane), 9 quads on 4 slabs (one empty) test_seg_fast_quads[256 | empty]
      <2,uint8> 257 (pair on lane 0, tail elsewhere) ...................... test_seg_fast_quads[257]
      <3,int64> 512 (pair on every lane, no tail) ......................... test_seg_fast_quads[512]
      <4,uint8> 513 (pair, then a tail on lane 0) ......................... test_seg_fast_quads[513]
      <4,uint8>, <3,int64>, <2,uint8> at three slabs ....................... test_seg_fast_refusals[fast-*], test_seg_grad_out[fast-*]
      <2,uint8> 64 slabs of 2056 quads (pair loop four times) ............. test_wrap_seg_backward_fast
    seg_loss_fwd_kernel<LT> (SlAcc<8>, sl_block_store<8>: 2 k1 + 2 float and 3 k1 int slots)
      k1 = 1 .. 8, both LT, 1 / 3 / 7 slabs on hw = 1, 7, 195, 1964 ........ test_seg_generic_shapes[hw-slabs-k1]
      more slabs than pixels (3 pixels, 5 slabs) .......................... test_seg_generic_shapes[3-5-5]
      each refusal of sl_fast_ok, hw % 4 == 0, three slabs:
        sk != 1 (NCHW) ..................................................... test_seg_fast_refusals[nchw]
        logits 4 bytes off a 16-byte boundary ............................. test_seg_fast_refusals[x_off4]
        uint8 labels 1 byte off / int64 labels 8 bytes off ................ test_seg_fast_refusals[u8_off1 | i64_off8]
        sn > hw k1 (an image-sliced view) ................................. test_seg_fast_refusals[sliced]
        k1 = 5 channels-last .............................................. test_seg_fast_refusals[k1=5]
        hw % 4 != 0 channels-last, k1 = 3 ................................. test_seg_generic_shapes[1-7-3]
    seg_loss_finalize_kernel
      per-image and batch Dice, do_bg on / off, k1 = 1 .. 8 ............... rotating through test_seg_generic_shapes / test_seg_fast_quads
      nb k1 = 320 > 256 and nb slabs = 280 > 256 (both loops go round twice) test_seg_finalize_loops[image | batch]
      nothing valid (CEden = 0) / one image without a valid pixel ......... test_seg_all_ignored[batch | image]
      bad label: NaN out and coef, sticky verdict ......................... test_label_decoding[*-2^32+1 | *-255 | *-lowword]
  mia_seg_loss_bwd
    seg_loss_bwd_fast_kernel<K1, LT>: all six .............................. test_seg_fast_quads[*] (the pairs listed above)
      grad_out NULL / 1 / -0.375 / 3.0 .................................... NULL: every other case; test_seg_grad_out[fast-*]
      grid.x capped at 512 blocks of 256 quads, the loop goes round twice . test_wrap_seg_backward_fast
    seg_loss_bwd_kernel<LT> (sl_pixel_bwd<8>)
      k1 = 1 .. 8 ........................................................... test_seg_generic_shapes[*]
      the backward's extra condition: dlogits NCHW for channels-last logits test_seg_fast_refusals[dl_nchw]
                                      dlogits 4 bytes off .................. test_seg_fast_refusals[dl_off4]
      grad_out 1 / -0.375 / 3.0 ............................................ test_seg_grad_out[generic-*]
      grid capped at 8192 blocks, the loop goes round twice ............... test_wrap_seg_backward_generic
  sl_class / sl_quad_classes (label decoding)
    int64 2^32 + 1 is a bad label (not class 1) ............................ test_label_decoding[fast | generic | topk -2^32+1]
    ignore -100: ignored as int64, never matches a uint8 label ............ test_label_decoding[*-int64-ignore-100 | *-uint8-ignore-100]
    uint8 255 with ignore -100 is a bad label ............................. test_label_decoding[*-255]
    int64 2^32 - 100 (the ignore label's low word alone) is a bad label ... test_label_decoding[*-lowword]
  mia_topk_ce_fwd
    topk_nll_kernel<LT> (tk_pixel_nll), k1 = 1, 5, 8 and 2, 3, 4 ........... test_topk_tie_free[*], test_topk_one_class, test_topk_ties[*]
      grid capped at 4096 blocks, the loop goes round twice ............... test_wrap_topk_forward
    topk_hist_kernel: N / 4096 blocks (1024 at most, reached at 4 194 304 values: no case here), so every thread goes round its
      loop 16 times in every case above 4096 values; pass 0 counts every value, and its 256 bins must add up to N in every case;
      above 1024 x 256 = 262 144 values ................................... test_wrap_topk_forward, test_wrap_topk_backward
    topk_scan_kernel: the deciding pass
      pass 0 (losses over 20 binades) ...................................... test_topk_tie_free[span]
      pass 1 (ordinary losses share few exponents) ........................ test_topk_tie_free[k1=*]
      passes 2 and 3 (every valid nll shares its upper 16 bits) ........... test_topk_dense_ramp
      r < m with n_gt > 0 (a tie at the threshold) ........................ test_topk_ties[2-1 | 64-1 | 64-63 | 1000-500]
      tau = 0: n_top exceeds the non-zero losses, m counts ignored pixels . test_topk_tau_zero
      n_top = N / n_top = 1 / a class of weight 0 .......................... test_topk_tie_free[n_top=N | n_top=1 | weight0]
    topk_sum_kernel (256 blocks, wraps above 65 536 values) ................ test_wrap_topk_forward, test_wrap_topk_backward
    topk_finish_kernel: r tau + sum, 1/n and (r/m)/n ....................... every top-k case (exact against select_check)
  mia_topk_ce_bwd
    topk_bwd_kernel<LT>: support {valid, bits >= tau}, scales 1/n, (r/m)/n . every top-k case
      grid capped at 8192 blocks, the loop goes round twice ............... test_wrap_topk_backward
  run-to-run bit identity of out, sel and the gradient ..................... test_topk_bit_identity[tie | wrap]
  ops._loss_slabs / SegLossFn's workspace / the kernels' partition (two slabs at 128 x 132) test_public_classes_two_slabs[cl | nchw]

k1 = 1 runs with do_bg only: without it the reference drops its only class and takes the mean over an empty class axis (NaN);
the kernel divides by nk = 0 there, and nothing is pinned for that combination.

Bounds.  Values (loss, ce, dc): |d| < VAL_TOL = 2e-6; gradients: |d| < GRAD_ATOL = 2e-7 AND max|d| / max|grad| < 2^-18 (32 fp32
ulps, the bound of tests/test_gpu_region_loss.py: at the large shapes gradients are of order 1/N and the absolute bound is empty);
counts, tau, r, m and the gradient's support exact.  One case, test_topk_tie_free[span], has class weights up to 1e3: its loss is
about 3e4 and its gradients reach 5, where one fp32 ulp (2e-3, 5e-7) already exceeds the absolute bounds; there they are scaled by
max(1, |reference|), which changes nothing for any other case.

Per-pixel nll (tk_pixel_nll), |device - float64|, derived from the arithmetic (_seg_loss_ref.pixel_nll_bound), e = 2^-24:
  v - mx rounds once, expf is within 2 ulp (HIP's documented 1 ulp, doubled) and k1 - 1 additions round once each:
        |d se| / se <= (max|v - mx| + 4 + k1 - 1) e
  logf within 1 ulp: |d log se| <= |d se| / se + 2 e log se;  mx + log se and the subtraction of the label's logit round once:
        |d u| <= |d log se| + e (|lse| + u),  u = lse - v[label]
  the class weight multiplies and rounds once more:  |d nll| <= w (|d u| + e u).
  For logits 2 N(0, 1) that is at most 3.2e-6 (k1 = 8), typically 1e-6; see the table for what was measured.

Route against route (test_seg_fast_refusals): the two forwards evaluate a pixel with the same operations -- __expf, __logf, one
division -- so their per-pixel terms differ only where the compiler contracts mx + log2(se) ln 2 into one rounding (e |lse| on a
CE term).  The sums differ in order: a thread adds T terms (T - 1 roundings), the wave six levels, the block three more, each
within e of a running sum of non-negative terms; the slabs are added in double.  So each of I, P, CEnum, CEden differs between
the routes by at most 2 (T + 10) e relatively, a ratio of two of them by twice that:
        |d loss| <= 4 (T + 10) e (ce_w ce + dice_w |dc|) + 2 e |loss|     (the last term: out[] is stored as fp32)
At hw = 780 on three slabs T = 4 (one quad per thread on the fast route, two pixels on the generic one): 6.2e-6 for ce = 1.6.
Counts must be equal.  Where only the backward is refused the forwards are the same kernel and out / coef must be bit-identical.

Measured on an MI355X (max over the cases of each test; every case prints its figures before it asserts; the table is also in
DESIGN.md, "Fold-trainer losses"):
  test                                     |dvalue|   |dgrad|    dgrad rel (bound 3.81e-6)   nll |d| / its bound
  test_seg_fast_quads                      9.5e-08    3.4e-09    1.9e-07
  test_seg_generic_shapes (k1 = 1 .. 8)    3.5e-07    3.5e-08    2.1e-07
  test_seg_fast_refusals                   1.6e-07    3.1e-10    1.8e-07       route against route 2.4e-07 (bound 7.3e-06 .. 8.3e-06)
  test_seg_grad_out                        1.1e-07    6.9e-10    2.0e-07
  test_seg_finalize_loops (7 slabs, k1 8)  1.2e-07    6.7e-10    2.4e-07
  test_seg_all_ignored                     1.0e-07    1.4e-10    1.8e-07
  test_label_decoding                      2.2e-07    1.1e-09    2.2e-07       0.41
  test_wrap_seg_backward_fast / _generic   1.5e-07    3.4e-13    2.1e-07
  test_topk_tie_free k1 = 5, 8             3.1e-07    1.0e-09    2.6e-07       0.33
  test_topk_tie_free n_top = N, 1, weight0 5.6e-07    8.0e-08    1.7e-07       0.34
  test_topk_tie_free[span] (loss 14349)    2.3e-05    8.0e-07    1.5e-07       0.47   (scaled bounds 2.9e-02, 1.1e-06)
  test_topk_ties                           2.1e-07    5.4e-10    1.6e-07       0.41
  test_topk_tau_zero / _dense_ramp         3.8e-08    1.6e-10    1.7e-07       0.35
  test_wrap_topk_forward / _backward       1.7e-07    9.5e-13    1.4e-07       0.29
  test_public_classes_two_slabs            9.5e-08    3.7e-11    2.5e-07
The relative gradient figures stay at or below 2.6e-07 (two fp32 ulps) against 3.81e-06, k1 > 4 and multi-slab sums included; a
per-pixel nll reaches at most 0.47 of its derived bound.  No branch disagreed with float64, so csrc/seg_loss.hip is unchanged.
"""
import functools

import numpy as np
import pytest
import torch

import _seg_loss_ref as R

pytestmark = pytest.mark.gpu
VAL_TOL, GRAD_ATOL, GRAD_REL = 2e-6, 2e-7, 2.0 ** -18
IGN = R.IGN
NAN_BITS = 0x7FC00000  # torch's fill NaN as a bit pattern: no count and no finite sum looks like it
SENT = -7.0e33  # fill of the logits gradient, so that a NaN the kernels compute (bad label) is told from an element never written
COUNT_SENT = -(2 ** 40) - 7


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _abi():
    import mia_hip
    from mia_hip import ops
    return mia_hip, ops


# ------------------------------------------------------------------ placing tensors
class Pix:
    """A logical [nb, k1, hw] fp32 tensor inside a filled flat device buffer: "cl" channels-last, "nchw", "sliced" (channels-last
    rows of an image four pixels longer, so sn > hw k1 while every image stays 16-byte aligned); `off` elements into the buffer."""

    def __init__(self, nb, k1, hw, layout, dev, off=0, values=None, fill=float("nan")):
        rows = hw + (4 if layout == "sliced" else 0)
        n = nb * rows * k1
        self.fill = fill
        self.flat = torch.full((off + n + 8,), fill, dtype=torch.float32, device=dev)
        body = self.flat[off:off + n]
        if layout == "nchw":
            self.view, self.st = body.view(nb, k1, hw), (k1 * hw, hw, 1)
        else:
            self.view, self.st = body.view(nb, rows, k1)[:, :hw].permute(0, 2, 1), (rows * k1, 1, k1)
        assert self.view.stride() == self.st and (self.view.data_ptr() % 16 == 0) == (off % 4 == 0)
        if values is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(values)).to(torch.float32))

    @property
    def ptr(self):
        return self.view.data_ptr()

    def take(self, finite=True):
        """The kernel's output as float64 numpy; every owned element was written, every other element still holds the fill."""
        got = self.view.detach().cpu().double().numpy().copy()
        assert not (got == self.fill).any(), "a gradient element was never written"
        if finite:
            assert np.isfinite(got).all()
        self.view.fill_(self.fill)
        rest = self.flat.cpu().numpy()
        assert (np.isnan(rest).all() if np.isnan(self.fill) else (rest == np.float32(self.fill)).all()), "a write outside the tensor"
        return got


def place_labels(labels, ltype, dev, off=0):
    lab = np.asarray(labels).reshape(-1)
    dt = torch.int64 if ltype == "int64" else torch.uint8
    if ltype == "uint8":
        assert lab.min() >= 0 and lab.max() <= 255
    flat = torch.zeros(off + lab.size + 16, dtype=dt, device=dev)
    view = flat[off:off + lab.size]
    view.copy_(torch.from_numpy(lab.astype(np.int64)).to(dt))
    return view


def expect_fast(x, lab, hw, k1, ltype, dl=None):
    """sl_fast_ok as the C entry points evaluate it, and with `dl` the backward's extra condition."""
    ok = (2 <= k1 <= 4 and x.st[1] == 1 and x.st[2] == k1 and x.st[0] == hw * k1 and hw % 4 == 0 and x.ptr % 16 == 0
          and lab.data_ptr() % (4 if ltype == "uint8" else 16) == 0)
    if dl is not None:
        ok = ok and dl.st == x.st and dl.ptr % 16 == 0
    return ok


def _i32(t):
    return t.view(torch.int32).cpu().numpy()


# ------------------------------------------------------------------ masked Dice + CE through the C ABI
def run_seg(c, dev, *, slabs, layout, ltype, route, bwd_route=None, ignore_arg="case", softmax=True, do_bg=True, batch=False,
            smooth=1e-5, w_ce=0.9, w_dice=0.6, gout=None, dl_layout=None, x_off=0, lab_off=0, dl_off=0, expect_bad=False):
    """mia_seg_loss_fwd, then mia_seg_loss_bwd.  c: a case of _seg_loss_ref (logits [nb,k1,hw], labels [nb,hw], weight).
    ignore_arg: the ignore label handed to the kernel (default: the case's own)."""
    mia_hip, ops = _abi()
    _p, cf, ci = ops._p, ops._c_float, ops._c_i64
    nb, k1, hw = c["logits"].shape
    ign = c["ignore"] if ignore_arg == "case" else ignore_arg
    x = Pix(nb, k1, hw, layout, dev, off=x_off, values=c["logits"])
    lab = place_labels(c["labels"], ltype, dev, lab_off)
    dl = Pix(nb, k1, hw, dl_layout or ("cl" if layout == "sliced" else layout), dev, off=dl_off, fill=SENT)
    assert expect_fast(x, lab, hw, k1, ltype) == (route == "fast"), "the case does not take the forward route it is listed under"
    assert expect_fast(x, lab, hw, k1, ltype, dl) == ((bwd_route or route) == "fast"), "... nor the backward route"
    cw = None if c["weight"] is None else torch.tensor(c["weight"], dtype=torch.float32, device=dev)
    flags = ((mia_hip.SEGLOSS_SOFTMAX if softmax else 0) | (mia_hip.SEGLOSS_DO_BG if do_bg else 0) | (mia_hip.SEGLOSS_BATCH if batch else 0)
             | (mia_hip.SEGLOSS_LABEL_U8 if ltype == "uint8" else 0) | (mia_hip.SEGLOSS_IGNORE if ign is not None else 0))
    words = mia_hip.lib().mia_seg_loss_workspace(nb, k1, slabs)
    stride = 5 * k1 + 2
    nslice = nb * slabs * stride
    assert words == nslice + nslice % 2 + nb * k1 * 6
    ws = torch.empty((words + 1) // 2 + 1, dtype=torch.float64, device=dev).view(torch.float32)  # 8-byte aligned, one double spare
    ws.fill_(float("nan"))
    coef = torch.full((nb * k1 * 2 + 1 + 4,), float("nan"), dtype=torch.float32, device=dev)
    out = torch.full((3 + 4,), float("nan"), dtype=torch.float32, device=dev)
    counts = torch.full((nb * k1 * 3 + 4,), COUNT_SENT, dtype=torch.int64, device=dev)
    bad = torch.zeros(2, dtype=torch.int32, device=dev)
    mia_hip.call("mia_seg_loss_fwd", _p(x.view), _p(lab), _p(cw), nb, ci(hw), k1, ci(x.st[0]), ci(x.st[1]), ci(x.st[2]), flags,
                 ci(ign if ign is not None else 0), cf(smooth), cf(w_dice), cf(w_ce), slabs, _p(ws), _p(coef), _p(out), _p(counts),
                 _p(bad), ops._stream())
    gd = None if gout is None else torch.tensor([gout], dtype=torch.float32, device=dev)
    mia_hip.call("mia_seg_loss_bwd", _p(x.view), _p(lab), _p(cw), _p(coef), _p(gd), _p(dl.view), nb, ci(hw), k1, ci(x.st[0]),
                 ci(x.st[1]), ci(x.st[2]), ci(dl.st[0]), ci(dl.st[1]), ci(dl.st[2]), flags, ci(ign if ign is not None else 0), ops._stream())
    torch.cuda.synchronize()
    # every word the kernels own was written, nothing else was
    wbits = _i32(ws)
    assert not (wbits[:nslice] == NAN_BITS).any(), "a word of a workspace slice was never written"
    tot = ws[nslice + nslice % 2:words].view(torch.float64).cpu().numpy()
    assert tot.size == nb * k1 * 3 and np.isfinite(tot).all(), "a double behind the slices was never written"
    assert (wbits[nslice:nslice + nslice % 2] == NAN_BITS).all() and (wbits[words:] == NAN_BITS).all(), "a write outside the workspace"
    cf_, out_, cnt = coef.cpu().numpy(), out.cpu().numpy(), counts.cpu().numpy()
    assert np.isnan(cf_[nb * k1 * 2 + 1:]).all() and np.isnan(out_[3:]).all() and (cnt[nb * k1 * 3:] == COUNT_SENT).all()
    cf_, out_, cnt = cf_[:nb * k1 * 2 + 1], out_[:3], cnt[:nb * k1 * 3].reshape(nb, k1, 3)
    assert not (cnt == COUNT_SENT).any(), "a count was never written"
    if expect_bad:
        assert np.isnan(out_).all() and np.isnan(cf_).all() and bad.tolist() == [0, 1], "a bad label must poison out and coef"
    else:
        assert np.isfinite(out_).all() and np.isfinite(cf_).all(), "an entry of out / coef was never written"
        assert bad.tolist() == [0, 0]
        if not do_bg:
            assert not cf_[:-1].reshape(nb, k1, 2)[:, 0].any(), "class 0 without do_bg carries exact zeros"
    return dict(out=out_.astype(np.float64), coef=cf_, counts=cnt, grad=dl.take(finite=not expect_bad), tot=tot.reshape(nb, k1, 3),
                raw=(out[:3].clone(), coef[:nb * k1 * 2 + 1].clone()))


@functools.lru_cache(maxsize=None)
def _seg_ref(key, softmax, do_bg, batch, smooth, w_ce, w_dice):
    c = CASES[key]
    return R.seg_loss(c["logits"], c["labels"], ignore=c["ignore"], weight=c["weight"], softmax=softmax, do_bg=do_bg, batch_dice=batch,
                      smooth=smooth, w_ce=w_ce, w_dice=w_dice)


CASES = {}


def seg_case(key, *args, **kw):
    if key not in CASES:
        CASES[key] = R.build_case(*args, **kw)
    return CASES[key]


def check_grad(got, want, what, scale=1.0):
    top = np.abs(want).max()
    d = np.abs(got - want).max()
    rel = d / top if top > 0 else 0.0
    print(f"{what}: |dgrad| {d:.2e}  max|grad| {top:.2e}  rel {rel:.2e} (2^-18 = {GRAD_REL:.2e})")
    if top == 0:
        assert not got.any(), "the reference gradient is exactly 0"
    assert d < GRAD_ATOL * scale and rel < GRAD_REL
    return d, rel


def check_seg(got, c, key, what, *, softmax=True, do_bg=True, batch=False, smooth=1e-5, w_ce=0.9, w_dice=0.6, gout=None):
    """Each figure is printed before it is asserted."""
    ref = _seg_ref(key, softmax, do_bg, batch, smooth, w_ce, w_dice)
    dv = [abs(got["out"][0] - ref["loss"]), abs(got["out"][1] - ref["ce"]), abs(got["out"][2] - ref["dc"])]
    print(f"{what}: |dloss| {dv[0]:.2e} |dce| {dv[1]:.2e} |ddc| {dv[2]:.2e}  (loss {ref['loss']:.4f})")
    assert max(dv) < VAL_TOL
    assert np.array_equal(got["counts"], ref["counts"]), "tp / fp / fn are exact integers"
    nb, k1, hw = c["logits"].shape
    lab = c["labels"]
    valid = np.ones_like(lab, dtype=bool) if c["ignore"] is None else lab != c["ignore"]
    g_want = np.stack([((lab == k) & valid).sum(1) for k in range(k1)], 1)
    assert np.array_equal(got["tot"][..., 2], g_want.astype(np.float64)), "G is the integer count of labelled pixels"
    want = ref["grad"] * (1.0 if gout is None else gout)
    check_grad(got["grad"], want, what)
    ign = np.broadcast_to(~valid[:, None], want.shape)
    assert not got["grad"][ign].any(), "ignored pixels carry exact zeros"
    return ref


def _rot(i, k1):
    """The switches rotate over the cases (no full product): softmax off on every fifth case, do_bg x batch_dice by the two low
    bits, class weights on two cases of three, and the ignore label 255 / none / -100 in turn."""
    return dict(softmax=i % 5 != 0, do_bg=True if k1 == 1 else bool(i % 2), batch=bool((i // 2) % 2)), i % 3 != 0, (IGN, None, -100)[i % 3]


QUADS = [("1", 8, 2), ("255", 8 * 255, 2), ("256", 8 * 256, 2), ("257", 8 * 257, 2), ("512", 8 * 512, 2), ("513", 8 * 513, 2),
         ("769", 8 * 769, 2), ("ragged", 40, 3), ("empty", 36, 4)]


@pytest.mark.parametrize("i", range(len(QUADS)), ids=[q[0] for q in QUADS])
def test_seg_fast_quads(i):
    """The fast route at every exit of its loops: a slab of 1, 255, 256, 257, 512, 513 and 769 quads (two slabs of an image of
    8 x that many pixels; six images on the tiny sizes, which keeps the gradients well below 1, where the absolute bound means something), a ragged last slab (10 quads as 4 + 4 + 2) and an empty one (9 quads as 3 + 3 + 3 + 0).  k1 = 2 + i % 3
    and the label type i % 2 reach all six template instances of the forward and of the backward."""
    dev = _dev()
    name, hw, slabs = QUADS[i]
    k1, ltype = 2 + i % 3, ("int64", "uint8")[i % 2]
    fl, weighted, ign = _rot(i, k1)
    key = ("quads", name)
    c = seg_case(key, 6 if hw <= 40 else 2, k1, hw, ignore=ign, ltype=ltype, seed=i, prob=not fl["softmax"], weighted=weighted)
    got = run_seg(c, dev, slabs=slabs, layout="cl", ltype=ltype, route="fast", ignore_arg=ign, **fl)
    check_seg(got, c, key, f"fast quads {name} k1={k1} {ltype} {fl} w={weighted} ign={ign}", **fl)


GENERIC = [(hw, slabs) for hw in (1, 7, 195, 1964) for slabs in (1, 3, 7)] + [(3, 5)]


@pytest.mark.parametrize("i", range(len(GENERIC)), ids=[f"{hw}-{s}-{1 + i % 8}" for i, (hw, s) in enumerate(GENERIC)])
def test_seg_generic_shapes(i):
    """The generic route (any strides, run-time k1 <= 8) with k1 = 1 + i % 8 on one, three and seven slabs of 1, 7, 195 and 1964
    pixels -- ragged and empty slabs, more slabs than pixels (3 on 5), more pixels than threads -- both label types, both layouts.
    Eight images on the tiny sizes keep the gradients well below 1, where the absolute bound means something."""
    dev = _dev()
    hw, slabs = GENERIC[i]
    k1, ltype = 1 + i % 8, ("int64", "uint8")[(i // 2) % 2]
    fl, weighted, ign = _rot(i, k1)
    layout = "nchw" if (2 <= k1 <= 4 and hw % 4 == 0) or i % 2 else "cl"
    key = ("generic", i)
    c = seg_case(key, 8 if hw < 100 else 2, k1, hw, ignore=ign, ltype=ltype, seed=i, prob=not fl["softmax"], weighted=weighted)
    got = run_seg(c, dev, slabs=slabs, layout=layout, ltype=ltype, route="generic", ignore_arg=ign, **fl)
    check_seg(got, c, key, f"generic hw={hw} slabs={slabs} k1={k1} {layout} {ltype} {fl} w={weighted} ign={ign}", **fl)


REFUSALS = {
    # name: (k1, ltype, run_seg arguments, forward route, backward route)
    "fast-4-uint8": (4, "uint8", dict(layout="cl"), "fast", "fast"),
    "fast-3-int64": (3, "int64", dict(layout="cl"), "fast", "fast"),
    "nchw": (3, "int64", dict(layout="nchw"), "generic", "generic"),
    "x_off4": (4, "uint8", dict(layout="cl", x_off=1), "generic", "generic"),
    "u8_off1": (4, "uint8", dict(layout="cl", lab_off=1), "generic", "generic"),
    "i64_off8": (3, "int64", dict(layout="cl", lab_off=1), "generic", "generic"),
    "sliced": (3, "int64", dict(layout="sliced"), "generic", "generic"),
    "k1=5": (5, "uint8", dict(layout="cl"), "generic", "generic"),
    "dl_nchw": (4, "uint8", dict(layout="cl", dl_layout="nchw"), "fast", "generic"),
    "dl_off4": (3, "int64", dict(layout="cl", dl_off=1), "fast", "generic"),
}
REFUSAL_HW, REFUSAL_SLABS, REFUSAL_T = 780, 3, 4
_FL = dict(softmax=True, do_bg=False, batch=False)


@pytest.mark.parametrize("name", list(REFUSALS))
def test_seg_fast_refusals(name):
    """Every term of sl_fast_ok and of the backward's extra condition refuses the fast route on its own, at hw % 4 == 0 and three
    slabs; the refused call still matches float64, and against the fast route on the same numbers the counts are equal and the
    values within the route-against-route bound of the file's docstring (bit-identical where only the backward is refused)."""
    dev = _dev()
    k1, ltype, kw, route, bwd_route = REFUSALS[name]
    key = ("refusal", k1, ltype)
    c = seg_case(key, 2, k1, REFUSAL_HW, ignore=IGN, ltype=ltype, seed=k1, weighted=True)
    got = run_seg(c, dev, slabs=REFUSAL_SLABS, ltype=ltype, route=route, bwd_route=bwd_route, **kw, **_FL)
    ref = check_seg(got, c, key, f"refusal {name}", **_FL)
    if name.startswith("fast") or k1 == 5:
        return
    fast = run_seg(c, dev, slabs=REFUSAL_SLABS, layout="cl", ltype=ltype, route="fast", **_FL)
    assert np.array_equal(got["counts"], fast["counts"]) and np.array_equal(got["tot"][..., 2], fast["tot"][..., 2])
    if route == "fast":  # the same forward kernel on the same bytes
        assert torch.equal(got["raw"][0], fast["raw"][0]) and torch.equal(got["raw"][1], fast["raw"][1])
    bound = 4 * (REFUSAL_T + 10) * R.EPS32 * (0.9 * abs(ref["ce"]) + 0.6 * abs(ref["dc"])) + 2 * R.EPS32 * abs(ref["loss"])
    d = np.abs(got["out"] - fast["out"]).max()
    print(f"refusal {name}: route against route |dvalue| {d:.2e} (bound {bound:.2e})")
    assert d <= bound


@pytest.mark.parametrize("gout", [1.0, -0.375, 3.0])
@pytest.mark.parametrize("route", ["fast", "generic"])
def test_seg_grad_out(route, gout):
    """grad_out as a device scalar on both backward routes (NULL, which reads as 1, is what every other case passes)."""
    dev = _dev()
    key = ("refusal", 2, "uint8")
    c = seg_case(key, 2, 2, REFUSAL_HW, ignore=IGN, ltype="uint8", seed=2, weighted=True)
    got = run_seg(c, dev, slabs=REFUSAL_SLABS, layout="cl" if route == "fast" else "nchw", ltype="uint8", route=route, gout=gout, **_FL)
    check_seg(got, c, key, f"grad_out {route} {gout}", gout=gout, **_FL)


@pytest.mark.parametrize("batch", [False, True], ids=["image", "batch"])
def test_seg_finalize_loops(batch):
    """nb k1 = 320 and nb slabs = 280 both exceed the finalize block's 256 threads: its (image, class) loop, its CE loop over the
    slices and its coef loop all go round twice; per-image and batch Dice."""
    dev = _dev()
    key = ("finalize",)
    c = seg_case(key, 40, 8, 28, ignore=IGN, ltype="int64", seed=7, weighted=True)
    fl = dict(softmax=True, do_bg=False, batch=batch)
    got = run_seg(c, dev, slabs=7, layout="cl", ltype="int64", route="generic", **fl)
    check_seg(got, c, key, f"finalize loops batch={batch}", **fl)


@pytest.mark.parametrize("which", ["batch", "image"])
@pytest.mark.parametrize("route", ["fast", "generic"])
def test_seg_all_ignored(route, which):
    """Nothing valid in the whole batch: ce = 0 and coef[last] = 0 (the CE term is dropped), every gradient an exact zero.  One
    image without a valid pixel: its gradients are exact zeros, its Dice terms smooth / smooth."""
    dev = _dev()
    key = ("all_ignored", which)
    c = seg_case(key, 3, 3, 780, ignore=IGN, ltype="int64", seed=3, frac_ignored=1.1 if which == "batch" else 0.2,
                 all_ignored_image=1)
    got = run_seg(c, dev, slabs=REFUSAL_SLABS, layout="cl" if route == "fast" else "nchw", ltype="int64", route=route, **_FL)
    check_seg(got, c, key, f"all ignored {which} {route}", **_FL)
    assert not got["grad"][1].any() and not got["counts"][1].any()
    if which == "batch":
        assert got["out"][1] == 0.0 and got["coef"][-1] == 0.0 and not got["grad"].any() and got["out"][2] == -1.0
    else:
        assert got["coef"][-1] > 0.0 and got["grad"][0].any()


LABEL_CASES = ["int64-ignore-100", "uint8-ignore-100", "2^32+1", "255", "lowword"]


def _label_case(kind):
    ltype = "uint8" if kind in ("uint8-ignore-100", "255") else "int64"
    key = ("labels", ltype)
    if key not in CASES:
        CASES[key] = R.label_case(ltype)
    c = dict(CASES[key])
    bad = kind in ("2^32+1", "255", "lowword")
    if bad:
        c["labels"] = c["labels"].copy()
        # the second pixel of a quad in the last slab of the second image: the quad loaders' hi / lo words of an odd position
        c["labels"][1, 777] = {"2^32+1": 2 ** 32 + 1, "255": 255, "lowword": 2 ** 32 - 100}[kind]
    return c, key, ltype, bad


@pytest.mark.parametrize("kind", LABEL_CASES)
@pytest.mark.parametrize("route", ["fast", "generic", "topk"])
def test_label_decoding(route, kind):
    """sl_quad_classes (fast route) and the scalar sl_class (generic route, top-k) with ignore_label = -100, torch's default: int64
    labels of -100 are ignored; a uint8 label can never match, so nothing is ignored; and a label that is neither -- 2^32 + 1, whose
    low word is class 1; 2^32 - 100, whose low word is the ignore label's; a uint8 255 -- raises the working flag: NaN results, NaN
    gradients, and the sticky verdict, as in test_ignore_label_against_the_bad_label_protocol."""
    dev = _dev()
    c, key, ltype, bad = _label_case(kind)
    assert (c["ignore"] == -100 and (c["labels"] == -100).any()) if ltype == "int64" else (c["ignore"] is None and c["labels"].min() >= 0)
    if route == "topk":
        n_top = R.LABEL_CASE_N_TOP
        got = run_topk(c, dev, n_top, "cl", ltype, ignore_arg=-100, expect_bad=bad)
        if bad:
            assert np.isnan(got["out"]) and np.isnan(got["sel"][1:3]).all() and np.isnan(got["grad"]).any()
        else:
            check_topk(got, c, n_top, f"labels topk {kind}")
        return
    got = run_seg(c, dev, slabs=REFUSAL_SLABS, layout="cl" if route == "fast" else "nchw", ltype=ltype, route=route, ignore_arg=-100,
                  expect_bad=bad, **_FL)
    if bad:
        valid = np.broadcast_to(((c["labels"] >= 0) & (c["labels"] < 3))[:, None], got["grad"].shape)
        assert np.isnan(got["grad"][valid]).all() and not got["grad"][~valid].any()
    else:
        check_seg(got, c, key, f"labels {route} {kind}", **_FL)


def test_wrap_seg_backward_fast():
    """seg_loss_bwd_fast_kernel's grid is capped at 512 blocks x 256 quads = 524 288 pixels per image: one channels-last image of
    524 288 + 2048 pixels (514 blocks' worth) sends blocks 0 and 1 round the loop a second time.  64 slabs, as ops._loss_slabs
    chooses: 2056 quads per slab, four turns of the forward's pair loop plus its tail."""
    dev = _dev()
    from mia_hip import ops
    hw = 512 * 256 * 4 + 2048
    assert ops._loss_slabs(hw) == 64 and (hw // 4 + 255) // 256 > 512
    key = ("wrap_fast",)
    c = seg_case(key, 1, 2, hw, ignore=IGN, ltype="uint8", seed=1, weighted=True)
    got = run_seg(c, dev, slabs=64, layout="cl", ltype="uint8", route="fast", gout=-0.375, **_FL)
    check_seg(got, c, key, "wrap seg bwd fast", gout=-0.375, **_FL)


def test_wrap_seg_backward_generic():
    """seg_loss_bwd_kernel's grid is capped at 8192 blocks x 256 = 2 097 152 pixels: two NCHW images of 1 048 576 + 1029 pixels
    (8201 blocks' worth) wrap it, and a wrapped block crosses from the first image into the second."""
    dev = _dev()
    hw = 8192 * 256 // 2 + 1029
    assert (2 * hw + 255) // 256 > 8192
    key = ("wrap_generic",)
    c = seg_case(key, 2, 2, hw, ignore=IGN, ltype="int64", seed=2)
    got = run_seg(c, dev, slabs=128, layout="nchw", ltype="int64", route="generic", gout=3.0, **_FL)
    check_seg(got, c, key, "wrap seg bwd generic", gout=3.0, **_FL)


# ------------------------------------------------------------------ top-k CE through the C ABI
TK_HIST = 4 * 256


def run_topk(c, dev, n_top, layout, ltype, *, ignore_arg="case", gout=None, dl_layout=None, expect_bad=False):
    """mia_topk_ce_fwd, then mia_topk_ce_bwd; the workspace is read back whole: nll [N], sel [4], histograms [4][256], state [4],
    partial sums [256]."""
    mia_hip, ops = _abi()
    _p, ci = ops._p, ops._c_i64
    nb, k1, hw = c["logits"].shape
    n = nb * hw
    ign = c["ignore"] if ignore_arg == "case" else ignore_arg
    x = Pix(nb, k1, hw, layout, dev, values=c["logits"])
    lab = place_labels(c["labels"], ltype, dev)
    dl = Pix(nb, k1, hw, dl_layout or layout, dev, fill=SENT)
    cw = None if c["weight"] is None else torch.tensor(c["weight"], dtype=torch.float32, device=dev)
    flags = (mia_hip.SEGLOSS_LABEL_U8 if ltype == "uint8" else 0) | (mia_hip.SEGLOSS_IGNORE if ign is not None else 0)
    words = mia_hip.lib().mia_topk_ce_workspace(ci(n))
    assert words == n + 4 + TK_HIST + 4 + 256
    ws = torch.full((words + 8,), float("nan"), dtype=torch.float32, device=dev)
    out = torch.full((1 + 3,), float("nan"), dtype=torch.float32, device=dev)
    bad = torch.zeros(2, dtype=torch.int32, device=dev)
    mia_hip.call("mia_topk_ce_fwd", _p(x.view), _p(lab), _p(cw), nb, ci(hw), k1, ci(x.st[0]), ci(x.st[1]), ci(x.st[2]), flags,
                 ci(ign if ign is not None else 0), ci(n_top), _p(ws), _p(out), _p(bad), ops._stream())
    gd = None if gout is None else torch.tensor([gout], dtype=torch.float32, device=dev)
    mia_hip.call("mia_topk_ce_bwd", _p(x.view), _p(lab), _p(cw), _p(ws), _p(gd), _p(dl.view), nb, ci(hw), k1, ci(x.st[0]), ci(x.st[1]),
                 ci(x.st[2]), ci(dl.st[0]), ci(dl.st[1]), ci(dl.st[2]), flags, ci(ign if ign is not None else 0), ops._stream())
    torch.cuda.synchronize()
    w = _i32(ws).view(np.uint32)
    bits, sel, hist = w[:n].copy(), w[n:n + 4], w[n + 4:n + 4 + TK_HIST].reshape(4, 256)
    state, part = w[n + 4 + TK_HIST:n + 8 + TK_HIST], w[n + 8 + TK_HIST:words]
    assert not (bits == NAN_BITS).any(), "an nll was never written"
    assert not (hist == NAN_BITS).any() and not (state[:3] == NAN_BITS).any() and not (part == NAN_BITS).any() and part.size == 256
    assert (w[words:] == NAN_BITS).all() and np.isnan(out[1:].cpu().numpy()).all(), "a write outside the workspace"
    assert int(hist[0].sum(dtype=np.int64)) == n, "pass 0 counts every value once"
    selv = sel.view(np.float32)
    if expect_bad:
        assert bad.tolist() == [0, 1]
    else:
        assert bad.tolist() == [0, 0] and not (sel[:3] == NAN_BITS).any()
    raw = (out.clone(), ws[n:n + 3].clone(), dl.flat.clone())
    return dict(bits=bits, sel=selv.copy(), sel_bits=sel.copy(), state=state.copy(), hist=hist.copy(), out=float(out[0].item()),
                grad=dl.take(finite=not expect_bad), raw=raw)


def check_topk(got, c, n_top, what, gout=None, scale=False):
    """nll against float64 within the per-pixel bound; tau, r, m exactly against select_check on the device's own bits; the
    gradient's support exactly {valid, bits >= tau}; value and gradient (hence the scales 1/n and (r/m)/n) against float64."""
    nb, k1, hw = c["logits"].shape
    n = nb * hw
    nll = R.pixel_nll(c["logits"], c["labels"], c["ignore"], c["weight"])
    bound = R.pixel_nll_bound(c["logits"], c["labels"], c["ignore"], c["weight"])
    dev_nll = got["bits"].view(np.float32).astype(np.float64)
    err = np.abs(dev_nll - nll)
    worst = (err / np.maximum(bound, 1e-300)).max() if (bound > 0).any() else 0.0
    print(f"{what}: nll max|d| {err.max():.2e}, max |d| / bound {worst:.3f} (max bound {bound.max():.2e})")
    assert (err <= bound).all(), "a per-pixel nll is further from float64 than the derived bound"
    valid = (np.ones(n, dtype=bool) if c["ignore"] is None else c["labels"].reshape(-1) != c["ignore"])
    assert not got["bits"][~valid].any(), "ignored pixels store +0"
    tau, r, m = R.select_check(got["bits"], n_top)
    print(f"{what}: tau {np.array([tau], dtype=np.uint32).view(np.float32)[0]:.6g} r {r} m {m}; device state {got['state'][:3].tolist()}")
    assert (int(got["state"][0]), int(got["state"][1]), int(got["state"][2])) == (tau, r, m)
    assert int(got["sel_bits"][0]) == tau
    assert got["sel"][1] == np.float32(1.0 / n_top) and got["sel"][2] == np.float32((r / m) / n_top)
    live = valid & (got["bits"] >= tau)
    grad = got["grad"]
    if k1 == 1:
        assert not grad.any()  # softmax of one class is 1: every term cancels exactly
    else:
        assert np.array_equal(grad.any(axis=1).reshape(-1), live), "the gradient's support is {valid, bits >= tau}"
    want = R.topk_ce(c["logits"], c["labels"], 100.0 * (n_top + 0.5) / n, ignore=c["ignore"], weight=c["weight"])
    assert want["n"] == n_top
    s = max(1.0, abs(want["loss"])) if scale else 1.0
    dv = abs(got["out"] - want["loss"])
    print(f"{what}: |dvalue| {dv:.2e} (loss {want['loss']:.6g}); float64 n_gt {want['n_gt']} n_eq {want['n_eq']}")
    assert dv < VAL_TOL * s
    assert (want["n_gt"], want["n_eq"]) == (n_top - r, m), "the device ties where float64 ties"
    wg = want["grad"] * (1.0 if gout is None else gout)
    check_grad(grad, wg, what, scale=max(1.0, np.abs(wg).max()) if scale else 1.0)
    return tau, r, m


@functools.lru_cache(maxsize=None)
def _free_cases():
    return R.topk_free_cases()


@pytest.mark.parametrize("name", list(R.topk_free_cases()))
def test_topk_tie_free(name):
    """The tie-free grid at k1 = 5 and 8 (the public-class grid of test_gpu_seg_loss.py has 2, 3, 4), n_top = N, n_top = 1, a class of
    weight 0, and losses over many binades (class weights 1e-3 .. 1e3, logits x 8) so that the first radix pass decides.  That no
    two losses near the threshold can swap is asserted on the CPU for each (test_seg_loss_host.py), so r = m = 1 here."""
    dev = _dev()
    c = _free_cases()[name]
    got = run_topk(c, dev, c["n_top"], c["layout"], c["ltype"], gout=-0.375 if "k1=8" in name else None)
    tau, r, m = check_topk(got, c, c["n_top"], f"topk {name}", gout=-0.375 if "k1=8" in name else None, scale=name == "span")
    assert (r, m) == (1, 1)
    if name == "span":
        assert np.count_nonzero(got["hist"][0]) >= 8 and got["hist"][1].sum() < 0.5 * got["bits"].size
    if name == "weight0":
        assert not got["grad"][np.broadcast_to((c["labels"] == 2)[:, None], got["grad"].shape)].any()


@pytest.mark.parametrize("ltype", ["int64", "uint8"])
def test_topk_one_class(ltype):
    """k1 = 1: every nll is 0, so everything ties at tau = 0 (r = n_top, m = N), the loss is 0 and the gradient exactly 0 -- the
    one member of the extended grid that cannot be tie-free."""
    dev = _dev()
    c = seg_case(("topk1", ltype), 3, 1, 620, ignore=IGN, ltype=ltype, seed=1)
    got = run_topk(c, dev, 186, "cl", ltype)
    assert check_topk(got, c, 186, f"topk k1=1 {ltype}") == (0, 186, 1860)
    assert got["out"] == 0.0


@pytest.mark.parametrize("m,r", list(R.TIE_CASES), ids=lambda v: str(v))
def test_topk_ties(m, r):
    """A tie at the threshold with pixels above it: group A (n_gt distinct larger losses), m bit-identical copies of one pixel
    spread over the images, group B below; n_top = |A| + r.  k1 and the layouts rotate."""
    dev = _dev()
    i = list(R.TIE_CASES).index((m, r))
    k1 = (3, 2, 8, 3)[i]
    c = R.tie_case(m, r, k1=k1, **R.TIE_CASES[(m, r)])
    got = run_topk(c, dev, c["n_top"], ("cl", "nchw")[i % 2], ("int64", "uint8")[(i // 2) % 2], gout=3.0 if i == 3 else None)
    tau, r_, m_ = check_topk(got, c, c["n_top"], f"topk tie m={m} r={r} k1={k1}", gout=3.0 if i == 3 else None)
    assert (r_, m_) == (r, m) and np.array_equal(got["bits"] == tau, c["tied"])


def test_topk_tau_zero():
    """k = 90 % with 20 % of the pixels ignored: n_top exceeds the number of non-zero losses, so tau = 0, every valid pixel lies
    above it and the m pixels at tau are the ignored ones -- which share r slots on paper and still get exactly zero gradient."""
    dev = _dev()
    c = seg_case(("tau0",), 2, 3, 1000, ignore=IGN, ltype="uint8", seed=5)
    nll = R.pixel_nll(c["logits"], c["labels"], c["ignore"])
    bound = R.pixel_nll_bound(c["logits"], c["labels"], c["ignore"])
    valid = c["labels"].reshape(-1) != IGN
    assert (nll[valid] > 100 * bound[valid]).all()  # from float64 alone: no valid loss can round to zero
    n_top, n_valid = 1800, int(valid.sum())
    assert n_valid < n_top
    got = run_topk(c, dev, n_top, "nchw", "uint8")
    assert check_topk(got, c, n_top, "topk tau=0") == (0, n_top - n_valid, 2000 - n_valid)
    assert not got["grad"][np.broadcast_to(~valid.reshape(2, 1, 1000), got["grad"].shape)].any()


def test_topk_dense_ramp():
    """Every valid nll in [1 + 2^-10, 1 + 2^-7 - 2^-10]: the upper 16 bits of all of them are 0x3F80, asserted first on the nll
    read back from the device, so passes 0 and 1 find one occupied bin above the zeros and passes 2 and 3 pick tau in the middle of
    the ramp."""
    dev = _dev()
    c = R.dense_ramp()
    got = run_topk(c, dev, c["n_top"], "cl", "int64")
    valid = c["labels"].reshape(-1) != IGN
    assert np.unique(got["bits"][valid] >> 16).tolist() == [0x3F80] and not got["bits"][~valid].any()
    assert np.count_nonzero(got["hist"][0]) == 2 and np.count_nonzero(got["hist"][1]) == 1  # bin 0 holds the zeros on pass 0 only
    assert np.count_nonzero(got["hist"][2]) > 100 and got["hist"][2].sum() == c["n_valid"]
    tau, r, m = check_topk(got, c, c["n_top"], "topk dense ramp")
    assert (r, m) == (1, 1)


def _wrap_topk(dev, nb, hw, n_above, frac, ltype, layout, gout=None):
    c = R.gap_case(nb, hw, n_above, frac_ignored=frac)
    got = run_topk(c, dev, c["n_top"], layout, ltype, gout=gout)
    return c, got


def test_wrap_topk_forward():
    """topk_nll_kernel's grid is capped at 4096 blocks x 256 = 1 048 576 pixels: 2 x (524 288 + 515) pixels wrap it.  The same
    size is past topk_hist_kernel's 1024 x 256 = 262 144 (its grid is N / 4096 blocks, 257 here, each thread going round 16 times)
    and past topk_sum_kernel's 256 blocks x 256 = 65 536 values (17 rounds).  The selection is tie-free by construction
    (_seg_loss_ref.gap_case), asserted on the CPU."""
    dev = _dev()
    hw = 4096 * 256 // 2 + 515
    assert (2 * hw + 255) // 256 > 4096 and 2 * hw > 262144
    c, got = _wrap_topk(dev, 2, hw, 150000, 0.2, "uint8", "cl")
    assert check_topk(got, c, c["n_top"], "wrap topk fwd")[1:] == (1, 1)


def test_wrap_topk_backward():
    """topk_bwd_kernel's grid is capped at 8192 blocks x 256 = 2 097 152 pixels: 2 x (1 048 576 + 1029) NCHW pixels wrap it."""
    dev = _dev()
    hw = 8192 * 256 // 2 + 1029
    assert (2 * hw + 255) // 256 > 8192
    c, got = _wrap_topk(dev, 2, hw, 200000, 0.0, "int64", "nchw", gout=-0.375)
    assert check_topk(got, c, c["n_top"], "wrap topk bwd", gout=-0.375)[1:] == (1, 1)


@pytest.mark.parametrize("which", ["tie", "wrap"])
def test_topk_bit_identity(which):
    """Two runs of a tie case and of a case that wraps every grid: out, sel and the whole gradient buffer bit for bit."""
    dev = _dev()
    runs = []
    for _ in range(2):
        if which == "tie":
            c = R.tie_case(64, 63, k1=3, **R.TIE_CASES[(64, 63)])
            runs.append(run_topk(c, dev, c["n_top"], "cl", "int64"))
        else:
            runs.append(_wrap_topk(dev, 2, 4096 * 256 // 2 + 515, 150000, 0.2, "uint8", "cl")[1])
    a, b = runs
    assert np.array_equal(a["bits"], b["bits"]) and np.array_equal(a["state"][:3], b["state"][:3]) and np.array_equal(a["hist"], b["hist"])
    for u, v in zip(a["raw"], b["raw"]):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))


# ------------------------------------------------------------------ the public classes at the slab count Python chooses
@pytest.mark.parametrize("layout", ["cl", "nchw"])
def test_public_classes_two_slabs(layout):
    """DC_and_CE_loss and TopKLoss at 128 x 132 = 16 896 pixels, where ops._loss_slabs gives two slabs: _loss_slabs, SegLossFn's
    workspace sizing and the kernels' partition agree (k1 = 3, both layouts)."""
    from losses.ce_loss import TopKLoss
    from losses.compound_losses import DC_and_CE_loss
    from mia_hip import ops
    dev = _dev()
    h, w = 128, 132
    assert ops._loss_slabs(h * w) == 2
    key = ("public",)
    c = seg_case(key, 3, 3, h * w, ignore=IGN, seed=4)
    t = torch.from_numpy(c["logits"]).float().reshape(3, 3, h, w).to(dev)
    if layout == "cl":
        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    y = torch.from_numpy(c["labels"]).reshape(3, 1, h, w).to(dev)
    fl = dict(softmax=True, do_bg=False, batch=False, smooth=1e-5, w_ce=0.9, w_dice=0.6)
    ref = _seg_ref(key, *fl.values())
    x = t.clone().requires_grad_(True)
    fn = DC_and_CE_loss({"smooth": 1e-5, "do_bg": False}, {}, weight_ce=0.9, weight_dice=0.6, ignore_label=IGN)
    v = fn(x, y)
    v.backward()
    dv = abs(v.item() - ref["loss"])
    print(f"public DC_and_CE {layout}: |dvalue| {dv:.2e}")
    assert dv < VAL_TOL and abs(fn.last_ce.item() - ref["ce"]) < VAL_TOL and abs(fn.last_dc.item() - ref["dc"]) < VAL_TOL
    assert x.grad.stride() == x.stride()
    check_grad(x.grad.cpu().double().numpy().reshape(3, 3, -1), ref["grad"], f"public DC_and_CE {layout}")
    assert np.array_equal(fn.last_hard_counts.cpu().numpy(), ref["counts"])
    want = R.topk_ce(c["logits"], c["labels"], 10, ignore=IGN)
    assert want["n_eq"] == 1 and want["n"] == int(3 * h * w * 10 / 100)  # the rank gap itself: test_rank_gap_of_every_tie_free_case
    x = t.clone().requires_grad_(True)
    v = TopKLoss(ignore_index=IGN, k=10)(x, y)
    v.backward()
    dv = abs(v.item() - want["loss"])
    print(f"public TopKLoss {layout}: |dvalue| {dv:.2e}")
    assert dv < VAL_TOL
    g = x.grad.cpu().double().numpy().reshape(3, 3, -1)
    check_grad(g, want["grad"], f"public TopKLoss {layout}")
    assert np.array_equal(g.any(axis=1), want["grad"].any(axis=1))
    ops.check_labels()
