"""Bit-exact integer probes of every conv, input-gradient and weight-gradient kernel family (csrc/conv_mma*.hip, conv64*.hip,
conv_bt.hip, conv_pw.hip, stem.hip, wgrad_*.hip) and of the weight pack / split (pack.hip).

Operands are small integers, so every product is exact in bf16 / f16 / fp32 and every fp32 partial sum is an integer below 2^24
(asserted on the reference: tests/_conv_ref.py `exact_ok`): the result of ANY correct kernel, whatever its tiling and summation
order, is the fp64 convolution rounded once to the storage dtype.  Comparisons are torch.equal -- per element, borders, seams,
channel tails and statistics included; there is no tolerance anywhere in this file.  Each row names the kernel family it must
hit and asserts `mia_conv_mma_family` / `mia_wgrad_family` (the dispatcher's own selection function) before it launches.

The case tables are imported by tests/test_conv_ref_host.py, which checks the preconditions of every row and that every family
appears, without a GPU."""
import functools
import zlib

import pytest
import torch

import _conv_ref as R

BF, F32 = torch.bfloat16, torch.float32
G3S1, G3S2, G2S2, T3S2, T2S2, G1 = R.G3S1, R.G3S2, R.G2S2, R.T3S2, R.T2S2, R.G1
W3S1, W3S2, W2S2 = R.W3S1, R.W3S2, R.W2S2
KS = {G3S1: 3, G3S2: 3, G2S2: 2, T3S2: 3, T2S2: 2, G1: 1}
# K-terms that meet in one output element (T3S2: at most 2 x 2 taps per parity class; T2S2: one)
TAPS_PER_OUT = {G3S1: 9, G3S2: 9, G2S2: 4, T3S2: 4, T2S2: 1, G1: 1}

# every kernel-selection option a row depends on is set explicitly (other tests leave some of them changed) and restored
CONV_OPTS = {"conv_bt": 1, "conv_bt_order": 1, "conv64": 1, "conv64_dma": 1, "conv_s2_wide": 1, "conv_pw": 1, "conv_pw_s2": 1,
             "conv_xcd": 1, "f32_split": 2, "reserve_cus": 0}
WGRAD_OPTS = {"wgrad_bt": 1, "wgrad_t2": 1, "wgrad_dma": 1, "wgrad_xcd": 1, "f32_split": 2, "reserve_cus": 0}


def _conv(name, mode, dtype, c1, c2, nout, fam, hw=(19, 37), n=2, **kw):
    """hw: INPUT size.  Keys: split_out (o1 of two destinations), grad (input gradient: the parameter is packed with n_from_d0 = 0;
    G3S1 then flips the taps), bias, stats (None: no statistics run; else the family of the run WITH statistics), odd (T3S2 output
    parity), opts, variant ('plain' | 'nl' | 'acc'), slope, split (fp32: 0 = exact MFMAs, 1 / 2 = option f32_split with maxima)."""
    row = dict(name=name, mode=mode, dtype=dtype, c1=c1, c2=c2, nout=nout, fam=fam, hw=hw, n=n, split_out=None, grad=False,
               bias=None, stats=None, odd=(0, 0), opts={}, variant="plain", slope=0.0, split=0)
    row.update(kw)
    if row["bias"] is None:  # the forwards carry a bias, the gradients none (as the model calls them)
        row["bias"] = not row["grad"] and row["variant"] != "acc"
    return row


CONV_ROWS = [
    # ---- bf16, 3x3 stride 1
    _conv("g3s1_dma_2dest", G3S1, BF, 64, 0, 128, "CONV64_DMA", split_out=64, grad=True, stats="CONV64_DMA"),
    _conv("g3s1_dma_all", G3S1, BF, 64, 0, 64, "CONV64_DMA", opts={"conv64_dma": 2}, stats="CONV64_DMA"),
    _conv("g3s1_conv64", G3S1, BF, 64, 0, 64, "CONV64", stats="CONV64"),
    _conv("g3s1_conv64_2dest", G3S1, BF, 64, 0, 128, "CONV64", split_out=64, grad=True, opts={"conv64_dma": 0}, stats="CONV64"),
    _conv("g3s1_bt128", G3S1, BF, 128, 0, 128, "CONV_BT", stats="CONV_BT"),
    _conv("g3s1_bt96", G3S1, BF, 96, 0, 96, "CONV_BT", stats="CONV_BT"),
    _conv("g3s1_bt64", G3S1, BF, 128, 0, 64, "CONV_BT", stats="CONV_BT"),
    _conv("g3s1_bt_2src", G3S1, BF, 64, 64, 128, "CONV_BT", stats="CONV_BT"),
    _conv("g3s1_bt_2dest", G3S1, BF, 128, 0, 128, "CONV_BT", split_out=64, grad=True, stats="CONV_BT"),
    _conv("g3s1_fast", G3S1, BF, 128, 0, 128, "FAST", opts={"conv_bt": 0}, stats="FAST"),
    _conv("g3s1_fast_32_96", G3S1, BF, 32, 96, 64, "FAST", stats="FAST"),
    _conv("g3s1_fast_512", G3S1, BF, 512, 0, 32, "FAST", stats="FAST"),  # cin = 512: a corner pixel sums 4 x 512 terms
    _conv("g3s1_generic", G3S1, BF, 12, 20, 40, "GENERIC", stats="GENERIC"),
    _conv("g3s1_7x21", G3S1, BF, 64, 0, 64, "FAST", hw=(7, 21), stats="FAST"),  # hout <= 8: 8-row tiles, no persistent kernel
    # persistent kernels with more work items than workgroups (shapes of tests/test_gpu_ops.py's multi-item cases)
    _conv("g3s1_conv64_items", G3S1, BF, 64, 0, 64, "CONV64", hw=(200, 216), n=3, stats="CONV64"),
    _conv("g3s1_dma_items", G3S1, BF, 64, 0, 64, "CONV64_DMA", hw=(200, 216), n=2, opts={"conv64_dma": 2}, stats="CONV64_DMA"),
    _conv("g3s1_bt_items", G3S1, BF, 64, 0, 128, "CONV_BT", hw=(200, 216), n=3, stats="CONV_BT"),
    # ---- bf16, 3x3 stride 2 (input 37 x 73 -> 19 x 37)
    _conv("g3s2_wide", G3S2, BF, 128, 0, 128, "S2_WIDE", hw=(37, 73), opts={"conv_pw_s2": 0}, stats="S2_WIDE"),
    _conv("g3s2_pw", G3S2, BF, 64, 0, 128, "CONV_PW", hw=(37, 73), stats="FAST"),  # ragged maps: no statistics on conv_pw
    _conv("g3s2_pw_stats", G3S2, BF, 64, 0, 128, "CONV_PW", hw=(32, 64), stats="CONV_PW"),  # 16 x 32: whole 128-pixel runs
    _conv("g3s2_fast", G3S2, BF, 64, 0, 64, "FAST", hw=(37, 73), opts={"conv_pw_s2": 0}, stats="FAST"),
    _conv("g3s2_generic", G3S2, BF, 12, 20, 40, "GENERIC", hw=(37, 73), stats="GENERIC"),
    _conv("g3s2_7x21", G3S2, BF, 64, 0, 128, "FAST", hw=(13, 41), opts={"conv_pw_s2": 0}, stats="FAST"),
    # ---- bf16, transposed 3x3 stride 2 (the strided conv's input gradient): all four parity classes, odd and even output sizes
    _conv("t3s2_fast_odd", T3S2, BF, 128, 0, 64, "FAST", odd=(1, 1), grad=True),
    _conv("t3s2_fast_even", T3S2, BF, 64, 0, 64, "FAST", odd=(0, 1), grad=True, split_out=32),
    _conv("t3s2_generic", T3S2, BF, 40, 0, 32, "GENERIC", odd=(1, 0), grad=True, split_out=12),
    _conv("t3s2_7x21", T3S2, BF, 64, 0, 64, "FAST", hw=(4, 11), odd=(1, 1), grad=True),
    # ---- bf16, ConvTranspose 2x2 forward (T2S2) and input gradient (G2S2)
    _conv("t2s2_pw", T2S2, BF, 128, 0, 64, "CONV_PW", grad=True, bias=True),  # (the ConvTranspose parameter is [cin][cout]: n_from_d0 = 0)
    _conv("t2s2_pw_items", T2S2, BF, 128, 0, 64, "CONV_PW", hw=(128, 96), n=4, grad=True, bias=True),
    _conv("t2s2_fast", T2S2, BF, 128, 0, 64, "FAST", grad=True, bias=True, opts={"conv_pw": 0}),
    _conv("t2s2_generic", T2S2, BF, 20, 0, 12, "GENERIC", grad=True, bias=True),
    _conv("t2s2_7x21", T2S2, BF, 64, 0, 32, "FAST", hw=(3, 10), grad=True, bias=True),
    _conv("g2s2_pw", G2S2, BF, 64, 0, 128, "CONV_PW", hw=(38, 74), bias=False, stats="FAST"),
    _conv("g2s2_fast", G2S2, BF, 64, 0, 128, "FAST", hw=(38, 74), bias=False, opts={"conv_pw": 0}),
    _conv("g2s2_generic", G2S2, BF, 12, 0, 20, "GENERIC", hw=(38, 74), bias=False, stats="GENERIC"),
    _conv("g2s2_7x21", G2S2, BF, 32, 0, 64, "FAST", hw=(14, 42), bias=False),
    # ---- bf16, 1x1
    _conv("g1_fast_64_128", G1, BF, 64, 0, 128, "FAST", stats="FAST"),
    _conv("g1_fast_96_32", G1, BF, 96, 0, 32, "FAST", stats="FAST"),
    _conv("g1_fast_512", G1, BF, 512, 0, 128, "FAST"),
    _conv("g1_generic", G1, BF, 12, 0, 20, "GENERIC", stats="GENERIC"),
    _conv("g1_dgrad", G1, BF, 128, 0, 64, "FAST", grad=True),
    _conv("g1_7x21", G1, BF, 64, 0, 64, "FAST", hw=(7, 21)),
    # ---- fp32: exact-MFMA kernels (no maxima) and the split-f16 kernels (option f32_split = 1 / 2, size gate lifted)
    *[_conv(f"f32_{tag}_s{sp}", mode, F32, c1, c2, nout, fam, hw=hw, split=sp, **kw)
      for sp in (0, 1, 2)
      for tag, mode, c1, c2, nout, fam, hw, kw in [
          ("g3s1", G3S1, 64, 0, 64, "FAST", (19, 37), dict(stats="FAST")),
          ("g3s1_2src", G3S1, 32, 32, 48, "FAST", (19, 37), dict(stats="FAST")),
          ("g3s1_dgrad", G3S1, 64, 0, 64, "FAST", (19, 37), dict(grad=True, split_out=32)),
          ("g3s2", G3S2, 32, 0, 64, "FAST", (37, 73), dict(stats="FAST")),
          ("g3s2_2src", G3S2, 16, 16, 32, "FAST", (37, 73), dict()),
          ("t3s2", T3S2, 64, 0, 32, "FAST", (19, 37), dict(grad=True, odd=(1, 1))),
          ("t2s2", T2S2, 64, 0, 32, "FAST", (19, 37), dict(grad=True, bias=True)),
      ]],
    _conv("f32_g3s1_generic", G3S1, F32, 12, 20, 40, "GENERIC", stats="GENERIC"),
    _conv("f32_g3s1_7x21", G3S1, F32, 32, 0, 32, "FAST", hw=(7, 21), split=2),
    # ---- normalise-on-load (conv64): integer coefficients, each slope
    *[_conv(f"nl_slope_{s}", G3S1, BF, 64, 0, 64, "NL", variant="nl", slope=s, stats="NL") for s in (0.0, 0.5, 1.0)],
    # ---- out += conv
    _conv("acc_t3s2_bf16", T3S2, BF, 128, 0, 64, "ACC", variant="acc", grad=True, odd=(1, 1)),
    _conv("acc_g3s1_bf16", G3S1, BF, 64, 0, 64, "ACC", variant="acc", grad=True),
    _conv("acc_t3s2_f32", T3S2, F32, 64, 0, 32, "ACC", variant="acc", grad=True, odd=(0, 0)),
    _conv("acc_g3s1_f32", G3S1, F32, 32, 0, 32, "ACC", variant="acc", grad=True),
    _conv("acc_t3s2_f32_split", T3S2, F32, 64, 0, 32, "ACC", variant="acc", grad=True, odd=(1, 1), split=2),
    _conv("acc_g3s1_f32_split", G3S1, F32, 32, 0, 32, "ACC", variant="acc", grad=True, split=1),
]
CONV_BY_NAME = {r["name"]: r for r in CONV_ROWS}
assert len(CONV_BY_NAME) == len(CONV_ROWS)


def _wg(name, mode, dtype, c1, c2, cdy, fam, hw=(19, 37), n=2, **kw):
    """hw: the dy grid.  Keys: opts, nl (slope or None), split, model (ops.WGRAD_KSPLIT_MODEL)."""
    row = dict(name=name, mode=mode, dtype=dtype, c1=c1, c2=c2, cdy=cdy, fam=fam, hw=hw, n=n, opts={}, nl=None, split=0, model=True)
    row.update(kw)
    return row


WGRAD_ROWS = [
    _wg("dma96", W3S1, BF, 96, 0, 96, "DMA96"),
    _wg("dma96_2src", W3S1, BF, 96, 96, 96, "DMA96"),
    _wg("bt_3s1", W3S1, BF, 128, 0, 128, "BT"),
    _wg("bt_3s2", W3S2, BF, 64, 0, 128, "BT"),
    _wg("bt_2s2", W2S2, BF, 64, 0, 128, "BT"),
    _wg("dma", W3S1, BF, 64, 0, 64, "DMA"),
    _wg("dma_2src_slabs", W3S1, BF, 64, 32, 64, "DMA", model=False),  # plain split rule: one slab per pixel tile
    _wg("dma_7x21", W3S1, BF, 64, 0, 64, "DMA", hw=(7, 21)),
    _wg("2wg", W3S1, BF, 64, 0, 64, "2WG", opts={"wgrad_dma": 0}),
    _wg("2wg_slabs", W3S1, BF, 64, 0, 64, "2WG", opts={"wgrad_dma": 0}, model=False),
    *[_wg(f"2wg_nl_{s}", W3S1, BF, 64, 0, 64, "2WG_NL", nl=s) for s in (0.0, 0.5, 1.0)],
    _wg("tile_fast_3s2", W3S2, BF, 32, 0, 64, "TILE_FAST"),
    _wg("tile_fast_2s2", W2S2, BF, 64, 0, 128, "TILE_FAST", opts={"wgrad_t2": 0}),
    _wg("tile_fast_3s2_7x21", W3S2, BF, 64, 0, 64, "TILE_FAST", hw=(7, 21)),
    _wg("generic_bf16", W3S1, BF, 12, 20, 40, "GENERIC"),
    _wg("generic_bf16_3s2", W3S2, BF, 12, 0, 20, "GENERIC"),
    _wg("generic_bf16_2s2", W2S2, BF, 12, 0, 20, "GENERIC"),
    *[_wg(f"f32_fast_{tag}_s{sp}", mode, F32, c1, c2, cdy, "F32_FAST", split=sp)
      for sp in (0, 1, 2) for tag, mode, c1, c2, cdy in [("3s1", W3S1, 64, 0, 64), ("3s1_2src", W3S1, 32, 64, 48), ("3s2", W3S2, 32, 0, 64),
                                                          ("2s2", W2S2, 32, 0, 64)]],
    *[_wg(f"f32_narrow_{tag}_s{sp}", mode, F32, c1, 0, cdy, "F32_NARROW", split=sp)
      for sp in (0, 2) for tag, mode, c1, cdy in [("3s1", W3S1, 32, 32), ("3s2", W3S2, 16, 32), ("2s2", W2S2, 16, 32)]],
    _wg("generic_f32", W3S1, F32, 10, 7, 13, "GENERIC"),  # fp32: channel counts that are no multiple of 4
]
WGRAD_BY_NAME = {r["name"]: r for r in WGRAD_ROWS}
assert len(WGRAD_BY_NAME) == len(WGRAD_ROWS)

STEM_ROWS = [(c0, dtype) for c0 in (16, 8, 96) for dtype in (F32, BF)]  # c0 % 16 == 0: the MFMA kernel; 8: the VALU kernel


def _seed(name, extra=0):
    return zlib.crc32(name.encode()) % (1 << 30) + extra


# ------------------------------------------------------------------ operands + fp64 reference (CPU; shared with the host test)
@functools.lru_cache(maxsize=3)
def conv_case(name, stats):
    """Operands and reference of one row: dense `nonneg` operands without statistics (large values: low-precision accumulators or a
    wrong rounding mode cannot pass), sparse `signed` ones with (|y| <= 256, so it does not matter where the kernel sums)."""
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    row = CONV_BY_NAME[name]
    g = R.gen(_seed(name, int(stats)))
    mode, n, (hin, win), c1, c2, nout = row["mode"], row["n"], row["hw"], row["c1"], row["c2"], row["nout"]
    hout, wout = R.out_hw(mode, hin, win, row["odd"])
    cin, k = c1 + c2, KS[mode]
    # out += conv in bf16 adds the tile as the kernel holds it for the store, i.e. ALREADY rounded to bf16: out = rn(out + rn(conv))
    # (csrc/conv_mma_fast.hip epilogue; pinned by tests/test_gpu_ops.py::test_skip_gradient_accumulated_in_the_stride2_input_gradient).
    # With |conv| <= 256 (sparse operands, asserted below) rn(conv) = conv, and the result is the fp64 sum rounded once.
    acc_bf16 = row["variant"] == "acc" and row["dtype"] == BF
    if stats or acc_bf16:
        d = R.stats_density(TAPS_PER_OUT[mode] * cin, hout * wout)
        if row["variant"] == "nl":  # the normalised operand is denser and larger than a `signed` one (up to |2 * 4 + 2|)
            d /= 4.0 if row["slope"] == 0.5 else 2.0
        draw = lambda shape: R.signed(shape, g, d)  # noqa: E731
    else:
        draw = lambda shape: R.nonneg(shape, g)  # noqa: E731
    param = draw((cin, nout, k, k) if row["grad"] else (nout, cin, k, k))
    w_nk = param.transpose(0, 1) if row["grad"] else param
    flip = row["grad"] and mode == G3S1
    bias = R.int_bias(nout, g) if row["bias"] else None
    c = dict(row=row, param=param, w_nk=w_nk, flip=flip, bias=bias, hout=hout, wout=wout, out0=None, coefs=None)
    if row["variant"] == "nl":
        slope = row["slope"]
        step = 2 if slope == 0.5 else 1  # even pre-activation values keep slope 0.5 on integers
        y = R.signed((n, cin, hin, win), g, 1.0 if not stats else 0.5) * step
        scale = torch.randint(-2, 3, (n, cin), generator=g).double()
        shift = torch.randint(-1, 2, (n, cin), generator=g).double() * step
        c.update(raw=y, coefs=(scale, shift), x=R.nl_operand(y, scale, shift, slope))
    else:
        c["x"] = draw((n, cin, hin, win))
    x1, x2 = c["x"][:, :c1], (c["x"][:, c1:] if c2 else None)
    y64 = R.conv_ref(mode, x1, x2, w_nk, bias, flip, hw=(hout, wout))
    if row["variant"] == "acc":
        # previous values: bf16-representable integers up to 2040 (multiples of 8), so that the sums are odd, large and need rounding
        c["out0"] = torch.randint(-255, 256, tuple(y64.shape), generator=g).double() * 8
        conv_small = bool(y64.abs().max() <= 256)
        y64 = y64 + c["out0"]
    c.update(x1=x1, x2=x2, y64=y64)
    c["ok"] = R.exact_ok(mode, x1, x2, w_nk, bias, flip, (hout, wout), c["out0"], y64, stats)
    if acc_bf16:
        c["ok"]["|conv| <= 256 (bf16 out += conv)"] = conv_small
    return c


@functools.lru_cache(maxsize=3)
def wgrad_case(name):
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    row = WGRAD_BY_NAME[name]
    g = R.gen(_seed(name))
    mode, n, (hy, wy), c1, c2, cdy = row["mode"], row["n"], row["hw"], row["c1"], row["c2"], row["cdy"]
    hx, wx = (hy, wy) if mode == W3S1 else ((2 * hy - 1, 2 * wy - 1) if mode == W3S2 else (2 * hy, 2 * wy))
    dy = R.nonneg((n, cdy, hy, wy), g)
    c = dict(row=row, dy=dy, coefs=None)
    if row["nl"] is not None:
        step = 2 if row["nl"] == 0.5 else 1
        raw = R.signed((n, c1, hx, wx), g) * step
        scale = torch.randint(-2, 3, (n, c1), generator=g).double()
        shift = torch.randint(-1, 2, (n, c1), generator=g).double() * step
        c.update(raw=raw, coefs=(scale, shift), x=R.nl_operand(raw, scale, shift, row["nl"]))
    else:
        c["x"] = R.nonneg((n, c1 + c2, hx, wx), g)
    x1, x2 = c["x"][:, :c1], (c["x"][:, c1:] if c2 else None)
    c.update(x1=x1, x2=x2, ref=R.wgrad_ref(mode, x1, x2, dy), ok=R.wgrad_exact_ok(mode, x1, x2, dy))
    return c


@functools.lru_cache(maxsize=None)
def stem_case(c0):
    g = R.gen(900 + c0)
    n, h, w = 2, 19, 37
    x = R.nonneg((n, 1, h, w), g)
    wt = R.signed((c0, 1, 3, 3), g)
    b = R.int_bias(c0, g)
    dy = R.signed((n, c0, h, w), g)
    y64 = R.conv_ref(G3S1, x, None, wt, b)
    ok = R.exact_ok(G3S1, x, None, wt, b, y64=y64, stats=True)
    ok.update(R.wgrad_exact_ok(W3S1, x, None, dy))
    return dict(x=x, w=wt, b=b, dy=dy, y64=y64, dw=R.wgrad_ref(W3S1, x, None, dy), ok=ok)


def large_values_ok(c):
    """`nonneg` rows: the reference holds odd |y| above 256 (not representable in bf16: the store must round, to nearest even) and,
    where the K extent allows it at all (mean product ~5.3 per term), values of 2^11 and more."""
    row, y = c["row"], c["y64"].abs()
    terms = TAPS_PER_OUT[row["mode"]] * (row["c1"] + row["c2"])
    if row["variant"] == "acc":  # the previous values carry the magnitude
        terms = 512
    need_odd = terms >= 64 and row["variant"] != "nl"
    need_big = terms >= 512 and row["variant"] != "nl"
    return (not need_odd or bool(((y > 256) & (y % 2 == 1)).any())) and (not need_big or bool((y >= 2048).any()))


def wgrad_large_values_ok(c):
    """Dense `nonneg` rows with at least 512 pixels (mean product ~5.3 each): some |dW| of 2^11 and more."""
    row = c["row"]
    return row["nl"] is not None or row["n"] * row["hw"][0] * row["hw"][1] < 512 or bool((c["ref"].abs() >= 2048).any())


# ------------------------------------------------------------------ GPU side
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _nhwc(x, dtype, dev):
    return x.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev)


def _nchw(t):
    return t.cpu().permute(0, 3, 1, 2)


def _same(got, want, what):
    """Exact equality; on a mismatch the message says where (first indices, count)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        first = [(tuple(i.tolist()), got[tuple(i)].item(), want[tuple(i)].item()) for i in bad[:8]]
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ; first (index, got, want): {first}")


class _Options:
    """Set library options (every one the dispatch depends on) and ops-level gates for one row; restore on exit."""

    def __init__(self, base, opts, split, model=True):
        self.want = dict(base, **opts)
        if split:
            self.want["f32_split"] = split
        self.split, self.model = split, model

    def __enter__(self):
        import mia_hip
        from mia_hip import ops
        self.saved = {k: mia_hip.get_option(k) for k in self.want}
        self.gate, self.kmodel = ops.F32_SPLIT_MIN_MACS, ops.WGRAD_KSPLIT_MODEL
        for k, v in self.want.items():
            mia_hip.set_option(k, v)
        ops.F32_SPLIT_MIN_MACS = 0 if self.split else 1 << 62  # lifted: test-sized launches run the split kernels / never: exact MFMAs
        ops.WGRAD_KSPLIT_MODEL = self.model

    def __exit__(self, *exc):
        import mia_hip
        from mia_hip import ops
        ops.F32_SPLIT_MIN_MACS, ops.WGRAD_KSPLIT_MODEL = self.gate, self.kmodel
        for k, v in self.saved.items():
            mia_hip.set_option(k, v)


def _conv_family(row, npad, kpad, hout, wout, stats):
    import mia_hip
    o1 = row["split_out"] or row["nout"]
    variant = {"plain": mia_hip.CONV_VAR_PLAIN, "nl": mia_hip.CONV_VAR_NL, "acc": mia_hip.CONV_VAR_ACC}[row["variant"]]
    variant |= (mia_hip.CONV_VAR_STATS if stats else 0) | (mia_hip.CONV_VAR_BIAS if row["bias"] else 0)
    return mia_hip.lib().mia_conv_mma_family(row["mode"], mia_hip.BF16 if row["dtype"] == BF else mia_hip.F32, row["c1"], row["c2"], o1,
                                             row["nout"] - o1, npad, kpad, hout, wout, variant, int(bool(row["split"])))


def _run_conv(name, stats):
    import mia_hip
    from mia_hip import ops
    c = conv_case(name, stats)
    row, dtype = c["row"], c["row"]["dtype"]
    assert all(c["ok"].values()), c["ok"]  # preconditions of exactness, on the reference alone
    if not stats:
        assert large_values_ok(c)
    dev = _dev()
    want_fam = row["stats"] if stats else row["fam"]
    hout, wout, nout, mode = c["hout"], c["wout"], row["nout"], row["mode"]
    with _Options(CONV_OPTS, row["opts"], row["split"]):
        wp, npad, kpad = ops.PackCache().get(c["param"].float().to(dev), ops._dt(dtype), not row["grad"])
        fam = _conv_family(row, npad, kpad, hout, wout, stats)
        assert fam == mia_hip.CONV_FAM[want_fam], (name, "dispatches to family", fam, "not", want_fam)
        bias = None if c["bias"] is None else c["bias"].float().to(dev)
        if row["variant"] == "nl":
            raw = _nhwc(c["raw"], dtype, dev)
            coefs = torch.zeros(5, row["n"], row["c1"])
            coefs[2], coefs[3] = c["coefs"][0].float(), c["coefs"][1].float()
            coefs = coefs.to(dev)
            y1, y2, st = ops.conv_mma(mode, raw, None, wp, npad, kpad, False, bias, nout, (hout, wout), want_stats=stats,
                                      nl=(coefs, row["slope"]))
        elif row["variant"] == "acc":
            x1 = _nhwc(c["x1"], dtype, dev)
            y1, y2, st = _nhwc(c["out0"], dtype, dev), None, None
            amw = getattr(wp, "_mia_amax", None) if row["split"] else None
            mia_hip.call("mia_conv_mma_acc", mode, ops._dt(dtype), ops._p(x1), row["c1"], ops._p(wp), npad, kpad, int(c["flip"]), ops._p(y1),
                         nout, row["n"], row["hw"][0], row["hw"][1], hout, wout, ops._p(None if amw is None else ops.amax_slot(x1)),
                         ops._p(None if amw is None else amw[0]), ops._p(None if amw is None else getattr(wp, "_mia_split", None)),
                         ops._stream())
        else:
            x1 = _nhwc(c["x1"], dtype, dev)
            x2 = None if c["x2"] is None else _nhwc(c["x2"], dtype, dev)
            y1, y2, st = ops.conv_mma(mode, x1, x2, wp, npad, kpad, c["flip"], bias, nout, (hout, wout), want_stats=stats,
                                      out_split=row["split_out"])
        torch.cuda.synchronize()
    got = _nchw(y1) if y2 is None else torch.cat([_nchw(y1), _nchw(y2)], 1)
    _same(got, R.expected(c["y64"], dtype), f"{name}: output")
    if stats:
        _same(st.double().sum(1).cpu(), R.stats_ref(c["y64"]), f"{name}: statistics (sum, sum of squares) per (image, channel)")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [r["name"] for r in CONV_ROWS])
def test_conv_family_is_exact_on_integer_operands(name):
    """Dense operands, no statistics: output == fp64 reference rounded once."""
    _run_conv(name, False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [r["name"] for r in CONV_ROWS if r["stats"] is not None])
def test_conv_family_statistics_are_exact_on_integer_operands(name):
    """Sparse signed operands with the statistics epilogue: outputs as above, and the per-(image, channel) sum and sum of squares
    (fp32 partials of integers, added on the host in fp64) equal the fp64 sums exactly -- one pixel counted twice or not at all in
    any tile of any partition changes them."""
    _run_conv(name, True)


@pytest.mark.gpu
@pytest.mark.parametrize("xcd", [1, 0])
@pytest.mark.parametrize("name", [r["name"] for r in WGRAD_ROWS])
def test_wgrad_family_is_exact_on_integer_operands(name, xcd):
    """mia_conv_wgrad (+ _nl) and mia_wgrad_reduce with the split count ops.conv_wgrad picks: dW == fp64 reference (sums of integers
    below 2^24 are exact in any slab order), block order option wgrad_xcd on and off."""
    import mia_hip
    from mia_hip import ops
    c = wgrad_case(name)
    row, dtype = c["row"], c["row"]["dtype"]
    assert all(c["ok"].values()), c["ok"]
    assert wgrad_large_values_ok(c)
    dev = _dev()
    mode, c1, c2, cdy = row["mode"], row["c1"], row["c2"], row["cdy"]
    with _Options(WGRAD_OPTS, dict(row["opts"], wgrad_xcd=xcd), row["split"], row["model"]):
        fam = mia_hip.lib().mia_wgrad_family(mode, ops._dt(dtype), c1, c2, cdy, -(-cdy // 64) * 64, int(row["nl"] is not None),
                                             int(bool(row["split"])))
        assert fam == mia_hip.WGRAD_FAM[row["fam"]], (name, "dispatches to family", fam, "not", row["fam"])
        dy = _nhwc(c["dy"], dtype, dev)
        ks = 2 if mode == W2S2 else 3
        shape = (cdy, c1 + c2, ks, ks)
        if row["nl"] is not None:
            coefs = torch.zeros(5, row["n"], c1)
            coefs[2], coefs[3] = c["coefs"][0].float(), c["coefs"][1].float()
            dw = ops.conv_wgrad(mode, _nhwc(c["raw"], dtype, dev), None, dy, shape, cdy, c1, nl=(coefs.to(dev), row["nl"]))
        else:
            x2 = None if c["x2"] is None else _nhwc(c["x2"], dtype, dev)
            dw = ops.conv_wgrad(mode, _nhwc(c["x1"], dtype, dev), x2, dy, shape, cdy, c1 + c2)
        torch.cuda.synchronize()
    _same(dw.double().cpu(), c["ref"], f"{name}: weight gradient")


@pytest.mark.gpu
@pytest.mark.parametrize("c0,dtype", STEM_ROWS)
def test_stem_is_exact_on_integer_operands(c0, dtype):
    """mia_stem_fwd (MFMA kernel for c0 % 16 == 0, VALU kernel otherwise; fp32 image) with its statistics, and mia_stem_wgrad."""
    from mia_hip import call, lib, ops
    c = stem_case(c0)
    assert all(c["ok"].values()), c["ok"]
    dev = _dev()
    n, _, h, w = c["x"].shape
    xd = c["x"].float().to(dev).reshape(n, h, w, 1)
    wd, bd = c["w"].float().reshape(c0, 9).to(dev).contiguous(), c["b"].float().to(dev)
    y = torch.empty((n, h, w, c0), device=dev, dtype=dtype)
    stats = torch.empty((n, lib().mia_stem_slabs(), c0, 2), device=dev, dtype=torch.float32)
    call("mia_stem_fwd", ops._p(xd), ops._dt(xd), ops._p(wd), ops._p(bd), ops._p(y), ops._dt(y), ops._p(stats), n, h, w, c0, ops._stream())
    dyd = _nhwc(c["dy"], dtype, dev)
    ws = torch.empty(lib().mia_stem_wgrad_workspace(c0), device=dev, dtype=torch.float32)
    dw = torch.empty((c0, 1, 3, 3), device=dev, dtype=torch.float32)
    call("mia_stem_wgrad", ops._p(xd), ops._dt(xd), ops._p(dyd), ops._dt(dyd), ops._p(ws), ops._p(dw), n, h, w, c0, 0, ops._stream())
    torch.cuda.synchronize()
    _same(_nchw(y), R.expected(c["y64"], dtype), "stem output")
    _same(stats.double().sum(1).cpu(), R.stats_ref(c["y64"]), "stem statistics")
    _same(dw.double().cpu(), c["dw"], "stem weight gradient")


PACK_SHAPES = [(96, 96, 3), (40, 96, 3), (96, 40, 2), (3, 40, 1), (40, 3, 3), (16, 16, 3), (16, 16, 1), (128, 64, 2), (3, 3, 2)]


def pack_weights(d0, d1, k):
    """Gaussian weights with exact bf16 ties planted (1 + 2^-8 rounds down to even, 1 + 3 * 2^-8 up) and a value below the tie."""
    w = torch.randn(d0, d1, k, k, generator=R.gen(d0 * 100 + d1 + k))
    flat = w.view(-1)
    flat[0], flat[1], flat[2], flat[3] = 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 - 2.0 ** -20
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("n_from_d0", [True, False])
@pytest.mark.parametrize("shape", PACK_SHAPES)
def test_pack_weight_layout_and_rounding(shape, n_from_d0, dtype):
    """mia_pack_weight against the [tap][npad][kpad] restatement, bit-equal: both orientations, 9 / 4 / 1 taps, padded and unpadded
    channel counts, the tiled path and the small one (npad * kpad < 4096: 16 -> 16 and 3 -> 3, kpad = 32 or 16), round to nearest
    even on planted ties.  fp32: the maximum slot and the split words of mia_split_f16_batch against `split_ref`."""
    from mia_hip import ops
    dev = _dev()
    w = pack_weights(*shape)
    wd = w.to(dev)
    buf, npad, kpad = ops.PackCache().get(wd, ops._dt(dtype), n_from_d0)
    torch.cuda.synchronize()
    want = R.pack_ref(w, dtype, n_from_d0, npad, kpad)
    _same(buf.cpu().view(torch.int16 if dtype == BF else torch.int32), want.view(torch.int16 if dtype == BF else torch.int32), "packed weights")
    if dtype == F32:
        amax = buf._mia_amax[0].cpu().view(torch.float32).item()
        assert amax == w.abs().max().item()
        _same(buf._mia_split.cpu(), R.split_ref(want, amax), "split-f16 words")
