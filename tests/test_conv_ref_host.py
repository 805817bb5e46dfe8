"""CPU checks of the bit-exact conv probe (tests/_conv_ref.py, tests/test_gpu_conv_exact.py): the fp64 restatement against torch's
own fp32 convs and autograd, the exactness preconditions of EVERY row of the GPU file's case tables, the kernel family every row
must reach (the library's dispatch queries launch nothing, so they run here), and four planted faults that the exact comparison
must reject -- with a report of whether the tolerance metric of tests/test_gpu_ops.py would have accepted them."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _conv_ref as R
import test_gpu_conv_exact as X


def relerr(got, ref):  # the metric of tests/test_gpu_ops.py
    return ((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-12)).item()


# ------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("c1,c2", [(5, 0), (3, 4)])
def test_restatement_matches_fp32_autograd_for_every_mode(c1, c2):
    g = R.gen(7 + c2)
    n, cin, cout, h, w = 2, c1 + c2, 6, 9, 11
    x = torch.randn(n, cin, h, w, generator=g)
    x1, x2 = x[:, :c1], (x[:, c1:] if c2 else None)
    close = lambda a, b: torch.allclose(a.float(), b, rtol=1e-4, atol=1e-4)  # noqa: E731  (fp32 torch against the fp64 restatement)
    for stride, fwd, bwd, wg in ((1, R.G3S1, R.G3S1, R.W3S1), (2, R.G3S2, R.T3S2, R.W3S2)):
        wt = torch.randn(cout, cin, 3, 3, generator=g)
        b = torch.randn(cout, generator=g)
        xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
        yr = F.conv2d(xr, wr, b, stride=stride, padding=1)
        dy = torch.randn(yr.shape, generator=g)
        yr.backward(dy)
        assert close(R.conv_ref(fwd, x1, x2, wt, b), yr.detach())
        assert close(R.conv_ref(bwd, dy, None, wt.transpose(0, 1), None, flip=(stride == 1), hw=(h, w)), xr.grad)
        assert close(R.wgrad_ref(wg, x1, x2, dy), wr.grad)
        assert close(R.stats_ref(yr.detach().double())[..., 1], (yr.detach() ** 2).sum((2, 3)))
    # ConvTranspose2d 2x2 / stride 2: forward T2S2, input gradient G2S2, weight gradient W2S2 (x := grad_output, dy := input)
    wt = torch.randn(cin, cout, 2, 2, generator=g)
    b = torch.randn(cout, generator=g)
    xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    yr = F.conv_transpose2d(xr, wr, b, stride=2)
    dy = torch.randn(yr.shape, generator=g)
    yr.backward(dy)
    assert close(R.conv_ref(R.T2S2, x1, x2, wt.transpose(0, 1), b), yr.detach())
    assert close(R.conv_ref(R.G2S2, dy, None, wt), xr.grad)
    assert close(R.wgrad_ref(R.W2S2, dy, None, x), wr.grad)
    # 1x1 and its input gradient
    wt = torch.randn(cout, cin, 1, 1, generator=g)
    xr = x.clone().requires_grad_(True)
    yr = F.conv2d(xr, wt, b)
    dy = torch.randn(yr.shape, generator=g)
    yr.backward(dy)
    assert close(R.conv_ref(R.G1, x1, x2, wt, b), yr.detach())
    assert close(R.conv_ref(R.G1, dy, None, wt.transpose(0, 1)), xr.grad)
    # accumulating form and the normalise-on-load operand
    out0 = torch.randn(n, cin, h, w, generator=g)
    assert close(R.conv_acc_ref(R.G3S1, out0, dy, wt.new_zeros(cin, cout, 3, 3)), out0)
    sc, sh = torch.randn(n, cin, generator=g), torch.randn(n, cin, generator=g)
    assert close(R.nl_operand(x, sc, sh, 0.25), F.leaky_relu(sc[:, :, None, None] * x + sh[:, :, None, None], 0.25))


def test_expected_rounds_once_to_nearest_even():
    y = torch.tensor([257.0, 259.0, 258.0, -257.0, 2049.0 * 4 + 16, 3.0], dtype=torch.float64)
    assert R.expected(y, torch.bfloat16).double().tolist() == [256.0, 260.0, 258.0, -256.0, 8192.0, 3.0]
    assert torch.equal(R.expected(y, torch.float32).double(), y)


def test_pack_and_split_restatements():
    w = torch.arange(2 * 3 * 4, dtype=torch.float32).reshape(2, 3, 2, 2)
    p = R.pack_ref(w, torch.float32, True, 64, 16)
    assert p.shape == (4, 64, 16) and p[3, 1, 2] == w[1, 2, 1, 1] and p[:, 2:].abs().sum() == 0 and p[:, :, 3:].abs().sum() == 0
    p = R.pack_ref(w, torch.float32, False, 64, 16)
    assert p[2, 2, 1] == w[1, 2, 1, 0] and p[:, 3:].abs().sum() == 0
    assert R.split_exp(3.0) == 13 and R.split_exp(0.0) == 120 and R.split_exp(2.0 ** 14) == 0
    x = torch.tensor([3.0, 1.0 + 2.0 ** -12, -0.75, 0.0])
    words = R.split_ref(x, 3.0).numpy().view("uint32")
    import numpy as np
    h = (words & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float64)
    l = (words >> 16).astype(np.uint16).view(np.float16).astype(np.float64)
    assert ((h + l) * 2.0 ** -13 == x.double().numpy()).all() and l[1] != 0


# ------------------------------------------------------------------ every row of the GPU file's tables
@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("name", [r["name"] for r in X.CONV_ROWS])
def test_conv_rows_meet_the_exactness_preconditions(name, stats):
    if stats and X.CONV_BY_NAME[name]["stats"] is None:
        return
    c = X.conv_case(name, stats)
    assert all(c["ok"].values()), c["ok"]
    if not stats:
        assert X.large_values_ok(c)
    else:  # a statistics case that is all zeros would prove nothing
        assert (c["y64"] != 0).double().mean() > 0.5


@pytest.mark.parametrize("name", [r["name"] for r in X.WGRAD_ROWS])
def test_wgrad_rows_meet_the_exactness_preconditions(name):
    c = X.wgrad_case(name)
    assert all(c["ok"].values()), c["ok"]
    assert X.wgrad_large_values_ok(c)
    assert (c["ref"] != 0).double().mean() > 0.5


def test_stem_rows_meet_the_exactness_preconditions():
    for c0, _ in X.STEM_ROWS:
        assert all(X.stem_case(c0)["ok"].values())


def test_every_family_is_the_asserted_family_of_some_row():
    import mia_hip
    conv = {r["fam"] for r in X.CONV_ROWS} | {r["stats"] for r in X.CONV_ROWS if r["stats"]}
    assert conv == set(mia_hip.CONV_FAM), set(mia_hip.CONV_FAM) ^ conv
    wg = {r["fam"] for r in X.WGRAD_ROWS}
    assert wg == set(mia_hip.WGRAD_FAM), set(mia_hip.WGRAD_FAM) ^ wg
    d = mia_hip.parse_defines()
    assert {f"MIA_CONV_FAM_{k}": v for k, v in mia_hip.CONV_FAM.items()} == {k: v for k, v in d.items() if k.startswith("MIA_CONV_FAM_")}
    assert {f"MIA_WGRAD_FAM_{k}": v for k, v in mia_hip.WGRAD_FAM.items()} == {k: v for k, v in d.items() if k.startswith("MIA_WGRAD_FAM_")}
    assert (d["MIA_CONV_VAR_STATS"], d["MIA_CONV_VAR_BIAS"]) == (mia_hip.CONV_VAR_STATS, mia_hip.CONV_VAR_BIAS)


def _with_options(base, opts, split):
    import contextlib
    import mia_hip

    @contextlib.contextmanager
    def cm():
        want = dict(base, **opts)
        if split:
            want["f32_split"] = split
        saved = {k: mia_hip.get_option(k) for k in want}
        try:
            for k, v in want.items():
                mia_hip.set_option(k, v)
            yield
        finally:
            for k, v in saved.items():
                mia_hip.set_option(k, v)
    return cm()


def test_every_row_dispatches_to_its_family():
    """The dispatch queries are pure host code: the family of every row, with and without statistics, is checked here too."""
    import __graft_entry__ as ge
    import mia_hip
    ge.build()
    pad = lambda v, m: -(-v // m) * m  # noqa: E731
    for r in X.CONV_ROWS:
        hout, wout = R.out_hw(r["mode"], *r["hw"], r["odd"])
        npad, kpad = pad(r["nout"], 64), pad(r["c1"] + r["c2"], 32 if r["dtype"] == X.BF else 16)
        with _with_options(X.CONV_OPTS, r["opts"], r["split"]):
            assert X._conv_family(r, npad, kpad, hout, wout, False) == mia_hip.CONV_FAM[r["fam"]], r["name"]
            if r["stats"]:
                assert X._conv_family(r, npad, kpad, hout, wout, True) == mia_hip.CONV_FAM[r["stats"]], (r["name"], "with statistics")
    for r in X.WGRAD_ROWS:
        with _with_options(X.WGRAD_OPTS, r["opts"], r["split"]):
            fam = mia_hip.lib().mia_wgrad_family(r["mode"], mia_hip.BF16 if r["dtype"] == X.BF else mia_hip.F32, r["c1"], r["c2"], r["cdy"],
                                                 pad(r["cdy"], 64), int(r["nl"] is not None), int(bool(r["split"])))
            assert fam == mia_hip.WGRAD_FAM[r["fam"]], r["name"]
    # shapes a variant rejects come back as a negative code
    lib = mia_hip.lib()
    assert lib.mia_conv_mma_family(R.G3S1, mia_hip.BF16, 128, 0, 128, 0, 128, 128, 19, 37, mia_hip.CONV_VAR_NL, 0) < 0
    assert lib.mia_conv_mma_family(R.T3S2, mia_hip.BF16, 40, 0, 32, 0, 64, 64, 19, 37, mia_hip.CONV_VAR_ACC, 0) < 0
    assert lib.mia_wgrad_family(R.W3S2, mia_hip.BF16, 64, 0, 64, 64, 1, 0) < 0
    # the transposed modes have no statistics epilogue (their four parity classes would share one entry per tile): an argument error
    some = ctypes.c_void_p(64)  # (rejected before any pointer is looked at)
    for mode in (R.T3S2, R.T2S2):
        rc = lib.mia_conv_mma(mode, mia_hip.BF16, None, 0, None, 0, None, 0, 0, 0, None, None, 0, None, 0, some, 1, 1, 1, 1, 1, None, None, None,
                              None, None, None, None)
        assert rc < 0 and b"statistics" in lib.mia_last_error()


# ------------------------------------------------------------------ planted faults
def _trunc_bf16(y64):
    bits = y64.float().view(torch.int32) & -65536
    return bits.view(torch.float32).to(torch.bfloat16)


def test_planted_faults_are_rejected_by_the_exact_comparison(capsys):
    """Each fault is applied to the REFERENCE output on the CPU; the exact comparison must reject it.  Whether the tolerance metric of
    tests/test_gpu_ops.py (max|got - ref| / max|ref| against 2e-2 for bf16 outputs, 1e-3 + 2e-2 for statistics) would have accepted
    it is printed: a measurement of the old suite (recorded in DESIGN.md), not an acceptance number."""
    bf = torch.bfloat16
    lines = []

    def report(what, got, want, bar):
        assert not torch.equal(got, want), what
        e = relerr(got, want)
        lines.append(f"planted fault: {what}: exact comparison rejects: yes; old metric {e:.2e} against {bar:.1e} accepts: "
                     f"{'yes' if e < bar else 'no'}")

    # 1. one K-element dropped for one corner pixel at cin = 512 (sparse operands: every |y| <= 256 is a bf16 value, so any change shows)
    c = X.conv_case("g3s1_fast_512", True)
    x, w = c["x"], c["w_nk"]
    k, o = next((k, o) for k in range(512) for o in range(32) if x[0, k, 0, 0] * w[o, k, 1, 1] != 0)
    bad = c["y64"].clone()
    bad[0, o, 0, 0] -= x[0, k, 0, 0] * w[o, k, 1, 1]
    report("one K-element dropped at a corner pixel, cin = 512", R.expected(bad, bf), R.expected(c["y64"], bf), 2e-2)
    # 2. one pixel added twice to one statistics entry
    c = X.conv_case("g3s1_conv64", True)
    y = c["y64"]
    py, px = next((i, j) for i in range(y.shape[2]) for j in range(y.shape[3]) if y[1, 5, i, j] != 0)
    st = R.stats_ref(y)
    bad = st.clone()
    bad[1, 5, 0] += y[1, 5, py, px]
    bad[1, 5, 1] += y[1, 5, py, px] ** 2
    report("one pixel counted twice in one statistics entry", bad, st, 1e-3 + 2e-2)
    # 3. truncation instead of round-to-nearest-even on the bf16 store (dense operands: odd values above 256)
    c = X.conv_case("g3s1_fast", False)
    report("bf16 store truncates", _trunc_bf16(c["y64"]), R.expected(c["y64"], bf), 2e-2)
    # 4. the accumulator rounded to bf16 between 32-channel chunks (128 channels: four chunks)
    acc = torch.zeros_like(c["y64"])
    for k0 in range(0, 128, 32):
        part = R.conv_ref(R.G3S1, c["x"][:, k0:k0 + 32], None, c["w_nk"][:, k0:k0 + 32], c["bias"] if k0 == 0 else None)
        acc = (acc + part).float().to(bf).double()
    report("accumulator rounded to bf16 between 32-channel chunks", acc.to(bf), R.expected(c["y64"], bf), 2e-2)
    with capsys.disabled():
        print()
        for l in lines:
            print(l)
    assert len(lines) == 4
