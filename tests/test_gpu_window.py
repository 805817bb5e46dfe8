"""Sliding-window prediction on the GPU (csrc/predict.hip `mia_window_accum` / `mia_window_finalize`, inference/predictor.py):
the kernels against the float64 restatement of tests/_window_ref.py within bounds derived from fp32 rounding, for planar logits and
the head's channels-last view and for every dispatch branch (one pixel or four per thread, mirrored or not, both finalize widths);
untouched pixels, flips, determinism, the single-window case against `ensemble_predict`, and `EnsemblePredictor` end to end on two
small networks."""
import numpy as np
import pytest
import torch

import _predict_ref as R
import _window_ref as WR
from test_window_host import Recorder, run_recorded

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _as_layout(l, layout):
    """l [n,k,h,w] on the device as contiguous NCHW ("nchw"), as the channels-last view the model's head returns ("head"), or as
    planar logits whose class stride is no multiple of 4 ("odd": always the one-pixel branch)."""
    n, k1, h, w = l.shape
    if layout == "head":
        nhwc = torch.empty(n, h, w, k1, device=l.device)
        nhwc.copy_(l.permute(0, 2, 3, 1))
        out = nhwc.permute(0, 3, 1, 2)
        assert out.stride(1) == 1 and out.stride(3) == k1
    elif layout == "odd":
        buf = torch.empty(n, k1, h * w + 1, device=l.device)
        out = buf[:, :, :h * w].view(n, k1, h, w)
        out.copy_(l)
        assert out.stride(1) == h * w + 1
    else:
        out = l.contiguous()
    return out


def _dev_weights(ph, pw, importance, dev):
    from inference import window_weights
    return torch.from_numpy(window_weights(ph, importance)).to(dev), torch.from_numpy(window_weights(pw, importance)).to(dev)


# canvas B, K, H, W; patch; overlap; mirror axes; models.  Dispatch branches (four pixels per thread needs pw, x0, W multiples of 4):
CASES = {
    "x0_unaligned": (2, 3, 40, 52, 16, 24, .5, (2, 3), 3),   # x starts 0/9/19/28: one-pixel branch mirrored and not, 4-wide at x0 = 0, 28
    "odd_width": (1, 2, 27, 31, 16, 16, .5, (3,), 2),        # W = 31: one-pixel accumulate and one-pixel finalize
    "vector": (2, 4, 64, 64, 32, 32, .5, (), 1),             # starts 0/16/32: four-pixel branch, planar and channels-last, not mirrored
    "one_window": (1, 3, 16, 16, 16, 16, .5, (2, 3), 1),     # four-pixel branch with every flip combination
    "five_models": (2, 3, 96, 100, 32, 48, .5, (2, 3), 5),   # x starts 0/17/35/52: both branches mirrored, more than one block
    "eight_classes": (1, 8, 20, 24, 8, 8, .5, (2,), 2),      # K1 = 8
    "one_class": (1, 1, 8, 8, 8, 8, .5, (), 1),              # K1 = 1, one window
}


def _drive(case, layout, dev, seed=0, importance="gaussian"):
    """Every (model, mirror combination, window) as one `window_accum` on a batch slice of one synthetic logits tensor, then
    `window_finalize`: (labels, probs, raw canvas, the logits per forward on the CPU, ys, xs, weights)."""
    from inference import window_accum, window_finalize, window_starts
    from inference.predictor import coverage_1d
    b, k1, h, w, ph, pw, ov, mirror, m = case
    ys, xs = window_starts(h, ph, ov), window_starts(w, pw, ov)
    combos = WR.mirror_combos(mirror)
    weights = [1.0 + 0.5 * i for i in range(m)]
    n = m * len(combos) * len(ys) * len(xs)
    cpu = torch.randn(n * b, k1, ph, pw, generator=torch.Generator().manual_seed(1000 + seed + h * w)) * 4
    logits = _as_layout(cpu.to(dev), layout)
    gy, gx = _dev_weights(ph, pw, importance, dev)
    ry = torch.from_numpy((1.0 / coverage_1d(gy.cpu().numpy(), ys, h)).astype(np.float32)).to(dev)
    rx = torch.from_numpy((1.0 / coverage_1d(gx.cpu().numpy(), xs, w)).astype(np.float32)).to(dev)
    canvas = torch.zeros(b, k1, h, w, device=dev)
    at = 0
    for mi in range(m):
        for combo in combos:
            for y0 in ys:
                for x0 in xs:
                    window_accum(logits[at:at + b], canvas, gy, gx, y0, x0, weights[mi], 2 in combo, 3 in combo)
                    at += b
    raw = canvas.clone()
    pred = torch.full((b, h, w), -7, device=dev, dtype=torch.int64)
    window_finalize(canvas, pred, ry, rx, 1.0 / (len(combos) * sum(weights)), normalise=True)
    return pred, canvas, raw, [cpu], ys, xs, weights


@pytest.mark.parametrize("layout", ["nchw", "head"])
@pytest.mark.parametrize("name", list(CASES))
def test_kernels_match_restatement(name, layout):
    from inference import window_finalize, window_weights
    dev = _dev()
    case = CASES[name]
    b, k1, h, w, ph, pw, ov, mirror, m = case
    pred, probs, raw, rec, ys, xs, weights = _drive(case, layout, dev)
    P, label, gap, T = WR.blend(rec, b, h, w, ys, xs, window_weights(ph), window_weights(pw), m, mirror, weights)
    WR.check(pred, probs, P, label, gap, T, f"{name} {layout}")
    assert torch.equal(pred, raw.argmax(1))  # the labels are those of the raw canvas: taken before any scaling
    # without normalise the canvas is left alone, and pred may be omitted when normalising
    again, pred2 = raw.clone(), torch.empty_like(pred)
    window_finalize(again, pred2)
    assert torch.equal(again, raw) and torch.equal(pred2, pred)


def test_untouched_pixels():
    from inference import window_accum
    dev = _dev()
    for layout in ("nchw", "head"):
        for (h, w, ph, pw, y0, x0) in [(32, 40, 16, 24, 8, 12), (27, 31, 16, 15, 5, 7), (32, 40, 16, 24, 16, 16), (16, 24, 16, 24, 0, 0)]:
            logits = _as_layout((torch.randn(2, 3, ph, pw, generator=torch.Generator().manual_seed(1)) * 4).to(dev), layout)
            gy, gx = _dev_weights(ph, pw, "gaussian", dev)
            canvas = torch.full((2, 3, h, w), 7.0, device=dev)
            window_accum(logits, canvas, gy, gx, y0, x0, 1.5, True, True)
            inside = torch.zeros(h, w, dtype=torch.bool, device=dev)
            inside[y0:y0 + ph, x0:x0 + pw] = True
            assert (canvas[:, :, ~inside] == 7.0).all()
            want = 7.0 + 1.5 * (gy[:, None] * gx[None, :]) * logits.softmax(1).flip((2, 3))
            assert (canvas[:, :, y0:y0 + ph, x0:x0 + pw] - want).abs().max().item() < 2e-6  # one ulp of 8.5 and the softmax


@pytest.mark.parametrize("layout", ["nchw", "head", "odd"])
@pytest.mark.parametrize("flip_h,flip_w", [(False, False), (True, False), (False, True), (True, True)])
def test_flips_and_branches_are_bit_equal(flip_h, flip_w, layout):
    """Accumulating `logits` with the flags bit-equals accumulating the flipped logits without them, whatever layout and branch:
    a 4-aligned window (four pixels per thread for "nchw" and "head", one for "odd"), the same window at an unaligned x0, and a
    window of odd width."""
    from inference import window_accum
    dev = _dev()
    dims = [d for d, f in ((2, flip_h), (3, flip_w)) if f]
    for (h, w, ph, pw, y0, x0) in [(32, 40, 16, 24, 8, 12), (32, 40, 16, 24, 8, 13), (27, 31, 16, 15, 5, 7)]:
        g = torch.Generator().manual_seed(h + x0)
        plain = (torch.randn(2, 3, ph, pw, generator=g) * 4).to(dev)
        start = torch.randn(2, 3, h, w, generator=g).to(dev)
        gy, gx = _dev_weights(ph, pw, "gaussian", dev)
        got, want = start.clone(), start.clone()
        window_accum(_as_layout(plain, layout), got, gy, gx, y0, x0, 1.25, flip_h, flip_w)
        flipped = plain.flip(dims).contiguous() if dims else plain
        window_accum(_as_layout(flipped, "odd"), want, gy, gx, y0, x0, 1.25, False, False)  # the one-pixel branch, not mirrored
        assert torch.equal(got, want), (layout, flip_h, flip_w, h, w, x0, int((got != want).sum()))
        assert not torch.equal(got, start)


def test_finalize_widths_are_bit_equal():
    """The four-pixel finalize (W a multiple of 4) and the one-pixel finalize (an unaligned view of the same values) agree in bits."""
    from inference import window_finalize
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    vals = torch.rand(2, 3, 12, 20, generator=g).to(dev)
    vals[0, 1, 3] = vals[0, 2, 3]  # ties between classes 1 and 2
    ry, rx = torch.rand(12, generator=g).to(dev) + 0.5, torch.rand(20, generator=g).to(dev) + 0.5
    a, pa = vals.clone(), torch.empty(2, 12, 20, device=dev, dtype=torch.int64)
    window_finalize(a, pa, ry, rx, 0.3, normalise=True)
    store = torch.empty(vals.numel() + 1, device=dev)  # the same canvas one float off 16-byte alignment
    c = store[1:].view(2, 3, 12, 20)
    c.copy_(vals)
    pc = torch.empty_like(pa)
    window_finalize(c, pc, ry, rx, 0.3, normalise=True)
    assert torch.equal(a, c) and torch.equal(pa, pc) and torch.equal(pa, vals.argmax(1))
    assert torch.equal(a, vals * ((0.3 * ry)[:, None] * rx[None, :]))


def test_determinism_and_window_batch():
    from inference import window_starts, window_weights
    dev = _dev()
    for layout in ("nchw", "head"):
        one = _drive(CASES["x0_unaligned"], layout, dev)
        two = _drive(CASES["x0_unaligned"], layout, dev)
        assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
    x = torch.randn(2, 2, 40, 52, generator=torch.Generator().manual_seed(5)).to(dev)
    models = [Recorder(3, 2, 16, 24, 20 + i).to(dev) for i in range(2)]
    kw = dict(mirror_axes=(2, 3), weights=[1.0, 1.5])
    base = run_recorded(models, x, (16, 24), window_batch=1, **kw)
    assert base[0].is_cuda and base[1].is_cuda
    for wb in (1, 3, 16):
        labels, probs, rec = run_recorded(models, x, (16, 24), window_batch=wb, **kw)
        assert torch.equal(labels, base[0]) and torch.equal(probs, base[1]), wb
    ys, xs = window_starts(40, 16, .5), window_starts(52, 24, .5)
    P, label, gap, T = WR.blend(base[2], 2, 40, 52, ys, xs, window_weights(16), window_weights(24), 2, (2, 3), [1.0, 1.5])
    WR.check(base[0], base[1], P, label, gap, T, "recorder on the device")
    # the patches the network saw are those of the CPU path: FH.crop and FH.rot90_flip against slicing and flip
    cpu_models = [Recorder(3, 2, 16, 24, 20 + i) for i in range(2)]
    run_recorded(cpu_models, x.cpu(), (16, 24), window_batch=3, **kw)
    run_recorded(models, x, (16, 24), window_batch=3, **kw)
    assert all(torch.equal(a.cpu(), c) for a, c in zip(models[0].inputs, cpu_models[0].inputs))


class _Fixed(torch.nn.Module):
    def __init__(self, logits):
        super().__init__()
        self.logits = logits

    def forward(self, x):
        return self.logits


def test_single_window_equals_ensemble_predict():
    from inference import ensemble_predict, sliding_window_predict
    dev = _dev()
    for layout in ("nchw", "head"):
        for (b, k1, h, w) in [(2, 3, 64, 72), (1, 4, 33, 35)]:
            g = torch.Generator().manual_seed(h)
            logits = [_as_layout((torch.randn(b, k1, h, w, generator=g) * 4).to(dev), layout) for _ in range(3)]
            models, weights = [_Fixed(l) for l in logits], [1.0, 0.5, 2.0]
            x = torch.zeros(b, 1, h, w, device=dev)
            got = sliding_window_predict(models, x, (h, w), importance="constant", weights=weights)
            want = ensemble_predict(models, x, weights)
            _, label, gap = R.ensemble(logits, weights)
            decided = gap >= R.GAP_BOUND * sum(weights)
            share = 1.0 - decided.double().mean().item()
            print(f"{layout} {b}x{k1}x{h}x{w}: {int((got != want).sum())} pixels differ, undecided share {share:.3e}")
            assert share < R.MAX_UNDECIDED
            assert torch.equal(got.cpu()[decided], want.cpu()[decided]) and torch.equal(got.cpu()[decided], label[decided])


def test_ensemble_predictor_end_to_end():
    from inference import EnsemblePredictor, ensemble_predict, sliding_window_predict, window_starts, window_weights
    from mia_hip import ops
    dev = _dev()
    tiled = EnsemblePredictor(None, folds=(0, 1), channels_list=[16, 32, 64], device=dev, patch_size=(64, 64), mirror_axes=(2, 3),
                              window_batch=3)
    for i, net in enumerate(tiled.models):  # two differently seeded networks
        torch.manual_seed(40 + i)
        net.load_state_dict(type(net)(2, 3, 3, [16, 32, 64]).state_dict())
    ops.bump_param_epoch()
    rec = []
    hooks = [net.register_forward_hook(lambda mod, inp, out: rec.append((out[0] if isinstance(out, (list, tuple)) else out).detach().float().clone()))
             for net in tiled.models]
    X = torch.rand(2, 3, 96, 112, generator=torch.Generator().manual_seed(3)) * 255.0
    raw = tiled.predict_batch(X, do_denoise=False)
    assert raw.shape == (2, 96, 112) and raw.dtype == torch.int64 and raw.is_cuda
    ys, xs = window_starts(96, 64, .5), window_starts(112, 64, .5)
    assert (ys, xs) == ([0, 32], [0, 24, 48]) and len(rec) == 2 * 4 * 2 and rec[0].shape == (6, 3, 64, 64)
    P, label, gap, T = WR.blend(rec, 2, 96, 112, ys, xs, window_weights(64), window_weights(64), 2, (2, 3))
    x = tiled.preprocess(X)
    assert x.shape == (2, 3, 96, 112)
    labels, probs = sliding_window_predict(tiled.models, x, (64, 64), mirror_axes=(2, 3), window_batch=3, return_probs=True)
    assert torch.equal(labels, raw)
    WR.check(labels, probs, P, label, gap, T, "two UNets, 96x112, 64x64 windows, both mirror axes")
    out = tiled.predict_batch(X)
    assert torch.equal(out, tiled.processor.denoise_masks(raw, backend="tensor"))
    assert not any(net.training for net in tiled.models)
    # without a patch size the predictor returns exactly what it returned before: ensemble_predict on the preprocessed batch
    for hk in hooks:
        hk.remove()
    plain = EnsemblePredictor(None, folds=(0, 1), channels_list=[16, 32, 64], device=dev)
    plain.models = tiled.models
    want = plain.processor.postprocess(ensemble_predict(plain.models, plain.preprocess(X), None), (96, 112))
    assert torch.equal(plain.predict_batch(X, do_denoise=False), want)
    sized = EnsemblePredictor((96, 112), folds=(0, 1), channels_list=[16, 32, 64], device=dev)
    sized.models = tiled.models
    assert torch.equal(sized.predict_batch(X, do_denoise=False), want)


def test_argument_checks():
    import mia_hip
    from inference import window_accum, window_finalize
    dev = _dev()
    gy, gx = _dev_weights(4, 4, "gaussian", dev)
    l, canvas = torch.zeros(1, 3, 4, 4, device=dev), torch.zeros(1, 3, 8, 8, device=dev)
    with pytest.raises(mia_hip.MiaError):  # k1 = 9
        window_accum(torch.zeros(1, 9, 4, 4, device=dev), torch.zeros(1, 9, 8, 8, device=dev), gy, gx, 0, 0)
    with pytest.raises(mia_hip.MiaError):
        window_finalize(torch.zeros(1, 9, 8, 8, device=dev), torch.zeros(1, 8, 8, device=dev, dtype=torch.int64))
    for y0, x0 in [(5, 0), (0, 5), (-1, 0), (0, -1), (8, 8)]:  # a window that crosses the canvas edge is refused, not clipped
        with pytest.raises(mia_hip.MiaError, match="does not lie inside"):
            window_accum(l, canvas, gy, gx, y0, x0)
    with pytest.raises(ValueError):  # gy of the wrong length
        window_accum(l, canvas, torch.ones(5, device=dev), gx, 0, 0)
    with pytest.raises(ValueError):
        window_accum(l, canvas, gy, gx.double(), 0, 0)
    with pytest.raises(ValueError):  # canvas not contiguous
        window_accum(l, torch.zeros(1, 3, 8, 16, device=dev)[..., ::2], gy, gx, 0, 0)
    with pytest.raises(ValueError):
        window_accum(l, torch.zeros(1, 2, 8, 8, device=dev), gy, gx, 0, 0)
    with pytest.raises(ValueError):
        window_finalize(torch.zeros(1, 3, 8, 16, device=dev)[..., ::2], None, None, None, 1.0, False)
    with pytest.raises(ValueError):
        window_finalize(canvas, torch.zeros(1, 8, 8, device=dev, dtype=torch.int32))
    with pytest.raises(ValueError):
        window_finalize(canvas, None, torch.ones(7, device=dev), torch.ones(8, device=dev), 1.0, True)
    with pytest.raises(mia_hip.MiaError):  # nothing to do
        window_finalize(canvas)
    assert (canvas == 0).all()
    with pytest.raises(mia_hip.MiaError):  # CPU tensors never reach the kernels
        window_accum(l.cpu(), canvas.cpu(), gy.cpu(), gx.cpu(), 0, 0)
    with pytest.raises(mia_hip.MiaError):
        window_accum(l, canvas, gy.cpu(), gx, 0, 0)
    with pytest.raises(mia_hip.MiaError):
        window_finalize(canvas.cpu(), torch.zeros(1, 8, 8, dtype=torch.int64))
