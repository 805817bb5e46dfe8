"""CPU checks of sliding-window prediction (inference/predictor.py): the window grid and the importance weights against known
answers, the separable normalisation against the brute-force coverage, the float64 restatement of tests/_window_ref.py against a
hand-computed case, and `sliding_window_predict` on CPU tensors against that restatement fed with the logits a recording stand-in
network returned -- none of it needs a GPU."""
import math
import os

import numpy as np
import pytest
import torch

import _window_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Recorder(torch.nn.Module):
    """A stand-in network whose logits depend on the input and on the patch-local position, `A . x + R[k, i, j]` with a fixed
    random R: a wrong flip-back or a wrong window offset changes the answer.  Records inputs, outputs and the mode of every call."""

    def __init__(self, k1, c, ph, pw, seed, fail_at=None):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.register_buffer("A", torch.randn(k1, c, generator=g) * 3)
        self.register_buffer("R", torch.randn(k1, ph, pw, generator=g) * 4)
        self.fail_at, self.inputs, self.outputs, self.seen = fail_at, [], [], []

    def forward(self, x):
        self.seen.append(self.training)
        if self.fail_at is not None and len(self.seen) > self.fail_at:
            raise RuntimeError("boom")
        out = torch.einsum("kc,nchw->nkhw", self.A, x) + self.R[None]
        self.inputs.append(x.detach().clone())
        self.outputs.append(out.detach().clone())
        return out


def run_recorded(models, x, patch, **kw):
    """(labels, probs, recorded logits of every forward in call order)."""
    from inference import sliding_window_predict
    for m in models:
        m.inputs.clear(), m.outputs.clear(), m.seen.clear()
    labels, probs = sliding_window_predict(models, x, patch, return_probs=True, **kw)
    return labels, probs, [o for m in models for o in m.outputs]


@pytest.mark.parametrize("args,want", [((40, 16, .5), [0, 8, 16, 24]), ((52, 24, .5), [0, 9, 19, 28]), ((27, 16, .5), [0, 6, 11]),
                                       ((31, 16, .5), [0, 8, 15]), ((66, 32, .25), [0, 17, 34]), ((96, 32, .5), [0, 16, 32, 48, 64]),
                                       ((16, 16, .5), [0])])
def test_window_starts_known_answers(args, want):
    from inference import window_starts
    got = window_starts(*args)
    assert got == want and all(isinstance(v, int) for v in got)
    assert got[0] == 0 and got[-1] == args[0] - args[1]


def test_window_starts_properties_and_errors():
    from inference import window_starts
    for n, p, ov in [(100, 48, .5), (1400, 512, .5), (1024, 512, .5), (33, 32, 0.0), (97, 13, .75), (20, 8, .5), (24, 8, 0.0)]:
        s = window_starts(n, p, ov)
        assert s[0] == 0 and s[-1] == n - p and s == sorted(set(s))
        assert max(b - a for a, b in zip(s, s[1:])) <= math.ceil(p * (1 - ov))  # neighbours overlap by at least `overlap`
    assert window_starts(1024, 512, .5) == [0, 256, 512] and window_starts(24, 8, 0.0) == [0, 8, 16]
    for bad in [(15, 16, .5), (32, 16, 1.0), (32, 16, -0.1), (32, 0, .5)]:
        with pytest.raises(ValueError):
            window_starts(*bad)


def test_window_weights():
    from inference import window_weights
    for p in (1, 2, 7, 8, 16, 24, 33, 512):
        g = window_weights(p)
        assert g.dtype == np.float32 and g.shape == (p,)
        assert np.array_equal(g, g[::-1])                                   # symmetric
        assert g.max() == g[(p - 1) // 2] == g[p // 2]                      # the maximum sits at the centre (pair)
        if p % 2:
            assert g[p // 2] == 1.0
        else:
            assert g[p // 2] == np.float32(math.exp(-0.5 * (0.5 / (p * 0.125)) ** 2))
        assert g[0] == np.float32(math.exp(-0.5 * (((p - 1) / 2) / (p * 0.125)) ** 2))  # closed-form end value
        assert np.all(np.diff(g[: p // 2 + 1]) >= 0)
    assert window_weights(9, sigma_scale=0.25)[0] == np.float32(math.exp(-0.5 * (4 / 2.25) ** 2))
    c = window_weights(5, "constant")
    assert c.dtype == np.float32 and np.array_equal(c, np.ones(5, np.float32))
    with pytest.raises(ValueError):
        window_weights(5, "triangle")


@pytest.mark.parametrize("h,w,ph,pw,ov", [(40, 52, 16, 24, .5), (27, 31, 16, 16, .5), (66, 40, 32, 16, .25), (16, 16, 16, 16, .5)])
def test_separable_normalisation_matches_brute_force_coverage(h, w, ph, pw, ov):
    from inference import window_starts, window_weights
    from inference.predictor import coverage_1d
    ys, xs = window_starts(h, ph, ov), window_starts(w, pw, ov)
    gy, gx = window_weights(ph), window_weights(pw)
    cov = np.zeros((h, w), dtype=np.float64)
    g2 = gy.astype(np.float64)[:, None] * gx.astype(np.float64)[None, :]
    for y0 in ys:
        for x0 in xs:
            cov[y0:y0 + ph, x0:x0 + pw] += g2
    sep = coverage_1d(gy, ys, h)[:, None] * coverage_1d(gx, xs, w)[None, :]
    assert sep.dtype == np.float64 and cov.min() > 0
    assert np.abs(sep / cov - 1).max() < 1e-14


def test_restatement_hand_computed():
    ln = math.log
    # one image of 1 x 3 pixels, two classes, windows of 1 x 2 at x0 = 0 and 1, weights gy = [1], gx = [1, 3];
    # softmax(log a, log b) = (a, b) / (a + b); the records are fp32, so log 3 carries a rounding of 6e-8 and the answers 1e-7
    tol = dict(atol=1e-7, rtol=0)
    w0 = torch.tensor([[[[ln(3.0), 0.0]], [[ln(1.0), 0.0]]]])        # pixels (.75, .25), (.5, .5)
    w1 = torch.tensor([[[[ln(1.0), 0.0]], [[ln(3.0), 0.0]]]])        # pixels (.25, .75), (.5, .5)
    P, label, gap, T = WR.blend([w0, w1], 1, 1, 3, [0], [0, 1], [1.0], [1.0, 3.0], 1)
    # x = 0: (.75, .25) / 1; x = 1: (3 (.5, .5) + (.25, .75)) / 4; x = 2: 3 (.5, .5) / 3 -- an exact tie goes to class 0
    want = torch.tensor([[[[0.75, 0.4375, 0.5]], [[0.25, 0.5625, 0.5]]]], dtype=torch.float64)
    assert torch.allclose(P, want, **tol) and T == 2
    assert label.tolist() == [[[0, 1, 0]]]
    assert torch.allclose(gap, torch.tensor([[[0.5, 0.125, 0.0]]], dtype=torch.float64), **tol)
    # the same with the W axis mirrored: the logits of a mirrored pass belong to the mirrored patch and are flipped back
    w0m = torch.tensor([[[[0.0, ln(1.0)]], [[0.0, ln(3.0)]]]])       # flipped back: x = 0 gets (.25, .75), x = 1 gets (.5, .5)
    w1m = torch.zeros(1, 2, 1, 2)                                    # (.5, .5) twice
    P, label, gap, T = WR.blend([torch.cat([w0, w1]), torch.cat([w0m, w1m])], 1, 1, 3, [0], [0, 1], [1.0], [1.0, 3.0], 1, (3,))
    # x = 0: ((.75, .25) + (.25, .75)) / 2; x = 1: ((1.75, 2.25) + 3 (.5, .5) + (.5, .5)) / 8; x = 2: 6 (.5, .5) / 6
    want = torch.tensor([[[[0.5, 0.46875, 0.5]], [[0.5, 0.53125, 0.5]]]], dtype=torch.float64)
    assert torch.allclose(P, want, **tol) and T == 4
    assert label.tolist() == [[[0, 1, 0]]]
    # two models with weights 1 and 3: P = (P_a + 3 P_b) / 4 where both see the same windows
    P2, _, _, T2 = WR.blend([w0, w1, w1, w0], 1, 1, 3, [0], [0, 1], [1.0], [1.0, 3.0], 2, (), [1.0, 3.0])
    assert T2 == 4 and torch.allclose(P2[0, :, 0, 0], torch.tensor([0.375, 0.625], dtype=torch.float64), **tol)
    assert WR.mirror_combos((3, 2)) == [(), (3,), (2,), (3, 2)] and WR.mirror_combos(()) == [()]


CPU_CASES = [  # b, c, k1, h, w, ph, pw, overlap, mirror, models
    (2, 2, 3, 40, 52, 16, 24, .5, (2, 3), 3),
    (1, 1, 2, 27, 31, 16, 16, .5, (3,), 2),
    (2, 3, 4, 64, 64, 32, 32, .5, (), 1),
    (1, 2, 3, 16, 16, 16, 16, .5, (3, 2), 1),
    (1, 1, 1, 20, 24, 8, 8, .25, (2,), 2),
]


@pytest.mark.parametrize("case", CPU_CASES)
def test_sliding_window_cpu_matches_restatement(case):
    from inference import window_starts, window_weights
    b, c, k1, h, w, ph, pw, ov, mirror, m = case
    g = torch.Generator().manual_seed(h * w + m)
    x = torch.randn(b, c, h, w, generator=g)
    models = [Recorder(k1, c, ph, pw, 10 + i) for i in range(m)]
    for i, mod in enumerate(models):
        mod.train(i % 2 == 0)
    weights = [1.0 + 0.5 * i for i in range(m)]
    labels, probs, rec = run_recorded(models, x, (ph, pw), overlap=ov, mirror_axes=mirror, weights=weights)
    ys, xs = window_starts(h, ph, ov), window_starts(w, pw, ov)
    assert len(rec) == m * len(WR.mirror_combos(mirror)) * len(ys) * len(xs)
    # the network saw the windows of x row-major, and the mirrored windows afterwards
    assert torch.equal(models[0].inputs[0], x[:, :, :ph, :pw])
    assert torch.equal(models[0].inputs[len(xs) if len(ys) > 1 else 0], x[:, :, ys[min(1, len(ys) - 1)]:ys[min(1, len(ys) - 1)] + ph, :pw])
    if mirror:
        assert torch.equal(models[0].inputs[len(ys) * len(xs)], x[:, :, :ph, :pw].flip(mirror[0]))
    P, label, gap, T = WR.blend(rec, b, h, w, ys, xs, window_weights(ph), window_weights(pw), m, mirror, weights)
    assert labels.dtype == torch.int64 and labels.shape == (b, h, w) and probs.shape == (b, k1, h, w) and probs.dtype == torch.float32
    WR.check(labels, probs, P, label, gap, T, str(case))
    assert (probs.sum(1) - 1).abs().max().item() < 1e-5
    for i, mod in enumerate(models):
        assert mod.training == (i % 2 == 0) and not any(mod.seen)  # run in eval mode, mode restored
    from inference import sliding_window_predict
    assert torch.equal(sliding_window_predict(models, x, (ph, pw), ov, mirror, weights), labels)


def test_constant_importance_and_int_patch_size():
    from inference import window_starts
    x = torch.randn(1, 2, 24, 24, generator=torch.Generator().manual_seed(3))
    models = [Recorder(3, 2, 8, 8, 1)]
    labels, probs, rec = run_recorded(models, x, 8, overlap=.5, importance="constant")
    s = window_starts(24, 8, .5)
    P, label, gap, T = WR.blend(rec, 1, 24, 24, s, s, np.ones(8, np.float32), np.ones(8, np.float32), 1)
    WR.check(labels, probs, P, label, gap, T, "constant")


def test_window_batch_is_bit_identical():
    x = torch.randn(2, 2, 40, 52, generator=torch.Generator().manual_seed(5))
    models = [Recorder(3, 2, 16, 24, 20 + i) for i in range(2)]
    base = run_recorded(models, x, (16, 24), mirror_axes=(2, 3), weights=[1.0, 1.5], window_batch=1)
    n_forwards = len(base[2])
    for wb in (3, 16):  # 16 windows: 3 leaves a ragged last chunk, 16 is all of them in one forward
        labels, probs, rec = run_recorded(models, x, (16, 24), mirror_axes=(2, 3), weights=[1.0, 1.5], window_batch=wb)
        assert torch.equal(labels, base[0]) and torch.equal(probs, base[1])
        assert len(rec) == n_forwards // 16 * math.ceil(16 / wb) and rec[0].shape[0] == wb * 2
        assert torch.equal(torch.cat(rec), torch.cat(base[2]))  # the same patches in the same order


@pytest.mark.parametrize("h,w,top,left", [(10, 40, 3, 0), (11, 40, 2, 0), (40, 13, 0, 1), (9, 12, 3, 2)])
def test_padding_of_short_axes(h, w, top, left):
    from inference import window_starts, window_weights
    x = torch.randn(2, 2, h, w, generator=torch.Generator().manual_seed(h)) + 3.0
    models = [Recorder(3, 2, 16, 16, 30)]
    labels, probs, rec = run_recorded(models, x, (16, 16), mirror_axes=(3,))
    assert labels.shape == (2, h, w) and probs.shape == (2, 3, h, w) and labels.is_contiguous() and probs.is_contiguous()
    hp, wp = max(h, 16), max(w, 16)
    seen = models[0].inputs[0]  # the first window: zero padding split evenly, the odd pixel at the end
    want = torch.zeros(2, 2, hp, wp)
    want[:, :, top:top + h, left:left + w] = x
    assert torch.equal(seen, want[:, :, :16, :16])
    ys, xs = window_starts(hp, 16, .5), window_starts(wp, 16, .5)
    P, label, gap, T = WR.blend(rec, 2, hp, wp, ys, xs, window_weights(16), window_weights(16), 1, (3,))
    crop = (slice(None), slice(top, top + h), slice(left, left + w))
    WR.check(labels, probs, P[:, :, crop[1], crop[2]], label[crop], gap[crop], T, f"padded {h}x{w}")


def test_modes_restored_when_a_model_raises():
    from inference import sliding_window_predict
    x = torch.zeros(1, 1, 24, 24)
    models = [Recorder(2, 1, 16, 16, 1).train(), Recorder(2, 1, 16, 16, 2, fail_at=2).train(), Recorder(2, 1, 16, 16, 3).eval()]
    with pytest.raises(RuntimeError, match="boom"):
        sliding_window_predict(models, x, 16, mirror_axes=(2,))
    assert [m.training for m in models] == [True, True, False]
    assert len(models[0].seen) == 8 and len(models[1].seen) == 3 and not models[2].seen
    for bad in [dict(mirror_axes=(1,)), dict(mirror_axes=(2, 2)), dict(weights=[1.0]), dict(window_batch=0), dict(overlap=1.0),
                dict(importance="cone")]:
        with pytest.raises(ValueError):
            sliding_window_predict(models, x, 16, **bad)
        assert [m.training for m in models] == [True, True, False]
    with pytest.raises(ValueError):
        sliding_window_predict([], x, 16)
    with pytest.raises(ValueError):
        sliding_window_predict(models[:1], x[0], 16)


def test_predictor_without_patch_size_is_unchanged_on_cpu():
    from inference import EnsemblePredictor, ensemble_predict, sliding_window_predict
    plain = EnsemblePredictor(32, folds=(0,), channels_list=[8, 16], device="cpu")
    assert plain.patch_size is None and plain.mirror_axes == () and plain.window_batch == 1
    tiled = EnsemblePredictor(None, folds=(0,), channels_list=[8, 16], device="cpu", patch_size=16, overlap=0.25, mirror_axes=(3,),
                              window_batch=2)
    assert tiled.patch_size == [16, 16] and tiled.image_size is None and tiled.overlap == 0.25
    with pytest.raises(ValueError):
        EnsemblePredictor(None, folds=(0,), channels_list=[8, 16], device="cpu", patch_size=16, mirror_axes=(1,))
    # predict_batch routes by patch_size (stand-in networks: the real ones run on the GPU only)
    x = torch.rand(1, 2, 24, 24, generator=torch.Generator().manual_seed(1)) * 255
    for p in (plain, tiled):
        p.models = [Recorder(3, 2, 16, 16, 4)]
        p.processor.image_size = None
    plain.models = [Recorder(3, 2, 24, 24, 4)]
    assert torch.equal(plain.predict_batch(x, do_denoise=False), ensemble_predict(plain.models, x / 255.0))
    assert torch.equal(tiled.predict_batch(x, do_denoise=False),
                       sliding_window_predict(tiled.models, x / 255.0, 16, 0.25, (3,), window_batch=2))


def test_header_declares_and_library_exports_window_entry_points():
    import mia_hip
    protos = mia_hip.parse_header()
    assert len(protos["mia_window_accum"][1]) == 19 and len(protos["mia_window_finalize"][1]) == 11
    with open(os.path.join(ROOT, "include", "mia_hip.h")) as fh:
        txt = fh.read()
    assert txt.index("mia_softmax_accum(") < txt.index("mia_window_accum(") < txt.index("mia_window_finalize(")
    lib = mia_hip.lib()
    # argument checks come before any launch: no device needed
    assert lib.mia_window_accum(None, None, None, None, 1, 3, 8, 8, 16, 16, 0, 0, 192, 64, 1, 1.0, 0, 0, None) == -1  # MIA_EARG
    assert lib.mia_window_finalize(None, None, None, None, 1, 3, 16, 16, 1.0, 1, None) == -1
    assert b"mia_window_finalize" in mia_hip.lib().mia_last_error()
