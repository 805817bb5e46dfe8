"""The prediction path on the GPU (csrc/predict.hip, inference/predictor.py, UnetProcessor.denoise_masks): `mia_softmax_accum`
against the float64 ensemble restatement of tests/_predict_ref.py within bounds derived from fp32 rounding, ties, determinism and
the `first` flag; `mia_mask_denoise` bit for bit against the scipy restatement in oracle/ and against the tensor path; and
`EnsemblePredictor` end to end on three small networks."""
import numpy as np
import pytest
import torch

import _predict_ref as R
from test_processor_host import blobs

pytestmark = pytest.mark.gpu

SIZES = [(5, 5, 7), (3, 2, 5), (2, 4, 3), (1, 1, 1), (0, 0, 1), (8, 8, 7)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _logits(m, b, k1, h, w, scale, seed, layout, dev):
    """m logits tensors [b,k1,h,w] on the device: contiguous NCHW, or the channels-last view the model's head returns."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(m):
        l = (torch.randn(b, k1, h, w, generator=g) * scale).to(dev)
        if layout == "head":
            nhwc = torch.empty(b, h, w, k1, device=dev)
            nhwc.copy_(l.permute(0, 2, 3, 1))
            l = nhwc.permute(0, 3, 1, 2)
            assert l.stride(1) == 1 and l.stride(3) == k1
        out.append(l)
    return out


def _accumulate(logits, weights, dev):
    from inference import softmax_accum
    b, k1, h, w = logits[0].shape
    prob = torch.full((b, k1, h, w), float("nan"), device=dev)  # `first` must overwrite it
    pred = torch.full((b, h, w), -7, device=dev, dtype=torch.int64)
    for i, (l, wt) in enumerate(zip(logits, weights)):
        softmax_accum(l, prob, pred if i == len(logits) - 1 else None, wt, first=i == 0)
    return prob, pred


@pytest.mark.parametrize("layout", ["nchw", "head"])
@pytest.mark.parametrize("scale", [2.0, 6.0])
@pytest.mark.parametrize("k1", [2, 3, 4])
@pytest.mark.parametrize("m", [1, 3, 5, 7])
def test_softmax_accum_matches_restatement(m, k1, scale, layout):
    dev = _dev()
    for shape_i, (b, h, w) in enumerate([(2, 336, 544), (3, 255, 257), (1, 1, 1), (2, 64, 66)]):
        for weights in ([1.0] * m, [0.5 + 0.75 * i for i in range(m)]):
            logits = _logits(m, b, k1, h, w, scale, 1000 * m + 100 * k1 + 10 * shape_i + int(scale), layout, dev)
            prob, pred = _accumulate(logits, weights, dev)
            S, _, _ = R.ensemble(logits, weights)
            err = (prob.cpu().double() - S).abs().max().item()
            bound = R.SUM_BOUND * sum(abs(v) for v in weights)
            print(f"M={m} k1={k1} s={scale} {layout} {b}x{h}x{w} w0={weights[0]}: max|prob_sum - S| = {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (err, bound)
            if b * h * w >= 1000:
                R.check_labels(pred, logits, weights)
            else:  # too few pixels for a share: every decided pixel must match
                _, label, gap = R.ensemble(logits, weights)
                ok = gap >= R.GAP_BOUND * sum(abs(v) for v in weights)
                assert torch.equal(pred.cpu()[ok], label[ok])


def test_softmax_accum_single_model_without_sum():
    from inference import ensemble_predict, softmax_accum
    dev = _dev()
    for layout in ("nchw", "head"):
        logits = _logits(1, 2, 3, 100, 101, 4.0, 5, layout, dev)
        pred = torch.empty((2, 100, 101), device=dev, dtype=torch.int64)
        softmax_accum(logits[0], None, pred, 1.0, first=True)
        R.check_labels(pred, logits)

        class One(torch.nn.Module):
            def forward(self, x):
                return logits[0]
        assert torch.equal(ensemble_predict([One()], torch.zeros(1, device=dev)), pred)


def test_softmax_accum_argument_checks():
    import mia_hip
    from inference import softmax_accum
    dev = _dev()
    l = torch.zeros(1, 3, 4, 4, device=dev)
    with pytest.raises(mia_hip.MiaError):
        softmax_accum(l, None, None, 1.0, first=True)
    with pytest.raises(mia_hip.MiaError):
        softmax_accum(l, None, torch.empty(1, 4, 4, device=dev, dtype=torch.int64), 1.0, first=False)
    with pytest.raises(mia_hip.MiaError):
        softmax_accum(torch.zeros(1, 9, 4, 4, device=dev), torch.zeros(1, 9, 4, 4, device=dev), None, 1.0, first=True)
    with pytest.raises(ValueError):
        softmax_accum(l, torch.zeros(1, 3, 4, 5, device=dev), None, 1.0, first=True)


@pytest.mark.parametrize("layout", ["nchw", "head"])
def test_softmax_accum_ties_determinism_and_first(layout):
    dev = _dev()
    for (b, h, w) in [(2, 64, 64), (1, 33, 35)]:  # the four-pixel and the one-pixel path
        logits = _logits(3, b, 3, h, w, 3.0, 77, layout, dev)
        for l in logits:
            l[:, 2] = l[:, 1]                # classes 1 and 2 identical in every model
            l[:, :, : h // 2] = 0.25         # all classes equal in the upper half
        prob, pred = _accumulate(logits, [1.0, 1.0, 1.0], dev)
        assert torch.isfinite(prob).all()    # the NaN pre-fill is gone
        assert pred.min() >= 0 and (pred[:, : h // 2] == 0).all()
        assert (pred != 2).all()             # never the higher of two tied classes
        assert torch.equal(prob[:, 1], prob[:, 2])
        want = torch.where(prob[:, 1] > prob[:, 0], 1, 0)
        assert torch.equal(pred, want)
        prob2, pred2 = _accumulate(logits, [1.0, 1.0, 1.0], dev)
        assert torch.equal(prob, prob2) and torch.equal(pred, pred2)  # bit-identical from run to run


def _denoise_inputs(h_small, w_small):
    """(name, label maps) the denoise is checked on: blobs, uniform random maps at three densities (set and unset pixels on every
    tile seam), constant maps, labels outside {0, 1, 2}."""
    cases = [("blobs_61x83", blobs(3, 61, 83, seed=3)), ("blobs_336x544", blobs(2, 336, 544, seed=4))]
    for dens in (0.05, 0.5, 0.95):
        cases.append((f"random{dens}_130x200", R.random_labels(3, 130, 200, dens, seed=int(dens * 100))))
        cases.append((f"random{dens}_576x576", R.random_labels(2, 576, 576, dens, seed=int(dens * 100) + 1)))
    for v in (0, 1, 2):
        cases.append((f"all_{v}", np.full((1, h_small, w_small), v, dtype=np.int64)))
    odd = blobs(2, h_small, w_small, seed=9)
    g = np.random.default_rng(5)
    odd[g.random(odd.shape) < 0.1] = -3
    odd[g.random(odd.shape) < 0.1] = 7
    odd[0, :10, :10] = np.iinfo(np.int64).min
    odd[1, -10:, -10:] = np.iinfo(np.int64).max
    cases.append(("labels_outside_0_1_2", odd))
    return cases


@pytest.mark.parametrize("sizes", SIZES)
def test_mask_denoise_exact(sizes):
    from models.unet.unet_processor import UnetProcessor
    from oracle import processor_ref
    dev = _dev()
    d, e, k = sizes
    proc = UnetProcessor(image_size=None, dilate_size=d, erode_size=e, smooth_kernel=k)
    for name, masks in _denoise_inputs(70, 129):
        t = torch.from_numpy(masks).to(dev)
        assert proc._kernel_covers(t)
        got = proc.denoise_masks(t, backend="kernel")
        assert torch.equal(t, torch.from_numpy(masks).to(dev))  # the input is left alone
        tensor_path = proc.denoise_masks(t, backend="tensor")
        n_bad = int((got != tensor_path).sum())
        print(f"{sizes} {name}: {n_bad} pixels differ from the tensor path")
        assert got.dtype == torch.int64 and got.shape == t.shape and n_bad == 0, (name, n_bad)
        assert torch.equal(proc.denoise_masks(t), got)  # the default dispatch takes the kernel
        g = got.cpu().numpy()
        for i in range(masks.shape[0]):
            want = processor_ref.denoise_one_mask(masks[i], d, e, k)
            assert np.array_equal(g[i], want), (name, i, int((g[i] != want).sum()))
        assert torch.equal(proc.denoise_masks(t[0]), got[0])  # one [H,W] map


@pytest.mark.parametrize("h,w", [(1, 1), (4, 4), (5, 300), (64, 64), (65, 63), (128, 192), (200, 7)])
def test_mask_denoise_small_and_seam_shapes(h, w):
    from models.unet.unet_processor import UnetProcessor
    dev = _dev()
    for (d, e, k) in [(5, 5, 7), (2, 4, 3), (0, 0, 1), (8, 8, 7)]:
        if h <= k // 2 or w <= k // 2:
            continue
        proc = UnetProcessor(image_size=None, dilate_size=d, erode_size=e, smooth_kernel=k)
        for dens in (0.3, 0.8):
            t = torch.from_numpy(R.random_labels(5, h, w, dens, seed=h * 1000 + w)).to(dev)
            assert torch.equal(proc.denoise_masks(t, backend="kernel"), proc.denoise_masks(t, backend="tensor")), (h, w, d, e, k, dens)


def test_mask_denoise_fallback_shapes():
    """What `mia_mask_denoise_supported` turns down goes through the tensor path and still matches the restatement."""
    import mia_hip
    from models.unet.unet_processor import UnetProcessor
    from oracle import processor_ref
    dev = _dev()
    masks = blobs(2, 61, 83, seed=12)
    t = torch.from_numpy(masks).to(dev)
    for (d, e, k) in [(9, 3, 5), (2, 12, 7)]:
        proc = UnetProcessor(image_size=None, dilate_size=d, erode_size=e, smooth_kernel=k)
        assert not proc._kernel_covers(t)
        with pytest.raises(ValueError):
            proc.denoise_masks(t, backend="kernel")
        got = proc.denoise_masks(t).cpu().numpy()
        for i in range(2):
            assert np.array_equal(got[i], processor_ref.denoise_one_mask(masks[i], d, e, k))
        out = torch.empty_like(t)
        rc = mia_hip.lib().mia_mask_denoise(t.data_ptr(), out.data_ptr(), 2, 61, 83, d, e, k, None)
        assert rc == -2  # MIA_EUNSUPPORTED: the C entry point refuses, it does not guess
    proc = UnetProcessor()
    assert not proc._kernel_covers(t.int()) and not proc._kernel_covers(t.cpu())
    assert torch.equal(proc.denoise_masks(t.int()).long(), proc.denoise_masks(t))  # other dtypes: tensor path, same labels
    assert proc.denoise_masks(t.int()).dtype == torch.int32


def test_ensemble_predictor_end_to_end():
    from inference import EnsemblePredictor
    dev = _dev()
    pred = EnsemblePredictor(256, folds=(0, 1, 2), channels_list=[16, 32, 64], device=dev)
    for i, net in enumerate(pred.models):  # three differently seeded networks
        torch.manual_seed(20 + i)
        fresh = type(net)(2, 3, 3, [16, 32, 64])
        net.load_state_dict(fresh.state_dict())
    from mia_hip import ops
    ops.bump_param_epoch()
    g = torch.Generator().manual_seed(3)
    X = torch.rand(8, 3, 336, 544, generator=g) * 255.0
    x = pred.preprocess(X)
    assert x.shape == (8, 3, 256, 256)
    with torch.no_grad():
        logits = [net(x).float() for net in pred.models]
    assert not torch.equal(logits[0], logits[1])
    raw = pred.predict_batch(X, do_denoise=False)
    assert raw.shape == (8, 336, 544) and raw.dtype == torch.int64 and raw.is_cuda
    from inference import ensemble_predict
    small = ensemble_predict(pred.models, x)
    R.check_labels(small, logits)
    assert torch.equal(raw, pred.processor.postprocess(small, (336, 544)))
    out = pred.predict_batch(X)
    assert torch.equal(out, pred.processor.denoise_masks(raw, backend="tensor"))
    one = pred.predict(X[0].numpy())
    assert isinstance(one, np.ndarray) and one.shape == (336, 544) and np.array_equal(one, out[0].cpu().numpy())
    assert not any(net.training for net in pred.models)
