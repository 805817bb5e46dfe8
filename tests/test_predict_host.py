"""CPU checks of the prediction path: the float64 ensemble restatement against hand-computed answers, `ensemble_predict` on CPU
tensors (stand-in models), `EnsemblePredictor.load`, the C-ABI declarations, and `denoise_masks` on CPU tensors through the new
dispatch -- none of it needs a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import _predict_ref as R
from test_processor_host import blobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Fixed(torch.nn.Module):
    """A stand-in network: returns fixed logits, records the mode it was called in, optionally raises."""

    def __init__(self, logits, fail=False):
        super().__init__()
        self.logits, self.fail, self.seen = logits, fail, []

    def forward(self, x):
        self.seen.append(self.training)
        if self.fail:
            raise RuntimeError("boom")
        return self.logits


def test_restatement_hand_computed():
    ln = np.log
    # two models, 2 x 2 pixels, two classes; softmax(log a, log b) = (a, b) / (a + b)
    m0 = torch.tensor([[[[ln(3.0), ln(1.0)], [0.0, ln(1.0)]], [[ln(1.0), ln(3.0)], [0.0, ln(3.0)]]]])
    m1 = torch.tensor([[[[ln(1.0), ln(1.0)], [5.0, ln(3.0)]], [[ln(1.0), ln(1.0)], [5.0, ln(1.0)]]]])
    S, label, gap = R.ensemble([m0, m1])
    want = torch.tensor([[[[1.25, 0.75], [1.0, 1.0]], [[0.75, 1.25], [1.0, 1.0]]]], dtype=torch.float64)
    assert torch.allclose(S, want, atol=1e-15, rtol=0)
    # pixel (1, 0): identical logits in both models; pixel (1, 1): 1/4 + 3/4 against 3/4 + 1/4 -- exact ties go to class 0
    assert label.tolist() == [[[0, 1], [0, 0]]]
    assert torch.allclose(gap, torch.tensor([[[0.5, 0.5], [0.0, 0.0]]], dtype=torch.float64), atol=1e-15, rtol=0)
    S2, label2, _ = R.ensemble([m0, m1], [1.0, 3.0])
    assert torch.allclose(S2[0, :, 0, 0], torch.tensor([2.25, 1.75], dtype=torch.float64), atol=1e-15, rtol=0)
    assert label2.tolist() == [[[0, 1], [0, 0]]]  # (1, 1): 1/4 + 9/4 against 3/4 + 3/4


@pytest.mark.parametrize("m,k1,weights", [(1, 3, None), (3, 2, None), (5, 3, None), (4, 4, [0.5, 2.0, 1.0, 0.25])])
def test_ensemble_predict_cpu_matches_restatement(m, k1, weights):
    from inference import ensemble_predict
    g = torch.Generator().manual_seed(100 * m + k1)
    logits = [torch.randn(2, k1, 9, 11, generator=g) * 4 for _ in range(m)]
    models = [Fixed(l) for l in logits]
    for i, mod in enumerate(models):
        mod.train(i % 2 == 0)
    pred, probs = ensemble_predict(models, torch.zeros(2, 1, 9, 11), weights, return_probs=True)
    S, _, _ = R.ensemble(logits, weights)
    assert pred.dtype == torch.int64 and pred.shape == (2, 9, 11) and probs.shape == (2, k1, 9, 11)
    wsum = float(m) if weights is None else sum(abs(w) for w in weights)
    assert (probs.double() - S).abs().max().item() <= R.SUM_BOUND * wsum
    R.check_labels(pred, logits, weights)
    assert torch.equal(ensemble_predict(models, torch.zeros(1), weights), pred)
    for i, mod in enumerate(models):
        assert mod.training == (i % 2 == 0) and mod.seen == [False, False]  # run in eval mode, mode restored


def test_ensemble_predict_tie_goes_to_lowest_class():
    from inference import ensemble_predict
    l = torch.zeros(1, 3, 2, 2)
    l[0, :, 0, 1] = torch.tensor([-1.0, 2.0, 2.0])
    assert ensemble_predict([Fixed(l), Fixed(l)], torch.zeros(1)).tolist() == [[[0, 1], [0, 0]]]


def test_ensemble_predict_restores_modes_when_a_model_raises():
    from inference import ensemble_predict
    l = torch.zeros(1, 2, 2, 2)
    models = [Fixed(l).train(), Fixed(l, fail=True).train(), Fixed(l).eval()]
    with pytest.raises(RuntimeError, match="boom"):
        ensemble_predict(models, torch.zeros(1))
    assert [m.training for m in models] == [True, True, False]
    with pytest.raises(ValueError):
        ensemble_predict([], torch.zeros(1))
    with pytest.raises(ValueError):
        ensemble_predict(models[:1], torch.zeros(1), weights=[1.0, 2.0])


def test_predictor_load(tmp_path):
    from inference import EnsemblePredictor
    from models.unet import UNet
    folds, saved = (0, 2, 3), {}
    for k in folds:
        torch.manual_seed(50 + k)
        net = UNet(2, 3, 3, [8, 16])
        saved[k] = {n: v.detach().clone() for n, v in net.state_dict().items()}
        os.makedirs(tmp_path / f"fold_{k}")
        torch.save({"model": saved[k], "epoch": k}, tmp_path / f"fold_{k}" / "checkpoint_best.pth")
    pred = EnsemblePredictor(32, folds=folds, channels_list=[8, 16], device="cpu")
    assert pred.image_size == [32, 32] and len(pred.models) == 3 and not any(m.training for m in pred.models)
    assert pred.load(tmp_path) is pred
    for net, k in zip(pred.models, folds):
        sd = net.state_dict()
        assert sd.keys() == saved[k].keys()
        assert all(torch.equal(sd[n], saved[k][n]) for n in sd)
    assert not torch.equal(pred.models[0].state_dict()["decoder.seg_output.weight"], pred.models[1].state_dict()["decoder.seg_output.weight"])
    with pytest.raises(FileNotFoundError, match="fold_1"):
        EnsemblePredictor(32, folds=(0, 1), channels_list=[8, 16], device="cpu").load(tmp_path)


def test_header_declares_prediction_entry_points():
    import mia_hip
    protos = mia_hip.parse_header()
    assert len(protos["mia_softmax_accum"][1]) == 12
    assert len(protos["mia_mask_denoise_supported"][1]) == 5
    assert len(protos["mia_mask_denoise"][1]) == 9
    with open(os.path.join(ROOT, "include", "mia_hip.h")) as fh:
        txt = fh.read()
    assert re.search(r"entry/fugc2025/predict\.py|predict\.py:55-90", txt) and "unet_processor.py:72-160" in txt


def test_library_exports_prediction_entry_points():
    import mia_hip
    lib = mia_hip.lib()
    assert lib.mia_mask_denoise_supported(336, 544, 5, 5, 7) == 1
    assert lib.mia_mask_denoise_supported(61, 83, 8, 8, 7) == 1 and lib.mia_mask_denoise_supported(1, 1, 0, 0, 1) == 1
    for bad in [(336, 544, 9, 5, 7), (336, 544, 5, -1, 7), (336, 544, 5, 5, 9), (336, 544, 5, 5, 4), (3, 544, 5, 5, 7), (336, 2, 5, 5, 5)]:
        assert lib.mia_mask_denoise_supported(*bad) == 0, bad
    # argument checks come before any launch: no device needed
    assert lib.mia_softmax_accum(None, None, None, 1, 4, 3, 12, 4, 1, 1.0, 1, None) == -1  # MIA_EARG
    assert lib.mia_mask_denoise(None, None, 1, 8, 8, 5, 5, 7, None) < 0


@pytest.mark.parametrize("sizes", [(5, 5, 7), (3, 2, 5), (2, 4, 3), (1, 1, 1), (0, 0, 1), (8, 8, 7), (9, 3, 5)])
def test_denoise_cpu_tensors_unchanged(sizes):
    from models.unet.unet_processor import UnetProcessor
    from oracle import processor_ref
    d, e, k = sizes
    proc = UnetProcessor(image_size=None, dilate_size=d, erode_size=e, smooth_kernel=k)
    masks = blobs(3, 61, 83, seed=7 * d + k)
    t = torch.from_numpy(masks)
    got = proc.denoise_masks(t)
    assert got.dtype == torch.int64 and torch.equal(got, proc.denoise_masks(t, backend="tensor"))
    for i in range(3):
        assert np.array_equal(got[i].numpy(), processor_ref.denoise_one_mask(masks[i], d, e, k)), i
    assert torch.equal(proc.denoise_masks(t[0]), got[0])
    with pytest.raises(ValueError):
        proc.denoise_masks(t, backend="kernel")  # CPU tensors never reach the kernel
    with pytest.raises(ValueError):
        proc.denoise_masks(t, backend="fast")
