"""GPU checks of the region ensemble (`mia_sigmoid_accum` in csrc/predict.hip, `inference.sigmoid_accum` and
`ensemble_predict_regions`) against the float64 restatement in tests/_region_loss_ref.py."""
import numpy as np
import pytest
import torch

import _region_loss_ref as R
from test_region_loss_host import Fixed

pytestmark = pytest.mark.gpu
WEIGHTS = [0.5, 1.0, 2.0]
# (shape, class_order): four pixels per thread at 37 x 52, one pixel per thread at 19 x 21 (odd size)
CASES = [((2, 3, 37, 52), [1, 2, 3]), ((1, 2, 19, 21), [2, 1])]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _logits(shape, layout, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(3):
        t = (3 * torch.randn(*shape, generator=g)).to(dev)
        if layout == "nhwc":
            t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        out.append(t)
    return out


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("shape,order", CASES, ids=["37x52", "19x21"])
def test_ensemble_predict_regions_matches_restatement(shape, order, layout):
    from inference import ensemble_predict_regions
    dev = _dev()
    logits = _logits(shape, layout, dev)
    models = [Fixed(l) for l in logits]
    models[1].eval()
    pred, prob = ensemble_predict_regions(models, torch.zeros(1, device=dev), order, WEIGHTS, return_probs=True)
    assert pred.dtype == torch.int64 and tuple(pred.shape) == (shape[0],) + shape[2:]
    assert prob.dtype == torch.float32 and prob.is_contiguous() and tuple(prob.shape) == shape
    want_sum = R.sigmoid_sum([l.cpu().numpy() for l in logits], WEIGHTS)
    err = np.abs(prob.cpu().numpy() - want_sum).max()
    print(f"{shape} {layout}: max|prob_sum - float64| {err:.2e}")
    assert err < 1e-6 * sum(WEIGHTS)
    # labels: the restated rule wherever the float64 mean probability is further than 1e-5 from 1/2 in every channel
    want = R.regions_to_labels(want_sum, order, 0.5 * sum(WEIGHTS))
    far = (np.abs(want_sum / sum(WEIGHTS) - 0.5) > 1e-5).all(1)
    assert 1.0 - far.mean() <= 1e-3
    assert np.array_equal(pred.cpu().numpy()[far], want[far])
    # ... and exactly the rule on the fp32 sum the kernel itself produced
    assert np.array_equal(pred.cpu().numpy(), R.regions_to_labels(prob.cpu().numpy(), order, np.float32(0.5 * sum(WEIGHTS))))
    assert [m.seen for m in models] == [[False]] * 3 and [m.training for m in models] == [True, False, True]
    # a second run is bit-identical, with or without the probabilities
    pred2, prob2 = ensemble_predict_regions(models, torch.zeros(1, device=dev), order, WEIGHTS, return_probs=True)
    assert torch.equal(pred, pred2) and torch.equal(prob, prob2)
    assert torch.equal(ensemble_predict_regions(models, torch.zeros(1, device=dev), order, WEIGHTS), pred)
    # the CPU branch is the same definition
    cpu = ensemble_predict_regions([Fixed(l.cpu()) for l in logits], torch.zeros(1), order, WEIGHTS)
    assert np.array_equal(cpu.numpy()[far], pred.cpu().numpy()[far])


@pytest.mark.parametrize("shape,order", CASES, ids=["37x52", "19x21"])
def test_rule_single_model_and_modes(shape, order):
    from inference import ensemble_predict_regions, regions_to_labels, sigmoid_accum
    dev = _dev()
    logits = _logits(shape, "nchw", dev, seed=1)
    # one model, no running sum: the plain thresholded map (sigmoid(z) > 1/2 <=> z > 0 away from the threshold)
    pred = ensemble_predict_regions([Fixed(logits[0])], torch.zeros(1, device=dev), order)
    z = logits[0]
    far = (z.abs() > 1e-4).all(1)
    want = regions_to_labels((z > 0).float(), order, 0.5)
    assert far.float().mean() > 0.999 and torch.equal(pred[far], want[far])
    direct = torch.empty_like(pred)
    sigmoid_accum(z, None, direct, torch.tensor(order, device=dev), 1.0, 0.5, first=True)
    assert torch.equal(direct, pred)
    # a later region overwrites an earlier one: with every channel far above the threshold the last label wins everywhere,
    # with none above it everything is background, and the order of `class_order` is the order of writing
    big = torch.full(shape, 8.0, device=dev)
    assert (ensemble_predict_regions([Fixed(big)], big, order) == order[-1]).all()
    assert (ensemble_predict_regions([Fixed(big)], big, order[::-1]) == order[0]).all()
    assert (ensemble_predict_regions([Fixed(-big)], big, order) == 0).all()
    first_only = -big.clone()
    first_only[:, 0] = 8.0
    assert (ensemble_predict_regions([Fixed(first_only), Fixed(first_only)], big, order) == order[0]).all()
    # every model gets its mode back after an exception
    models = [Fixed(logits[0]), Fixed(logits[1], fail=True), Fixed(logits[2])]
    models[2].eval()
    with pytest.raises(RuntimeError):
        ensemble_predict_regions(models, torch.zeros(1, device=dev), order)
    assert [m.training for m in models] == [True, True, False]


def test_sigmoid_accum_argument_checks():
    import mia_hip
    from inference import sigmoid_accum
    dev = _dev()
    l = torch.zeros(1, 3, 4, 4, device=dev)
    order = torch.tensor([1, 2, 3], device=dev)
    with pytest.raises(mia_hip.MiaError):
        sigmoid_accum(l, None, None, None, 1.0, 0.5, first=True)
    with pytest.raises(mia_hip.MiaError):
        sigmoid_accum(l, None, torch.empty(1, 4, 4, device=dev, dtype=torch.int64), order, 1.0, 0.5, first=False)
    with pytest.raises(ValueError):
        sigmoid_accum(l, torch.zeros(1, 3, 4, 5, device=dev), None, None, 1.0, 0.5, first=True)
    with pytest.raises(ValueError):
        sigmoid_accum(l, None, torch.empty(1, 4, 4, device=dev, dtype=torch.int64), order[:2], 1.0, 0.5, first=True)
    with pytest.raises(ValueError):
        sigmoid_accum(l, None, torch.empty(1, 4, 4, device=dev, dtype=torch.int32), order, 1.0, 0.5, first=True)
