"""GPU checks of the validation / selection reductions (csrc/metrics.hip: argmax + hard Dice, selector scores) against the float64
restatement in tests/_metrics_ref.py, through metric.segmentation.predict_and_dice / label_dice and activelearning.scores.selector_scores
(which choose the slab count: hw // 2048, at least 1, at most 128).  Every element of every output is compared.

What is pinned -> case (ids of _metrics_ref.ARGMAX_CASES / SCORE_CASES: hw - K1 - batch):
  one slab (hw = 2240), fewer pixels than threads (hw = 7) ............ [2240-*], [7-*]
  two slabs, ragged last slab (65 x 67 = 2 * 2178 - 1) ................ [65x67-*]
  128 slabs (512 x 513), the 128-slab cap with a ragged last slab ..... [512x513-3-1], [515x517-3-1]
  K1 = 1, 2, 3, 8 (MAXK); scores K1 >= 2 .............................. every size below 512
  NCHW and channels-last storage ...................................... [*-nchw], [*-cl]
  exact ties: all classes equal, the last two tie for the maximum, the first and the last tie (the FIRST maximum must win; margin 0);
  -inf on a class; a class absent from the labels; a class never predicted: planted by _metrics_ref.logits_case in every case
  logits x 80 (saturated softmax) ..................................... test_*[*-80.0]
  labels = None (prediction only), label-map mode (logits == NULL) .... test_predict_without_labels, test_label_map_mode

Tolerances: pred, counts (integers < 2^24) and label maps bit-equal; Dice within 2^-23 of the float64 value (one fp64 expression rounded
once to fp32); scores rtol 2e-5, atol 1e-6."""
import numpy as np
import pytest
import torch

import _metrics_ref as M

pytestmark = pytest.mark.gpu

DICE_TOL = 2.0 ** -23
SCORE_RTOL, SCORE_ATOL = 2e-5, 1e-6


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _logits(z, layout, dev):
    t = torch.from_numpy(z).to(dev)
    if layout == "cl":
        t = t.contiguous(memory_format=torch.channels_last)
        assert t.stride(1) == 1 or t.shape[1] == 1
    return t


def _check_dice(pred, dice, counts, z, lab):
    nb, k1 = z.shape[:2]
    wp, wc, wd = M.argmax_dice(z.reshape(nb, k1, -1), lab.reshape(nb, -1))
    assert pred.dtype == torch.long and np.array_equal(pred.cpu().numpy().reshape(nb, -1), wp)
    assert np.array_equal(counts.cpu().numpy().astype(np.float64), wc)
    d = dice.cpu().numpy().astype(np.float64)
    assert np.isfinite(d).all() and np.abs(d - wd).max() <= DICE_TOL, float(np.abs(d - wd).max())


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("scale", [1.0, 80.0])
@pytest.mark.parametrize("case", M.ARGMAX_CASES, ids=M.case_id)
def test_argmax_dice(case, scale, layout):
    from metric.segmentation import predict_and_dice
    dev = _dev()
    hw_id, k1, nb = case
    z, lab = M.logits_case(hw_id, k1, nb, scale=scale)
    pred, dice, counts = predict_and_dice(_logits(z, layout, dev), torch.from_numpy(lab).to(dev))
    _check_dice(pred, dice, counts, z, lab)


@pytest.mark.parametrize("case", [("65x67", 3, 2), ("7", 8, 2)], ids=M.case_id)
def test_predict_without_labels(case):
    from metric.segmentation import predict_and_dice
    dev = _dev()
    z, _ = M.logits_case(*case)
    pred, dice, counts = predict_and_dice(_logits(z, "nchw", dev), None)
    assert dice is None and counts is None
    assert np.array_equal(pred.cpu().numpy().reshape(case[2], -1), M.argmax_dice(z.reshape(case[2], case[1], -1))[0])


@pytest.mark.parametrize("case", [("2240", 3, 2), ("65x67", 8, 2), ("515x517", 3, 1), ("7", 1, 2)], ids=M.case_id)
def test_label_map_mode(case):
    """logits == NULL: `pred` is an input.  The prediction here is an arbitrary label map (labels of another seed), not an argmax."""
    from metric.segmentation import label_dice
    dev = _dev()
    hw_id, k1, nb = case
    _, lab = M.logits_case(hw_id, k1, nb)
    _, pr = M.logits_case(hw_id, k1, nb, seed=5)
    pd = torch.from_numpy(pr).to(dev)
    keep = pd.clone()
    dice, counts = label_dice(pd, torch.from_numpy(lab).to(dev), k1)
    wc, wd = M.counts_dice(pr.reshape(nb, -1), lab.reshape(nb, -1), k1)
    assert torch.equal(pd, keep)  # the input label map is left alone
    assert np.array_equal(counts.cpu().numpy().astype(np.float64), wc)
    assert np.abs(dice.cpu().numpy().astype(np.float64) - wd).max() <= DICE_TOL


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("scale", [1.0, 80.0])
@pytest.mark.parametrize("case", M.SCORE_CASES, ids=M.case_id)
def test_selector_scores(case, scale, layout):
    from activelearning.scores import selector_scores
    dev = _dev()
    hw_id, k1, nb = case
    z, _ = M.logits_case(hw_id, k1, nb, scale=scale)
    got = selector_scores(_logits(z, layout, dev), 1e-8).cpu().numpy().astype(np.float64)
    want = M.selector_scores(z.reshape(nb, k1, -1), 1e-8)
    assert got.shape == want.shape and np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=SCORE_RTOL, atol=SCORE_ATOL)
