"""Restatements for the prediction path (TEST INFRASTRUCTURE ONLY): the fold ensemble of the reference's
`entry/fugc2025/predict.py:144-161,:55-57` in float64 torch, and the inputs the denoise tests share."""
import numpy as np
import torch

# Bounds of the GPU reduction, from fp32 rounding: an fp32 softmax value is within a few ulp (6e-8) of the exact one and M of them
# are added, so |prob_sum - S| <= 2e-6 * sum|w|; two classes whose exact sums differ by more than twice that cannot swap.
SUM_BOUND = 2e-6
GAP_BOUND = 4e-6
MAX_UNDECIDED = 1e-3  # share of pixels that may fall under the gap


def ensemble(logits, weights=None):
    """(S [B,K,H,W] float64, label [B,H,W] int64, gap [B,H,W] float64) with S = sum_m w_m * softmax(logits_m.double(), 1),
    label = S.argmax(1) and gap = top1(S) - top2(S) (+inf for a single class)."""
    weights = [1.0] * len(logits) if weights is None else list(weights)
    assert len(weights) == len(logits) and len(logits) > 0
    S = None
    for w, l in zip(weights, logits):
        p = float(w) * l.detach().cpu().double().softmax(1)
        S = p if S is None else S + p
    label = S.argmax(1)
    if S.shape[1] > 1:
        top = S.topk(2, dim=1).values
        gap = top[:, 0] - top[:, 1]
    else:
        gap = torch.full(label.shape, float("inf"), dtype=torch.float64)
    return S, label, gap


def check_labels(got, logits, weights=None):
    """`got` equals the restatement's labels wherever the gap decides; returns the share of pixels left out (< MAX_UNDECIDED)."""
    weights = [1.0] * len(logits) if weights is None else list(weights)
    _, label, gap = ensemble(logits, weights)
    decided = gap >= GAP_BOUND * sum(abs(w) for w in weights)
    share = 1.0 - decided.double().mean().item()
    wrong = int(((got.cpu() != label) & decided).sum())
    print(f"labels: {wrong} mismatches over {int(decided.sum())} decided pixels, undecided share {share:.3e}")
    assert share < MAX_UNDECIDED, share
    assert wrong == 0, wrong
    return share


def random_labels(n, h, w, density, seed):
    """Uniform random label maps: a pixel is foreground with probability `density`, then class 1 or 2 with equal odds."""
    g = np.random.default_rng(seed)
    fg = g.random((n, h, w)) < density
    return np.where(fg, g.integers(1, 3, size=(n, h, w)), 0).astype(np.int64)
