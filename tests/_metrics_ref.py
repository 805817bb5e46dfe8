"""Float64 restatement of the validation / selection reductions (csrc/metrics.hip) for tests/test_metrics_host.py and
tests/test_gpu_metrics.py, plus the seeded inputs and case tables the two share.  numpy only.

  argmax_dice      pred = argmax over classes of the logits (softmax is monotone; the FIRST maximum wins, like torch.argmax), and per
                   (image, class) the counts |P & G|, |P|, |G| of `pred == k` against `label == k` with Dice = 2 |P & G| / (|P| + |G|),
                   0 where the prediction is empty (medpy.metric.dc as `calculate_metric_percase` uses it).  Label-map mode takes `pred`
                   as an input instead of logits.
  selector_scores  per image: entropy mean_{c,h,w}(-p log2(p + smooth)), least confidence mean_{h,w}(-max_c p), margin
                   mean_{h,w}(-(p_top1 - p_top2)), p = softmax of the logits.
"""
import numpy as np

f32, f64 = np.float32, np.float64
MAXK = 8


def slabs_of(hw):
    """Pixel slabs per image that metric.segmentation / activelearning.scores ask the kernels for."""
    return max(1, min(128, hw // 2048))


def slab_lengths(hw):
    """Pixels of each slab: ceil(hw / slabs) per slab, the last one takes what is left."""
    s = slabs_of(hw)
    per = (hw + s - 1) // s
    return [max(0, min(per, hw - i * per)) for i in range(s)]


def counts_dice(pred, labels, k1):
    """pred, labels [B, P] integer -> (counts [B, k1, 3] = (|P & G|, |P|, |G|), dice [B, k1]) in float64."""
    b = pred.shape[0]
    counts = np.zeros((b, k1, 3), dtype=f64)
    for k in range(k1):
        p, g = pred == k, labels == k
        counts[:, k, 0], counts[:, k, 1], counts[:, k, 2] = (p & g).sum(1), p.sum(1), g.sum(1)
    den = counts[..., 1] + counts[..., 2]
    dice = np.where(counts[..., 1] > 0, 2.0 * counts[..., 0] / np.where(den > 0, den, 1.0), 0.0)
    return counts, dice


def argmax_dice(logits, labels=None):
    """logits [B, K1, P] fp32 -> (pred [B, P] int64, counts, dice); counts and dice are None without labels."""
    pred = np.argmax(np.asarray(logits), axis=1).astype(np.int64)  # numpy: first occurrence of the maximum
    if labels is None:
        return pred, None, None
    return (pred,) + counts_dice(pred, np.asarray(labels), logits.shape[1])


def selector_scores(logits, smooth=1e-8):
    """logits [B, K1, P] fp32 -> [B, 3] float64 (entropy, -max prob, -(top1 - top2))."""
    z = np.asarray(logits, dtype=f64)
    z = z - z.max(axis=1, keepdims=True)
    e = np.exp(z)
    p = e / e.sum(axis=1, keepdims=True)
    ent = (-p * np.log2(p + f64(f32(smooth)))).mean(axis=(1, 2))
    top = np.sort(p, axis=1)
    return np.stack([ent, (-top[:, -1]).mean(axis=1), (-(top[:, -1] - top[:, -2])).mean(axis=1)], axis=1)


# --------------------------------------------------------------------------- inputs and case tables
# id -> (h, w): one slab; two slabs with a ragged last one; exactly 128 slabs of 2052; the 128-slab cap with a ragged last slab; fewer
# pixels than threads
HW = {"2240": (40, 56), "65x67": (65, 67), "512x513": (512, 513), "515x517": (515, 517), "7": (1, 7)}
# (hw id, K1, batch): every K1 at the small sizes, K1 = 3 at the large ones
ARGMAX_CASES = [(s, k1, 2) for s in ("2240", "65x67", "7") for k1 in (1, 2, 3, 8)] + [("512x513", 3, 1), ("515x517", 3, 1)]
SCORE_CASES = [c for c in ARGMAX_CASES if c[1] >= 2]
case_id = lambda c: "-".join(str(v) for v in c)


def logits_case(hw_id, k1, nb, seed=0, scale=1.0):
    """(logits [B, K1, H, W] fp32, labels [B, H, W] int64) with planted edge pixels in every image (positions spread over the slabs):
      * pixel 0: all classes equal (an exact tie of everything: class 0 must win, p1 == p2);
      * pixel P // 3: the two LAST classes tie for the maximum (the first of the two must win; margin 0);
      * pixel P // 2 of every image but the first: -inf on class 0;
      * pixel P - 1 (the end of the last slab): the first and the last class tie (the first must win).
    For K1 > 1, class 0 never occurs in the labels of image 0 (absent class) and class K1 - 1 lies below every other logit of image 0
    and loses every planted tie (never predicted: Dice 0 by the empty-prediction rule).  Logits are multiples of 2^-6 times `scale`."""
    h, w = HW[hw_id]
    p = h * w
    g = np.random.default_rng(seed + 1000 * k1 + p)
    z = (g.integers(-256, 257, size=(nb, k1, p)).astype(f64) / 64.0)  # in [-4, 4]
    labels = g.integers(0, k1, size=(nb, p))
    if k1 > 1:
        z[0, k1 - 1] = -5.0
        labels[0][labels[0] == 0] = 1
    for b in range(nb):
        z[b, :, 0] = 1.5
        if k1 >= 2:
            z[b, :, p // 3] = -2.0
            z[b, k1 - 2:, p // 3] = 3.25
            z[b, 0, p - 1] = z[b, k1 - 1, p - 1] = 4.5
            if b > 0:
                z[b, 0, p // 2] = -np.inf
    z = (z * scale).astype(f32)
    return z.reshape(nb, k1, h, w), labels.reshape(nb, h, w).astype(np.int64)
