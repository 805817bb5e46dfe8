"""Float64 numpy restatement of the region-based loss (csrc/region_loss.hip, include/mia_hip.h) and of the region-to-label rule
(mia_sigmoid_accum).  Written from the definition, not from the kernel: no slabs, no quads, no coefficient table in fp32.

    p = sigmoid(z);  over the valid pixels of (image b, channel c):  I = sum p t,  P = sum p,  G = sum t
    dc = -mean (2I + smooth) / max(G + P + smooth, 1e-8)   (channels 1.. without do_bg; I, P, G summed over the batch with batch_dice)
    CE = sum_valid [pw t softplus(-z) + (1 - t) softplus(z)] / N,  N = B C HW without ignore, max(#valid pixels, 1e-8) with it
    value = ce_w CE + dice_w dc;  counts = tp, fp, fn of (z > 0) against (t > 0.5) over the valid pixels
    dvalue/dz = valid [ce_w (p (1 + (pw - 1) t) - pw t) / N + dice_w p (1 - p) (a t + b)],  a = d dc / dI, b = d dc / dP, both 0 where
    the denominator was clipped."""
import numpy as np


def expand_regions(labels, regions, ignore_label=None):
    """labels [B,H,W] or [B,1,H,W] -> (t [B,C,H,W] float64 of 0/1, valid [B,H,W] bool)."""
    labels = np.asarray(labels)
    if labels.ndim == 4:
        labels = labels[:, 0]
    t = np.stack([np.isin(labels, list(r)) for r in regions], 1).astype(np.float64)
    valid = np.ones(labels.shape, bool) if ignore_label is None else labels != ignore_label
    return t, valid


def split_dense(target, use_ignore):
    """dense target [B,C(+1),H,W] -> (t float64 [B,C,H,W], valid [B,H,W] bool)."""
    target = np.asarray(target).astype(np.float64)
    if use_ignore:
        return target[:, :-1], target[:, -1] == 0
    return target, np.ones((target.shape[0],) + target.shape[2:], bool)


def softplus(z):
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def region_loss(z, t, valid, use_ignore, pos_weight=None, smooth=1.0, do_bg=True, batch_dice=False, ce_w=1.0, dice_w=1.0):
    """dict(value, ce, dc, grad [B,C,H,W], counts int64 [B,C,3]) in float64."""
    z = np.asarray(z, np.float64)
    t = np.asarray(t, np.float64)
    b, c, h, w = z.shape
    v = np.asarray(valid, bool).reshape(b, 1, h, w).astype(np.float64)
    pw = np.ones(c) if pos_weight is None else np.asarray(pos_weight, np.float64).reshape(c)
    pw = pw.reshape(1, c, 1, 1)
    e = np.exp(-np.abs(z))
    p = np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    bce = (pw * t * softplus(-z) + (1.0 - t) * softplus(z)) * v
    n = max(float(v.sum()), 1e-8) if use_ignore else float(b * c * h * w)
    ce = bce.sum() / n
    I, P, G = (p * t * v).sum((2, 3)), (p * v).sum((2, 3)), (t * v).sum((2, 3))
    if batch_dice:
        I, P, G = I.sum(0, keepdims=True), P.sum(0, keepdims=True), G.sum(0, keepdims=True)
    k0 = 0 if do_bg else 1
    if c - k0 < 1:
        raise ValueError("no Dice term left")
    num, den = 2 * I + smooth, G + P + smooth
    clip = den < 1e-8
    dcl = np.where(clip, 1e-8, den)
    use = np.zeros((1, c))
    use[:, k0:] = 1.0
    cnt = use.sum() * I.shape[0]
    dc = -((num / dcl) * use).sum() / cnt
    a = np.where(clip, 0.0, -2.0 / dcl) * use / cnt
    bb = np.where(clip, 0.0, num / (dcl * dcl)) * use / cnt
    a, bb = a[:, :, None, None], bb[:, :, None, None]  # [B or 1, C, 1, 1] broadcasts over the batch with batch_dice
    grad = v * (ce_w * (p * (1.0 + (pw - 1.0) * t) - pw * t) / n + dice_w * p * (1.0 - p) * (a * t + bb))
    hp, ht, vb = z > 0, t > 0.5, v > 0
    counts = np.stack([(hp & ht & vb).sum((2, 3)), (hp & ~ht & vb).sum((2, 3)), (~hp & ht & vb).sum((2, 3))], -1).astype(np.int64)
    return dict(value=ce_w * ce + dice_w * dc, ce=ce, dc=dc, grad=grad, counts=counts)


def region_loss_dense(z, target, use_ignore, **kw):
    t, valid = split_dense(target, use_ignore)
    return region_loss(z, t, valid, use_ignore, **kw)


def region_loss_index(z, labels, regions, ignore_label=None, **kw):
    t, valid = expand_regions(labels, regions, ignore_label)
    return region_loss(z, t, valid, ignore_label is not None, **kw)


def regions_to_labels(prob_sum, class_order, threshold):
    """pred = 0; for i: pred[prob_sum[:, i] > threshold] = class_order[i] -- later regions overwrite earlier ones."""
    prob_sum = np.asarray(prob_sum)
    pred = np.zeros((prob_sum.shape[0],) + prob_sum.shape[2:], np.int64)
    for i, lab in enumerate(class_order):
        pred[prob_sum[:, i] > threshold] = int(lab)
    return pred


def sigmoid_sum(logits_list, weights):
    """float64 sum_m weights[m] * sigmoid(logits[m])."""
    acc = 0.0
    for z, wt in zip(logits_list, weights):
        z = np.asarray(z, np.float64)
        e = np.exp(-np.abs(z))
        acc = acc + wt * np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return acc
