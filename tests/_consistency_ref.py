"""float64 numpy restatement of the mean-teacher consistency loss (csrc/consistency.hip, losses/consistency_loss.py), of the
exponential moving average and of its alpha schedule, for the tests.

Student logits zs and teacher logits zt, [B, K, H, W]; ps = softmax(zs, 1), pt = softmax(zt, 1), e = ps - pt, d = sum_k e_k^2:

    plain:   L = sum d / (B K H W)                                              torch.mean((ps - pt) ** 2)
    masked:  u = -sum_k pbar_k log(pbar_k + 1e-6), keep = (u < threshold), L = sum keep d / (den_scale sum keep + 1e-16)
    dL/dzs_j = coef keep 2 ps_j (e_j - sum_k ps_k e_k),  coef = 1 / denominator

    teacher = alpha teacher + (1 - alpha) student,  alpha_i = min(1 - 1 / (i + 1), ema_decay)
"""
import math

import numpy as np


def softmax(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def entropy(pbar):
    """u [B, H, W] of pbar [B, K, H, W]."""
    p = np.asarray(pbar, np.float64)
    return -(p * np.log(p + 1e-6)).sum(1)


def keep_mask(pbar, threshold):
    return entropy(pbar) < float(threshold)


def evaluate(zs, zt, keep=None, den_scale=2.0):
    """dict(value, grad, coef, n_keep, value_mag, grad_mag): L and dL/dzs in float64 for a boolean `keep` [B, H, W] (None = the plain
    form), and the magnitudes the tests' bounds are stated in:
      value_mag = coef sum keep sum_k |e_k| (ps_k + pt_k)
      grad_mag  = 2 coef keep ps_j ((ps_j + pt_j) + sum_k ps_k (ps_k + pt_k))      per element"""
    ps, pt = softmax(zs), softmax(zt)
    b, k, h, w = ps.shape
    e = ps - pt
    if keep is None:
        m = np.ones((b, h, w), np.float64)
        den = float(b * k * h * w)
    else:
        m = np.asarray(keep).astype(np.float64).reshape(b, h, w)
        den = den_scale * m.sum() + 1e-16
    coef = 1.0 / den
    m1 = m[:, None]
    value = coef * (m1 * e * e).sum()
    grad = coef * m1 * 2.0 * ps * (e - (ps * e).sum(1, keepdims=True))
    value_mag = coef * (m1 * np.abs(e) * (ps + pt)).sum()
    grad_mag = 2.0 * coef * m1 * ps * ((ps + pt) + (ps * (ps + pt)).sum(1, keepdims=True))
    return dict(value=float(value), grad=grad, coef=coef, n_keep=int(m.sum()), value_mag=float(value_mag), grad_mag=grad_mag)


def ema(teacher, student, alpha):
    t, s, a = np.asarray(teacher, np.float64), np.asarray(student, np.float64), float(alpha)
    return a * t + (1.0 - a) * s


def ema_bound(teacher, student, alpha):
    """2 * 2^-24 * (|alpha t| + |(1 - alpha) s|): two fp32 roundings of the magnitudes being added."""
    t, s, a = np.asarray(teacher, np.float64), np.asarray(student, np.float64), float(alpha)
    return 2.0 * 2.0 ** -24 * (np.abs(a * t) + np.abs((1.0 - a) * s))


def ema_alpha(step, ema_decay):
    return min(1.0 - 1.0 / (step + 1), float(ema_decay))


def entropy_threshold(ramp, num_classes):
    return (0.75 + 0.25 * float(ramp)) * math.log(num_classes)


def make_case(nb, k1, h, w, seed=None):
    """The generator of tests/test_gpu_consistency.py: logits 2 N(0,1), teacher = student + N(0,1), pbar = the mean of four
    soft-maxes of noisy copies of the teacher, rounded to fp32.  Returns fp32 arrays zs, zt, pbar [nb, k1, h, w]."""
    rng = np.random.default_rng(1000 * k1 + h + w if seed is None else seed)
    zs = (2.0 * rng.standard_normal((nb, k1, h, w))).astype(np.float32)
    zt = (zs + rng.standard_normal((nb, k1, h, w))).astype(np.float32)
    pbar = np.mean([softmax(zt + rng.standard_normal((nb, k1, h, w))) for _ in range(4)], axis=0).astype(np.float32)
    return zs, zt, pbar


def thresholds(k1):
    """0.75 ln K and 0.875 ln K, rounded to fp32 (as the device reads them)."""
    return [float(np.float32(f * math.log(k1))) for f in (0.75, 0.875)]
