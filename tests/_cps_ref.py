"""float64 numpy restatement of cross pseudo supervision (csrc/cps.hip, losses/cross_pseudo.py), for the tests.

Logits za, zb [B, K, H, W], N = B H W:

    ya = argmax_k za_k, yb = argmax_k zb_k          on the logits as given (fp32 in the tests), ties to the lowest index
    ca = [max_k softmax(za)_k >= tau], cb likewise
    LA = (1/N) sum cb (logsumexp(za) - za[yb]),  LB = (1/N) sum ca (logsumexp(zb) - zb[ya])
    dLA/dza_j = (w/N) cb (pa_j - [j = yb]),  dLB/dzb_j = (w/N) ca (pb_j - [j = ya])
    counts = (sum ca, sum cb, sum [ya = yb]);  code = ya | yb << 3 | ca << 6 | cb << 7
"""
import numpy as np

import _consistency_ref as C


def labels(z):
    """argmax over the class axis of the logits AS GIVEN (no conversion: the comparison is on the fp32 values themselves)."""
    return np.argmax(np.asarray(z), axis=1)


def max_prob(z):
    """max_k softmax(z)_k in float64, [B, H, W]."""
    return C.softmax(z).max(1)


def flags(z, tau):
    return max_prob(z) >= float(tau)


def encode(ya, yb, ca, cb):
    return (ya | (yb << 3) | (ca.astype(np.int64) << 6) | (cb.astype(np.int64) << 7)).astype(np.uint8)


def decode(code):
    c = np.asarray(code).astype(np.int64)
    return c & 7, (c >> 3) & 7, ((c >> 6) & 1).astype(bool), ((c >> 7) & 1).astype(bool)


def _side(z, y, flag, w):
    """One direction: network with logits z learns label map y where `flag` is set.  -> (L, grad, value_mag, grad_mag)"""
    z = np.asarray(z, np.float64)
    b, k, h, wd = z.shape
    n = float(b * h * wd)
    mx = z.max(1)
    lse = mx + np.log(np.exp(z - mx[:, None]).sum(1))
    zy = np.take_along_axis(z, y[:, None], 1)[:, 0]
    m = np.asarray(flag).astype(np.float64)
    value = (m * (lse - zy)).sum() / n
    p = C.softmax(z)
    onehot = (np.arange(k)[None, :, None, None] == y[:, None]).astype(np.float64)
    grad = (w / n) * m[:, None] * (p - onehot)
    value_mag = (m * (1.0 + np.abs(zy - mx))).sum() / n
    grad_mag = (w / n) * m[:, None] * (p + onehot)
    return float(value), grad, float(value_mag), grad_mag


def evaluate(za, zb, tau=0.0, w=1.0, ca=None, cb=None):
    """dict(value_a, value_b, value, grad_a, grad_b, ya, yb, ca, cb, counts, code, value_mag_a, value_mag_b, grad_mag_a, grad_mag_b)
    in float64.  ca / cb: boolean maps [B, H, W] to use instead of the float64 flags (the tests pass the device's own).  `value` is
    w (LA + LB); the gradients carry w.  The magnitudes the tests' bounds are stated in:
      value_mag_A = (1/N) sum cb (1 + |za[yb] - max za|)        (the term is log sum exp(z - max) + (max - z_y), the first <= ln K)
      grad_mag    = (w/N) flag (p_j + [j = y])                  per element"""
    ya, yb = labels(za), labels(zb)
    ca = flags(za, tau) if ca is None else np.asarray(ca).astype(bool)
    cb = flags(zb, tau) if cb is None else np.asarray(cb).astype(bool)
    va, ga, vma, gma = _side(za, yb, cb, w)
    vb, gb, vmb, gmb = _side(zb, ya, ca, w)
    counts = (int(ca.sum()), int(cb.sum()), int((ya == yb).sum()))
    return dict(value_a=va, value_b=vb, value=w * (va + vb), grad_a=ga, grad_b=gb, ya=ya, yb=yb, ca=ca, cb=cb, counts=counts,
                code=encode(ya, yb, ca, cb), value_mag_a=vma, value_mag_b=vmb, grad_mag_a=gma, grad_mag_b=gmb)


def make_case(nb, k1, h, w, seed=None):
    """The generator of the consistency tests with its default seeds: za = its student logits, zb = its teacher logits (fp32)."""
    zs, zt, _ = C.make_case(nb, k1, h, w, seed)
    return zs, zt


def tie_case(nb, k1, h, w, seed=7):
    """Logits 0.5 * randint(-2, 3): many pixels have a tied top-2 (28 % at k1 = 3)."""
    rng = np.random.default_rng(seed)
    za = (0.5 * rng.integers(-2, 3, (nb, k1, h, w))).astype(np.float32)
    zb = (0.5 * rng.integers(-2, 3, (nb, k1, h, w))).astype(np.float32)
    return za, zb


def thresholds():
    """0.6 and 0.9, rounded to fp32 (as the device reads them)."""
    return [float(np.float32(0.6)), float(np.float32(0.9))]
