"""float64 numpy restatement of weak-to-strong consistency (csrc/w2s.hip, losses/weak_strong.py), for the tests.  Written from the
definition, not from the kernel.

Code: for weak logits zw [B, K, H, W] and a threshold tau, y = argmax_k zw_k on the logits as given (ties to the lowest index),
keep = [max_k softmax(zw)_k >= tau], code = y | keep << 7.

Mix: out[n] = mask[n or 0] != 0 ? x[perm[n]] : x[n].

Loss: strong logits zs [B, K, H, W], code [B, H, W], mask [H, W] or [B, H, W], perm [B]; mask or perm None: no mix.  For pixel (n, p):
c = code[mask[n][p] ? perm[n] : n][p], y = c & 7, m = c >> 7 (a label >= K: not kept), q = softmax(zs), N = B H W,

    CE  = (1/N) sum m (logsumexp(zs) - zs[y])
    I_k = sum m q_k [y = k]   Z_k = sum m q_k^2   Y_k = sum m [y = k]
    D   = (1/K) sum_k (1 - (2 I_k + s) / (Z_k + Y_k + s))                 no kept pixel: 0
    L   = weight (ce_w CE + dice_w D)
    dL/dzs_j = m [ cec (q_j - [j = y]) + q_j (g_j - sum_k g_k q_k) ],  cec = weight ce_w / N,
    g_k = -(weight dice_w / K) (2 [y = k] / den_k - 2 q_k (2 I_k + s) / den_k^2),  den_k = Z_k + Y_k + s
    counts = (sum m, pixels whose mask byte is set)
"""
import numpy as np


def softmax(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def labels(z):
    """argmax over the class axis of the logits AS GIVEN (no conversion: the comparison is on the fp32 values themselves)."""
    return np.argmax(np.asarray(z), axis=1)


def max_prob(z):
    """max_k softmax(z)_k in float64, [B, H, W]."""
    return softmax(z).max(1)


def encode(y, keep):
    return (np.asarray(y).astype(np.int64) | (np.asarray(keep).astype(np.int64) << 7)).astype(np.uint8)


def decode(code):
    c = np.asarray(code).astype(np.int64)
    return c & 7, ((c >> 7) & 1).astype(bool)


def code_of(zw, tau):
    """The code map of weak logits at threshold tau, with the float64 confidence."""
    return encode(labels(zw), max_prob(zw) >= float(tau))


def _mask_b(mask, b, h, w):
    m = np.asarray(mask) != 0
    return np.broadcast_to(m if m.ndim == 3 else m[None], (b, h, w))


def mix(x, perm, mask):
    """mask != 0 ? x[perm] : x for x [B, C, H, W] of any dtype (the bits of the chosen operand)."""
    x = np.asarray(x)
    b, _, h, w = x.shape
    return np.where(_mask_b(mask, b, h, w)[:, None], x[np.asarray(perm)], x)


def select(code, mask, perm):
    """(the code byte that supervises every pixel, the number of pixels whose mask byte is set)."""
    code = np.asarray(code)
    if mask is None or perm is None:
        return code, 0
    m = _mask_b(mask, *code.shape)
    return np.where(m, code[np.asarray(perm)], code), int(m.sum())


def evaluate(zs, code, mask=None, perm=None, weight=1.0, ce_w=1.0, dice_w=0.0, s=1e-10):
    """dict in float64: value, ce, dice, counts = (kept, pasted), grad [B, K, H, W], and the magnitudes the GPU tests' bounds multiply:
      ce_mag    = (1/N) sum m (1 + |zs_y - max zs|)                                  the CPS one
      dice_mag  = (1/K) sum_k (2 I_k / den_k + (2 I_k + s) Z_k / den_k^2)            the BCP quotient one
      value_mag = weight (ce_w ce_mag + dice_w dice_mag)
      grad_mag  = the sum of the absolute values of the gradient's terms, per element:
                  m [ cec (q_j + [j = y]) + q_j (a_j + b_j) + q_j sum_k (a_k + b_k) q_k ],
                  a_k = (weight dice_w / K) 2 [y = k] / den_k,  b_k = (weight dice_w / K) 2 q_k (2 I_k + s) / den_k^2"""
    z = np.asarray(zs, np.float64)
    b, k, h, w = z.shape
    n_all = float(b * h * w)
    c, pasted = select(code, mask, perm)
    y, keep = decode(c)
    keep = keep & (y < k)
    ysafe = np.where(y < k, y, 0)
    mf = keep.astype(np.float64)
    q = softmax(z)
    mx = z.max(1)
    lse = mx + np.log(np.exp(z - mx[:, None]).sum(1))
    zy = np.take_along_axis(z, ysafe[:, None], 1)[:, 0]
    onehot = (np.arange(k)[None, :, None, None] == ysafe[:, None]).astype(np.float64)
    ce = float((mf * (lse - zy)).sum() / n_all)
    ce_mag = float((mf * (1.0 + np.abs(zy - mx))).sum() / n_all)
    cec = weight * ce_w / n_all
    grad = cec * mf[:, None] * (q - onehot)
    grad_mag = cec * mf[:, None] * (q + onehot)
    kept = int(keep.sum())
    dice = dice_mag = 0.0
    if kept > 0:
        mk = mf[:, None]
        inter = (mk * q * onehot).sum((0, 2, 3))
        zz = (mk * q * q).sum((0, 2, 3))
        yy = (mk * onehot).sum((0, 2, 3))
        num, den = 2.0 * inter + s, zz + yy + s
        dice = float((1.0 - num / den).mean())
        dice_mag = float((2.0 * inter / den + num * zz / den ** 2).mean())
        wd = weight * dice_w
        a = wd * (2.0 / (k * den))[None, :, None, None] * onehot
        bq = wd * (2.0 * num / (k * den ** 2))[None, :, None, None] * q
        g = -(a - bq)
        grad = grad + mk * q * (g - (g * q).sum(1, keepdims=True))
        grad_mag = grad_mag + mk * (q * (a + bq) + q * ((a + bq) * q).sum(1, keepdims=True))
    return dict(value=float(weight * (ce_w * ce + dice_w * dice)), ce=ce, dice=dice, counts=(kept, pasted), grad=grad, ce_mag=ce_mag,
                dice_mag=dice_mag, value_mag=float(weight * (ce_w * ce_mag + dice_w * dice_mag)), grad_mag=grad_mag)


# ---------------------------------------------------------------- case generators
SCALES = (5.0, 0.7, 2.0)


def make_case(nb, k1, h, w, seed=None, absent=False):
    """(zw, zs) fp32: weak logits scale * N(0, 1) with the scale cycling over SCALES from image to image (confidences from near
    one-hot to near uniform), strong logits = weak + 1.5 N(0, 1).  Class 0 of the first pixel of the first image gets + 8, so that
    even a one-pixel case keeps a pixel at the thresholds below.  absent: the last class is never the weak arg-max."""
    rng = np.random.default_rng(2000 * k1 + 3 * h + w if seed is None else seed)
    sc = np.array([SCALES[n % len(SCALES)] for n in range(nb)])[:, None, None, None]
    zw = (sc * rng.standard_normal((nb, k1, h, w))).astype(np.float32)
    zw[0, 0, 0, 0] = zw[0, :, 0, 0].max() + np.float32(8.0)  # before the strong logits are derived: they follow it
    zs = (zw + 1.5 * rng.standard_normal((nb, k1, h, w))).astype(np.float32)
    if absent and k1 > 1:
        zw[:, k1 - 1] = -30.0
    return zw, zs


def tie_case(nb, k1, h, w, seed=7):
    """Logits 0.5 * randint(-2, 3), as tests/_cps_ref.py: many pixels have a tied top-2, and the confidences take few values."""
    rng = np.random.default_rng(seed)
    zw = (0.5 * rng.integers(-2, 3, (nb, k1, h, w))).astype(np.float32)
    zs = (0.5 * rng.integers(-2, 3, (nb, k1, h, w))).astype(np.float32)
    return zw, zs


def saturated_case(nb, k1, h, w, seed=3):
    """Weak and strong logits of +-80: every soft-max is one-hot in fp32, and half of the strong tops differ from the weak label
    (terms of 160 whose label has a soft-max of 0 in fp32)."""
    rng = np.random.default_rng(seed)
    top = rng.integers(0, k1, (nb, h, w))
    zw = np.full((nb, k1, h, w), -80.0, np.float32)
    np.put_along_axis(zw, top[:, None], 80.0, 1)
    other = np.where(rng.random((nb, h, w)) < 0.5, top, (top + 1) % k1)
    zs = np.full((nb, k1, h, w), -80.0, np.float32)
    np.put_along_axis(zs, other[:, None], 80.0, 1)
    return zw, zs


def thresholds():
    """0.6 and 0.9 rounded to fp32 (as the device reads them): away from the few confidence values of the tie case."""
    return [float(np.float32(0.6)), float(np.float32(0.9))]


def ambiguous(zw, tau):
    """Pixels whose float64 confidence lies within 1e-6 of tau: the only ones where a device flag may differ."""
    return np.abs(max_prob(zw) - float(tau)) < 1e-6


def make_mask(nb, h, w, kind, seed=5):
    """None ("none"), or a CutMix mask with a box of about half the height and 0.6 of the width at a drawn corner: [h, w] with 1 inside
    ("hw") or [nb, h, w] with a corner per image and 255 inside ("bhw").  Where the image is too small for a box, random bytes with
    both values present whenever there are two pixels."""
    if kind == "none":
        return None
    rng = np.random.default_rng(seed + 17 * h + w)
    bh, bw = int(h * 0.5), int(w * 0.6)

    def one():
        m = np.zeros((h, w), np.uint8)
        if bh * bw == 0:
            m = (rng.random((h, w)) < 0.5).astype(np.uint8)
            if h * w > 1:
                m.reshape(-1)[0], m.reshape(-1)[-1] = 1, 0
            return m
        y0, x0 = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1))
        m[y0:y0 + bh, x0:x0 + bw] = 1
        return m

    if kind == "hw":
        return one()
    assert kind == "bhw"
    return np.stack([one() for _ in range(nb)]) * np.uint8(255)


def make_perm(nb, kind):
    """None ("none"), the identity, the reverse, or ("fixed") a permutation that keeps image 0 and rotates the others by one."""
    if kind == "none":
        return None
    if kind == "identity":
        return np.arange(nb)
    if kind == "reverse":
        return np.arange(nb)[::-1].copy()
    assert kind == "fixed"
    return np.concatenate([[0], np.roll(np.arange(1, nb), 1)]).astype(np.int64)


# what tests/test_gpu_w2s.py runs, shared with the host test of the ambiguity cap
SHAPES = [(1, 1, 1), (2, 1, 7), (4, 37, 61), (2, 336, 544)]
K1S = [2, 3, 8]
