"""float64 numpy restatement of bidirectional copy-paste (csrc/bcp.hip, losses/copy_paste.py), for the tests.

Mask: ones with one zero box.  Mix: out = mask != 0 ? fg : bg.  Loss, for logits z [B, K, H, W], label maps ya, yb [B, H, W] and a mask
[H, W] or [B, H, W]; region A is mask != 0 and reads ya, region B is mask == 0 and reads yb; p = softmax(z); per region r

    I_rk = sum m_r p_k [y_r = k]   Z_rk = sum m_r p_k^2   Y_rk = sum m_r [y_r = k]   N_r = sum m_r      over all images and pixels
    D_r = (1/K) sum_k (1 - (2 I_rk + s) / (Z_rk + Y_rk + s))
    C_r = sum m_r (logsumexp(z) - z[y_r]) / (N_r + 1e-16)                 an empty region: D_r = C_r = 0
    L = wa (D_A + C_A) / 2 + wb (D_B + C_B) / 2
    dL/dz_j = (w_r/2) [ (p_j - [j = y_r]) / (N_r + 1e-16) + sum_k g_rk p_k ([k = j] - p_j) ]
    g_rk = -(1/K) (2 [y_r = k] / den_rk - 2 p_k (2 I_rk + s) / den_rk^2),  den_rk = Z_rk + Y_rk + s

A pixel reads only its own region's label.
"""
import numpy as np


def box_mask(h, w, ratio, y0, x0):
    """uint8 [h, w]: ones, zero on the int(h ratio) x int(w ratio) box whose top-left corner is (y0, x0)."""
    bh, bw = int(h * ratio), int(w * ratio)
    assert 0 <= y0 <= h - bh and 0 <= x0 <= w - bw
    m = np.ones((h, w), np.uint8)
    m[y0:y0 + bh, x0:x0 + bw] = 0
    return m


def find_box(mask):
    """(y0, x0, bh, bw) of the zero set of a mask if that set is exactly one axis-aligned box (bh = bw = 0: no zero), else None."""
    zero = np.asarray(mask) == 0
    if not zero.any():
        return 0, 0, 0, 0
    ys, xs = np.where(zero.any(1))[0], np.where(zero.any(0))[0]
    y0, y1, x0, x1 = ys[0], ys[-1] + 1, xs[0], xs[-1] + 1
    full = np.zeros_like(zero)
    full[y0:y1, x0:x1] = True
    return (int(y0), int(x0), int(y1 - y0), int(x1 - x0)) if np.array_equal(full, zero) else None


def mix(fg, bg, mask):
    """mask != 0 ? fg : bg; mask [H, W] or [B, H, W] against [B, C, H, W]."""
    m = np.asarray(mask) != 0
    m = m[None, None] if m.ndim == 2 else m[:, None]
    return np.where(m, fg, bg)


def softmax(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def evaluate(z, ya, yb, mask, wa=1.0, wb=1.0, s=1e-10):
    """dict in float64: value; terms = [D_A, C_A, D_B, C_B]; counts = (N_A, N_B); grad [B, K, H, W]; and the magnitudes the GPU tests'
    bounds multiply:
      term_mags  = [magD_A, magC_A, magD_B, magC_B],  magC_r = sum m_r (1 + |z_y - max z|) / N_r  (the CPS one),
                   magD_r = (1/K) sum_k (2 I_rk / den_rk + (2 I_rk + s) Z_rk / den_rk^2)   (a relative error of I and Z through the quotient)
      value_mag  = wa (magD_A + magC_A) / 2 + wb (magD_B + magC_B) / 2
      grad_mag   = the sum of the absolute values of the gradient's terms, per element:
                   (w_r/2) [ (p_j + [j = y_r]) / (N_r + 1e-16) + p_j (a_j + b_j) + p_j sum_k (a_k + b_k) p_k ],
                   a_k = (1/K) 2 [y_r = k] / den_rk, b_k = (1/K) 2 p_k (2 I_rk + s) / den_rk^2"""
    z = np.asarray(z, np.float64)
    b, k, h, w = z.shape
    m = np.asarray(mask) != 0
    m = np.broadcast_to(m if m.ndim == 3 else m[None], (b, h, w))
    y = np.where(m, np.asarray(ya).reshape(b, h, w).astype(np.int64), np.asarray(yb).reshape(b, h, w).astype(np.int64))
    assert ((y >= 0) & (y < k)).all(), "the restatement takes in-range selected labels"
    p = softmax(z)
    mx = z.max(1)
    lse = mx + np.log(np.exp(z - mx[:, None]).sum(1))
    zy = np.take_along_axis(z, y[:, None], 1)[:, 0]
    onehot = (np.arange(k)[None, :, None, None] == y[:, None]).astype(np.float64)
    terms, mags, counts = [], [], []
    grad = np.zeros_like(z)
    grad_mag = np.zeros_like(z)
    for mr, wr in ((m, float(wa)), (~m, float(wb))):
        n = int(mr.sum())
        counts.append(n)
        if n == 0:
            terms += [0.0, 0.0]
            mags += [0.0, 0.0]
            continue
        mf = mr.astype(np.float64)[:, None]
        inter = (mf * p * onehot).sum((0, 2, 3))
        zz = (mf * p * p).sum((0, 2, 3))
        yy = (mf * onehot).sum((0, 2, 3))
        num, den = 2.0 * inter + s, zz + yy + s
        terms += [float((1.0 - num / den).mean()), float((mf[:, 0] * (lse - zy)).sum() / (n + 1e-16))]
        mags += [float((2.0 * inter / den + num * zz / den ** 2).mean()), float((mf[:, 0] * (1.0 + np.abs(zy - mx))).sum() / n)]
        a = (2.0 / (k * den))[None, :, None, None] * onehot
        bq = (2.0 * num / (k * den ** 2))[None, :, None, None] * p
        g = -(a - bq)
        ce = (p - onehot) / (n + 1e-16)
        grad += 0.5 * wr * mf * (ce + p * (g - (g * p).sum(1, keepdims=True)))
        grad_mag += 0.5 * wr * mf * ((p + onehot) / (n + 1e-16) + p * (a + bq) + p * ((a + bq) * p).sum(1, keepdims=True))
    value = wa * (terms[0] + terms[1]) / 2 + wb * (terms[2] + terms[3]) / 2
    value_mag = wa * (mags[0] + mags[1]) / 2 + wb * (mags[2] + mags[3]) / 2
    return dict(value=float(value), terms=terms, counts=tuple(counts), grad=grad, term_mags=mags, value_mag=float(value_mag),
                grad_mag=grad_mag)


# ---------------------------------------------------------------- case generators
def make_mask(nb, h, w, per_image=False, seed=5):
    """A 2/3 box mask at a drawn corner ([h, w], or [nb, h, w] with a corner per image and 255 for "one"); where the image is too small
    for a box (int(h 2/3) int(w 2/3) == 0) random bytes, so that both regions are populated whenever there are two pixels."""
    rng = np.random.default_rng(seed + 17 * h + w)
    bh, bw = int(h * 2 / 3), int(w * 2 / 3)

    def one():
        if bh * bw == 0:
            m = (rng.random((h, w)) < 0.5).astype(np.uint8)
            if h * w > 1:
                m.reshape(-1)[0], m.reshape(-1)[-1] = 1, 0
            return m
        return box_mask(h, w, 2 / 3, int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1)))

    if not per_image:
        return one()
    return np.stack([one() for _ in range(nb)]) * np.uint8(255)


def make_case(nb, k1, h, w, seed=11, absent=False):
    """(z fp32 with a spread of a few units, ya, yb int64 in [0, k1)).  absent: the last class never occurs in yb (nor class 0 in ya),
    so a class is absent from a region whatever the mask."""
    rng = np.random.default_rng(seed + 1000 * k1 + h * w)
    z = (2.5 * rng.standard_normal((nb, k1, h, w))).astype(np.float32)
    ya = rng.integers(0, k1, (nb, h, w))
    yb = rng.integers(0, k1, (nb, h, w))
    if absent and k1 > 1:
        ya[ya == 0] = k1 - 1
        yb[yb == k1 - 1] = 0
    return z, ya.astype(np.int64), yb.astype(np.int64)


def saturated_case(nb, k1, h, w, seed=3):
    """Logits of +-80: every soft-max is one-hot in fp32, half of the labels disagree with it (terms of 160)."""
    rng = np.random.default_rng(seed)
    top = rng.integers(0, k1, (nb, h, w))
    z = np.full((nb, k1, h, w), -80.0, np.float32)
    np.put_along_axis(z, top[:, None], 80.0, 1)
    ya = np.where(rng.random((nb, h, w)) < 0.5, top, (top + 1) % k1).astype(np.int64)
    yb = np.where(rng.random((nb, h, w)) < 0.5, top, (top + 1) % k1).astype(np.int64)
    return z, ya, yb
