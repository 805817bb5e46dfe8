"""Float64 numpy restatement of the pyramid consistency loss (test infrastructure only; csrc/urpc.hip,
losses/pyramid_consistency.py), with analytic gradients for every scale, plus the seeded inputs and case tables that
tests/test_urpc_host.py (CPU) and tests/test_gpu_urpc.py (GPU) share.

    U(n, f)   the [n f, n] matrix of torch's interpolate(scale_factor=f, mode="bilinear", align_corners=False) along one axis
    u_s       = Uy z_s Ux^T per (image, class); z_s itself for f_s = 1
    p_s, lp_s = softmax / log-softmax over the classes, lp = u - logsumexp(u);  m = (1/S) sum_s p_s
    v_s = sum_k [m_k log m_k - m_k lp_sk],  w_s = exp(-v_s),  D_s = sum_k (m_k - p_sk)^2
    sums[s] = (sum D_s w_s, sum w_s, sum v_s) over the P = N H W pixels
    L_s = (sums[s][0] / (P K)) / (sums[s][1] / P + 1e-8) + sums[s][2] / P,  L = mean_s L_s,  out = (weight L, L)

Gradient of gout * weight * L, term by term (no shortcut that the kernel's arrangement would share: the class-independent part of the
mean's gradient and sum_k m_k = 1 are NOT used here):
    dL/dv_s = [1/P - w_s (al_s D_s + be_s)] / S,  dL/dD_s = al_s w_s / S,  al_s = 1 / (P K b_s),  be_s = -a_s / (b_s^2 P)
    dL/dm_k = sum_s [dL/dv_s (log m_k + 1 - lp_sk) + dL/dD_s 2 (m_k - p_sk)]
    dL/dp_tk = dL/dm_k / S - dL/dD_t 2 (m_k - p_tk),   dL/dlp_tk = -dL/dv_t m_k
    dL/du_tk = p_tk (dL/dp_tk - sum_j dL/dp_tj p_tj) + dL/dlp_tk - p_tk sum_j dL/dlp_tj,   dz_t = Uy^T du_t Ux

Logits are [N, h, w, K] (class last, like _ds_loss_ref)."""
import functools

import numpy as np

FACTOR_SETS = ((1, 2), (1, 16), (1, 4, 16), (1, 2, 4, 8, 16), (1, 8, 2))
COARSE_HW = ((1, 1), (1, 5), (3, 3), (5, 7))   # in pixels of the coarsest scale: clamped taps, ragged tiles
ALL_K1 = (1, 2, 3, 4, 5, 8)
LAYOUTS = ("cl", "nchw", "pad")
DYN_WEIGHT = 0.37
GOUT = 0.625


def upsample_matrix(n, f):
    """U [n * f, n], float64."""
    dst = np.arange(n * f, dtype=np.float64)
    src = np.maximum((dst + 0.5) / f - 0.5, 0.0)
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    lam = src - i0
    u = np.zeros((n * f, n))
    rows = np.arange(n * f)
    np.add.at(u, (rows, i0), 1.0 - lam)
    np.add.at(u, (rows, i1), lam)
    return u


def upsample(z, f):
    """z [N, h, w, K] -> [N, h f, w f, K], float64."""
    z = np.asarray(z, dtype=np.float64)
    if f == 1:
        return z
    return np.einsum("Yy,byxk,Xx->bYXk", upsample_matrix(z.shape[1], f), z, upsample_matrix(z.shape[2], f))


def evaluate(zs, factors, weight=1.0, gout=1.0):
    """sums [S, 3], terms [S], out [2] = (weight L, L), dz: one [N, h_s, w_s, K] per scale, all float64."""
    s_n = len(zs)
    us = [upsample(z, f) for z, f in zip(zs, factors)]
    n, hh, ww, k1 = us[0].shape
    npix = float(n * hh * ww)
    lps = []
    for u in us:
        d = u - u.max(-1, keepdims=True)
        lps.append(d - np.log(np.exp(d).sum(-1, keepdims=True)))
    ps = [np.exp(lp) for lp in lps]
    m = sum(ps) / s_n
    assert (m > 0).all(), "float64 keeps every class of these inputs above 0"
    lm = np.log(m)
    ent = (m * lm).sum(-1)
    v = [ent - (m * lp).sum(-1) for lp in lps]
    w = [np.exp(-x) for x in v]
    d = [((m - p) ** 2).sum(-1) for p in ps]
    sums = np.array([[(d[s] * w[s]).sum(), w[s].sum(), v[s].sum()] for s in range(s_n)])
    a, b = sums[:, 0] / (npix * k1), sums[:, 1] / npix + 1e-8
    terms = a / b + sums[:, 2] / npix
    loss = terms.mean()
    scale = gout * weight / s_n
    al, be = 1.0 / (npix * k1 * b), -a / (b * b * npix)
    dv = [scale * (1.0 / npix - w[s] * (al[s] * d[s] + be[s])) for s in range(s_n)]
    dd = [scale * al[s] * w[s] for s in range(s_n)]
    dm = sum(dv[s][..., None] * (lm + 1.0 - lps[s]) + dd[s][..., None] * 2.0 * (m - ps[s]) for s in range(s_n))
    dz = []
    for t, f in enumerate(factors):
        dp = dm / s_n - dd[t][..., None] * 2.0 * (m - ps[t])
        dlp = -dv[t][..., None] * m
        du = ps[t] * (dp - (dp * ps[t]).sum(-1, keepdims=True)) + dlp - ps[t] * dlp.sum(-1, keepdims=True)
        if f == 1:
            dz.append(du)
        else:
            h, wd = zs[t].shape[1:3]
            dz.append(np.einsum("Yy,bYXk,Xx->byxk", upsample_matrix(h, f), du, upsample_matrix(wd, f)))
    return dict(sums=sums, terms=terms, out=np.array([weight * loss, loss]), dz=dz)


def make_case(nb, k1, ch, cw, factors, seed=0, amp=4.0):
    """Logits of every scale, seeded, on a grid of 1/8 in [-amp, amp] (exact in fp32), as float64 [nb, h_s, w_s, k1]; the full
    resolution is the coarsest factor times (ch, cw)."""
    top = max(factors)
    rng = np.random.default_rng(1000 * seed + 100 * k1 + 10 * ch + cw + 7 * len(factors) + top)
    n8 = int(round(amp * 8))
    return [rng.integers(-n8, n8 + 1, size=(nb, ch * top // f, cw * top // f, k1)).astype(np.float64) / 8.0 for f in factors]


@functools.lru_cache(maxsize=4)
def reference(key):
    """(zs, answer) of one case, computed once and shared; callers leave both unchanged.
    key = (nb, k1, ch, cw, factors, weight, gout, seed, amp); weight / gout None = 1."""
    nb, k1, ch, cw, factors, weight, gout, seed, amp = key
    zs = make_case(nb, k1, ch, cw, factors, seed, amp)
    w32 = 1.0 if weight is None else float(np.float32(weight))  # the kernels read the weight as an fp32 value
    g32 = 1.0 if gout is None else float(np.float32(gout))
    return zs, evaluate(zs, factors, w32, g32)


def key(nb, k1, ch, cw, factors, weight=None, gout=None, seed=0, amp=4.0):
    return (nb, k1, ch, cw, tuple(factors), weight, gout, seed, amp)


def shape_cases():
    """(nb, k1, ch, cw, factors, slabs): every factor set on every coarse shape; nb, k1 and the slab count rotate so that each
    factor set meets one, two and three slabs, both batch sizes and both class routes (compile-time 2, 3, 4; run-time 1, 5, 8)."""
    out = []
    i = 0
    for fs in FACTOR_SETS:
        for ch, cw in COARSE_HW:
            out.append((1 if i % 2 else 3, ALL_K1[i % len(ALL_K1)], ch, cw, fs, 1 + i % 3))
            i += 1
    # every class count on a shape with several gather tiles per scale and ragged last tiles
    for j, k1 in enumerate(ALL_K1):
        out.append((3 if j % 2 else 1, k1, 3, 5, (1, 2, 4, 8), 3))
    return out
