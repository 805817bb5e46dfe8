"""Restatements, in float64 or exact integer arithmetic on the CPU, of what every training step runs besides the convs, norms and
losses: clip-by-global-norm and the Adam / AdamW / SGD update over the flat buffers (csrc/optim.hip) and the weight packing, fp16
splitting, maxima, relayout, column sums, residual add, Dropout2d masks and label feed helpers of csrc/pack.hip.  They are written
from the definitions (torch.optim's documented updates, Random123's Philox4x32-10, `dst[t][n][k] = w[n][k][t]`), not from the
kernels' loops; what IS taken from the kernels is the launch geometry the rounding counts `k` of the bounds depend on.

Bounds.  u = 2^-24 is the unit roundoff of fp32 (round to nearest).  An expression made of sums and products of fp32 leaves, where
the path from a leaf to the result crosses at most k roundings, is off by at most k u sum |terms| to first order; every bound below
is such a sum, with the count of each path written next to it, plus ONE ulp of the stored result, which covers the second-order
terms and results in the subnormal range.  A fused multiply-add rounds once where the counts assume twice, so contraction can only
help.  Division and square root are correctly rounded in the library's build (no fast-math flag): one rounding each.
"""
import math
import struct

import numpy as np

U = 2.0 ** -24
ADAM, ADAMW, SGD = 0, 1, 2  # include/mia_hip.h MIA_OPT_*
KINDS = {"adam": ADAM, "adamw": ADAMW, "sgd": SGD}
F = np.float32
M32 = np.uint64(0xFFFFFFFF)


def ulp32(x):
    """Spacing of fp32 at |x| (2^-149 at zero), as float64."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ================================================================== optimizer (csrc/optim.hip)
def kernel_scalars(lr, beta1, beta2, eps, wd, step, clip1=1.0, grad_scale=1.0):
    """The fp32 scalars `ops.optim_step` hands the kernel at step `step`, as float64 numbers: the bias corrections are formed in
    double from the Python betas and rounded once, cs = float32(clip[1]) * float32(grad_scale) is ONE fp32 product (clip1 = 1 when
    no clip buffer is passed).  `clip1` / `grad_scale` are kept for the wrong variants of `step_f32`."""
    cs = F(clip1) * F(grad_scale)
    assert cs.dtype == np.float32
    return dict(lr=float(F(lr)), beta1=float(F(beta1)), beta2=float(F(beta2)), eps=float(F(eps)), wd=float(F(wd)),
                bc1=float(F(1.0 - beta1 ** step)), bc2=float(F(1.0 - beta2 ** step)), cs=float(cs),
                clip1=float(F(clip1)), grad_scale=float(F(grad_scale)))


def step(kind, p, g, m, v, s, first):
    """One update in float64 from the scalars `s` (kernel_scalars, or plain doubles for the comparison with torch.optim).

        g' = cs g (+ wd p: Adam and SGD, "coupled" decay)
        SGD:    m' = g' on the first step, beta1 m + g' after;  p' = p - lr m'
        Adam:   m' = beta1 m + (1 - beta1) g',  v' = beta2 v + (1 - beta2) g'^2,
                p' = p (1 - lr wd: AdamW only) - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)

    Returns dict(p, m, v, bound_p, bound_m, bound_v) (v entries None for SGD).  Rounding counts, per leaf-to-result path (1 - beta
    is exact in fp32 for beta in [1/2, 1], Sterbenz, asserted here):
      g'      kg = 1 (g cs), 2 with coupled decay (+ the product wd p and the sum);        G = |g cs| + |wd p|
      SGD m'  km = kg on the first step (stored as it is), kg + 1 after (the sum; beta1 m: 2) M = beta1 |m| + G
      SGD p'  the p leaf 1 (the subtraction), the m' leaf km + 2 (lr m', the subtraction): u |p| + (km + 2) u lr M
      Adam m' km = kg + 2 ((1 - beta1) g', the sum; beta1 m: 2);                            M = beta1 |m| + (1 - beta1) G
      Adam v' kv = 2 kg + 3 (two factors g', two products, the sum; beta2 v: 2);            V = beta2 |v| + (1 - beta2) G^2
      Adam p' the kernel takes the square root of the STORED v', so its error Ev = bound_v moves sqrt(v') by at most
              min(Ev / sqrt(v'), sqrt(Ev)); then with S = sqrt(v') / sqrt(bc2), D = S + eps, T = (lr / bc1) m' / D:
                ED = that / sqrt(bc2) + 3 u S (sqrt, sqrt(bc2), the division) + u D (the sum)
                ET = (lr / bc1) (bound_m / D + |m'| ED / (D (D - ED))) + 3 u |T| (lr / bc1, m' / D, their product)
              AdamW's p (1 - lr wd): 3 roundings (lr wd, 1 - x, the product) on |p| (1 + lr wd); the subtraction u (|p_eff| + |T|)."""
    p, g, m = (np.asarray(a, np.float64) for a in (p, g, m))
    lr, b1, b2, eps, wd, bc1, bc2, cs = (s[k] for k in ("lr", "beta1", "beta2", "eps", "wd", "bc1", "bc2", "cs"))
    for b in (b1,) if kind == SGD else (b1, b2):
        if isinstance(b, float) and float(F(b)) == b:  # the fp32 scalars of a kernel comparison
            assert float(F(1) - F(b)) == 1.0 - b, "1 - beta is not exact in fp32"
    gc = g * cs
    coupled = wd != 0.0 and kind != ADAMW
    gi = gc + wd * p if coupled else gc
    G = np.abs(gc) + np.abs(wd * p) if coupled else np.abs(gc)
    kg = 2 if coupled else 1
    if kind == SGD:
        if first:
            m2, M, km = gi, G, kg
        else:
            m2, M, km = b1 * m + gi, b1 * np.abs(m) + G, kg + 1
        p2 = p - lr * m2
        return dict(p=p2, m=m2, v=None, bound_m=km * U * M + ulp32(m2), bound_v=None,
                    bound_p=U * np.abs(p) + (km + 2) * U * lr * M + ulp32(p2))
    v = np.asarray(v, np.float64)
    c1, c2 = 1.0 - b1, 1.0 - b2
    pe = p * (1.0 - lr * wd) if kind == ADAMW else p
    m2, M, km = b1 * m + c1 * gi, b1 * np.abs(m) + c1 * G, kg + 2
    v2, V, kv = b2 * v + c2 * gi * gi, b2 * np.abs(v) + c2 * G * G, 2 * kg + 3
    bound_m, bound_v = km * U * M + ulp32(m2), kv * U * V + ulp32(v2)
    sv, sb = np.sqrt(v2), math.sqrt(bc2)
    S = sv / sb
    D = S + eps
    T = (lr / bc1) * m2 / D
    with np.errstate(divide="ignore", invalid="ignore"):
        esv = np.minimum(np.where(sv > 0, bound_v / sv, np.inf), np.sqrt(bound_v))
        ED = esv / sb + 3 * U * S + U * D
        inv = np.where(D > ED, ED / (D * (D - ED)), np.inf)
        ET = (lr / bc1) * (bound_m / D + np.abs(m2) * inv) + 3 * U * np.abs(T)
    p2 = pe - T
    bound_p = (3 * U * np.abs(p) * (1.0 + lr * wd) if kind == ADAMW else 0.0) + ET + U * (np.abs(pe) + np.abs(T)) + ulp32(p2)
    return dict(p=p2, m=m2, v=v2, bound_p=bound_p, bound_m=bound_m, bound_v=bound_v)


# what a subtly wrong kernel would do; (name, kinds it applies to, needs first_step)
VARIANTS = [("wd_dropped", (ADAM, ADAMW, SGD), None), ("adamw_coupled", (ADAMW,), None), ("eps_in_sqrt", (ADAM, ADAMW), None),
            ("bc2_not_rooted", (ADAM, ADAMW), None), ("bc1_omitted", (ADAM, ADAMW), None), ("sgd_first_momentum", (SGD,), True),
            ("clip_ignored", (ADAM, ADAMW, SGD), None), ("grad_scale_twice", (ADAM, ADAMW, SGD), None),
            ("stale_m", (ADAM, ADAMW, SGD), None)]


def step_f32(kind, p, g, m, v, s, first, variant=None):
    """The same formulas evaluated operation by operation in numpy float32, in the textbook order and without fused multiply-adds
    (variant = None), or one of the wrong VARIANTS.  Returns (p', m', v') as float32 arrays (v' None for SGD)."""
    p, g, m = (np.asarray(a, np.float32) for a in (p, g, m))
    lr, b1, b2, eps, wd, bc1, bc2 = (F(s[k]) for k in ("lr", "beta1", "beta2", "eps", "wd", "bc1", "bc2"))
    cs = F(s["clip1"]) * F(s["grad_scale"])
    one = F(1)
    if variant == "clip_ignored":
        cs = F(s["grad_scale"])
    elif variant == "grad_scale_twice":
        cs = cs * F(s["grad_scale"])
    elif variant == "wd_dropped":
        wd = F(0)
    elif variant == "adamw_coupled":
        kind = ADAM
    gi = g * cs
    pi = p
    if kind == SGD:
        if wd != 0:
            gi = gi + wd * pi
        buf = gi if (first and variant != "sgd_first_momentum") else b1 * m + gi
        p2 = pi - lr * (m if variant == "stale_m" else buf)
        assert p2.dtype == buf.dtype == np.float32
        return p2, buf, None
    v = np.asarray(v, np.float32)
    if kind == ADAMW:
        pi = pi * (one - lr * wd)
    elif wd != 0:
        gi = gi + wd * pi
    mi = b1 * m + (one - b1) * gi
    vi = b2 * v + (one - b2) * gi * gi
    if variant == "eps_in_sqrt":
        denom = np.sqrt(vi / bc2 + eps)
    elif variant == "bc2_not_rooted":
        denom = np.sqrt(vi) / bc2 + eps
    else:
        denom = np.sqrt(vi) / np.sqrt(bc2) + eps
    size = lr if variant == "bc1_omitted" else lr / bc1
    p2 = pi - size * ((m if variant == "stale_m" else mi) / denom)
    assert p2.dtype == mi.dtype == vi.dtype == np.float32
    return p2, mi, vi


def optim_case(n, seed):
    """fp32 (p, m, v) that make every term of the update larger than rounding AND let the eps-sized differences show: element i
    lives at a scale s_i = 10^U(-4, 0); m ~ s N, v = s^2 (0.5 + U) >= 0; p ~ s N on even elements (so that the coupled decay wd p
    does not drown a small gradient there) and ~ 4 N on odd ones."""
    rng = np.random.default_rng(seed)
    sc = 10.0 ** rng.uniform(-4.0, 0.0, n)
    p = np.where(np.arange(n) % 2 == 0, sc, 4.0) * rng.standard_normal(n)
    m = sc * rng.standard_normal(n)
    v = sc * sc * (0.5 + rng.random(n))
    return p.astype(np.float32), m.astype(np.float32), v.astype(np.float32), sc


def optim_grad(sc, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return (scale * sc * rng.standard_normal(sc.shape[0])).astype(np.float32)


def grad_norm(g, grad_scale):
    """float64 grad_scale ||g||_2 with the fp32 grad_scale the kernel receives."""
    g = np.asarray(g, np.float64)
    return float(F(grad_scale)) * math.sqrt(float((g * g).sum()))


def grad_norm_blocks(n):
    q = (n // 4 + 255) // 256
    return q + 1 if q < 1024 else 1024


def grad_norm_bound(n, nrm):
    """Every term of sum g^2 is positive, so the bound is relative.  Longest path of a square to a block's partial sum: its own
    product (1), the three additions inside its quad (3), one addition into the thread's running sum per loop trip, L =
    ceil(quads / threads) of them, one for the thread's tail element (1), and the two 64-lane butterflies of block_sum (6 + 6):
    k = 17 + L.  The fold over blocks is in double.  sqrt halves a relative error; the conversion of the root to fp32 and the product
    with grad_scale add one rounding each: |error| <= nrm u (k / 2 + 2) + 1 ulp."""
    loops = -(-(n // 4) // (256 * grad_norm_blocks(n)))
    k = 17 + loops
    return abs(nrm) * U * (k / 2 + 2) + float(ulp32(nrm))


def clip_coef_f32(nrm32, max_norm):
    """min(1, max_norm / (norm + 1e-6)) in numpy float32 from the DEVICE's norm; 1 when max_norm <= 0."""
    if max_norm <= 0:
        return F(1)
    with np.errstate(invalid="ignore"):
        c = F(max_norm) / (F(nrm32) + F(1e-6))
        return F(1) if c > F(1) else c


def dyn_bytes(lr, bc1, bc2, first, seed, offset):
    return struct.pack("<4f2Q", lr, bc1, bc2, 1.0 if first else 0.0, seed, offset)


# ================================================================== packing (csrc/pack.hip)
def pad_to(v, m):
    return (v + m - 1) // m * m


def pack_weight(w, n_from_d0, npad, kpad):
    """w: fp32 torch tensor [D0, D1, kh, kw] -> [taps, npad, kpad] fp32, dst[t][n][k] = w[n][k][t] (n_from_d0) or w[k][n][t], zero
    padded; the bf16 form is `.to(torch.bfloat16)` of it."""
    import torch
    d0, d1 = w.shape[0], w.shape[1]
    w3 = w.detach().cpu().reshape(d0, d1, -1)
    nk = w3 if n_from_d0 else w3.permute(1, 0, 2)
    out = torch.zeros(w3.shape[2], npad, kpad, dtype=torch.float32)
    out[:, :nk.shape[0], :nk.shape[1]] = nk.permute(2, 0, 1)
    return out


def amax_bits(x):
    """Bit pattern of max |x| over an fp32 array as an unsigned integer maximum (NaN patterns order above infinity)."""
    return int((bits32(x).reshape(-1) & np.uint32(0x7FFFFFFF)).max())


def split_exponent(amax_pattern):
    return min(120, 141 - ((int(amax_pattern) >> 23) & 0xFF))


def split_f16(x, amax_pattern):
    """Words h | l << 16 of x 2^e: h = fp16(x 2^e), l = fp16(x 2^e - h), both round-to-nearest-even with subnormals kept."""
    xs = np.asarray(x, np.float32) * F(2.0 ** split_exponent(amax_pattern))
    with np.errstate(over="ignore"):
        h = xs.astype(np.float16)
        l = (xs - h.astype(np.float32)).astype(np.float16)
    return h.view(np.uint16).astype(np.uint32) | (l.view(np.uint16).astype(np.uint32) << np.uint32(16))


# ================================================================== column sums
def colsum_blocks(p):
    return max(1, min(256, p // 64))


def colsum_k(p, c, bf16, vector, accumulate):
    """Additions on the longest path of one element to out[c].  The rows are cut into B = clamp(p / 64, 1, 256) blocks of per =
    ceil(p / B); a block's `lanes` threads per channel stride over them (ceil(per / lanes) additions each), one thread adds the
    lanes' sums in turn (lanes), the final kernel's 16 lanes per channel stride over the B partial rows (ceil(B / 16)) and are added
    in turn (16); accumulate adds one.  lanes: vector route 16 (fp32) / 32 (bf16); generic route 256 / min(c, 256)."""
    b = colsum_blocks(p)
    per = -(-p // b)
    lanes = (32 if bf16 else 16) if vector else 256 // min(c, 256)
    return -(-per // lanes) + lanes + -(-b // 16) + 16 + (1 if accumulate else 0)


# ================================================================== Dropout2d masks
def philox4x32_10(ctr, key):
    """Random123 Philox4x32-10.  ctr: four uint64 arrays (or scalars) holding 32-bit words, key: two 32-bit words; returns four
    uint64 arrays of 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & M32 for c in ctr)
    k0, k1 = np.uint64(key[0]) & M32, np.uint64(key[1]) & M32
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # 32 x 32 -> 64 bits, no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def dropout_mask(n, keep, seed, offset):
    """Element 4 q + e is word e of Philox(counter = (q lo, q hi, offset lo, offset hi), key = seed's words); it survives, with the
    value float32(1) / float32(keep), when its top 24 bits / 2^24 < float32(keep)."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    offset, seed = int(offset) & (2 ** 64 - 1), int(seed) & (2 ** 64 - 1)
    z = np.zeros_like(q)
    words = philox4x32_10((q & M32, q >> np.uint64(32), z + np.uint64(offset & 0xFFFFFFFF), z + np.uint64(offset >> 32)),
                          (seed & 0xFFFFFFFF, seed >> 32))
    w = np.stack(words, 1).reshape(-1)[:n]
    u = (w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return np.where(u < float(F(keep)), F(1) / F(keep), F(0)).astype(np.float32)
