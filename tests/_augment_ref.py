"""Float64 restatement of the augmentation / resize / normalisation kernels (csrc/augment.hip) for tests/test_augment_host.py (which
checks it against torch on the CPU) and tests/test_gpu_augment.py (which checks the kernels against it), plus the seeded inputs and case
tables the two share.  numpy only.

Written from the operations' definitions (the header comments of csrc/augment.hip and the reference lines they cite).  VALUES are
accumulated in float64.  What the definitions do in fp32 -- the source index of nearest / nearest-exact / bilinear resizing, the tap range
of the antialiased filter, the Philox uniforms ((c >> 8) + 0.5f) * 2^-24 and the angle 6.2831853f * u -- is done in numpy.float32, one
rounded operation at a time, so that a kernel and this file can differ by accumulation order, by a fused multiply-add where the compiler
forms one, and by the device's libm only.  Affine and
elastic source indices are not restated here: oracle/transforms_ref.py has them bit-exact already.

Apply flags (selected-sample mode): 1 = transform the sample, 0 = copy it through, -1 = skip it (the output keeps what it held)."""
import numpy as np

f32, f64 = np.float32, np.float64
EW_GAMMA, EW_CONTRAST, EW_NOISE, EW_ZSCORE = 0, 1, 2, 3
GRID_CAP = 8192 * 256  # work items one launch covers before its grid-stride loop takes a second trip
SENTINEL = -7.0


# --------------------------------------------------------------------------- inputs
def image(shape, seed, bits=10):
    """Seeded image in [0, 1] whose values are multiples of 2^-bits (exact in fp32, exact under power-of-two scaling)."""
    g = np.random.default_rng(seed)
    return (g.integers(0, 2 ** bits + 1, size=shape).astype(f64) / 2 ** bits).astype(f32)


def batch_of(base, nb):
    """[nb, C, H, W] cheap variations of one [C, H, W] base image: sample b is the base rolled by (3 b + 1, 5 b + 2) pixels and scaled by
    (nb + b) / (2 nb), so that no two samples agree and a wrong sample index changes the answer."""
    return np.stack([(np.roll(base, (3 * b + 1, 5 * b + 2), axis=(-2, -1)).astype(f64) * ((nb + b) / (2.0 * nb))).astype(f32)
                     for b in range(nb)])


def with_flags(ref, x, apply, sentinel=SENTINEL):
    """Expected output of a stage under apply flags: `ref` where the flag is 1, the input where 0, the sentinel where -1."""
    out = np.array(ref, dtype=f64, copy=True)
    for b, a in enumerate(apply):
        if a == 0:
            out[b] = x[b]
        elif a < 0:
            out[b] = sentinel
    return out


# --------------------------------------------------------------------------- gaussian blur
def gauss1d(k, sigma):
    """torchvision _get_gaussian_kernel1d: exp(-0.5 (j / sigma)^2) on j = -(k - 1) / 2 .. (k - 1) / 2, normalised."""
    j = np.arange(k, dtype=f64) - (k - 1) * 0.5
    w = np.exp(-0.5 * (j / f64(f32(sigma))) ** 2)
    return w / w.sum()


def blur(x, sigma, ksize):
    """F.gaussian_blur per sample: k x k outer-product kernel on the reflect-padded image.  x [B, C, H, W]."""
    x = np.asarray(x, dtype=f64)
    out = np.empty_like(x)
    h, w = x.shape[-2:]
    for b in range(x.shape[0]):
        k = int(ksize[b])
        r = k // 2
        w1 = gauss1d(k, sigma[b])
        pad = np.pad(x[b], ((0, 0), (r, r), (r, r)), mode="reflect")
        acc = np.zeros_like(x[b])
        for i in range(k):
            for j in range(k):
                acc += (w1[i] * w1[j]) * pad[:, i:i + h, j:j + w]
        out[b] = acc
    return out


# --------------------------------------------------------------------------- statistics / element-wise
LUMA = tuple(f64(f32(v)) for v in (0.2989, 0.587, 0.114))  # torchvision rgb_to_grayscale, fp32 constants


def sample_stats(x, gray=False):
    """[B, 2] = (mean, unbiased std) over C*H*W of each sample, two-pass in float64 (n = 1: std 0); gray with C == 3: of the luma."""
    x = np.asarray(x, dtype=f64)
    out = np.zeros((x.shape[0], 2), dtype=f64)
    for b in range(x.shape[0]):
        v = (LUMA[0] * x[b, 0] + LUMA[1] * x[b, 1] + LUMA[2] * x[b, 2]) if (gray and x.shape[1] == 3) else x[b]
        v = v.reshape(-1)
        m = v.sum() / v.size
        out[b, 0] = m
        out[b, 1] = np.sqrt(((v - m) ** 2).sum() / (v.size - 1)) if v.size > 1 else 0.0
    return out


def elementwise(x, op, p0=None, mean_std=None, aux=None):
    """The four intensity ops on [B, ...]: gamma x^p0[b]; contrast clamp(f x + (1 - f) mean[b], 0, 1); noise clamp(x + aux, 0, 1);
    z-score (x - mean[b]) / max(std[b], 1e-8).  p0 is taken as the fp32 numbers the kernel gets, mean_std as given (fp32 rows to
    restate the op alone, float64 rows of `sample_stats` for the true result)."""
    x = np.asarray(x, dtype=f64)
    bs = (-1,) + (1,) * (x.ndim - 1)
    if op == EW_GAMMA:
        return np.power(x, np.asarray(p0, dtype=f32).astype(f64).reshape(bs))
    if op == EW_CONTRAST:
        f = np.asarray(p0, dtype=f32).astype(f64).reshape(bs)
        m = np.asarray(mean_std, dtype=f64)[:, 0].reshape(bs)
        return np.clip(f * x + (1.0 - f) * m, 0.0, 1.0)
    if op == EW_NOISE:
        return np.clip(x + np.asarray(aux, dtype=f64), 0.0, 1.0)
    ms = np.asarray(mean_std, dtype=f64)
    return (x - ms[:, 0].reshape(bs)) / np.maximum(ms[:, 1], f64(f32(1e-8))).reshape(bs)


# --------------------------------------------------------------------------- Philox4x32-10 and the noise
M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Random123 Philox4x32 with 10 rounds.  ctr [..., 4] and key (k0, k1) of 32-bit words -> [..., 4] uint32."""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    lo = np.uint64(MASK)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 -> 64 bits, no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & lo]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def uniforms(words):
    """((c >> 8) + 0.5f) * 2^-24 in fp32, as specified: the sum rounds to even above 2^23."""
    return ((words >> np.uint32(8)).astype(f32) + f32(0.5)) * f32(1.0 / 16777216.0)


TWO_PI_F32 = f32(6.2831853)


def noise_normals(quads, seed, offset):
    """[Q, 4] float64 standard normals of the quads `quads` (int64 indices): counter (quad lo, quad hi, offset lo, offset hi), key
    (seed lo, seed hi); Box-Muller on the pairs (u0, u1) and (u2, u3): sqrt(-2 ln u0) (cos, sin)(6.2831853f * u1)."""
    q = np.asarray(quads, dtype=np.int64)
    ctr = np.stack([q & MASK, q >> 32, np.full_like(q, offset & MASK), np.full_like(q, (offset >> 32) & MASK)], axis=-1)
    u = uniforms(philox4x32_10(ctr, (seed & MASK, (seed >> 32) & MASK)))
    assert u.dtype == f32
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0].astype(f64))), np.sqrt(-2.0 * np.log(u[:, 2].astype(f64)))
    a1, a3 = (TWO_PI_F32 * u[:, 1]).astype(f64), (TWO_PI_F32 * u[:, 3]).astype(f64)  # fp32 products
    return np.stack([r0 * np.cos(a1), r0 * np.sin(a1), r1 * np.cos(a3), r1 * np.sin(a3)], axis=-1)


def noise_z(total, seed, offset):
    """The normal that element i of a batch of `total` elements gets: lane i % 4 of quad i // 4 (the quads run over the whole batch)."""
    quads = (total + 3) // 4
    return noise_normals(np.arange(quads, dtype=np.int64), seed, offset).reshape(-1)[:total]


def noise_clip(x, sigma, seed, offset):
    """clamp(x + sigma[b] * z, 0, 1) on [B, ...]."""
    x = np.asarray(x, dtype=f64)
    z = noise_z(x.size, seed, offset).reshape(x.shape)
    sg = np.asarray(sigma, dtype=f32).astype(f64).reshape((-1,) + (1,) * (x.ndim - 1))
    return np.clip(x + sg * z, 0.0, 1.0)


# --------------------------------------------------------------------------- resize
def nearest_index(isz, osz, exact=False, arithmetic=f32):
    """Source index of every output index: legacy nearest min(floor(dst * in / out), in - 1); nearest-exact
    min(floor((dst + 0.5) * in / out), in - 1).  The definition is fp32 arithmetic (`arithmetic=f64` is there to find the sizes at
    which that matters)."""
    scale = arithmetic(isz) / arithmetic(osz)
    d = np.arange(osz).astype(arithmetic)
    if exact:
        d = d + arithmetic(0.5)
    return np.minimum(np.floor(d * scale).astype(np.int64), isz - 1)


def bilinear_index(isz, osz):
    """area_pixel_compute_source_index (align_corners=False) in fp32: s = max(scale * (dst + 0.5) - 0.5, 0), i0 = int(s),
    i1 = i0 + (i0 < in - 1), weight of i1 = s - i0.  Returns (i0, i1, weight as float64)."""
    scale = f32(isz) / f32(osz)
    s = scale * (np.arange(osz).astype(f32) + f32(0.5))  # rounded product ...
    s = np.maximum(s - f32(0.5), f32(0.0))               # ... then the subtraction
    i0 = s.astype(np.int64)
    i1 = i0 + (i0 < isz - 1)
    lam = s - i0.astype(f32)
    assert s.dtype == f32 and lam.dtype == f32
    return i0, i1, lam.astype(f64)


def resize_bilinear(x, oh, ow):
    """interpolate(bilinear, align_corners=False) on the last two axes."""
    x = np.asarray(x, dtype=f64)
    y0, y1, ly = bilinear_index(x.shape[-2], oh)
    x0, x1, lx = bilinear_index(x.shape[-1], ow)
    ly = ly[:, None]
    top = (1.0 - lx) * x[..., y0, :][..., x0] + lx * x[..., y0, :][..., x1]
    bot = (1.0 - lx) * x[..., y1, :][..., x0] + lx * x[..., y1, :][..., x1]
    return (1.0 - ly) * top + ly * bot


def resize_bilinear_adjoint(dout, h, w):
    """Adjoint of resize_bilinear: din[.., h, w] = scatter of dout[.., oh, ow] with the same four weights.  Returns (din, A, K), A =
    the same scatter of |weight * dout| and K [h, w] = the number of output pixels with a non-zero weight on each input pixel: what the fp32 error
    of a scatter in arbitrary order is bounded by."""
    g = np.asarray(dout, dtype=f64)
    oh, ow = g.shape[-2:]
    y0, y1, ly = bilinear_index(h, oh)
    x0, x1, lx = bilinear_index(w, ow)
    lead = g.shape[:-2]
    g2 = g.reshape(-1, oh, ow)
    din = np.zeros((g2.shape[0], h, w), dtype=f64)
    mag = np.zeros_like(din)
    cnt = np.zeros((h, w), dtype=np.int64)
    for yy, wy, first_y in ((y0, 1.0 - ly, True), (y1, ly, False)):
        for xx, wx, first_x in ((x0, 1.0 - lx, True), (x1, lx, False)):
            wgt = wy[:, None] * wx[None, :]
            iy, ix = np.broadcast_to(yy[:, None], (oh, ow)), np.broadcast_to(xx[None, :], (oh, ow))
            for p in range(g2.shape[0]):
                np.add.at(din[p], (iy, ix), wgt * g2[p])
                np.add.at(mag[p], (iy, ix), np.abs(wgt * g2[p]))
            new = ((first_y | (y1 != y0))[:, None] & (first_x | (x1 != x0))[None, :]) & (wgt != 0)  # a corner met twice counts once
            np.add.at(cnt, (iy[new], ix[new]), 1)
    return din.reshape(lead + (h, w)), mag.reshape(lead + (h, w)), cnt


def aa_taps(isz, osz):
    """Antialiased (triangle) filter of torch's _upsample_bilinear2d_aa along one axis: per output index the tap range [lo, hi) --
    fp32 arithmetic: centre = scale * (o + 0.5), lo = max(int(centre - support + 0.5), 0), hi = min(int(centre + support + 0.5), in)
    with support = max(scale, 1) -- and the normalised float64 weights max(0, 1 - |(j - centre + 0.5) / support|)."""
    scale = f32(isz) / f32(osz)
    support = scale if scale >= f32(1.0) else f32(1.0)
    invscale = f32(1.0) / scale if scale >= f32(1.0) else f32(1.0)
    centre = scale * (np.arange(osz).astype(f32) + f32(0.5))
    lo = np.maximum(((centre - support) + f32(0.5)).astype(np.int64), 0)
    hi = np.minimum(((centre + support) + f32(0.5)).astype(np.int64), isz)
    assert centre.dtype == f32
    taps = []
    for o in range(osz):
        j = np.arange(lo[o], hi[o])
        wt = np.maximum(1.0 - np.abs((j.astype(f64) - f64(centre[o]) + 0.5) * f64(invscale)), 0.0)
        taps.append((j, wt / wt.sum() if wt.sum() != 0 else wt))
    return taps


def _aa_axis(x, osz, axis):
    x = np.moveaxis(x, axis, -1)
    out = np.empty(x.shape[:-1] + (osz,), dtype=f64)
    for o, (j, wt) in enumerate(aa_taps(x.shape[-1], osz)):
        out[..., o] = (x[..., j] * wt).sum(-1)
    return np.moveaxis(out, -1, axis)


def resize_aa(x, oh, ow):
    """interpolate(bilinear, antialias=True): the separable filter along W, then along H."""
    return _aa_axis(_aa_axis(np.asarray(x, dtype=f64), ow, -1), oh, -2)


def resize_nearest(x, oh, ow):
    """interpolate(nearest) on the last two axes, any element type."""
    x = np.asarray(x)
    return x[..., nearest_index(x.shape[-2], oh), :][..., nearest_index(x.shape[-1], ow)]


def lowres(x, low_hw):
    """SimulateLowRes: sample b seen through a nearest-exact downsample to low_hw[b], then bilinear back to its own size."""
    x = np.asarray(x, dtype=f64)
    h, w = x.shape[-2:]
    out = np.empty_like(x)
    for b, (lh, lw) in enumerate(low_hw):
        low = x[b][..., nearest_index(h, lh, exact=True), :][..., nearest_index(w, lw, exact=True)]
        out[b] = resize_bilinear(low, h, w)
    return out


# --------------------------------------------------------------------------- rot90 / flips / crop
def rot90_flip(x, k, flip_h, flip_w):
    """torch.rot90(x, k, (-2, -1)), then the flips of the rotated image's H / W axes."""
    out = np.rot90(np.asarray(x), k, axes=(-2, -1))
    if flip_h:
        out = np.flip(out, -2)
    if flip_w:
        out = np.flip(out, -1)
    return np.ascontiguousarray(out)


def crop(x, top, left, oh, ow):
    x = np.asarray(x)
    return np.stack([x[b, ..., top[b]:top[b] + oh, left[b]:left[b] + ow] for b in range(x.shape[0])])


# --------------------------------------------------------------------------- case tables (shared by the host and the GPU tests)
# (id, (h, w), (oh, ow)): legacy nearest resizing at sizes where fp32 and exact index arithmetic disagree, both directions
NEAREST_CASES = [("up_6x4", (6, 4), (74, 82)), ("down_74x82", (74, 82), (6, 4)), ("odd_36x52", (36, 52), (17, 23))]
# in -> low sizes of the nearest-exact step of `lowres` where fp32 and exact arithmetic disagree: found by `nearest_disagreements`
# (tests/test_augment_host.py asserts that they do)
LOWRES_CASES = [("60x64", (60, 64), [(43, 41), (55, 47), (58, 49), (53, 55), (30, 32)], [1, 1, 0, -1, 1])]
BILINEAR_SIZES = [(72, 80), (17, 23), (1, 1), (36, 52), (37, 53)]       # from 36 x 52
AA_SIZES = [(17, 80), (72, 23), (36, 23), (5, 7), (1, 1)]               # from 36 x 52
BWD_CASES = [((9, 13), (36, 52)), ((36, 52), (9, 13)), ((7, 5), (16, 11)), ((1, 6), (4, 6)), ((6, 1), (6, 3)), ((8, 8), (8, 8))]
# (id, shape [B, C, H, W] or None for hand-built, gray)
STATS_CASES = [("n1", (2, 1, 1, 1), False), ("n35", (2, 1, 5, 7), False), ("n1961", (3, 1, 37, 53), False), ("luma", (2, 3, 36, 52), True),
               ("rand36x52", (2, 1, 36, 52), False)]
HARD_STATS = [("m0.9_s0.01", 0.9, 0.01), ("m0.9_s0.002", 0.9, 0.002), ("m1000_s30", 1000.0, 30.0)]  # 256 x 256, one image each
# (id, per_sample, nb, sigmas, seed, offset, apply): the noise cases
NOISE_CASES = [
    ("quad_spans_two", 6 * 7 + 1, 2, [0.03, 0.1], 1234, 1, None),            # per_sample = 43: quad 10 holds 40..42 of sample 0 and 0 of sample 1
    ("total_not_x4", 5 * 9, 3, [0.05, 0.02, 0.08], 7, 3, None),              # 135 elements: the last quad has three live lanes
    ("flags", 5 * 9, 4, [0.05, 0.02, 0.08, 0.04], 99, 0, [1, 0, -1, 1]),     # 45 per sample: quads span (1, 0), (0, -1), (-1, 1)
    ("high_words", 40 * 64, 2, [0.1, 0.06], 0xFEDCBA9876543210, (1 << 32) + 5, None),  # c3 = 1, k1 = 0xFEDCBA98
]


def nearest_disagreements(isz, osz, exact=False):
    """Output indices at which fp32 and float64 index arithmetic pick different source pixels."""
    return np.nonzero(nearest_index(isz, osz, exact, f32) != nearest_index(isz, osz, exact, f64))[0]


def stats_image(shape, seed):
    return image(shape, seed)


def hard_stats_image(mean, std, seed=0):
    """One 256 x 256 low-contrast / raw-intensity image: N(mean, std) rounded to fp32."""
    g = np.random.default_rng(seed)
    return (mean + std * g.standard_normal((1, 1, 256, 256))).astype(f32)
