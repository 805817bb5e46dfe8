"""Float64 restatement of the tail of a training step (test infrastructure only): the 1x1 segmentation head and the head fused with
the last block's norm + LeakyReLU (csrc/head.hip), the norm backward fed by the head (csrc/norm.hip, mia_norm_act_bwd_head[_w])
and the fused Dice + cross-entropy loss (csrc/dice_ce.hip), plus the seeded case tables that tests/test_head_loss_host.py (CPU) and
tests/test_gpu_head_loss.py (GPU) share.  Activations are NHWC with the pixels flattened, [N, P, C]; logits and their gradient
are [N, P, K].

    head        logits = x W^T + b         dx = dl W         dW = dl^T x         db = sum dl
    fused head  x = lrelu(scale y + shift) first (per-(n, c) rows), then the same formulas
    head-fed norm backward: _norm_ref.norm_act(y, gamma, beta, dz = dl W, ...), whose dy, dgamma, dbeta, dbias, c1, c2, v are reused
    Dice + CE   p = softmax(v) (or v), t = one-hot(label) (or a dense target); per (image b, class k):
                I = sum_p p t,  S = sum_p p (p^2 if squared),  T = sum_p t (t^2 if squared);  batch: the three are averaged over b
                dice = mean over the kept (b, k) of 1 - (2 I + smooth) / (S + T + smooth)       (classes kb.., kb = 0 with do_bg else 1)
                ce = mean over all pixels of sum_k t_k (logsumexp(v) - v_k)
                out = (ce_w ce + dice_w dice, ce, dice)
                coef[b, k] = (alpha, beta) = d dice / d(I_b,k, S_b,k) = (-2 / den, num / den^2) / (kept count)   (0 for k < kb)
                d dice / d p_k = alpha t_k + beta (2 p_k if squared else 1) =: g_k
                dlogits_k = gout (dice_w (p_k (g_k - sum_j g_j p_j) if softmax else g_k) + ce_w / (B P) ((sum_j t_j) softmax_k - t_k))

The kernels take W, b, scale, shift, smooth and the loss weights as fp32: the inputs made here are rounded once to fp32 (activations
once to their storage dtype) and both sides consume those numbers."""
import functools

import numpy as np
import torch

import _norm_ref as N

f64, lrelu, DT = N.f64, N.lrelu, N.DT
HW = N.HW_RAGGED                         # 1961 pixels: ragged for every lane count and slab count used here
SMOOTH = float(np.float32(1e-5))
f32r = lambda t: t.float().double()      # round once to fp32


# ------------------------------------------------------------------ head
def head(x, w, b, dl=None):
    """logits [N, P, K] of x [N, P, C]; with dl also dx, dW, db."""
    x, w, b = f64(x), f64(w), f64(b)
    out = dict(logits=x @ w.T + b)
    if dl is not None:
        dl = f64(dl)
        out.update(dx=dl @ w, dw=torch.einsum("npk,npc->kc", dl, x), db=dl.sum((0, 1)))
    return out


def head_norm(y, scale, shift, slope, w, b, dl=None):
    """The head on x = lrelu(scale y + shift) with per-(n, c) rows scale / shift [N, C]."""
    x = lrelu(f64(scale)[:, None, :] * f64(y) + f64(shift)[:, None, :], slope)
    out = head(x, w, b, dl)
    out["x"] = x
    return out


def head_fed_norm_bwd(y, gamma, beta, w, dl, mode, m=None, slope=N.SLOPE, training=True, running=None):
    """norm_act with dz = dl W, plus the head's own dW / db on the block's activated output z."""
    w, dl = f64(w), f64(dl)
    r = N.norm_act(y, gamma, beta, dl @ w, mode, m=m, slope=slope, training=training, running=running)
    r["dw"] = torch.einsum("npk,npc->kc", dl, r["z"])
    r["db"] = dl.sum((0, 1))
    return r


# ------------------------------------------------------------------ Dice + CE
def dice_ce(logits, target, softmax=True, do_bg=True, batch=False, squared=False, smooth=SMOOTH, dice_w=1.0, ce_w=1.0, gout=1.0):
    """Closed form of the loss and its gradient.  logits [B, P, K]; target: int labels [B, P] or a dense float target [B, P, K].
    Returns sums [B, K, 3], coef [B, K, 2], out [3], dlogits [B, P, K]."""
    v = f64(logits)
    nb, npx, k1 = v.shape
    if target.dtype in (torch.int64, torch.int32):
        t = torch.nn.functional.one_hot(target.long(), k1).double()
    else:
        t = f64(target)
    sm = torch.softmax(v, -1)
    p = sm if softmax else v
    I, S, T = (p * t).sum(1), (p * p if squared else p).sum(1), (t * t if squared else t).sum(1)
    sums = torch.stack([I, S, T], -1)
    kb = 0 if do_bg else 1
    nk = k1 - kb
    if batch:
        Ib, Sb, Tb = I.mean(0, keepdim=True), S.mean(0, keepdim=True), T.mean(0, keepdim=True)
        num, den = 2 * Ib + smooth, Sb + Tb + smooth
        dice = (1 - num / den)[:, kb:].sum() / nk
        alpha, beta = (-(2 / den) / nb / nk).expand(nb, k1), (num / den ** 2 / nb / nk).expand(nb, k1)
    else:
        num, den = 2 * I + smooth, S + T + smooth
        dice = (1 - num / den)[:, kb:].sum() / (nb * nk)
        alpha, beta = -(2 / den) / (nb * nk), num / den ** 2 / (nb * nk)
    coef = torch.stack([alpha, beta], -1).clone()
    coef[:, :kb] = 0.0
    ce = (t * (torch.logsumexp(v, -1, keepdim=True) - v)).sum() / (nb * npx)
    out = torch.stack([ce_w * ce + dice_w * dice, ce, dice])
    g = coef[:, None, :, 0] * t + coef[:, None, :, 1] * (2 * p if squared else torch.ones_like(p))
    dd = sm * (g - (g * sm).sum(-1, keepdim=True)) if softmax else g
    dc = (t.sum(-1, keepdim=True) * sm - t) / (nb * npx)
    return dict(sums=sums, coef=coef, out=out, dlogits=gout * (dice_w * dd + ce_w * dc))


# ------------------------------------------------------------------ seeded inputs
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * (hash(k) if isinstance(k, int) else sum(map(ord, str(k)))) for i, k in enumerate(key)) % (2 ** 31))


def head_inputs(dt, c0, k1, n, hw, seed=0):
    """x [n, hw, c0] on a grid of 1/8 (exact in bf16 and fp32), dl [n, hw, k1] fp32, W / b fp32."""
    g = _gen("head", dt, c0, k1, n, hw, seed)
    x = torch.randint(-24, 25, (n, hw, c0), generator=g).double() / 8
    w = f32r(torch.randn(k1, c0, generator=g).double() / np.sqrt(c0))
    b = f32r(torch.randn(k1, generator=g).double())
    dl = f32r(torch.randn(n, hw, k1, generator=g).double())
    return dict(x=x, w=w, b=b, dl=dl)


def fused_inputs(dt, c0, k1, n, hw, seed=0):
    """y in the storage dtype, fp32 rows scale / shift with one (n, c) row of scale exactly 0, W / b / dl fp32."""
    g = _gen("fused", dt, c0, k1, n, hw, seed)
    y = (torch.randn(n, hw, c0, generator=g).double() * 1.5 + torch.randn(c0, generator=g).double()).to(DT[dt]).double()
    scale = f32r(torch.randn(n, c0, generator=g).double() * 0.8)
    scale[n - 1, 1] = 0.0
    shift = f32r(torch.randn(n, c0, generator=g).double() * 0.5)
    w = f32r(torch.randn(k1, c0, generator=g).double() / np.sqrt(c0))
    b = f32r(torch.randn(k1, generator=g).double())
    dl = f32r(torch.randn(n, hw, k1, generator=g).double())
    return dict(y=y, scale=scale, shift=shift, w=w, b=b, dl=dl)


def fed_key(c, dt, mode, k1, n=3, hw=HW, frozen=False):
    return (c, dt, mode, k1, n, hw, frozen)


def fed_inputs(key):
    """Inputs of one head-fed norm-backward case, built like _norm_ref.make_inputs (pre-activations kept away from the LeakyReLU kink:
    |y - mu| in [0.7, 1.4] channel scales, |mu| <= 0.3, beta opposite to mu) with the gradient replaced by fp32 logits gradients and a
    head weight.  tests/test_head_loss_host.py checks the outcome for every key of fed_cases()."""
    c, dt, mode, k1, n, hw, frozen = key
    gen = _gen("fed", *key)
    q = lambda t: t.to(DT[dt]).double()
    sgn = lambda *s: torch.where(torch.rand(*s, generator=gen) < 0.5, -1.0, 1.0).double()
    sigma = 0.5 + 1.5 * torch.rand(c, generator=gen).double()
    mu = sgn(c) * (0.1 + 0.2 * torch.rand(c, generator=gen).double())
    y = q(sigma * (mu + sgn(n, hw, c) * (0.7 + 0.7 * torch.rand(n, hw, c, generator=gen).double())))
    gamma = f32r(0.8 + 0.4 * torch.rand(c, generator=gen).double())
    beta = f32r(-torch.sign(mu) * (0.1 + 0.1 * torch.rand(c, generator=gen).double()))
    m = N.drop_mask(gen, n, c)
    running = None
    if mode == "batch":
        running = (f32r(sigma * (mu + 0.1)), f32r(1.5 * sigma * sigma * 1.15))
    w = f32r(torch.randn(k1, c, generator=gen).double() / np.sqrt(c))
    dl = f32r(torch.randn(n, hw, k1, generator=gen).double())
    return dict(y=y, gamma=gamma, beta=beta, m=m, running=running, w=w, dl=dl)


@functools.lru_cache(maxsize=2)
def fed_reference(key):
    """(inputs, answer) of one head-fed case, computed once and shared; callers leave both unchanged."""
    c, dt, mode, k1, n, hw, frozen = key
    i = fed_inputs(key)
    return i, head_fed_norm_bwd(i["y"], i["gamma"], i["beta"], i["w"], i["dl"], mode, m=i["m"], training=not frozen, running=i["running"])


def loss_inputs(nb, hw, k1, seed=0, softmax=True, dense=False, special=None):
    """fp32 logits [nb, hw, k1] (N(0, 2) for softmax; probabilities in (0, 1) when the kernel is told not to apply it) and int64 labels
    [nb, hw], or a dense fp32 target [nb, hw, k1] of soft class probabilities.
    special = "absent": class k1 - 1 does not occur in image 0's labels;  "unpredicted": class 0 is nowhere the arg-max;
    "one_class": every label of image nb - 1 is class 1."""
    g = _gen("loss", nb, hw, k1, seed, softmax, dense, special)
    logits = f32r(torch.randn(nb, hw, k1, generator=g).double() * 2) if softmax else f32r(0.02 + 0.96 * torch.rand(nb, hw, k1, generator=g).double())
    labels = torch.randint(0, k1, (nb, hw), generator=g)
    if special == "absent":
        labels[0] = torch.randint(0, k1 - 1, (hw,), generator=g)
    elif special == "unpredicted":
        logits[..., 0] = f32r(logits[..., 1:].max(-1).values - 1.0)
    elif special == "one_class":
        labels[nb - 1] = 1
    else:
        assert special is None
    if dense:
        return logits, f32r(torch.softmax(torch.randn(nb, hw, k1, generator=g).double() * 2, -1))
    return logits, labels


BAD_LABELS = ("k1", -1, 2 ** 32 + 1)     # a label equal to the class count, a negative one, and a valid low word under a set high word


def bad_labels(labels, k1, which):
    """A copy of labels [nb, hw] with ONE bad value at (nb - 1, 5) (hw >= 8: inside the second quad of the image)."""
    out = labels.clone()
    out[-1, 5] = k1 if which == "k1" else which
    return out


# ------------------------------------------------------------------ the shared case tables
FAST_C0 = {"f32": (16, 32, 64), "bf16": (32, 64, 128)}          # 4 / 8 / 16 sixteen-byte units per pixel
FUSED_C0 = {"f32": (16, 32, 48, 64), "bf16": (32, 64, 96, 128)}  # 4 / 8 / 12 / 16 units
FAST_K1 = (2, 3, 4)
CAPPED = ("f32", 64, 3, 1, 887 * 887)    # head forward with the fast kernel's grid capped at 16384 blocks: the one large case
MAX_CASE_BYTES = 16 << 20


def head_fwd_cases():
    """(dtype, c0, k1, n, hw, logits layout, x misaligned)"""
    out = []
    for dt in DT:
        for c0 in FAST_C0[dt]:
            for k1 in FAST_K1:
                out.append((dt, c0, k1, 2, HW, "cl", False))                       # 18 fast instantiations, paired loop + tail
    out += [("f32", 64, 3, 1, 15, "cl", False), ("bf16", 32, 2, 1, 15, "cl", False)]     # npix < 2 * LANES
    for dt, c0 in (("f32", 12), ("f32", 40), ("bf16", 16)):
        for k1 in (1, 5, 8):
            out.append((dt, c0, k1, 2, HW, "cl", False))                           # generic kernel, 16-byte loads
    for dt, c0 in (("f32", 7), ("bf16", 7), ("bf16", 12), ("bf16", 20)):
        for k1 in (3, 8):
            out.append((dt, c0, k1, 2, HW, "cl", False))                           # generic kernel, scalar loads
    out.append(("f32", 12, 3, 2, 362 * 363, "cl", False))                          # generic kernel's 8192-block cap
    for dt, c0, k1 in (("f32", 32, 3), ("bf16", 128, 4), ("f32", 12, 5), ("bf16", 20, 2)):
        out += [(dt, c0, k1, 3, HW, "nchw", False), (dt, c0, k1, 2, HW, "pad", False)]
    for dt, c0 in (("f32", 32), ("f32", 12), ("f32", 7), ("bf16", 64), ("bf16", 16), ("bf16", 20)):
        out.append((dt, c0, 3, 2, HW, "cl", True))                                 # x one element into its buffer
    return out


def head_bwd_cases():
    """(dtype, c0, k1, n, hw, dl layout, misaligned tensor or None)"""
    out = []
    for dt in DT:
        for c0 in FAST_C0[dt]:
            for k1 in FAST_K1:
                out += [(dt, c0, k1, 2, HW, "cl", None), (dt, c0, k1, 2, HW, "nchw", None)]
    out += [("f32", 32, 3, 1, 37, "cl", None), ("bf16", 32, 2, 2, 300 * 301, "cl", None)]  # one weight block; the 2048-block cap
    for dt, c0 in (("f32", 12), ("f32", 40), ("f32", 128), ("f32", 252), ("bf16", 16), ("bf16", 248)):
        for k1 in (1, 3, 5, 8):
            out.append((dt, c0, k1, 2, HW, "cl", None))                            # *_vec_kernel
    for dt, c0 in (("f32", 7), ("bf16", 7), ("bf16", 12), ("bf16", 20), ("f32", 4), ("f32", 256), ("f32", 300)):
        for k1 in (3, 8):
            out.append((dt, c0, k1, 2, HW, "cl", None))                            # scalar generic kernels
    out.append(("f32", 300, 2, 3, HW, "nchw", None))
    for dt, c0 in (("f32", 32), ("bf16", 64), ("f32", 40)):
        out += [(dt, c0, 3, 2, HW, "cl", "x"), (dt, c0, 3, 2, HW, "cl", "dx")]
    return out


HEAD_OPTION_CASES = (("f32", 32, 3), ("bf16", 64, 4), ("f32", 40, 5), ("bf16", 16, 2), ("f32", 7, 3), ("bf16", 20, 8))  # fast / vec / scalar


def fused_cases():
    """(dtype, c0, k1, n, hw, logits or dl layout, slope) of mia_head_norm_fwd / mia_head_norm_wgrad"""
    out = []
    for dt in DT:
        for c0 in FUSED_C0[dt]:
            for k1 in FAST_K1:
                for hw in (195, 1024, HW):
                    out.append((dt, c0, k1, 3, hw, "cl", N.SLOPE))
                out.append((dt, c0, k1, 3, HW, "nchw", N.SLOPE))
            out.append((dt, c0, 3, 3, HW, "cl", 1.0))
    return out


FED_CHANNELS = (32, 64, 96, 128, 160)       # CG = 32: 32, 96, 160;  CG = 64: 64, 128
FED_STREAM = (("f32", 288), ("bf16", 288))  # fp32: 72 units on 64 per block, gy = 2; bf16: 36 of 64 lanes live
LONG_SLAB = N.LONG_SLAB


def fed_cases():
    """Every input set whose dy a GPU test compares: (channels, dtype, mode, k1, images, pixels, frozen)."""
    keys = []
    for c in FED_CHANNELS:
        for dt in DT:
            for k1 in FAST_K1:
                keys.append(fed_key(c, dt, "instance", k1))
            keys.append(fed_key(c, dt, "batch", 3))
    for dt, c in FED_STREAM:
        keys.append(fed_key(c, dt, "instance", 3))
    for dt in DT:
        for k1 in (2, 4):
            keys.append(fed_key(64, dt, "batch", k1))
        keys.append(fed_key(64, dt, "batch", 3, frozen=True))
        keys.append(fed_key(64, dt, "instance", 3, LONG_SLAB["n"], LONG_SLAB["hw"]))
    return keys


LOSS_FAST_HW = ((1964, 1), (1964, 3), (1964, 7), (6000, 1), (36, 4))   # (pixels, slabs); 491 quads; 1500 quads; 9 quads on 4 slabs
LOSS_FLAGS = tuple((s, d, b, q) for s in (True, False) for d in (True, False) for b in (False, True) for q in (False, True))
LOSS_WEIGHTS = ((0.6, 0.9), (1.0, 0.0), (0.0, 1.0))
LOSS_GOUT = 0.375
# every (images, pixels, classes) a loss test of tests/test_gpu_head_loss.py runs
LOSS_SHAPES = (tuple(sorted({(3, hw, k1) for hw, _ in LOSS_FAST_HW for k1 in FAST_K1}))  # fast, refusals, weights, hand-built, bad labels
               + ((3, 1961, 3), (3, 1964, 1), (3, 1964, 5), (3, 1964, 8))                # generic
               + ((3, 144, 3), (40, 16, 8), (70, 16, 4)))                                # flags, finalize loops


def case_bytes():
    """{case id: bytes of its largest input tensor} over every table (CAPPED excluded)."""
    esz = {"f32": 4, "bf16": 2}
    out = {}
    for name, cases in (("fwd", head_fwd_cases()), ("bwd", head_bwd_cases()), ("fused", fused_cases())):
        for k in cases:
            out[(name,) + k] = k[3] * k[4] * max(k[1] * esz[k[0]], k[2] * 4)
    for k in fed_cases():
        out[("fed",) + k] = k[4] * k[5] * k[0] * esz[k[1]]
    for nb, hw, k1 in LOSS_SHAPES:  # fp32 logits / dense target [nb, hw, k1] or int64 labels [nb, hw]
        out[("loss", nb, hw, k1)] = nb * hw * max(k1 * 4, 8)
    return out
