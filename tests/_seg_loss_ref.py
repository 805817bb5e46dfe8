"""Float64 restatement of the fold-trainer losses (test infrastructure only): masked soft Dice + weighted cross-entropy with an
ignore label, the hard tp / fp / fn of the arg-max prediction, and the top-k cross-entropy with this project's tie rule.

    valid = (label != ignore);  p = softmax(logits) or the logits;  t = onehot(label) where valid
    I = sum valid p t,  P = sum valid p,  G = sum valid t   per (image, class)
    dc = -mean_k (2 I + smooth) / max(G + P + smooth, 1e-8)     (class 0 dropped without do_bg; I, P, G summed over images with batch_dice)
    ce = sum valid w[label] nll / sum valid w[label],  0 when nothing is valid;   nll = logsumexp - logit[label]
    loss = w_ce ce + w_dice dc

Gradients come from autograd over these float64 expressions."""
import numpy as np
import torch


def _prep(logits, labels, ignore, weight):
    x = torch.as_tensor(np.asarray(logits), dtype=torch.float64).clone().requires_grad_(True)
    b, k1 = x.shape[:2]
    lab = torch.as_tensor(np.asarray(labels)).reshape(b, *x.shape[2:]).long()
    valid = torch.ones_like(lab, dtype=torch.bool) if ignore is None else lab != int(ignore)
    assert bool(((lab >= 0) & (lab < k1))[valid].all()), "a label is neither a class nor the ignore label"
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    onehot = torch.nn.functional.one_hot(safe, k1).movedim(-1, 1).to(torch.float64) * valid[:, None]
    w = torch.ones(k1, dtype=torch.float64) if weight is None else torch.as_tensor(np.asarray(weight), dtype=torch.float64)
    nll = (torch.logsumexp(x, 1) - torch.gather(x, 1, safe[:, None])[:, 0]) * w[safe] * valid
    return x, lab, valid, onehot, w, safe, nll


def hard_counts(logits, labels, ignore=None):
    """int64 [B, K1, 3]: tp, fp, fn of argmax (lowest index on a tie) against the labels over the valid pixels."""
    x = np.asarray(logits, dtype=np.float64)
    b, k1 = x.shape[:2]
    lab = np.asarray(labels).reshape(b, -1).astype(np.int64)
    valid = np.ones_like(lab, dtype=bool) if ignore is None else lab != int(ignore)
    a = x.reshape(b, k1, -1).argmax(1)  # numpy: first maximum
    out = np.zeros((b, k1, 3), dtype=np.int64)
    for k in range(k1):
        out[:, k, 0] = (valid & (a == k) & (lab == k)).sum(1)
        out[:, k, 1] = (valid & (a == k) & (lab != k)).sum(1)
        out[:, k, 2] = (valid & (a != k) & (lab == k)).sum(1)
    return out


def seg_loss(logits, labels, ignore=None, weight=None, softmax=True, do_bg=True, batch_dice=False, smooth=1.0, w_ce=1.0,
             w_dice=1.0):
    """dict(loss, ce, dc, grad [like logits], counts [B,K1,3])."""
    x, lab, valid, onehot, w, safe, nll = _prep(logits, labels, ignore, weight)
    p = torch.softmax(x, 1) if softmax else x
    axes = tuple(range(2, x.ndim))
    vm = valid[:, None].to(torch.float64)
    I, P, G = (p * onehot).sum(axes), (p * vm).sum(axes), onehot.sum(axes)
    if not do_bg:
        I, P, G = I[:, 1:], P[:, 1:], G[:, 1:]
    if batch_dice:
        I, P, G = I.sum(0), P.sum(0), G.sum(0)
    dc = -((2 * I + smooth) / torch.clip(G + P + smooth, 1e-8)).mean()
    den = (w[safe] * valid).sum()
    ce = nll.sum() / den if float(den) != 0.0 else x.sum() * 0.0
    loss = w_ce * ce + w_dice * dc
    loss.backward()
    return dict(loss=loss.item(), ce=ce.item(), dc=dc.item(), grad=x.grad.numpy(), counts=hard_counts(logits, labels, ignore))


def topk_ce(logits, labels, k, ignore=None, weight=None):
    """dict(loss, grad, tau, n, n_gt, n_eq): mean of the n = int(N k / 100) largest per-pixel losses (ignored pixels are zeros among
    the N).  Tie rule: the n_eq pixels equal to tau share the n - n_gt remaining slots equally."""
    x, lab, valid, onehot, w, safe, nll = _prep(logits, labels, ignore, weight)
    flat = nll.detach().reshape(-1)
    n = int(flat.numel() * k / 100)
    if n == 0:
        return dict(loss=float("nan"), grad=np.zeros(x.shape), tau=float("inf"), n=0, n_gt=0, n_eq=0)
    tau = torch.sort(flat, descending=True).values[n - 1]
    gt, eq = nll.detach() > tau, nll.detach() == tau
    n_gt, n_eq = int(gt.sum()), int(eq.sum())
    share = gt.to(torch.float64) + eq.to(torch.float64) * ((n - n_gt) / n_eq)
    loss = (share * nll).sum() / n
    loss.backward()
    return dict(loss=loss.item(), grad=x.grad.numpy(), tau=tau.item(), n=n, n_gt=n_gt, n_eq=n_eq)


# ================================================================== inputs and exact checks of the branch tests
# (tests/test_gpu_seg_loss_branches.py runs them on the device, tests/test_seg_loss_host.py checks every claim made here on the CPU)
IGN = 255
CLASS_WEIGHTS = (0.2, 1.0, 3.0, 0.5, 2.0, 0.75, 1.5, 0.25)  # the first k1 of them; the head of tests/test_seg_loss_host.py's WEIGHTS
EPS32 = 2.0 ** -24  # half an fp32 ulp relative: one rounding


def fp32(a):
    """Round to fp32 and return as float64: what the device sees, exactly."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def applies(ignore, ltype):
    """The ignore label as the kernel applies it: a value outside a byte can never match a uint8 label."""
    return ignore if ignore is not None and (ltype == "int64" or 0 <= ignore < 256) else None


def build_case(nb, k1, hw, ignore=None, ltype="int64", seed=0, frac_ignored=0.2, scale=2.0, prob=False, weighted=False,
               all_ignored_image=None, absent_class=None, zero_weight_class=None):
    """Seeded inputs: dict(logits [nb,k1,hw] float64 holding fp32 values, labels [nb,hw] int64, weight (list or None), ignore = the
    ignore label the kernel will apply).  prob: values in (0.05, 0.95) for the Dice on raw inputs.  Switches: every label of one
    image ignored, one class absent from the labels, class weight 0 for one class."""
    rs = np.random.RandomState([seed, nb, k1, hw])
    logits = fp32(rs.uniform(0.05, 0.95, (nb, k1, hw)) if prob else rs.randn(nb, k1, hw) * scale)
    labels = rs.randint(0, k1, (nb, hw)).astype(np.int64)
    if absent_class is not None:
        assert k1 > 1
        labels[labels == absent_class] = (absent_class + 1) % k1
    eff = applies(ignore, ltype)
    drop = rs.rand(nb, hw) < frac_ignored  # drawn in every case, so a case's logits do not depend on its ignore label
    if eff is not None:
        labels[drop] = eff
        if all_ignored_image is not None:
            labels[all_ignored_image] = eff
    else:
        assert all_ignored_image is None
    weight = None
    if weighted or zero_weight_class is not None:
        weight = [float(np.float32(v)) for v in CLASS_WEIGHTS[:k1]]
        if zero_weight_class is not None:
            weight[zero_weight_class] = 0.0
    return dict(logits=logits, labels=labels, weight=weight, ignore=eff)


def pixel_nll(logits, labels, ignore=None, weight=None):
    """float64 [B*HW]: w[label] (logsumexp - logit[label]) in the order the kernel stores it, 0 on ignored pixels."""
    return _prep(logits, labels, ignore, weight)[6].detach().numpy().reshape(-1)


def pixel_nll_bound(logits, labels, ignore=None, weight=None):
    """float64 [B*HW]: the bound on |device nll - float64 nll| per pixel derived in test_gpu_seg_loss_branches.py (roundings of
    tk_pixel_nll, expf within 2 ulp, logf within 1 ulp), in units of the pixel's own numbers."""
    x = np.asarray(logits, dtype=np.float64)
    b, k1 = x.shape[:2]
    x = x.reshape(b, k1, -1)
    lab = np.asarray(labels).reshape(b, -1).astype(np.int64)
    valid = np.ones_like(lab, dtype=bool) if ignore is None else lab != int(ignore)
    safe = np.where(valid, lab, 0)
    w = np.ones(k1) if weight is None else np.asarray(weight, dtype=np.float64)
    mx = x.max(1)
    d = (mx[:, None] - x).max(1)  # the largest |v - mx|
    se = np.exp(x - mx[:, None]).sum(1)
    lse = mx + np.log(se)
    u = lse - np.take_along_axis(x, safe[:, None], 1)[:, 0]
    rel_se = (d + 4 + (k1 - 1)) * EPS32  # the subtraction, expf (2 ulp = 4 half-ulps), k1 - 1 additions
    err = rel_se + 2 * EPS32 * np.log(se) + EPS32 * (np.abs(lse) + u)  # d log = d se / se; logf 1 ulp; mx + log; - vc
    return ((w[safe] * (err + EPS32 * u)) * valid).reshape(-1)  # times the class weight, rounded once more


def select_check(nll_bits_u32, n_top):
    """(tau bits, r, m) of the n_top-th largest bit pattern by an integer sort: tau = that value, r = n_top - #{> tau}, m = #{== tau}."""
    bits = np.asarray(nll_bits_u32, dtype=np.uint32).reshape(-1)
    assert 1 <= n_top <= bits.size
    tau = np.sort(bits)[bits.size - n_top]
    return int(tau), int(n_top - np.count_nonzero(bits > tau)), int(np.count_nonzero(bits == tau))


def selection_margin(nll, bound, n_top, tied=None):
    """How far the n_top largest float64 losses stay above the rest when every pixel moves by its bound: min over the selected of
    (nll - bound) minus max over the others of (nll + bound).  Positive: an evaluation within the bound selects the same pixels
    (this is the rank gap "more than twice the per-pixel bound", with each pixel's own bound).  `tied`: a mask of pixels to leave
    out (the tie group of a tie case, which is compared from both sides separately)."""
    nll, bound = np.asarray(nll, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    order = np.argsort(-nll, kind="stable")
    top = np.zeros(nll.size, dtype=bool)
    top[order[:n_top]] = True
    keep = np.ones(nll.size, dtype=bool) if tied is None else ~tied
    lo = (nll - bound)[top & keep]
    hi = (nll + bound)[~top & keep]
    return (lo.min() if lo.size else np.inf) - (hi.max() if hi.size else -np.inf)


def tie_case(m, r, n_a, n_b, nb, k1=3, seed=0):
    """Three groups of pixels over nb images (n_a + m + n_b = nb * hw): A, n_a pixels whose label logit lies 3 .. 7 below the
    largest other logit (nll >= 3, all distinct); T, m copies of ONE pixel (logits (1.5, 0, .., 0), label 1: nll = log(e^1.5 + k1 - 1)
    <= 2.45, the same bits in any arithmetic); B, n_b pixels whose label logit lies 0.5 .. 3.5 above every other (nll <= log(1 + (k1 -
    1) e^-0.5) <= 1.66, and 0.48 / 0.80 against T's 1.70 / 1.87 for k1 = 2 / 3).  n_top = n_a + r: n_gt = n_a, and the m tied pixels
    share r slots.  T sits at evenly spaced positions (so it is spread over images and blocks), A and B are shuffled over the rest.
    dict(logits, labels, n_top, n_gt, m, r, tied [N] bool)."""
    assert k1 >= 2 and 0 < r <= m
    n = n_a + m + n_b
    assert n % nb == 0
    hw = n // nb
    rs = np.random.RandomState([seed, m, r, n])
    x = rs.randn(n, k1) * 1.5
    lab = rs.randint(0, k1, n)
    tied = np.zeros(n, dtype=bool)
    tied[((np.arange(m) + 0.5) * n / m).astype(np.int64)] = True
    assert tied.sum() == m
    rest = rs.permutation(np.flatnonzero(~tied))
    ia, ib = rest[:n_a], rest[n_a:]
    other = np.where(np.arange(k1)[None] == lab[:, None], -np.inf, x).max(1)
    gap = np.zeros(n)
    gap[ia] = -(3.0 + 4.0 * (rs.permutation(n_a) + 0.5) / n_a)
    gap[ib] = 0.5 + 3.0 * rs.rand(n_b)
    x[np.arange(n), lab] = other + gap
    x[tied] = 0.0
    x[tied, 0] = 1.5
    lab[tied] = 1
    logits = fp32(x).reshape(nb, hw, k1).transpose(0, 2, 1).copy()
    return dict(logits=logits, labels=lab.reshape(nb, hw).astype(np.int64), n_top=n_a + r, n_gt=n_a, m=m, r=r, tied=tied,
                weight=None, ignore=None)


TIE_CASES = {(2, 1): dict(n_a=300, n_b=898, nb=2), (64, 1): dict(n_a=300, n_b=836, nb=2), (64, 63): dict(n_a=300, n_b=836, nb=2),
             (1000, 500): dict(n_a=600, n_b=1400, nb=3)}


def gap_case(nb, hw, n_above, seed=0, frac_ignored=0.0):
    """Two classes, label 0, logits (0, d): nll = log(1 + e^d).  n_above pixels have d in [3, 8] (nll >= 3.04), ONE pixel d = 2
    (nll = 2.127), the others d in [-8, 0.5] (nll <= 0.98): n_top = n_above + 1 selects down to the single pixel whatever the
    rounding -- a tie-free selection at any number of pixels.  frac_ignored of the pixels below carry the ignore label 255."""
    n = nb * hw
    rs = np.random.RandomState([seed, nb, hw % (2 ** 31), n_above])
    d = rs.uniform(-8.0, 0.5, n)
    pos = rs.permutation(n)
    d[pos[:n_above]] = rs.uniform(3.0, 8.0, n_above)
    d[pos[n_above]] = 2.0
    lab = np.zeros(n, dtype=np.int64)
    if frac_ignored:
        lab[pos[n_above + 1:][rs.rand(n - n_above - 1) < frac_ignored]] = IGN
    logits = np.stack([np.zeros(n), fp32(d)], 0).reshape(2, nb, hw).transpose(1, 0, 2).copy()
    return dict(logits=logits, labels=lab.reshape(nb, hw), n_top=n_above + 1, weight=None, ignore=IGN if frac_ignored else None)


RAMP_LO, RAMP_HI = 1.0 + 2.0 ** -10, 1.0 + 2.0 ** -7 - 2.0 ** -10


def dense_ramp(nb=2, hw=768, frac_ignored=0.2, seed=0):
    """Two classes, label 0, logits (0, d_i) with d_i = d0 + i eps laid out so that nll_i = log(1 + e^d_i) rises in equal steps from
    RAMP_LO to RAMP_HI.  fp32 values in [1, 1 + 2^-7) share sign, exponent and the top 7 mantissa bits -- the upper 16 bits of the
    pattern -- so the first two radix passes see one occupied bin (besides the zeros of the ignored pixels) and passes 2 and 3 pick
    the threshold.  The margin to either end of that range is 2^-10 = 9.8e-4, a thousand times the per-pixel bound (about 6e-7
    here).  n_top = half the valid pixels.  The order of the pixels is shuffled."""
    n = nb * hw
    rs = np.random.RandomState([seed, nb, hw])
    valid = rs.rand(n) >= frac_ignored
    v = int(valid.sum())
    target = RAMP_LO + (RAMP_HI - RAMP_LO) * np.arange(v) / (v - 1)
    d = np.zeros(n)
    d[np.flatnonzero(valid)[rs.permutation(v)]] = np.log(np.expm1(target))
    lab = np.where(valid, 0, IGN).astype(np.int64)
    logits = np.stack([np.zeros(n), fp32(d)], 0).reshape(2, nb, hw).transpose(1, 0, 2).copy()
    return dict(logits=logits, labels=lab.reshape(nb, hw), n_top=v // 2, weight=None, ignore=IGN, n_valid=v)


SPAN_WEIGHTS = (1e-3, 0.1, 10.0, 1e3)
LABEL_CASE_N_TOP = 156


def label_case(ltype):
    """The inputs of the label-decoding cases: ignore_label = -100 (applies to int64 labels only), 2 x 780 pixels, three classes."""
    return build_case(2, 3, 780, ignore=-100, ltype=ltype, seed=9)


def topk_free_cases():
    """The tie-free top-k cases of test_gpu_seg_loss_branches.py: id -> dict(inputs..., n_top, layout, ltype).  Every one must have
    a positive selection_margin (tests/test_seg_loss_host.py); the seeds were chosen so."""
    out = {}

    def add(name, nb, k1, hw, k, layout, ltype, ignore=IGN, seed=0, n_top=None, **kw):
        c = build_case(nb, k1, hw, ignore=ignore, ltype=ltype, seed=seed, **kw)
        c.update(n_top=int(nb * hw * k / 100) if n_top is None else n_top, layout=layout, ltype=ltype)
        out[name] = c

    add("k1=5-hw=620-k=10", 3, 5, 620, 10, "nchw", "int64")
    add("k1=5-hw=1964-k=25", 3, 5, 1964, 25, "cl", "uint8")
    add("k1=8-hw=620-k=25", 3, 8, 620, 25, "cl", "int64")
    add("k1=8-hw=1964-k=10", 3, 8, 1964, 10, "nchw", "uint8")
    add("n_top=N", 2, 3, 500, 100, "cl", "int64", ignore=None)
    add("n_top=1", 2, 3, 500, 0, "nchw", "uint8", n_top=1)
    add("weight0", 3, 4, 620, 10, "cl", "int64", zero_weight_class=2)
    add("span", 3, 4, 620, 10, "nchw", "int64", scale=8.0)
    out["span"]["weight"] = [float(np.float32(v)) for v in SPAN_WEIGHTS]
    return out
