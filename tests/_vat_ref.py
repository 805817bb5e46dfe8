"""fp64 restatement of the virtual-adversarial-training pieces (csrc/vat.hip, csrc/stem_dgrad.hip) in plain torch on the CPU, with the
magnitudes the GPU tests turn into error bounds.

    p = softmax(zt), log q = log_softmax(z), L = coef * sum p (log p - log q), dL/dz = coef (q - p)        (p == 0 terms are 0)
"""
import torch
import torch.nn.functional as F


def kl(z, zt, den):
    """(L, dL/dz, value magnitude, gradient magnitude) in float64.  The magnitudes are what fp32 roundings act on:
    coef * sum p (|log p| + |log q|) for the value, coef * (p + q) per element for the gradient."""
    z, zt = z.double(), zt.double()
    lq, lp = torch.log_softmax(z, 1), torch.log_softmax(zt, 1)
    p, q = lp.exp(), lq.exp()
    coef = 1.0 / float(den)
    value = coef * torch.where(p > 0, p * (lp - lq), torch.zeros_like(p)).sum()
    mag = coef * torch.where(p > 0, p * (lp.abs() + lq.abs()), torch.zeros_like(p)).sum()
    return value, coef * (q - p), mag, coef * (p + q)


def normalize(u):
    """u / (||u||_2 + 1e-8) per sample (the published `_l2_normalize`)."""
    u = u.double()
    n = u.reshape(u.shape[0], -1).norm(dim=1).reshape(-1, *([1] * (u.ndim - 1)))
    return u / (n + 1e-8)


def sumsq(x):
    return (x.double() ** 2).reshape(x.shape[0], -1).sum(1)


def perturb(x, g, gscale, s):
    """x + s * (gscale g) / (gscale ||g|| + 1e-8) per sample."""
    x, g = x.double(), g.double()
    n = g.reshape(g.shape[0], -1).norm(dim=1).reshape(-1, *([1] * (g.ndim - 1)))
    return x + s * (gscale * g) / (gscale * n + 1e-8)


def stem_dgrad(dy_nchw, w):
    """d/dx of conv2d(x [N,1,H,W], w [C0,1,3,3], padding=1) contracted with dy [N,C0,H,W], by autograd in float64."""
    n, _, h, wd = dy_nchw.shape
    x = torch.zeros(n, 1, h, wd, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w.double().reshape(-1, 1, 3, 3), None, padding=1).backward(dy_nchw.double())
    return x.grad[:, 0]


# (dtype name, C0, (n, h, w)) of every integer probe of tests/test_gpu_stem_dgrad.py
EDGE_SHAPES = [(1, 1, 1), (2, 1, 37), (2, 19, 1), (2, 7, 21), (2, 3, 16), (2, 3, 17), (3, 200, 216)]
PROBES = [("bf16", c, (2, 19, 37)) for c in (8, 32, 64, 96, 256)] + [("fp32", c, (2, 19, 37)) for c in (4, 36, 64)] + \
         [(dt, 64, s) for dt in ("bf16", "fp32") for s in EDGE_SHAPES]


def probe_operands(c0, shape, seed):
    """dy [N, C0, H, W] integers in [-3, 3] and w [C0, 9] integers in [-2, 2], float64."""
    g = torch.Generator().manual_seed(seed)
    n, h, w = shape
    dy = torch.randint(-3, 4, (n, c0, h, w), generator=g).double()
    wt = torch.randint(-2, 3, (c0, 9), generator=g).double()
    return dy, wt
