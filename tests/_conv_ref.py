"""fp64 restatement of the conv, input-gradient and weight-gradient entry points (csrc/conv_*.hip, stem.hip, wgrad_*.hip, pack.hip)
in plain torch on the CPU, and the integer operands on which every one of those kernels must reproduce it BIT FOR BIT.

Why exact: products of small integers are exact in bf16, f16 and fp32; fp32 accumulation of integers is exact in any order while
every partial sum stays below 2^24 (bounded by the same conv of absolute values: `exact_ok`); the split-f16 path scales by powers of
two and rescales with ldexp (csrc/common.h SplitF16).  The expected result is then the fp64 result rounded ONCE to the storage dtype.

Conventions: activations are NCHW float64 here; `w_nk` is the weight as the kernel's packed copy sees it, [n][k][kh][kw] with n the
output and k the input channel of THIS launch (for an input gradient that is the parameter with its first two axes swapped)."""
import numpy as np
import torch
import torch.nn.functional as F

G3S1, G3S2, G2S2, T3S2, T2S2, G1 = range(6)      # mia_hip.CONV_*
W3S1, W3S2, W2S2 = range(3)                      # mia_hip.WGRAD_*
LIMIT = float(1 << 24)


def _cat(x1, x2):
    return x1 if x2 is None else torch.cat([x1, x2], 1)


def out_hw(mode, hin, win, odd=(0, 0)):
    """Output size of a mode; T3S2 (gradient of a stride-2 conv) has two pre-images: odd = (1, 1) picks the odd sizes."""
    if mode in (G3S1, G1):
        return hin, win
    if mode == G3S2:
        return (hin + 1) // 2, (win + 1) // 2
    if mode == G2S2:
        return hin // 2, win // 2
    if mode == T3S2:
        return 2 * hin - odd[0], 2 * win - odd[1]
    return 2 * hin, 2 * win


def conv_ref(mode, x1, x2, w_nk, bias=None, flip=False, hw=None):
    """out[n] = bias[n] + sum_taps sum_k cat(x1, x2)[p * s + tap - pad][k] * w_nk[n][k][tap] in float64 (NCHW)."""
    x = _cat(x1, x2).double()
    w = w_nk.double()
    b = None if bias is None else bias.double()
    if mode == G3S1:
        return F.conv2d(x, w.flip(2, 3) if flip else w, b, padding=1)
    assert not flip
    if mode == G3S2:
        return F.conv2d(x, w, b, stride=2, padding=1)
    if mode == G2S2:
        return F.conv2d(x, w, b, stride=2)
    if mode == G1:
        return F.conv2d(x, w, b)
    if mode == T2S2:
        return F.conv_transpose2d(x, w.transpose(0, 1), b, stride=2)
    assert mode == T3S2 and hw is not None
    op = (hw[0] - (2 * x.shape[2] - 1), hw[1] - (2 * x.shape[3] - 1))
    return F.conv_transpose2d(x, w.transpose(0, 1), b, stride=2, padding=1, output_padding=op)


def conv_acc_ref(mode, out0, x1, w_nk, flip=False):
    """mia_conv_mma_acc: out += conv."""
    return out0.double() + conv_ref(mode, x1, None, w_nk, None, flip, hw=tuple(out0.shape[2:]))


def nl_operand(y, scale, shift, slope):
    """Normalise-on-load: x = lrelu(scale[n, c] * y + shift[n, c], slope)."""
    t = scale.double()[:, :, None, None] * y.double() + shift.double()[:, :, None, None]
    return torch.where(t > 0, t, t * slope)


def wgrad_ref(mode, x1, x2, dy):
    """dW[n][k][kh][kw] = sum_p dy[p][n] * cat(x1, x2)[p * s + tap - pad][k] (float64 autograd of the matching conv)."""
    x, g = _cat(x1, x2).double(), dy.double()
    ks, s, pad = (2, 2, 0) if mode == W2S2 else (3, 1 if mode == W3S1 else 2, 1)
    w = torch.zeros(g.shape[1], x.shape[1], ks, ks, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, None, stride=s, padding=pad).backward(g)
    return w.grad


def stats_ref(y64):
    """Per-(n, c) sum and sum of squares, [N][C][2]."""
    return torch.stack([y64.sum((2, 3)), (y64 * y64).sum((2, 3))], -1)


# ------------------------------------------------------------------ operands
def gen(seed):
    return torch.Generator().manual_seed(seed)


def signed(shape, g, density=1.0):
    """Integers in {-2 .. 2}; an element is non-zero with probability `density`."""
    v = torch.randint(1, 3, shape, generator=g).double() * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)
    return v * (torch.rand(shape, generator=g, dtype=torch.float64) < density)


def nonneg(shape, g):
    """Integers in {0 .. 3}, weighted towards 3 so that wide sums pass 2^11."""
    p = torch.tensor([0.1, 0.1, 0.2, 0.6], dtype=torch.float64)
    n = int(np.prod(shape))
    return torch.multinomial(p, n, replacement=True, generator=g).double().reshape(shape)


def int_bias(n, g):
    return torch.randint(-8, 9, (n,), generator=g).double()


def stats_density(terms, pixels):
    """Density of a `signed` operand pair for a statistics case: the output's standard deviation is about 2.5 d sqrt(terms); keep
    4.5 of them below 256 and pixels * sigma^2 well below 2^24 (the test asserts the actual preconditions, this only aims)."""
    sigma = min(40.0, 0.6 * (LIMIT / pixels) ** 0.5)
    return min(0.5, sigma / (2.5 * terms ** 0.5))


def expected(y64, dtype):
    """ONE rounding to the storage dtype (round to nearest even); every |y| is an integer below 2^24, so the fp32 step is exact."""
    return y64.to(torch.float32).to(dtype)


# ------------------------------------------------------------------ preconditions (on the reference alone)
def exact_ok(mode, x1, x2, w_nk, bias=None, flip=False, hw=None, out0=None, y64=None, stats=False):
    """{name: bool}: integer operands, every fp32 partial sum below 2^24, and for statistics |y| <= 256 (exact in bf16, so summing
    before or after the store rounding is the same), sum |y| and sum y^2 below 2^24 per (n, c)."""
    ops = [t for t in (x1, x2, w_nk, bias, out0) if t is not None]
    ok = {"integers": all(bool((t.double() == t.double().round()).all()) for t in ops)}
    bound = conv_ref(mode, x1.abs(), None if x2 is None else x2.abs(), w_nk.abs(), None if bias is None else bias.abs(), flip, hw)
    if out0 is not None:
        bound = bound + out0.double().abs()
    ok["partial sums < 2^24"] = bool(bound.max() < LIMIT)
    if stats:
        ok["|y| <= 256"] = bool(y64.abs().max() <= 256)
        ok["sum |y| < 2^24"] = bool(y64.abs().sum((2, 3)).max() < LIMIT)
        ok["sum y^2 < 2^24"] = bool((y64 * y64).sum((2, 3)).max() < LIMIT)
    return ok


def wgrad_exact_ok(mode, x1, x2, dy):
    ints = all(bool((t.double() == t.double().round()).all()) for t in (x1, x2, dy) if t is not None)
    bound = wgrad_ref(mode, x1.abs(), None if x2 is None else x2.abs(), dy.abs())
    return {"integers": ints, "sum |x||dy| < 2^24": bool(bound.max() < LIMIT)}


# ------------------------------------------------------------------ packed weights / split words
def pack_ref(w, dtype, n_from_d0, npad, kpad):
    """mia_pack_weight: w [D0][D1][kh][kw] fp32 -> [tap][npad][kpad] in `dtype` (RNE), zero padded; element (t, n, k) = w[a][b][t]
    with (a, b) = (n, k) when n indexes D0, else (k, n)  (csrc/pack.hip:16-17)."""
    d0, d1 = w.shape[:2]
    taps = w.shape[2] * w.shape[3]
    w3 = w.reshape(d0, d1, taps).float()
    nk = w3 if n_from_d0 else w3.transpose(0, 1)          # [n][k][t]
    out = torch.zeros(taps, npad, kpad, dtype=torch.float32)
    out[:, :nk.shape[0], :nk.shape[1]] = nk.permute(2, 0, 1)
    return out.to(dtype)


def split_exp(amax):
    """csrc/common.h SplitF16::exp_of on the fp32 bit pattern of max |x|."""
    bits = int(np.float32(amax).view(np.uint32)) & 0x7FFFFFFF
    return min(120, 141 - ((bits >> 23) & 0xFF))


def split_ref(packed_f32, amax):
    """mia_split_f16_batch: words (h | l << 16) of x * 2^e, h = float16(x 2^e), l = float16(x 2^e - h), both RNE."""
    x = packed_f32.numpy().astype(np.float32) * np.float32(2.0 ** split_exp(amax))
    h = x.astype(np.float16)
    l = (x - h.astype(np.float32)).astype(np.float16)
    return torch.from_numpy((h.view(np.uint16).astype(np.uint32) | (l.view(np.uint16).astype(np.uint32) << 16)).view(np.int32))
