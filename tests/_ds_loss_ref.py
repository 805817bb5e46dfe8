"""Float64 restatement of the deep-supervision loss (test infrastructure only): Dice + CE of bilinearly upsampled low-resolution
logits (csrc/ds_loss.hip), plus the seeded inputs and case tables that tests/test_ds_loss_host.py (CPU) and
tests/test_gpu_ds_loss.py (GPU) share.

    U(n, f)   the [n f, n] matrix of torch's interpolate(scale_factor=f, mode="bilinear", align_corners=False) along one axis:
              src = max((dst + 0.5) / f - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, n - 1), row dst holds (1 - l) at i0 and l at i1
              (both land on one pixel at a clamped border)
    u         = Uy z Ux^T per (image, class)
    loss      = _head_loss_ref.dice_ce on u (pixels flattened), which also gives du = its dlogits
    dz        = Uy^T du Ux

Low-resolution logits are [B, h, w, K] here (class last, like _head_loss_ref's [B, P, K]); labels are [B, H, W]."""
import functools

import torch

import _head_loss_ref as R

SMOOTH = R.SMOOTH
FACTORS = (2, 4, 8, 16)


def upsample_matrix(n, factor):
    """U [n * factor, n], float64."""
    dst = torch.arange(n * factor, dtype=torch.float64)
    src = ((dst + 0.5) / factor - 0.5).clamp(min=0.0)
    i0 = src.floor().long()
    i1 = (i0 + 1).clamp(max=n - 1)
    lam = src - i0.double()
    u = torch.zeros(n * factor, n, dtype=torch.float64)
    rows = torch.arange(n * factor)
    u.index_put_((rows, i0), 1.0 - lam, accumulate=True)
    u.index_put_((rows, i1), lam, accumulate=True)
    return u


def upsample(z, factor):
    """z [B, h, w, K] -> [B, h f, w f, K], float64."""
    z = z.double()
    uy, ux = upsample_matrix(z.shape[1], factor), upsample_matrix(z.shape[2], factor)
    return torch.einsum("Yy,byxk,Xx->bYXk", uy, z, ux)


def ds_dice_ce(z, labels, factor, softmax=True, do_bg=True, batch=False, squared=False, smooth=SMOOTH, dice_w=1.0, ce_w=1.0, gout=1.0):
    """sums [B, K, 3], coef [B, K, 2], out [3] of the loss on the upsampled logits, and dz [B, h, w, K]."""
    nb, h, w, k1 = z.shape
    u = upsample(z, factor)
    r = R.dice_ce(u.reshape(nb, -1, k1), labels.reshape(nb, -1), softmax, do_bg, batch, squared, smooth, dice_w, ce_w, gout)
    du = r["dlogits"].reshape(nb, h * factor, w * factor, k1)
    uy, ux = upsample_matrix(h, factor), upsample_matrix(w, factor)
    return dict(sums=r["sums"], coef=r["coef"], out=r["out"], dz=torch.einsum("Yy,bYXk,Xx->byxk", uy, du, ux), u=u, du=du)


def ds_inputs(nb, h, w, factor, k1, seed=0, softmax=True, special=None):
    """fp32 low-resolution logits [nb, h, w, k1] and int64 labels [nb, h f, w f], from _head_loss_ref.loss_inputs' generators, the
    hand-built sets of `special` included ("absent" and "one_class" act on the labels, "unpredicted" on the low-resolution logits)."""
    z, _ = R.loss_inputs(nb, h * w, k1, seed=seed, softmax=softmax, special="unpredicted" if special == "unpredicted" else None)
    _, labels = R.loss_inputs(nb, h * factor * w * factor, k1, seed=seed, softmax=softmax, special=special)
    return z.reshape(nb, h, w, k1), labels.reshape(nb, h * factor, w * factor)


@functools.lru_cache(maxsize=4)
def reference(key):
    """(z, labels, answer) of one case, computed once and shared; callers leave all three unchanged.
    key = (nb, h, w, factor, k1, flags, weights, gout, special, seed)"""
    nb, h, w, factor, k1, flags, weights, gout, special, seed = key
    z, labels = ds_inputs(nb, h, w, factor, k1, seed=seed, softmax=flags[0], special=special)
    w0, w1 = (float(torch.tensor(x, dtype=torch.float32)) for x in weights)  # the kernels take the weights as C floats
    return z, labels, ds_dice_ce(z, labels, factor, *flags, dice_w=w0, ce_w=w1, gout=1.0 if gout is None else gout)


DEFAULT_FLAGS = (True, True, False, False)
DEFAULT_WEIGHTS = (0.6, 0.9)


def key(nb, h, w, factor, k1, flags=DEFAULT_FLAGS, weights=DEFAULT_WEIGHTS, gout=None, special=None, seed=0):
    return (nb, h, w, factor, k1, flags, weights, gout, special, seed)


# ------------------------------------------------------------------ the shared case tables
# Low-resolution shapes: (1,1) both taps clamp onto one pixel; (1,5) one clamped axis; (3,3); (5,7) ragged against every tile; and per
# factor one shape that spans more than one backward tile in both directions for every class count (tiles: 16x16 at factor 2, 8x8 at
# 4, 4x4 at 8, at most 3x3 at 16) and, with three slabs, more than one forward slab.
SMALL_HW = ((1, 1), (1, 5), (3, 3), (5, 7))
MULTI_TILE = {2: (40, 24), 4: (18, 11), 8: (9, 6), 16: (5, 4)}
FAST_K1, GENERIC_K1 = (2, 3, 4), (1, 5, 8)


def shape_cases():
    """(nb, h, w, factor, k1, slabs): every factor x every small shape on both routes, and the multi-tile shape with every k1."""
    out = []
    for f in FACTORS:
        for i, (h, w) in enumerate(SMALL_HW):
            out.append((1 if i % 2 else 3, h, w, f, FAST_K1[i % 3], 1 + i % 2))
            out.append((3 if i % 2 else 1, h, w, f, GENERIC_K1[i % 3], 2 - i % 2))
        for k1 in FAST_K1 + GENERIC_K1:
            out.append((3 if k1 in (3, 5) else 1, *MULTI_TILE[f], f, k1, 3))
    return out


def interp_shapes():
    """every (h, w, factor) a GPU case uses"""
    return sorted({(h, w, f) for _, h, w, f, _, _ in shape_cases()} | {(5, 7, 4), (6, 5, 4)})


LAYOUTS = ("cl", "nchw", "pad")
FLAG_SHAPE = (3, 6, 5, 4)   # nb, h, w, factor of the flag / weight / hand-built / bad-label cases (24 x 20 pixels per image)
