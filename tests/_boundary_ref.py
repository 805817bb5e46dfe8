"""float64 restatement of the boundary loss (Kervadec et al., MIDL 2019: `one_hot2dist` + `SurfaceLoss`) for the tests of
csrc/boundary.hip and losses/boundary_loss.py.

For index labels y[b] in 0..k1-1, a tuple `classes` (default 1..k1-1) and spacing (sh, sw), with G = (y[b] == k):

    phi[b,k] = edt(~G) * ~G - (edt(G) - 1) * G            edt = scipy.ndimage.distance_transform_edt(., sampling=spacing)

The `- 1` is literal whatever the spacing.  Pixels outside the array do not exist (scipy's rule).  Two special cases never reach
scipy: a class absent from the image gives phi = 0 (Kervadec), and so does a class that fills the image (the project's own rule:
scipy's transform of an all-true mask measures to an imaginary point).

    L = (1/N) sum_{b, k in classes, p} softmax(z)[b,k,p] phi[b,k,p],     N = B * len(classes) * H * W
    dL/dz_j = g s_j (w_j - sum_k w_k s_k),  w_k = phi_k / N for k in classes, else 0
"""
import numpy as np
import torch


def default_classes(k1, classes=None):
    return tuple(range(1, k1)) if classes is None else tuple(sorted(int(c) for c in classes))


def _spacing(spacing):
    return (1.0, 1.0) if spacing is None else (float(spacing[0]), float(spacing[1]))


def phi_mask(g, spacing=None):
    """phi of one boolean mask [H,W], float64, by scipy."""
    from scipy import ndimage
    g = np.asarray(g, dtype=bool)
    if not g.any() or g.all():
        return np.zeros(g.shape, np.float64)
    s = _spacing(spacing)
    return ndimage.distance_transform_edt(~g, sampling=s) * ~g - (ndimage.distance_transform_edt(g, sampling=s) - 1.0) * g


def unsigned_mask(g, spacing=None):
    """The unsigned distance d behind phi_mask (to the nearest pixel of the other set; 0 where there is no boundary)."""
    from scipy import ndimage
    g = np.asarray(g, dtype=bool)
    if not g.any() or g.all():
        return np.zeros(g.shape, np.float64)
    s = _spacing(spacing)
    return ndimage.distance_transform_edt(~g, sampling=s) * ~g + ndimage.distance_transform_edt(g, sampling=s) * g


def phi_labels(labels, k1, classes=None, spacing=None, unsigned=False):
    """[B, len(classes), H, W] float64 of index labels [B,H,W]; a label outside 0..k1-1 belongs to no class."""
    labels = np.asarray(labels)
    fn = unsigned_mask if unsigned else phi_mask
    return np.stack([np.stack([fn(labels[b] == k, spacing) for k in default_classes(k1, classes)]) for b in range(labels.shape[0])])


def brute_phi(g, spacing=None):
    """phi of one mask straight from the definition: pairwise distances over np.argwhere (small masks only)."""
    g = np.asarray(g, dtype=bool)
    out = np.zeros(g.shape, np.float64)
    if not g.any() or g.all():
        return out
    s = np.asarray(_spacing(spacing))
    inside, outside = np.argwhere(g) * s, np.argwhere(~g) * s
    d2 = ((inside[:, None, :] - outside[None, :, :]) ** 2).sum(-1)
    out[g] = -(np.sqrt(d2.min(1)) - 1.0)
    out[~g] = np.sqrt(d2.min(0))
    return out


def loss(logits, phi, classes):
    """L in float64 torch (autograd flows to `logits`); phi [B, len(classes), H, W]."""
    s = torch.softmax(logits.double(), 1)
    return (s[:, list(classes)] * torch.as_tensor(phi, dtype=torch.float64)).mean()


def grad_formula(logits, phi, classes, g=1.0):
    """(dL/dlogits by the analytic formula, its magnitude s_j (|w_j| + sum_k |w_k| s_k), L, (1/N) sum |s phi|), all float64."""
    z = torch.as_tensor(logits).double()
    phi = torch.as_tensor(phi, dtype=torch.float64)
    s = torch.softmax(z, 1)
    w = torch.zeros_like(s)
    w[:, list(classes)] = phi / phi.numel()
    grad = g * s * (w - (w * s).sum(1, keepdim=True))
    mag = s * (w.abs() + (w.abs() * s).sum(1, keepdim=True))
    return grad, mag, (w * s).sum(), (w * s).abs().sum()
