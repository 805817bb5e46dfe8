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
