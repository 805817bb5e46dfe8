"""Float64 restatement of sliding-window prediction (TEST INFRASTRUCTURE ONLY): Gaussian-blended overlapping windows, mirrored
passes flipped back, fold models on top.  It takes the fp32 logits of every forward as recorded, in call order, and builds the
weighted sum S and the coverage by brute-force two-dimensional slice-adds: no separable shortcut, no shared code with the package
beyond the list of window starts and the fp32 one-dimensional weights it is handed."""
import torch

from _predict_ref import MAX_UNDECIDED, SUM_BOUND

ULP = 6e-8  # one fp32 rounding of a value <= 1


def mirror_combos(mirror_axes):
    """(), each axis alone in the order given, then both."""
    axes = list(mirror_axes)
    return [()] + [(a,) for a in axes] + ([tuple(axes)] if len(axes) == 2 else [])


def blend(records, b, h, w, ys, xs, gy, gx, n_models, mirror_axes=(), weights=None):
    """records: fp32 logits of every forward in call order -- model, then mirror combination, then window row-major -- each
    [n * b, K, ph, pw] for n consecutive windows (window-major along the batch).  The logits of a mirrored pass are those of the
    mirrored patch.  gy [ph], gx [pw]: the one-dimensional importance weights.

    Returns (P [b,K,h,w] float64 = S / coverage, label [b,h,w] int64, gap [b,h,w] float64 = top1 - top2 of P (+inf for one class),
    T = the largest number of terms any pixel received)."""
    weights = [1.0] * n_models if weights is None else [float(v) for v in weights]
    assert len(weights) == n_models
    combos = mirror_combos(mirror_axes)
    gy, gx = torch.as_tensor(gy).double(), torch.as_tensor(gx).double()
    ph, pw = gy.numel(), gx.numel()
    g2 = gy[:, None] * gx[None, :]
    allrec = torch.cat([r.detach().cpu().float() for r in records], 0)
    windows = [(y0, x0) for y0 in ys for x0 in xs]
    assert allrec.shape[0] == n_models * len(combos) * len(windows) * b and tuple(allrec.shape[2:]) == (ph, pw), allrec.shape
    k1 = allrec.shape[1]
    S = torch.zeros(b, k1, h, w, dtype=torch.float64)
    cov = torch.zeros(h, w, dtype=torch.float64)
    terms = torch.zeros(h, w, dtype=torch.int64)
    at = 0
    for m in range(n_models):
        for combo in combos:
            for (y0, x0) in windows:
                p = allrec[at:at + b].double().softmax(1)
                at += b
                if combo:
                    p = p.flip(combo)
                S[:, :, y0:y0 + ph, x0:x0 + pw] += weights[m] * g2 * p
                cov[y0:y0 + ph, x0:x0 + pw] += weights[m] * g2
                terms[y0:y0 + ph, x0:x0 + pw] += 1
    assert int(terms.min()) > 0, "a pixel no window covers"
    P = S / cov
    label = P.argmax(1)
    if k1 > 1:
        top = P.topk(2, dim=1).values
        gap = top[:, 0] - top[:, 1]
    else:
        gap = torch.full(label.shape, float("inf"), dtype=torch.float64)
    return P, label, gap, int(terms.max())


def prob_bound(T):
    """Bound on |normalised probability - P|: SUM_BOUND for the softmax and the scale factors, one fp32 ulp per addition."""
    return SUM_BOUND + T * ULP


def check(labels, probs, P, label, gap, T, what=""):
    """Normalised probabilities within prob_bound(T) of P; labels equal wherever the gap is at least twice that; the undecided share
    below MAX_UNDECIDED in cases of 1000 pixels or more.  Prints every figure before it asserts."""
    bound = prob_bound(T)
    err = (probs.detach().cpu().double() - P).abs().max().item()
    decided = gap >= 2 * bound
    share = 1.0 - decided.double().mean().item()
    wrong = int(((labels.detach().cpu() != label) & decided).sum())
    print(f"{what}: T={T} max|probs - P| = {err:.3e} (bound {bound:.3e}); {wrong} label mismatches over {int(decided.sum())} decided "
          f"pixels, undecided share {share:.3e}")
    assert err <= bound, (err, bound)
    assert wrong == 0, wrong
    if label.numel() >= 1000:
        assert share < MAX_UNDECIDED, share
    return err, share
