"""fp64 reference of the batched BADGE gradient embedding (TEST INFRASTRUCTURE ONLY): the closed form the HIP kernel
implements (`csrc/badge_embed.hip`), and the quantity it must equal -- autograd through the reference losses
(`src/losses/dice_loss.py:32-76` DiceLoss + `torch.nn.CrossEntropyLoss`) on a 1x1 conv head, one image at a time as
`src/activelearning/badge_selector.py:19-35,80-96` does it."""
import torch


def dice_loss_restated(outputs, targets, k1, smooth, do_bg, squared):
    """dice_loss.py:32-76 with softmax=True, batch=False, written out here so `squared` is covered whatever the oracle takes."""
    p = torch.softmax(outputs, dim=1)
    y = torch.zeros_like(p).scatter_(1, targets.long().unsqueeze(1), 1.0)
    if not do_bg:
        p, y = p[:, 1:], y[:, 1:]
    inter = (p * y).sum((2, 3))
    if squared:
        s_in, s_t = (p ** 2).sum((2, 3)), (y ** 2).sum((2, 3))
    else:
        s_in, s_t = p.sum((2, 3)), y.sum((2, 3))
    return (1 - (2 * inter + smooth) / (s_in + s_t + smooth)).mean()


def embed_autograd(feat_nhwc, weight, bias, smooth, do_bg, squared, dice=None, ce=None):
    """Per image: d(ce + dice)(logits, argmax logits) / d weight with logits = conv1x1(feat), in feat's dtype (fp64 in the
    tests).  `dice(outputs, targets)` / `ce(outputs, targets)` default to the restatement above and F.cross_entropy.
    Returns (embed [B, K1*C0], loss [B])."""
    k1, c0 = weight.shape[0], weight.shape[1]
    embeds, losses = [], []
    for b in range(feat_nhwc.shape[0]):
        w = weight.detach().clone().reshape(k1, c0, 1, 1).requires_grad_(True)
        x = feat_nhwc[b:b + 1].permute(0, 3, 1, 2)
        out = torch.nn.functional.conv2d(x, w, bias)
        pred = out.detach().argmax(1)
        l_ce = ce(out, pred) if ce else torch.nn.functional.cross_entropy(out, pred)
        l_dice = dice(out, pred) if dice else dice_loss_restated(out, pred, k1, smooth, do_bg, squared)
        loss = l_ce + l_dice
        (g,) = torch.autograd.grad(loss, w)
        embeds.append(g.flatten())
        losses.append(loss.detach())
    return torch.stack(embeds), torch.stack(losses)


def embed_closed_form(logits, feat_nhwc, smooth, do_bg, squared):
    """The kernel's formulas in the dtype of `logits` (fp64 in the tests): logits [B,K1,H,W], feat_nhwc [B,H,W,C0] ->
    (embed [B, K1*C0], loss [B], A [B, K1*C0]) with A[c,k] = sum_pixels |dz_c| |feat_k|, the error unit of the GPU test."""
    b, k1, h, w = logits.shape
    c0 = feat_nhwc.shape[3]
    npix = h * w
    z = logits.reshape(b, k1, npix)
    f = feat_nhwc.reshape(b, npix, c0).to(z.dtype)
    p = torch.softmax(z, dim=1)
    a = z.argmax(1)  # first maximum
    y = torch.zeros_like(p).scatter_(1, a.unsqueeze(1), 1.0)
    big_i = (p * y).sum(2)
    big_z = (p * p).sum(2) if squared else p.sum(2)
    big_y = y.sum(2)
    den = big_z + big_y + smooth
    num = 2 * big_i + smooth
    in_s = torch.ones(k1, dtype=z.dtype)
    if not do_bg:
        in_s[0] = 0
    n = in_s.sum()
    ce = (torch.logsumexp(z, dim=1) - z.gather(1, a.unsqueeze(1)).squeeze(1)).sum(1) / npix
    loss = ce + ((1 - num / den) * in_s).sum(1) / n
    g = (-2 * y / den[:, :, None] + (num / den ** 2)[:, :, None] * (2 * p if squared else torch.ones_like(p))) * in_s[None, :, None] / n
    dz = p * (g - (p * g).sum(1, keepdim=True)) + (p - y) / npix
    embed = torch.einsum("bcp,bpk->bck", dz, f).reshape(b, k1 * c0)
    unit = torch.einsum("bcp,bpk->bck", dz.abs(), f.abs()).reshape(b, k1 * c0)
    return embed, loss, unit
