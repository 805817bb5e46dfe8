"""Batched BADGE gradient embeddings on the GPU (`csrc/badge_embed.hip`, `activelearning.scores.badge_embeddings`,
`BADGESelector(embed_batch_size=...)`): the kernel against the fp64 closed form of `_badge_ref` on raw tensors, its exactness
properties, the selector pinned to the reference's own embeddings (`tests/golden/selectors.npz`), and the selector contract.

Error unit of the kernel test: u = max |got - ref| / A with A[c,k] = sum_pixels |dz_c| |feat_k| from the fp64 reference (feat at its
stored, bf16-rounded values).  The bound is not fixed in advance: the existing per-image path (HeadFn -> hip_cross_entropy + DiceLoss
-> autograd.grad on the weight) runs on the same inputs, its error is u0, and the fused kernel must satisfy
u <= max(2 u0, 32 * 2^-24) -- 2 for a different summation order over the same number of fp32 terms, the floor against a lucky u0.
Every case prints its u and u0 (`pytest -s`); profiles/badge_embed.txt is the record they belong in."""
import os

import numpy as np
import pytest
import torch

import _badge_ref as R

pytestmark = pytest.mark.gpu

SMOOTH = 1e-5
FLOOR = 32 * 2.0 ** -24
# (B, K1, C0, H, W, dtype, squared too); the last row is chosen from the launcher's slab rule: three slabs, the last one ragged
ROWS = [(3, 3, 8, 1, 1, torch.float32, False), (2, 2, 4, 7, 9, torch.float32, False), (1, 5, 20, 37, 53, torch.bfloat16, True),
        (3, 3, 64, 64, 64, torch.bfloat16, False), (2, 4, 96, 96, 96, torch.float32, True), (2, 3, 16, 97, 97, torch.bfloat16, False)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _inputs(b, k1, c0, h, w, dtype, seed, single_class_image=None):
    """feat [B,H,W,C0] in `dtype`, a random head scaled so that the logits spread over several units (arg-max margins are not
    near-ties), and the head's own fp32 logits (logical NCHW, channels-last strides)."""
    from mia_hip import ops
    dev = _dev()
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(b, h, w, c0, generator=g)
    weight = torch.randn(k1, c0, 1, 1, generator=g) * (3.0 / c0 ** 0.5)
    bias = torch.zeros(k1)
    if single_class_image is not None:
        feat[single_class_image] *= 0.02
        bias[k1 - 1] = 2.0
    feat = feat.to(dev).to(dtype).contiguous()
    weight, bias = weight.to(dev), bias.to(dev)
    with torch.no_grad():
        logits = ops.HeadFn.apply(feat, weight, bias)
    return feat, weight, bias, logits


def _existing_path(feat, weight, bias, do_bg, squared):
    """What BADGESelector.cal_scores does per image today, on raw tensors."""
    from losses.ce_loss import hip_cross_entropy
    from losses.dice_loss import DiceLoss
    from mia_hip import ops
    k1 = weight.shape[0]
    dice, ce = DiceLoss(k1 - 1, smooth=SMOOTH, do_bg=do_bg, squared=squared), torch.nn.CrossEntropyLoss()
    out = []
    for i in range(feat.shape[0]):
        w = weight.clone().requires_grad_(True)
        logits = ops.HeadFn.apply(feat[i:i + 1], w, bias)
        pred = logits.softmax(1).argmax(1)
        loss = hip_cross_entropy(ce, logits, pred) + dice(logits, pred)
        (g,) = torch.autograd.grad(loss, w)
        out.append(g.flatten())
    return torch.stack(out)


def _units(got, ref, unit):
    return float(((got.double().cpu() - ref).abs() / unit.clamp_min(1e-300)).max())


@pytest.mark.parametrize("do_bg", [True, False])
@pytest.mark.parametrize("row", ROWS, ids=lambda r: f"B{r[0]}K{r[1]}C{r[2]}_{r[3]}x{r[4]}_{'bf16' if r[5] == torch.bfloat16 else 'f32'}")
def test_kernel_against_fp64_closed_form(row, do_bg):
    from activelearning.scores import badge_embeddings, badge_slabs
    b, k1, c0, h, w, dtype, with_squared = row
    single = 0 if (h, w) == (64, 64) else None
    feat, weight, bias, logits = _inputs(b, k1, c0, h, w, dtype, seed=h * 131 + k1, single_class_image=single)
    if (h, w) == (97, 97):
        assert badge_slabs(4096, k1, c0, dtype) == 1 and badge_slabs(4097, k1, c0, dtype) == 2  # 4096 pixels per slab ...
        assert badge_slabs(h * w, k1, c0, dtype) == 3 and (h * w) % 4096 != 0                   # ... so three, the last one ragged
    if single is not None:
        assert bool((logits[single].argmax(0) == k1 - 1).all())
        assert len(torch.unique(logits[1].argmax(0))) > 1
    for squared in ((False, True) if with_squared else (False,)):
        ref, ref_loss, unit = R.embed_closed_form(logits.double().cpu(), feat.double().cpu(), SMOOTH, do_bg, squared)
        u0 = _units(_existing_path(feat, weight, bias, do_bg, squared), ref, unit)
        bound = max(2 * u0, FLOOR)
        for layout in ("head", "nchw"):
            lg = logits if layout == "head" else logits.contiguous()
            assert lg.is_contiguous() == (layout == "nchw") or k1 == 1 or h * w == 1
            got, loss = badge_embeddings(lg, feat, SMOOTH, do_bg, squared)
            assert got.shape == (b, k1 * c0) and loss.shape == (b,) and got.dtype == torch.float32
            u = _units(got, ref, unit)
            print(f"badge_embed B={b} K1={k1} C0={c0} {h}x{w} {str(dtype)[6:]} do_bg={int(do_bg)} squared={int(squared)} "
                  f"logits={layout}: u={u / 2.0 ** -24:.2f} u0={u0 / 2.0 ** -24:.2f} (units of 2^-24)")
            assert u <= bound, (u, u0, layout, squared)
            np.testing.assert_allclose(loss.cpu().numpy(), ref_loss.numpy(), rtol=1e-5)


@pytest.mark.parametrize("k1,c0,h,w,dtype", [(3, 16, 97, 97, torch.bfloat16), (4, 32, 64, 64, torch.float32), (2, 20, 5, 3, torch.float32)])
def test_bits_do_not_depend_on_the_run_or_on_the_batch(k1, c0, h, w, dtype):
    from activelearning.scores import badge_embeddings
    feat, _, _, logits = _inputs(5, k1, c0, h, w, dtype, seed=11)
    e1, l1 = badge_embeddings(logits, feat, SMOOTH, True, False)
    e2, l2 = badge_embeddings(logits, feat, SMOOTH, True, False)
    assert torch.equal(e1, e2) and torch.equal(l1, l2)
    assert bool(torch.isfinite(e1).all()) and float(e1.abs().max()) > 0
    for i in (0, 3, 4):
        ei, li = badge_embeddings(logits[i:i + 1], feat[i:i + 1], SMOOTH, True, False)
        assert torch.equal(ei[0], e1[i]) and torch.equal(li[0], l1[i]), i
    ec, lc = badge_embeddings(logits[2:3].clone(), feat[2:3].clone(), SMOOTH, True, False)
    assert torch.equal(ec[0], e1[2]) and torch.equal(lc[0], l1[2])


def test_unsupported_shapes_raise():
    import mia_hip
    from activelearning.scores import badge_embeddings
    dev = _dev()
    with pytest.raises(mia_hip.MiaError):
        badge_embeddings(torch.zeros(1, 3, 4, 4, device=dev), torch.zeros(1, 4, 4, 6, device=dev))
    with pytest.raises(mia_hip.MiaError):
        badge_embeddings(torch.zeros(1, 9, 4, 4, device=dev), torch.zeros(1, 4, 4, 8, device=dev))
    with pytest.raises(mia_hip.MiaError):
        badge_embeddings(torch.zeros(1, 1, 4, 4, device=dev), torch.zeros(1, 4, 4, 8, device=dev), do_bg=False)
    with pytest.raises(mia_hip.MiaError):
        badge_embeddings(torch.zeros(1, 3, 4, 4, device=dev), torch.zeros(1, 4, 5, 8, device=dev))


# ------------------------------------------------------------------ the selector
class _DS(torch.utils.data.Dataset):
    def __init__(self, images, names):
        self.images, self.image_idx = images, list(names)

    def __len__(self):
        return len(self.image_idx)

    def __getitem__(self, i):
        return {"image": self.images[i], "case_name": self.image_idx[i]}


class _ActiveDataset:
    """The four members the reference selectors touch (datasets/active_dataset.py)."""

    def __init__(self, images, n_labeled):
        names = [f"case_{i:02d}" for i in range(len(images))]
        self.train_dataset = _DS(images[:n_labeled], names[:n_labeled])
        self.pool_dataset = _DS(images[n_labeled:], names[n_labeled:])

    def get_size(self):
        return len(self.train_dataset), len(self.pool_dataset)

    def get_pool_dataset(self):
        return self.pool_dataset

    def get_train_dataset(self):
        return self.train_dataset


def _golden():
    return dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "selectors.npz"), allow_pickle=False))


def _al_loss():
    from losses.compound_losses import DiceAndCELoss
    return DiceAndCELoss(dice_kwargs=dict(num_classes=2, do_bg=True), ce_loss=torch.nn.CrossEntropyLoss)


def _selector(loss, **kw):
    from activelearning import BADGESelector
    return BADGESelector(dice_loss=loss.dice_loss, ce_loss=loss.ce_loss, batch_size=1, num_workers=0, pin_memory=False, **kw)


def test_fused_selector_matches_reference_vectors(monkeypatch):
    """The model and images of `tests/golden/selectors.npz`, set up as `test_selectors_match_reference_vectors` does; ten pool
    images at embed_batch_size=4 run as batches of 4, 4 and 2."""
    from models.unet import UNet
    dev = _dev()
    monkeypatch.delenv("MIA_BADGE_BATCH", raising=False)
    d = _golden()
    model = UNet(2, 1, 3, [8, 16, 32], normalization="instance", dropout_prob=None)
    model.load_state_dict({k[5:]: torch.from_numpy(v.copy()) for k, v in d.items() if k.startswith("init/")})
    model = model.to(dev)
    ad = _ActiveDataset(torch.from_numpy(d["images"]), int(d["n_labeled"]))
    assert ad.get_size()[1] == 10
    loss = _al_loss()
    sel = _selector(loss, embed_batch_size=4)
    assert sel.embed_path(model) == "fused"
    names, embeds = sel.cal_scores(ad, model, dev)
    assert list(names) == list(d["badge/names"])
    np.testing.assert_allclose(embeds, d["badge/embeds"], rtol=2e-3, atol=2e-6)
    monkeypatch.setenv("MIA_BADGE_BATCH", "4")
    sel_env = _selector(loss)
    assert sel_env.embed_path(model) == "fused"
    names_env, embeds_env = sel_env.cal_scores(ad, model, dev)
    assert list(names_env) == list(d["badge/names"])
    np.testing.assert_allclose(embeds_env, d["badge/embeds"], rtol=2e-3, atol=2e-6)
    np.testing.assert_array_equal(embeds_env, embeds)


def _pool(norm, seed=7):
    from models.unet import UNet
    dev = _dev()
    torch.manual_seed(seed)
    model = UNet(2, 1, 3, [8, 16, 32], normalization=norm, dropout_prob=None)
    if norm == "batch":  # running statistics that are not the initial (0, 1)
        g = torch.Generator().manual_seed(seed + 1)
        for k, v in model.state_dict().items():
            if k.endswith("running_mean"):
                v.copy_(torch.randn(v.shape, generator=g) * 0.1)
            elif k.endswith("running_var"):
                v.copy_(torch.rand(v.shape, generator=g) + 0.5)
    model = model.to(dev)
    g = torch.Generator().manual_seed(9)
    images = torch.rand(14, 1, 32, 32, generator=g) * torch.linspace(0.2, 3.0, 14).view(-1, 1, 1, 1)
    return dev, model, images


def test_fused_selector_matches_the_per_image_path_on_a_batch_norm_model(monkeypatch):
    monkeypatch.delenv("MIA_BADGE_BATCH", raising=False)
    dev, model, images = _pool("batch")
    assert any(k.endswith("running_mean") for k in model.state_dict())
    ad = _ActiveDataset(images, 4)
    loss = _al_loss()
    names0, embeds0 = _selector(loss).cal_scores(ad, model, dev)
    names1, embeds1 = _selector(loss, embed_batch_size=4).cal_scores(ad, model, dev)
    assert list(names1) == list(names0) == ad.pool_dataset.image_idx
    np.testing.assert_allclose(embeds1, embeds0, rtol=2e-3, atol=2e-6)


def test_fused_selector_contract(monkeypatch):
    from losses.dice_loss import DiceLoss
    monkeypatch.delenv("MIA_BADGE_BATCH", raising=False)
    dev, model, images = _pool("instance")
    ad = _ActiveDataset(images, 4)
    loss = _al_loss()
    sel = _selector(loss, embed_batch_size=4)
    for q in model.parameters():  # gradients a training step would have left
        q.grad = torch.ones_like(q)
    picks = sel.select_next_batch(ad, 3, model, dev)
    assert len(picks) == 3 and len(set(picks)) == 3 and set(picks) <= set(ad.pool_dataset.image_idx)
    assert all(q.grad is None or float(q.grad.abs().sum()) == 0.0 for q in model.parameters())
    assert not model.training
    # empty labelled set -> the seeded random pick (badge_selector.py:112-120)
    ad0 = _ActiveDataset(images, 0)
    torch.manual_seed(5)
    picks = sel.select_next_batch(ad0, 5, model, dev)
    torch.manual_seed(5)
    idx = torch.sort(torch.rand(14), descending=True)[1][:5]
    assert picks == [ad0.pool_dataset.image_idx[int(i)] for i in idx]
    # an ineligible loss takes the per-image path whatever embed_batch_size says: the old result bit for bit
    from activelearning import BADGESelector
    dice = DiceLoss(2, do_bg=True, softmax=False)
    kw = dict(dice_loss=dice, ce_loss=loss.ce_loss, batch_size=1, num_workers=0, pin_memory=False)
    old = BADGESelector(**kw)
    new = BADGESelector(embed_batch_size=4, **kw)
    assert new.embed_path(model) == "autograd" and "softmax=False" in new.embed_path_reason
    n0, e0 = old.cal_scores(ad, model, dev)
    n1, e1 = new.cal_scores(ad, model, dev)
    assert list(n0) == list(n1)
    np.testing.assert_array_equal(e0, e1)
