"""Hausdorff distance / average surface distance / Jaccard of calculate_metric_percase on the GPU (csrc/surface.hip,
metric/segmentation.py) against the float64 scipy restatement of tests/_surface_ref.py: HD at rel 1e-6, ASD at rel 1e-5, NaN and
inf in identical positions; the full (DSC, HD, ASD, JC) table, determinism, isolation across volumes, and the validation steps
valid_slices(full_metrics=True) and valid_volumns."""
import numpy as np
import pytest
import torch

import _surface_ref as R

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _close(got, want, rel):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(np.isposinf(got), np.isposinf(want))
    ok = np.isfinite(want)
    np.testing.assert_array_equal(np.isfinite(got), ok)
    np.testing.assert_allclose(got[ok], want[ok], rtol=rel, atol=0)


def _label_maps(shape, k1, seed):
    """Label maps of one image / volume [(D,)H,W] in 0..k1-1: ellipses / ellipsoids, thresholded smoothed noise, single pixels."""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    grids = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    out = []
    for _ in range(2):
        lab = np.zeros(shape, np.int64)
        for c in range(1, k1):
            kind = rng.integers(0, 4)
            if kind == 0:
                r = sum(((g - rng.uniform(0, s)) / max(1.0, rng.uniform(0.15, 0.5) * s)) ** 2 for g, s in zip(grids, shape))
                lab[r < 1] = c
            elif kind == 1:
                noise = ndimage.gaussian_filter(rng.standard_normal(shape), sigma=max(1.0, min(shape) / 8))
                lab[noise > np.quantile(noise, 0.8)] = c
            elif kind == 2:
                lab[tuple(int(rng.integers(0, s)) for s in shape)] = c
            # kind 3: class c absent here
        out.append(lab)
    return out[0], out[1]


def _batch(n, shape, k1, seed):
    preds, labs = [], []
    for i in range(n):
        p, l = _label_maps(shape, k1, seed * 100 + i)
        if i % 4 == 1:                               # full image in pred, edge-touching label
            p[...] = 1
            l[...] = 0
            l[(slice(0, max(1, shape[0] // 3)),)] = 1
        if i % 4 == 2 and k1 > 2:                    # class 2 empty in pred, class 1 empty in label
            p[p == 2] = 0
            l[l == 1] = 0
        if i % 4 == 3:                               # both empty
            p[...] = 0
            l[...] = 0
        preds.append(p)
        labs.append(l)
    return np.stack(preds), np.stack(labs)


def _check_surface(pred, lab, k1, spacing):
    from metric.segmentation import surface_distances
    dev = _dev()
    hd, asd = surface_distances(torch.from_numpy(pred).to(dev), torch.from_numpy(lab).to(dev), k1, spacing)
    hd, asd = hd.cpu().numpy(), asd.cpu().numpy()
    want = [R.surface_table(pred[i], lab[i], k1, spacing) for i in range(pred.shape[0])]
    _close(hd, np.stack([w[0] for w in want]), 1e-6)
    _close(asd, np.stack([w[1] for w in want]), 1e-5)


@pytest.mark.parametrize("shape", [(1, 1, 1), (4, 37, 61), (3, 336, 544)])
@pytest.mark.parametrize("k1", [2, 3, 8])
@pytest.mark.parametrize("spacing", [None, (1.3, 0.4)])
def test_images_match_restatement(shape, k1, spacing):
    pred, lab = _batch(shape[0], shape[1:], k1, seed=k1 + shape[1])
    _check_surface(pred, lab, k1, spacing)


@pytest.mark.parametrize("shape,spacing", [((1, 1, 40, 33), None), ((1, 1, 40, 33), (2.0, 0.5, 1.5)), ((2, 5, 40, 33), None),
                                           ((1, 17, 64, 48), (1.7, 0.9, 1.1)), ((1, 48, 256, 256), (2.5, 0.7, 0.6))])
def test_volumes_match_restatement(shape, spacing):
    pred, lab = _batch(shape[0], shape[1:], 3, seed=shape[1])
    _check_surface(pred, lab, 3, spacing)


def test_one_slice_volume_differs_from_the_image():
    from metric.segmentation import surface_distances
    dev = _dev()
    p, l = _label_maps((40, 33), 2, seed=5)
    p[10:20, 5:25] = 1
    l[12:24, 8:30] = 1
    _, asd2 = surface_distances(torch.from_numpy(p[None]).to(dev), torch.from_numpy(l[None]).to(dev), 2)
    _, asd3 = surface_distances(torch.from_numpy(p[None, None]).to(dev), torch.from_numpy(l[None, None]).to(dev), 2)
    _close(asd2.cpu().numpy()[0], R.surface_table(p, l, 2)[1], 1e-5)
    _close(asd3.cpu().numpy()[0], R.surface_table(p[None], l[None], 2)[1], 1e-5)
    assert abs(float(asd2[0, 1]) - float(asd3[0, 1])) > 0.1


def test_pair_differing_only_along_d():
    """Prediction and label equal in every (h, w) plane position but shifted along D: HD and ASD come from the D pass alone."""
    shape = (12, 30, 26)
    p = np.zeros(shape, np.int64)
    l = np.zeros(shape, np.int64)
    p[2:6, 8:20, 6:18] = 1
    l[5:9, 8:20, 6:18] = 1
    _check_surface(p[None], l[None], 2, (2.5, 0.7, 0.6))
    _check_surface(p[None], l[None], 2, None)


def test_full_table_matches_calculate_metric_percase():
    from metric.segmentation import percase_metrics
    dev = _dev()
    for shape, spacing, nc in (((6, 37, 61), (1.3, 0.4), 3), ((2, 5, 40, 33), (2.0, 0.8, 1.1), 2), ((4, 1, 40, 33), None, 2)):
        pred, lab = _batch(shape[0], shape[1:], nc + 1, seed=len(shape) + nc)
        m_all, m_cls = percase_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(lab).to(dev), nc, spacing)
        assert m_all.shape == (shape[0], 4) and m_cls.shape == (shape[0], nc, 4)
        ref = [R.percase_table(pred[i], lab[i], nc, spacing) for i in range(shape[0])]
        want_all = np.stack([r[0] for r in ref])
        want_cls = np.stack([r[1] for r in ref])
        for got, want in ((m_all.cpu().numpy(), want_all), (m_cls.cpu().numpy(), want_cls)):
            _close(got[..., 0], want[..., 0], 1e-6)
            _close(got[..., 1], want[..., 1], 1e-6)
            _close(got[..., 2], want[..., 2], 1e-5)
            _close(got[..., 3], want[..., 3], 1e-6)
        assert np.isnan(want_all[:, 1]).any() or np.isnan(want_cls[..., 1]).any()  # the empty-prediction rows are exercised
        assert np.isposinf(want_cls[..., 1]).any()                               # and the empty-label rows


def test_deterministic_and_isolated_per_volume():
    from metric.segmentation import surface_distances
    dev = _dev()
    for shape, spacing in (((5, 64, 48), (1.3, 0.4)), ((3, 6, 40, 33), (2.0, 0.8, 1.1))):
        pred, lab = _batch(shape[0], shape[1:], 8, seed=3)
        p, l = torch.from_numpy(pred).to(dev), torch.from_numpy(lab).to(dev)
        h1, a1 = surface_distances(p, l, 8, spacing)
        h2, a2 = surface_distances(p, l, 8, spacing)
        assert torch.equal(h1.view(torch.int32), h2.view(torch.int32)) and torch.equal(a1.view(torch.int32), a2.view(torch.int32))
        for i in range(shape[0]):
            hi, ai = surface_distances(p[i:i + 1].clone(), l[i:i + 1].clone(), 8, spacing)
            assert torch.equal(hi[0].view(torch.int32), h1[i].view(torch.int32))
            assert torch.equal(ai[0].view(torch.int32), a1[i].view(torch.int32))


def _setup():
    """The setup of test_chained_validation_step_matches_oracle_chain (tests/test_gpu_unet.py)."""
    from losses.compound_losses import DiceAndCELoss
    from models.unet import UNet
    from models.unet.unet_processor import UnetProcessor
    dev = _dev()
    torch.manual_seed(7)
    num_classes, size, (h0, w0), b = 2, 128, (336, 544), 3
    model = UNet(2, 1, num_classes + 1, [8, 16, 32, 64], normalization="batch", dropout_prob=0.1)
    g = torch.Generator().manual_seed(3)
    for m in model.modules():
        if hasattr(m, "running_mean") and m.running_mean is not None:
            m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g))
            m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
    model = model.to(dev)
    image = torch.rand(b, 1, h0, w0, generator=g)
    yy, xx = torch.meshgrid(torch.arange(h0), torch.arange(w0), indexing="ij")
    label = torch.zeros(b, h0, w0, dtype=torch.long)
    for i in range(b):
        label[i][((yy - 150 - 20 * i) / 60.0) ** 2 + ((xx - 200) / 90.0) ** 2 < 1] = 1
        label[i][((yy - 200) / 40.0) ** 2 + ((xx - 400 + 30 * i) / 50.0) ** 2 < 1] = 2
    proc = UnetProcessor(image_size=size)
    loss_fn = DiceAndCELoss(dice_kwargs=dict(num_classes=num_classes, do_bg=True), ce_loss=torch.nn.CrossEntropyLoss)
    return model, proc, image, label, num_classes, loss_fn


@pytest.mark.parametrize("do_denoise,spacing", [(False, None), (True, None), (False, (0.8, 1.25))])
def test_valid_slices_full_metrics(do_denoise, spacing):
    from metric.segmentation import valid_slices
    model, proc, image, label, nc, loss_fn = _setup()
    d_all, d_cls, loss0, pred0 = valid_slices(model, proc, image, label, nc, loss_fn, do_denoise=do_denoise)
    m_all, m_cls, loss, pred = valid_slices(model, proc, image, label, nc, loss_fn, do_denoise=do_denoise, spacing=spacing,
                                            full_metrics=True)
    assert model.training
    assert torch.equal(pred, pred0) and torch.equal(loss, loss0)
    assert m_all.shape == (3, 4) and m_cls.shape == (3, nc, 4)
    assert torch.equal(m_all[:, 0].view(torch.int32), d_all.view(torch.int32))
    assert torch.equal(m_cls[..., 0].view(torch.int32), d_cls.view(torch.int32))
    got_p, lab = pred.cpu().numpy(), label.numpy()
    for i in range(3):
        w_all, w_cls = R.percase_table(got_p[i], lab[i], nc, spacing)
        for got, want in ((m_all[i].cpu().numpy(), w_all), (m_cls[i].cpu().numpy(), w_cls)):
            _close(got[..., 1], want[..., 1], 1e-6)
            _close(got[..., 2], want[..., 2], 1e-5)
            _close(got[..., 3], want[..., 3], 1e-6)


def test_valid_volumns_matches_slices_and_3d_restatement():
    from losses.compound_losses import DiceAndCELoss
    from metric.segmentation import valid_slices, valid_volumns
    from models.unet import UNet
    from models.unet.unet_processor import UnetProcessor
    dev = _dev()
    torch.manual_seed(11)
    nc, d, h, w = 2, 6, 80, 72
    model = UNet(2, 1, nc + 1, [8, 16, 32], normalization="instance", dropout_prob=None).to(dev).train()
    g = torch.Generator().manual_seed(5)
    image = torch.rand(1, 1, d, h, w, generator=g)
    zz, yy, xx = torch.meshgrid(torch.arange(d), torch.arange(h), torch.arange(w), indexing="ij")
    label = torch.zeros(1, d, h, w, dtype=torch.long)
    label[0][((zz - 2.5) / 3.0) ** 2 + ((yy - 35) / 20.0) ** 2 + ((xx - 30) / 18.0) ** 2 < 1] = 1
    label[0][((yy - 60) / 10.0) ** 2 + ((xx - 50) / 12.0) ** 2 < 1] = 2
    image = image + 0.5 * label.unsqueeze(1).float()  # give the net something to segment
    proc = UnetProcessor(image_size=64)
    loss_fn = DiceAndCELoss(dice_kwargs=dict(num_classes=nc, do_bg=True), ce_loss=torch.nn.CrossEntropyLoss)
    spacing = (2.5, 0.7, 0.6)
    m_all, m_cls, loss, pred = valid_volumns(model, proc, image, label, nc, loss_fn, spacing=spacing)
    assert model.training  # restored
    assert m_all.shape == (1, 4) and m_cls.shape == (1, nc, 4) and pred.shape == (d, h, w)
    slices = image[0].permute(1, 0, 2, 3).contiguous()
    _, _, loss_s, pred_s = valid_slices(model, proc, slices, label[0], nc, loss_fn)
    assert torch.equal(pred, pred_s)
    assert torch.equal(loss, loss_s)
    # the loss is loss_fn on the slice batch: logits of the eval forward against labels nearest-resized to the output size
    from transforms.hip import functional_hip as FH
    model.eval()
    with torch.no_grad():
        out = model(proc.preprocess(slices.to(dev)))
        ll = FH.resize_nearest(label[0].to(dev).unsqueeze(1), out.shape[-2], out.shape[-1]).squeeze(1)
        want_loss = loss_fn(out, ll)
    model.train()
    assert abs(float(loss) - float(want_loss)) < 1e-6
    w_all, w_cls = R.percase_table(pred.cpu().numpy(), label[0].numpy(), nc, spacing)
    for got, want in ((m_all[0].cpu().numpy(), w_all), (m_cls[0].cpu().numpy(), w_cls)):
        _close(got[..., 0], want[..., 0], 1e-6)
        _close(got[..., 1], want[..., 1], 1e-6)
        _close(got[..., 2], want[..., 2], 1e-5)
        _close(got[..., 3], want[..., 3], 1e-6)
    model.eval()
    valid_volumns(model, proc, image, label, nc)
    assert not model.training  # eval mode restored as well
