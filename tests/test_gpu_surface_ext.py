"""HD95 / ASSD / surface Dice on the GPU (mia_surface_metrics in csrc/surface.hip, metric.segmentation.surface_metrics) against the
float64 scipy restatement of tests/_surface_ext_ref.py: HD_q at rel 1e-6 (a rank-k value moves by no more than the largest
perturbation of an element, and the fp32 squared distances are within a few 1e-7 of exact: the argument for HD), ASSD at rel 1e-5,
NaN and inf in identical positions, and the surface-Dice counts exactly -- each tolerance is put into a relative gap of >= 1e-3
between two neighbouring distinct distances, so fp32 cannot flip a comparison.  Also: hd / asd are surface_distances' bits, two
runs and a volume run alone give the same bits, and percase_metrics / valid_volumns carry the columns through."""
import functools
import math

import numpy as np
import pytest
import torch
from scipy import ndimage

import _surface_ext_ref as E
from test_gpu_surface_metrics import _batch, _close, _dev

pytestmark = pytest.mark.gpu

CASES = [((2, 37, 61), 3, None), ((2, 37, 61), 3, (1.3, 0.4)), ((2, 96, 130), 4, (1.3, 0.4)), ((2, 336, 544), 4, (0.8, 1.25)),
         ((2, 5, 40, 33), 3, None), ((1, 17, 64, 48), 3, (1.7, 0.9, 1.1)), ((1, 48, 128, 160), 3, (2.5, 0.7, 0.6))]


def pair(shape, k1, seed):
    """(pred, label) of one image / volume: arg-max of smoothed noise, the prediction perturbed -- every class present on both
    sides (but for the odd one) with ragged borders, so the pooled distances have many distinct values and a long tail."""
    rng = np.random.default_rng(seed)
    sig = [max(1.0, s / 6) for s in shape]
    base = np.stack([ndimage.gaussian_filter(rng.standard_normal(shape), sig) for _ in range(k1)])
    pert = np.stack([ndimage.gaussian_filter(rng.standard_normal(shape), sig) for _ in range(k1)])
    base[0] += 0.5 * base.std()
    return (base + 0.6 * pert).argmax(0), base.argmax(0)


def _sets(pred, lab, k1, spacing):
    """[m][i] -> (S1, S2) of mask m in volume i, or None where one side is empty."""
    out = []
    for m in range(k1):
        row = []
        for i in range(pred.shape[0]):
            a, b = E.masks(pred[i], lab[i], k1)[m]
            row.append(E.surface_sets(a, b, spacing) if a.any() and b.any() else None)
        out.append(row)
    return out


def _tau(sets_m):
    """A tolerance for one mask that no distance of the batch comes near: from the middle of the sorted distinct positive distances
    outward, the first neighbouring pair with a relative gap >= 1e-3; their midpoint.  None when there is no such pair."""
    vals = [s for pair_ in sets_m if pair_ is not None for s in pair_]
    u = np.unique(np.concatenate(vals)) if vals else np.zeros(0)
    u = u[u > 0]
    mid = (u.size - 1) // 2
    for step in range(u.size):
        for j in (mid + step, mid - step):
            if 0 <= j < u.size - 1 and (u[j + 1] - u[j]) / (u[j] + u[j + 1]) >= 1e-3:
                return float(0.5 * (u[j] + u[j + 1]))
    return None


def _want(pred, lab, k1, spacing, q, taus):
    """(hd_pct, assd, nsd, n) [N,k1] float64 from the restatement."""
    rows = [E.ext_table(pred[i], lab[i], k1, spacing, q, taus) for i in range(pred.shape[0])]
    n = np.array([[sum(np.count_nonzero(E.border(x)) for x in ab) for ab in E.masks(pred[i], lab[i], k1)] for i in range(pred.shape[0])])
    return tuple(np.stack([r[j] for r in rows]) for j in range(3)) + (n,)


@functools.lru_cache(maxsize=None)
def _case(idx):
    """Inputs, tolerances and the q = 95 restatement of CASES[idx], computed once and never written to."""
    shape, k1, spacing = CASES[idx]
    ps, ls = zip(*[pair(shape[1:], k1, 1000 * idx + i) for i in range(shape[0])])
    pred, lab = np.stack(ps), np.stack(ls)
    sets = _sets(pred, lab, k1, spacing)
    taus = [_tau(s) for s in sets]
    assert all(t is not None for t in taus), taus
    return pred, lab, k1, spacing, tuple(taus), sets, _want(pred, lab, k1, spacing, 95.0, taus)


def _run(pred, lab, k1, spacing, q=95.0, taus=1.0):
    from metric.segmentation import surface_metrics
    dev = _dev()
    return surface_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(lab).to(dev), k1, spacing, q, taus)


def _bits(t):
    return t.view(torch.int32)


def _compare(got, want):
    hd_pct, assd, nsd, n = want
    _close(got.hd_pct.cpu().numpy(), hd_pct, 1e-6)
    _close(got.assd.cpu().numpy(), assd, 1e-5)
    g = got.nsd.cpu().numpy().astype(np.float64)
    _close(g, nsd, 1e-6)
    np.testing.assert_array_equal(np.rint(g * n), np.rint(nsd * n))  # the counts themselves


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_matches_restatement(idx):
    from metric.segmentation import surface_distances
    pred, lab, k1, spacing, taus, _, want = _case(idx)
    got = _run(pred, lab, k1, spacing, 95.0, taus)
    _compare(got, want)
    dev = _dev()
    hd, asd = surface_distances(torch.from_numpy(pred).to(dev), torch.from_numpy(lab).to(dev), k1, spacing)
    assert torch.equal(_bits(got.hd), _bits(hd)) and torch.equal(_bits(got.asd), _bits(asd))
    fin = np.isfinite(want[0])
    assert fin.sum() >= fin.size - 1  # every mask pair but at most one is non-empty on both sides


def test_rank_step_takes_both_branches():
    """Over the 2-D cases, v[k + 1] == v[k] for some mask pairs and the next distinct value for others (the restatement's view of
    the inputs that test_matches_restatement runs)."""
    same = other = 0
    for idx in range(4):
        for row in _case(idx)[5]:
            for s in row:
                if s is None:
                    continue
                v = np.sort(np.hstack(s))
                k = int(math.floor((v.size - 1) * 0.95))
                same += v[k + 1] == v[k]
                other += v[k + 1] > v[k]
    assert same > 0 and other > 0, (same, other)


@pytest.mark.parametrize("q", [50.0, 100.0])
def test_other_percentiles(q):
    pred, lab, k1, spacing, taus, sets, _ = _case(2)
    got = _run(pred, lab, k1, spacing, q, taus)
    _compare(got, _want(pred, lab, k1, spacing, q, taus))
    if q == 100.0:  # the larger of the two surface-to-surface maxima -- not hd, which runs over all mask pixels
        top = np.array([[max(s[0].max(), s[1].max()) if s is not None else np.nan for s in row] for row in sets]).T  # [N,k1]
        ok = ~np.isnan(top)
        assert ok.sum() >= ok.size - 1
        np.testing.assert_allclose(got.hd_pct.cpu().numpy()[ok], top[ok], rtol=1e-6, atol=0)


def test_single_pixel_in_both_masks():
    one = np.ones((1, 1, 1), np.int64)  # n = 2, pos = 0.95, both distances 0
    got = _run(one, one, 2, None)
    for t, v in ((got.hd, 0.0), (got.asd, 0.0), (got.hd_pct, 0.0), (got.assd, 0.0), (got.nsd, 1.0)):
        assert t.shape == (1, 2) and (t.cpu().numpy() == v).all()


def test_empty_set_patterns():
    """The batch of test_gpu_surface_metrics: full image vs an edge-touching label, a class empty in the prediction, another empty in
    the label, both empty.  Unit spacing: squared distances are integers, which 1.5^2 keeps clear of."""
    pred, lab = _batch(4, (37, 61), 3, seed=5)
    want = _want(pred, lab, 3, None, 95.0, 1.5)
    assert np.isnan(want[0]).any() and np.isposinf(want[0]).any() and np.isfinite(want[0]).any()
    got = _run(pred, lab, 3, None, 95.0, 1.5)
    _compare(got, want)
    assert (got.nsd.cpu().numpy()[~np.isfinite(want[0])] == 0).all()


def test_deterministic_and_isolated_per_volume():
    for idx in (1, 3, 4):
        pred, lab, k1, spacing, taus, _, _ = _case(idx)
        a = _run(pred, lab, k1, spacing, 95.0, taus)
        b = _run(pred, lab, k1, spacing, 95.0, taus)
        for x, y in zip(a, b):
            assert torch.equal(_bits(x), _bits(y))
        for i in range(pred.shape[0]):
            c = _run(pred[i:i + 1].copy(), lab[i:i + 1].copy(), k1, spacing, 95.0, taus)
            for x, y in zip(a, c):
                assert torch.equal(_bits(x[i]), _bits(y[0]))


def test_percase_metrics_extended_columns():
    from metric.segmentation import percase_metrics
    dev = _dev()
    for idx in (1, 4):
        pred, lab, k1, spacing, taus, _, _ = _case(idx)
        p, l = torch.from_numpy(pred).to(dev), torch.from_numpy(lab).to(dev)
        b_all, b_cls = percase_metrics(p, l, k1 - 1, spacing)
        m_all, m_cls = percase_metrics(p, l, k1 - 1, spacing, extended=True, percentile=90.0, tolerance=taus)
        assert m_all.shape == (pred.shape[0], 7) and m_cls.shape == (pred.shape[0], k1 - 1, 7)
        assert torch.equal(_bits(m_all[:, :4].contiguous()), _bits(b_all)) and torch.equal(_bits(m_cls[..., :4].contiguous()), _bits(b_cls))
        s = _run(pred, lab, k1, spacing, 90.0, taus)
        for j, t in enumerate((s.hd_pct, s.assd, s.nsd)):
            assert torch.equal(_bits(m_all[:, 4 + j].contiguous()), _bits(t[:, 0].contiguous()))
            assert torch.equal(_bits(m_cls[..., 4 + j].contiguous()), _bits(t[:, 1:].contiguous()))


def test_valid_volumns_extended():
    """The volume step of test_valid_volumns_matches_slices_and_3d_restatement with extended=True: [1,7] / [1,num_classes,7], the
    first four columns unchanged and the last three the restatement on the step's own prediction."""
    from metric.segmentation import valid_volumns
    from models.unet import UNet
    from models.unet.unet_processor import UnetProcessor
    dev = _dev()
    torch.manual_seed(11)
    nc, d, h, w = 2, 6, 80, 72
    model = UNet(2, 1, nc + 1, [8, 16, 32], normalization="instance", dropout_prob=None).to(dev).eval()
    g = torch.Generator().manual_seed(5)
    image = torch.rand(1, 1, d, h, w, generator=g)
    zz, yy, xx = torch.meshgrid(torch.arange(d), torch.arange(h), torch.arange(w), indexing="ij")
    label = torch.zeros(1, d, h, w, dtype=torch.long)
    label[0][((zz - 2.5) / 3.0) ** 2 + ((yy - 35) / 20.0) ** 2 + ((xx - 30) / 18.0) ** 2 < 1] = 1
    label[0][((yy - 60) / 10.0) ** 2 + ((xx - 50) / 12.0) ** 2 < 1] = 2
    image = image + 0.5 * label.unsqueeze(1).float()
    proc = UnetProcessor(image_size=64)
    spacing = (2.5, 0.7, 0.6)
    b_all, b_cls, _, pred0 = valid_volumns(model, proc, image, label, nc, spacing=spacing)
    p, l = pred0.cpu().numpy()[None], label.numpy()
    taus = [t if t is not None else 1.0 for t in (_tau(s) for s in _sets(p, l, nc + 1, spacing))]
    m_all, m_cls, _, pred = valid_volumns(model, proc, image, label, nc, spacing=spacing, extended=True, tolerance=taus)
    assert torch.equal(pred, pred0)
    assert m_all.shape == (1, 7) and m_cls.shape == (1, nc, 7)
    assert torch.equal(_bits(m_all[:, :4].contiguous()), _bits(b_all)) and torch.equal(_bits(m_cls[..., :4].contiguous()), _bits(b_cls))
    hd_pct, assd, nsd, n = _want(p, l, nc + 1, spacing, 95.0, taus)
    got = np.concatenate([m_all.cpu().numpy()[:, None], m_cls.cpu().numpy()], 1).astype(np.float64)  # [1, nc + 1, 7]
    _close(got[..., 4], hd_pct, 1e-6)
    _close(got[..., 5], assd, 1e-5)
    _close(got[..., 6], nsd, 1e-6)
    np.testing.assert_array_equal(np.rint(got[..., 6] * n), np.rint(nsd * n))
