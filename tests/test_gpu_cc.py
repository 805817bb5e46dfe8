"""The connected-component kernels (csrc/components.hip) on the GPU: root maps and filtered maps bit for bit against the scipy
restatement (tests/_cc_ref.py) and against the tensor backend, with `check=True` on every kernel call.  Shapes that are no tile
multiples plus one real size; both connectivities, per class and foreground, labels in {0, 1, 2}; patterns that stress the merge
across tile borders and slices (percolating noise, serpentine, spiral, diagonals through tile corners, checkerboards, ties)."""
import functools

import numpy as np
import pytest
import torch

import _cc_ref as R

pytestmark = pytest.mark.gpu

SHAPES_2D = [(1, 1, 1), (3, 61, 83), (2, 130, 200), (2, 257, 255), (1, 336, 544)]
SHAPES_3D = [(2, 5, 40, 72), (1, 9, 70, 130)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _spiral(h, w):
    """A one-pixel square spiral from the top-left corner inwards, arms one empty pixel apart."""
    a = np.zeros((h, w), dtype=np.int64)
    y = x = 0
    dy, dx = 0, 1
    a[0, 0] = 1
    while True:
        moved = False
        for _ in range(2):
            ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < h and 0 <= nx < w and a[ny, nx] == 0 and not (0 <= fy < h and 0 <= fx < w and a[fy, fx]):
                y, x = ny, nx
                a[y, x] = 1
                moved = True
                break
            dy, dx = dx, -dy  # turn right
        if not moved:
            return a


def _serpentine(h, w):
    """One snake through every tile: every second row is full, and the rows are joined alternately at the right and the left end."""
    a = np.zeros((h, w), dtype=np.int64)
    a[0::2] = 1
    for y in range(1, h, 2):
        a[y, w - 1 if (y // 2) % 2 == 0 else 0] = 1
    return a


def _two_blobs(h, w):
    """Two squares of the same size (the tie), in different corners; a smaller third one."""
    a = np.zeros((h, w), dtype=np.int64)
    s = max(1, min(h, w) // 4)
    a[:s, w - s:] = 2
    a[h - s:, :s] = 2
    if min(h, w) >= 4:
        a[h // 2, w // 2] = 2
    return a


def patterns_2d(n, h, w):
    """name -> labels [n, h, w] in {0, 1, 2}."""
    yy, xx = np.mgrid[:h, :w]
    out = {}
    for dens in (0.3, 0.59, 0.9):  # 0.59 is near the percolation threshold: winding components across many tiles
        out[f"random{dens}"] = R.random_labels((n, h, w), dens, seed=int(dens * 100) + h)
    out["empty"] = np.zeros((n, h, w), dtype=np.int64)
    out["full"] = np.full((n, h, w), 2, dtype=np.int64)
    single = {
        "checkerboard": ((yy + xx) % 2).astype(np.int64),
        "checkerboard12": (1 + (yy + xx) % 2).astype(np.int64),
        # one-pixel diagonals of class 1 (x - y = 48 passes (15, 63) -> (16, 64)), anti-diagonals of class 2 ((15, 64) -> (16, 63))
        "diagonals": np.where((xx - yy) % 12 == 0, 1, np.where((xx + yy) % 12 == 7, 2, 0)).astype(np.int64),
        "serpentine": _serpentine(h, w),
        "spiral": _spiral(h, w),
        "stripes": (1 + xx % 2).astype(np.int64),
        "two_blobs": _two_blobs(h, w),
    }
    for name, a in single.items():  # the other images of the batch: mirrored, so that roots differ
        out[name] = np.stack([a if i % 2 == 0 else np.ascontiguousarray(a[::-1, ::-1]) for i in range(n)])
    return out


def patterns_3d(n, d, h, w):
    out = {}
    for dens in (0.3, 0.59, 0.9):
        out[f"random{dens}"] = R.random_labels((n, d, h, w), dens, seed=int(dens * 100) + d)
    out["empty"] = np.zeros((n, d, h, w), dtype=np.int64)
    out["full"] = np.ones((n, d, h, w), dtype=np.int64)
    zz, yy, xx = np.mgrid[:d, :h, :w]
    out["checkerboard"] = np.broadcast_to(((zz + yy + xx) % 2).astype(np.int64), (n, d, h, w)).copy()
    out["serpentine"] = np.broadcast_to(np.stack([_serpentine(h, w) if z % 2 == 0 else np.zeros((h, w), dtype=np.int64) for z in range(d)]),
                                        (n, d, h, w)).copy()
    out["serpentine"][:, 1::2, h - 1, 0] = 1  # one voxel in every slice between two snakes, below a snake's end or beside it
    a = np.zeros((d, h, w), dtype=np.int64)
    a[0, 4:12, 4:12] = 1        # two blobs of class 1, two slices apart ...
    a[2, 11:20, 11:20] = 1
    a[1, 11, 11] = 1            # ... joined only through this voxel of the slice between them
    a[3, 10:16, 58:64] = 2      # two blobs of class 2 in neighbouring slices that touch only diagonally, (15, 63) -> (16, 64),
    a[4, 16:21, 64:71] = 2      # across a tile corner: one component with 26 neighbours, two with 6
    a[4, 30:33, 5:8] = 2
    out["bridges"] = np.broadcast_to(a, (n, d, h, w)).copy()
    return out


def _check_all(pats, ndim, dev):
    from inference import connected_components, filter_components
    for name, labels in pats.items():
        t = torch.from_numpy(labels).to(dev)
        for conn in (1, ndim):
            for fg in (False, True):
                kw = dict(ndim=ndim, connectivity=conn, n_classes=3, foreground=fg)
                got = connected_components(t, backend="kernel", check=True, **kw)
                assert got.dtype == torch.int32 and got.shape == t.shape
                want = R.roots(labels, ndim, conn, 3, fg)
                assert np.array_equal(got.cpu().numpy(), want), (name, conn, fg, int((got.cpu().numpy() != want).sum()))
                assert torch.equal(got, connected_components(t, backend="tensor", **kw)), (name, conn, fg)
                got = filter_components(t, backend="kernel", check=True, **kw)
                want = R.filtered(labels, True, 0, None, fg, 0, ndim, conn, 3)
                assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), (name, conn, fg)
                assert torch.equal(got, filter_components(t, backend="tensor", **kw)), (name, conn, fg)


@pytest.mark.parametrize("shape", SHAPES_2D, ids=["x".join(map(str, s)) for s in SHAPES_2D])
def test_components_2d(shape):
    _check_all(patterns_2d(*shape), 2, _dev())


@pytest.mark.parametrize("shape", SHAPES_3D, ids=["x".join(map(str, s)) for s in SHAPES_3D])
def test_components_3d(shape):
    dev = _dev()
    pats = patterns_3d(*shape)
    a = pats["bridges"][0]
    # the patterns do what they are there for
    assert len(np.unique(R.roots(a, 3, 1)[a == 1])) == 1
    cut = np.where(np.arange(a.shape[0])[:, None, None] == 1, 0, a)  # without the slice that holds the bridge
    assert len(np.unique(R.roots(cut, 3, 3)[cut == 1])) == 2
    assert len(np.unique(R.roots(a, 3, 1)[a == 2])) == 3 and len(np.unique(R.roots(a, 3, 3)[a == 2])) == 2
    _check_all(pats, 3, dev)


@pytest.mark.parametrize("shape,ndim", [((2, 130, 200), 2), ((2, 5, 40, 72), 3)], ids=["2d", "3d"])
def test_min_size_fill_and_class_mask(shape, ndim):
    from inference import filter_components, keep_largest_component
    dev = _dev()
    labels = R.random_labels(shape, 0.59, seed=17)
    t = torch.from_numpy(labels).to(dev)
    for conn in (1, ndim):
        for fg in (False, True):
            for keep, ms, fill in ((False, 5, 0), (True, 5, 0), (False, 50, 7), (True, 1000000, 3)):
                kw = dict(keep_largest=keep, min_size=ms, foreground=fg, fill=fill, ndim=ndim, connectivity=conn, n_classes=3)
                got = filter_components(t, backend="kernel", check=True, **kw)
                want = R.filtered(labels, keep, ms, None, fg, fill, ndim, conn, 3)
                assert np.array_equal(got.cpu().numpy(), want), (conn, fg, keep, ms, fill)
                assert torch.equal(got, filter_components(t, backend="tensor", **kw))
        for classes in ((1,), (2,), (1, 2)):
            kw = dict(classes=classes, min_size=3, ndim=ndim, connectivity=conn, n_classes=3)
            got = filter_components(t, backend="kernel", check=True, **kw)
            assert np.array_equal(got.cpu().numpy(), R.filtered(labels, True, 3, classes, False, 0, ndim, conn, 3)), (conn, classes)
            assert torch.equal(got, filter_components(t, backend="tensor", **kw))
        assert torch.equal(keep_largest_component(t, ndim=ndim, connectivity=conn, n_classes=3, check=True),
                           filter_components(t, keep_largest=True, ndim=ndim, connectivity=conn, n_classes=3, backend="tensor"))


def test_out_of_range_labels_pass_through():
    from inference import compact_ids, connected_components, filter_components
    dev = _dev()
    labels = R.random_labels((2, 61, 83), 0.6, seed=31, n_labels=6)  # labels 3, 4, 5 are out of range for n_classes = 3
    labels[0, :7, :9] = -3
    labels[1, 30:40, 40:60] = 1 << 40
    t = torch.from_numpy(labels).to(dev)
    for conn in (1, 2):
        for fg in (False, True):
            kw = dict(connectivity=conn, n_classes=3, foreground=fg)
            roots = connected_components(t, backend="kernel", check=True, **kw)
            assert np.array_equal(roots.cpu().numpy(), R.roots(labels, 2, conn, 3, fg))
            assert bool((roots[t > 2] == 0).all()) and bool((roots[t < 0] == 0).all())
            got = filter_components(t, backend="kernel", check=True, fill=9, **kw)
            assert np.array_equal(got.cpu().numpy(), R.filtered(labels, True, 0, None, fg, 9, 2, conn, 3))
            assert torch.equal(got[(t > 2) | (t < 0)], t[(t > 2) | (t < 0)])
            if fg:
                assert np.array_equal(compact_ids(roots).cpu().numpy(), R.compact(labels, 2, conn, 3))
    # n_classes from the data: every label takes part
    assert np.array_equal(connected_components(t.clamp(0, 5), check=True).cpu().numpy(), R.roots(np.clip(labels, 0, 5), 2, 1, 6))


def test_same_call_twice_gives_equal_bits():
    from inference import connected_components, filter_components
    dev = _dev()
    t2 = torch.from_numpy(R.random_labels((2, 257, 255), 0.59, seed=41)).to(dev)
    t3 = torch.from_numpy(R.random_labels((1, 9, 70, 130), 0.45, seed=42)).to(dev)
    for t, ndim in ((t2, 2), (t3, 3)):
        for conn in (1, ndim):
            a = connected_components(t, ndim=ndim, connectivity=conn, n_classes=3, check=True)
            b = connected_components(t, ndim=ndim, connectivity=conn, n_classes=3, check=True)
            assert torch.equal(a, b)
            fa = filter_components(t, ndim=ndim, connectivity=conn, n_classes=3, min_size=4, check=True)
            fb = filter_components(t, ndim=ndim, connectivity=conn, n_classes=3, min_size=4, check=True)
            assert torch.equal(fa, fb)


def test_auto_backend_and_argument_errors_on_the_gpu():
    from inference import connected_components, filter_components
    dev = _dev()
    labels = R.random_labels((61, 83), 0.5, seed=51)
    t = torch.from_numpy(labels).to(dev)
    assert np.array_equal(connected_components(t, n_classes=3, check=True).cpu().numpy(), R.roots(labels))
    assert np.array_equal(filter_components(t, n_classes=3, check=True).cpu().numpy(), R.filtered(labels))
    strided = torch.from_numpy(np.ascontiguousarray(labels.T)).to(dev).T  # not contiguous
    assert np.array_equal(filter_components(strided, n_classes=3, backend="kernel", check=True).cpu().numpy(), R.filtered(labels))
    t32 = t.int()  # the kernels take int64 only: auto goes through the tensor ops, "kernel" refuses
    assert filter_components(t32, n_classes=3).dtype == torch.int32
    assert np.array_equal(filter_components(t32, n_classes=3).cpu().numpy(), R.filtered(labels))
    with pytest.raises(ValueError):
        filter_components(t32, n_classes=3, backend="kernel")
    with pytest.raises(ValueError):
        connected_components(t32, n_classes=3, backend="kernel")


def test_ensemble_predictor_keep_largest_end_to_end():
    from inference import EnsemblePredictor, filter_components
    from mia_hip import ops
    dev = _dev()
    pred = EnsemblePredictor(64, folds=(0, 1), channels_list=[16, 32, 64], device=dev, keep_largest="foreground", min_component_size=3)
    for i, net in enumerate(pred.models):
        torch.manual_seed(70 + i)
        net.load_state_dict(type(net)(2, 3, 3, [16, 32, 64]).state_dict())
    ops.bump_param_epoch()
    X = torch.rand(3, 3, 61, 83, generator=torch.Generator().manual_seed(5)) * 255.0
    for den in (False, True):
        cleaned = pred.predict_batch(X, do_denoise=den)
        pred.keep_largest, pred.min_component_size = None, 0
        plain = pred.predict_batch(X, do_denoise=den)
        pred.keep_largest, pred.min_component_size = "foreground", 3
        assert cleaned.shape == (3, 61, 83) and cleaned.dtype == torch.int64 and cleaned.is_cuda
        assert torch.equal(cleaned, filter_components(plain, foreground=True, min_size=3, n_classes=3, check=True))
        assert np.array_equal(cleaned.cpu().numpy(), R.filtered(plain.cpu().numpy(), True, 3, None, True, 0, 2, 1, 3))
