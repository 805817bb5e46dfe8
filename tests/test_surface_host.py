"""CPU checks of the surface-distance metrics (HD / ASD of calculate_metric_percase): the float64 restatement against the
brute-force definitions, the C-ABI argument checks and workspace bound of mia_surface_distance, and the Python wrappers'
argument checks -- none of it needs a GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import mia_hip
from _surface_ref import asd, brute_asd, brute_hd, hd


def _cases():
    rng = np.random.default_rng(11)
    out = []
    for i in range(50):
        ndim = 2 if i % 2 == 0 else 3
        shape = tuple(int(v) for v in rng.integers(1, 9, size=ndim)) if ndim == 3 else tuple(int(v) for v in rng.integers(1, 17, size=2))
        kind = i % 5
        if kind == 0:    # random sparse / dense
            a, b = rng.random(shape) < 0.3, rng.random(shape) < 0.5
        elif kind == 1:  # single pixels
            a, b = np.zeros(shape, bool), np.zeros(shape, bool)
            a[tuple(rng.integers(0, s) for s in shape)] = True
            b[tuple(rng.integers(0, s) for s in shape)] = True
        elif kind == 2:  # full array vs a random mask
            a, b = np.ones(shape, bool), rng.random(shape) < 0.2
        elif kind == 3:  # edge-touching boxes
            a, b = np.zeros(shape, bool), np.zeros(shape, bool)
            a[(slice(0, max(1, shape[0] // 2)),) + (slice(None),) * (ndim - 1)] = True
            b[(slice(None),) * (ndim - 1) + (slice(shape[-1] // 2, None),)] = True
        else:            # full vs full
            a, b = np.ones(shape, bool), np.ones(shape, bool)
        if not b.any():
            b[(0,) * ndim] = True
        if not a.any():
            a[tuple(s - 1 for s in shape)] = True
        spacing = None if i % 3 == 0 else tuple(float(v) for v in rng.uniform(0.3, 2.5, size=ndim))
        out.append((a, b, spacing))
    return out


@pytest.mark.parametrize("case", range(50))
def test_restatement_equals_brute_force(case):
    a, b, s = _cases()[case]
    assert math.isclose(hd(a, b, s), brute_hd(a, b, s), rel_tol=1e-12, abs_tol=1e-12)
    assert math.isclose(asd(a, b, s), brute_asd(a, b, s), rel_tol=1e-12, abs_tol=1e-12)


def test_one_slice_volume_border_differs_from_the_image():
    """In a [1,H,W] volume every foreground voxel is a border voxel (its neighbours along D lie outside); in the [H,W] image only
    the rim is.  Both restatements agree with the brute force, and the two ASDs differ."""
    yy, xx = np.mgrid[:20, :24]
    a = (yy - 9) ** 2 + (xx - 11) ** 2 < 36
    b = (yy - 10) ** 2 + (xx - 13) ** 2 < 30
    a3, b3 = a[None], b[None]
    assert math.isclose(asd(a, b), brute_asd(a, b), rel_tol=1e-12)
    assert math.isclose(asd(a3, b3), brute_asd(a3, b3), rel_tol=1e-12)
    assert abs(asd(a, b) - asd(a3, b3)) > 0.1
    assert hd(a, b) == hd(a3, b3)


def test_empty_set_rules():
    z, o = np.zeros((4, 5), bool), np.ones((4, 5), bool)
    assert math.isnan(hd(z, o)) and math.isnan(asd(z, o)) and math.isnan(hd(z, z))
    assert hd(o, z) == math.inf and asd(o, z) == math.inf


def _err(rc):
    l = mia_hip.lib()
    assert rc < 0
    return l.mia_last_error().decode()


def _call(**kw):
    args = dict(pred=1, labels=1, nvol=1, ndim=2, d=1, h=8, w=8, k1=2, sd=1.0, sh=1.0, sw=1.0, ws=1, hd=1, asd=1)
    args.update(kw)
    ptr = lambda v: None if v is None else ctypes.c_void_p(16 * v)  # never dereferenced: the checks fail before any launch
    return mia_hip.lib().mia_surface_distance(ptr(args["pred"]), ptr(args["labels"]), args["nvol"], args["ndim"], args["d"], args["h"],
                                              args["w"], args["k1"], ctypes.c_float(args["sd"]), ctypes.c_float(args["sh"]),
                                              ctypes.c_float(args["sw"]), ptr(args["ws"]), ptr(args["hd"]), ptr(args["asd"]), None)


def test_abi_argument_errors_without_a_gpu():
    assert "k1=0" in _err(_call(k1=0))
    assert "k1=9" in _err(_call(k1=9))
    assert "d == 1" in _err(_call(ndim=2, d=2))
    assert "ndim=4" in _err(_call(ndim=4))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert "spacing" in _err(_call(ndim=3, d=2, sd=bad))
        assert "spacing" in _err(_call(sh=bad))
        assert "spacing" in _err(_call(sw=bad))
    for name in ("pred", "labels", "ws", "hd", "asd"):
        assert "null" in _err(_call(**{name: None}))
    assert "limits" in _err(_call(ndim=3, d=1025))
    assert "limits" in _err(_call(w=4097))
    with pytest.raises(mia_hip.MiaError):
        mia_hip.call("mia_surface_distance", None, None, 1, 2, 1, 8, 8, 2, ctypes.c_float(1), ctypes.c_float(1), ctypes.c_float(1),
                     None, None, None, None)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (4, 1, 37, 61), (32, 1, 336, 544), (2, 5, 40, 33), (1, 88, 576, 576),
                                   (1, 1024, 512, 512), (7, 3, 4096, 17)])
def test_workspace_bound(shape):
    l = mia_hip.lib()
    vox = int(np.prod(shape))
    for k1 in range(1, 9):
        ws = l.mia_surface_distance_workspace(*shape, k1)
        assert 0 < ws <= 4 * vox + (1 << 20), (shape, k1, ws)
    if shape == (1, 88, 576, 576):
        assert l.mia_surface_distance_workspace(*shape, 8) * 4 < (1 << 29)  # under 0.5 GiB


def test_workspace_reports_overflow():
    l = mia_hip.lib()
    assert l.mia_surface_distance_workspace(200, 1024, 4096, 4096, 1) < 0
    assert l.mia_surface_distance_workspace(1, 1, 8, 8, 0) < 0
    assert l.mia_surface_distance_workspace(1, 1, 8, 8, 9) < 0


def test_python_wrappers_reject_bad_arguments_before_any_launch():
    from metric.segmentation import percase_metrics, surface_distances, valid_volumns
    p2, p3 = torch.zeros(2, 8, 8, dtype=torch.long), torch.zeros(1, 3, 8, 8, dtype=torch.long)
    for fn, k in ((surface_distances, 2), (percase_metrics, 1)):
        with pytest.raises(mia_hip.MiaError):  # CPU tensors: no CPU fallback
            fn(p2, p2, k)
        with pytest.raises(mia_hip.MiaError):
            fn(p3, p3, k, spacing=(2.0, 1.0, 1.0))
        with pytest.raises(ValueError):
            fn(p2, torch.zeros(2, 8, 9, dtype=torch.long), k)
        with pytest.raises(ValueError):
            fn(torch.zeros(8, 8, dtype=torch.long), torch.zeros(8, 8, dtype=torch.long), k)
        for bad in ((1.0,), (1.0, 1.0, 1.0), (1.0, 0.0), (float("nan"), 1.0)):
            with pytest.raises(ValueError):
                fn(p2, p2, k, spacing=bad)
        for bad in ((1.0, 1.0), (1.0, -1.0, 1.0)):
            with pytest.raises(ValueError):
                fn(p3, p3, k, spacing=bad)
    with pytest.raises(AssertionError):  # one volume per call, as the reference asserts
        valid_volumns(torch.nn.Linear(1, 1), None, torch.zeros(2, 1, 3, 8, 8), torch.zeros(2, 3, 8, 8, dtype=torch.long), 1)
