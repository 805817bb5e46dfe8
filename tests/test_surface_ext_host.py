"""CPU checks of the symmetric surface metrics (HD95 / ASSD / surface Dice: mia_surface_metrics, metric.segmentation.surface_metrics):
the float64 restatement against brute-force pairwise definitions, the empty-set rules, the C-ABI argument checks and workspace bound,
and the Python wrappers' argument checks -- none of it needs a GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import mia_hip
from _surface_ext_ref import brute_ext_metrics, ext_metrics, ext_table, percentile_linear
from test_surface_host import _cases


@pytest.mark.parametrize("case", range(50))
def test_restatement_equals_brute_force(case):
    a, b, s = _cases()[case]
    for q in (50.0, 95.0, 99.9, 100.0):
        got, want = ext_metrics(a, b, s, q, 1.5), brute_ext_metrics(a, b, s, q, 1.5)
        for g, w in zip(got, want):
            assert math.isclose(g, w, rel_tol=1e-12, abs_tol=1e-12), (q, got, want)


def test_percentile_formula_is_numpys_linear_method():
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 20, 21, 118, 1001):
        v = rng.random(n) * 7
        for q in (0.1, 50.0, 95.0, 99.9, 100.0):
            assert math.isclose(percentile_linear(v, q), float(np.percentile(v, q)), rel_tol=1e-14, abs_tol=0)


def test_empty_set_rules():
    z, o = np.zeros((4, 5), bool), np.ones((4, 5), bool)
    for a, b in ((z, o), (z, z)):
        h, s, n = ext_metrics(a, b)
        assert math.isnan(h) and math.isnan(s) and n == 0.0
    assert ext_metrics(o, z) == (math.inf, math.inf, 0.0)
    lab = np.zeros((4, 5), np.int64)
    lab[1, 2] = 1
    h, s, n = ext_table(np.zeros_like(lab), lab, 2, None, 95.0, (1.0, 2.0))
    assert np.isnan(h).all() and np.isnan(s).all() and (n == 0).all()
    h, s, n = ext_table(lab, lab, 2)
    assert (h == 0).all() and (s == 0).all() and (n == 1).all()


def _err(rc):
    assert rc < 0
    return mia_hip.lib().mia_last_error().decode()


def _call(**kw):
    args = dict(pred=1, labels=1, nvol=1, ndim=2, d=1, h=8, w=8, k1=2, sd=1.0, sh=1.0, sw=1.0, percentile=95.0, tol=(1.0, 1.0), ws=1,
                hd=1, asd=1, hd_pct=1, assd=1, nsd=1)
    args.update(kw)
    ptr = lambda v: None if v is None else ctypes.c_void_p(16 * v)  # never dereferenced: the checks fail before any launch
    tol = None if args["tol"] is None else (ctypes.c_float * len(args["tol"]))(*args["tol"])
    return mia_hip.lib().mia_surface_metrics(ptr(args["pred"]), ptr(args["labels"]), args["nvol"], args["ndim"], args["d"], args["h"],
                                             args["w"], args["k1"], ctypes.c_float(args["sd"]), ctypes.c_float(args["sh"]),
                                             ctypes.c_float(args["sw"]), ctypes.c_double(args["percentile"]), tol, ptr(args["ws"]),
                                             ptr(args["hd"]), ptr(args["asd"]), ptr(args["hd_pct"]), ptr(args["assd"]), ptr(args["nsd"]),
                                             None)


def test_abi_argument_errors_without_a_gpu():
    for bad in (0.0, -1.0, 100.5, float("nan")):
        assert "percentile" in _err(_call(percentile=bad))
    for bad in ((-0.5, 1.0), (1.0, float("nan")), (float("inf"), 1.0)):
        assert "tolerance" in _err(_call(tol=bad))
    for name in ("pred", "labels", "tol", "ws", "hd", "asd", "hd_pct", "assd", "nsd"):
        assert "null" in _err(_call(**{name: None}))
    # inherited from mia_surface_distance
    assert "k1=0" in _err(_call(k1=0, tol=(1.0,)))
    assert "k1=9" in _err(_call(k1=9, tol=(1.0,) * 9))
    assert "d == 1" in _err(_call(ndim=2, d=2))
    assert "ndim=4" in _err(_call(ndim=4))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert "spacing" in _err(_call(ndim=3, d=2, sd=bad))
        assert "spacing" in _err(_call(sh=bad))
        assert "spacing" in _err(_call(sw=bad))
    assert "limits" in _err(_call(ndim=3, d=1025))
    assert "limits" in _err(_call(w=4097))
    assert "limits" in _err(_call(nvol=4097))
    with pytest.raises(mia_hip.MiaError):
        mia_hip.call("mia_surface_metrics", None, None, 1, 2, 1, 8, 8, 2, ctypes.c_float(1), ctypes.c_float(1), ctypes.c_float(1),
                     ctypes.c_double(95.0), None, None, None, None, None, None, None, None)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (4, 1, 37, 61), (32, 1, 336, 544), (2, 5, 40, 33), (1, 88, 576, 576),
                                   (1, 1024, 512, 512), (7, 3, 4096, 17)])
def test_workspace_bound(shape):
    l = mia_hip.lib()
    vox = int(np.prod(shape))
    for k1 in range(1, 9):
        ws = l.mia_surface_metrics_workspace(*shape, k1)
        assert l.mia_surface_distance_workspace(*shape, k1) < ws <= 5 * vox + (1 << 20), (shape, k1, ws)


def test_workspace_reports_overflow():
    l = mia_hip.lib()
    assert l.mia_surface_metrics_workspace(200, 1024, 4096, 4096, 1) < 0
    assert l.mia_surface_metrics_workspace(1, 1, 8, 8, 0) < 0
    assert l.mia_surface_metrics_workspace(1, 1, 8, 8, 9) < 0
    assert l.mia_surface_metrics_workspace(4096, 1, 8, 8, 1) > 0
    assert l.mia_surface_metrics_workspace(4097, 1, 8, 8, 1) < 0


def test_python_wrappers_reject_bad_arguments_before_any_launch():
    from metric.segmentation import percase_metrics, surface_metrics, valid_slices, valid_volumns
    p2, p3 = torch.zeros(2, 8, 8, dtype=torch.long), torch.zeros(1, 3, 8, 8, dtype=torch.long)
    ext = lambda pred, lab, k, **kw: percase_metrics(pred, lab, k, extended=True, **kw)
    for fn, k, ntol in ((surface_metrics, 2, 2), (ext, 1, 2)):
        with pytest.raises(mia_hip.MiaError):  # CPU tensors: no CPU fallback
            fn(p2, p2, k)
        with pytest.raises(mia_hip.MiaError):
            fn(p3, p3, k, spacing=(2.0, 1.0, 1.0), percentile=50, tolerance=(0.5,) * ntol)
        with pytest.raises(ValueError):
            fn(p2, torch.zeros(2, 8, 9, dtype=torch.long), k)
        with pytest.raises(ValueError):
            fn(torch.zeros(8, 8, dtype=torch.long), torch.zeros(8, 8, dtype=torch.long), k)
        for bad in ((1.0,), (1.0, 1.0, 1.0), (1.0, 0.0), (float("nan"), 1.0)):
            with pytest.raises(ValueError):
                fn(p2, p2, k, spacing=bad)
        for bad in (0, -1.0, 100.5, float("nan")):
            with pytest.raises(ValueError):
                fn(p2, p2, k, percentile=bad)
        for bad in (-1.0, float("nan"), float("inf"), (1.0,) * (ntol + 1), (1.0, -2.0), torch.ones(ntol + 2)):
            with pytest.raises(ValueError):
                fn(p2, p2, k, tolerance=bad)
    for bad in (0, 9):
        with pytest.raises(ValueError):
            surface_metrics(p2, p2, bad)
    with pytest.raises(ValueError):  # the extra columns belong to the full table
        valid_slices(torch.nn.Linear(1, 1), None, torch.zeros(1, 1, 8, 8), torch.zeros(1, 8, 8, dtype=torch.long), 1, extended=True)
    with pytest.raises(AssertionError):  # one volume per call, as the reference asserts
        valid_volumns(torch.nn.Linear(1, 1), None, torch.zeros(2, 1, 3, 8, 8), torch.zeros(2, 3, 8, 8, dtype=torch.long), 1, extended=True)
