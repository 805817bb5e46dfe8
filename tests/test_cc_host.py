"""CPU checks of the connected-component clean-up: the scipy restatement against hand-written cases, the tensor backend of
`inference.components` against the restatement (root maps, `compact_ids`, every filter option; 2-D and 3-D, both
connectivities), the C-ABI declarations and argument checks of `mia_cc_*`, and the wiring into `UnetProcessor.postprocess` --
none of it needs a GPU.  All comparisons are exact."""
import os
import re

import numpy as np
import pytest
import torch

import _cc_ref as R
from test_processor_host import blobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 5 x 7.  Class 1: a diagonal pair at (0,0)-(1,1), and a 2 x 2 block at rows 3-4, columns 0-1.  Class 2: two pieces of three voxels
# each (the size tie), a row at (0,3..5) and a column at (2..4,6), that touch nowhere, not even diagonally.
HAND = np.array([[1, 0, 0, 2, 2, 2, 0],
                 [0, 1, 0, 0, 0, 0, 0],
                 [0, 0, 0, 0, 0, 0, 2],
                 [1, 1, 0, 0, 0, 0, 2],
                 [1, 1, 0, 0, 0, 0, 2]], dtype=np.int64)


def test_restatement_hand_written_cases():
    r4 = R.roots(HAND, 2, 1)
    want4 = np.array([[1, 0, 0, 4, 4, 4, 0],
                      [0, 9, 0, 0, 0, 0, 0],
                      [0, 0, 0, 0, 0, 0, 21],
                      [22, 22, 0, 0, 0, 0, 21],
                      [22, 22, 0, 0, 0, 0, 21]], dtype=np.int32)
    assert r4.dtype == np.int32 and np.array_equal(r4, want4)
    # the diagonal pair is one component under 8-connectivity and two under 4-connectivity
    r8 = R.roots(HAND, 2, 2)
    want8 = want4.copy()
    want8[1, 1] = 1
    assert np.array_equal(r8, want8)
    # foreground: classes merge where they touch -- here they do not, so only the keys change nothing
    assert np.array_equal(R.roots(HAND, 2, 1, foreground=True), want4)
    # keep the largest per class: class 1 keeps the 2 x 2 block; class 2 is a size tie and keeps the piece met first (the row)
    keep = R.filtered(HAND, True, 0, None, False, 0, 2, 1)
    want = HAND.copy()
    want[0, 0] = want[1, 1] = 0
    want[2:, 6] = 0
    assert np.array_equal(keep, want)
    # the whole foreground: only the 2 x 2 block (4 voxels) survives
    fgk = R.filtered(HAND, True, 0, None, True, 0, 2, 1)
    only = np.zeros_like(HAND)
    only[3:, :2] = 1
    assert np.array_equal(fgk, only)
    # min_size alone, a fill value, and a class list
    ms = R.filtered(HAND, False, 3, None, False, 7, 2, 1)
    want = HAND.copy()
    want[0, 0] = want[1, 1] = 7
    assert np.array_equal(ms, want)
    assert np.array_equal(R.filtered(HAND, False, 2, None, False, 7, 2, 1), want)   # two components of one voxel
    assert np.array_equal(R.filtered(HAND, False, 2, None, False, 7, 2, 2), HAND)   # one component of two voxels
    c2 = R.filtered(HAND, True, 0, (2,), False, 0, 2, 1)
    want = HAND.copy()
    want[2:, 6] = 0
    assert np.array_equal(c2, want)
    assert np.array_equal(R.compact(HAND, 2, 1), np.array([[1, 0, 0, 2, 2, 2, 0],
                                                          [0, 3, 0, 0, 0, 0, 0],
                                                          [0, 0, 0, 0, 0, 0, 4],
                                                          [5, 5, 0, 0, 0, 0, 4],
                                                          [5, 5, 0, 0, 0, 0, 4]], dtype=np.int32))


def _cases():
    """(name, labels, ndim) -- small, with every structure the definition distinguishes."""
    yield "hand", HAND, 2
    yield "random2d", R.random_labels((3, 17, 23), 0.59, 1), 2
    yield "dense2d", R.random_labels((2, 9, 31), 0.9, 2), 2
    yield "single", R.random_labels((13, 11), 0.5, 3), 2
    yield "blobs", blobs(2, 31, 43, seed=5), 2
    yield "random3d", R.random_labels((2, 4, 9, 13), 0.4, 4), 3
    yield "volume", R.random_labels((5, 8, 11), 0.59, 5), 3
    odd = R.random_labels((2, 12, 12), 0.6, 6, n_labels=5)
    odd[0, 0, :3] = -4      # out of range: no component, passes through
    odd[1, 5, 5] = 300
    yield "out_of_range", odd, 2
    yield "empty", np.zeros((2, 6, 7), dtype=np.int64), 2
    yield "full", np.ones((2, 6, 7), dtype=np.int64), 2


CASES = list(_cases())


@pytest.mark.parametrize("name,labels,ndim", CASES, ids=[c[0] for c in CASES])
def test_tensor_backend_matches_restatement(name, labels, ndim):
    from inference import compact_ids, connected_components, filter_components, keep_largest_component
    t = torch.from_numpy(labels)
    for conn in (1, ndim):
        for fg in (False, True):
            got = connected_components(t, ndim=ndim, connectivity=conn, n_classes=3, foreground=fg)
            assert got.dtype == torch.int32 and got.shape == t.shape
            assert np.array_equal(got.numpy(), R.roots(labels, ndim, conn, 3, fg)), (conn, fg)
            assert torch.equal(got, connected_components(t, ndim=ndim, connectivity=conn, n_classes=3, foreground=fg, backend="tensor"))
            if fg:
                ids = compact_ids(got, ndim=ndim)
                assert ids.dtype == torch.int32 and np.array_equal(ids.numpy(), R.compact(labels, ndim, conn, 3)), conn
            for keep, ms, fill in ((True, 0, 0), (False, 4, 0), (True, 3, 9), (False, 0, 0)):
                got = filter_components(t, keep_largest=keep, min_size=ms, foreground=fg, fill=fill, ndim=ndim, connectivity=conn,
                                        n_classes=3)
                assert got.dtype == t.dtype and got.shape == t.shape
                want = R.filtered(labels, keep, ms, None, fg, fill, ndim, conn, 3)
                assert np.array_equal(got.numpy(), want), (conn, fg, keep, ms, fill)
            if not fg:
                got = filter_components(t, classes=(2,), min_size=2, ndim=ndim, connectivity=conn, n_classes=3)
                assert np.array_equal(got.numpy(), R.filtered(labels, True, 2, (2,), False, 0, ndim, conn, 3)), conn
        assert torch.equal(keep_largest_component(t, ndim=ndim, connectivity=conn, n_classes=3),
                           filter_components(t, keep_largest=True, ndim=ndim, connectivity=conn, n_classes=3))


def test_n_classes_defaults_to_the_largest_label_and_other_dtypes():
    from inference import connected_components, filter_components
    labels = R.random_labels((2, 14, 15), 0.6, 11, n_labels=6)
    t = torch.from_numpy(labels)
    assert np.array_equal(connected_components(t).numpy(), R.roots(labels, 2, 1, 6))
    assert np.array_equal(filter_components(t).numpy(), R.filtered(labels, n_classes=6))
    t8 = t.to(torch.uint8)
    got = filter_components(t8, n_classes=6)
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), R.filtered(labels, n_classes=6))
    empty = torch.zeros((0, 4, 4), dtype=torch.int64)
    assert connected_components(empty).shape == (0, 4, 4) and filter_components(empty).shape == (0, 4, 4)


def test_python_argument_errors():
    from inference import connected_components, filter_components
    t = torch.from_numpy(HAND)
    for kw in ({"backend": "kernel"}, {"backend": "fast"}, {"ndim": 4}, {"connectivity": 3}, {"connectivity": 0}, {"n_classes": 257},
               {"ndim": 3}):
        with pytest.raises(ValueError):
            connected_components(t, **kw)
    with pytest.raises(ValueError):
        filter_components(t, backend="kernel")  # CPU tensors never reach the kernels
    with pytest.raises(ValueError):
        filter_components(t, classes=(1,), foreground=True)
    with pytest.raises(ValueError):
        filter_components(t, classes=(5,), n_classes=3)
    with pytest.raises(ValueError):
        filter_components(t, min_size=-1)
    with pytest.raises(ValueError):
        connected_components(t.float())


def test_header_declares_component_entry_points():
    import mia_hip
    protos = mia_hip.parse_header()
    assert len(protos["mia_cc_workspace"][1]) == 6
    assert len(protos["mia_cc_label"][1]) == 12
    assert len(protos["mia_cc_filter"][1]) == 17
    with open(os.path.join(ROOT, "include", "mia_hip.h")) as fh:
        txt = fh.read()
    sect = txt[txt.index("Connected components of int64 label maps"):]
    assert re.search(r"unet_processor\.py:121-125", sect) and ":72-113" in sect


def test_argument_errors_without_a_device():
    import ctypes
    import mia_hip
    lib = mia_hip.lib()
    one = ctypes.c_void_p(8)  # never dereferenced: every call below is turned down before any launch
    ok = (1, 2, 1, 8, 8, 1, 3, 0)  # nvol, ndim, d, h, w, connectivity, n_classes, foreground
    assert lib.mia_cc_label(None, one, *ok, one, None) == -1 and lib.mia_cc_label(one, None, *ok, one, None) == -1
    assert lib.mia_cc_label(one, one, *ok, None, None) == -1
    for bad in [(1, 4, 1, 8, 8, 1, 3, 0), (1, 1, 1, 8, 8, 1, 3, 0), (1, 2, 1, 8, 8, 3, 3, 0), (1, 2, 1, 8, 8, 0, 3, 0), (1, 3, 2, 8, 8, 2, 3, 0),
                (0, 2, 1, 8, 8, 1, 3, 0), (1, 2, 1, 0, 8, 1, 3, 0), (1, 2, 1, 8, -1, 1, 3, 0), (1, 2, 1, 8, 8, 1, 257, 0), (1, 2, 1, 8, 8, 1, 0, 0),
                (1, 3, 2048, 1024, 1024, 1, 3, 0)]:
        assert lib.mia_cc_label(one, one, *bad, one, None) == -1, bad
        assert lib.mia_cc_filter(one, ctypes.c_void_p(16), *bad, 1, 0, None, 0, one, one, None) == -1, bad
    assert b"mia_cc_filter" in lib.mia_last_error()
    two = ctypes.c_void_p(16)
    assert lib.mia_cc_filter(None, two, *ok, 1, 0, None, 0, one, one, None) == -1
    assert lib.mia_cc_filter(one, one, *ok, 1, 0, None, 0, one, one, None) == -1       # in place
    assert lib.mia_cc_filter(one, two, *ok, 1, 0, None, 0, None, one, None) == -1      # no workspace
    assert lib.mia_cc_filter(one, two, *ok, 1, 0, None, 0, ctypes.c_void_p(12), one, None) == -1  # misaligned workspace
    assert lib.mia_cc_filter(one, two, *ok, 1, -1, None, 0, one, one, None) == -1      # negative min_size
    with pytest.raises(mia_hip.MiaError):
        mia_hip.call("mia_cc_label", None, None, *ok, None, None)


def test_workspace_grows_with_the_volume():
    import mia_hip
    lib = mia_hip.lib()
    prev = 0
    for shape in [(1, 2, 1, 1, 1), (1, 2, 1, 61, 83), (32, 2, 1, 336, 544), (1, 3, 88, 576, 576), (88, 2, 1, 576, 576), (2, 3, 88, 576, 576)]:
        ws = lib.mia_cc_workspace(*shape, 3)
        voxels = shape[0] * shape[2] * shape[3] * shape[4]
        assert ws >= 2 * voxels and ws >= prev, shape  # a parent and a size per voxel, plus the winners
        assert ws <= 2 * voxels + 8 * shape[0] * shape[2] * 3 + 8
        prev = ws
    assert lib.mia_cc_workspace(88, 2, 1, 576, 576, 3) == lib.mia_cc_workspace(1, 3, 88, 576, 576, 3) + 2 * 87 * 3
    assert lib.mia_cc_workspace(1, 3, 2048, 1024, 1024, 3) < 0      # 2^31 voxels in one volume
    assert lib.mia_cc_workspace(1, 2, 1, 65536, 32768, 3) < 0       # 2^31 voxels in one image
    assert lib.mia_cc_workspace(2048, 2, 1, 1024, 1024, 3) < 0      # the workspace itself does not fit an int
    assert lib.mia_cc_workspace(1, 2, 1, 8, 8, 257) < 0 and lib.mia_cc_workspace(1, 5, 1, 8, 8, 3) < 0


def test_postprocess_default_is_the_old_call():
    from models.unet.unet_processor import UnetProcessor
    proc = UnetProcessor(image_size=[61, 83])  # no resize: that step runs on the GPU only
    masks = torch.from_numpy(blobs(3, 61, 83, seed=21))
    for P, shape, den in ((masks, (61, 83), False), (masks, (61, 83), True), (masks[0], (61, 83), True)):
        old = proc.postprocess(P, shape, den)
        assert torch.equal(proc.postprocess(P, shape, do_denoise=den), old)
        assert torch.equal(proc.postprocess(P, shape, do_denoise=den, keep_largest=None, min_component_size=0), old)


def test_postprocess_keep_largest_modes():
    from inference import filter_components
    from models.unet.unet_processor import UnetProcessor
    proc = UnetProcessor(image_size=None)
    masks = blobs(3, 61, 83, seed=23)
    t = torch.from_numpy(masks)
    for mode, kw in (("foreground", {"foreground": True}), ("per_class", {}), ((2,), {"classes": (2,)})):
        got = proc.postprocess(t, (61, 83), keep_largest=mode, n_classes=3)
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), R.filtered(masks, n_classes=3, **kw)), mode
        assert (got != t).any()  # the speckles are gone
    got = proc.postprocess(t, (61, 83), do_denoise=True, keep_largest="foreground", min_component_size=5)
    den = proc.postprocess(t, (61, 83), do_denoise=True)
    assert torch.equal(got, filter_components(den, foreground=True, min_size=5))  # applied last, after the denoise
    assert torch.equal(proc.postprocess(t, (61, 83), min_component_size=6, n_classes=3),
                       torch.from_numpy(R.filtered(masks, keep_largest=False, min_size=6)))
    with pytest.raises(ValueError):
        proc.postprocess(t, (61, 83), keep_largest="largest")


def test_predictor_passes_the_clean_up_on():
    from inference import EnsemblePredictor
    pred = EnsemblePredictor(32, folds=(0,), channels_list=[8, 16], device="cpu", keep_largest="foreground", min_component_size=4)
    assert pred.keep_largest == "foreground" and pred.min_component_size == 4 and pred.output_classes == 3
    plain = EnsemblePredictor(32, folds=(0,), channels_list=[8, 16], device="cpu")
    assert plain.keep_largest is None and plain.min_component_size == 0
