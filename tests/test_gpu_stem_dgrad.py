"""Bit-exact integer probes of the stem input gradient (csrc/stem_dgrad.hip: mia_stem_dgrad), in the manner of test_gpu_conv_exact.py.

dy holds integers in [-3, 3] and w integers in [-2, 2]: every product is exact in bf16 and fp32 and every fp32 partial sum is an integer
below 2^24 (tests/test_vat_host.py checks that on the reference for every row), so the result of any correct kernel is the fp64 result.
All comparisons are torch.equal; there is no tolerance in this file."""
import ctypes

import pytest
import torch

import _vat_ref as V

pytestmark = pytest.mark.gpu
DT = {"bf16": torch.bfloat16, "fp32": torch.float32}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _run(dy_nhwc, w2, n, h, w, c0):
    from mia_hip import ops
    dx = torch.full((n, h, w), float("nan"), device=dy_nhwc.device, dtype=torch.float32)
    ops.call("mia_stem_dgrad", ops._p(dy_nhwc), ops._dt(dy_nhwc), ops._p(w2), ops._p(dx), n, h, w, c0, ops._stream())
    return dx


@pytest.mark.parametrize("row", range(len(V.PROBES)), ids=[f"{d}-c{c}-{'x'.join(map(str, s))}" for d, c, s in V.PROBES])
def test_stem_dgrad_integer_probe(row):
    dev = _dev()
    dt, c0, (n, h, w) = V.PROBES[row]
    dy, wt = V.probe_operands(c0, (n, h, w), 1000 + row)
    ref = V.stem_dgrad(dy, wt).float()
    dy_dev = dy.permute(0, 2, 3, 1).contiguous().to(device=dev, dtype=DT[dt])
    w_dev = wt.float().to(dev)
    got = _run(dy_dev, w_dev, n, h, w, c0)
    assert torch.equal(got.cpu(), ref)
    again = _run(dy_dev, w_dev, n, h, w, c0)  # run to run: equal bits
    assert torch.equal(got, again)


def test_stem_dgrad_bad_arguments_raise_before_any_launch():
    from mia_hip import MiaError, ops
    dev = _dev()
    w = torch.zeros(260 * 9, device=dev)
    dy = torch.zeros(2 * 4 * 4 * 260, device=dev, dtype=torch.bfloat16)
    dx = torch.full((2, 4, 4), 7.0, device=dev)
    for dtype, n, h, wd, c0 in ((ops.BF16, 2, 4, 4, 6), (ops.F32, 2, 4, 4, 6), (ops.BF16, 2, 4, 4, 260), (ops.BF16, 2, 0, 4, 64),
                                (5, 2, 4, 4, 64)):
        with pytest.raises(MiaError):
            ops.call("mia_stem_dgrad", ops._p(dy), dtype, ops._p(w), ops._p(dx), n, h, wd, c0, ops._stream())
    with pytest.raises(MiaError):
        ops.call("mia_stem_dgrad", None, ops.BF16, ops._p(w), ops._p(dx), 2, 4, 4, 64, ops._stream())
    torch.cuda.synchronize()
    assert bool((dx == 7.0).all())  # nothing was launched
