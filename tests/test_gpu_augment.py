"""GPU checks of the augmentation / resize / normalisation kernels (csrc/augment.hip) at kernel level against the float64 restatement in
tests/_augment_ref.py (affine and elastic: against oracle/transforms_ref.py, which is bit-exact for them), called through the C ABI
(mia_hip.call) or the transforms.functional_hip wrappers.  Every comparison covers EVERY element of the output; skipped samples
(apply = -1) must keep the sentinel their output buffer was filled with.

What is pinned -> test:
  second trip of every grid-stride loop (> 8192 * 256 work items), distinct parameters per sample
      blur, the four element-wise ops, noise, bilinear, antialiased (both passes), nearest, rot90, crop ... test_grid_stride_*
      affine / elastic, 16-byte path (33 x 512 x 512) and scalar path (W % 4 != 0) ..................... test_grid_stride_warps
      copy_selected (33 x 512 x 512 words) ............................................................. test_grid_stride_copy_selected
  sample statistics: n = 1, n < 64 slabs, luma, low-contrast and raw-intensity images, selective ...... test_sample_stats*, test_hard_stats_zscore
  blur: mixed kernel sizes in one batch, k = 1, k = 9 on 5 x 5 and 5 x 64, C = 3, apply flags ......... test_blur_*
  element-wise: in place == out of place, gamma at 0 and 1, contrast clamping, z-score of zeros ....... test_elementwise_*
  noise: known answer of quad 0, quads spanning samples, ragged total, flags, high counter words ...... test_noise_*
  bilinear / antialiased / nearest / low-res at the sizes of _augment_ref's tables ..................... test_resize_*, test_lowres
  resize_bilinear_bwd against the adjoint, h = 1, w = 1, identity ..................................... test_resize_bilinear_bwd
  rot90 x flips x non-square x 4 / 8 bytes, crop windows at both corners ............................... test_rot90_flip_all, test_crop_windows

Tolerances.  Bit-equal: nearest, rot90, crop, copy_selected, affine / elastic label maps, every apply = 0 / -1 sample, in place against out
of place.  The project's ceilings otherwise: blur 2e-6, contrast / gamma 2e-6, z-score 2e-5, bilinear / antialiased 3e-6, low-res 2e-6,
elastic image 1e-6 (images in [0, 1]).  Statistics: mean within 4 fp32 ulp of max |x|, std to 1e-6 relative.  resize_bilinear_bwd:
|error| <= (K + 3) 2^-24 sum |w g| per element (K output pixels add into it, in arbitrary order; each term carries the roundings of two
weights and two products).  Noise: the normals depend on the device's logf / cosf / sinf / sqrtf; NOISE_Z_TOL below is 4 x the error
measured against the float64 restatement."""
import ctypes

import numpy as np
import pytest
import torch

import _augment_ref as A
from oracle import transforms_ref as T

pytestmark = pytest.mark.gpu

BLUR_TOL, EW_TOL, Z_TOL, RESIZE_TOL, LOWRES_TOL, ELASTIC_TOL = 2e-6, 2e-6, 2e-5, 3e-6, 2e-6, 1e-6
STD_RTOL = 1e-6
# max |z_gpu - z_ref| over the 8.65 M normals of test_noise_normals_measured, measured on an MI355X: 6.99e-7; the tolerance is 4 x that
# (margin for another compiler version's logf / cosf / sinf / sqrtf), far below the 1e-5 above which the restatement or the kernel is wrong
NOISE_Z_MEASURED = 7.0e-7
NOISE_Z_TOL = 4 * NOISE_Z_MEASURED
S = A.SENTINEL


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _abi():
    from mia_hip import call
    from mia_hip.ops import _c_i64, _p, _stream
    return call, _p, _c_i64, _stream


def _fh():
    from transforms import functional_hip as FH
    return FH


def dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def err(got, want):
    """max |got - want| over every element; the output must be finite everywhere."""
    g = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    w = np.asarray(want, dtype=np.float64)
    assert g.shape == w.shape, (g.shape, w.shape)
    assert np.isfinite(g).all(), "an output element was never written (or is not finite)"
    return float(np.abs(g - w).max())


def same(got, want):
    g = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    w = np.asarray(want)
    return g.shape == w.shape and np.array_equal(g, w.astype(g.dtype))


_CACHE = {}


def base512():
    """[9, 1, 512, 512] fp32: nine cheap variations of one image (a read-only shared input of the grid-stride cases)."""
    if "b9" not in _CACHE:
        _CACHE["b9"] = A.batch_of(A.image((1, 512, 512), 1), 9)
        _CACHE["b9"].setflags(write=False)
    return _CACHE["b9"]


def ints(dev, vals):
    return torch.tensor([int(v) for v in vals], dtype=torch.int32, device=dev)


def flts(dev, vals):
    return torch.from_numpy(np.asarray(vals, dtype=np.float32)).to(dev)


# =========================================================================== grid-stride loops
def test_grid_stride_blur():
    call, _p, _i64, _st = _abi()
    dev = _dev()
    x = base512()
    ks = [1, 3, 5, 7, 9, 3, 5, 7, 9]
    sg = [0.4 + 0.17 * b for b in range(9)]
    assert x.size > A.GRID_CAP
    xd = dv(x, dev)
    out = torch.full_like(xd, S)
    sgd, ksd = flts(dev, sg), ints(dev, ks)  # held across the launch
    call("mia_gaussian_blur", _p(xd), _p(out), 9, 1, 512, 512, _p(sgd), _p(ksd), 9, None, _st())
    assert err(out, A.blur(x, sg, ks)) < BLUR_TOL


def test_grid_stride_elementwise():
    FH = _fh()
    dev = _dev()
    x = base512()
    xd = dv(x, dev)
    p0 = [0.7 + 0.1 * b for b in range(9)]
    ms = np.array([[0.3 + 0.02 * b, 0.1 + 0.03 * b] for b in range(9)], dtype=np.float32)
    msd = dv(ms, dev)
    aux = (A.batch_of(A.image((1, 512, 512), 2), 9).astype(np.float64) - 0.4).astype(np.float32)
    assert err(FH.elementwise(xd, FH.EW_GAMMA, p0=p0), A.elementwise(x, A.EW_GAMMA, p0=p0)) < EW_TOL
    f = [0.5 + 0.25 * b for b in range(9)]
    assert err(FH.elementwise(xd, FH.EW_CONTRAST, p0=f, mean_std=msd), A.elementwise(x, A.EW_CONTRAST, p0=f, mean_std=ms)) < EW_TOL
    assert err(FH.elementwise(xd, FH.EW_NOISE, aux=dv(aux, dev)), A.elementwise(x, A.EW_NOISE, aux=aux)) < 2.0 ** -23
    # z-score: |z| up to 1 / 0.1 = 10 here; the op is one subtraction and one division: relative 2^-23
    want = A.elementwise(x, A.EW_ZSCORE, mean_std=ms)
    assert err(FH.elementwise(xd, FH.EW_ZSCORE, mean_std=msd), want) < np.abs(want).max() * 2.0 ** -22


@pytest.mark.parametrize("nb", [9, 33])
def test_grid_stride_noise(nb):
    """nb = 33: 2.16 M quads, the noise kernel's loop (one quad per work item) takes its second trip; nb = 9: 2.36 M elements."""
    FH = _fh()
    dev = _dev()
    x = A.batch_of(A.image((1, 512, 512), 3), nb)
    sg = [0.01 + 0.003 * b for b in range(nb)]
    assert (x.size + 3) // 4 > A.GRID_CAP or nb == 9
    out = FH.noise_clip(dv(x, dev), sg, seed=77, offset=5)
    assert err(out, A.noise_clip(x, sg, 77, 5)) < max(sg) * NOISE_Z_TOL + 2.0 ** -23


def test_grid_stride_resize_bilinear():
    FH = _fh()
    dev = _dev()
    x = A.batch_of(A.image((1, 384, 384), 4), 9)
    assert 9 * 512 * 512 > A.GRID_CAP
    assert err(FH.resize_bilinear(dv(x, dev), 512, 512), A.resize_bilinear(x, 512, 512)) < RESIZE_TOL


@pytest.mark.parametrize("size", [(256, 512), (1024, 256)], ids=["pass_w", "pass_h"])
def test_grid_stride_resize_aa(size):
    """(256, 512): the pass along W writes 9 * 512 * 512 items; (1024, 256): the pass along H writes 9 * 1024 * 256.  Scales 2, 1 and 0.5
    are exact in fp32, so the tap arithmetic is exact at coordinates up to 512 too."""
    FH = _fh()
    dev = _dev()
    x = base512()
    oh, ow = size
    assert max(9 * 512 * ow, 9 * oh * ow) > A.GRID_CAP
    assert err(FH.resize_bilinear(dv(x, dev), oh, ow, antialias=True), A.resize_aa(x, oh, ow)) < RESIZE_TOL


def test_grid_stride_resize_nearest():
    FH = _fh()
    dev = _dev()
    x = A.batch_of(A.image((1, 384, 384), 5), 9)
    assert same(FH.resize_nearest(dv(x, dev), 512, 512), A.resize_nearest(x, 512, 512))
    lab = (np.arange(9 * 384 * 384, dtype=np.int64) * 2654435761 % (1 << 40)).reshape(9, 384, 384)
    assert same(FH.resize_nearest(dv(lab, dev), 512, 512), A.resize_nearest(lab, 512, 512))


def test_grid_stride_rot90_and_crop():
    FH = _fh()
    dev = _dev()
    x = A.batch_of(A.image((1, 512, 520), 6), 9)
    assert 9 * 512 * 520 > A.GRID_CAP
    assert same(FH.rot90_flip(dv(x, dev), 1, True, False), A.rot90_flip(x, 1, True, False))
    assert same(FH.rot90_flip(dv(x, dev), 2, False, True), A.rot90_flip(x, 2, False, True))
    big = A.batch_of(A.image((1, 520, 530), 7), 9)
    top, left = [b % 9 for b in range(9)], [(2 * b + 1) % 19 for b in range(9)]
    top[8], left[8] = 8, 18  # flush with the bottom-right corner
    assert same(FH.crop(dv(big, dev), top, left, 512, 512), A.crop(big, top, left, 512, 512))


def test_grid_stride_copy_selected():
    call, _p, _i64, _st = _abi()
    dev = _dev()
    nb, per = 33, 512 * 512
    assert nb * per // 4 > A.GRID_CAP
    src = torch.arange(nb * per, dtype=torch.int32, device=dev).view(nb, per)
    dst = torch.full_like(src, -7)
    ap = [1 if b % 3 == 0 else (0 if b % 3 == 1 else -1) for b in range(nb)]
    apd = ints(dev, ap)
    call("mia_copy_selected", _p(src), _p(dst), _i64(per * 4), nb, _p(apd), _st())
    want = torch.where(torch.tensor([a > 0 for a in ap], device=dev)[:, None], src, torch.full_like(src, -7))
    assert torch.equal(dst, want)


def _warp_inputs(nb, h, w):
    base = A.image((1, h, w), 8)
    img = A.batch_of(base, nb)
    lab = ((np.arange(h * w, dtype=np.int64).reshape(1, h, w) * 7919) % 5 + np.arange(nb, dtype=np.int64).reshape(nb, 1, 1)) % 7
    idx = torch.arange(1, h * w + 1, dtype=torch.long).reshape(1, h, w)  # an index image: 0 marks "outside"
    return img, lab, idx


def _gather(idx_out, img, lab):
    src = idx_out.numpy().reshape(-1) - 1
    inside = src >= 0
    wi = np.where(inside, img.reshape(-1)[np.maximum(src, 0)], np.float32(0)).reshape(img.shape)
    wl = np.where(inside, lab.reshape(-1)[np.maximum(src, 0)], 0).reshape(lab.shape)
    return wi, wl


@pytest.mark.parametrize("shape", [(33, 512, 512), (9, 512, 457)], ids=["vec4", "scalar"])
def test_grid_stride_warps(shape):
    """Affine (nearest) and elastic warps of image + int64 label with a matrix / displacement grid of its own per sample.  The source index of
    every output pixel comes from the oracle run on an index image (it is bit-exact for both warps); image and label are gathered
    with it, so the per-sample cost on the CPU is one index map."""
    from transforms.joint_transform import inverse_affine_matrix
    FH = _fh()
    dev = _dev()
    nb, h, w = shape
    assert nb * h * w // (4 if w % 4 == 0 else 1) > A.GRID_CAP
    img, lab, idx = _warp_inputs(nb, h, w)
    # five matrices, sample b takes number b % 5 (the oracle's index map costs 0.4 s per 512 x 512 map): a sample index taken from the
    # first trip is off by 32 (vec4) or 8 (scalar) samples, which 5 does not divide; image and label differ for every sample anyway
    par = [(-20.0 + 9.5 * j, (j - 2, j % 3 - 1), 0.8 + 0.13 * j, (float(j % 4), 0.0)) for j in range(5)]
    maps = [T.apply_affine(idx, a, tr, sc, sh) for a, tr, sc, sh in par]
    mats = [inverse_affine_matrix([0.0, 0.0], a, [1.0 * t for t in tr], sc, list(sh)) for a, tr, sc, sh in par]
    oi, ol = FH.affine_nearest(dv(img, dev), dv(lab, dev), [mats[b % 5] for b in range(nb)])
    oi, ol = oi.cpu().numpy(), ol.cpu().numpy()
    for b in range(nb):
        wi, wl = _gather(maps[b % 5], img[b], lab[b])
        assert np.array_equal(oi[b], wi) and np.array_equal(ol[b], wl), b
    g = torch.Generator().manual_seed(4)
    disp = torch.randn(nb, 2, 4, 4, generator=g) * 5.0
    oi, ol = FH.elastic_warp(dv(img, dev), dv(lab, dev), disp.to(dev))
    oi, ol = oi.cpu().numpy(), ol.cpu().numpy()
    worst = 0.0
    for b in range(nb):
        _, wl = _gather(T.apply_elastic(idx, disp[b]), img[b], lab[b])
        assert np.array_equal(ol[b], wl), b
        worst = max(worst, err(oi[b], T.apply_elastic(torch.from_numpy(img[b]), disp[b]).numpy()))
    assert worst < ELASTIC_TOL


# =========================================================================== sample statistics, z-score
def _stats_ok(got, x, gray):
    want = A.sample_stats(x, gray)
    g = got.cpu().numpy().astype(np.float64)
    for b in range(x.shape[0]):
        ulp = float(np.spacing(np.float32(np.abs(x[b]).max())))
        assert abs(g[b, 0] - want[b, 0]) <= 4 * ulp, (b, g[b, 0], want[b, 0])
        if want[b, 1] == 0:
            assert g[b, 1] == 0
        else:
            assert abs(g[b, 1] / want[b, 1] - 1.0) <= STD_RTOL, (b, g[b, 1], want[b, 1])
    return want


@pytest.mark.parametrize("case", A.STATS_CASES, ids=lambda c: c[0])
def test_sample_stats(case):
    FH = _fh()
    dev = _dev()
    _, shape, gray = case
    x = A.stats_image(shape, 2)
    _stats_ok(FH.sample_stats(dv(x, dev), gray=gray), x, gray)


@pytest.mark.parametrize("case", A.HARD_STATS, ids=lambda c: c[0])
def test_hard_stats_zscore(case):
    """Low-contrast and raw-intensity images: sums of v and v^2 in fp32 lose the variance to cancellation (before the sums were taken
    about a pivot, measured on an MI355X: std off by 1.0e-5 / 2.3e-3 / 7.0e-6 relative, z-score by 4.9e-5 / 1.1e-2 / 3.3e-5; since then
    3.6e-8 / 2.7e-8 / 2.1e-8 and 2.2e-6 / 5.8e-6 / 2.8e-7).  The z-score is compared to the TRUE one
    (float64 statistics), so it also has to absorb the fp32 rounding of the mean the kernel hands on: ulp(mean) / (2 std) <= 1.5e-5."""
    FH = _fh()
    dev = _dev()
    _, mean, std = case
    x = A.hard_stats_image(mean, std)
    xd = dv(x, dev)
    ms = FH.sample_stats(xd)
    want = _stats_ok(ms, x, False)
    z = FH.elementwise(xd, FH.EW_ZSCORE, mean_std=ms)
    e = err(z, A.elementwise(x, A.EW_ZSCORE, mean_std=want))
    print(f"hard stats {case[0]}: std rel err {abs(ms[0, 1].item() / want[0, 1] - 1):.2e}, mean err {abs(ms[0, 0].item() - want[0, 0]):.2e}, max z err {e:.2e}")
    assert e < Z_TOL


def test_sample_stats_selective_rows():
    call, _p, _i64, _st = _abi()
    FH = _fh()
    dev = _dev()
    for c, gray in ((1, 0), (3, 1)):
        x = A.stats_image((5, c, 36, 52), 6)
        x[1] = np.nan  # a skipped sample is not read
        x[3] = np.nan
        xd = dv(x, dev)
        ap = [1, -1, 0, -1, 1]
        ws = torch.empty(FH.lib().mia_sample_stats_workspace(5), device=dev)
        ms = torch.full((5, 2), S, device=dev)
        apd = ints(dev, ap)
        call("mia_sample_stats_sel", _p(xd), 5, c, _i64(36 * 52), gray, _p(ws), _p(ms), _p(apd), _st())
        full = FH.sample_stats(xd, gray=bool(gray))
        assert torch.equal(ms[[0, 2, 4]], full[[0, 2, 4]]) and (ms[[1, 3]] == 0).all()
        _stats_ok(ms[[0, 2, 4]], x[[0, 2, 4]], bool(gray))


# =========================================================================== blur
def test_blur_mixed_kernel_sizes_and_flags():
    call, _p, _i64, _st = _abi()
    dev = _dev()
    for c in (1, 3):
        x = A.image((7, c, 36, 52), 11)
        ks, sg = [1, 3, 5, 7, 9, 5, 9], [0.3, 0.62, 1.0, 1.6, 1.9, 0.75, 2.3]
        ap = [1, 1, 1, 1, 1, 0, -1]
        xd = dv(x, dev)
        out = torch.full_like(xd, S)
        sgd, ksd, apd = flts(dev, sg), ints(dev, ks), ints(dev, ap)  # held across the launch
        call("mia_gaussian_blur", _p(xd), _p(out), 7, c, 36, 52, _p(sgd), _p(ksd), 9, _p(apd), _st())
        want = A.with_flags(A.blur(x, sg, ks), x, ap)
        assert err(out, want) < BLUR_TOL
        o = out.cpu().numpy()
        assert np.array_equal(o[5], x[5]) and (o[6] == S).all() and err(o[0], x[0]) < 2.0 ** -23  # k = 1: the image itself


@pytest.mark.parametrize("hw", [(5, 5), (5, 64)])
def test_blur_k9_on_the_smallest_image(hw):
    """k = 9 needs H, W > 4: on H = 5 every column reflects at both ends for every row."""
    FH = _fh()
    dev = _dev()
    x = A.image((2, 3) + hw, 12)
    sg, ks = [1.9, 2.4], [9, 9]
    assert err(FH.gaussian_blur(dv(x, dev), sg, ks), A.blur(x, sg, ks)) < BLUR_TOL


# =========================================================================== element-wise
def test_elementwise_in_place_equals_out_of_place():
    call, _p, _i64, _st = _abi()
    dev = _dev()
    x = A.image((4, 3, 36, 52), 13)
    x[0, 0, 0, :2] = (0.0, 1.0)
    ms = dv(np.array([[0.4, 0.2], [0.5, 0.3], [0.6, 0.25], [0.45, 0.15]], dtype=np.float32), dev)
    p0 = flts(dev, [0.7, 1.0, 1.37, 2.5])
    aux = dv((A.image((4, 3, 36, 52), 14).astype(np.float64) - 0.5).astype(np.float32), dev)
    ap = ints(dev, [1, 0, -1, 1])
    for op in range(4):
        for flags in (None, ap):
            xd = dv(x, dev)
            out = torch.full_like(xd, S)
            call("mia_elementwise", _p(xd), _p(out), _i64(3 * 36 * 52), 4, op, _p(p0), _p(ms), _p(aux), _p(flags), _st())
            inpl = torch.where(ap.view(4, 1, 1, 1) < 0, torch.full_like(xd, S), xd) if flags is not None else xd.clone()
            call("mia_elementwise", _p(inpl), _p(inpl), _i64(3 * 36 * 52), 4, op, _p(p0), _p(ms), _p(aux), _p(flags), _st())
            assert torch.equal(out, inpl), (op, flags is not None)  # bits
            want = A.elementwise(x, op, p0=p0.cpu().numpy(), mean_std=ms.cpu().numpy(), aux=aux.cpu().numpy())
            if flags is not None:
                want = A.with_flags(want, x, [1, 0, -1, 1])
                o = out.cpu().numpy()
                assert np.array_equal(o[1], x[1]) and (o[2] == S).all()
            tol = np.abs(want).max() * 2.0 ** -22 if op == A.EW_ZSCORE else EW_TOL  # z-score: one subtraction, one division
            assert err(out, want) < tol, op


def test_elementwise_gamma_and_contrast_edges():
    FH = _fh()
    dev = _dev()
    for c in (1, 3):
        x = A.image((1, c, 36, 52), 9)
        x[0, 0, 0, :4] = (0.0, 1.0, 0.0, 1.0)
        xd = dv(x, dev)
        for gm in (0.7, 1.0, 1.37, 1.5):
            out = FH.elementwise(xd, FH.EW_GAMMA, p0=[gm])
            assert err(out, A.elementwise(x, A.EW_GAMMA, p0=[gm])) < EW_TOL
            assert out[0, 0, 0, 0].item() == 0.0 and out[0, 0, 0, 1].item() == 1.0  # pow(0, g) = 0, pow(1, g) = 1, exactly
        ms = FH.sample_stats(xd, gray=(c == 3))
        _stats_ok(ms, x, c == 3)
        true_ms = A.sample_stats(x, c == 3)
        for f in (0.0, 0.8, 1.25, 2.5):
            out = FH.elementwise(xd, FH.EW_CONTRAST, p0=[f], mean_std=ms)
            assert err(out, A.elementwise(x, A.EW_CONTRAST, p0=[f], mean_std=true_ms)) < EW_TOL
        assert out.min().item() == 0.0 and out.max().item() == 1.0  # f = 2.5 clamps at both ends


def test_zscore_of_zeros_is_zero():
    FH = _fh()
    dev = _dev()
    xd = torch.zeros(2, 1, 36, 52, device=dev)
    ms = FH.sample_stats(xd)
    assert (ms == 0).all()
    z = FH.elementwise(xd, FH.EW_ZSCORE, mean_std=ms)
    assert (z == 0).all() and not torch.signbit(z).any()


# =========================================================================== noise
def _normals(dev, nb, per, seed, offset):
    """The kernel's normals, exactly: in = 0 and sigma = +-1/8 give clamp(+-z / 8, 0, 1) -- a power-of-two scaling, no rounding -- so the
    positive normals come out of the first launch and the negative ones out of the second (|z| < 6 < 8)."""
    FH = _fh()
    x = torch.zeros(nb, per, device=dev)
    pos = FH.noise_clip(x, [0.125] * nb, seed=seed, offset=offset)
    neg = FH.noise_clip(x, [-0.125] * nb, seed=seed, offset=offset)
    assert not ((pos > 0) & (neg > 0)).any() and pos.max().item() < 1.0 and neg.max().item() < 1.0
    return ((pos - neg) * 8.0).cpu().numpy().reshape(-1)


def test_noise_known_answer_quad0():
    """Seed 0, offset 0, quad 0: the Philox words are the Random123 known answer 6627e8d5 e169c58d bc57ac4c 9b00dbd8; the four normals
    follow from it by the definition (uniforms ((c >> 8) + 0.5) 2^-24, Box-Muller), written out here without _augment_ref's Philox."""
    dev = _dev()
    words = np.array([0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8], dtype=np.uint64)
    # one rounding to fp32 (scaling by 2^-24 commutes with it): the definition's fp32 sum rounds the same way
    u = (((words >> 8).astype(np.float64) + 0.5) / 16777216.0).astype(np.float32)
    assert np.array_equal(u, A.uniforms(words.astype(np.uint32)))
    a1, a3 = float(np.float32(6.2831853) * u[1]), float(np.float32(6.2831853) * u[3])  # fp32 products
    u = u.astype(np.float64)
    r0, r1 = np.sqrt(-2 * np.log(u[0])), np.sqrt(-2 * np.log(u[2]))
    want = np.array([r0 * np.cos(a1), r0 * np.sin(a1), r1 * np.cos(a3), r1 * np.sin(a3)])
    z = _normals(dev, 1, 4, 0, 0)
    assert np.abs(z - want).max() < NOISE_Z_TOL, (z, want)
    assert np.abs(A.noise_normals([0], 0, 0)[0] - want).max() < 1e-12


def test_noise_normals_measured():
    """Every normal of 33 x 512 x 512 elements (2.16 M quads: both trips of the loop) against the float64 restatement; prints the
    measured maximum that NOISE_Z_TOL is derived from."""
    dev = _dev()
    nb, per = 33, 512 * 512
    z = _normals(dev, nb, per, 0x1234ABCD5678, 9)
    ref = A.noise_z(nb * per, 0x1234ABCD5678, 9)
    e = float(np.abs(z - ref).max())
    print(f"noise: max |z_gpu - z_ref| = {e:.3e} over {z.size} normals (NOISE_Z_TOL = {NOISE_Z_TOL:.1e})")
    assert NOISE_Z_TOL <= 1e-5
    assert e < NOISE_Z_TOL
    assert abs(z.mean()) < 2e-3 and abs(z.std() - 1.0) < 2e-3


@pytest.mark.parametrize("case", A.NOISE_CASES, ids=lambda c: c[0])
def test_noise_cases(case):
    call, _p, _i64, _st = _abi()
    dev = _dev()
    _, per, nb, sg, seed, offset, ap = case
    x = A.image((nb, per), 15)
    xd = dv(x, dev)
    out = torch.full_like(xd, S)
    sgd, apd = flts(dev, sg), (ints(dev, ap) if ap else None)  # held across the launch
    call("mia_noise_clip", _p(xd), _p(out), _i64(per), nb, _p(sgd), ctypes.c_uint64(seed), ctypes.c_uint64(offset), _p(apd), _st())
    want = A.noise_clip(x, sg, seed, offset)
    if ap:
        want = A.with_flags(want, x, ap)
    assert err(out, want) < max(sg) * NOISE_Z_TOL + 2.0 ** -23
    if ap:
        o = out.cpu().numpy()
        for b, a in enumerate(ap):
            assert a > 0 or np.array_equal(o[b], x[b] if a == 0 else np.full_like(x[b], S))
    assert np.abs(want - x)[[b for b in range(nb) if not ap or ap[b] > 0]].max() > 0.01  # and the noise is there


# =========================================================================== resize
def _img36():
    return A.image((2, 3, 36, 52), 3)


@pytest.mark.parametrize("size", A.BILINEAR_SIZES, ids=str)
def test_resize_bilinear(size):
    FH = _fh()
    dev = _dev()
    x = _img36()
    out = FH.resize_bilinear(dv(x, dev), *size)
    assert err(out, A.resize_bilinear(x, *size)) < RESIZE_TOL
    if size == (36, 52):
        assert same(out, x)


@pytest.mark.parametrize("size", A.AA_SIZES, ids=str)
def test_resize_antialiased(size):
    """(17, 80), (72, 23): one axis shrinks, the other grows; (36, 23): one stays; (5, 7): more than 7 x down (15 to 16 taps);
    (1, 1): the mean-like filter over the whole image."""
    FH = _fh()
    dev = _dev()
    x = _img36()
    assert err(FH.resize_bilinear(dv(x, dev), size[0], size[1], antialias=True), A.resize_aa(x, *size)) < RESIZE_TOL


@pytest.mark.parametrize("case", A.NEAREST_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("dtype", [np.float32, np.int32, np.int64], ids=["f32", "i32", "i64"])
def test_resize_nearest(case, dtype):
    """6 x 4 -> 74 x 82: output row 37 reads source row 2 and output column 41 source column 1 in fp32 (3 and 2 in exact arithmetic)."""
    FH = _fh()
    dev = _dev()
    _, (h, w), (oh, ow) = case
    x = (np.arange(2 * 3 * h * w).reshape(2, 3, h, w) * 37 % 1009).astype(dtype)
    out = FH.resize_nearest(dv(x, dev), oh, ow)
    assert out.dtype == dv(x, dev).dtype and same(out, A.resize_nearest(x, oh, ow))


@pytest.mark.parametrize("case", A.LOWRES_CASES, ids=lambda c: c[0])
def test_lowres(case):
    call, _p, _i64, _st = _abi()
    dev = _dev()
    _, (h, w), low, ap = case
    nb = len(low)
    x = A.image((nb, 2, h, w), 8)
    xd = dv(x, dev)
    out = torch.full_like(xd, S)
    lw = torch.tensor(low, dtype=torch.int32, device=dev)
    apd = ints(dev, ap)
    call("mia_resize_bilinear", _p(xd), _p(out), nb, 2, h, w, h, w, _p(lw), _p(apd), _st())
    assert err(out, A.with_flags(A.lowres(x, low), x, ap)) < LOWRES_TOL
    o = out.cpu().numpy()
    for b, a in enumerate(ap):
        assert a > 0 or np.array_equal(o[b], x[b] if a == 0 else np.full_like(x[b], S))


@pytest.mark.parametrize("case", A.BWD_CASES, ids=str)
def test_resize_bilinear_bwd(case):
    call, _p, _i64, _st = _abi()
    dev = _dev()
    (h, w), (oh, ow) = case
    g = np.random.default_rng(21)
    dout = (g.integers(-512, 513, size=(2, 3, oh, ow)) / 256.0).astype(np.float32)
    din = torch.zeros(2, 3, h, w, device=dev)
    dd = dv(dout, dev)
    call("mia_resize_bilinear_bwd", _p(dd), _p(din), 2, 3, h, w, oh, ow, _st())
    want, mag, cnt = A.resize_bilinear_adjoint(dout, h, w)
    got = din.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    bound = (cnt[None, None] + 3) * 2.0 ** -24 * mag
    bad = np.abs(got - want) > bound
    assert not bad.any(), (int(bad.sum()), float((np.abs(got - want) / np.maximum(bound, 1e-300)).max()))
    if (h, w) == (oh, ow):
        assert np.array_equal(got, dout)


# =========================================================================== rot90 / crop
@pytest.mark.parametrize("dtype", [np.float32, np.int64], ids=["4B", "8B"])
def test_rot90_flip_all(dtype):
    FH = _fh()
    dev = _dev()
    x = np.arange(2 * 3 * 5 * 8).reshape(2, 3, 5, 8).astype(dtype)
    xd = dv(x, dev)
    for k in range(4):
        for fh in (False, True):
            for fw in (False, True):
                assert same(FH.rot90_flip(xd, k, fh, fw), A.rot90_flip(x, k, fh, fw)), (k, fh, fw)


@pytest.mark.parametrize("dtype", [np.float32, np.int64], ids=["4B", "8B"])
def test_crop_windows(dtype):
    FH = _fh()
    dev = _dev()
    h, w, oh, ow = 9, 11, 5, 7
    x = np.arange(3 * 2 * h * w).reshape(3, 2, h, w).astype(dtype)
    xd = dv(x, dev)
    top, left = [0, h - oh, 2], [0, w - ow, 1]
    assert same(FH.crop(xd, top, left, oh, ow), A.crop(x, top, left, oh, ow))
    assert same(FH.crop(xd, [0] * 3, [0] * 3, h, w), x)  # the full-size window
