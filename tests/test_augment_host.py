"""CPU checks of the float64 restatement in tests/_augment_ref.py: against torch on the CPU (F.interpolate in its four modes and its
autograd, F.conv2d on a reflect-padded image, torch.rot90 / flip, torch.std), against oracle/transforms_ref.py where it has the
operation, the Random123 known answers of Philox4x32-10, and the properties the shared case tables claim.  None of it needs a GPU.

torch's float64 kernels do the resize INDEX arithmetic in float64 too, the definition (and the restatement) in fp32: float64 torch is
compared to 1e-12 where the scale is a power of two (both exact) and to the size of that index rounding elsewhere; fp32 torch is compared
at fp32 accumulation error."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _augment_ref as A
from oracle import transforms_ref as T

RTOL = 1e-12
t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))


def err(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max())


# --------------------------------------------------------------------------- resize
@pytest.mark.parametrize("size", A.BILINEAR_SIZES + [(9, 13), (144, 208)])
def test_bilinear_matches_interpolate(size):
    x = A.image((2, 3, 36, 52), 3)
    got = A.resize_bilinear(x, *size)
    assert err(got, F.interpolate(torch.from_numpy(x), size=size, mode="bilinear", align_corners=False).numpy()) < 2e-6
    d = err(got, F.interpolate(t64(x), size=size, mode="bilinear", align_corners=False).numpy())
    dyadic = all(np.log2(i / o) == int(np.log2(i / o)) for i, o in zip((36, 52), size))
    assert d < (RTOL if dyadic else 1e-5), d


@pytest.mark.parametrize("case", A.BWD_CASES, ids=str)
def test_bilinear_adjoint(case):
    (h, w), (oh, ow) = case
    g = np.random.default_rng(5)
    x, dout = g.standard_normal((2, 3, h, w)), g.standard_normal((2, 3, oh, ow))
    din, mag, cnt = A.resize_bilinear_adjoint(dout, h, w)
    lhs, rhs = (dout * A.resize_bilinear(x, oh, ow)).sum(), (din * x).sum()
    assert abs(lhs - rhs) < RTOL * max(1.0, abs(lhs)), (lhs, rhs)
    xt = t64(x).requires_grad_(True)
    F.interpolate(xt, size=(oh, ow), mode="bilinear", align_corners=False).backward(t64(dout))
    dyadic = all(np.log2(i / o) == int(np.log2(i / o)) for i, o in zip((h, w), (oh, ow)))
    assert err(din, xt.grad.numpy()) < (1e-11 if dyadic else 1e-5)
    assert (mag >= np.abs(din) - 1e-12).all() and cnt.sum() >= oh * ow and cnt.min() >= 0
    if (h, w) == (oh, ow):
        assert err(din, dout) == 0.0 and (cnt == 1).all()
    if (h, w, oh, ow) == (1, 6, 4, 6):
        assert (cnt == 4).all()  # h = 1: y0 == y1, each output pixel reaches one input pixel once


@pytest.mark.parametrize("size", A.AA_SIZES + [(18, 26), (36, 26)])
def test_antialiased_matches_interpolate(size):
    x = A.image((2, 3, 36, 52), 3)
    got = A.resize_aa(x, *size)
    want = F.interpolate(torch.from_numpy(x), size=size, mode="bilinear", align_corners=False, antialias=True).numpy()
    assert err(got, want) < 3e-6
    if size == (18, 26):  # scale 2: index arithmetic exact on both sides
        assert err(got, F.interpolate(t64(x), size=size, mode="bilinear", align_corners=False, antialias=True).numpy()) < RTOL


@pytest.mark.parametrize("case", A.NEAREST_CASES, ids=lambda c: c[0])
def test_nearest_matches_interpolate(case):
    _, (h, w), (oh, ow) = case
    x = np.arange(2 * h * w, dtype=np.float32).reshape(2, 1, h, w)
    assert np.array_equal(A.resize_nearest(x, oh, ow), F.interpolate(torch.from_numpy(x), size=(oh, ow), mode="nearest").numpy())
    lab = np.arange(h * w, dtype=np.int64).reshape(1, h, w)
    assert np.array_equal(A.resize_nearest(lab, oh, ow), T.apply_resize_label(torch.from_numpy(lab), (oh, ow)).numpy())


@pytest.mark.parametrize("case", A.LOWRES_CASES, ids=lambda c: c[0])
def test_lowres_matches_interpolate(case):
    _, (h, w), low, _ = case
    x = A.image((len(low), 1, h, w), 8)
    got = A.lowres(x, low)
    for b, lo in enumerate(low):
        down = F.interpolate(torch.from_numpy(x[b:b + 1]), lo, mode="nearest-exact")
        idx = np.arange(h * w, dtype=np.float32).reshape(1, 1, h, w)
        want_idx = F.interpolate(torch.from_numpy(idx), lo, mode="nearest-exact").numpy()[0, 0]
        mine = idx[0, 0][A.nearest_index(h, lo[0], exact=True), :][:, A.nearest_index(w, lo[1], exact=True)]
        assert np.array_equal(mine, want_idx)
        assert err(got[b], F.interpolate(down, (h, w), mode="bilinear")[0].numpy()) < 2e-6
    assert err(A.lowres(x[:1], [(30, 32)]), T.apply_lowres(torch.from_numpy(x[0]), [0.5, 0.5]).numpy()[None]) < 2e-6


# --------------------------------------------------------------------------- blur, statistics, element-wise
@pytest.mark.parametrize("k,sigma,hw", [(1, 0.3, (5, 5)), (3, 0.62, (36, 52)), (5, 1.0, (36, 52)), (7, 1.6, (20, 24)), (9, 1.9, (5, 5)), (9, 2.1, (5, 64))])
def test_blur_matches_conv2d(k, sigma, hw):
    x = A.image((2, 3) + hw, 7)
    got = A.blur(x, [sigma, sigma], [k, k])
    s = float(np.float32(sigma))
    j = torch.arange(k, dtype=torch.float64) - (k - 1) * 0.5
    k1 = torch.exp(-0.5 * (j / s) ** 2)
    k1 = k1 / k1.sum()
    kern = (k1[:, None] * k1[None, :]).expand(3, 1, k, k)
    want = F.conv2d(F.pad(t64(x), [k // 2] * 4, mode="reflect"), kern, groups=3).numpy()
    assert err(got, want) < RTOL
    assert err(got[0], T.apply_gaussian_blur(torch.from_numpy(x[0]), k, s).numpy()) < 2e-6
    if k == 1:
        assert err(got, x) < RTOL


@pytest.mark.parametrize("case", A.STATS_CASES, ids=lambda c: c[0])
def test_sample_stats_matches_torch(case):
    _, shape, gray = case
    x = A.stats_image(shape, 2)
    got = A.sample_stats(x, gray)
    for b in range(shape[0]):
        v = t64(x[b])
        if gray:
            v = sum(float(np.float32(c)) * v[i] for i, c in enumerate((0.2989, 0.587, 0.114)))
        assert abs(got[b, 0] - v.mean().item()) < RTOL
        assert abs(got[b, 1] - (v.std().item() if v.numel() > 1 else 0.0)) < RTOL
    if shape[-2:] == (1, 1):
        assert (got[:, 1] == 0).all()


@pytest.mark.parametrize("case", A.HARD_STATS, ids=lambda c: c[0])
def test_hard_stats_images(case):
    _, mean, std = case
    x = A.hard_stats_image(mean, std)
    ms = A.sample_stats(x)
    assert abs(ms[0, 0] - mean) < 0.02 * std and abs(ms[0, 1] / std - 1.0) < 0.02
    assert abs(ms[0, 1] - t64(x).std().item()) < RTOL * mean
    z = A.elementwise(x, A.EW_ZSCORE, mean_std=ms)
    xt = t64(x)
    assert err(z, ((xt - xt.mean()) / xt.std().clip(1e-8)).numpy()) < 1e-9  # normalization.py:17-21 in float64
    # an fp32 mean is off by up to half an ulp: that alone moves z by ulp(mean) / (2 std), inside the 2e-5 the GPU test allows
    assert np.spacing(np.float32(mean)) / (2 * std) < 1.6e-5


def test_elementwise_matches_oracle():
    for c in (1, 3):
        x = A.image((1, c, 36, 52), 9)
        x[0, 0, 0, :4] = (0.0, 1.0, 0.0, 1.0)
        ms = A.sample_stats(x, gray=(c == 3)).astype(np.float32)
        for f in (0.0, 0.8, 1.0, 1.25, 2.5):
            assert err(A.elementwise(x, A.EW_CONTRAST, p0=[f], mean_std=ms)[0], T.apply_contrast(torch.from_numpy(x[0]), f).numpy()) < 2e-6
        out = A.elementwise(x, A.EW_CONTRAST, p0=[2.5], mean_std=ms)
        assert out.min() == 0.0 and out.max() == 1.0  # clamps at both ends
        for gm in (0.7, 1.0, 1.37):
            got = A.elementwise(x, A.EW_GAMMA, p0=[gm])
            assert err(got[0], T.apply_gamma(torch.from_numpy(x[0]), gm).numpy()) < 2e-6
            assert got[0, 0, 0, 0] == 0.0 and got[0, 0, 0, 1] == 1.0
        z = A.elementwise(x, A.EW_ZSCORE, mean_std=A.sample_stats(x).astype(np.float32))
        assert err(z[0], T.apply_zscore(torch.from_numpy(x[0])).numpy()) < 2e-5
        nz = np.random.default_rng(1).standard_normal(x.shape).astype(np.float32) * 0.3
        assert err(A.elementwise(x, A.EW_NOISE, aux=nz)[0], T.apply_noise(torch.from_numpy(x[0]), torch.from_numpy(nz[0])).numpy()) < 1e-7
    zero = np.zeros((1, 1, 4, 4), dtype=np.float32)
    assert (A.elementwise(zero, A.EW_ZSCORE, mean_std=A.sample_stats(zero).astype(np.float32)) == 0).all()


# --------------------------------------------------------------------------- rot90 / crop
@pytest.mark.parametrize("dtype", [np.float32, np.int64])
def test_rot90_flip_matches_torch(dtype):
    x = np.arange(2 * 3 * 5 * 8).reshape(2, 3, 5, 8).astype(dtype)
    for k in range(4):
        for fh in (False, True):
            for fw in (False, True):
                want = torch.rot90(torch.from_numpy(x), k, (-2, -1))
                want = torch.flip(want, [d for d, f in ((-2, fh), (-1, fw)) if f]) if (fh or fw) else want
                assert np.array_equal(A.rot90_flip(x, k, fh, fw), want.numpy()), (k, fh, fw)


def test_crop_matches_slicing():
    x = np.arange(3 * 2 * 9 * 11, dtype=np.float32).reshape(3, 2, 9, 11)
    got = A.crop(x, [0, 4, 2], [0, 4, 1], 5, 7)
    for b, (i, j) in enumerate(((0, 0), (4, 4), (2, 1))):
        assert np.array_equal(got[b], T.apply_crop(torch.from_numpy(x[b]), i, j, 5, 7).numpy())
    assert np.array_equal(A.crop(x, [0] * 3, [0] * 3, 9, 11), x)


# --------------------------------------------------------------------------- Philox and the noise
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert tuple(int(v) for v in A.philox4x32_10(np.array(ctr, dtype=np.uint32), key)) == want
    batch = A.philox4x32_10(np.array([ctr, (1, 0, 0, 0)], dtype=np.uint32), key)  # vectorised over counters
    assert tuple(int(v) for v in batch[0]) == want and tuple(int(v) for v in batch[1]) != want


def test_uniforms_and_first_quad():
    u = A.uniforms(np.array([0, 0xff, 0x100, 0xffffffff, 0x80000000], dtype=np.uint32))
    assert u.dtype == np.float32
    assert u[0] == u[1] == np.float32(2.0 ** -25) and u[2] == np.float32(1.5 * 2.0 ** -24)
    assert u[3] == np.float32(1.0)  # (2^24 - 1) + 0.5 rounds to 2^24 in fp32: the definition's fp32 arithmetic, kept
    assert u[4] == np.float32(0.5)  # 2^23 + 0.5 rounds to even
    # seed 0, offset 0, quad 0 = the first known answer
    w = np.array(KAT[0][2], dtype=np.uint32)
    uu = A.uniforms(w).astype(np.float64)
    z = A.noise_normals([0], 0, 0)[0]
    two_pi = float(np.float32(6.2831853))
    want = [np.sqrt(-2 * np.log(uu[0])) * np.cos(two_pi * uu[1]), np.sqrt(-2 * np.log(uu[0])) * np.sin(two_pi * uu[1]),
            np.sqrt(-2 * np.log(uu[2])) * np.cos(two_pi * uu[3]), np.sqrt(-2 * np.log(uu[2])) * np.sin(two_pi * uu[3])]
    assert err(z, want) < 2e-6  # the fp32 rounding of the angle, times |r| < 6
    assert np.abs(z).max() < 6.0


def test_noise_statistics_and_layout():
    z = A.noise_z(1 << 16, 1234, 1)
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02 and abs(np.mean(z[0::4] * z[1::4])) < 0.02
    assert not np.array_equal(z[:64], A.noise_z(64, 1234, 2)) and not np.array_equal(z[:64], A.noise_z(64, 1235, 1))
    assert np.array_equal(z[:61], A.noise_z(61, 1234, 1))  # element i depends on i alone
    hi = A.noise_z(8, 1234, (1 << 32) + 1)
    assert not np.array_equal(hi, z[:8])  # the high offset word is part of the counter
    x = np.full((2, 5), 0.5, dtype=np.float32)
    out = A.noise_clip(x, [0.0, 10.0], 3, 0)
    assert (out[0] == 0.5).all() and set(np.unique(out[1])) <= {0.0, 1.0}


# --------------------------------------------------------------------------- the case tables
def test_case_tables_hold_what_they_claim():
    ids = [c[0] for c in A.NEAREST_CASES] + [c[0] for c in A.LOWRES_CASES] + [c[0] for c in A.STATS_CASES] + [c[0] for c in A.HARD_STATS] + \
          [c[0] for c in A.NOISE_CASES]
    assert len(set(ids)) == len(ids)
    assert len(set(map(str, A.BWD_CASES))) == len(A.BWD_CASES) and len(set(A.BILINEAR_SIZES)) == 5 and len(set(A.AA_SIZES)) == 5
    # an index where fp32 and exact nearest arithmetic differ, and torch sides with fp32
    assert A.nearest_disagreements(6, 74).tolist() == [37] and A.nearest_index(6, 74)[37] == 2 and A.nearest_index(6, 74, arithmetic=np.float64)[37] == 3
    assert A.nearest_disagreements(4, 82).tolist() == [41] and A.nearest_index(4, 82)[41] == 1 and A.nearest_index(4, 82, arithmetic=np.float64)[41] == 2
    assert any(c[1] == (6, 4) and c[2] == (74, 82) for c in A.NEAREST_CASES)
    for _, (h, w), low, flags in A.LOWRES_CASES:
        live = [lo for lo, f in zip(low, flags) if f > 0]
        assert any(len(A.nearest_disagreements(h, lh, exact=True)) for lh, _ in live)
        assert any(len(A.nearest_disagreements(w, lw, exact=True)) for _, lw in live)
        assert {1, 0, -1} <= set(flags)
    # noise: a quad that spans two samples with different sigmas; a total that is no multiple of 4; mixed flags; high words
    by = {c[0]: c for c in A.NOISE_CASES}
    _, per, nb, sg, _, _, _ = by["quad_spans_two"]
    assert per % 4 != 0 and (per // 4 * 4) // per == 0 and (per // 4 * 4 + 3) // per == 1 and sg[0] != sg[1]
    assert (by["total_not_x4"][1] * by["total_not_x4"][2]) % 4 != 0
    assert {1, 0, -1} <= set(by["flags"][6])
    assert by["high_words"][4] >> 32 and by["high_words"][5] >> 32
    # bilinear backward: h == 1, w == 1, identity, up and down
    assert any(c[0][0] == 1 for c in A.BWD_CASES) and any(c[0][1] == 1 for c in A.BWD_CASES) and any(c[0] == c[1] for c in A.BWD_CASES)
    # statistics: n = 1, n below the 64 slabs, a luma case
    ns = {c[0]: int(np.prod(c[1][1:])) for c in A.STATS_CASES}
    assert ns["n1"] == 1 and ns["n35"] == 35 < 64 and ns["n1961"] == 1961 and any(c[2] and c[1][1] == 3 for c in A.STATS_CASES)
    # batch_of: no two samples agree
    bt = A.batch_of(A.image((1, 8, 8), 0), 9)
    assert all(not np.array_equal(bt[i], bt[j]) for i in range(9) for j in range(i))
    assert 9 * 512 * 512 > A.GRID_CAP and 33 * 512 * 512 // 4 > A.GRID_CAP
