"""Boundary loss on the GPU (csrc/boundary.hip, losses/boundary_loss.py) against the float64 restatement of
tests/_boundary_ref.py: signed distance maps, the fused softmax x phi loss and its gradient, and a TrainEngine run.

Tolerances.  Unit spacing: every test shape has H^2 + W^2 < 2^24, so squared distances are exact integers in fp32 and a correctly
rounded square root of an exact operand is the fp32 rounding of the true root: |phi - float32(ref)| <= 1 ulp of float32(ref) (0
where ref is 0).  Spacing (1.3, 0.4): |phi - ref| <= 1e-6 * max(1, d), d the unsigned distance (the project's HD tolerance for the
same arithmetic; max(1, .) covers the cancellation in d - 1).  Loss: each of the handful of fp32 roundings contributes at most
2^-24 relative to the magnitude of what it rounds; 32 * 2^-24 ~ 2e-6 is allowed:
    value     |L - ref| <= 2e-6 * (1/N) sum |s phi|
    gradient  |g - ref| <= 2e-6 * s_j (|w_j| + sum_k |w_k| s_k) + 1e-12    per element
Each test prints the largest observed ratio to its bound (pytest -s shows them; tools/microbench_boundary.py records them)."""
import functools

import numpy as np
import pytest
import torch

import _boundary_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 1, 7), (2, 9, 1), (4, 37, 61), (2, 336, 544)]
LOSS_SHAPES = [(1, 1, 1), (4, 37, 61), (2, 336, 544)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _label_map(shape, k1, rng):
    """One image in 0..k1-1: per class an ellipse, thresholded smoothed noise, a single pixel, or nothing."""
    from scipy import ndimage
    grids = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
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
    return lab


@functools.lru_cache(maxsize=None)
def _batch(shape, k1):
    """[n,H,W] int64: image 0 random with one isolated pixel of the last class, 1 filled by class 1, 2 without class 1, 3 empty."""
    n, hw = shape[0], shape[1:]
    rng = np.random.default_rng(1000 * k1 + hw[0] + hw[1])
    labs = []
    for i in range(n):
        lab = _label_map(hw, k1, rng)
        if i % 4 == 0:
            lab[hw[0] // 2, hw[1] // 3] = k1 - 1
        if i % 4 == 1:
            lab[...] = 1
        if i % 4 == 2:
            lab[lab == 1] = 0
        if i % 4 == 3:
            lab[...] = 0
        labs.append(lab)
    out = np.stack(labs)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ref(shape, k1, classes, spacing):
    lab = _batch(shape, k1)
    return R.phi_labels(lab, k1, classes, spacing), R.phi_labels(lab, k1, classes, spacing, unsigned=True)


def _t(a):
    return torch.from_numpy(np.array(a))  # a writable copy: the cached batches are read-only


def _phi(lab, k1, classes, spacing, dtype=torch.int64):
    from losses.boundary_loss import signed_distance_map
    t = _t(lab).to(_dev()).to(dtype)
    return signed_distance_map(t, k1 - 1, classes, spacing)


def _check_phi(got, ref, d, spacing):
    got = got.double().cpu().numpy()
    assert got.shape == ref.shape
    np.testing.assert_array_equal(got[ref == 0], 0)  # empty / full classes and inner border pixels: zeros in the reference's positions
    if spacing is None:
        ref32 = ref.astype(np.float32)
        tol = np.where(ref32 == 0, 0.0, np.spacing(np.abs(ref32)).astype(np.float64))
        err = np.abs(got - ref32.astype(np.float64))
        print(f"unit spacing: bit-equal={bool((err == 0).all())} max err/ulp={float((err / np.maximum(tol, 1e-300)).max()):.3g}")
    else:
        tol = 1e-6 * np.maximum(1.0, d)
        err = np.abs(got - ref)
        print(f"spacing {spacing}: max err/bound={float((err / tol).max()):.3g}")
    assert (err <= tol).all(), float((err - tol).max())


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("k1", [2, 3, 8])
@pytest.mark.parametrize("spacing", [None, (1.3, 0.4)])
def test_distance_map_matches_restatement(shape, k1, spacing):
    lab = _batch(shape, k1)
    ref, d = _ref(shape, k1, None, spacing)
    got = _phi(lab, k1, None, spacing)
    assert got.dtype == torch.float32 and tuple(got.shape) == (shape[0], k1 - 1, shape[1], shape[2])
    _check_phi(got, ref, d, spacing)
    assert torch.equal(_phi(lab, k1, None, spacing, torch.uint8), got)  # byte labels: the same bits
    assert torch.equal(_phi(lab, k1, None, spacing), got)               # and run to run
    for b in range(shape[0]):  # the no-boundary rule
        for ci, c in enumerate(range(1, k1)):
            n = int((lab[b] == c).sum())
            if n == 0 or n == lab[b].size:
                assert not got[b, ci].any()


@pytest.mark.parametrize("shape", [(2, 1, 7), (4, 37, 61)])
@pytest.mark.parametrize("k1,classes", [(2, (0, 1)), (3, (0, 2)), (8, (0, 3, 7))])
def test_distance_map_class_subset_with_background(shape, k1, classes):
    for spacing in (None, (1.3, 0.4)):
        ref, d = _ref(shape, k1, classes, spacing)
        got = _phi(_batch(shape, k1), k1, classes, spacing)
        assert got.shape[1] == len(classes)
        _check_phi(got, ref, d, spacing)


def test_foreign_label_is_member_of_no_class():
    lab = _batch((4, 37, 61), 3).copy()
    lab[0, 5:9, 5:9] = 9
    lab[2, 0, 0] = -1
    got = _phi(lab, 3, (0, 1, 2), None)
    _check_phi(got, R.phi_labels(lab, 3, (0, 1, 2)), None, None)


def test_images_do_not_see_each_other():
    lab = _batch((4, 37, 61), 3)
    perm = [2, 0, 3, 1]
    got = _phi(lab, 3, None, (1.3, 0.4))
    assert torch.equal(_phi(lab[perm], 3, None, (1.3, 0.4)), got[perm])
    assert torch.equal(_phi(lab[1:2], 3, None, (1.3, 0.4)), got[1:2])


def test_wrapper_shapes_and_limits():
    import mia_hip
    from losses.boundary_loss import signed_distance_map
    dev = _dev()
    y = _t(_batch((4, 37, 61), 3)).to(dev)
    assert torch.equal(signed_distance_map(y[:, None], 2), signed_distance_map(y, 2))
    with pytest.raises(mia_hip.MiaError):
        signed_distance_map(torch.zeros(1, 1, 4097, dtype=torch.int64, device=dev), 2)
    with pytest.raises(mia_hip.MiaError):
        signed_distance_map(y, 8)  # 9 classes


# ---------------------------------------------------------------- loss
def _logits(shape, k1, layout, seed=0):
    g = torch.Generator().manual_seed(seed + shape[1])
    z = torch.randn(shape[0], k1, shape[1], shape[2], generator=g) * 3
    z = z.to(_dev())
    if layout == "channels_last":
        z = z.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)  # the head's layout: logical NCHW over NHWC memory
    return z.requires_grad_(True)


def _check_loss(z, phi, classes, loss, grad, g=1.0, what=""):
    rg, mag, rv, rabs = R.grad_formula(z.detach().cpu(), phi.cpu(), classes, g)
    ev = abs(loss - g * float(rv)) / (2e-6 * abs(g) * float(rabs)) if float(rabs) > 0 else float(loss != 0)
    eg = float(((grad.double().cpu() - rg).abs() / (2e-6 * abs(g) * mag + 1e-12)).max())
    print(f"{what}: value err/bound={ev:.3g} gradient max err/bound={eg:.3g}")
    assert ev <= 1.0 and eg <= 1.0


@pytest.mark.parametrize("shape", LOSS_SHAPES)
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("k1,classes", [(3, None), (8, (0, 3, 7))])
def test_loss_and_gradient_match_restatement(shape, layout, k1, classes):
    from losses.boundary_loss import BoundaryLoss
    lab = _t(_batch(shape, k1)).to(_dev())
    z = _logits(shape, k1, layout)
    fn = BoundaryLoss(k1 - 1, classes)
    phi = _phi(_batch(shape, k1), k1, classes, None)
    loss = fn(z, lab)
    loss.backward()
    assert loss.ndim == 0 and z.grad.stride() == z.stride()
    assert torch.equal(fn.last_value, loss.detach())
    _check_loss(z, phi, fn.classes, loss.item(), z.grad, what=f"{shape} {layout} k1={k1}")
    # a precomputed map, byte labels, [B,1,H,W] labels and a second run: the same bits
    g0 = z.grad.clone()
    for y, dist in ((lab, phi), (lab.to(torch.uint8), None), (lab[:, None], None), (lab, None)):
        z.grad = None
        l2 = fn(z, y, dist)
        l2.backward()
        assert torch.equal(l2, loss) and torch.equal(z.grad, g0)


def test_grad_out_and_device_weight_scale_value_and_gradient():
    from losses.boundary_loss import BoundaryLoss
    shape, k1 = (4, 37, 61), 3
    dev = _dev()
    lab = _t(_batch(shape, k1)).to(dev)
    z = _logits(shape, k1, "channels_last", seed=1)
    fn = BoundaryLoss(2, spacing=(1.3, 0.4))
    phi = _phi(_batch(shape, k1), k1, None, (1.3, 0.4))
    (fn(z, lab) * -2.5).backward()
    _check_loss(z, phi, (1, 2), -2.5 * fn.last_value.item(), z.grad, g=-2.5, what="grad_out -2.5")
    w = torch.tensor([0.375], device=dev)
    z.grad = None
    lw = fn(z, lab, weight=w)
    lw.backward()
    _check_loss(z, phi, (1, 2), lw.item(), z.grad, g=0.375, what="weight 0.375")
    plain = fn.last_value.item()
    assert lw.item() == pytest.approx(0.375 * plain, rel=1e-6)
    w.fill_(0.0)  # the kernels read the weight when they run
    z.grad = None
    l0 = fn(z, lab, weight=w)
    l0.backward()
    assert l0.item() == 0 and not z.grad.any() and fn.last_value.item() == plain


def test_out_of_range_label_gives_nan_and_check_labels_raises():
    import mia_hip
    from losses.boundary_loss import BoundaryLoss
    from mia_hip import ops
    shape, k1 = (4, 37, 61), 3
    ops.check_labels()
    lab = _t(_batch(shape, k1)).to(_dev()).clone()
    z = _logits(shape, k1, "nchw")
    fn = BoundaryLoss(2)
    for bad, dtype in ((3, torch.int64), (-1, torch.int64), (255, torch.uint8)):
        y = lab.clone()
        y[1, 7, 9] = bad
        z.grad = None
        loss = fn(z, y.to(dtype))
        loss.backward()
        assert torch.isnan(loss) and torch.isnan(z.grad).all()
        clean = fn(z, lab)  # a clean forward in between does not erase the verdict
        assert torch.isfinite(clean)
        with pytest.raises(mia_hip.MiaError):
            ops.check_labels()
        ops.check_labels()


def test_graph_capture_replays_to_the_eager_bits():
    from losses.boundary_loss import BoundaryLoss
    shape, k1 = (4, 37, 61), 3
    dev = _dev()
    labs = _t(_batch(shape, k1)).to(dev)
    fn = BoundaryLoss(2)
    w = torch.tensor([0.25], device=dev)
    z0, z1 = _logits(shape, k1, "channels_last", seed=2), _logits(shape, k1, "channels_last", seed=3)

    def eager(z, y):
        z = z.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
        loss = fn(z, y, weight=w)
        loss.backward()
        return loss.detach().clone(), z.grad.clone()

    want0 = eager(z0, labs)  # also the warm-up: flags and allocator
    zs = z0.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    ys = labs.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = fn(zs, ys, weight=w)
        loss.backward()
    graph.replay()
    assert torch.equal(loss, want0[0]) and torch.equal(zs.grad, want0[1])
    with torch.no_grad():  # new logits, new labels (the map is recomputed inside the graph), new weight
        zs.copy_(z1)
        ys.copy_(labs.flip(0))
    w.fill_(0.75)
    graph.replay()
    want1 = eager(z1, labs.flip(0))
    assert torch.equal(loss, want1[0]) and torch.equal(zs.grad, want1[1])
    assert not torch.equal(want1[0], want0[0])


# ---------------------------------------------------------------- engine
def test_engine_graph_steps_equal_eager_and_follow_set_alpha():
    from losses.boundary_loss import BoundaryLoss, RegionAndBoundaryLoss
    from losses.compound_losses import DiceAndCELoss
    from models.unet import UNet
    from training.engine import TrainEngine
    dev = _dev()
    g = torch.Generator().manual_seed(4)
    batches = [(torch.rand(2, 1, 32, 32, generator=g), (torch.rand(2, 32, 32, generator=g) * 3).long().clamp_(0, 2)) for _ in range(7)]
    for _, y in batches:
        y[:, 8:20, 6:18] = 1
        y[:, 22:28, 20:30] = 2

    def run(graph, alphas):
        """Warm-up steps (the engine's own, eager), three steps at alpha 0.01, one at alphas[-1]."""
        torch.manual_seed(7)
        m = UNet(2, 1, 3, [4, 8, 16], normalization="instance", dropout_prob=None).to(dev)
        loss_fn = RegionAndBoundaryLoss(DiceAndCELoss(dice_kwargs=dict(num_classes=2, do_bg=True)), BoundaryLoss(2), alpha=0.01)
        eng = TrainEngine(m, loss_fn, "adam", start_lr=1e-2, num_iters=20, lr_warmup_iter=2, graph=graph)
        losses = []
        for i, (x, y) in enumerate(batches):
            if i == len(batches) - 1:
                loss_fn.set_alpha(alphas[-1])
            losses.append(eng.train_step({"image": x.to(dev), "label": y.to(dev)}))
        torch.cuda.synchronize()
        if graph:
            assert eng.graph_mode and len(eng._graphs) == 1, "the step was not captured"
        return torch.stack(losses).cpu(), {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, loss_fn

    n_warm = TrainEngine.GRAPH_WARMUP
    assert len(batches) == n_warm + 4
    lg, pg, fg = run(True, (0.01, 0.5))
    le, pe, fe = run(False, (0.01, 0.5))
    assert torch.equal(lg, le), (lg, le)  # three replayed steps and the step after set_alpha(0.5), bit for bit
    assert all(torch.equal(pg[k], pe[k]) for k in pe)
    lo, po, _ = run(True, (0.01, 0.01))
    assert torch.equal(lo[:-1], lg[:-1]) and not torch.equal(lo[-1], lg[-1])  # the replay did read the new alpha
    assert torch.isfinite(lg).all()
    # the by-products reconstruct the returned loss: (1 - alpha) region + alpha boundary
    for f, l in ((fg, lg), (fe, le)):
        want = 0.5 * f.last_region.item() + 0.5 * f.last_boundary.item()
        assert l[-1].item() == pytest.approx(want, rel=1e-6, abs=1e-7)
