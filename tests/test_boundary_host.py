"""CPU-side checks of the boundary loss: the scipy restatement of tests/_boundary_ref.py against the brute-force definition, its
analytic gradient against autograd, the argument errors of the new C-ABI entry points (reported without a device), the missing CPU
fallback, and RegionAndBoundaryLoss's alpha arithmetic on stub losses."""
import ctypes

import numpy as np
import pytest
import torch

import _boundary_ref as R
import mia_hip


def _masks():
    out = {}
    m = np.zeros((9, 11), bool); m[4, 6] = True
    out["single_pixel"] = m
    m = np.zeros((9, 11), bool); m[0:4, 0:5] = True
    out["touches_edge"] = m
    m = np.zeros((9, 11), bool); m[1:8, 2:10] = True; m[3:6, 4:7] = False
    out["hole"] = m
    out["absent"] = np.zeros((9, 11), bool)
    out["full"] = np.ones((9, 11), bool)
    rng = np.random.default_rng(3)
    out["noise"] = rng.random((8, 7)) > 0.6
    out["1x1_set"] = np.ones((1, 1), bool)
    out["1x1_clear"] = np.zeros((1, 1), bool)
    m = np.zeros((1, 9), bool); m[0, 2:4] = True; m[0, 8] = True
    out["1xW"] = m
    m = np.zeros((7, 1), bool); m[0:2, 0] = True
    out["Hx1"] = m
    return out


@pytest.mark.parametrize("name", sorted(_masks()))
@pytest.mark.parametrize("spacing", [None, (1.3, 0.4)])
def test_restatement_equals_brute_force_definition(name, spacing):
    m = _masks()[name]
    got, want = R.phi_mask(m, spacing), R.brute_phi(m, spacing)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    if name in ("absent", "full", "1x1_set", "1x1_clear"):
        assert (got == 0).all()


def test_definition_signs_and_edge_rule():
    m = _masks()["touches_edge"]
    phi = R.phi_mask(m)
    assert phi[0, 0] == -(min(4, 5) - 1)         # the corner is deep inside: the image edge is no boundary
    assert phi[3, 4] == 0 and phi[3, 0] == 0      # inner border pixels get 0 at unit spacing
    assert phi[4, 0] == 1 and phi[8, 10] == np.hypot(5, 6)
    assert (phi[m] <= 0).all() and (phi[~m] > 0).all()


def test_phi_labels_layout_and_foreign_label():
    lab = np.zeros((2, 5, 6), np.int64)
    lab[0, 1:3, 1:4] = 1
    lab[1, 2, 2] = 2
    lab[1, 0, 0] = 7                              # belongs to no class
    phi = R.phi_labels(lab, 3)
    assert phi.shape == (2, 2, 5, 6)
    np.testing.assert_array_equal(phi[0, 0], R.phi_mask(lab[0] == 1))
    assert (phi[0, 1] == 0).all() and (phi[1, 0] == 0).all()
    phi0 = R.phi_labels(lab, 3, classes=(0, 2))
    np.testing.assert_array_equal(phi0[1, 0], R.phi_mask(lab[1] == 0))
    np.testing.assert_array_equal(phi0[1, 1], R.phi_mask(lab[1] == 2))


@pytest.mark.parametrize("classes", [(1, 2), (0, 2), (1,)])
def test_analytic_gradient_equals_autograd(classes):
    g = torch.Generator().manual_seed(5)
    z = (torch.randn(2, 3, 6, 5, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    lab = torch.randint(0, 3, (2, 6, 5), generator=g).numpy()
    phi = R.phi_labels(lab, 3, classes, (1.3, 0.4))
    l = R.loss(z, phi, classes)
    (l * 0.7).backward()
    grad, mag, val, _ = R.grad_formula(z.detach(), phi, classes, 0.7)
    assert abs(float(val) - l.item()) <= 1e-14 * max(1.0, abs(l.item()))
    assert ((z.grad - grad).abs() <= 1e-13 * mag + 1e-300).all()


# ---------------------------------------------------------------- C ABI: argument errors without a device
def _ptr(v):
    return None if v is None else ctypes.c_void_p(16 * v)  # never dereferenced: the checks fail before any launch


def _err(rc):
    assert rc < 0
    return mia_hip.lib().mia_last_error().decode()


def _sdm(**kw):
    a = dict(labels=1, u8=0, nb=1, h=8, w=8, k1=3, mask=6, sh=1.0, sw=1.0, ws=1, phi=1)
    a.update(kw)
    return mia_hip.lib().mia_signed_distance_map(_ptr(a["labels"]), a["u8"], a["nb"], a["h"], a["w"], a["k1"], a["mask"],
                                                 ctypes.c_float(a["sh"]), ctypes.c_float(a["sw"]), _ptr(a["ws"]), _ptr(a["phi"]), None)


def _fwd(**kw):
    a = dict(logits=1, labels=1, u8=0, phi=1, weight=None, nb=1, hw=64, k1=3, mask=6, slabs=1, ws=1, coef=1, out=1, bad=1)
    a.update(kw)
    return mia_hip.lib().mia_boundary_loss_fwd(_ptr(a["logits"]), _ptr(a["labels"]), a["u8"], _ptr(a["phi"]), _ptr(a["weight"]), a["nb"],
                                               ctypes.c_int64(a["hw"]), a["k1"], a["mask"], ctypes.c_int64(192), ctypes.c_int64(64),
                                               ctypes.c_int64(1), a["slabs"], _ptr(a["ws"]), _ptr(a["coef"]), _ptr(a["out"]),
                                               _ptr(a["bad"]), None)


def _bwd(**kw):
    a = dict(logits=1, phi=1, coef=1, weight=None, gout=None, dl=1, nb=1, hw=64, k1=3, mask=6)
    a.update(kw)
    i64 = ctypes.c_int64
    return mia_hip.lib().mia_boundary_loss_bwd(_ptr(a["logits"]), _ptr(a["phi"]), _ptr(a["coef"]), _ptr(a["weight"]), _ptr(a["gout"]),
                                               _ptr(a["dl"]), a["nb"], i64(a["hw"]), a["k1"], a["mask"], i64(192), i64(64), i64(1),
                                               i64(192), i64(64), i64(1), None)


def test_sdm_workspace_and_limits():
    l = mia_hip.lib()
    assert l.mia_sdm_workspace(2, 5, 7, 3, 6) == 2 * 2 * 5 * 7
    assert l.mia_sdm_workspace(2, 5, 7, 3, 1) == 2 * 5 * 7
    assert l.mia_sdm_workspace(1, 4096, 4096, 8, 0xFF) == 8 * 4096 * 4096
    for bad in ((0, 5, 7, 3, 6), (1, 4097, 7, 3, 6), (1, 5, 4097, 3, 6), (1, 5, 7, 9, 6), (1, 5, 7, 0, 1), (1, 5, 7, 3, 0),
                (1, 5, 7, 3, 8), (1, 5, 7, 3, -2), (16, 4096, 4096, 8, 0xFF), (40000, 2, 2, 3, 6)):
        assert l.mia_sdm_workspace(*bad) < 0, bad
    assert l.mia_boundary_loss_workspace(3, 4) == 24
    assert l.mia_boundary_loss_workspace(0, 4) < 0 and l.mia_boundary_loss_workspace(3, 0) < 0


def test_signed_distance_map_argument_errors():
    for name in ("labels", "ws", "phi"):
        assert "null pointer" in _err(_sdm(**{name: None}))
    assert "k1=9" in _err(_sdm(k1=9, mask=6))
    assert "class_mask" in _err(_sdm(mask=0))
    assert "class_mask" in _err(_sdm(mask=8))          # class 3 of k1 = 3
    assert "limits" in _err(_sdm(h=4097))
    assert "limits" in _err(_sdm(w=4097))
    assert "limits" in _err(_sdm(nb=0))
    assert "spacing" in _err(_sdm(sh=0.0))
    assert "spacing" in _err(_sdm(sw=float("inf")))
    assert "spacing" in _err(_sdm(sw=float("nan")))
    assert "too small" in _err(_sdm(sh=1e-30))
    assert "too large" in _err(_sdm(sh=1e15, h=4096))


def test_boundary_loss_argument_errors():
    for name in ("logits", "labels", "phi", "ws", "coef", "out", "bad"):
        assert "null pointer" in _err(_fwd(**{name: None}))
    assert "bad shape" in _err(_fwd(nb=0))
    assert "bad shape" in _err(_fwd(hw=0))
    assert "bad shape" in _err(_fwd(slabs=0))
    assert "k1=9" in _err(_fwd(k1=9))
    assert "class_mask" in _err(_fwd(mask=0))
    assert "class_mask" in _err(_fwd(mask=9))
    for name in ("logits", "phi", "coef", "dl"):
        assert "null pointer" in _err(_bwd(**{name: None}))
    assert "bad shape" in _err(_bwd(nb=0))
    assert "k1=0" in _err(_bwd(k1=0, mask=1))
    assert "class_mask" in _err(_bwd(mask=16))


# ---------------------------------------------------------------- Python layer
def test_no_cpu_fallback():
    from losses.boundary_loss import BoundaryLoss, signed_distance_map
    z = torch.randn(1, 3, 8, 8)
    y = torch.randint(0, 3, (1, 8, 8))
    with pytest.raises(mia_hip.MiaError):
        BoundaryLoss(2)(z, y)
    with pytest.raises(mia_hip.MiaError):
        signed_distance_map(y, 2)


def test_constructor_checks():
    from losses.boundary_loss import BoundaryLoss, RegionAndBoundaryLoss
    b = BoundaryLoss(2)
    assert b.num_classes == 3 and b.classes == (1, 2) and b.mask == 6
    assert BoundaryLoss(2, classes=(2, 0)).classes == (0, 2)
    with pytest.raises(NotImplementedError):
        BoundaryLoss(2, dimension=3)
    with pytest.raises(mia_hip.MiaError):
        BoundaryLoss(2, classes=(3,))
    with pytest.raises(mia_hip.MiaError):
        BoundaryLoss(2, classes=())
    with pytest.raises(NotImplementedError):
        BoundaryLoss(2, spacing=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        RegionAndBoundaryLoss(b, b, mode="mix")


class _StubRegion(torch.nn.Module):
    def forward(self, z, y):
        return z.sum() * 2.0


class _StubBoundary(torch.nn.Module):
    last_value = None

    def forward(self, z, y, dist=None, *, weight=None):
        self.last_value = (z * z).sum().detach()
        return (z * z).sum() * weight[0]


@pytest.mark.parametrize("mode", ["rebalance", "add"])
def test_alpha_arithmetic_on_stub_losses(mode):
    from losses.boundary_loss import RegionAndBoundaryLoss
    loss = RegionAndBoundaryLoss(_StubRegion(), _StubBoundary(), alpha=0.25, mode=mode)
    z = torch.tensor([1.0, -2.0, 0.5], requires_grad=True)
    r, b = 2.0 * (-0.5), 1.0 + 4.0 + 0.25

    def want(a):
        return ((1.0 - a) if mode == "rebalance" else 1.0) * r + a * b

    out = loss(z, None)
    assert out.item() == pytest.approx(want(0.25), rel=1e-6)
    assert loss.alpha == 0.25 and float(loss.last_region) == r and float(loss.last_boundary) == b
    out.backward()
    rw = 0.75 if mode == "rebalance" else 1.0
    torch.testing.assert_close(z.grad, rw * 2.0 + 0.25 * 2.0 * z.detach())
    buf = loss._buf
    loss.set_alpha(0.5)
    assert loss._buf is buf, "set_alpha writes the existing device buffer (a captured graph keeps reading it)"
    assert loss.alpha == 0.5 and loss(z, None).item() == pytest.approx(want(0.5), rel=1e-6)
    loss.set_alpha(0.0)
    assert loss(z, None).item() == pytest.approx(r, rel=1e-6)
