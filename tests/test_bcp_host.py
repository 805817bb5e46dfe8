"""Host-side tests of bidirectional copy-paste (no GPU): the float64 restatement against the published expression under torch's
autograd and against central differences, the box mask, the argument checks of the new entry points, the no-CPU-fallback rule and
`BCPEngine`'s batch checks."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bcp_ref as R
import mia_hip


# ---------------------------------------------------------------- the restatement against the published expression
def _published_dice(score, target, mask, k, smooth=1e-10):
    """The masked Dice of the published code: per class 1 - (2 sum(s t m) + smooth) / (sum(s s m) + sum(t t m) + smooth), mean."""
    loss = 0.0
    for c in range(k):
        s, t = score[:, c], (target == c).double()
        inter, y_sum, z_sum = (s * t * mask).sum(), (t * t * mask).sum(), (s * s * mask).sum()
        loss = loss + (1 - (2 * inter + smooth) / (z_sum + y_sum + smooth))
    return loss / k


def _published_mix_loss(z, img_l, patch_l, mask, image_weight, patch_weight):
    """`mix_loss` of the published training script: two soft-max Dice terms and two masked CE means, halved."""
    k = z.shape[1]
    patch_mask = 1 - mask
    soft = F.softmax(z, dim=1)
    dice = _published_dice(soft, img_l, mask, k) * image_weight + _published_dice(soft, patch_l, patch_mask, k) * patch_weight
    ce = image_weight * (F.cross_entropy(z, img_l, reduction="none") * mask).sum() / (mask.sum() + 1e-16)
    ce = ce + patch_weight * (F.cross_entropy(z, patch_l, reduction="none") * patch_mask).sum() / (patch_mask.sum() + 1e-16)
    return (dice + ce) / 2


@pytest.mark.parametrize("per_image", [False, True], ids=["mask_hw", "mask_bhw"])
@pytest.mark.parametrize("k1", [2, 4, 8])
def test_restatement_equals_published_expression(k1, per_image):
    nb, h, w = 2, 9, 11
    z, ya, yb = R.make_case(nb, k1, h, w, absent=k1 == 4)
    mask = R.make_mask(nb, h, w, per_image)
    for wa, wb in ((1.0, 1.0), (0.5, 1.0), (1.0, 0.0)):
        ref = R.evaluate(z, ya, yb, mask, wa, wb)
        t = torch.tensor(z, dtype=torch.float64, requires_grad=True)
        m = torch.tensor((mask != 0).astype(np.float64))
        m = m.expand(nb, h, w) if m.ndim == 3 else m[None].expand(nb, h, w)
        loss = _published_mix_loss(t, torch.tensor(ya), torch.tensor(yb), m, wa, wb)
        loss.backward()
        assert 0 < ref["counts"][0] < nb * h * w and sum(ref["counts"]) == nb * h * w  # both regions
        assert abs(loss.item() - ref["value"]) <= 1e-12 * abs(ref["value"])
        g = t.grad.numpy()
        assert np.abs(g - ref["grad"]).max() <= 1e-12 * np.abs(g).max()
        assert ref["value"] == pytest.approx(wa * (ref["terms"][0] + ref["terms"][1]) / 2 + wb * (ref["terms"][2] + ref["terms"][3]) / 2,
                                             rel=1e-15)


def test_restatement_gradient_against_central_differences():
    nb, k1, h, w = 1, 3, 3, 4
    z, ya, yb = R.make_case(nb, k1, h, w)
    z = z.astype(np.float64)
    mask = R.make_mask(nb, h, w)
    ref = R.evaluate(z, ya, yb, mask, 0.5, 1.0)
    eps = 1e-6
    num = np.zeros_like(z)
    for i in range(z.size):
        d = np.zeros(z.size)
        d[i] = eps
        d = d.reshape(z.shape)
        num.reshape(-1)[i] = (R.evaluate(z + d, ya, yb, mask, 0.5, 1.0)["value"] - R.evaluate(z - d, ya, yb, mask, 0.5, 1.0)["value"]) / (2 * eps)
    assert np.abs(num - ref["grad"]).max() <= 1e-8 * max(1.0, np.abs(ref["grad"]).max())
    assert (np.abs(ref["grad"]) <= ref["grad_mag"] * (1 + 1e-12)).all()  # the bound's magnitude dominates the gradient


def test_restatement_edges():
    nb, k1, h, w = 2, 3, 5, 6
    z, ya, yb = R.make_case(nb, k1, h, w)
    ones, zeros = np.ones((h, w), np.uint8), np.zeros((h, w), np.uint8)
    a = R.evaluate(z, ya, yb, ones, 1.0, 1.0)
    assert a["counts"] == (nb * h * w, 0) and a["terms"][2:] == [0.0, 0.0] and np.isfinite(a["grad"]).all()
    b = R.evaluate(z, ya, yb, zeros, 1.0, 1.0)
    assert b["counts"] == (0, nb * h * w) and b["terms"][:2] == [0.0, 0.0]
    # a pixel reads only its own region's label: garbage in the other map changes nothing
    junk = np.full_like(yb, 255)
    c = R.evaluate(z, ya, junk, ones, 1.0, 1.0)
    assert c["value"] == a["value"] and np.array_equal(c["grad"], a["grad"])
    # the single-source case: region A alone is the masked Dice + CE of ya
    single = R.evaluate(z, ya, ya, ones, 1.0, 0.0)
    assert single["value"] == a["value"] and np.array_equal(single["grad"], a["grad"])
    assert not R.evaluate(z, ya, yb, R.make_mask(nb, h, w), 0.0, 0.0)["grad"].any()
    sat = R.evaluate(*R.saturated_case(nb, k1, h, w), R.make_mask(nb, h, w))
    assert np.isfinite(sat["value"]) and np.isfinite(sat["grad"]).all() and sat["terms"][1] > 10
    assert np.array_equal(R.mix(np.float32([[[[1, 2]]]]), np.float32([[[[3, 4]]]]), np.uint8([[0, 7]])), np.float32([[[[3, 2]]]]))


# ---------------------------------------------------------------- the box mask
@pytest.mark.parametrize("h,w,ratio", [(32, 32, 2 / 3), (37, 61, 2 / 3), (8, 12, 0.5), (5, 5, 1.0), (3, 100, 0.34)])
def test_box_mask_is_one_box_inside_the_image(h, w, ratio):
    from losses.copy_paste import random_box_mask
    corners = set()
    for seed in range(40):
        torch.manual_seed(seed)
        m = random_box_mask(h, w, ratio, device="cpu")
        assert m.dtype == torch.uint8 and tuple(m.shape) == (h, w) and set(np.unique(m.numpy())) <= {0, 1}
        box = R.find_box(m.numpy())
        assert box is not None and box[2:] == (int(h * ratio), int(w * ratio))  # exactly one zero box of that size, inside
        assert np.array_equal(m.numpy(), R.box_mask(h, w, ratio, box[0], box[1]))
        corners.add(box[:2])
        torch.manual_seed(seed)
        assert torch.equal(random_box_mask(h, w, ratio, device="cpu"), m)  # reproducible under torch.manual_seed
    positions = (h - int(h * ratio) + 1) * (w - int(w * ratio) + 1)
    assert len(corners) > min(positions, 40) // 3  # the corner moves
    for y0, x0 in corners:
        assert 0 <= y0 <= h - int(h * ratio) and 0 <= x0 <= w - int(w * ratio)


def test_box_mask_ratio_zero_and_generator():
    from losses.copy_paste import random_box_mask
    assert random_box_mask(7, 9, 0.0, device="cpu").all()
    assert random_box_mask(1, 1, 2 / 3, device="cpu").all()  # int(2/3) = 0: no box
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    a = [random_box_mask(30, 30, generator=g1, device="cpu") for _ in range(3)]
    b = [random_box_mask(30, 30, generator=g2, device="cpu") for _ in range(3)]
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not all(torch.equal(a[0], x) for x in a[1:])
    with pytest.raises(ValueError):
        random_box_mask(8, 8, 1.5, device="cpu")


# ---------------------------------------------------------------- C ABI: argument errors without a device
def _ptr(v):
    return None if v is None else ctypes.c_void_p(16 * v)  # never dereferenced: the checks fail before any launch


def _i64(v):
    return ctypes.c_int64(v)


def _mix(**kw):
    a = dict(fg=1, bg=1, mask=1, out=1, nb=1, c=2, hw=64, msn=0, osn=128)
    a.update(kw)
    mia_hip.call("mia_bcp_mix", _ptr(a["fg"]), _ptr(a["bg"]), _ptr(a["mask"]), _ptr(a["out"]), a["nb"], a["c"], _i64(a["hw"]),
                 _i64(a["msn"]), _i64(a["osn"]), None)


def _fwd(**kw):
    a = dict(z=1, la=1, lb=1, mask=1, nb=1, hw=64, k1=3, st=(192, 64, 1), msn=0, u8=0, slabs=1, ws=1, coef=1, out=1, counts=1, bad=1)
    a.update(kw)
    mia_hip.call("mia_bcp_loss_fwd", _ptr(a["z"]), _ptr(a["la"]), _ptr(a["lb"]), _ptr(a["mask"]), a["nb"], _i64(a["hw"]), a["k1"],
                 *(_i64(s) for s in a["st"]), _i64(a["msn"]), a["u8"], ctypes.c_float(1e-10), ctypes.c_float(1.0), ctypes.c_float(1.0),
                 a["slabs"], _ptr(a["ws"]), _ptr(a["coef"]), _ptr(a["out"]), _ptr(a["counts"]), _ptr(a["bad"]), None)


def _bwd(**kw):
    a = dict(z=1, la=1, lb=1, mask=1, coef=1, gout=None, dz=1, nb=1, hw=64, k1=3, st=(192, 64, 1), gst=(192, 64, 1), msn=0, u8=0)
    a.update(kw)
    mia_hip.call("mia_bcp_loss_bwd", _ptr(a["z"]), _ptr(a["la"]), _ptr(a["lb"]), _ptr(a["mask"]), _ptr(a["coef"]), _ptr(a["gout"]),
                 _ptr(a["dz"]), a["nb"], _i64(a["hw"]), a["k1"], *(_i64(s) for s in a["st"]), *(_i64(s) for s in a["gst"]),
                 _i64(a["msn"]), a["u8"], None)


def test_bcp_argument_errors():
    for name in ("fg", "bg", "mask", "out"):
        with pytest.raises(mia_hip.MiaError, match="mia_bcp_mix: null pointer"):
            _mix(**{name: None})
    for kw in (dict(nb=0), dict(c=0), dict(hw=0), dict(hw=1 << 31), dict(c=1 << 16, hw=1 << 16)):
        with pytest.raises(mia_hip.MiaError, match="mia_bcp_mix: bad shape"):
            _mix(**kw)
    for kw in (dict(msn=32), dict(osn=127), dict(msn=-64)):
        with pytest.raises(mia_hip.MiaError, match="mia_bcp_mix: bad strides"):
            _mix(**kw)
    for name in ("z", "la", "lb", "mask", "ws", "coef", "out", "counts", "bad"):
        with pytest.raises(mia_hip.MiaError, match="mia_bcp_loss_fwd: null pointer"):
            _fwd(**{name: None})
    for kw in (dict(nb=0), dict(hw=0), dict(slabs=0), dict(nb=1 << 16, hw=1 << 16), dict(nb=1 << 20, slabs=1 << 10)):
        with pytest.raises(mia_hip.MiaError, match="mia_bcp_loss_fwd: bad shape"):
            _fwd(**kw)
    for k1 in (0, 9):
        with pytest.raises(mia_hip.MiaError, match=f"k1={k1}"):
            _fwd(k1=k1)
        with pytest.raises(mia_hip.MiaError, match=f"k1={k1}"):
            _bwd(k1=k1)
    for kw in (dict(st=(192, -64, 1)), dict(msn=8)):
        with pytest.raises(mia_hip.MiaError, match="mia_bcp_loss_fwd: bad strides"):
            _fwd(**kw)
    for name in ("z", "la", "lb", "mask", "coef", "dz"):
        with pytest.raises(mia_hip.MiaError, match="mia_bcp_loss_bwd: null pointer"):
            _bwd(**{name: None})
    for kw in (dict(nb=0), dict(hw=0), dict(nb=1 << 16, hw=1 << 16)):
        with pytest.raises(mia_hip.MiaError, match="mia_bcp_loss_bwd: bad shape"):
            _bwd(**kw)
    for kw in (dict(gst=(192, 64, -1)), dict(st=(-1, 64, 1)), dict(msn=1)):
        with pytest.raises(mia_hip.MiaError, match="mia_bcp_loss_bwd: bad strides"):
            _bwd(**kw)
    lib = mia_hip.lib()
    assert lib.mia_bcp_loss_workspace(3, 8, 4) == 3 * 4 * 2 * (17 * 2 + 9)  # per block and region: 2 K + 1 pairs and K + 1 counts
    assert lib.mia_bcp_loss_workspace(0, 3, 4) < 0 and lib.mia_bcp_loss_workspace(3, 9, 4) < 0 and lib.mia_bcp_loss_workspace(3, 3, 0) < 0
    assert lib.mia_bcp_loss_workspace(1 << 20, 8, 1 << 10) < 0


def test_new_symbols_are_declared_and_exported():
    protos = mia_hip.parse_header()
    l = ctypes.CDLL(mia_hip.LIB_PATH)
    for name, nargs in (("mia_bcp_mix", 10), ("mia_bcp_loss_workspace", 3), ("mia_bcp_loss_fwd", 22), ("mia_bcp_loss_bwd", 19)):
        assert name in protos and len(protos[name][1]) == nargs, name
        assert hasattr(l, name), f"{name} declared in include/mia_hip.h but not exported"


# ---------------------------------------------------------------- Python layer
def test_no_cpu_fallback_and_class_limit():
    from losses.copy_paste import CopyPasteLoss
    from mia_hip import ops
    z = torch.randn(2, 3, 8, 8, requires_grad=True)
    ya, yb = torch.randint(0, 3, (2, 8, 8)), torch.randint(0, 3, (2, 8, 8))
    mask = torch.ones(8, 8, dtype=torch.uint8)
    for fused in (True, False):
        with pytest.raises(mia_hip.MiaError):
            CopyPasteLoss(2, fused=fused)(z, ya, yb, mask)
    with pytest.raises(mia_hip.MiaError):
        ops.CopyPasteLossFn.apply(z, ya, yb, mask, 1.0, 1.0, 1e-10)
    with pytest.raises(mia_hip.MiaError):
        ops.bcp_mix(torch.zeros(1, 1, 4, 4), torch.ones(1, 1, 4, 4), torch.ones(4, 4, dtype=torch.uint8))
    with pytest.raises(mia_hip.MiaError):
        CopyPasteLoss(8)  # nine classes with the background
    assert ops.BCP_MAX_CLASSES == 8 and CopyPasteLoss(7).num_classes == 8
    assert CopyPasteLoss(11, fused=False).num_classes == 12  # the tensor-op form takes more
    assert CopyPasteLoss(2).smooth == 1e-10


def test_tensor_op_form_equals_the_restatement_in_float64():
    """`fused=False` is the same definition: its float64 value and gradient on the CPU, through the function the module calls."""
    from losses.copy_paste import copy_paste_loss_tensor_ops
    nb, k1, h, w = 2, 12, 7, 9  # more classes than the kernels take
    z, ya, yb = R.make_case(nb, k1, h, w)
    for per_image in (False, True):
        mask = R.make_mask(nb, h, w, per_image)
        ref = R.evaluate(z, ya, yb, mask, 0.5, 1.0)
        t = torch.tensor(z, dtype=torch.float64, requires_grad=True)
        loss, terms, counts = copy_paste_loss_tensor_ops(t, torch.tensor(ya), torch.tensor(yb), torch.tensor(mask), 0.5, 1.0)
        loss.backward()
        assert abs(loss.item() - ref["value"]) <= 1e-12 * abs(ref["value"])
        assert np.abs(terms.numpy() - np.array(ref["terms"])).max() <= 1e-12 and tuple(counts.tolist()) == ref["counts"]
        assert np.abs(t.grad.numpy() - ref["grad"]).max() <= 1e-12 * np.abs(ref["grad"]).max()
    empty = copy_paste_loss_tensor_ops(torch.tensor(z, dtype=torch.float64), torch.tensor(ya), torch.tensor(yb),
                                       torch.ones(h, w, dtype=torch.uint8))
    assert empty[1][2] == 0 and empty[1][3] == 0 and torch.isfinite(empty[0]) and empty[2].tolist() == [nb * h * w, 0]
    bad = torch.tensor(ya).clone()
    bad[0, 0, 0] = k1
    assert torch.isnan(copy_paste_loss_tensor_ops(torch.tensor(z), bad, torch.tensor(yb), torch.ones(h, w, dtype=torch.uint8))[0])
    assert torch.isfinite(copy_paste_loss_tensor_ops(torch.tensor(z), torch.tensor(ya), bad, torch.ones(h, w, dtype=torch.uint8))[0])


def _tiny(seed, classes=3):
    from models.unet import UNet
    torch.manual_seed(seed)
    return UNet(2, 1, classes, [4, 8], normalization="instance")


def test_bcp_engine_constructor_and_batch_checks():
    from losses.copy_paste import CopyPasteLoss
    from training.semi import BCPEngine, MeanTeacherEngine, _EMATeacher
    eng = BCPEngine(_tiny(1), _tiny(2), labeled_bs=4)
    assert isinstance(eng, _EMATeacher) and issubclass(MeanTeacherEngine, _EMATeacher)
    assert isinstance(eng.loss, CopyPasteLoss) and eng.loss.num_classes == 3 and eng.num_classes == 3
    assert eng.u_weight == 0.5 and eng.mask_ratio == 2 / 3 and eng.ema_decay == 0.99 and eng.pseudo_largest_component and not eng.pretrain
    assert eng.ema_step == 0 and torch.equal(eng.teacher_flat, eng.optimizer.flat_param)  # adopted bit for bit
    for p, o, t in zip(eng.optimizer.params, eng.optimizer.offsets, eng.teacher_params):
        assert t.data_ptr() == eng.teacher_flat.data_ptr() + 4 * o and not t.requires_grad
    for lb in (3, 1, 0):
        with pytest.raises(ValueError, match="labeled_bs"):
            BCPEngine(_tiny(1), _tiny(2), labeled_bs=lb)
    with pytest.raises(ValueError, match="mask_ratio"):
        BCPEngine(_tiny(1), _tiny(2), labeled_bs=2, mask_ratio=1.5)
    with pytest.raises(ValueError, match="architecture"):
        BCPEngine(_tiny(1), _tiny(2, classes=4), labeled_bs=2)
    for nimg in (6, 9, 4):
        batch = {"image": torch.zeros(nimg, 1, 16, 16), "label": torch.zeros(4, 16, 16, dtype=torch.long)}
        with pytest.raises(ValueError, match="labeled_bs=4"):
            eng.train_step(batch)
    with pytest.raises(ValueError, match="labeled_bs=4"):
        eng.train_step({"image": torch.zeros(8, 1, 16, 16), "label": torch.zeros(2, 16, 16, dtype=torch.long)})
    assert eng.current_iter == 0
