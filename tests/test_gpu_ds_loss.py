"""GPU checks of the deep-supervision loss (csrc/ds_loss.hip: Dice + CE of bilinearly upsampled low-resolution logits) against the
float64 restatement in tests/_ds_loss_ref.py, called through the C ABI, then at op, model and engine level.  Inputs are seeded and
exactly representable in fp32; every output buffer (the gaps of padded layouts included) starts as NaN, the gaps must still be NaN
afterwards and every element a kernel owns finite.

Launch -> branch -> case (test[parameters]):
  mia_ds_loss_fwd
    ds_loss_fwd_kernel<K1, VEC = true>, K1 = 2, 3, 4 (two pixels per 16-byte label load)
      every factor x (1,1) / (1,5) / (3,3) / (5,7), one and two slabs of rows .... test_ds_shapes[*] with k1 in 2, 3, 4
      three slabs of rows, the last ragged or empty ............................... test_ds_shapes[*-(40,24) | (18,11) | (9,6) | (5,4)-*-3]
      more slabs than rows (two rows on five slabs: three empty blocks) ........... test_ds_more_slabs_than_rows
    ds_loss_fwd_kernel<8, VEC>, run-time k1 = 1, 5, 8 ............................. test_ds_shapes[*] with k1 in 1, 5, 8
    ds_loss_fwd_kernel<*, VEC = false> (labels 8 bytes off a 16-byte boundary) ..... every fourth case of test_ds_shapes, test_ds_layouts[*-off]
    z channels-last / NCHW / padded pixel stride k1 + 1 ........................... test_ds_layouts, and in rotation test_ds_shapes
    dice_ce_finalize_kernel (shared with mia_dice_ce_fwd), all 16 flag sets ....... test_ds_flags[fast | generic]
    MIA_LOSS_DENSE, factor 3, k1 = 9 refused ...................................... test_ds_argument_errors
  mia_ds_loss_bwd
    ds_loss_bwd_kernel<K1>, K1 = 2, 3, 4 and <8> with k1 = 1, 5, 8
      tile larger than the image, both taps on one pixel ......................... test_ds_shapes[*-1-1-*]
      ragged last tile in both directions, 2 x 2 .. 5 x 2 tiles ................... test_ds_shapes[*-(40,24) | (18,11) | (9,6) | (5,4)-*]
      tile shrunk to fit the LDS budget (factor 16: 3x3 for k1 <= 3, 2x3 for 4, 2x2 for 5, 1x2 for 8) test_ds_shapes[*-16-*]
      dz channels-last / NCHW / padded, independent of z's layout ................. test_ds_layouts (all nine pairs)
      grad_out NULL and a device scalar; dice_w / ce_w != 1, one of them 0 ........ test_ds_weights_and_upstream
    hand-built label sets ........................................................ test_ds_hand_built
    labels k1, -1, 2^32 + 1 ...................................................... test_ds_bad_labels[fast | generic]
    two calls, bit-identical out / sums / dz ..................................... test_ds_deterministic
  ops.UpsampleDiceCEFn against DiceCEFn(ResizeBilinearFn(z)) ...................... test_op_matches_the_composition
  UNet.forward(upsample_ds=False), DeepSupervisionLoss fused against fused=False .. test_model_*
  TrainEngine(deep_supervision=True) ............................................. test_engine_*

Tolerances (the rules of tests/test_gpu_head_loss.py; relerr = max |error| / max |reference|, float64): loss scalars absolutely
2e-6; sums and coef 2e-5 (label counts exact); dz relerr < 2e-5 -- at factor 16 a dz element sums up to 32 x 32 products, the figures
are printed before they are asserted.  Model level: eval outputs atol 1e-4, parameter gradients relerr 1e-4 (the bound of the head's
dW)."""
import os

import numpy as np
import pytest
import torch

import _ds_loss_ref as D
import _head_loss_ref as R
import test_gpu_head_loss as HL
import test_gpu_norm as G

pytestmark = pytest.mark.gpu

TOL32, LOSS_ATOL, GRAD_TOL = G.TOL32, 2e-6, 1e-4
_dev, _abi, rel = G._dev, G._abi, G.rel
Buf, nan_f32, place_labels, flag_bits = HL.Buf, HL.nan_f32, HL.place_labels, HL.flag_bits
_id = lambda k: "-".join(str(x) for x in k)
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def run_ds(z, labels, factor, dev, *, slabs=1, flags=D.DEFAULT_FLAGS, layout="cl", dz_layout=None, weights=D.DEFAULT_WEIGHTS, gout=None,
           labels_off=False, bad=None, dense=False):
    """mia_ds_loss_fwd, then mia_ds_loss_bwd.  z [B, h, w, K] float64 (fp32-exact), labels [B, H, W] int64."""
    mia_hip, ops = _abi()
    _p, cf = ops._p, ops._c_float
    nb, h, w, k1 = z.shape
    zb = Buf((nb, h * w, k1), layout, dev, values=z.reshape(nb, h * w, k1))
    tg = place_labels(labels, dev, labels_off)
    bits = flag_bits(flags, dense)
    ws = nan_f32((mia_hip.lib().mia_ds_loss_workspace(nb, k1, slabs),), dev)
    sums, coef, out = nan_f32((nb, k1, 3), dev), nan_f32((nb, k1, 2), dev), nan_f32((3,), dev)
    bad = torch.zeros(2, dtype=torch.int32, device=dev) if bad is None else bad
    mia_hip.call("mia_ds_loss_fwd", _p(zb.view), _p(tg), nb, h, w, factor, k1, *zb.strides(ops), bits, cf(R.SMOOTH), cf(weights[0]),
                 cf(weights[1]), slabs, _p(ws), _p(sums), _p(coef), _p(out), _p(bad), ops._stream())
    dz = Buf((nb, h * w, k1), dz_layout or layout, dev)
    gd = None if gout is None else torch.tensor([gout], dtype=torch.float32, device=dev)
    mia_hip.call("mia_ds_loss_bwd", _p(zb.view), _p(tg), _p(coef), _p(gd), _p(dz.view), nb, h, w, factor, k1, *zb.strides(ops),
                 *dz.strides(ops), bits, cf(weights[0]), cf(weights[1]), ops._stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ws).all()), "a slab partial was never written"
    return dict(sums=sums, coef=coef, out=out, bad=bad, dz=dz)


def check_ds(got, ref, what=""):
    """Each figure is printed before it is asserted."""
    figs = {"out": (got["out"].double().cpu() - ref["out"]).abs().max().item()}
    for j, name in enumerate(("I", "S")):
        figs[name] = rel(got["sums"][..., j], ref["sums"][..., j])
    for j, name in enumerate(("alpha", "beta")):
        figs[name] = rel(got["coef"][..., j], ref["coef"][..., j])
    dz = got["dz"]
    dz.check_written()
    nb, p, k1 = dz.view.shape
    want = ref["dz"].reshape(nb, p, k1)
    top = want.abs().max().item()
    figs["dz_abs"] = (dz.view.double().cpu() - want).abs().max().item()
    figs["dz_rel"] = figs["dz_abs"] / top if top > 0 else 0.0
    print(f"ds loss {what}: " + " ".join(f"{k}={v:.3e}" for k, v in figs.items()))
    assert bool(torch.isfinite(got["out"]).all()) and figs["out"] < LOSS_ATOL
    assert figs["I"] < TOL32 and figs["S"] < TOL32 and figs["alpha"] < TOL32 and figs["beta"] < TOL32
    assert torch.equal(got["sums"][..., 2].double().cpu(), ref["sums"][..., 2]), "label counts are integers"
    assert not got["coef"].cpu()[ref["coef"] == 0].any()
    if top == 0:  # one class: softmax = 1 = t, every term of the gradient cancels exactly
        assert not dz.view.any(), "the gradient of a one-class loss is exactly 0"
    assert figs["dz_rel"] < TOL32
    assert got["bad"].tolist() == [0, 0]


# ================================================================== kernel level
@pytest.mark.parametrize("i,case", list(enumerate(D.shape_cases())), ids=lambda v: _id(v) if isinstance(v, tuple) else f"c{v}")
def test_ds_shapes(i, case):
    """Every factor on the shapes at which a tap clamps, a tile or a slab is ragged or empty, and more than one tile and slab are at
    work, for every class count of both routes; z and dz layouts and the labels' alignment rotate through the cases."""
    dev = _dev()
    nb, h, w, f, k1, slabs = case
    z, labels, ref = D.reference(D.key(nb, h, w, f, k1))
    got = run_ds(z, labels, f, dev, slabs=slabs, layout=D.LAYOUTS[i % 3], dz_layout=D.LAYOUTS[(i // 3) % 3], labels_off=i % 4 == 3)
    check_ds(got, ref, _id(case))


@pytest.mark.parametrize("k1", [3, 8])
def test_ds_more_slabs_than_rows(k1):
    """One low-resolution pixel at factor 2 is two rows of two labels; on five slabs three blocks own no row and write zeros."""
    dev = _dev()
    z, labels, ref = D.reference(D.key(3, 1, 1, 2, k1))
    check_ds(run_ds(z, labels, 2, dev, slabs=5), ref, f"five slabs k1={k1}")


@pytest.mark.parametrize("off", [False, True], ids=["aligned", "off"])
@pytest.mark.parametrize("dz_layout", D.LAYOUTS)
@pytest.mark.parametrize("layout", D.LAYOUTS)
@pytest.mark.parametrize("k1", [3, 5])
def test_ds_layouts(k1, layout, dz_layout, off):
    """Channels-last (what HeadFn returns), NCHW-contiguous and a padded pixel stride, for z and independently for dz."""
    dev = _dev()
    z, labels, ref = D.reference(D.key(3, 5, 7, 4, k1, gout=R.LOSS_GOUT))
    got = run_ds(z, labels, 4, dev, slabs=3, layout=layout, dz_layout=dz_layout, gout=R.LOSS_GOUT, labels_off=off)
    check_ds(got, ref, f"k1={k1} z={layout} dz={dz_layout} off={off}")


@pytest.mark.parametrize("flags", R.LOSS_FLAGS, ids=lambda f: "".join("SDBQ"[j] if v else "-" for j, v in enumerate(f)))
@pytest.mark.parametrize("route", ["fast", "generic"])
def test_ds_flags(route, flags):
    """All 16 sets of softmax / do_bg / batch / squared.  Softmax off: the inputs are probabilities in (0, 1), and so are their
    interpolations."""
    dev = _dev()
    nb, h, w, f = D.FLAG_SHAPE
    z, labels, ref = D.reference(D.key(nb, h, w, f, 3 if route == "fast" else 5, flags=flags, gout=R.LOSS_GOUT))
    got = run_ds(z, labels, f, dev, slabs=2, flags=flags, layout="cl" if route == "fast" else "nchw", gout=R.LOSS_GOUT)
    check_ds(got, ref, f"{route} {flags}")


@pytest.mark.parametrize("gout", [None, R.LOSS_GOUT])
@pytest.mark.parametrize("weights", R.LOSS_WEIGHTS, ids=_id)
@pytest.mark.parametrize("route", ["fast", "generic"])
def test_ds_weights_and_upstream(route, weights, gout):
    """(dice_w, ce_w) = (0.6, 0.9), Dice alone, CE alone; grad_out NULL (1) and a device scalar that is neither 0 nor 1."""
    dev = _dev()
    nb, h, w, f = D.FLAG_SHAPE
    flags = (True, False, False, False)
    z, labels, ref = D.reference(D.key(nb, h, w, f, 4 if route == "fast" else 8, flags=flags, weights=weights, gout=gout, seed=2))
    got = run_ds(z, labels, f, dev, slabs=3, flags=flags, weights=weights, gout=gout)
    check_ds(got, ref, f"{route} {weights} gout={gout}")


@pytest.mark.parametrize("route", ["fast", "generic"])
@pytest.mark.parametrize("do_bg", [False, True])
@pytest.mark.parametrize("special", ["absent", "unpredicted", "one_class"])
def test_ds_hand_built(special, do_bg, route):
    """The hand-built sets of _head_loss_ref.loss_inputs: a class absent from one image's labels (T = 0, I = 0: the smooth term
    alone), low-resolution logits whose class 0 is nowhere the maximum, an image of a single class."""
    dev = _dev()
    nb, h, w, f = D.FLAG_SHAPE
    flags = (True, do_bg, False, False)
    z, labels, ref = D.reference(D.key(nb, h, w, f, 3 if route == "fast" else 5, flags=flags, special=special))
    got = run_ds(z, labels, f, dev, slabs=3, flags=flags)
    check_ds(got, ref, f"{route} {special} do_bg={do_bg}")


@pytest.mark.parametrize("flags", [D.DEFAULT_FLAGS, (False, False, False, True)], ids=["softmax", "plain_squared"])
@pytest.mark.parametrize("which", R.BAD_LABELS, ids=str)
@pytest.mark.parametrize("route", ["fast", "generic"])
def test_ds_bad_labels(route, which, flags):
    """One label equal to k1, negative, or with its high word set over a valid low word: out and coef all NaN, the working flag
    re-armed and the sticky verdict set, no finite gradient anywhere.  A clean call afterwards on the same flags returns the correct
    finite loss and leaves the verdict standing."""
    dev = _dev()
    nb, h, w, f = D.FLAG_SHAPE
    k1 = 3 if route == "fast" else 5
    z, labels, ref = D.reference(D.key(nb, h, w, f, k1, flags=flags))
    wrong = R.bad_labels(labels.reshape(nb, -1), k1, which).reshape(labels.shape)
    got = run_ds(z, wrong, f, dev, slabs=3, flags=flags)
    assert bool(torch.isnan(got["out"]).all()) and bool(torch.isnan(got["coef"]).all())
    assert got["bad"].tolist() == [0, 1]
    dz = got["dz"]
    assert not bool(torch.isfinite(dz.view).any()), "a finite gradient after a bad label"
    assert bool(torch.isnan(dz.flat[dz.view.numel():]).all()), "wrote outside dz"
    clean = run_ds(z, labels, f, dev, slabs=3, flags=flags, bad=got["bad"])
    assert clean["bad"].tolist() == [0, 1], "the verdict is sticky"
    clean["bad"] = torch.zeros(2, dtype=torch.int32)
    check_ds(clean, ref, f"clean after bad {route} {which}")


@pytest.mark.parametrize("f,k1", [(2, 3), (4, 2), (8, 4), (16, 8)])
def test_ds_deterministic(f, k1):
    """No atomics, fixed accumulation order: two calls on the same inputs agree bit for bit."""
    dev = _dev()
    h, w = D.MULTI_TILE[f]
    z, labels, _ = D.reference(D.key(3 if k1 == 3 else 1, h, w, f, k1))
    a, b = (run_ds(z, labels, f, dev, slabs=3, dz_layout="nchw") for _ in range(2))
    for k in ("out", "sums", "coef"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["dz"].view, b["dz"].view)


def test_ds_argument_errors():
    mia_hip, _ = _abi()
    dev = _dev()
    z, labels, _ = D.reference(D.key(1, 3, 3, 2, 3))
    with pytest.raises(mia_hip.MiaError, match="dense"):
        run_ds(z, labels, 2, dev, dense=True)
    with pytest.raises(mia_hip.MiaError, match="factor"):
        run_ds(z, labels, 3, dev)
    z9, labels9 = D.ds_inputs(1, 3, 3, 2, 9)
    with pytest.raises(mia_hip.MiaError, match="k1=9"):
        run_ds(z9, labels9, 2, dev)
    assert mia_hip.lib().mia_ds_loss_workspace(3, 4, 5) == 3 * 5 * 13


# ================================================================== op level
@pytest.mark.parametrize("f,k1", [(2, 3), (4, 3), (8, 2), (16, 5)])
def test_op_matches_the_composition(f, k1):
    """ops.UpsampleDiceCEFn against DiceCEFn(ResizeBilinearFn(z)), the path it replaces: same loss within 2e-6, same dz within the
    rule above; check_labels() covers the new op."""
    from mia_hip import ops
    from transforms.hip.functional_hip import ResizeBilinearFn
    dev = _dev()
    h, w = D.MULTI_TILE[f]
    z, labels, ref = D.reference(D.key(3 if k1 in (3, 5) else 1, h, w, f, k1))
    flags = flag_bits(D.DEFAULT_FLAGS)
    zc = z.float().to(dev).contiguous().permute(0, 3, 1, 2)  # logical [B, K, h, w], channels-last storage like HeadFn's output
    lab = labels.to(dev)
    try:
        ops.check_labels()  # a verdict an earlier test left standing is not this test's
    except ops.MiaError:
        pass
    a = zc.clone().requires_grad_(True)
    fused = ops.UpsampleDiceCEFn.apply(a, lab, f, flags, R.SMOOTH, 0.6, 0.9, 0)
    assert ops.DiceCEFn.last_sums is not None and rel(ops.DiceCEFn.last_sums, ref["sums"]) < TOL32
    fused.backward()
    b = zc.clone().requires_grad_(True)
    comp = ops.DiceCEFn.apply(ResizeBilinearFn.apply(b, h * f, w * f), lab, flags, R.SMOOTH, 0.6, 0.9, 0)
    comp.backward()
    ops.check_labels()
    err = rel(a.grad, b.grad)
    print(f"op f={f} k1={k1}: loss {fused.item():.7f} / {comp.item():.7f} / {ref['out'][0].item():.7f} dz_rel={err:.3e}")
    assert abs(fused.item() - comp.item()) < LOSS_ATOL and abs(fused.item() - ref["out"][0].item()) < LOSS_ATOL
    assert err < TOL32
    bad = lab.clone()
    bad[0, 0, 0] = k1
    assert torch.isnan(ops.UpsampleDiceCEFn.apply(zc, bad, f, flags, R.SMOOTH, 0.6, 0.9, 0)).item()
    with pytest.raises(ops.MiaError, match="label lies outside"):
        ops.check_labels()


# ================================================================== model level
def _golden_model(dev):
    d = dict(np.load(os.path.join(GOLDEN, "unet_ds.npz")))
    from models.unet import UNet
    m = UNet(2, 1, 3, [4, 8, 16, 32], normalization="instance", dropout_prob=None, deep_supervision=True, ds_layer=3)
    m.load_state_dict({k[5:]: torch.from_numpy(v.copy()) for k, v in d.items() if k.startswith("init/")})
    return d, m.to(dev)


def _loss(**kw):
    from losses.compound_losses import DiceAndCELoss
    from losses.deep_supervision import DeepSupervisionLoss
    return DeepSupervisionLoss(DiceAndCELoss(dice_kwargs=dict(num_classes=2, do_bg=True)), **kw)


def test_model_low_resolution_outputs():
    """upsample_ds=False: the main logits and the heads' own-resolution logits (16 x 16, 8 x 8), which the restatement's upsampling
    takes to the reference's eval/ds{i}; the default still returns today's upsampled list."""
    dev = _dev()
    d, m = _golden_model(dev)
    x = torch.from_numpy(d["x"]).to(dev)
    with torch.no_grad():
        low = m.eval()(x, return_ds=True, upsample_ds=False)
        full = m(x, return_ds=True)
    assert [tuple(o.shape[-2:]) for o in low] == [(32, 32), (16, 16), (8, 8)]
    for i, o in enumerate(low):
        o = o.cpu().double().permute(0, 2, 3, 1)
        up = o if i == 0 else D.upsample(o, 32 // o.shape[1])
        np.testing.assert_allclose(up.permute(0, 3, 1, 2).numpy(), d[f"eval/ds{i}"], atol=1e-4)
        np.testing.assert_allclose(full[i].cpu().numpy(), d[f"eval/ds{i}"], atol=1e-4)


def test_model_fused_loss_matches_the_composition():
    """DeepSupervisionLoss on the fused kernel against fused=False (ResizeBilinearFn + DiceCEFn) through the whole model: the total
    within 2e-6, every parameter gradient within relerr 1e-4, and the heads do receive one."""
    dev = _dev()
    d, m = _golden_model(dev)
    x, y = torch.from_numpy(d["x"]).to(dev), torch.from_numpy(d["labels"]).to(dev)
    grads, totals = [], []
    for fused in (True, False):
        loss_fn = _loss(fused=fused)
        m.train().zero_grad(set_to_none=True)
        total = loss_fn(m(x, return_ds=True, upsample_ds=False), y)
        total.backward()
        assert tuple(loss_fn.last_terms.shape) == (3,) and loss_fn.last_terms.is_cuda
        w = [4 / 7, 2 / 7, 1 / 7]
        assert abs(sum(wi * t for wi, t in zip(w, loss_fn.last_terms.tolist())) - total.item()) < LOSS_ATOL
        totals.append(total.item())
        grads.append({n: p.grad.detach().clone() for n, p in m.named_parameters()})
    print(f"model: total fused {totals[0]:.7f} composition {totals[1]:.7f}")
    assert abs(totals[0] - totals[1]) < LOSS_ATOL
    for n, g in grads[0].items():
        err = rel(g, grads[1][n])
        assert err < GRAD_TOL, (n, err)
    assert grads[0]["decoder.ds.0.0.weight"].abs().max().item() > 0 and grads[0]["decoder.ds.1.0.weight"].abs().max().item() > 0


# ================================================================== engine
def _engine(dev, **kw):
    from losses.compound_losses import DiceAndCELoss
    from models.unet import UNet
    from training.engine import TrainEngine
    torch.manual_seed(11)
    m = UNet(2, 1, 3, [4, 8, 16, 32], normalization="instance", dropout_prob=None, deep_supervision=True, ds_layer=3).to(dev)
    loss_fn = DiceAndCELoss(dice_kwargs=dict(num_classes=2, do_bg=True))
    return m, TrainEngine(m, loss_fn, "adam", {"weight_decay": 5e-4}, start_lr=1e-2, num_iters=100, lr_warmup_iter=2, **kw)


def _batch():
    d = np.load(os.path.join(GOLDEN, "unet_ds.npz"))
    return {"image": torch.from_numpy(d["x"]), "label": torch.from_numpy(d["labels"])}


def test_engine_trains_the_auxiliary_heads():
    """Three steps with deep_supervision=True move every decoder.ds.* parameter; without it they get no gradient and stay put."""
    dev = _dev()
    batch = _batch()
    for ds in (True, False):
        m, eng = _engine(dev, deep_supervision=ds, graph=False)
        before = {n: p.detach().clone() for n, p in m.named_parameters() if n.startswith("decoder.ds.")}
        assert len(before) == 4
        losses = [eng.train_step(batch).item() for _ in range(3)]
        assert all(np.isfinite(losses))
        for n, p in m.named_parameters():
            if n in before:
                assert (not torch.equal(p.detach(), before[n])) == ds, n
        if ds:
            terms = eng.loss_fn.last_terms.tolist()
            assert abs(sum(w * t for w, t in zip([4 / 7, 2 / 7, 1 / 7], terms)) - losses[-1]) < 1e-5


def test_engine_graph_replay_equals_eager_bit_for_bit():
    """graph=True (capture after GRAPH_WARMUP eager steps, then replays) against graph=False: the loss has no atomics left, so losses
    and parameters agree bit for bit."""
    from training.engine import TrainEngine
    dev = _dev()
    batch = _batch()
    runs = []
    for graph in (False, True):
        m, eng = _engine(dev, deep_supervision=True, graph=graph)
        losses = [eng.train_step(batch) for _ in range(TrainEngine.GRAPH_WARMUP + 3)]
        torch.cuda.synchronize()
        if graph:
            assert eng.graph_mode and len(eng._graphs) == 1, "the step was not replayed from a graph"
        runs.append(([l.item() for l in losses], {n: p.detach().clone() for n, p in m.named_parameters()}))
    assert runs[0][0] == runs[1][0]
    for n, p in runs[0][1].items():
        assert torch.equal(p, runs[1][1][n]), n


def test_engine_without_deep_supervision_is_unchanged():
    """deep_supervision=False is the engine as it was: the same losses, bit for bit, as an engine built without the keyword."""
    dev = _dev()
    batch = _batch()
    runs = []
    for kw in ({}, {"deep_supervision": False}):
        m, eng = _engine(dev, graph=False, **kw)
        assert not hasattr(eng.loss_fn, "last_terms"), "the loss is not wrapped"
        runs.append([eng.train_step(batch).item() for _ in range(3)])
    assert runs[0] == runs[1]
