"""GPU checks of the pyramid consistency loss (csrc/urpc.hip: URPC between the S outputs a network makes at several scales, bilinear
upsampling in registers) against the float64 restatement in tests/_urpc_ref.py, called through the C ABI, then at op and engine
level.  Inputs are seeded and exactly representable in fp32; every output buffer (the gaps of padded layouts and the rows around a
batch slice included) starts as NaN, the gaps must still be NaN afterwards and every element a kernel owns finite.  The inputs' gaps
are NaN too: a read outside a tensor poisons the result.

Launch -> branch -> case (test[parameters]):
  mia_urpc_fwd
    urpc_fwd_kernel<K1, S>, K1 = 2, 3, 4 and <8, S> with run-time k1 = 1, 5, 8; S = 2, 3, 5
      factor sets (1,2) (1,16) (1,4,16) (1,2,4,8,16) (1,8,2) x coarse (1,1) (1,5) (3,3) (5,7): clamped taps ... test_urpc_shapes[*]
      one, two, three slabs of rows, the last ragged ........................................... test_urpc_shapes[*] (slabs rotate)
      more slabs than rows (two rows on five slabs: three empty blocks) ......................... test_urpc_more_slabs_than_rows
      S = 4, every class count, several gather tiles per scale .................................. test_urpc_shapes[*-(1, 2, 4, 8)-3]
      z_s channels-last / NCHW / padded, rotating per scale; a batch slice of a larger tensor .... test_urpc_shapes (every fifth: slices)
    urpc_finalize_kernel: dyn NULL and dyn = {0.37, .} ......................................... test_urpc_shapes (alternating)
    one class: L = 0 exactly .................................................................. test_urpc_shapes[*] with k1 = 1
  mia_urpc_bwd
    urpc_bwd_full_kernel<K1, S> (f = 1), dz_0 in its own layout ................................ test_urpc_shapes[*]
    urpc_bwd_gather_kernel<K1, S> per f > 1: tile larger than the image; ragged last tiles; tiles shrunk to the LDS budget at
      factor 16; the written scale swapped into slot 0, factors out of order ................... test_urpc_shapes[*]
    grad_out NULL and a device scalar; dz_s layouts independent of z_s ......................... test_urpc_shapes (rotating)
    one class: every dz exactly 0 ............................................................. test_urpc_shapes[*] with k1 = 1
  saturated logits (|z| <= 20, and K = 2 with |z| <= 200) ...................................... test_urpc_saturation
  two calls, bit-identical out / sums / terms / dz ............................................. test_urpc_deterministic
  ops.PyramidConsistencyFn against PyramidConsistencyLoss(fused=False) ......................... test_op_matches_the_composition
  batch slices of full-batch tensors: the labelled rows of every .grad are exactly 0 ........... test_op_on_batch_slices
  training.semi.URPCEngine ..................................................................... test_engine_*

Tolerances (the rules of tests/test_gpu_head_loss.py / test_gpu_ds_loss.py; relerr = max |error| / max |reference|, float64): loss
scalars (out, terms) absolutely 2e-6; sums per column and every dz relerr < 2e-5.  Model level: parameter gradients relerr 1e-4.
Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import _urpc_ref as R
import test_gpu_head_loss as HL
import test_gpu_norm as G

pytestmark = pytest.mark.gpu

TOL32, LOSS_ATOL, GRAD_TOL = G.TOL32, 2e-6, 1e-4
_dev, _abi, rel = G._dev, G._abi, G.rel
Buf, nan_f32 = HL.Buf, HL.nan_f32
_id = lambda k: "-".join(str(x) for x in k)


class SlicedBuf(Buf):
    """A Buf of n + 2 images whose `view` is the n in the middle: what `output[lb:]` hands the kernels.  The rows around the slice
    stay NaN, so `check_written` also proves that nothing outside the slice was written (or, for an input, read)."""

    def __init__(self, shape, layout, dev, values=None):
        n, p, k = shape
        super().__init__((n + 2, p, k), layout, dev)
        self.view = self.view[1:n + 1]
        if values is not None:
            self.view.copy_(values.float())


def _buf(sliced, shape, layout, dev, values=None):
    return (SlicedBuf if sliced else Buf)(shape, layout, dev, values=values)


def run_urpc(zs, factors, dev, *, slabs=1, layouts=None, dz_layouts=None, weight=None, gout=None, sliced=False):
    """mia_urpc_fwd, then mia_urpc_bwd.  zs: float64 (fp32-exact) [N, h_s, w_s, K] per scale."""
    mia_hip, ops = _abi()
    _p = ops._p
    ns = len(zs)
    nb, hh, ww, k1 = zs[0].shape
    layouts = layouts or ["cl"] * ns
    dz_layouts = dz_layouts or layouts
    zb = [_buf(sliced, (nb, z.shape[1] * z.shape[2], k1), lay, dev, torch.from_numpy(z).reshape(nb, -1, k1)) for z, lay in zip(zs, layouts)]
    dzb = [_buf(sliced, (nb, z.shape[1] * z.shape[2], k1), lay, dev) for z, lay in zip(zs, dz_layouts)]
    strides = lambda bufs: [(b.sn, b.sk, b.sp) for b in bufs]
    zp, zst = ops._host_arrays([b.view for b in zb], strides(zb))
    dp, dst = ops._host_arrays([b.view for b in dzb], strides(dzb))
    fac = (ops.ctypes.c_int * ns)(*factors)
    ws = nan_f32((mia_hip.lib().mia_urpc_workspace(nb, ns, slabs),), dev)
    sums, terms, out = nan_f32((ns, 3), dev), nan_f32((ns,), dev), nan_f32((2,), dev)
    dyn = None if weight is None else torch.tensor([weight, float("nan")], dtype=torch.float32, device=dev)
    gd = None if gout is None else torch.tensor([gout], dtype=torch.float32, device=dev)
    mia_hip.call("mia_urpc_fwd", zp, fac, zst, ns, nb, hh, ww, k1, _p(dyn), slabs, _p(ws), _p(sums), _p(terms), _p(out), ops._stream())
    mia_hip.call("mia_urpc_bwd", zp, fac, zst, dp, dst, ns, nb, hh, ww, k1, _p(sums), _p(dyn), _p(gd), ops._stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ws).all()), "a slab partial was never written"
    return dict(sums=sums, terms=terms, out=out, dz=dzb)


def figures(got, ref):
    f = {"out": np.abs(got["out"].double().cpu().numpy() - ref["out"]).max(),
         "terms": np.abs(got["terms"].double().cpu().numpy() - ref["terms"]).max()}
    for j, name in enumerate(("A", "B", "C")):
        top = np.abs(ref["sums"][:, j]).max()
        f[name] = np.abs(got["sums"][:, j].double().cpu().numpy() - ref["sums"][:, j]).max() / top if top > 0 else 0.0
    for s, (dz, want) in enumerate(zip(got["dz"], ref["dz"])):
        want = want.reshape(dz.view.shape)
        top = np.abs(want).max()
        f[f"dz{s}"] = np.abs(dz.view.double().cpu().numpy() - want).max() / top if top > 0 else 0.0
    return f


def check_urpc(got, ref, what="", loss_atol=LOSS_ATOL):
    """Each figure is printed before it is asserted."""
    for dz in got["dz"]:
        dz.check_written()
    f = figures(got, ref)
    print(f"urpc {what}: " + " ".join(f"{k}={v:.3e}" for k, v in f.items()))
    for k in ("out", "terms", "sums"):
        assert bool(torch.isfinite(got[k]).all()), k
    assert f["out"] < loss_atol and f["terms"] < loss_atol
    assert f["A"] < TOL32 and f["B"] < TOL32 and f["C"] < TOL32
    for s in range(len(got["dz"])):
        assert f[f"dz{s}"] < TOL32, s
    return f


# ================================================================== kernel level
@pytest.mark.parametrize("i,case", list(enumerate(R.shape_cases())), ids=lambda v: _id(v) if isinstance(v, tuple) else f"c{v}")
def test_urpc_shapes(i, case):
    """Every factor set on the shapes at which a tap clamps, a tile or a slab is ragged or empty and more than one tile and slab are at
    work, for every class count of both routes.  Layouts of z_s and dz_s rotate independently per scale; every fifth case hands the
    kernels batch slices; dyn and the upstream gradient alternate between NULL and a device value."""
    dev = _dev()
    nb, k1, ch, cw, factors, slabs = case
    weight = None if i % 2 else R.DYN_WEIGHT
    gout = None if i % 3 else R.GOUT
    zs, ref = R.reference(R.key(nb, k1, ch, cw, factors, weight, gout))
    lay = [R.LAYOUTS[(i + s) % 3] for s in range(len(factors))]
    dlay = [R.LAYOUTS[(i // 3 + 2 * s) % 3] for s in range(len(factors))]
    got = run_urpc(zs, factors, dev, slabs=slabs, layouts=lay, dz_layouts=dlay, weight=weight, gout=gout, sliced=i % 5 == 4)
    check_urpc(got, ref, _id(case))
    if k1 == 1:  # softmax = 1 = m at every scale: every term cancels exactly
        assert got["out"].tolist() == [0.0, 0.0] and not got["terms"].any()
        assert all(not dz.view.any() for dz in got["dz"]), "the gradient of a one-class loss is exactly 0"


@pytest.mark.parametrize("k1", [3, 8])
def test_urpc_more_slabs_than_rows(k1):
    """One coarse pixel at factor 2 is two full-resolution rows; on five slabs three blocks own no row and write zeros."""
    dev = _dev()
    zs, ref = R.reference(R.key(3, k1, 1, 1, (1, 2)))
    check_urpc(run_urpc(zs, (1, 2), dev, slabs=5), ref, f"five slabs k1={k1}")


@pytest.mark.parametrize("k1,factors,amp", [(3, (1, 4, 16), 20.0), (2, (1, 2, 8), 200.0)], ids=["k3-20", "k2-200"])
def test_urpc_saturation(k1, factors, amp):
    """Logits on [-amp, amp]: soft-max outputs round to 0 and 1 in fp32 (at 200 also m_k = 0 and w_s = 0), the scales disagree at most
    pixels.  log p is u - logsumexp(u) and p dv/dp = -m is formed without a division, so the loss and every dz stay finite and
    within the rules.
    Measured on an MI355X: at 20, L = 4.78, loss error 9.6e-8, dz relerr <= 3.4e-7; at 200, L = 36.80, loss error 1.37e-6 (fp32 numbers
    are 3.8e-6 apart there, so rounding L alone can cost 1.9e-6; the sums arrive in double), dz relerr <= 1.5e-6.  The fused=False
    fp32 path on the same inputs: 9.6e-8 and 5.2e-6."""
    dev = _dev()
    zs, ref = R.reference(R.key(3, k1, 2, 3, factors, R.DYN_WEIGHT, R.GOUT, amp=amp))
    got = run_urpc(zs, factors, dev, slabs=2, weight=R.DYN_WEIGHT, gout=R.GOUT)
    check_urpc(got, ref, f"saturation k1={k1} amp={amp} L={ref['out'][1]:.4f}")


@pytest.mark.parametrize("k1,factors", [(3, (1, 2)), (2, (1, 4, 16)), (8, (1, 2, 4, 8, 16)), (4, (1, 8, 2))], ids=str)
def test_urpc_deterministic(k1, factors):
    """No atomics, fixed accumulation order: two calls on the same inputs agree bit for bit."""
    dev = _dev()
    zs, _ = R.reference(R.key(3, k1, 3, 3, factors))
    a, b = (run_urpc(zs, factors, dev, slabs=3, dz_layouts=["nchw"] * len(factors)) for _ in range(2))
    for k in ("out", "sums", "terms"):
        assert torch.equal(a[k], b[k]), k
    for x, y in zip(a["dz"], b["dz"]):
        assert torch.equal(x.view, y.view)


# ================================================================== op level
def _leaves(zs, dev, extra_rows=0):
    """Channels-last storage like the heads' outputs, logical [N, K, h, w]; extra_rows images of zeros in front."""
    out = []
    for z in zs:
        t = torch.from_numpy(z).float()
        if extra_rows:
            t = torch.cat([torch.zeros(extra_rows, *t.shape[1:]), t])
        out.append(t.to(dev).contiguous().permute(0, 3, 1, 2).requires_grad_(True))
    return out


@pytest.mark.parametrize("k1,factors", [(3, (1, 2, 4)), (2, (1, 16)), (5, (1, 8, 2)), (4, (1, 2, 4, 8, 16))], ids=str)
def test_op_matches_the_composition(k1, factors):
    """ops.PyramidConsistencyFn (through PyramidConsistencyLoss) against fused=False, the tensor-op form of the definition, on the same
    tensors: both within 2e-6 of the float64 loss, the fused dz within the rule, the two gradients within the rule of each other."""
    from losses.pyramid_consistency import PyramidConsistencyLoss
    dev = _dev()
    zs, ref = R.reference(R.key(3, k1, 3, 5, factors, R.DYN_WEIGHT, None))
    dyn = torch.tensor([R.DYN_WEIGHT, 0.0], dtype=torch.float32, device=dev)
    res = {}
    for fused in (True, False):
        leaves = _leaves(zs, dev)
        loss_fn = PyramidConsistencyLoss(fused=fused)
        loss = loss_fn(leaves, dyn=dyn)
        loss.backward()
        assert tuple(loss_fn.last_terms.shape) == (len(factors),) and loss_fn.last_terms.is_cuda and loss_fn.last_value.is_cuda
        res[fused] = (loss.item(), loss_fn.last_value.item(), loss_fn.last_terms.double().cpu().numpy(), [l.grad for l in leaves])
    want = [torch.from_numpy(dz).permute(0, 3, 1, 2) for dz in ref["dz"]]
    figs = {"fused": abs(res[True][0] - ref["out"][0]), "composed": abs(res[False][0] - ref["out"][0]),
            "fused_terms": np.abs(res[True][2] - ref["terms"]).max()}
    for s in range(len(factors)):
        figs[f"dz{s}"] = rel(res[True][3][s], want[s])
        figs[f"dz{s}_composed"] = rel(res[False][3][s], want[s])
    print(f"op k1={k1} {factors}: " + " ".join(f"{k}={v:.3e}" for k, v in figs.items()))
    assert figs["fused"] < LOSS_ATOL and figs["composed"] < LOSS_ATOL and figs["fused_terms"] < LOSS_ATOL
    assert abs(res[True][1] - ref["out"][1]) < LOSS_ATOL
    for s in range(len(factors)):
        assert figs[f"dz{s}"] < TOL32 and rel(res[True][3][s], res[False][3][s]) < TOL32


def test_op_on_batch_slices():
    """The engine's call: `[o[lb:] for o in outs]` of full-batch tensors.  Loss and the unlabelled rows' gradients are those of the
    unsliced call; the labelled rows of every .grad are exactly 0."""
    from losses.pyramid_consistency import PyramidConsistencyLoss
    dev = _dev()
    factors, lb = (1, 2, 4), 2
    zs, ref = R.reference(R.key(3, 3, 3, 5, factors, None, None))
    leaves = _leaves(zs, dev, extra_rows=lb)
    loss = PyramidConsistencyLoss(fused=True)([l[lb:] for l in leaves])
    loss.backward()
    print(f"slices: loss {loss.item():.7f} / {ref['out'][0]:.7f}")
    assert abs(loss.item() - ref["out"][0]) < LOSS_ATOL
    for leaf, dz in zip(leaves, ref["dz"]):
        assert not leaf.grad[:lb].any(), "a labelled image received a consistency gradient"
        assert rel(leaf.grad[lb:], torch.from_numpy(dz).permute(0, 3, 1, 2)) < TOL32


# ================================================================== engine
LB, B, HW = 2, 4, 32


def _engine(dev, **kw):
    from losses.compound_losses import DiceAndCELoss
    from models.unet import UNet
    from training.semi import URPCEngine
    torch.manual_seed(11)
    m = UNet(2, 1, 3, [4, 8, 16, 32], normalization="instance", dropout_prob=None, deep_supervision=True, ds_layer=3).to(dev)
    args = dict(labeled_bs=LB, consistency_weight=0.5, optimizer_kwargs={"weight_decay": 5e-4}, start_lr=1e-2, num_iters=100, lr_warmup_iter=0)
    args.update(kw)
    return m, URPCEngine(m, DiceAndCELoss(dice_kwargs=dict(num_classes=2, do_bg=True)), **args)


def _batch(seed, dev, images=B):
    g = torch.Generator().manual_seed(seed)
    return {"image": torch.rand(images, 1, HW, HW, generator=g).to(dev), "label": torch.randint(0, 3, (LB, HW, HW), generator=g).to(dev)}


def _grads(eng):
    opt = eng.optimizer
    names = {id(p): n for n, p in eng.model.named_parameters()}
    return {names[id(p)]: opt.flat_grad[o:o + p.numel()].clone() for p, o in zip(opt.params, opt.offsets)}


def test_engine_fused_step_matches_the_composed_step():
    """One step from the same initial state with the fused kernel and with fused=False: the loss within 2e-6, every parameter gradient
    within relerr 1e-4 (the model-level bound of test_gpu_ds_loss.py), and the auxiliary heads do receive one."""
    from losses.pyramid_consistency import PyramidConsistencyLoss
    dev = _dev()
    batch = _batch(0, dev)
    runs = []
    for fused in (True, False):
        _, eng = _engine(dev, consistency=PyramidConsistencyLoss(fused=fused))
        loss = eng.train_step(batch)
        assert eng.last_consistency.item() > 0 and tuple(eng.consistency.last_terms.shape) == (3,)
        runs.append((loss.item(), eng.last_consistency.item(), _grads(eng)))
    print(f"engine: loss fused {runs[0][0]:.7f} composed {runs[1][0]:.7f}; consistency {runs[0][1]:.7f} / {runs[1][1]:.7f}")
    assert abs(runs[0][0] - runs[1][0]) < LOSS_ATOL and abs(runs[0][1] - runs[1][1]) < LOSS_ATOL
    for n, g in runs[0][2].items():
        err = rel(g, runs[1][2][n])
        assert err < GRAD_TOL, (n, err)
    assert runs[0][2]["decoder.ds.0.0.weight"].abs().max().item() > 0 and runs[0][2]["decoder.ds.1.0.weight"].abs().max().item() > 0


def test_engine_weight_zero_is_the_supervised_step():
    """consistency_weight = 0: the loss and every parameter gradient equal those of the step that only supervises the labelled half
    (consistency=False) -- a zero weight leaves exact zeros, never a NaN, in the unlabelled images' gradients."""
    dev = _dev()
    batch = _batch(1, dev)
    _, with_term = _engine(dev, consistency_weight=0.0)
    _, without = _engine(dev, consistency=False)
    la, lb = with_term.train_step(batch), without.train_step(batch)
    assert with_term.last_consistency.item() > 0 and without.last_consistency is None
    assert torch.equal(la, lb)
    ga, gb = _grads(with_term), _grads(without)
    assert max(g.abs().max().item() for g in ga.values()) > 0
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


def test_engine_fully_labelled_batch_skips_the_term():
    dev = _dev()
    _, eng = _engine(dev)
    loss = eng.train_step(_batch(2, dev, images=LB))
    assert eng.last_consistency is None and torch.equal(loss, eng.last_supervised)


def test_engine_three_steps():
    dev = _dev()
    m, eng = _engine(dev, consistency_weight=type("Ramp", (), {"step": staticmethod(lambda i: 0.1 * (i + 1))})())
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    losses = [eng.train_step(_batch(i, dev)) for i in range(3)]
    assert all(l.is_cuda for l in losses) and bool(torch.isfinite(torch.stack(losses)).all())
    assert eng.last_consistency is not None and eng.last_consistency.is_cuda and torch.isfinite(eng.last_consistency).item()
    assert eng.dyn[0].item() == pytest.approx(0.3, rel=1e-6) and eng.current_iter == 3
    assert all(not torch.equal(p.detach(), before[n]) for n, p in m.named_parameters()), "a parameter never moved"
    assert np.isfinite(eng.loss_value(losses[-1]))
    pred = eng.predict(_batch(9, dev)["image"])
    assert tuple(pred.shape) == (B, HW, HW) and pred.dtype == torch.int64 and not m.training
