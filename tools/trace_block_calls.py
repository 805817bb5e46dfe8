"""Record what the block functions of mia_hip/ops.py ask of the library, to compare two commits of ops.py / norm.hip.

    python tools/trace_block_calls.py --out DIR          one commit: DIR/trace.txt and DIR/tensors.pt (needs a GPU)
    python tools/trace_block_calls.py --compare A B      two such directories: exit status 0 only if they agree

`ops.call` is replaced by a recorder (and `ops._p` by a wrapper that remembers which tensor an address belongs to); every case runs
forward + backward.  trace.txt gets one line per library call -- the name, every non-pointer argument, and for a pointer null / ptr
plus the shape and dtype of its tensor where known -- and per case the caching allocator's allocation count.  tensors.pt gets each
case's logits, loss, parameter gradients and input gradient.  The file reaches into nothing else of ops, so the same file runs on
either commit: copy it into the other checkout.  The cases are listed in CASES below; each reaches a different branch of the norm
backward plumbing."""
import argparse
import ctypes
import hashlib
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _d in (ROOT, os.path.join(ROOT, "medical-image-analysis_amd")):
    if _d not in sys.path:
        sys.path.insert(0, _d)


class Recorder:
    def __init__(self, ops):
        self.ops, self.raw_call, self.raw_p, self.lines, self.known, self.ncalls = ops, ops.call, ops._p, [], {}, 0

    def __enter__(self):
        def p(t):
            if t is not None:
                self.known[t.data_ptr()] = "%s,%s" % (list(t.shape), str(t.dtype).replace("torch.", ""))
            return self.raw_p(t)

        def call(name, *args):
            self.lines.append(name + " " + " ".join(self.fmt(a) for a in args))
            self.known.clear()
            self.ncalls += 1
            return self.raw_call(name, *args)

        self.ops.call, self.ops._p = call, p
        return self

    def __exit__(self, *exc):
        self.ops.call, self.ops._p = self.raw_call, self.raw_p

    def fmt(self, a):
        if a is None:
            return "null"
        if isinstance(a, ctypes.c_void_p):
            return "null" if not a.value else "ptr[%s]" % self.known.get(a.value, "?")
        if isinstance(a, (bool, int, float)):
            return repr(a)
        if isinstance(a, ctypes._SimpleCData):
            return "%s:%r" % (type(a).__name__, a.value)
        return type(a).__name__  # byref(...)


def _allocs():
    torch.cuda.synchronize()
    return torch.cuda.memory_stats()["allocation.all.allocated"]


def _keep(t, limit=1 << 22):
    """A large tensor is kept as the SHA-256 of its bytes (bit-equality is all that is asked of it)."""
    if t.numel() * t.element_size() <= limit:
        return t
    return torch.frombuffer(bytearray(hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).digest()), dtype=torch.uint8)


def _loss_fn():
    from losses.compound_losses import DiceAndCELoss
    from losses.dice_loss import DiceLoss
    return DiceAndCELoss(dice_loss=DiceLoss, dice_kwargs=dict(num_classes=2, do_bg=True), ce_loss=torch.nn.CrossEntropyLoss, ce_kwargs={})


def _data(shape, classes=3, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g), torch.randint(0, classes, (shape[0],) + tuple(shape[2:]), generator=g)


def _unet(dev, channels, dtype=torch.float32, train=True, **kw):
    from models.unet import UNet
    torch.manual_seed(1337)
    m = UNet(2, 1, 3, channels, **kw).to(dev)
    m.set_compute_dtype(dtype)
    return m.train() if train else m.eval()


def _model_case(dev, out, model, shape, x_grad=False, return_ds=False):
    x, y = _data(shape)
    x = x.to(dev).requires_grad_(x_grad)
    if return_ds:  # the auxiliary logits stay at their own resolution: the loss upsamples on the fly (torch's bilinear backward adds
        from losses.deep_supervision import DeepSupervisionLoss  # with atomics and is not reproducible from run to run)
        outs = model(x, return_ds=True, upsample_ds=False)
        loss = DeepSupervisionLoss(_loss_fn())(outs, y.to(dev))
    else:
        outs = [model(x)]
        loss = _loss_fn()(outs[0], y.to(dev))
    loss.backward()
    for i, o in enumerate(outs):
        out["logits%d" % i] = o
    out["loss"] = loss
    for k, p in model.named_parameters():
        out["grad." + k] = p.grad
    if x_grad:
        out["grad.input"] = x.grad


def case_a(dev, out, dtype=torch.bfloat16):
    """UNet, instance norm, 64-channel level 0: normalise-on-load pairs, head_w (c == 64), two-piece skip gradients."""
    _model_case(dev, out, _unet(dev, [64, 128], dtype, normalization="instance", dropout_prob=None), (2, 1, 64, 64))


def case_b(dev, out):
    """(a) in fp32: the amax outputs of the apply pass."""
    case_a(dev, out, torch.float32)


def case_c(dev, out):
    """PlainBlock 24 -> 24 at 2x24x17x19, stride 1 and 2, bf16 and fp32, dup=True: scalar reduce / apply kernels, explicit sum of the pieces."""
    from models.unet.blocks import PlainBlock
    for stride in (1, 2):
        for dtype in (torch.bfloat16, torch.float32):
            torch.manual_seed(1337)
            blk = PlainBlock(2, 24, 24, stride=stride).to(dev).train()
            g = torch.Generator().manual_seed(stride)
            x = torch.randn(2, 17, 19, 24, generator=g).to(dev, dtype).requires_grad_(True)
            z, skip = blk.forward_nhwc(x, dup=True)
            g1, g2 = (torch.randn(z.shape, generator=g).to(dev) for _ in range(2))
            loss = (z.float() * g1).sum() + (skip.float() * g2).sum()
            loss.backward()
            tag = "s%d.%s." % (stride, str(dtype).replace("torch.", ""))
            out[tag + "z"], out[tag + "loss"], out[tag + "grad.input"] = z, loss, x.grad
            for k, p in blk.named_parameters():
                out[tag + "grad." + k] = p.grad


def case_d(dev, out):
    """Batch norm: training; eval with an input that requires grad (fixed statistics); Dropout2d 0.2 (drop_scale)."""
    for tag, train, x_grad, drop in (("train.", True, False, None), ("eval.", False, True, None), ("drop.", True, False, 0.2)):
        sub = {}
        _model_case(dev, sub, _unet(dev, [16, 32, 64], train=train, normalization="batch", dropout_prob=drop), (2, 1, 64, 64), x_grad)
        out.update({tag + k: v for k, v in sub.items()})


def case_e(dev, out):
    """Residual blocks + deep supervision at 2x1x32x32: PointwiseNormFn stride 1 and 2, ScaleLReLUFn with and without a mask."""
    for tag, drop in (("nomask.", None), ("mask.", 0.2)):
        sub = {}
        m = _unet(dev, [8, 16, 32], block_type="res", norm_key="instance", dropout_prob=drop, deep_supervision=True, ds_layer=2)
        _model_case(dev, sub, m, (2, 1, 32, 32), return_ds=True)
        out.update({tag + k: v for k, v in sub.items()})


def case_f(dev, out):
    """mia_norm_act_bwd directly, n=17, hw=256*256, c=32, bf16, slabs=64: n * slabs > 1024, the separate sum launch."""
    from mia_hip import BF16, NORM_INSTANCE, ops
    n, hw, c, slabs = 17, 256 * 256, 32, 64
    torch.manual_seed(7)
    y, dz = (torch.randn(n, hw, c, device=dev).bfloat16() for _ in range(2))
    co = torch.randn(5, n, c, device=dev)
    co[0] = co[0].abs() + 0.5
    dy = torch.empty_like(y)
    part = torch.empty((n, slabs, c, 2), device=dev)
    cc, dgb = torch.empty((2, n, c), device=dev), torch.empty((3, c), device=dev)
    p = ops._p
    ops.call("mia_norm_act_bwd", p(dz), None, p(y), p(dy), BF16, p(co[2]), p(co[3]), p(co[0]), p(co[1]), p(co[4]), n, ops._c_i64(hw), c,
             NORM_INSTANCE, 0, ops._c_float(0.01), slabs, p(part), p(cc[0]), p(cc[1]), p(dgb[0]), p(dgb[1]), p(dgb[2]), 0, None, ops._stream())
    out.update(dy=dy, cc=cc, dgb=dgb)


def _knob_case(knob):
    def run(dev, out):
        from mia_hip import ops
        old = getattr(ops, knob)
        setattr(ops, knob, False)
        try:
            case_a(dev, out)
        finally:
            setattr(ops, knob, old)
    run.__doc__ = "(a) with ops.%s off." % knob
    return run


def _engine(dev, graph, **kw):
    from training.engine import TrainEngine
    m = _unet(dev, [64, 128], torch.bfloat16, normalization="instance", dropout_prob=None)
    return TrainEngine(m, _loss_fn(), "adam", {"weight_decay": 5e-4}, start_lr=1e-2, num_iters=100, lr_warmup_iter=2, graph=graph, **kw)


def case_engine(dev, out):
    """TrainEngine on (a): 3 eager steps; with graph=True its GRAPH_WARMUP eager steps, then 3 replayed ones.  Losses and final parameters."""
    from training.engine import TrainEngine
    x, y = _data((2, 1, 64, 64))
    for tag, graph, steps in (("eager.", False, 3), ("graph.", True, TrainEngine.GRAPH_WARMUP + 3)):
        eng = _engine(dev, graph)
        out[tag + "losses"] = torch.stack([eng.train_step({"image": x, "label": y}).detach().float() for _ in range(steps)])
        out[tag + "params"] = eng.optimizer.flat_param
        assert bool(eng._graphs) == graph


def _sync_worker(rank, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=2)
    from mia_hip import ops
    from training.engine import TrainEngine
    dev = torch.device("cuda:0")
    m = _unet(dev, [8, 16, 32], normalization="batch", dropout_prob=None)
    eng = TrainEngine(m, _loss_fn(), "adam", {"weight_decay": 5e-4}, start_lr=1e-2, num_iters=100, lr_warmup_iter=2, bucket_bytes=4096,
                      sync_batchnorm=True)
    x, y = _data((4, 1, 32, 32), seed=42)
    lo = 2 * rank
    with Recorder(ops) as rec:
        a0 = _allocs()
        losses = [eng.train_step({"image": x[lo:lo + 2], "label": y[lo:lo + 2]}).item() for _ in range(2)]
        rec.lines.append("allocations %d" % (_allocs() - a0))
    q.put((rank, rec.lines, rec.ncalls, torch.tensor(losses), eng.optimizer.flat_param.cpu()))
    dist.barrier()
    dist.destroy_process_group()


def case_h(dev, out, lines):
    """Synchronised batch norm: two gloo ranks on the one GPU, two TrainEngine steps each (the setup of tests/test_gpu_dp.py)."""
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sync_worker, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
    ncalls = 0
    for rank, rlines, n, losses, params in res:
        lines += ["rank%d %s" % (rank, l) for l in rlines]
        out["rank%d.losses" % rank], out["rank%d.params" % rank] = losses, params
        ncalls += n
    return ncalls


CASES = dict(a=case_a, b=case_b, c=case_c, d=case_d, e=case_e, f=case_f, engine=case_engine,
             **{"g." + k: _knob_case(k) for k in ("FUSE_HEAD_W", "FUSE_STEM_BWD", "FUSE_NL", "FUSE_ACC")})


def run(outdir, names):
    from mia_hip import ops
    dev = torch.device("cuda:0")
    os.makedirs(outdir, exist_ok=True)
    lines, tensors, ncalls = [], {}, 0
    for name in names:
        out = {}
        if name == "h":
            lines.append("# case h: " + case_h.__doc__)
            ncalls += case_h(dev, out, lines)
        else:
            lines.append("# case %s: %s" % (name, CASES[name].__doc__))
            torch.manual_seed(1337)
            ops.clear_hints()
            with Recorder(ops) as rec:
                a0 = _allocs()
                CASES[name](dev, out)
                rec.lines.append("allocations %d" % (_allocs() - a0))
            lines += rec.lines
            ncalls += rec.ncalls
        tensors.update({"%s/%s" % (name, k): _keep(v.detach().cpu()) for k, v in out.items() if v is not None})
        print("case %s: %d tensors" % (name, len(out)), flush=True)
    with open(os.path.join(outdir, "trace.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    torch.save(tensors, os.path.join(outdir, "tensors.pt"))
    print("%d calls in %d cases, %d tensors -> %s" % (ncalls, len(names), len(tensors), outdir))


def compare(a, b):
    la, lb = (open(os.path.join(d, "trace.txt")).read().splitlines() for d in (a, b))
    diff = [i for i, (x, y) in enumerate(zip(la, lb)) if x != y]
    ncalls = sum(1 for l in la if not l.startswith(("#", "allocations")) and not l.split(" ", 1)[-1].startswith("allocations"))
    ncases = sum(1 for l in la if l.startswith("# case"))
    ok = not diff and len(la) == len(lb)
    print("traces equal: %d calls in %d cases" % (ncalls, ncases) if ok else "traces DIFFER: %d vs %d lines, first at line %s" % (len(la), len(lb), diff[:1]))
    for i in diff[:5]:
        print("  A:", la[i][:300], "\n  B:", lb[i][:300])
    ta, tb = (torch.load(os.path.join(d, "tensors.pt")) for d in (a, b))
    bad = sorted(set(ta) ^ set(tb))
    for k in sorted(set(ta) & set(tb)):
        x, y = ta[k], tb[k]
        if x.shape != y.shape or x.dtype != y.dtype or not (torch.equal(x, y) or torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))):
            bad.append(k)
    print("tensors bit-equal: %d of %d" % (len(set(ta) | set(tb)) - len(bad), len(set(ta) | set(tb))))
    for case in sorted({k.split("/")[0] for k in bad}):
        ks = [k for k in bad if k.split("/")[0] == case]
        print("  differs in case %s: %d tensors, e.g. %s" % (case, len(ks), ", ".join(ks[:4])))
    return 0 if ok and not bad else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out")
    ap.add_argument("--cases", default=",".join(list(CASES) + ["h"]))
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    sys.exit(compare(*args.compare) if args.compare else run(args.out, args.cases.split(",")))
