"""Tensor-level wrappers + autograd glue over libmia_hip.so.

PyTorch-ROCm is used only as a container (device memory, streams, autograd graph); every FLOP and
every byte moved on the hot path goes through the HIP kernels behind ``include/mia_hip.h``.
Activations are plain contiguous NHWC tensors ``[N, H, W, C]`` in fp32 or bf16.  There is no CPU
fallback: tensors must live on a HIP device and the shared object must be built.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Tuple

import torch

from . import (BF16, CONV_G1, CONV_G2S2, CONV_G3S1, CONV_G3S2, CONV_T2S2, CONV_T3S2, F32, LOSS_BATCH, LOSS_DO_BG,
               LOSS_DENSE, LOSS_SOFTMAX, LOSS_SQUARED, NORM_BATCH, NORM_INSTANCE, REGLOSS_BATCH, REGLOSS_DO_BG, REGLOSS_IGNORE,
               REGLOSS_INDEX, REGLOSS_TARGET_U8, SEGLOSS_BATCH, SEGLOSS_DO_BG, SEGLOSS_IGNORE,
               SEGLOSS_LABEL_U8, SEGLOSS_SOFTMAX, WGRAD_2S2, WGRAD_3S1, WGRAD_3S2, MiaError, call, lib)

LRELU_SLOPE = 0.01
_c_int, _c_float, _c_i64 = ctypes.c_int, ctypes.c_float, ctypes.c_int64


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(t_or_dtype) -> int:
    d = t_or_dtype.dtype if isinstance(t_or_dtype, torch.Tensor) else t_or_dtype
    if d == torch.float32:
        return F32
    if d == torch.bfloat16:
        return BF16
    raise MiaError(f"unsupported activation dtype {d} (fp32 or bf16)")


def _need_dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise MiaError("libmia_hip operates on HIP device tensors only (no CPU fallback); got a CPU tensor")


def _pad(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def _kb(dtype: int) -> int:
    return 32 if dtype == BF16 else 16


# ------------------------------------------------------------------ operand maxima (fp32 convs on the f16 matrix cores)
# The fp32 tile kernels multiply on the f16 matrix cores from two-part split operands (csrc/common.h SplitF16); each operand tensor is
# scaled by a power of two taken from its max |x|, which the kernels read from a 4-byte device slot.  A slot travels with its
# tensor as a Python attribute (`_mia_amax` = (slot, tensor version)): the forward conv, the weight gradient that contracts the same
# activation in backward, and the two consumers of one gradient tensor share one reduction.  An attribute cannot outlive its tensor
# (unlike a table keyed by address), and a version change (in-place edit) makes the next consumer measure again.
F32_SPLIT_MIN_MACS = int(__import__('os').environ.get('MIA_F32_SPLIT_MIN_MACS', str(1 << 26)))  # below this many multiply-adds the exact kernel is as fast as the reduction + split


class _SlotArena:
    """Zeroed 4-byte slots, carved from chunks that ONE launch zeroes (a slot per norm / activation pass and per measured tensor
    would otherwise cost a zeroing launch each).  A slot is a view of its chunk, so the chunk lives as long as any of its slots.
    A chunk started outside a stream capture is never used inside one and vice versa: the zeroing launch must be part of the
    graph that uses the slots, or replays would fold into the previous replay's maxima (still safe -- a larger maximum only
    costs precision -- but no longer the eager step's arithmetic)."""
    CHUNK = 128

    def __init__(self):
        self.chunk, self.used, self.capturing, self.device = None, 0, False, None

    def reset(self) -> None:
        self.chunk = None

    def take(self, device) -> torch.Tensor:
        cap = torch.cuda.is_current_stream_capturing()
        if self.chunk is None or self.used >= self.CHUNK or cap != self.capturing or device != self.device:
            self.chunk = torch.empty(self.CHUNK, device=device, dtype=torch.int32)
            call("mia_zero", _p(self.chunk), _c_i64(self.CHUNK * 4), _stream())
            self.used, self.capturing, self.device = 0, cap, device
        self.used += 1
        return self.chunk[self.used - 1:self.used]


_ARENA = _SlotArena()


def amax_arena_reset() -> None:
    """Start a fresh chunk at the next request (training/engine.py: at both ends of a graph capture)."""
    _ARENA.reset()


def amax_slot(t: torch.Tensor) -> torch.Tensor:
    """Device slot (int32[1]) with max |t| as an fp32 bit pattern; measured once per tensor version (`mia_amax`)."""
    hit = getattr(t, "_mia_amax", None)
    if hit is not None and hit[1] == t._version:
        return hit[0]
    slot = _ARENA.take(t.device)
    tc = t if t.is_contiguous() else t.contiguous()
    call("mia_amax", _p(tc), _c_i64(tc.numel()), _p(slot), 0, _stream())
    try:
        t._mia_amax = (slot, t._version)
    except (AttributeError, RuntimeError):
        pass
    return slot


def _amax_new(t: torch.Tensor) -> Optional[torch.Tensor]:
    """A fresh slot, attached to `t`, that the kernel about to WRITE t fills as a by-product (`amax_out` of the norm / activation
    passes): the convs that consume t then need no reduction pass of their own.  fp32 tensors only."""
    if t.dtype != torch.float32:
        return None
    slot = _ARENA.take(t.device)
    t._mia_amax = (slot, t._version)
    return slot


def _dup_view(z: torch.Tensor) -> torch.Tensor:
    """Second handle on z (PlainBlockFn dup=True) that carries the same maximum slot."""
    v = z.view(z.shape)
    h = getattr(z, "_mia_amax", None)
    if h is not None:
        v._mia_amax = (h[0], v._version)
    return v


def _split_descs(items, device):
    """Device table for mia_split_f16_batch: items = [(packed fp32 buffer, int32 destination of the same shape, maximum slot)]."""
    import ctypes as C

    class SDesc(C.Structure):
        _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("n", C.c_int64), ("amax", C.c_void_p)]

    assert C.sizeof(SDesc) == lib().mia_split_desc_bytes()
    arr = (SDesc * len(items))()
    for i, (buf, dst, slot) in enumerate(items):
        arr[i] = SDesc(buf.data_ptr(), dst.data_ptr(), buf.numel(), slot.data_ptr())
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


def _split_ok(x: torch.Tensor, macs: int) -> bool:
    return x.dtype == torch.float32 and macs >= F32_SPLIT_MIN_MACS


# ------------------------------------------------------------------ weight packing (cached per parameter version)
PARAM_EPOCH = 0


def bump_param_epoch() -> None:
    """Parameters were modified behind torch's back (the fused optimizer kernel writes the flat buffer directly and
    does not touch tensor version counters): invalidate every packed-weight cache."""
    global PARAM_EPOCH
    PARAM_EPOCH += 1


class PackCache:
    """Packed copies of one fp32 parameter, invalidated by the tensor's version counter or the global epoch."""

    def __init__(self):
        self._store = {}

    def get(self, w: torch.Tensor, dtype: int, n_from_d0: bool, kpad_mult: Optional[int] = None) -> Tuple[torch.Tensor, int, int]:
        key = (dtype, n_from_d0)
        ver = (w._version, w.data_ptr(), PARAM_EPOCH)
        hit = self._store.get(key)
        if hit is not None and hit[0] == ver:
            return hit[1], hit[2], hit[3]
        d0, d1 = w.shape[0], w.shape[1]
        taps = w.shape[2] * w.shape[3]
        nn, kk = (d0, d1) if n_from_d0 else (d1, d0)
        npad, kpad = _pad(nn, 64), _pad(kk, _kb(dtype))
        buf = hit[1] if hit is not None else \
            torch.empty((taps, npad, kpad), device=w.device, dtype=torch.bfloat16 if dtype == BF16 else torch.float32)
        wc = w.detach()
        if not wc.is_contiguous():
            wc = wc.contiguous()
        call("mia_pack_weight", _p(wc), _p(buf), dtype, d0, d1, taps, npad, kpad, int(n_from_d0), _stream())
        if dtype == F32:  # the split-f16 kernels scale the weights by their maximum (amax_slot docstring); slot rides on the packed buffer
            slot = getattr(buf, "_mia_amax", None)
            slot = slot[0] if slot is not None else torch.empty(1, device=w.device, dtype=torch.int32)
            call("mia_amax", _p(wc), _c_i64(wc.numel()), _p(slot), 1, _stream())
            buf._mia_amax = (slot, buf._version)
            # ... and the packed weights once more as (h | l) fp16 words of w * 2^e, so the split kernels do not split them per tile
            sp = getattr(buf, "_mia_split", None)
            if sp is None:
                sp = torch.empty(buf.shape, device=w.device, dtype=torch.int32)
                buf._mia_split = sp
                buf._mia_split_desc = _split_descs([(buf, sp, slot)], w.device)
            call("mia_split_f16_batch", _p(buf._mia_split_desc), 1, _stream())
        self._store[key] = (ver, buf, npad, kpad)
        return buf, npad, kpad


class PackPlan:
    """All packed copies a model's step needs, refreshed by ONE `mia_pack_weight_batch` launch after the optimizer has
    rewritten the parameters (instead of one launch per tensor and orientation on first use).  Built from the packs the
    first steps left in the parameters' PackCaches; the results are planted into each parameter's PackCache with the current version key, so a
    parameter changed behind the plan's back (load_state_dict, in-place edits) simply misses and re-packs itself."""

    def __init__(self, params, dtype: int):
        import ctypes as C
        ents = []
        for w in params:
            c = _caches.get(id(w))
            if c is None or c[0]() is not w or not w.is_cuda or not w.is_contiguous() or w.ndim != 4:
                continue
            for (dt, n_from_d0) in c[1]._store:
                if dt == dtype:
                    ents.append(((id(w), dt, n_from_d0), (w, c[1])))
        if not ents:
            raise MiaError("PackPlan: no packed weights were requested yet (run a step first)")

        class Desc(C.Structure):
            _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("d0", C.c_int), ("d1", C.c_int), ("taps", C.c_int),
                        ("npad", C.c_int), ("kpad", C.c_int), ("n_from_d0", C.c_int), ("brick_begin", C.c_int), ("bricks_x", C.c_int)]

        assert C.sizeof(Desc) == lib().mia_pack_desc_bytes()
        arr = (Desc * len(ents))()
        self.entries, self.dtype, bricks, self.max_taps = [], dtype, 0, 1
        for i, ((_, _, n_from_d0), (w, pc)) in enumerate(ents):
            key = (dtype, n_from_d0)
            _, buf, npad, kpad = pc._store[key]
            d0, d1, taps = w.shape[0], w.shape[1], w.shape[2] * w.shape[3]
            if d0 * d1 * taps * 4 >= 1 << 31:
                raise MiaError("PackPlan: a weight tensor of 2 GiB or more is outside the batched pack kernel's 32-bit offsets")
            pa, pb = (npad, kpad) if n_from_d0 else (kpad, npad)  # padded extents along D0 / D1
            ta, tb = (16, 64) if n_from_d0 else (64, 16)
            bx, by = -(-pb // tb), -(-pa // ta)
            arr[i] = Desc(w.data_ptr(), buf.data_ptr(), d0, d1, taps, npad, kpad, int(n_from_d0), bricks, bx)
            bricks += bx * by
            self.max_taps = max(self.max_taps, taps)
            self.entries.append((w, pc, key, buf, npad, kpad, w.data_ptr()))
        self.total_bricks = bricks
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self.descs = host.to(self.entries[0][0].device)
        self.amax_descs = None
        if dtype == F32:  # maxima of every packed parameter in one launch; slot i rides on entry i's packed buffer
            class ADesc(C.Structure):
                _fields_ = [("src", C.c_void_p), ("n", C.c_int64)]

            assert C.sizeof(ADesc) == lib().mia_amax_desc_bytes()
            aarr = (ADesc * len(self.entries))()
            for i, (w, *_rest) in enumerate(self.entries):
                aarr[i] = ADesc(w.data_ptr(), w.numel())
            self.amax_descs = torch.frombuffer(bytearray(bytes(aarr)), dtype=torch.uint8).to(self.entries[0][0].device)
            self.amax_slots = torch.zeros(len(self.entries), device=self.entries[0][0].device, dtype=torch.int32)
            self.split_bufs = [getattr(e[3], "_mia_split", None) for e in self.entries]
            for i, e in enumerate(self.entries):
                if self.split_bufs[i] is None:
                    self.split_bufs[i] = torch.empty(e[3].shape, device=e[3].device, dtype=torch.int32)
            self.split_descs = _split_descs([(e[3], self.split_bufs[i], self.amax_slots[i:i + 1]) for i, e in enumerate(self.entries)],
                                            self.entries[0][0].device)
            # entry i's descriptor alone, for PackCache.get's per-tensor path: it must name the slot `plant` hangs on the buffer
            self.entry_split_descs = list(self.split_descs.split(lib().mia_split_desc_bytes()))

    def valid(self) -> bool:
        return all(w.data_ptr() == ptr for w, _, _, _, _, _, ptr in self.entries)

    def repack(self) -> None:
        call("mia_pack_weight_batch", _p(self.descs), len(self.entries), self.total_bricks, self.max_taps, self.dtype, _stream())
        if self.amax_descs is not None:
            call("mia_amax_batch", _p(self.amax_descs), len(self.entries), _p(self.amax_slots), _stream())
            call("mia_split_f16_batch", _p(self.split_descs), len(self.entries), _stream())
        self.plant()

    def plant(self) -> None:
        """Mark the plan's packed copies as current (host bookkeeping only): after `repack`, and after a graph replay whose
        captured re-pack launch rewrote them while the host-side keys stayed where the capture left them."""
        for i, (w, pc, key, buf, npad, kpad, _) in enumerate(self.entries):
            pc._store[key] = ((w._version, w.data_ptr(), PARAM_EPOCH), buf, npad, kpad)
            if self.amax_descs is not None:
                buf._mia_amax = (self.amax_slots[i:i + 1], buf._version)
                buf._mia_split = self.split_bufs[i]
                # a later per-tensor re-pack (another optimizer moved the epoch on) scales by THIS slot: the descriptor made with the
                # buffer's first slot would point at memory that slot no longer owns
                buf._mia_split_desc = self.entry_split_descs[i]


_caches = {}


def pack_cache(w: torch.Tensor) -> PackCache:
    c = _caches.get(id(w))
    if c is None or c[0]() is not w:
        import weakref
        pc = PackCache()
        _caches[id(w)] = (weakref.ref(w, lambda _r, k=id(w): _caches.pop(k, None)), pc)
        return pc
    return c[1]


# ------------------------------------------------------------------ layout helpers
def to_nhwc(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Logical NCHW tensor (any dense strides) -> contiguous NHWC tensor in `dtype` (HIP relayout kernel)."""
    _need_dev(x)
    n, c, h, w = x.shape
    if x.dtype not in (torch.float32, torch.bfloat16):
        x = x.float()
    sn, sc, sh, sw = x.stride()
    if x.dtype == dtype:
        if c == 1 and sw == 1 and (h == 1 or sh == w) and (n == 1 or sn == h * w):
            return x.reshape(n, h, w, 1)  # NCHW with C=1 is already NHWC
        if sc == 1 and sw == c and (h == 1 or sh == w * c) and (n == 1 or sn == h * w * c):
            return x.permute(0, 2, 3, 1)  # channels_last storage: zero-copy
    if x.requires_grad and torch.is_grad_enabled():
        return _RelayoutFn.apply(x, dtype)  # the image itself wants a gradient (VAT, saliency): keep the graph through the kernel
    if h > 1 and sh != w * sw:
        x = x.contiguous()
        sn, sc, sh, sw = x.stride()
    out = torch.empty((n, h, w, c), device=x.device, dtype=dtype)
    call("mia_relayout", _p(x), _dt(x), _p(out), _dt(out), n, c, _c_i64(h * w), _c_i64(sn), _c_i64(sc), _c_i64(sw),
         _c_i64(h * w * c), _c_i64(1), _c_i64(c), _stream())
    return out


class _RelayoutFn(torch.autograd.Function):
    """`to_nhwc` through `mia_relayout` for an input that requires a gradient; the backward is the same kernel in the opposite
    direction, back to the image's layout (its strides where H and W collapse, contiguous NCHW otherwise) and dtype."""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.save_for_backward(x)  # for its shape, strides and dtype
        return to_nhwc(x.detach(), dtype)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        n, c, h, w = x.shape
        g = g.contiguous()
        dx = torch.empty_like(x)  # x's strides where x is dense, contiguous otherwise
        sn, sc, sh, sw = dx.stride()
        if h > 1 and sh != w * sw:
            dx = torch.empty(x.shape, device=x.device, dtype=x.dtype)
            sn, sc, sh, sw = dx.stride()
        call("mia_relayout", _p(g), _dt(g), _p(dx), _dt(dx), n, c, _c_i64(h * w), _c_i64(h * w * c), _c_i64(1), _c_i64(c),
             _c_i64(sn), _c_i64(sc), _c_i64(sw), _stream())
        return dx, None


def nhwc_as_nchw(x: torch.Tensor) -> torch.Tensor:
    """Zero-copy logical-NCHW view (channels_last strides) of a contiguous NHWC tensor."""
    return x.permute(0, 3, 1, 2)


def cast_nhwc(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    if x.dtype == dtype:
        return x
    n, h, w, c = x.shape
    out = torch.empty_like(x, dtype=dtype)
    call("mia_relayout", _p(x), _dt(x), _p(out), _dt(out), n, c, _c_i64(h * w), _c_i64(h * w * c), _c_i64(1), _c_i64(c),
         _c_i64(h * w * c), _c_i64(1), _c_i64(c), _stream())
    return out


# ------------------------------------------------------------------ raw op wrappers
class LaunchProbe:
    """Brackets matching conv_mma launches with HIP events on the launch stream (bench.py roofline leg)."""

    def __init__(self, match):
        self.match, self.pairs, self.enabled = match, [], False

    def times_ms(self, tag=None):
        """Durations of the bracketed launches (all, or those whose match() returned `tag`)."""
        torch.cuda.synchronize()
        return [p[0].elapsed_time(p[1]) for p in self.pairs if tag is None or p[2] == tag]

    def records(self):
        """(duration_ms, tag, (mode, c1 + c2, nout, n, hout, wout)) per bracketed launch."""
        torch.cuda.synchronize()
        return [(p[0].elapsed_time(p[1]), p[2], p[3]) for p in self.pairs]


PROBE: Optional[LaunchProbe] = None


def conv_tiles(mode: int, hout: int, wout: int) -> int:
    ty, tx, th = _c_int(), _c_int(), _c_int()
    call("mia_conv_mma_tiles", mode, hout, wout, ctypes.byref(ty), ctypes.byref(tx), ctypes.byref(th))
    return ty.value * tx.value


def conv_mma(mode: int, x1: torch.Tensor, x2: Optional[torch.Tensor], wpack: torch.Tensor, npad: int, kpad: int,
             flip: bool, bias: Optional[torch.Tensor], nout: int, out_hw: Tuple[int, int], want_stats: bool = False,
             out_split: Optional[int] = None, nl=None, cr=None):
    """nl = (coefs [5, N, C] of the producing block, slope): x1 is that block's RAW conv output and the kernel normalises on
    load (`mia_conv_mma_nl`; the fused PlainBlock).  cr = (y_prod, coefs, slope): this launch is the input gradient that
    produces dz for the block with raw output `y_prod`, and its epilogue does that block's norm-backward reduction
    (`mia_conv_mma_cr`); the third return value is then the partials tensor [N, tiles, nout, 2]."""
    n, hin, win, c1 = x1.shape
    c2 = 0 if x2 is None else x2.shape[3]
    hout, wout = out_hw
    if out_split is None:
        out1 = torch.empty((n, hout, wout, nout), device=x1.device, dtype=x1.dtype)
        out2, o1, o2 = None, nout, 0
    else:
        o1, o2 = out_split, nout - out_split
        out1 = torch.empty((n, hout, wout, o1), device=x1.device, dtype=x1.dtype)
        out2 = torch.empty((n, hout, wout, o2), device=x1.device, dtype=x1.dtype)
    stats = None
    if want_stats or cr is not None:
        stats = torch.empty((n, conv_tiles(mode, hout, wout), nout, 2), device=x1.device, dtype=torch.float32)
    # fp32: operand maxima for the split-f16 products (None -> the library runs its exact fp32 kernels)
    am1 = am2 = amw = wsp = None
    if cr is None and nl is None and _split_ok(x1, n * hout * wout * nout * (c1 + c2)):
        wh = getattr(wpack, "_mia_amax", None)
        if wh is not None:
            amw, am1 = wh[0], amax_slot(x1)
            am2 = None if x2 is None else amax_slot(x2)
            wsp = getattr(wpack, "_mia_split", None)
    tag = PROBE.match(mode, c1, c2, nout, hin, win, bool(flip)) if (PROBE is not None and PROBE.enabled) else None
    probe = PROBE if tag else None
    if probe is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    if cr is not None:
        assert x2 is None and out_split is None and nl is None and bias is None
        yp, cf, sl = cr
        call("mia_conv_mma_cr", mode, _dt(x1), _p(x1), c1, _p(wpack), npad, kpad, int(flip), _p(out1), o1, _p(yp), _p(cf[2]), _p(cf[3]),
             _p(cf[0]), _p(cf[1]), _c_float(sl), _p(stats), n, hin, win, hout, wout, _stream())
    elif nl is not None:
        assert x2 is None and out_split is None and not flip
        call("mia_conv_mma_nl", mode, _dt(x1), _p(x1), c1, _p(nl[0][2]), _p(nl[0][3]), _c_float(nl[1]), _p(wpack), npad, kpad,
             _p(bias), _p(out1), o1, _p(stats), n, hin, win, hout, wout, _stream())
    else:
        # outputs that another conv consumes as they are (ConvTranspose output; the decoder conv's gradient w.r.t. it): maximum in the epilogue
        ao1 = _amax_new(out1) if (mode == CONV_T2S2 and x1.dtype == torch.float32) else None
        ao2 = _amax_new(out2) if (out2 is not None and x1.dtype == torch.float32) else None
        call("mia_conv_mma", mode, _dt(x1), _p(x1), c1, _p(x2), c2, _p(wpack), npad, kpad, int(flip), _p(bias), _p(out1), o1,
             _p(out2), o2, _p(stats), n, hin, win, hout, wout, _p(am1), _p(am2), _p(amw), _p(wsp), _p(ao1), _p(ao2), _stream())
    if probe is not None:
        e1.record()
        probe.pairs.append((e0, e1, tag, (mode, c1 + c2, nout, n, hout, wout)))
    return out1, out2, stats


WGRAD_TARGET_BLOCKS = int(__import__('os').environ.get('MIA_WGRAD_BLOCKS', '0'))  # 0 = ask the library (one or two workgroups per CU)


WGRAD_KSPLIT_MODEL = __import__('os').environ.get('MIA_WGRAD_KSPLIT_MODEL', '1') != '0'  # A/B knob


def _ksplit_by_cost(base: int, slots: int, ntiles: int, slab_bytes: int, flops: float) -> int:
    """Split-K count where base * ksplit cannot hit the machine's workgroup slots exactly (channel counts that are not powers of two:
    cfg5's 96-multiples).  The workgroups run in rounds of `slots`, so a count just above a multiple of `slots` wastes most of a round --
    384 channels: 36 column blocks x 8 slices = 288 of 512 slots, one round at 56 %; 768: 144 x 4 = 576 = two rounds at 56 % -- while every
    extra slice writes and re-reads one more fp32 slab.  Minimise rounds(k) * slots / (base * k) * compute + k * slab traffic over
    k = 1 .. 7 and the multiples of 8 (the XCD-aware launch order needs those)."""
    t_compute = flops / 1.2e15            # the kernels' sustained rate on these shapes
    cands = [k for k in range(1, 8) if k <= ntiles] + [k for k in range(8, min(ntiles, 1024) + 1, 8)]
    best, best_t = 1, None
    for k in cands:
        rounds = -(-base * k // slots)
        t = rounds * slots / (base * k) * t_compute + k * 2.0 * slab_bytes / 4.0e12
        if best_t is None or t < best_t * 0.98:   # (a larger k must win by 2 %)
            best, best_t = k, t
    return best


def conv_wgrad(mode: int, x1: torch.Tensor, x2: Optional[torch.Tensor], dy: torch.Tensor, grad_shape, nn: int, kk: int,
               out: Optional[torch.Tensor] = None, nl=None) -> torch.Tensor:
    """Weight gradient in the parameter's native layout (fp32), written into `out` when given.  nl = (coefs, slope): x1 is the
    producing block's raw conv output, normalised on load (`mia_conv_wgrad_nl`)."""
    n, hx, wx, c1 = x1.shape
    c2 = 0 if x2 is None else x2.shape[3]
    _, hy, wy, cdy = dy.shape
    dtype = _dt(x1)
    taps = 4 if mode == WGRAD_2S2 else 9
    npad, kpad = _pad(nn, 64), _pad(kk, 64)
    # column blocks of one split-K slice, workgroups to aim for and the tile height of the kernel the library will pick for this shape
    # (mia_wgrad_plan: 64-wide blocks cut per source, or 96-wide ones where every channel count is a multiple of 96 and not of 64)
    pb, pt, ph = _c_int(), _c_int(), _c_int()
    call("mia_wgrad_plan", mode, dtype, c1, c2, cdy, npad, hy, ctypes.byref(pb), ctypes.byref(pt), ctypes.byref(ph))
    ntiles = n * -(-hy // ph.value) * -(-wy // 16)
    # column blocks of one split-K slice: the kernels cut the input channels per SOURCE (ceil(c1 / 64) + ceil(c2 / 64) blocks, which
    # is more than kpad / 64 when neither source is a multiple of 64: cfg5's 96 + 96), and the XCD-aware launch order needs a split
    # count that is a multiple of 8 (86, 57 or 29 slices dropped those launches to the plain 2-D order and overfilled the chip:
    # 688 workgroups for 512 slots on cfg5's 192 -> 96 gradient)
    base = pb.value
    target = WGRAD_TARGET_BLOCKS or pt.value
    ksplit = max(1, min(ntiles, -(-target // base), 1024))
    if 8 <= ksplit < ntiles:  # (one tile per slice already: a small problem, leave it)
        ksplit -= ksplit % 8
    if dtype == BF16 and WGRAD_KSPLIT_MODEL and base * ksplit != target:
        ksplit = _ksplit_by_cost(base, target, ntiles, taps * npad * kpad * 4, 2.0 * taps * nn * kk * n * hy * wy)
    slabs = torch.empty((ksplit, taps, npad, kpad), device=x1.device, dtype=torch.float32)
    if nl is not None:
        assert x2 is None
        call("mia_conv_wgrad_nl", mode, dtype, _p(x1), c1, _p(nl[0][2]), _p(nl[0][3]), _c_float(nl[1]), _p(dy), cdy, _p(slabs),
             ksplit, npad, kpad, n, hx, wx, hy, wy, _stream())
    else:
        am1 = am2 = amd = None
        if _split_ok(x1, n * hy * wy * cdy * (c1 + c2)) and dy.dtype == torch.float32:
            am1, amd = amax_slot(x1), amax_slot(dy)
            am2 = None if x2 is None else amax_slot(x2)
        call("mia_conv_wgrad", mode, dtype, _p(x1), c1, _p(x2), c2, _p(dy), cdy, _p(slabs), ksplit, npad, kpad, n, hx, wx, hy,
             wy, _p(am1), _p(am2), _p(amd), _stream())
    grad = out if out is not None else torch.empty(grad_shape, device=x1.device, dtype=torch.float32)
    call("mia_wgrad_reduce", _p(slabs), ksplit, taps, npad, kpad, _p(grad), nn, kk, 0, _stream())
    return grad


def colsum(x: torch.Tensor) -> torch.Tensor:
    c = x.shape[-1]
    p = x.numel() // c
    ws = torch.empty(lib().mia_colsum_workspace(_c_i64(p), c), device=x.device, dtype=torch.float32)
    out = torch.empty(c, device=x.device, dtype=torch.float32)
    call("mia_colsum", _p(x), _dt(x), _c_i64(p), c, _p(ws), _p(out), 0, _stream())
    return out


# Gradient destinations: a flat optimizer registers, per parameter, the slice of its flat gradient buffer; backward nodes
# then let their kernels write the parameter gradient THERE and return that view, which autograd adopts as .grad without a
# copy or an accumulation kernel (82 tiny `add` launches per step otherwise).  Unregistered parameters get fresh tensors.
_GRAD_DEST = {}
_GRAD_CLAIMED = set()  # id(param) whose slice a backward node of the CURRENT accumulation already writes


def register_grad_dest(param: torch.Tensor, flat: torch.Tensor, offset: int) -> None:
    _GRAD_DEST[id(param)] = (__import__("weakref").ref(param), flat, offset, param.numel(), tuple(param.shape))
    _GRAD_CLAIMED.discard(id(param))


def unregister_grad_dest(param: torch.Tensor) -> None:
    _GRAD_DEST.pop(id(param), None)
    _GRAD_CLAIMED.discard(id(param))


def release_grad_dest(param: torch.Tensor) -> None:
    """The parameter's gradient has been accumulated (post-accumulate hook) or dropped (zero_grad): its slice may be
    handed out again."""
    _GRAD_CLAIMED.discard(id(param))


def grad_dest(param: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """A FRESH view of the registered slice (autograd only adopts a gradient nobody else references), handed out to at
    most ONE backward node per accumulation: a second node that uses the same parameter in the same backward pass (model
    called twice before one backward, shared weights) gets None -> a fresh tensor, and autograd sums the two; without the
    claim both kernels would write the same slice and autograd would add two aliased views (2x the last writer)."""
    if param is None:
        return None
    hit = _GRAD_DEST.get(id(param))
    if hit is None:
        return None
    if hit[0]() is not param:
        _GRAD_DEST.pop(id(param), None)
        _GRAD_CLAIMED.discard(id(param))
        return None
    if param.grad is not None:
        return None  # a gradient is already there (accumulation over several backward passes): autograd must ADD to it
    if id(param) in _GRAD_CLAIMED:
        return None
    _GRAD_CLAIMED.add(id(param))
    _, flat, off, n, shape = hit
    return flat[off:off + n].view(shape)


# Column sums that a producer kernel already had for free (conv epilogue statistics), keyed by the tensor they describe;
# consumed by the next backward node that would otherwise re-read that tensor just to sum it.
_COLSUM_HINT = {}


def _hint_colsum(t: torch.Tensor, sums: torch.Tensor) -> None:
    if len(_COLSUM_HINT) > 16:
        _COLSUM_HINT.clear()
    _COLSUM_HINT[t.data_ptr()] = (tuple(t.shape), t._version, sums)


def _take_colsum(t: torch.Tensor) -> Optional[torch.Tensor]:
    hit = _COLSUM_HINT.pop(t.data_ptr(), None)
    if hit is not None and hit[0] == tuple(t.shape) and hit[1] == t._version:
        return hit[2]
    return None


# Norm-backward partial sums computed by the epilogue of the input-gradient conv that produced a dz tensor (mia_conv_mma_cr):
# keyed by that tensor's storage address; the producing block's backward takes them and skips its own reduction pass.
_CR_HINT = {}
# (experiment of round 4, measured +-0 on the cfg3 step; the kernels exist only in probe builds of the library, -DMIA_EXPERIMENTS)
FUSE_CR = __import__('os').environ.get('MIA_FUSE_CR', '0') != '0'


def _hint_cr(dz: torch.Tensor, partials: torch.Tensor) -> None:
    if len(_CR_HINT) > 64:
        _CR_HINT.clear()
    _CR_HINT[dz.data_ptr()] = (partials, tuple(dz.shape))


def _take_cr(dz: torch.Tensor) -> Optional[torch.Tensor]:
    h = _CR_HINT.pop(dz.data_ptr(), None)
    return h[0] if (h is not None and h[1] == tuple(dz.shape)) else None


# Skip tensors have two consumers, so their gradient arrives in two pieces.  The decoder block (which runs first in backward) leaves
# its piece here, keyed by the skip tensor's storage address; the stride-2 block of the next encoder level then ADDS its piece into
# that tensor inside its input-gradient kernel (mia_conv_mma_acc) and returns no gradient of its own, so the skip block's norm
# backward reads one gradient tensor instead of two.
_ACC_HINT = {}
FUSE_ACC = __import__('os').environ.get('MIA_FUSE_ACC', '1') != '0'  # A/B knob


def _hint_acc(x: torch.Tensor, dx: torch.Tensor) -> None:
    if FUSE_ACC and dx is not None:
        _ACC_HINT[x.data_ptr()] = (dx, tuple(x.shape))


def _take_acc(x: torch.Tensor) -> Optional[torch.Tensor]:
    h = _ACC_HINT.pop(x.data_ptr(), None)
    return h[0] if (h is not None and h[1] == tuple(x.shape) and h[0].dtype == x.dtype) else None


def clear_hints() -> None:
    """Drop every producer -> consumer hint and gradient-destination claim (a step that was recorded but never ran -- a failed graph
    capture -- leaves them pointing at tensors nobody wrote)."""
    _COLSUM_HINT.clear()
    _CR_HINT.clear()
    _ACC_HINT.clear()
    _GRAD_CLAIMED.clear()


def cr_supported(dtype, cin: int, cout: int, h: int, w: int) -> bool:
    return (FUSE_CR and dtype == torch.bfloat16 and hasattr(lib(), "mia_conv_mma_cr")
            and bool(lib().mia_conv_cr_supported(CONV_G3S1, BF16, cout, cin, h, w)))


_COL_SLABS = int(__import__('os').environ.get('MIA_COL_SLABS', '64'))


def _slabs_for(hw: int) -> int:
    return max(1, min(_COL_SLABS, hw // 1024))


# ------------------------------------------------------------------ Dropout2d masks
class StepDyn:
    """Per-step scalars of a train step that is replayed from a captured hipGraph (training/engine.py graph mode).  Kernel
    arguments are frozen at capture, so what changes every iteration lives in 32 bytes of device memory that the host rewrites
    (one one-thread launch, `mia_step_dyn_set`) before each replay: fp32 {lr, 1 - beta1^t, 1 - beta2^t, first step} for `mia_optim_step_dyn`
    and u64 {Philox seed, base offset} for `mia_dropout_mask_dyn` (each mask launch adds its fixed distance from the base).
    While `ops._STEP_DYN` is set, `optim_step` and `dropout_mask` take these variants."""

    def __init__(self, device):
        self.dev = torch.zeros(32, dtype=torch.uint8, device=device)
        self.rng_span = 0   # Philox offsets one step consumes (counted while capturing)

    def set(self, lr: float, bc1: float, bc2: float, first: bool, seed: int, base_offset: int) -> None:
        """One one-thread launch whose arguments carry the values (copied at enqueue time: the host may run any number of
        replays ahead of the device, which a pinned staging buffer + async copy would not survive)."""
        call("mia_step_dyn_set", _p(self.dev), _c_float(lr), _c_float(bc1), _c_float(bc2), int(bool(first)),
             ctypes.c_uint64(seed & (2 ** 64 - 1)), ctypes.c_uint64(base_offset), _stream())

    @property
    def f32_ptr(self):
        return ctypes.c_void_p(self.dev.data_ptr())

    @property
    def u64_ptr(self):
        return ctypes.c_void_p(self.dev.data_ptr() + 16)


_STEP_DYN: Optional[StepDyn] = None


def dropout_mask(numel: int, keep: float, device) -> torch.Tensor:
    """`numel` Dropout2d channel multipliers in {0, 1/keep} (reference blocks.py:92-96) from the library's Philox kernel.
    Keyed by the device generator's (seed, offset) -- the pair torch.manual_seed / set_rng_state control, so runs are
    reproducible and per-rank seeds give per-rank masks (al_trainer.py:282-288) -- and the offset is advanced on the host
    like a PyTorch CUDA RNG consumer would: no host random numbers are drawn and no PyTorch kernel runs."""
    dev = torch.device(device)
    if _STEP_DYN is not None:  # captured step: seed / base offset come from device memory, this launch sits `rng_span` past the base
        out = torch.empty(numel, device=dev, dtype=torch.float32)
        call("mia_dropout_mask_dyn", _p(out), _c_i64(numel), _c_float(keep), _STEP_DYN.u64_ptr, ctypes.c_uint64(_STEP_DYN.rng_span), _stream())
        _STEP_DYN.rng_span += 4 * ((numel + 3) // 4)
        return out
    gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
    seed, off = int(gen.initial_seed()), int(gen.get_offset())
    gen.set_offset(off + 4 * ((numel + 3) // 4))
    out = torch.empty(numel, device=dev, dtype=torch.float32)
    call("mia_dropout_mask", _p(out), _c_i64(numel), _c_float(keep), ctypes.c_uint64(seed & (2 ** 64 - 1)), ctypes.c_uint64(off),
         _stream())
    return out


# ------------------------------------------------------------------ UniMatch's feature perturbation: cat(x, Dropout2d(x[rows]))
def _feat_drop_check(x: torch.Tensor, mask: torch.Tensor, row0: int) -> Tuple[int, int]:
    if x.ndim != 4:
        raise MiaError(f"feature_dropout_cat: x must be an NHWC activation [N, H, W, C], got {tuple(x.shape)}")
    if mask.ndim != 2 or mask.shape[1] != x.shape[3] or mask.dtype != torch.float32 or mask.device != x.device:
        raise MiaError(f"feature_dropout_cat: mask must be fp32 [nu, {x.shape[3]}] on {x.device}, got {mask.dtype} "
                       f"{tuple(mask.shape)} on {mask.device}")
    row0, nu = int(row0), int(mask.shape[0])
    if nu < 1 or row0 < 0 or row0 + nu > x.shape[0]:
        raise MiaError(f"feature_dropout_cat: rows [{row0}, {row0} + {nu}) outside the {x.shape[0]} images")
    return row0, nu


def feature_dropout_cat_tensor_ops(x: torch.Tensor, mask: torch.Tensor, row0: int) -> torch.Tensor:
    """The definition of `feature_dropout_cat` in tensor ops (any device, any floating dtype): x followed along the batch axis by
    the channel-dropped copies of its rows row0 .. row0 + nu - 1; the product is formed in fp32 (float64 for a float64 x) and a
    dropped channel is a selection."""
    row0, nu = _feat_drop_check(x, mask, row0)
    m = mask[:, None, None, :]
    wide = torch.float64 if x.dtype == torch.float64 else torch.float32
    return torch.cat((x, torch.where(m == 0, 0, x[row0:row0 + nu].to(wide) * m).to(x.dtype)))


class FeatDropCatFn(torch.autograd.Function):
    """out [N + nu, H, W, C] = cat(x, Dropout2d(x[row0 : row0 + nu])) in ONE pass over x, and its gradient in one pass over dy
    (include/mia_hip.h: mia_feat_drop_cat_fwd / _bwd; csrc/feat_drop.hip).  x: contiguous NHWC fp32 / bf16; mask: fp32 [nu, C] of
    {0, 1 / (1 - p)} (any values; 0 = dropped).  The output is an ordinary tensor: it carries no `_mia_dup` tag, whatever x carries."""

    @staticmethod
    def forward(ctx, x, mask, row0: int):
        ctx.set_materialize_grads(False)
        _need_dev(x, mask)
        row0, nu = _feat_drop_check(x, mask, row0)
        x, mask = x.contiguous(), mask.contiguous()
        n, h, w, c = x.shape
        out = torch.empty((n + nu, h, w, c), device=x.device, dtype=x.dtype)
        call("mia_feat_drop_cat_fwd", _dt(x), _p(x), _p(mask), _p(out), n, _c_i64(h * w), c, row0, nu, _p(_amax_new(out)), _stream())
        ctx.save_for_backward(mask)
        ctx.row0 = row0
        return out

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return None, None, None
        (mask,) = ctx.saved_tensors
        dy = dy.contiguous()
        nu = mask.shape[0]
        n, (h, w, c) = dy.shape[0] - nu, dy.shape[1:]
        dx = torch.empty((n, h, w, c), device=dy.device, dtype=dy.dtype)
        call("mia_feat_drop_cat_bwd", _dt(dy), _p(dy), _p(mask), _p(dx), n, _c_i64(h * w), c, ctx.row0, nu, _p(_amax_new(dx)), _stream())
        return dx, None, None


def feature_dropout_cat(x: torch.Tensor, mask: torch.Tensor, row0: int, *, fused: bool = True) -> torch.Tensor:
    """UniMatch's feature-perturbation input of the decoder for one encoder output: the N rows of x followed by the perturbed twins
    of rows row0 .. row0 + nu - 1, `cat(x, Dropout2d(x[row0 : row0 + nu]))`.  x: NHWC activation; mask: fp32 [nu, C] on x's device.
    fused=True: the HIP kernels (fp32 / bf16 on the device; no fallback); fused=False: `feature_dropout_cat_tensor_ops`, the same
    definition under autograd, which also serves CPU tensors and other dtypes.  Both give the same bits, forward and gradient."""
    if fused:
        return FeatDropCatFn.apply(x, mask, row0)
    return feature_dropout_cat_tensor_ops(x, mask, row0)


# ------------------------------------------------------------------ PlainBlock: conv3x3 -> dropout2d -> norm -> lrelu
class NormCfg:
    __slots__ = ("mode", "training", "eps", "momentum", "running_mean", "running_var", "num_batches", "drop_scale", "sync")

    def __init__(self, mode, training, eps=1e-5, momentum=0.1, running_mean=None, running_var=None, num_batches=None,
                 drop_scale=None, sync=None):
        self.mode, self.training, self.eps, self.momentum = mode, training, eps, momentum
        self.running_mean, self.running_var, self.num_batches, self.drop_scale = running_mean, running_var, num_batches, drop_scale
        self.sync = sync  # BatchSync or None

    fixed = property(lambda self: self.mode == NORM_BATCH and not self.training)  # eval batch norm: running statistics, no batch sums


class BatchSync:
    """Process group for synchronised batch-norm statistics (one process per GPU)."""

    def __init__(self, process_group=None):
        import torch.distributed as dist
        self.dist, self.pg = dist, process_group
        self.world = dist.get_world_size(process_group)

    def all_gather(self, local: torch.Tensor) -> torch.Tensor:
        out = torch.empty((self.world,) + tuple(local.shape), device=local.device, dtype=local.dtype)
        self.dist.all_gather([out[r] for r in range(self.world)], local, group=self.pg)  # works on gloo and RCCL
        return out

    def all_reduce_sum(self, t: torch.Tensor) -> torch.Tensor:
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.pg)
        return t


_BN_TRACKING = True


class no_bn_tracking:
    """Context manager: training-mode batch norm still normalises with the batch statistics, but the running statistics and
    `num_batches_tracked` stay untouched (the kernels get no pointer to them).  For extra forward passes that are not training steps,
    e.g. the power iteration of virtual adversarial training (the published code's `_disable_tracking_bn_stats`)."""

    def __enter__(self):
        global _BN_TRACKING
        self._was, _BN_TRACKING = _BN_TRACKING, False

    def __exit__(self, *exc):
        global _BN_TRACKING
        _BN_TRACKING = self._was
        return False


def _norm_finalize(ctx, cfg: NormCfg, stats, gamma, beta, y) -> torch.Tensor:
    """The [5, N, C] per-(n,c) coefficient table (xa, xb, scale, shift, sum_y) of a block with raw conv output y, from the conv-epilogue
    partials; batch statistics cover every rank when cfg.sync is set, and ctx.sync then keeps the group for backward."""
    n, h, w, cout = y.shape
    hw = h * w
    coefs = torch.empty((5, n, cout), device=y.device, dtype=torch.float32)
    ctx.sync = sync = cfg.sync if (cfg.sync is not None and cfg.mode == NORM_BATCH and cfg.training and cfg.sync.world > 1) else None
    track = _BN_TRACKING or not cfg.training  # (eval batch norm READS the running statistics)
    rmean, rvar, nbatch = (cfg.running_mean, cfg.running_var, cfg.num_batches) if track else (None, None, None)
    if sync is None:
        call("mia_norm_finalize", _p(stats), n, 0 if stats is None else stats.shape[1], cout, _c_i64(hw), cfg.mode, int(cfg.training),
             _p(cfg.drop_scale), _p(gamma.detach()), _p(beta.detach()), _c_float(cfg.eps), _c_float(cfg.momentum),
             _p(rmean), _p(rvar), _p(nbatch), _p(coefs[0]), _p(coefs[1]), _p(coefs[2]),
             _p(coefs[3]), _p(coefs[4]), _stream())
        return coefs
    local = torch.empty((3, cout), device=stats.device, dtype=torch.float32)
    call("mia_bn_sync_local_stats", _p(stats), n, stats.shape[1], cout, _c_i64(hw), _p(cfg.drop_scale), _p(coefs[0]),
         _p(coefs[1]), _p(local), _stream())
    gathered = sync.all_gather(local)
    call("mia_norm_finalize_sync", _p(gathered), sync.world, n, cout, _c_i64(hw), _p(cfg.drop_scale), _p(gamma.detach()),
         _p(beta.detach()), _c_float(cfg.eps), _c_float(cfg.momentum), _p(rmean), _p(rvar),
         _p(nbatch), _p(coefs[0]), _p(coefs[1]), _p(coefs[2]), _p(coefs[3]), _p(coefs[4]), _stream())
    return coefs


def _norm_act_fwd(y, scale, shift, slope) -> torch.Tensor:
    """z = lrelu(scale[n,c] * y + shift[n,c]) as a new tensor (`mia_norm_act_fwd`; an fp32 z carries its maximum slot)."""
    n, h, w, c = y.shape
    z = torch.empty_like(y)
    call("mia_norm_act_fwd", _p(y), _p(z), _dt(y), _p(scale), _p(shift), n, _c_i64(h * w), c, _c_float(slope), _p(_amax_new(z)), _stream())
    return z


class LazyAct:
    """Output of a PlainBlock whose normalisation + LeakyReLU (blocks.py:98-102) is NOT materialised: `y` is the raw conv
    output (it carries the autograd history and, by convention, the gradient delivered to it is d loss / d z), `coefs`
    the block's [5, N, C] coefficient table (rows 2 / 3 = scale / shift with Dropout2d folded in).  The next block's conv
    and weight gradient form z = lrelu(scale * y + shift) on load (`mia_conv_mma_nl`, `mia_conv_wgrad_nl`)."""
    __slots__ = ("y", "coefs", "slope")

    def __init__(self, y, coefs, slope):
        self.y, self.coefs, self.slope = y, coefs, slope

    @property
    def shape(self):
        return self.y.shape

    @property
    def dtype(self):
        return self.y.dtype

    @property
    def device(self):
        return self.y.device

    def materialize(self) -> torch.Tensor:
        return LazyMaterializeFn.apply(self.y, self.coefs, self.slope)


class LazyMaterializeFn(torch.autograd.Function):
    """z = lrelu(scale * y + shift) as a tensor (a consumer outside the fused kernels' contract).  The gradient passes
    through unchanged: the producer expects d loss / d z on its raw-output handle (see LazyAct)."""

    @staticmethod
    def forward(ctx, y, coefs, slope):
        return _norm_act_fwd(y, coefs[2], coefs[3], slope)

    @staticmethod
    def backward(ctx, dz):
        return dz, None, None


FUSE_HEAD_W = __import__('os').environ.get('MIA_FUSE_HEAD_W', '1') != '0'  # A/B knob: head dW / db in the norm-backward reduction pass
FUSE_STEM_BWD = __import__('os').environ.get('MIA_FUSE_STEM_BWD', '1') != '0'  # A/B knob: the stem's backward apply pass folded into its weight gradient
FUSE_NL = __import__('os').environ.get('MIA_FUSE_NL', '1') != '0'  # A/B knob: 0 = every block materialises its activation


def nl_supported(dtype, cin: int, cout: int, h: int, w: int, train: bool) -> bool:
    """Can a stride-1 3x3 block with these shapes consume its predecessor's raw output (normalise-on-load)?  bf16 only: the 64 -> 64
    register-staged kernels (the fp32 form of round 4 measured +-0 and is gone: the split-f16 products need the maximum of the
    NORMALISED tensor, which nobody has computed when the raw output is loaded)."""
    if not FUSE_NL or dtype != torch.bfloat16:
        return False
    if not lib().mia_conv_nl_supported(CONV_G3S1, BF16, cin, cout, h, w):
        return False
    return (not train) or bool(lib().mia_wgrad_nl_supported(WGRAD_3S1, BF16, cin, cout))


class _NormBwd:
    """Step 1 of a block's backward, the norm backward: the parameter run that every `mia_norm_*bwd*` entry shares (`_run`), the scratch
    behind it (slab partials `part`; `cc`: per-(n,c) sums, then the group means) and where the parameter gradients go -- the registered
    slices (`grad_dest`) of `dests` = (gamma, beta, bias) where there are any, rows of a private table otherwise or with dests=None."""

    def __init__(self, y, coefs, mode, fixed, slope, dests=None):
        self.y, self.coefs, self.mode, self.fixed, self.slope = y, coefs, mode, fixed, slope
        n, h, w, c = y.shape
        self.dtype, self.n, self.hw, self.c, self.slabs = _dt(y), n, h * w, c, _slabs_for(h * w)
        self.part = torch.empty((n, self.slabs, c, 2), device=y.device, dtype=torch.float32)
        self.cc = torch.empty((2, n, c), device=y.device, dtype=torch.float32)
        dgb = torch.empty((3, c), device=y.device, dtype=torch.float32)
        got = (None,) * 3 if dests is None else [grad_dest(p) for p in dests]
        self.dgamma, self.dbeta, self.dbias = (dgb[i] if g is None else g for i, g in enumerate(got))

    def _run(self, slabs, part):
        k = self.coefs
        return (_p(k[2]), _p(k[3]), _p(k[0]), _p(k[1]), _p(None if self.fixed else k[4]), self.n, _c_i64(self.hw), self.c, self.mode,
                int(self.fixed), _c_float(self.slope), slabs, _p(part), _p(self.cc[0]), _p(self.cc[1]), _p(self.dgamma),
                _p(self.dbeta), _p(self.dbias), 0)

    def plain(self, dz, dz2, dy) -> None:
        call("mia_norm_act_bwd", _p(dz), _p(dz2), _p(self.y), _p(dy), self.dtype, *self._run(self.slabs, self.part),
             _p(_amax_new(dy)), _stream())

    def sums(self, dz, dz2) -> None:
        """No apply pass: the only consumer of dy forms it on load from `cc` (the fused stem weight gradient)."""
        call("mia_norm_bwd_sums", _p(dz), _p(dz2), _p(self.y), self.dtype, *self._run(self.slabs, self.part), _stream())

    def pre(self, parts, dz, dy) -> None:
        """The reduction already ran in the epilogue of the conv that produced dz (`parts`); the apply pass only where dy is wanted."""
        call("mia_norm_act_bwd_pre", _p(None if dy is None else dz), _p(None if dy is None else self.y), _p(dy), self.dtype,
             *self._run(parts.shape[1], parts), _p(None if dy is None else _amax_new(dy)), _stream())

    def synced(self, sync: BatchSync, dz, dz2, dy) -> None:
        """Synchronised batch norm: the group means of g and g*xhat cover every rank's shard."""
        k, cc = self.coefs, self.cc
        tot = torch.empty((3, self.c), device=self.y.device, dtype=torch.float32)
        call("mia_norm_act_bwd_reduce", _p(dz), _p(dz2), _p(self.y), self.dtype, _p(k[2]), _p(k[3]), _p(k[0]), _p(k[1]), self.n,
             _c_i64(self.hw), self.c, _c_float(self.slope), self.slabs, _p(self.part), _p(cc[0]), _p(cc[1]), _p(tot), _stream())
        sync.all_reduce_sum(tot)
        call("mia_norm_act_bwd_apply_sync", _p(dz), _p(dz2), _p(self.y), _p(dy), self.dtype, _p(k[2]), _p(k[3]), _p(k[0]), _p(k[1]),
             _p(k[4]), self.n, _c_i64(self.hw), self.c, _c_float(self.slope), _p(cc[0]), _p(cc[1]), _p(tot), _p(self.dgamma),
             _p(self.dbeta), _p(self.dbias), 0, _p(_amax_new(dy)), _stream())

    def run(self, dz, dz2, sync, on_load: bool) -> Optional[torch.Tensor]:
        """Pick the entry.  Returns dy, or None where the only consumer forms it on load (the stem's weight gradient: it has no input gradient)."""
        pre = _take_cr(dz) if (dz2 is None and sync is None) else None  # reduction already done by the conv that produced dz
        dy = None if on_load else torch.empty_like(self.y)
        if pre is not None:
            self.pre(pre, dz, dy)
        elif sync is not None:
            self.synced(sync, dz, dz2, dy)
        elif on_load:
            self.sums(dz, dz2)
        else:
            self.plain(dz, dz2, dy)
        return dy

    def head(self, dl, st, w2, dy, entry="mia_norm_act_bwd_head", extra=()) -> None:
        """dz = W^T dl recomputed on the fly from the 1x1 head's weights w2 and its logits gradient dl (pixel strides st)."""
        call(entry, _p(dl), _p(w2), w2.shape[0], _c_i64(st[0]), _c_i64(st[1]), _c_i64(st[2]), _p(self.y), _p(dy), self.dtype,
             *self._run(self.slabs, self.part), *extra, _p(_amax_new(dy)), _stream())

    def head_w(self, dl, st, w2, dy, ws, dwh, dbh) -> None:
        """`head` whose reduction pass also accumulates the head's own dW / db (one pass over (dl, y))."""
        self.head(dl, st, w2, dy, "mia_norm_act_bwd_head_w", (_p(ws), _p(dwh), _p(dbh), 0))


def _block_wgrad(nb: _NormBwd, x1, x2, weight, stride: int, nl, dy, stem: bool = False, dz=None, dz2=None) -> torch.Tensor:
    """Step 2 of a block's backward: the conv weight gradient, written to the parameter's registered slice where there is one.  The stem
    has its own kernels; with dy=None (no apply pass ran: `_NormBwd.sums` / `pre`) its kernel forms dy on load from dz, y and the group means."""
    cout, cin = weight.shape[:2]
    y, k = nb.y, nb.coefs
    if not stem:
        dw = conv_wgrad(WGRAD_3S2 if stride == 2 else WGRAD_3S1, x1, x2, dy, weight.shape, cout, cin, out=grad_dest(weight), nl=nl)
    else:
        if dy is None and dz2 is not None:
            dz = dz + dz2
        ws = torch.empty(lib().mia_stem_wgrad_workspace(cout), device=y.device, dtype=torch.float32)
        dw = grad_dest(weight)
        if dw is None:
            dw = torch.empty(weight.shape, device=y.device, dtype=torch.float32)
        if dy is None:
            call("mia_stem_wgrad_fused", _p(x1), _dt(x1), _p(dz), _p(y), nb.dtype, _p(k[2]), _p(k[3]), _p(k[0]), _p(k[1]),
                 _p(nb.cc[0]), _p(nb.cc[1]), _c_float(nb.slope), _p(ws), _p(dw), nb.n, y.shape[1], y.shape[2], cout, 0, _stream())
        else:
            call("mia_stem_wgrad", _p(x1), _dt(x1), _p(dy), nb.dtype, _p(ws), _p(dw), nb.n, y.shape[1], y.shape[2], cout, 0, _stream())
    return dw


def _stem_dgrad(dy, weight, x1) -> torch.Tensor:
    """Step 3 for the stem: the image gradient [N, H, W, 1] from dy (`mia_stem_dgrad`, fp32), in the image's dtype."""
    n, h, w, cout = dy.shape
    w2 = weight.detach().reshape(cout, 9)
    if not w2.is_contiguous():
        w2 = w2.contiguous()
    dx = torch.empty((n, h, w, 1), device=dy.device, dtype=torch.float32)
    call("mia_stem_dgrad", _p(dy), _dt(dy), _p(w2), _p(dx), n, h, w, cout, _stream())
    return dx if x1.dtype == torch.float32 else cast_nhwc(dx, x1.dtype)


def _block_dgrad(x1, x2, weight, dy, stride: int, nl, dup_in: bool, need1: bool, need2: bool):
    """Step 3 of a block's backward, where somebody needs it: (dx1, dx2) from dy.  nl = (coefs, slope): x1 is the previous block's raw output."""
    dx1 = dx2 = None
    dtype = _dt(dy)
    n, ho, wo, cout = dy.shape
    c1, cin = x1.shape[3], weight.shape[1]
    wb, npad, kpad = pack_cache(weight).get(weight, dtype, n_from_d0=False)
    split = c1 if x2 is not None else None
    other = _take_acc(x1) if (stride == 2 and x2 is None and dup_in) else None
    if other is not None and lib().mia_conv_acc_supported(CONV_T3S2, dtype, cout, cin):
        # the other consumer of x1 (a skip tensor) has already written its gradient piece: add ours into it, return none of our own
        amw = getattr(wb, "_mia_amax", None) if _split_ok(dy, n * ho * wo * cout * cin) else None
        call("mia_conv_mma_acc", CONV_T3S2, dtype, _p(dy), cout, _p(wb), npad, kpad, 0, _p(other), cin, n, ho, wo,
             x1.shape[1], x1.shape[2], _p(None if amw is None else amax_slot(dy)), _p(None if amw is None else amw[0]),
             _p(None if amw is None else getattr(wb, "_mia_split", None)), _stream())
    elif stride == 2:
        dx1, dx2, _ = conv_mma(CONV_T3S2, dy, None, wb, npad, kpad, False, None, cin, (x1.shape[1], x1.shape[2]), out_split=split)
    elif nl is not None and cr_supported(dy.dtype, cin, cout, ho, wo):
        # x1 is the previous block's raw output: its norm-backward reduction rides in this conv's epilogue
        dx1, _, partials = conv_mma(CONV_G3S1, dy, None, wb, npad, kpad, True, None, cin, (ho, wo), cr=(x1,) + nl)
        _hint_cr(dx1, partials)
    else:
        # decoder block behind a ConvTranspose2d: dx2 is that layer's output gradient and its per-channel sum is
        # the transposed conv's bias gradient -- the epilogue statistics deliver it without another pass over dx2
        want = x2 is not None and need2
        dx1, dx2, st = conv_mma(CONV_G3S1, dy, None, wb, npad, kpad, True, None, cin, (ho, wo), want_stats=want, out_split=split)
        if want:
            sums = colsum(st.view(-1, 2 * cin)).view(cin, 2)[c1:, 0]
            _hint_colsum(dx2, sums)
        if x2 is not None and need1 and dup_in:
            _hint_acc(x1, dx1)  # x1 is the skip tensor: its other consumer may add its gradient piece into dx1
    return dx1, dx2


class PlainBlockFn(torch.autograd.Function):
    """Fused reference PlainBlock (src/models/unet/blocks.py:66-105) on NHWC tensors.

    inputs x1 [N,H,W,C1] (+ optional x2 [N,H,W,C2], concatenated along C: unet.py:213)."""

    @staticmethod
    def forward(ctx, x1, x2, weight, bias, gamma, beta, stride: int, cfg: NormCfg, out_dtype=None, slope: float = LRELU_SLOPE,
                dup: bool = False, lazy: bool = False, nl_coefs=None, nl_slope: float = LRELU_SLOPE):
        """lazy=True: the norm + LeakyReLU pass is skipped and (y, coefs) is returned for a `LazyAct` (the next block
        normalises on load).  nl_coefs: x1 is such a raw output of the previous block (its coefficient table).
        dup=True returns the output TWICE (two tensors on one storage): a skip tensor has two consumers, and handing
        each its own output makes autograd deliver their gradients separately to backward, which sums them on load inside
        the norm kernels instead of autograd launching an `add` over the full activation."""
        # x1 is one of the two views a `dup=True` block handed out (tagged by the model): exactly one gradient will ever arrive
        # for it, so the two consumers may share one gradient tensor (see _ACC_HINT).  Untagged tensors (e.g. a ResidualBlock's
        # output, whose several gradient pieces autograd itself adds up) never take that path.
        ctx.dup_in = bool(getattr(x1, "_mia_dup", False))
        ctx.set_materialize_grads(False)
        _need_dev(x1, x2, weight)
        x1 = x1.contiguous()
        x2 = None if x2 is None else x2.contiguous()
        out_dtype = out_dtype or x1.dtype
        cout = weight.shape[0]
        assert not (lazy and dup)
        # (an image that requires a gradient keeps the stem: same logits bit for bit, and backward has `mia_stem_dgrad`)
        stem = (weight.shape[1] == 1 and x2 is None and stride == 1 and x1.shape[3] == 1
                and cout % (8 if out_dtype == torch.bfloat16 else 4) == 0 and cout <= 256 and nl_coefs is None)
        if stem:
            z = PlainBlockFn._stem_forward(ctx, x1, weight, bias, gamma, beta, cfg, out_dtype, slope, lazy)
            return (z, _dup_view(z)) if dup else z  # (lazy: z is the (y, coefs) pair, and dup is off)
        if x1.dtype != out_dtype:
            x1 = cast_nhwc(x1, out_dtype)
        if x2 is not None and (x2.shape[:3] != x1.shape[:3] or x2.dtype != x1.dtype):
            # same failure point as torch.cat([skip, up], 1) in the reference (unet.py:213)
            raise RuntimeError(f"Sizes of tensors must match except in dimension 1: {tuple(x1.shape)} vs {tuple(x2.shape)} (NHWC)")
        dtype = _dt(x1)
        n, h, w, c1 = x1.shape
        if weight.shape[1] != c1 + (0 if x2 is None else x2.shape[3]):
            raise RuntimeError(f"conv weight expects {weight.shape[1]} input channels, got {c1 + (0 if x2 is None else x2.shape[3])}")
        ho, wo = ((h + 1) // 2, (w + 1) // 2) if stride == 2 else (h, w)
        wp, npad, kpad = pack_cache(weight).get(weight, dtype, n_from_d0=True)
        mode = CONV_G3S2 if stride == 2 else CONV_G3S1
        nl = None if nl_coefs is None else (nl_coefs, float(nl_slope))
        if nl is not None and (x2 is not None or stride != 1):
            raise MiaError("normalise-on-load serves one-source stride-1 blocks only")
        y, _, stats = conv_mma(mode, x1, x2, wp, npad, kpad, False, bias.detach().float(), cout, (ho, wo), want_stats=not cfg.fixed,
                               nl=nl)
        coefs = _norm_finalize(ctx, cfg, stats, gamma, beta, y)
        ctx.stride, ctx.mode, ctx.fixed, ctx.stem, ctx.slope = stride, cfg.mode, cfg.fixed, False, slope
        ctx.small = (bias, beta)  # identities only (gradient destinations); values are not needed in backward
        ctx.nl_slope = float(nl_slope)
        ctx.save_for_backward(x1, x2, y, coefs, weight, gamma, nl_coefs)
        if lazy:  # the consumer normalises on load: no apply pass, no activation tensor
            ctx.mark_non_differentiable(coefs)
            return y, coefs
        z = _norm_act_fwd(y, coefs[2], coefs[3], slope)
        return (z, _dup_view(z)) if dup else z

    @staticmethod
    def _norm_act(ctx, y, stats, gamma, beta, cfg, slope=LRELU_SLOPE):
        coefs = _norm_finalize(ctx, cfg, stats, gamma, beta, y)
        return _norm_act_fwd(y, coefs[2], coefs[3], slope), coefs

    @staticmethod
    def _stem_forward(ctx, x1, weight, bias, gamma, beta, cfg, out_dtype, slope, lazy=False):
        n, h, w, _ = x1.shape
        cout = weight.shape[0]
        dev = x1.device
        y = torch.empty((n, h, w, cout), device=dev, dtype=out_dtype)
        stats = torch.empty((n, lib().mia_stem_slabs(), cout, 2), device=dev, dtype=torch.float32)
        w2 = weight.detach().reshape(cout, 9)
        if not w2.is_contiguous():
            w2 = w2.contiguous()
        call("mia_stem_fwd", _p(x1), _dt(x1), _p(w2), _p(bias.detach()), _p(y), _dt(y), _p(stats), n, h, w, cout, _stream())
        ctx.stride, ctx.mode, ctx.fixed, ctx.stem, ctx.slope = 1, cfg.mode, cfg.fixed, True, slope
        ctx.small = (bias, beta)
        ctx.nl_slope = LRELU_SLOPE
        coefs = _norm_finalize(ctx, cfg, stats, gamma, beta, y)
        ctx.save_for_backward(x1, None, y, coefs, weight, gamma, None)
        if lazy:
            ctx.mark_non_differentiable(coefs)
            return y, coefs
        return _norm_act_fwd(y, coefs[2], coefs[3], slope)

    @staticmethod
    def backward(ctx, *grads):
        x1, x2, y, coefs, weight, gamma, nl_coefs = ctx.saved_tensors
        pieces = [g_.contiguous() for g_ in grads if g_ is not None]
        if not pieces:
            return (None,) * 14
        dz, dz2 = pieces[0], (pieces[1] if len(pieces) > 1 else None)
        if dz2 is not None and not (lib().mia_norm_two_piece_ok(_dt(y), y.shape[3]) and dz.data_ptr() % 16 == 0 and dz2.data_ptr() % 16 == 0):
            dz, dz2 = dz + dz2, None  # shapes outside the vectorised kernels: one explicit sum
        need_w = any(ctx.needs_input_grad[2:6])  # frozen parameters (ops.frozen_parameters): no weight gradient, no claimed slice
        nb = _NormBwd(y, coefs, ctx.mode, ctx.fixed, ctx.slope, (gamma, ctx.small[1], ctx.small[0]) if need_w else None)
        # the stem's dy is formed on load by its weight gradient -- unless the image wants a gradient too: `mia_stem_dgrad` reads dy
        on_load = ctx.stem and ctx.sync is None and FUSE_STEM_BWD and need_w and not ctx.needs_input_grad[0]
        dy = nb.run(dz, dz2, ctx.sync, on_load)
        nl = None if nl_coefs is None else (nl_coefs, ctx.nl_slope)
        dw = _block_wgrad(nb, x1, x2, weight, ctx.stride, nl, dy, ctx.stem, dz, dz2) if need_w else None
        dx1 = dx2 = None
        if ctx.stem:
            if ctx.needs_input_grad[0]:
                dx1 = _stem_dgrad(dy, weight, x1)
        elif ctx.needs_input_grad[0] or (x2 is not None and ctx.needs_input_grad[1]):
            dx1, dx2 = _block_dgrad(x1, x2, weight, dy, ctx.stride, nl, ctx.dup_in, *ctx.needs_input_grad[:2])
        if not need_w:
            return (dx1, dx2) + (None,) * 12
        return (dx1, dx2, dw, nb.dbias, nb.dgamma, nb.dbeta) + (None,) * 8


class PlainBlockHeadFn(torch.autograd.Function):
    """Last decoder PlainBlock (stride 1, one input) fused with the 1x1 segmentation head behind it
    (src/models/unet/blocks.py:66-105 + unet.py:176): logits = W_head * lrelu(norm(conv(x))) + b_head.

    The block's activated output has exactly one consumer, so it is never materialised: the head recomputes it from the
    raw conv output on load (`mia_head_norm_fwd` / `mia_head_norm_wgrad`) and the norm backward recomputes the head's
    input gradient W^T dlogits on the fly (`mia_norm_act_bwd_head`).  Saves the forward apply pass, the head's
    input-gradient kernel and two reads of that gradient (about 4.3 GB of HBM traffic per step on cfg3)."""

    @staticmethod
    def eligible(x1, weight, head_w, cfg: NormCfg, dtype) -> bool:
        if cfg.sync is not None or x1.ndim != 4 or weight.shape[1] == 1:
            return False
        n, h, w, _ = x1.shape
        cout, k1 = weight.shape[0], head_w.shape[0]
        return cout % 32 == 0 and lib().mia_head_norm_eligible(_dt(dtype), n, _c_i64(h * w), cout, k1) > 0

    @staticmethod
    def forward(ctx, x1, weight, bias, gamma, beta, cfg: NormCfg, head_w, head_b, slope: float = LRELU_SLOPE, nl_coefs=None,
                nl_slope: float = LRELU_SLOPE):
        """nl_coefs: x1 is the previous block's RAW conv output with that coefficient table (normalise-on-load)."""
        _need_dev(x1, weight, head_w)
        x1 = x1.contiguous()
        dtype = _dt(x1)
        n, h, w, c1 = x1.shape
        cout, k1 = weight.shape[0], head_w.shape[0]
        if weight.shape[1] != c1:
            raise RuntimeError(f"conv weight expects {weight.shape[1]} input channels, got {c1}")
        wp, npad, kpad = pack_cache(weight).get(weight, dtype, n_from_d0=True)
        y, _, stats = conv_mma(CONV_G3S1, x1, None, wp, npad, kpad, False, bias.detach().float(), cout, (h, w), want_stats=not cfg.fixed,
                               nl=None if nl_coefs is None else (nl_coefs, float(nl_slope)))
        coefs = _norm_finalize(ctx, cfg, stats, gamma, beta, y)
        ctx.nl_slope = float(nl_slope)
        w2 = head_w.detach().reshape(k1, cout).contiguous()
        logits = torch.empty((n, h, w, k1), device=x1.device, dtype=torch.float32)
        call("mia_head_norm_fwd", _p(y), dtype, _p(coefs[2]), _p(coefs[3]), _c_float(slope), _p(w2), _p(head_b.detach()),
             _p(logits), n, _c_i64(h * w), cout, k1, _c_i64(h * w * k1), _c_i64(1), _c_i64(k1), _stream())
        ctx.save_for_backward(x1, y, coefs, weight, gamma, head_w, nl_coefs)
        ctx.mode, ctx.fixed, ctx.slope = cfg.mode, cfg.fixed, slope
        ctx.small = (bias, beta, head_b)
        return logits.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dl):
        x1, y, coefs, weight, gamma, head_w, nl_coefs = ctx.saved_tensors
        bias_p, beta_p, head_b = ctx.small
        n, h, w, cout = y.shape
        k1 = head_w.shape[0]
        dev, hw = y.device, h * w
        if dl.dtype != torch.float32:
            dl = dl.float()
        st = _pix_strides(dl)
        if st is None or st[0] != hw * st[2]:
            dl = dl.contiguous()
            st = _pix_strides(dl)
        w2 = head_w.detach().reshape(k1, cout).contiguous()
        ni = ctx.needs_input_grad
        need_w = any(ni[1:5]) or ni[6] or ni[7]
        dy = torch.empty_like(y)
        nl = None if nl_coefs is None else (nl_coefs, ctx.nl_slope)
        if not need_w:  # frozen parameters: the norm backward with dz = W^T dl alone -- no head dW / db, no weight gradient, no claimed slice
            nb = _NormBwd(y, coefs, ctx.mode, ctx.fixed, ctx.slope)
            nb.head(dl, st, w2, dy)
            dx1 = _block_dgrad(x1, None, weight, dy, 1, nl, False, True, False)[0] if ni[0] else None
            return (dx1,) + (None,) * 10
        dwh, dbh = grad_dest(head_w), grad_dest(head_b)
        dwh = torch.empty((k1, cout), device=dev, dtype=torch.float32) if dwh is None else dwh
        dbh = torch.empty(k1, device=dev, dtype=torch.float32) if dbh is None else dbh
        nb = _NormBwd(y, coefs, ctx.mode, ctx.fixed, ctx.slope, (gamma, beta_p, bias_p))
        if FUSE_HEAD_W and lib().mia_head_w_supported(nb.dtype, cout, k1):
            # head dW / db and the block's norm-backward sums in ONE pass over (dl, y); then the apply pass with dz = W^T dl recomputed
            ws = torch.empty(n * nb.slabs * k1 * (cout + 1), device=dev, dtype=torch.float32)
            nb.head_w(dl, st, w2, dy, ws, dwh, dbh)
        else:
            ws = torch.empty(lib().mia_head_bwd_workspace(cout, k1), device=dev, dtype=torch.float32)
            call("mia_head_norm_wgrad", _p(dl), _p(y), nb.dtype, _p(coefs[2]), _p(coefs[3]), _c_float(ctx.slope), _p(dwh), _p(dbh),
                 _p(ws), n, _c_i64(hw), cout, k1, _c_i64(st[0]), _c_i64(st[1]), _c_i64(st[2]), 0, _stream())
            nb.head(dl, st, w2, dy)
        dw = _block_wgrad(nb, x1, None, weight, 1, nl, dy)
        dx1 = None
        if ctx.needs_input_grad[0]:
            dx1, _ = _block_dgrad(x1, None, weight, dy, 1, nl, False, True, False)
        return dx1, dw, nb.dbias, nb.dgamma, nb.dbeta, None, dwh.reshape(head_w.shape), dbh, None, None, None


class ConvTranspose2x2Fn(torch.autograd.Function):
    """nn.ConvTranspose2d(cin, cout, 2, 2) (src/models/unet/unet.py:142) as a pointwise MFMA GEMM + pixel shuffle."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _need_dev(x, weight)
        x = x.contiguous()
        dtype = _dt(x)
        n, h, w, cin = x.shape
        cout = weight.shape[1]
        wp, npad, kpad = pack_cache(weight).get(weight, dtype, n_from_d0=False)  # [tap][co][ci]
        out, _, _ = conv_mma(CONV_T2S2, x, None, wp, npad, kpad, False, bias.detach().float(), cout, (2 * h, 2 * w))
        ctx.save_for_backward(x, weight)
        ctx.small = (bias,)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight = ctx.saved_tensors
        dout = dout.contiguous()
        dtype = _dt(x)
        n, h, w, cin = x.shape
        cout = weight.shape[1]
        dbias = dw = None
        hinted = _take_colsum(dout)  # (taken in any case: a hint must not outlive its backward)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:  # (frozen parameters: neither)
            dbias = hinted if hinted is not None else colsum(dout)
            dst = grad_dest(ctx.small[0])
            if dst is not None:  # straight into the flat gradient slice (the hinted sums are a strided view of interleaved statistics)
                call("mia_gather_f32", _p(dbias), _c_i64(dbias.stride(0)), _p(dst), dbias.numel(), _stream())
                dbias = dst
            dw = conv_wgrad(WGRAD_2S2, dout, None, x, weight.shape, cin, cout, out=grad_dest(weight))
        dx = None
        if ctx.needs_input_grad[0]:
            wb, npad, kpad = pack_cache(weight).get(weight, dtype, n_from_d0=True)  # [tap][ci][co]
            dx, _, _ = conv_mma(CONV_G2S2, dout, None, wb, npad, kpad, False, None, cin, (h, w))
        return dx, dw, dbias


# ------------------------------------------------------------------ 1x1 head
def _pix_strides(t: torch.Tensor):
    """(sn, sk, sp) element strides of a logical [B,K,H,W] tensor whose H,W dims collapse, else None."""
    b, k, h, w = t.shape
    sn, sk, sh, sw = t.stride()
    if h == 1 or sh == w * sw:
        return sn, sk, sw
    return None


class HeadFn(torch.autograd.Function):
    """seg_output = Conv2d(c0, K1, 1) (src/models/unet/unet.py:176): NHWC activations -> fp32 logits
    returned as a logical-NCHW view with channels_last strides."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _need_dev(x, weight)
        x = x.contiguous()
        n, h, w, c0 = x.shape
        k1 = weight.shape[0]
        w2 = weight.detach().reshape(k1, c0).contiguous()
        logits = torch.empty((n, h, w, k1), device=x.device, dtype=torch.float32)
        call("mia_head_fwd", _p(x), _dt(x), _p(w2), _p(bias.detach()), _p(logits), n, _c_i64(h * w), c0, k1,
             _c_i64(h * w * k1), _c_i64(1), _c_i64(k1), _stream())
        ctx.save_for_backward(x, weight)
        ctx.small = (bias,)
        return logits.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dl):
        x, weight = ctx.saved_tensors
        n, h, w, c0 = x.shape
        k1 = weight.shape[0]
        if dl.dtype != torch.float32:
            dl = dl.float()
        st = _pix_strides(dl)
        if st is None:
            dl = dl.contiguous()
            st = _pix_strides(dl)
        w2 = weight.detach().reshape(k1, c0).contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        need_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if not need_w:  # frozen parameters: the input gradient alone, no weight kernels, no claimed slice
            if dx is not None:
                call("mia_head_bwd", _p(dl), _p(x), _dt(x), _p(w2), _p(dx), None, None, None, n, _c_i64(h * w), c0, k1,
                     _c_i64(st[0]), _c_i64(st[1]), _c_i64(st[2]), 0, _stream())
            return dx, None, None
        dw, db = grad_dest(weight), grad_dest(ctx.small[0])
        dw = torch.empty((k1, c0), device=x.device, dtype=torch.float32) if dw is None else dw
        db = torch.empty(k1, device=x.device, dtype=torch.float32) if db is None else db
        ws = torch.empty(lib().mia_head_bwd_workspace(c0, k1), device=x.device, dtype=torch.float32)
        call("mia_head_bwd", _p(dl), _p(x), _dt(x), _p(w2), _p(dx), _p(dw), _p(db), _p(ws), n, _c_i64(h * w), c0, k1,
             _c_i64(st[0]), _c_i64(st[1]), _c_i64(st[2]), 0, _stream())
        return dx, dw.reshape(weight.shape), db


# ------------------------------------------------------------------ Dice + CE
def loss_flags(softmax: bool, do_bg: bool, batch: bool, squared: bool) -> int:
    return (LOSS_SOFTMAX if softmax else 0) | (LOSS_DO_BG if do_bg else 0) | (LOSS_BATCH if batch else 0) | \
        (LOSS_SQUARED if squared else 0)


_BAD_FLAGS = {}
_LAST_BAD_LABEL = None  # the flags of the latest loss forward: ONE sticky verdict per device, read by check_labels()


def _bad_flags(dev) -> torch.Tensor:
    """Per-device int32[2], zeroed once: allocating and clearing a flag per loss call would put two fill kernels in every step.
    [0] working flag (set by the pixel kernels, re-armed by finalize), [1] sticky verdict.  Every loss forward takes its flags
    here, which also makes them the ones check_labels() looks at."""
    global _LAST_BAD_LABEL
    key = (dev.type, dev.index)
    t = _BAD_FLAGS.get(key)
    if t is None:
        t = torch.zeros(2, device=dev, dtype=torch.int32)
        _BAD_FLAGS[key] = t
    _LAST_BAD_LABEL = DiceCEFn.last_bad_label = t  # the class attribute is the holder's older name, kept readable
    return t


def _loss_logits(logits: torch.Tensor):
    """fp32 logits whose pixel dims collapse (made contiguous otherwise) and their (sn, sk, sp) strides."""
    if logits.dtype != torch.float32:
        logits = logits.float()
    st = _pix_strides(logits)
    if st is None:
        logits = logits.contiguous()
        st = _pix_strides(logits)
    return logits, st


def _loss_logits_pair(who: str, a: torch.Tensor, b: torch.Tensor, differ: str):
    """The opening of the losses between two logits tensors: `a` and `b` ([B, K, H, W], one shape) each through `_loss_logits`, as
    (a, a's strides, b, b's strides).  `differ` is the text of the shape error, with {a} and {b} for the two shapes."""
    if a.ndim != 4:
        raise NotImplementedError(f"the HIP {who} implements 2-D inputs [B, K, H, W]")
    if b.shape != a.shape:
        raise MiaError(differ.format(a=tuple(a.shape), b=tuple(b.shape)))
    return _loss_logits(a) + _loss_logits(b)


def _dyn_arg(who: str, dyn: Optional[torch.Tensor], numel: int, exact: bool) -> Optional[torch.Tensor]:
    """The run-time schedule buffer of a loss: None, or a contiguous fp32 device tensor of `numel` values (at least `numel` unless
    `exact`), detached."""
    if dyn is None:
        return None
    if dyn.dtype != torch.float32 or not dyn.is_contiguous() or (dyn.numel() != numel if exact else dyn.numel() < numel):
        what = "two contiguous fp32 values {weight, threshold} on the device" if exact else \
            "a contiguous fp32 device tensor whose first element is the weight"
        raise MiaError(f"{who}: `dyn` is {what}")
    return dyn.detach()


def _loss_slabs(hw: int) -> int:
    """Blocks per image of a loss forward: one per 8192 pixels, at most 256."""
    return max(1, min(256, hw // 8192))


def _loss_bwd_begin(logits: torch.Tensor, gout: torch.Tensor):
    """(dl, gst, g): the logits gradient to fill (it keeps the logits' dense strides), its strides, grad_out as one fp32 value."""
    dl = torch.empty_like(logits)
    return dl, _pix_strides(dl), gout.reshape(1).float().contiguous()


def _strides_i64(st):
    return _c_i64(st[0]), _c_i64(st[1]), _c_i64(st[2])


class DiceCEFn(torch.autograd.Function):
    """dice_w * DiceLoss + ce_w * CrossEntropy in one pass over the logits
    (src/losses/dice_loss.py:32-76, src/losses/compound_losses.py:33-49)."""

    @staticmethod
    def forward(ctx, logits, labels, flags: int, smooth: float, dice_w: float, ce_w: float, which: int):
        _need_dev(logits, labels)
        logits, st = _loss_logits(logits)
        b, k1, h, w = logits.shape
        if labels.shape == logits.shape and k1 > 1:
            # dense (already one-hot / soft) target: the reference skips its encoder (dice_loss.py:40-41) and
            # torch's CrossEntropyLoss treats it as class probabilities
            flags |= LOSS_DENSE
            labels = labels.to(torch.float32).contiguous()
        else:
            labels = labels.reshape(b, h, w)
            if labels.dtype != torch.long:
                labels = labels.long()
            labels = labels.contiguous()
        hw = h * w
        slabs = _loss_slabs(hw)
        dev = logits.device
        ws = torch.empty(lib().mia_dice_ce_workspace(b, k1, slabs), device=dev, dtype=torch.float32)
        sums = torch.empty((b, k1, 3), device=dev, dtype=torch.float32)
        coef = torch.empty((b, k1, 2), device=dev, dtype=torch.float32)  # every entry is written by the finalize kernel
        out = torch.empty(3, device=dev, dtype=torch.float32)
        bad = _bad_flags(dev)
        call("mia_dice_ce_fwd", _p(logits), _p(labels), b, _c_i64(hw), k1, *_strides_i64(st), flags,
             _c_float(smooth), _c_float(dice_w), _c_float(ce_w), slabs, _p(ws), _p(sums), _p(coef), _p(out), _p(bad), _stream())
        ctx.save_for_backward(logits, labels, coef)
        ctx.flags, ctx.dice_w, ctx.ce_w, ctx.st = flags, dice_w, ce_w, st
        ctx.bad = bad
        DiceCEFn.last_sums = sums
        return out[which]

    @staticmethod
    def backward(ctx, gout):
        logits, labels, coef = ctx.saved_tensors
        b, k1, h, w = logits.shape
        dl, gst, g = _loss_bwd_begin(logits, gout)
        st = ctx.st
        call("mia_dice_ce_bwd", _p(logits), _p(labels), _p(coef), _p(g), _p(dl), b, _c_i64(h * w), k1, *_strides_i64(st),
             *_strides_i64(gst), ctx.flags, _c_float(ctx.dice_w), _c_float(ctx.ce_w), _stream())
        return dl, None, None, None, None, None, None


DiceCEFn.last_bad_label = None
DiceCEFn.last_sums = None


def check_labels() -> None:
    """Raise if ANY Dice/CE forward on this device since the previous check met a label outside [0, K1) (host sync: call it
    where you already sync, e.g. next to the `loss.item()` you log).  The reference raises at the offending call (scatter
    index error in `DiceLoss._one_hot_encoder`, dice_loss.py:25-30, and the target bound check of CrossEntropyLoss); the
    kernels cannot, so they return NaN losses / NaN gradients for such a batch and keep a STICKY per-device verdict: a clean
    forward in between (validation, a second loss term) does not erase it; this call reads it and clears it.
    Ordering contract: every loss forward whose labels you want checked must have been ISSUED on the current stream before
    this call; losses running on other streams of the same device share the flag (their verdicts OR together)."""
    bad = _LAST_BAD_LABEL  # set by _bad_flags() in every loss forward; assigning DiceCEFn.last_bad_label yourself has no effect here
    if bad is not None and int(bad[1].item()) != 0:
        bad[1].zero_()
        raise MiaError("Dice/CE loss: a label lies outside [0, num_classes] (e.g. 255-valued masks or ignore_index -100); "
                       "the reference raises an index error for such targets")


DS_LOSS_FACTORS = (2, 4, 8, 16)
DS_LOSS_MAX_CLASSES = 8


class UpsampleDiceCEFn(torch.autograd.Function):
    """DiceCEFn on bilinearly upsampled logits (`Upsample(scale_factor=factor, mode="bilinear", align_corners=False)`, the
    deep-supervision heads of unet.py:193-197) without the upsampled tensor: the forward interpolates the low-resolution logits in
    registers, the backward gathers d loss / d z_lowres directly.  Index labels [B,H*factor,W*factor] only."""

    @staticmethod
    def forward(ctx, z, labels, factor: int, flags: int, smooth: float, dice_w: float, ce_w: float, which: int):
        _need_dev(z, labels)
        z, st = _loss_logits(z)
        b, k1, h, w = z.shape
        factor = int(factor)
        if factor not in DS_LOSS_FACTORS or not 1 <= k1 <= DS_LOSS_MAX_CLASSES:
            raise MiaError(f"UpsampleDiceCEFn: factor {factor} / {k1} classes not supported (factors {DS_LOSS_FACTORS}, up to "
                           f"{DS_LOSS_MAX_CLASSES} classes)")
        if flags & LOSS_DENSE or labels.numel() != b * h * factor * w * factor:
            raise MiaError(f"UpsampleDiceCEFn: index labels of {b}x{h * factor}x{w * factor} pixels expected, got {tuple(labels.shape)}")
        labels = labels.reshape(b, h * factor, w * factor)
        if labels.dtype != torch.long:
            labels = labels.long()
        labels = labels.contiguous()
        hw = h * factor * w * factor
        slabs = _loss_slabs(hw)
        dev = z.device
        ws = torch.empty(lib().mia_ds_loss_workspace(b, k1, slabs), device=dev, dtype=torch.float32)
        sums = torch.empty((b, k1, 3), device=dev, dtype=torch.float32)
        coef = torch.empty((b, k1, 2), device=dev, dtype=torch.float32)  # every entry is written by the finalize kernel
        out = torch.empty(3, device=dev, dtype=torch.float32)
        bad = _bad_flags(dev)
        call("mia_ds_loss_fwd", _p(z), _p(labels), b, h, w, factor, k1, *_strides_i64(st), flags,
             _c_float(smooth), _c_float(dice_w), _c_float(ce_w), slabs, _p(ws), _p(sums), _p(coef), _p(out), _p(bad), _stream())
        ctx.save_for_backward(z, labels, coef)
        ctx.factor, ctx.flags, ctx.dice_w, ctx.ce_w, ctx.st = factor, flags, dice_w, ce_w, st
        DiceCEFn.last_sums = sums
        return out[which]

    @staticmethod
    def backward(ctx, gout):
        z, labels, coef = ctx.saved_tensors
        b, k1, h, w = z.shape
        dz, gst, g = _loss_bwd_begin(z, gout)
        st = ctx.st
        call("mia_ds_loss_bwd", _p(z), _p(labels), _p(coef), _p(g), _p(dz), b, h, w, ctx.factor, k1, *_strides_i64(st),
             *_strides_i64(gst), ctx.flags, _c_float(ctx.dice_w), _c_float(ctx.ce_w), _stream())
        return dz, None, None, None, None, None, None, None


# ------------------------------------------------------------------ fold-trainer losses (masked soft Dice + CE, top-k CE)
def seg_loss_flags(softmax: bool, do_bg: bool, batch: bool) -> int:
    return (SEGLOSS_SOFTMAX if softmax else 0) | (SEGLOSS_DO_BG if do_bg else 0) | (SEGLOSS_BATCH if batch else 0)


def _seg_loss_inputs(logits, labels, class_w, flags: int, ignore_label):
    """Common argument handling of SegLossFn / TopKCEFn: fp32 logits with collapsible pixel strides, index labels [B,H,W] as
    uint8 (kept: one byte per pixel) or int64 (anything else is converted), class weights as K1 fp32 values."""
    _need_dev(logits, labels, class_w)
    if logits.ndim != 4:
        raise NotImplementedError("the HIP segmentation losses implement 2-D inputs [B, K, H, W]")
    logits, st = _loss_logits(logits)
    b, k1, h, w = logits.shape
    if labels.numel() != b * h * w:
        raise MiaError(f"labels {tuple(labels.shape)} do not index the pixels of logits {tuple(logits.shape)}")
    labels = labels.reshape(b, h, w)
    if labels.dtype == torch.uint8:
        flags |= SEGLOSS_LABEL_U8
    elif labels.dtype != torch.long:
        labels = labels.long()
    labels = labels.contiguous()
    if class_w is not None:
        if class_w.numel() != k1:
            raise MiaError(f"class weights: {class_w.numel()} values for {k1} classes")
        class_w = class_w.detach().to(device=logits.device, dtype=torch.float32).contiguous()
    if ignore_label is not None:
        flags |= SEGLOSS_IGNORE
    return logits, labels, class_w, st, flags, int(ignore_label) if ignore_label is not None else 0


class SegLossFn(torch.autograd.Function):
    """ce_w * CrossEntropy(weight, ignore) + dice_w * MemoryEfficientSoftDice(loss_mask = label != ignore) in one pass over the
    logits (src/losses/compound_losses.py:129-196, dice_loss.py:100-165), plus the hard tp / fp / fn of the arg-max prediction
    (dice_loss.py:168-225 as the fold trainers call it).  `which` picks the returned scalar: 0 total, 1 ce, 2 dc; the other two
    and the counts of the latest forward stay readable as `SegLossFn.last_out` ([3] fp32) and `SegLossFn.last_counts`
    ([B,K1,3] int64)."""

    @staticmethod
    def forward(ctx, logits, labels, class_w, flags: int, ignore_label, smooth: float, dice_w: float, ce_w: float, which: int):
        logits, labels, class_w, st, flags, ign = _seg_loss_inputs(logits, labels, class_w, flags, ignore_label)
        b, k1, h, w = logits.shape
        hw = h * w
        slabs = _loss_slabs(hw)
        dev = logits.device
        ws = torch.empty((lib().mia_seg_loss_workspace(b, k1, slabs) + 1) // 2, device=dev, dtype=torch.float64)  # 8-byte aligned
        coef = torch.empty(b * k1 * 2 + 1, device=dev, dtype=torch.float32)  # every entry is written by the finalize kernel
        out = torch.empty(3, device=dev, dtype=torch.float32)
        counts = torch.empty((b, k1, 3), device=dev, dtype=torch.int64)
        bad = _bad_flags(dev)
        call("mia_seg_loss_fwd", _p(logits), _p(labels), _p(class_w), b, _c_i64(hw), k1, *_strides_i64(st),
             flags, _c_i64(ign), _c_float(smooth), _c_float(dice_w), _c_float(ce_w), slabs, _p(ws), _p(coef), _p(out), _p(counts),
             _p(bad), _stream())
        ctx.save_for_backward(logits, labels, coef)
        ctx.class_w = class_w
        ctx.flags, ctx.ign, ctx.st = flags, ign, st
        SegLossFn.last_out = out
        SegLossFn.last_counts = counts
        return out[which]

    @staticmethod
    def backward(ctx, gout):
        logits, labels, coef = ctx.saved_tensors
        b, k1, h, w = logits.shape
        dl, gst, g = _loss_bwd_begin(logits, gout)
        st = ctx.st
        call("mia_seg_loss_bwd", _p(logits), _p(labels), _p(ctx.class_w), _p(coef), _p(g), _p(dl), b, _c_i64(h * w), k1,
             *_strides_i64(st), *_strides_i64(gst), ctx.flags, _c_i64(ctx.ign),
             _stream())
        return dl, None, None, None, None, None, None, None, None


SegLossFn.last_out = None
SegLossFn.last_counts = None


class TopKCEFn(torch.autograd.Function):
    """Mean of the hardest k % of the per-pixel (weighted, ignore-aware) cross-entropy (src/losses/ce_loss.py:18-32) without a
    sort: a radix select on the device finds the threshold.  Pixels that tie exactly with the threshold share the remaining
    slots equally -- this project's own deterministic rule where torch.topk's choice is unspecified."""

    @staticmethod
    def forward(ctx, logits, labels, class_w, ignore_label, k: float):
        logits, labels, class_w, st, flags, ign = _seg_loss_inputs(logits, labels, class_w, 0, ignore_label)
        b, k1, h, w = logits.shape
        n_pix = b * h * w
        n_top = int(n_pix * k / 100)
        if not 0 <= n_top <= n_pix:
            raise MiaError(f"TopKLoss: k={k} % selects {n_top} of {n_pix} pixels")
        dev = logits.device
        words = lib().mia_topk_ce_workspace(_c_i64(n_pix))
        if words <= 0:
            raise MiaError(f"TopKLoss: {n_pix} pixels are more than the radix select indexes")
        ws = torch.empty(words, device=dev, dtype=torch.float32)
        out = torch.empty(1, device=dev, dtype=torch.float32)
        bad = _bad_flags(dev)
        call("mia_topk_ce_fwd", _p(logits), _p(labels), _p(class_w), b, _c_i64(h * w), k1, *_strides_i64(st),
             flags, _c_i64(ign), _c_i64(n_top), _p(ws), _p(out), _p(bad), _stream())
        ctx.save_for_backward(logits, labels, ws)
        ctx.class_w = class_w
        ctx.flags, ctx.ign, ctx.st = flags, ign, st
        TopKCEFn.last_threshold = ws[n_pix]
        return out[0]

    @staticmethod
    def backward(ctx, gout):
        logits, labels, ws = ctx.saved_tensors
        b, k1, h, w = logits.shape
        dl, gst, g = _loss_bwd_begin(logits, gout)
        st = ctx.st
        call("mia_topk_ce_bwd", _p(logits), _p(labels), _p(ctx.class_w), _p(ws), _p(g), _p(dl), b, _c_i64(h * w), k1,
             *_strides_i64(st), *_strides_i64(gst), ctx.flags, _c_i64(ctx.ign), _stream())
        return dl, None, None, None, None


TopKCEFn.last_threshold = None


# ------------------------------------------------------------------ boundary loss (signed distance maps + softmax x phi)
SDM_MAX_HW = 4096
BOUNDARY_MAX_CLASSES = 8


def class_mask(k1: int, classes) -> Tuple[int, Tuple[int, ...]]:
    """(bit mask, ascending tuple) of the classes that take part; None = the foreground classes 1 .. k1-1 (Kervadec's `idc`)."""
    if not 1 <= k1 <= BOUNDARY_MAX_CLASSES:
        raise MiaError(f"boundary loss: {k1} classes not in [1, {BOUNDARY_MAX_CLASSES}]")
    cls = tuple(range(1, k1)) if classes is None else tuple(sorted({int(c) for c in classes}))
    if not cls or cls[0] < 0 or cls[-1] >= k1:
        raise MiaError(f"boundary loss: classes {cls} must be a non-empty subset of 0..{k1 - 1}")
    return sum(1 << c for c in cls), cls


def _boundary_labels(labels: torch.Tensor, b: int, h: int, w: int) -> torch.Tensor:
    """Index labels [B,H,W]: uint8 stays uint8 (one byte per pixel), anything else becomes int64."""
    if labels.numel() != b * h * w:
        raise MiaError(f"labels {tuple(labels.shape)} do not index {b}x{h}x{w} pixels")
    labels = labels.reshape(b, h, w)
    if labels.dtype != torch.uint8 and labels.dtype != torch.long:
        labels = labels.long()
    return labels.contiguous()


def signed_distance_map(labels: torch.Tensor, k1: int, classes=None, spacing=None) -> torch.Tensor:
    """phi [B, len(classes), H, W] fp32 of index labels [B,H,W] (include/mia_hip.h: mia_signed_distance_map).  No autograd, no
    host sync, `torch.empty` only."""
    _need_dev(labels)
    if labels.ndim != 3:
        raise MiaError(f"signed_distance_map: labels [B,H,W] expected, got {tuple(labels.shape)}")
    b, h, w = labels.shape
    mask, cls = class_mask(k1, classes)
    sh, sw = (1.0, 1.0) if spacing is None else (float(spacing[0]), float(spacing[1]))
    labels = _boundary_labels(labels, b, h, w)
    words = lib().mia_sdm_workspace(b, h, w, k1, mask)
    if words < 0:
        raise MiaError(f"signed_distance_map: {b}x{h}x{w} with {len(cls)} classes is outside the limits (h, w <= {SDM_MAX_HW}, "
                       f"B * classes <= 65535, B * classes * H * W < 2^31)")
    ws = torch.empty(words, device=labels.device, dtype=torch.float32)
    phi = torch.empty((b, len(cls), h, w), device=labels.device, dtype=torch.float32)
    call("mia_signed_distance_map", _p(labels), int(labels.dtype == torch.uint8), b, h, w, k1, mask, _c_float(sh), _c_float(sw),
         _p(ws), _p(phi), _stream())
    return phi


class BoundaryLossFn(torch.autograd.Function):
    """weight * mean over (image, selected class, pixel) of softmax(logits)_k * phi_k: one streaming forward pass and one
    streaming backward pass (csrc/boundary.hip).  `phi` [B, nc, H, W] fp32 carries no gradient; `weight` is None or a DEVICE
    fp32 tensor of one element that the kernels read when they run, so a captured step follows later writes to it.  The
    unweighted value of the latest forward stays readable as `BoundaryLossFn.last_out[1]`."""

    @staticmethod
    def forward(ctx, logits, labels, phi, mask: int, weight):
        _need_dev(logits, labels, phi, weight)
        if logits.ndim != 4:
            raise NotImplementedError("the HIP boundary loss implements 2-D inputs [B, K, H, W]")
        logits, st = _loss_logits(logits)
        b, k1, h, w = logits.shape
        labels = _boundary_labels(labels, b, h, w)
        nc = bin(mask).count("1")
        if tuple(phi.shape) != (b, nc, h, w) or phi.dtype != torch.float32:
            raise MiaError(f"boundary loss: distance map {tuple(phi.shape)} {phi.dtype}, expected fp32 {(b, nc, h, w)}")
        phi = phi.detach().contiguous()
        if weight is not None:
            if weight.dtype != torch.float32 or weight.numel() != 1:
                raise MiaError("boundary loss: `weight` is one fp32 value on the device")
            weight = weight.detach()
        hw = h * w
        slabs = _loss_slabs(hw)
        dev = logits.device
        ws = torch.empty(lib().mia_boundary_loss_workspace(b, slabs), device=dev, dtype=torch.float32)
        coef = torch.empty(1, device=dev, dtype=torch.float32)  # written by the finalize kernel
        out = torch.empty(3, device=dev, dtype=torch.float32)
        bad = _bad_flags(dev)
        call("mia_boundary_loss_fwd", _p(logits), _p(labels), int(labels.dtype == torch.uint8), _p(phi), _p(weight), b, _c_i64(hw), k1,
             mask, *_strides_i64(st), slabs, _p(ws), _p(coef), _p(out), _p(bad), _stream())
        ctx.save_for_backward(logits, phi, coef)
        ctx.weight = weight
        ctx.mask, ctx.st = mask, st
        BoundaryLossFn.last_out = out
        return out[0]

    @staticmethod
    def backward(ctx, gout):
        logits, phi, coef = ctx.saved_tensors
        b, k1, h, w = logits.shape
        dl, gst, g = _loss_bwd_begin(logits, gout)
        call("mia_boundary_loss_bwd", _p(logits), _p(phi), _p(coef), _p(ctx.weight), _p(g), _p(dl), b, _c_i64(h * w), k1, ctx.mask,
             *_strides_i64(ctx.st), *_strides_i64(gst), _stream())
        return dl, None, None, None, None


BoundaryLossFn.last_out = None


# ------------------------------------------------------------------ mean-teacher consistency (softmax MSE, uncertainty mask, EMA)
CONSISTENCY_MAX_CLASSES = 8


def _two_logits_slabs(hw: int) -> int:
    """Blocks per image of the forward of a loss between two logits tensors (consistency, cross pseudo supervision): one per 2048
    pixels (two four-pixel groups per thread), at most 1024.  Finer than `_loss_slabs`: the forward evaluates two soft-maxes in double
    per pixel, and the unlabelled half of a batch is few images."""
    return max(1, min(1024, hw // 2048))


class ConsistencyFn(torch.autograd.Function):
    """weight * softmax-MSE between student and teacher logits [B, K, H, W], optionally masked by the entropy of `prob_mean`
    (include/mia_hip.h: mia_consistency_fwd; csrc/consistency.hip): one streaming forward pass and one streaming backward pass.
    Only the student's logits get a gradient.  `dyn` is None or a DEVICE fp32 tensor {weight, threshold} that the kernels read when
    they run, so a captured step follows later writes to it; `prob_mean` (contiguous fp32 [B, K, H, W]) needs it.  By-products of
    the latest forward, all on the device: `last_out` = {weight * L, L, weight}, `last_kept` (int64, one element), `last_keep` (the
    byte map [B, H, W], None in the plain form)."""

    @staticmethod
    def forward(ctx, student, teacher, prob_mean, dyn, den_scale: float):
        _need_dev(student, teacher, prob_mean, dyn)
        student, st, teacher, tt = _loss_logits_pair("consistency loss", student, teacher.detach(),
                                                     "consistency loss: teacher logits {b} and student logits {a} differ")
        b, k1, h, w = student.shape
        dyn = _dyn_arg("consistency loss", dyn, 2, True)
        hw = h * w
        dev = student.device
        keep = None
        if prob_mean is not None:
            if tuple(prob_mean.shape) != (b, k1, h, w) or prob_mean.dtype != torch.float32:
                raise MiaError(f"consistency loss: prob_mean {tuple(prob_mean.shape)} {prob_mean.dtype}, expected fp32 {(b, k1, h, w)}")
            if dyn is None:
                raise MiaError("consistency loss: prob_mean needs `dyn` (the threshold is read from dyn[1])")
            prob_mean = prob_mean.detach().contiguous()
            if b > 0 and hw > 0:
                keep = torch.empty((b, h, w), device=dev, dtype=torch.uint8)  # every byte is written by the forward kernel
        slabs = _two_logits_slabs(hw)
        words = max(lib().mia_consistency_workspace(b, slabs), 0)  # < 0: a bad shape, reported by the call below
        buf = torch.empty(words + 4, device=dev, dtype=torch.float32)  # workspace | out[3] | coef: one allocation, every word written
        ws, out, coef = buf[:words], buf[words:words + 3], buf[words + 3:]
        kept = torch.empty(1, device=dev, dtype=torch.int64)
        call("mia_consistency_fwd", _p(student), _p(teacher), _p(prob_mean), _p(dyn), b, _c_i64(hw), k1, *_strides_i64(st),
             *_strides_i64(tt), _c_float(den_scale), slabs, _p(ws), _p(keep), _p(coef), _p(out), _p(kept), _stream())
        ctx.save_for_backward(student, teacher, coef)
        ctx.keep, ctx.dyn, ctx.st, ctx.tt = keep, dyn, st, tt
        ConsistencyFn.last_out, ConsistencyFn.last_kept, ConsistencyFn.last_keep = out, kept, keep
        return out[0]

    @staticmethod
    def backward(ctx, gout):
        student, teacher, coef = ctx.saved_tensors
        b, k1, h, w = student.shape
        dl, gst, g = _loss_bwd_begin(student, gout)
        call("mia_consistency_bwd", _p(student), _p(teacher), _p(ctx.keep), _p(coef), _p(ctx.dyn), _p(g), _p(dl), b, _c_i64(h * w), k1,
             *_strides_i64(ctx.st), *_strides_i64(ctx.tt), *_strides_i64(gst), _stream())
        return dl, None, None, None, None


ConsistencyFn.last_out = ConsistencyFn.last_kept = ConsistencyFn.last_keep = None


# ------------------------------------------------------------------ virtual adversarial training (KL distance, noise, perturbation)
class KLConsistencyFn(torch.autograd.Function):
    """weight * KL(softmax(target) || softmax(logits)) / den between two fp32 logits tensors [B, K, H, W] (include/mia_hip.h:
    mia_kl_fwd; csrc/vat.hip): one streaming pass each way.  Only `logits` gets a gradient.  `dyn` is None or a DEVICE fp32 tensor whose
    first element is the weight, read when the kernels run; `den` is the divisor of the sum over pixels and classes (B * H * W for a
    per-pixel mean, B for "batchmean").  `last_out` = {weight * L, L, weight} of the latest forward, on the device."""

    @staticmethod
    def forward(ctx, logits, target, dyn, den: float):
        _need_dev(logits, target, dyn)
        logits, st, target, tt = _loss_logits_pair("KL consistency", logits, target.detach(),
                                                   "KL consistency: target logits {b} and logits {a} differ")
        b, k1, h, w = logits.shape
        dyn = _dyn_arg("KL consistency", dyn, 1, False)
        hw = h * w
        dev = logits.device
        slabs = _two_logits_slabs(hw)
        words = max(lib().mia_kl_workspace(b, slabs), 0)  # < 0: a bad shape, reported by the call below
        buf = torch.empty(words + 4, device=dev, dtype=torch.float32)  # workspace | out[3] | coef: one allocation, every word written
        ws, out, coef = buf[:words], buf[words:words + 3], buf[words + 3:]
        call("mia_kl_fwd", _p(logits), _p(target), _p(dyn), b, _c_i64(hw), k1, *_strides_i64(st), *_strides_i64(tt),
             ctypes.c_double(float(den)), slabs, _p(ws), _p(coef), _p(out), _stream())
        ctx.save_for_backward(logits, target, coef)
        ctx.dyn, ctx.st, ctx.tt = dyn, st, tt
        KLConsistencyFn.last_out = out
        return out[0]

    @staticmethod
    def backward(ctx, gout):
        logits, target, coef = ctx.saved_tensors
        b, k1, h, w = logits.shape
        dl, gst, g = _loss_bwd_begin(logits, gout)
        call("mia_kl_bwd", _p(logits), _p(target), _p(coef), _p(ctx.dyn), _p(g), _p(dl), b, _c_i64(h * w), k1, *_strides_i64(ctx.st),
             *_strides_i64(ctx.tt), *_strides_i64(gst), _stream())
        return dl, None, None, None


KLConsistencyFn.last_out = None


def vat_noise(shape, device) -> torch.Tensor:
    """fp32 tensor of `shape` with values in U[-0.5, 0.5) from the library's Philox kernel (`mia_vat_noise`), keyed by the device
    generator's (seed, offset) and advancing the offset on the host exactly as `dropout_mask` does: `torch.manual_seed` reproduces it."""
    dev = torch.device(device)
    out = torch.empty(tuple(shape), device=dev, dtype=torch.float32)
    nb = int(shape[0])
    per = out.numel() // max(nb, 1)
    gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
    seed, off = int(gen.initial_seed()), int(gen.get_offset())
    gen.set_offset(off + 4 * ((out.numel() + 3) // 4))
    call("mia_vat_noise", _p(out), nb, _c_i64(per), ctypes.c_uint64(seed & (2 ** 64 - 1)), ctypes.c_uint64(off), _stream())
    return out


def sample_sumsq(x: torch.Tensor) -> torch.Tensor:
    """[B] fp32: the sum of squares of every sample of a contiguous fp32 tensor [B, ...] (`mia_sample_sumsq`: double, rounded once)."""
    _need_dev(x)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise MiaError("sample_sumsq: a contiguous fp32 tensor expected")
    nb = x.shape[0]
    per = x.numel() // max(nb, 1)
    words = max(lib().mia_sample_sumsq_workspace(nb, _c_i64(per)), 0)
    ws = torch.empty(words, device=x.device, dtype=torch.float32)
    out = torch.empty(nb, device=x.device, dtype=torch.float32)
    call("mia_sample_sumsq", _p(x), nb, _c_i64(per), _p(ws), _p(out), _stream())
    return out


def vat_perturb(x: torch.Tensor, g: torch.Tensor, sumsq: torch.Tensor, gscale: float, scale: float = 1.0,
                scale_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x + s * (gscale * g) / (gscale * sqrt(sumsq[n]) + 1e-8) per sample n (`mia_vat_perturb`); s = `scale_dev[0]` (a device fp32
    value read when the kernel runs) when given, else `scale`.  x, g: contiguous fp32 of one shape [B, ...]; sumsq: [B] fp32."""
    _need_dev(x, g, sumsq, scale_dev)
    for t in (x, g, sumsq):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise MiaError("vat_perturb: contiguous fp32 tensors expected")
    if g.shape != x.shape or sumsq.numel() != x.shape[0]:
        raise MiaError(f"vat_perturb: x {tuple(x.shape)}, g {tuple(g.shape)}, sumsq {tuple(sumsq.shape)} do not match")
    if scale_dev is not None and (scale_dev.dtype != torch.float32 or scale_dev.numel() < 1):
        raise MiaError("vat_perturb: a device `scale_dev` is one fp32 value")
    nb = x.shape[0]
    out = torch.empty_like(x)
    call("mia_vat_perturb", _p(x), _p(g), _p(sumsq), _c_float(gscale), _c_float(scale), _p(scale_dev), _p(out), nb,
         _c_i64(x.numel() // max(nb, 1)), _stream())
    return out


class frozen_parameters:
    """Context manager: every parameter of `model` has `requires_grad == False` inside and its earlier setting back on every exit
    path.  A forward AND its backward inside it (e.g. `torch.autograd.grad(loss, image)`) compute input gradients only: autograd
    records at forward time which inputs need a gradient, and the backward nodes of this file then launch no weight-gradient kernel, claim no `grad_dest` slice and return None for their parameters."""

    def __init__(self, model):
        self.model, self._saved = model, None

    def __enter__(self):
        self._saved = [(p, p.requires_grad) for p in self.model.parameters()]
        for p, _ in self._saved:
            p.requires_grad_(False)
        return self.model

    def __exit__(self, *exc):
        for p, r in self._saved:
            p.requires_grad_(r)
        self._saved = None
        return False


def ema_update(teacher_flat: torch.Tensor, student_flat: torch.Tensor, alpha) -> None:
    """teacher_flat = alpha * teacher_flat + (1 - alpha) * student_flat in place over flat fp32 buffers (include/mia_hip.h:
    mia_ema_update); `alpha` is a float in [0, 1] or a DEVICE fp32 tensor of one element read when the kernel runs.  alpha == 0
    copies the student bit for bit.  The kernel bypasses tensor version counters: the caller bumps the parameter epoch (or re-packs)
    when the buffer backs a model's parameters."""
    _need_dev(teacher_flat, student_flat)
    for t in (teacher_flat, student_flat):
        if t.dtype != torch.float32 or t.ndim != 1 or not t.is_contiguous():
            raise MiaError("ema_update: flat contiguous fp32 buffers expected")
    if teacher_flat.numel() != student_flat.numel():
        raise MiaError(f"ema_update: {teacher_flat.numel()} teacher values against {student_flat.numel()} student values")
    adev = None
    if isinstance(alpha, torch.Tensor):
        _need_dev(alpha)
        if alpha.dtype != torch.float32 or alpha.numel() != 1:
            raise MiaError("ema_update: a device `alpha` is one fp32 value")
        adev, alpha = alpha, 0.0
    call("mia_ema_update", _p(teacher_flat), _p(student_flat), _c_i64(teacher_flat.numel()), _c_float(float(alpha)), _p(adev), _stream())


# ------------------------------------------------------------------ pyramid consistency (URPC) between a network's own scales
URPC_MAX_SCALES = 5


def _urpc_slabs(hw: int) -> int:
    """Blocks per image of the pyramid-consistency forward: one per 2048 pixels, at most 256 (a pixel costs S soft-maxes and the
    unlabelled part of a batch is few images)."""
    return max(1, min(256, hw // 2048))


def _host_arrays(tensors, strides):
    """(device pointers, (sn, sk, sp) triples) as the host arrays the URPC entry points read during the call."""
    n = len(tensors)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors])
    return ptrs, (ctypes.c_int64 * (3 * n))(*[int(v) for st in strides for v in st])


class PyramidConsistencyFn(torch.autograd.Function):
    """`apply(dyn, *logits)` -> weight * L, the uncertainty rectified pyramid consistency (URPC) between the S = len(logits) outputs
    one network makes at several scales (include/mia_hip.h: mia_urpc_fwd; csrc/urpc.hip).  logits[0] is the full-resolution output
    [B, K, H, W]; every other entry is [B, K, H / f, W / f] with f in `DS_LOSS_FACTORS`, in any order; fp32, any layout whose H and W
    collapse (planar, the head's channels-last view, a batch slice of either).  Every entry gets a gradient.  `dyn` is None (weight
    1) or a DEVICE fp32 tensor whose first element is the weight, read when the kernels run.  By-products of the latest forward, on the
    device: `last_out` = {weight * L, L} and `last_terms` [S] (the per-scale L_s).  Nothing of full-resolution size is allocated in
    either direction."""

    @staticmethod
    def forward(ctx, dyn, *logits):
        _need_dev(dyn, *logits)
        ns = len(logits)
        if not 2 <= ns <= URPC_MAX_SCALES:
            raise MiaError(f"pyramid consistency: {ns} outputs, the kernel takes 2 to {URPC_MAX_SCALES}")
        if any(z.ndim != 4 for z in logits):
            raise NotImplementedError("the HIP pyramid consistency implements 2-D inputs [B, K, H, W]")
        b, k1, hh, ww = logits[0].shape
        factors = []
        for z in logits:
            if z.shape[0] != b or z.shape[1] != k1 or hh % z.shape[2] or ww % z.shape[3] or hh // z.shape[2] != ww // z.shape[3]:
                raise MiaError(f"pyramid consistency: output {tuple(z.shape)} against the full-resolution {tuple(logits[0].shape)}")
            factors.append(hh // z.shape[2])
        dyn = _dyn_arg("pyramid consistency", dyn, 1, False)
        zs, sts = zip(*[_loss_logits(z) for z in logits])
        dev = zs[0].device
        slabs = _urpc_slabs(hh * ww)
        words = max(lib().mia_urpc_workspace(b, ns, slabs), 0)  # < 0: a bad shape, reported by the call below
        buf = torch.empty(words + 4 * ns + 2, device=dev, dtype=torch.float32)  # workspace | sums | terms | out: every word written
        ws, sums = buf[:words], buf[words:words + 3 * ns]
        terms, out = buf[words + 3 * ns:words + 4 * ns], buf[words + 4 * ns:]
        zp, zst = _host_arrays(zs, sts)
        fac = (ctypes.c_int * ns)(*factors)
        call("mia_urpc_fwd", zp, fac, zst, ns, b, hh, ww, k1, _p(dyn), slabs, _p(ws), _p(sums), _p(terms), _p(out), _stream())
        ctx.save_for_backward(sums, *zs)
        ctx.dyn, ctx.factors, ctx.sts = dyn, factors, sts
        PyramidConsistencyFn.last_out, PyramidConsistencyFn.last_terms = out, terms
        return out[0]

    @staticmethod
    def backward(ctx, gout):
        sums, *zs = ctx.saved_tensors
        ns = len(zs)
        b, k1, hh, ww = zs[0].shape
        dzs = [torch.empty_like(z) for z in zs]
        g = gout.reshape(1).float().contiguous()
        zp, zst = _host_arrays(zs, ctx.sts)
        dp, dst = _host_arrays(dzs, [_pix_strides(d) for d in dzs])
        fac = (ctypes.c_int * ns)(*ctx.factors)
        call("mia_urpc_bwd", zp, fac, zst, dp, dst, ns, b, hh, ww, k1, _p(sums), _p(ctx.dyn), _p(g), _stream())
        return (None, *dzs)


PyramidConsistencyFn.last_out = PyramidConsistencyFn.last_terms = None


# ------------------------------------------------------------------ cross pseudo supervision (two networks, hard pseudo-labels)
CPS_MAX_CLASSES = 8


class CrossPseudoFn(torch.autograd.Function):
    """`apply(za, zb, dyn)` -> weight * (LA + LB), cross pseudo supervision between the logits [B, K, H, W] of two networks
    (include/mia_hip.h: mia_cps_fwd; csrc/cps.hip): each is trained with cross-entropy on the arg-max of the other, where the other's
    largest soft-max value reaches the threshold.  One streaming forward pass, and one streaming backward pass that writes BOTH
    gradients.  fp32, any layout whose H and W collapse (planar, the head's channels-last view, a batch slice of either; the two may
    differ).  `dyn` is None (weight 1, threshold 0: every pixel) or a DEVICE fp32 tensor {weight, threshold} that the kernels read
    when they run.  By-products of the latest forward, all on the device: `last_out` = {weight * (LA + LB), LA, LB, weight},
    `last_counts` (int64 [3]: confident pixels of A, of B, pixels where the two labels agree) and `last_code` (uint8 [B, H, W],
    see `cps_decode`), which is also what the backward reads."""

    @staticmethod
    def forward(ctx, za, zb, dyn):
        _need_dev(za, zb, dyn)
        za, sa, zb, sb = _loss_logits_pair("cross pseudo supervision loss", za, zb,
                                           "cross pseudo supervision: logits {a} and {b} differ")
        b, k1, h, w = za.shape
        dyn = _dyn_arg("cross pseudo supervision", dyn, 2, True)
        hw = h * w
        dev = za.device
        slabs = _two_logits_slabs(hw)
        words = max(lib().mia_cps_workspace(b, slabs), 0)  # < 0: a bad shape, reported by the call below
        buf = torch.empty(words + 4, device=dev, dtype=torch.float32)  # workspace | out[4]: one allocation, every word written
        ws, out = buf[:words], buf[words:]
        counts = torch.empty(3, device=dev, dtype=torch.int64)
        code = torch.empty((b, h, w), device=dev, dtype=torch.uint8)  # every byte is written by the forward kernel
        call("mia_cps_fwd", _p(za), _p(zb), _p(dyn), b, _c_i64(hw), k1, *_strides_i64(sa), *_strides_i64(sb), slabs, _p(ws), _p(code),
             _p(out), _p(counts), _stream())
        ctx.save_for_backward(za, zb)
        ctx.code, ctx.dyn, ctx.sa, ctx.sb = code, dyn, sa, sb
        CrossPseudoFn.last_out, CrossPseudoFn.last_counts, CrossPseudoFn.last_code = out, counts, code
        return out[0]

    @staticmethod
    def backward(ctx, gout):
        za, zb = ctx.saved_tensors
        b, k1, h, w = za.shape
        dza, gsa, g = _loss_bwd_begin(za, gout)
        dzb = torch.empty_like(zb)
        call("mia_cps_bwd", _p(za), _p(zb), _p(ctx.code), _p(ctx.dyn), _p(g), _p(dza), _p(dzb), b, _c_i64(h * w), k1,
             *_strides_i64(ctx.sa), *_strides_i64(ctx.sb), *_strides_i64(gsa), *_strides_i64(_pix_strides(dzb)), _stream())
        return dza, dzb, None


CrossPseudoFn.last_out = CrossPseudoFn.last_counts = CrossPseudoFn.last_code = None


def cps_decode(code: torch.Tensor):
    """(ya, yb, ca, cb) of `CrossPseudoFn.last_code`: the two label maps (int64) and the two confidence maps (bool), in plain tensor
    ops on whatever device `code` lives on -- for logging and tests, not the hot path."""
    c = code.to(torch.int64)
    return c & 7, (c >> 3) & 7, ((c >> 6) & 1).bool(), ((c >> 7) & 1).bool()


# ------------------------------------------------------------------ bidirectional copy-paste (mix under a mask, two-source loss)
BCP_MAX_CLASSES = 8


def _bcp_mask(who: str, mask: torch.Tensor, b: int, h: int, w: int):
    """(mask, image stride): a contiguous uint8 mask [H, W] (stride 0: one mask for the batch) or [B, H, W] (stride H * W)."""
    if mask.dtype != torch.uint8 or tuple(mask.shape) not in ((h, w), (b, h, w)):
        raise MiaError(f"{who}: the mask is uint8 [{h}, {w}] or [{b}, {h}, {w}], got {mask.dtype} {tuple(mask.shape)}")
    return mask.contiguous(), (h * w if mask.ndim == 3 else 0)


def _mix_out(who: str, x: torch.Tensor, out: Optional[torch.Tensor], whose: str):
    """(out, its image stride) of a mix of batches shaped like the contiguous `x`: a new tensor, or the caller's dense-image one."""
    b, c, h, w = x.shape
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or out.device != x.device or \
            out.stride()[1:] != x.stride()[1:] or (b > 1 and out.stride(0) < c * h * w):
        raise MiaError(f"{who}: `out` is fp32 of the {whose} shape with dense images (a batch slice of a contiguous tensor)")
    return out, (out.stride(0) if b > 1 else c * h * w)


def _hard_loss_logits(who: str, logits: torch.Tensor, limit: int):
    """The opening of the hard-label losses (csrc/hard_loss.h): fp32 logits [B, K, H, W] with K <= limit through `_loss_logits`."""
    if logits.ndim != 4:
        raise NotImplementedError(f"the HIP {who} implements 2-D inputs [B, K, H, W]")
    logits, st = _loss_logits(logits)
    if not 1 <= logits.shape[1] <= limit:
        raise MiaError(f"{who}: {logits.shape[1]} classes not in [1, {limit}] (the tensor-op form, fused=False, takes more)")
    return logits, st


def _hard_loss_buf(workspace: str, dev, b: int, k1: int, hw: int, ncoef: int, nout: int):
    """(slabs, workspace, coef, out, counts) of a hard-label loss forward: workspace | coef | out are views of ONE fp32 allocation
    whose every word the kernels write, `workspace` names the entry point that sizes it; counts is int64 [2]."""
    slabs = _two_logits_slabs(hw)
    words = max(getattr(lib(), workspace)(b, k1, slabs), 0)  # < 0: a bad shape, reported by the loss call
    buf = torch.empty(words + ncoef + nout, device=dev, dtype=torch.float32)
    return slabs, buf[:words], buf[words:words + ncoef], buf[words + ncoef:], torch.empty(2, device=dev, dtype=torch.int64)


def bcp_mix(fg: torch.Tensor, bg: torch.Tensor, mask: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[n, c, p] = fg[n, c, p] where mask[n or 0, p] != 0, else bg[n, c, p] (include/mia_hip.h: mia_bcp_mix; csrc/bcp.hip).
    fg, bg: contiguous fp32 [B, C, H, W]; mask: uint8 [H, W] or [B, H, W]; out: None (a new tensor) or fp32 [B, C, H, W] whose
    images are dense, e.g. a batch slice of a larger contiguous tensor.  A SELECTION, not `fg * m + bg * (1 - m)`: the bits of the
    chosen operand pass through, NaN payloads and -0.0 included, and a NaN in the operand not chosen does not spread.  No gradient."""
    _need_dev(fg, bg, mask, out)
    if fg.ndim != 4 or bg.shape != fg.shape or fg.dtype != torch.float32 or bg.dtype != torch.float32 or \
            not fg.is_contiguous() or not bg.is_contiguous():
        raise MiaError(f"bcp_mix: two contiguous fp32 [B, C, H, W] batches of one shape expected, got {tuple(fg.shape)} {fg.dtype} "
                       f"and {tuple(bg.shape)} {bg.dtype}")
    b, c, h, w = fg.shape
    mask, msn = _bcp_mask("bcp_mix", mask, b, h, w)
    out, osn = _mix_out("bcp_mix", fg, out, "inputs'")
    if fg.numel() == 0:
        return out
    call("mia_bcp_mix", _p(fg.detach()), _p(bg.detach()), _p(mask), _p(out), b, c, _c_i64(h * w), _c_i64(msn), _c_i64(osn), _stream())
    return out


class CopyPasteLossFn(torch.autograd.Function):
    """`apply(logits, label_a, label_b, mask, weight_a, weight_b, smooth)` -> the two-source loss of a copy-paste mixed batch
    (include/mia_hip.h: mia_bcp_loss_fwd; csrc/bcp.hip; the definition is the module text of losses/copy_paste.py): a pixel is
    supervised by `label_a` where `mask != 0` and by `label_b` elsewhere, each region with its own weight, its own squared-denominator
    Dice over the whole call and its own mean cross-entropy.  One streaming forward pass and one streaming backward pass; only the
    logits get a gradient.  fp32 logits [B, K, H, W], K <= 8, any layout whose H and W collapse; labels [B, H, W] int64 or uint8
    (anything else, or a mixed pair, is converted to int64); mask uint8 [H, W] or [B, H, W].  By-products of the latest forward, on
    the device: `last_out` = {L, D_A, C_A, D_B, C_B} and `last_counts` (int64 [2]: pixels of region A, of region B)."""

    @staticmethod
    def forward(ctx, logits, label_a, label_b, mask, weight_a: float, weight_b: float, smooth: float):
        _need_dev(logits, label_a, label_b, mask)
        logits, st = _hard_loss_logits("copy-paste loss", logits, BCP_MAX_CLASSES)
        b, k1, h, w = logits.shape
        if label_a.numel() != b * h * w or label_b.numel() != b * h * w:
            raise MiaError(f"copy-paste loss: labels {tuple(label_a.shape)} / {tuple(label_b.shape)} do not index the pixels of "
                           f"logits {tuple(logits.shape)}")
        u8 = label_a.dtype == torch.uint8 and label_b.dtype == torch.uint8
        label_a, label_b = (t.reshape(b, h, w) if u8 else t.reshape(b, h, w).long() for t in (label_a, label_b))
        label_a, label_b = label_a.contiguous(), label_b.contiguous()
        mask, msn = _bcp_mask("copy-paste loss", mask, b, h, w)
        hw, dev = h * w, logits.device
        slabs, ws, coef, out, counts = _hard_loss_buf("mia_bcp_loss_workspace", dev, b, k1, hw, 4 * k1 + 2, 5)
        call("mia_bcp_loss_fwd", _p(logits), _p(label_a), _p(label_b), _p(mask), b, _c_i64(hw), k1, *_strides_i64(st), _c_i64(msn),
             int(u8), _c_float(smooth), _c_float(weight_a), _c_float(weight_b), slabs, _p(ws), _p(coef), _p(out), _p(counts),
             _p(_bad_flags(dev)), _stream())
        ctx.save_for_backward(logits, label_a, label_b, mask, coef)
        ctx.st, ctx.msn, ctx.u8 = st, msn, u8
        CopyPasteLossFn.last_out, CopyPasteLossFn.last_counts = out, counts
        return out[0]

    @staticmethod
    def backward(ctx, gout):
        logits, label_a, label_b, mask, coef = ctx.saved_tensors
        b, k1, h, w = logits.shape
        dl, gst, g = _loss_bwd_begin(logits, gout)
        call("mia_bcp_loss_bwd", _p(logits), _p(label_a), _p(label_b), _p(mask), _p(coef), _p(g), _p(dl), b, _c_i64(h * w), k1,
             *_strides_i64(ctx.st), *_strides_i64(gst), _c_i64(ctx.msn), int(ctx.u8), _stream())
        return dl, None, None, None, None, None, None


CopyPasteLossFn.last_out = CopyPasteLossFn.last_counts = None


# ------------------------------------------------------------------ weak-to-strong consistency (pseudo-label codes, CutMix, loss)
W2S_MAX_CLASSES = 8
_PERM_FLAGS = {}


def _perm_flags(dev) -> torch.Tensor:
    """Per-device int32[2], zeroed once, laid out like `_bad_flags`: [1] is the sticky verdict "a device `perm` held an entry outside
    the batch" that the CutMix and weak-to-strong kernels raise and `check_perm()` reads and clears ([0] is unused: these kernels
    have no working flag to fold)."""
    key = (dev.type, dev.index)
    t = _PERM_FLAGS.get(key)
    if t is None:
        t = torch.zeros(2, device=dev, dtype=torch.int32)
        _PERM_FLAGS[key] = t
    return t


def check_perm() -> None:
    """Raise if a `cutmix_perm` or `WeakToStrongFn` call on any device since the previous check met a DEVICE `perm` with an entry
    outside [0, B) (host sync: call it where you already sync).  The kernels never use such an entry as an index: the image is paired
    with itself, and the verdict is kept until this call reads and clears it.  A host `perm` is checked when it is given."""
    for t in _PERM_FLAGS.values():
        if int(t[1].item()) != 0:
            t[1].zero_()
            raise MiaError("CutMix: a device `perm` held an entry outside [0, B); that image was paired with itself")


def _perm_arg(who: str, perm, b: int, dev) -> torch.Tensor:
    """`perm` as a contiguous int32 [B] tensor on `dev`.  A device tensor is taken as it is (int32 [B], contiguous; the kernels guard
    its entries).  A host sequence or a CPU tensor is validated here -- B integers in [0, B), not necessarily a permutation -- and
    uploaded."""
    if isinstance(perm, torch.Tensor) and perm.is_cuda:
        if perm.dtype != torch.int32 or perm.ndim != 1 or perm.numel() != b or not perm.is_contiguous() or perm.device != dev:
            raise MiaError(f"{who}: a device `perm` is a contiguous int32 [{b}] tensor on {dev}, got {perm.dtype} "
                           f"{tuple(perm.shape)} on {perm.device}")
        return perm
    t = torch.as_tensor(perm)
    if t.ndim != 1 or t.numel() != b or t.is_floating_point() or t.dtype == torch.bool:
        raise MiaError(f"{who}: `perm` holds {b} integers, one per image; got {t.dtype} {tuple(t.shape)}")
    t = t.to(torch.int64)
    if b and (int(t.min()) < 0 or int(t.max()) >= b):
        raise MiaError(f"{who}: `perm` entries must lie in [0, {b}); got {t.tolist()}")
    return t.to(torch.int32).to(dev, non_blocking=True)


def w2s_labels(zw: torch.Tensor, dyn: Optional[torch.Tensor] = None):
    """(code, kept): the pseudo-labels of the weak view's logits `zw` [B, K, H, W] (include/mia_hip.h: mia_w2s_labels; csrc/w2s.hip).
    `code` is uint8 [B, H, W] = argmax_k zw_k | keep << 7 with keep = (max_k softmax(zw)_k >= dyn[1]) -- ties to the lowest class, the
    threshold read on the device (`dyn` None: 0, every pixel kept); `kept` is the 0-dim int64 count of kept pixels.  fp32, K <= 8, any
    layout whose H and W collapse.  No gradient; an image's code does not depend on the rest of the batch (see `w2s_decode`)."""
    _need_dev(zw, dyn)
    if zw.ndim != 4:
        raise NotImplementedError("the HIP weak-to-strong labels implement 2-D inputs [B, K, H, W]")
    zw, st = _loss_logits(zw.detach())
    b, k1, h, w = zw.shape
    if not 1 <= k1 <= W2S_MAX_CLASSES:
        raise MiaError(f"w2s_labels: {k1} classes not in [1, {W2S_MAX_CLASSES}] (pseudo_label_code of losses/weak_strong.py takes more)")
    dyn = _dyn_arg("w2s_labels", dyn, 2, True)
    hw = h * w
    dev = zw.device
    slabs = _two_logits_slabs(hw)
    ws = torch.empty(max(b * slabs, 1), device=dev, dtype=torch.int32)
    code = torch.empty((b, h, w), device=dev, dtype=torch.uint8)  # every byte is written by the kernel
    kept = torch.empty(1, device=dev, dtype=torch.int64)
    call("mia_w2s_labels", _p(zw), _p(dyn), b, _c_i64(hw), k1, *_strides_i64(st), slabs, _p(ws), _p(code), _p(kept), _stream())
    return code, kept[0]


def w2s_decode(code: torch.Tensor):
    """(y, keep) of a weak-to-strong code map: the label map (int64) and the confidence map (bool), in plain tensor ops on whatever
    device `code` lives on -- for logging and tests, not the hot path."""
    c = code.to(torch.int64)
    return c & 7, ((c >> 7) & 1).bool()


def cutmix_perm(x: torch.Tensor, perm, mask: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[n, c, p] = x[perm[n], c, p] where mask[n or 0, p] != 0, else x[n, c, p]: CutMix of a batch with a permutation of itself,
    without the gathered copy `x[perm]` (include/mia_hip.h: mia_cutmix_perm; csrc/w2s.hip).  x: contiguous fp32 [B, C, H, W]; perm: B
    integers (a host sequence or CPU tensor, validated here and uploaded; or a device int32 [B] tensor taken as it is -- see
    `check_perm`); mask: uint8 [H, W] or [B, H, W]; out: None (a new tensor) or fp32 [B, C, H, W] whose images are dense, e.g. a batch
    slice of a larger contiguous tensor, and which does not overlap `x`.  A SELECTION like `bcp_mix`: the bits of the chosen operand
    pass through.  No gradient."""
    _need_dev(x, mask, out)
    if x.ndim != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise MiaError(f"cutmix_perm: a contiguous fp32 [B, C, H, W] batch expected, got {tuple(x.shape)} {x.dtype}")
    b, c, h, w = x.shape
    perm = _perm_arg("cutmix_perm", perm, b, x.device)
    mask, msn = _bcp_mask("cutmix_perm", mask, b, h, w)
    out, osn = _mix_out("cutmix_perm", x, out, "input's")
    if x.numel() == 0:
        return out
    call("mia_cutmix_perm", _p(x.detach()), _p(perm), _p(mask), _p(out), b, c, _c_i64(h * w), _c_i64(msn), _c_i64(osn),
         _p(_perm_flags(x.device)), _stream())
    return out


class WeakToStrongFn(torch.autograd.Function):
    """`apply(logits, code, mask, perm, dyn, ce_weight, dice_weight, smooth)` -> the weak-to-strong loss of a strong view
    (include/mia_hip.h: mia_w2s_loss_fwd; csrc/w2s.hip; the definition is the module text of losses/weak_strong.py): pixel (n, p) is
    supervised by `code[perm[n], p]` where `mask[n or 0, p] != 0` and by `code[n, p]` elsewhere, wherever that code's confidence bit
    is set.  `mask` or `perm` None: no mix.  One streaming forward pass and one streaming backward pass; only the logits get a
    gradient.  fp32 logits [B, K, H, W], K <= 8, any layout whose H and W collapse; code uint8 [B, H, W] (`w2s_labels`); mask uint8
    [H, W] or [B, H, W]; perm as for `cutmix_perm`; `dyn` None (weight 1) or the DEVICE fp32 {weight, threshold} -- the loss reads
    the weight only.  By-products of the latest forward, on the device: `last_out` = {L, CE, D, weight} and `last_counts` (int64 [2]:
    kept pixels of the mixed view, pixels taken from the partner)."""

    @staticmethod
    def forward(ctx, logits, code, mask, perm, dyn, ce_weight: float, dice_weight: float, smooth: float):
        _need_dev(logits, code, mask, dyn)
        logits, st = _hard_loss_logits("weak-to-strong loss", logits, W2S_MAX_CLASSES)
        b, k1, h, w = logits.shape
        if code.dtype != torch.uint8 or tuple(code.shape) != (b, h, w):
            raise MiaError(f"weak-to-strong loss: the code map is uint8 [{b}, {h}, {w}] (ops.w2s_labels), got {code.dtype} "
                           f"{tuple(code.shape)}")
        code, dev, hw, msn = code.contiguous(), logits.device, h * w, 0
        if mask is None or perm is None:
            mask = perm = None
        else:
            mask, msn = _bcp_mask("weak-to-strong loss", mask, b, h, w)
            perm = _perm_arg("weak-to-strong loss", perm, b, dev)
        dyn = _dyn_arg("weak-to-strong loss", dyn, 2, True)
        slabs, ws, coef, out, counts = _hard_loss_buf("mia_w2s_loss_workspace", dev, b, k1, hw, 2 * k1 + 1, 4)
        call("mia_w2s_loss_fwd", _p(logits), _p(code), _p(mask), _p(perm), _p(dyn), b, _c_i64(hw), k1, *_strides_i64(st), _c_i64(msn),
             _c_float(smooth), _c_float(ce_weight), _c_float(dice_weight), slabs, _p(ws), _p(coef), _p(out), _p(counts),
             _p(_perm_flags(dev)), _stream())
        ctx.save_for_backward(logits, code, coef)
        ctx.mask, ctx.perm, ctx.st, ctx.msn = mask, perm, st, msn
        WeakToStrongFn.last_out, WeakToStrongFn.last_counts = out, counts
        return out[0]

    @staticmethod
    def backward(ctx, gout):
        logits, code, coef = ctx.saved_tensors
        b, k1, h, w = logits.shape
        dl, gst, g = _loss_bwd_begin(logits, gout)
        call("mia_w2s_loss_bwd", _p(logits), _p(code), _p(ctx.mask), _p(ctx.perm), _p(coef), _p(g), _p(dl), b, _c_i64(h * w), k1,
             *_strides_i64(ctx.st), *_strides_i64(gst), _c_i64(ctx.msn), _stream())
        return dl, None, None, None, None, None, None, None


WeakToStrongFn.last_out = WeakToStrongFn.last_counts = None


# ------------------------------------------------------------------ dual-task consistency (level-set head against the soft-max)
DTC_MAX_CLASSES = 8


def sdm_extent(phi: torch.Tensor) -> torch.Tensor:
    """fp32 `[..., 2]` = {max phi, max -phi} over the last two dims of a signed distance map `phi` [B, C, H, W], both >= +0
    (include/mia_hip.h: mia_sdm_extent; csrc/dtc.hip): how far the map reaches outside and inside each object.  Integer max on the
    bit patterns, so the result is exact and does not depend on the order.  No autograd, no host sync."""
    _need_dev(phi)
    if phi.ndim != 4 or phi.dtype != torch.float32:
        raise MiaError(f"sdm_extent: an fp32 distance map [B, C, H, W] expected, got {tuple(phi.shape)} {phi.dtype}")
    phi = phi.detach().contiguous()
    b, c, h, w = phi.shape
    ext = torch.empty((b, c, 2), device=phi.device, dtype=torch.float32)  # zeroed and filled by the call
    if phi.numel() == 0:
        return ext.zero_()
    call("mia_sdm_extent", _p(phi), b * c, _c_i64(h * w), _p(ext), _stream())
    return ext


class DTCLossFn(torch.autograd.Function):
    """`apply(z, r, phi, extent, lb, k, dyn)` -> the dual-task consistency loss (include/mia_hip.h: mia_dtc_fwd; csrc/dtc.hip; the
    definition is the module text of losses/dual_task.py): `dyn[0] * L_cons + dyn[1] * L_sdf` between the segmentation logits `z`
    [B, K, H, W] and the level-set logits `r` [B, K - 1, H, W], both fp32 in any layout whose H and W collapse, 2 <= K <= 8.  The
    first `lb` images are labelled: `phi` is their fp32 signed distance map [lb, K - 1, H, W] at unit spacing (`signed_distance_map`)
    and `extent` its `sdm_extent` (None: computed here); with `lb = 0` both may be None.  One streaming forward pass and one streaming
    backward pass; `z` and `r` get a gradient, `phi` none.  `dyn` is None (both weights 1) or the DEVICE fp32 {consistency weight,
    beta} that the kernels read when they run.  By-product of the latest forward, on the device: `last_out` = {L, L_cons, L_sdf}."""

    @staticmethod
    def forward(ctx, z, r, phi, extent, lb: int, k: float, dyn):
        _need_dev(z, r, phi, extent, dyn)
        if z.ndim != 4 or r.ndim != 4:
            raise NotImplementedError("the HIP dual-task loss implements 2-D inputs [B, K, H, W]")
        z, st = _loss_logits(z)
        r, rt = _loss_logits(r)
        b, k1, h, w = z.shape
        if not 2 <= k1 <= DTC_MAX_CLASSES:
            raise MiaError(f"dual-task loss: {k1} classes not in [2, {DTC_MAX_CLASSES}] (the tensor-op form, fused=False, takes more)")
        if tuple(r.shape) != (b, k1 - 1, h, w):
            raise MiaError(f"dual-task loss: level-set logits {tuple(r.shape)}, expected {(b, k1 - 1, h, w)} for logits {tuple(z.shape)}")
        lb = int(lb)
        if not 0 <= lb <= b:
            raise MiaError(f"dual-task loss: labeled_bs={lb} not in [0, {b}]")
        if lb > 0:
            if phi is None or tuple(phi.shape) != (lb, k1 - 1, h, w) or phi.dtype != torch.float32:
                raise MiaError(f"dual-task loss: the distance map of the {lb} labelled images is fp32 {(lb, k1 - 1, h, w)}, got "
                               f"{None if phi is None else (tuple(phi.shape), phi.dtype)}")
            phi = phi.detach().contiguous()
            if extent is None:
                extent = sdm_extent(phi)
            elif tuple(extent.shape) != (lb, k1 - 1, 2) or extent.dtype != torch.float32:
                raise MiaError(f"dual-task loss: extents {tuple(extent.shape)} {extent.dtype}, expected fp32 {(lb, k1 - 1, 2)}")
            extent = extent.detach().contiguous()
        else:
            phi = extent = None
        dyn = _dyn_arg("dual-task loss", dyn, 2, True)
        hw, dev = h * w, z.device
        slabs = _two_logits_slabs(hw)
        words = max(b * slabs * 4, 0)
        buf = torch.empty(words + 5, device=dev, dtype=torch.float32)  # workspace | out[3] | coef[2]: one allocation, every word written
        ws, out, coef = buf[:words], buf[words:words + 3], buf[words + 3:]
        call("mia_dtc_fwd", _p(z), _p(r), _p(phi), _p(extent), b, lb, _c_i64(hw), k1, _c_float(k), *_strides_i64(st),
             *_strides_i64(rt), slabs, _p(ws), _stream())
        call("mia_dtc_finalize", _p(ws), _p(dyn), b, lb, _c_i64(hw), k1, slabs, _p(coef), _p(out), _stream())
        ctx.save_for_backward(z, r, coef)
        ctx.phi, ctx.extent, ctx.lb, ctx.k, ctx.st, ctx.rt = phi, extent, lb, float(k), st, rt
        DTCLossFn.last_out = out
        return out[0]

    @staticmethod
    def backward(ctx, gout):
        z, r, coef = ctx.saved_tensors
        b, k1, h, w = z.shape
        dz, gst, g = _loss_bwd_begin(z, gout)
        dr = torch.empty_like(r)
        call("mia_dtc_bwd", _p(z), _p(r), _p(ctx.phi), _p(ctx.extent), _p(coef), _p(g), _p(dz), _p(dr), b, ctx.lb, _c_i64(h * w), k1,
             _c_float(ctx.k), *_strides_i64(ctx.st), *_strides_i64(ctx.rt), *_strides_i64(gst), *_strides_i64(_pix_strides(dr)),
             _stream())
        return dz, dr, None, None, None, None, None


DTCLossFn.last_out = None


# ------------------------------------------------------------------ region-based loss (sigmoid soft Dice + BCE)
REGLOSS_MAX_CHANNELS = 8


def region_loss_flags(do_bg: bool, batch: bool) -> int:
    return (REGLOSS_DO_BG if do_bg else 0) | (REGLOSS_BATCH if batch else 0)


def region_bits(regions, device) -> torch.Tensor:
    """Device table for the index form: entry l (int32, read as uint32) has bit c set when label l belongs to `regions[c]`."""
    regions = [tuple(int(v) for v in r) for r in regions]
    if not 1 <= len(regions) <= REGLOSS_MAX_CHANNELS:
        raise NotImplementedError(f"the HIP region loss implements 1..{REGLOSS_MAX_CHANNELS} regions, got {len(regions)}")
    if any(v < 0 for r in regions for v in r):
        raise ValueError("regions: labels must be >= 0")
    n = max((v for r in regions for v in r), default=0) + 1
    bits = [0] * n
    for c, r in enumerate(regions):
        for v in r:
            bits[v] |= 1 << c
    return torch.tensor(bits, dtype=torch.int32, device=device)


class RegionLossFn(torch.autograd.Function):
    """ce_w * BCEWithLogits(pos_weight) + dice_w * MemoryEfficientSoftDice(sigmoid) over the valid pixels in one pass over the logits
    (src/losses/compound_losses.py:178-233), plus the hard tp / fp / fn of (logit > 0) against (target > 0.5).  `target` is dense
    [B,C,H,W] (or [B,C+1,H,W] with REGLOSS_IGNORE: the last channel marks ignored pixels) in bool, uint8 or fp32 -- handed to the
    kernel as it is -- or, with a `bits` table (`region_bits`), a label map [B,H,W] in uint8 or int64 whose `ignore_label` pixels are
    invalid.  `which` picks the returned scalar: 0 total, 1 ce, 2 dc; the other two and the counts of the latest forward stay
    readable as `RegionLossFn.last_out` ([3] fp32) and `RegionLossFn.last_counts` ([B,C,3] int64)."""

    @staticmethod
    def forward(ctx, logits, target, bits, pos_weight, flags: int, ignore_label, smooth: float, dice_w: float, ce_w: float, which: int):
        _need_dev(logits, target, bits, pos_weight)
        if logits.ndim != 4:
            raise NotImplementedError("the HIP region loss implements 2-D inputs [B, C, H, W]")
        logits, st = _loss_logits(logits)
        b, c, h, w = logits.shape
        if c > REGLOSS_MAX_CHANNELS:
            raise NotImplementedError(f"the HIP region loss implements up to {REGLOSS_MAX_CHANNELS} channels, got {c}")
        flags &= REGLOSS_DO_BG | REGLOSS_BATCH | REGLOSS_IGNORE
        n_labels, ign = 0, 0
        if bits is not None:
            flags |= REGLOSS_INDEX
            if target.numel() != b * h * w:
                raise MiaError(f"labels {tuple(target.shape)} do not index the pixels of logits {tuple(logits.shape)}")
            target = target.reshape(b, h, w)
            if target.dtype == torch.uint8:
                flags |= REGLOSS_TARGET_U8
            elif target.dtype != torch.long:
                target = target.long()
            bits = bits.to(device=logits.device, dtype=torch.int32).contiguous()
            n_labels = bits.numel()
            if ignore_label is not None:
                flags |= REGLOSS_IGNORE
                ign = int(ignore_label)
        else:
            ct = c + (1 if flags & REGLOSS_IGNORE else 0)
            if tuple(target.shape) != (b, ct, h, w):
                raise MiaError(f"dense target {tuple(target.shape)} for logits {tuple(logits.shape)}: expected {(b, ct, h, w)}")
            if target.dtype in (torch.bool, torch.uint8):
                flags |= REGLOSS_TARGET_U8
            elif target.dtype != torch.float32:
                target = target.float()
        target = target.contiguous()
        if pos_weight is not None:
            if pos_weight.numel() != c:
                raise MiaError(f"pos_weight: {pos_weight.numel()} values for {c} channels")
            pos_weight = pos_weight.detach().to(device=logits.device, dtype=torch.float32).reshape(c).contiguous()
        hw = h * w
        slabs = _loss_slabs(hw)
        dev = logits.device
        ws = torch.empty((lib().mia_region_loss_workspace(b, c, slabs) + 1) // 2, device=dev, dtype=torch.float64)  # 8-byte aligned
        coef = torch.empty(b * c * 2 + 1, device=dev, dtype=torch.float32)  # every entry is written by the finalize kernel
        out = torch.empty(3, device=dev, dtype=torch.float32)
        counts = torch.empty((b, c, 3), device=dev, dtype=torch.int64)
        bad = _bad_flags(dev)
        call("mia_region_loss_fwd", _p(logits), _p(target), _p(bits), n_labels, _p(pos_weight), b, _c_i64(hw), c,
             *_strides_i64(st), flags, _c_i64(ign), _c_float(smooth), _c_float(dice_w), _c_float(ce_w), slabs, _p(ws), _p(coef),
             _p(out), _p(counts), _p(bad), _stream())
        ctx.save_for_backward(logits, target, coef)
        ctx.bits, ctx.pos_weight = bits, pos_weight
        ctx.flags, ctx.ign, ctx.st, ctx.n_labels = flags, ign, st, n_labels
        RegionLossFn.last_out = out
        RegionLossFn.last_counts = counts
        return out[which]

    @staticmethod
    def backward(ctx, gout):
        logits, target, coef = ctx.saved_tensors
        b, c, h, w = logits.shape
        dl, gst, g = _loss_bwd_begin(logits, gout)
        st = ctx.st
        call("mia_region_loss_bwd", _p(logits), _p(target), _p(ctx.bits), ctx.n_labels, _p(ctx.pos_weight), _p(coef), _p(g), _p(dl), b,
             _c_i64(h * w), c, *_strides_i64(st), *_strides_i64(gst), ctx.flags,
             _c_i64(ctx.ign), _stream())
        return dl, None, None, None, None, None, None, None, None, None


RegionLossFn.last_out = None
RegionLossFn.last_counts = None


def hard_tp_fp_fn(logits: torch.Tensor, target: torch.Tensor, ignore_label=None) -> torch.Tensor:
    """int64 [B, K1, 3] = (tp, fp, fn) of the arg-max prediction per image and class, pixels labelled `ignore_label` left out
    (get_tp_fp_fn_tn(onehot(argmax), target, mask) of the fold trainers' online Dice) -- one kernel pass, no one-hot tensors."""
    with torch.no_grad():
        SegLossFn.apply(logits.detach(), target, None, 0, ignore_label, 1.0, 1.0, 1.0, 0)
    return SegLossFn.last_counts


# ------------------------------------------------------------------ optimizer helpers
def grad_norm(flat_grad: torch.Tensor, max_norm: float, grad_scale: float = 1.0) -> torch.Tensor:
    """out[0] = ||grad_scale*g||_2, out[1] = clip coefficient; stays on device (no sync)."""
    ws = torch.empty(lib().mia_grad_norm_workspace(), device=flat_grad.device, dtype=torch.float32)
    out = torch.empty(2, device=flat_grad.device, dtype=torch.float32)
    call("mia_grad_norm", _p(flat_grad), _c_i64(flat_grad.numel()), _c_float(max_norm), _c_float(grad_scale), _p(ws), _p(out),
         _stream())
    return out


def optim_step(kind: int, param, grad, m, v, lr, beta1, beta2, eps, wd, step: int, clip: Optional[torch.Tensor],
               grad_scale: float = 1.0):
    if _STEP_DYN is not None:  # captured step: lr / bias corrections / first-step flag are read from device memory
        call("mia_optim_step_dyn", _p(param), _p(grad), _p(m), _p(v), _c_i64(param.numel()), kind, _c_float(beta1), _c_float(beta2),
             _c_float(eps), _c_float(wd), _STEP_DYN.f32_ptr, _p(clip), _c_float(grad_scale), _stream())
        return
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    call("mia_optim_step", _p(param), _p(grad), _p(m), _p(v), _c_i64(param.numel()), kind, _c_float(lr), _c_float(beta1),
         _c_float(beta2), _c_float(eps), _c_float(wd), _c_float(bc1), _c_float(bc2), int(step == 1), _p(clip),
         _c_float(grad_scale), _stream())


def global_avg_pool(x_nhwc: torch.Tensor) -> torch.Tensor:
    """[N,H,W,C] -> [N,C] fp32 mean over H,W (adaptive_avg_pool2d(.,1).view(B,-1); reference unet.py:87-91)."""
    _need_dev(x_nhwc)
    x = x_nhwc.contiguous()
    n, h, w, c = x.shape
    part = torch.empty((n, 1, c, 2), device=x.device, dtype=torch.float32)
    call("mia_norm_stats", _p(x), _dt(x), n, _c_i64(h * w), c, 1, _p(part), _stream())
    return part[:, 0, :, 0] / float(h * w)


# ------------------------------------------------------------------ ResidualBlock pieces (reference blocks.py:108-164)
class PointwiseNormFn(torch.autograd.Function):
    """Conv2d(cin, cout, 1, stride) + Instance/BatchNorm without activation: the ``downsample_skip`` branch of the
    reference ResidualBlock (blocks.py:147-153).  Stride 1 runs the 1x1 MFMA mode; stride 2 runs the 2x2/s2 gather with
    only tap (0,0) populated (the other three taps are zero weights), so no extra kernels are needed."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, stride: int, cfg: NormCfg):
        _need_dev(x, weight)
        x = x.contiguous()
        dtype = _dt(x)
        n, h, w, cin = x.shape
        cout = weight.shape[0]
        if stride == 2 and (h % 2 or w % 2):
            raise MiaError("ResidualBlock stride-2 skip needs even H, W on the MI355X path")
        ho, wo = (h // 2, w // 2) if stride == 2 else (h, w)
        w4 = PointwiseNormFn._as_taps(weight, stride)
        wp, npad, kpad = PackCache().get(w4, dtype, n_from_d0=True)
        y, _, stats = conv_mma(CONV_G2S2 if stride == 2 else CONV_G1, x, None, wp, npad, kpad, False, bias.detach().float(), cout,
                               (ho, wo), want_stats=True)
        z, coefs = PlainBlockFn._norm_act(ctx, y, stats, gamma, beta, cfg, 1.0)
        ctx.save_for_backward(x, y, coefs, weight, gamma)
        ctx.stride, ctx.mode, ctx.fixed = stride, cfg.mode, cfg.fixed
        return z

    @staticmethod
    def _as_taps(weight, stride):
        w = weight.detach()
        if stride == 1:
            return w.contiguous()
        w4 = torch.zeros((w.shape[0], w.shape[1], 2, 2), device=w.device, dtype=w.dtype)
        w4[:, :, 0, 0] = w[:, :, 0, 0]
        return w4

    @staticmethod
    def backward(ctx, dz):
        x, y, coefs, weight, gamma = ctx.saved_tensors
        dz = dz.contiguous()
        dtype = _dt(y)
        n, ho, wo, cout = y.shape
        cin = weight.shape[1]
        nb = _NormBwd(y, coefs, ctx.mode, ctx.fixed, 1.0)  # parameter gradients in private rows (this node registers no destinations)
        dy = torch.empty_like(y)
        nb.plain(dz, None, dy)
        w4 = PointwiseNormFn._as_taps(weight, ctx.stride)
        need_w = any(ctx.needs_input_grad[1:5])  # (frozen parameters: no weight gradient)
        dw = None
        if not need_w:
            pass
        elif ctx.stride == 2:
            g4 = conv_wgrad(WGRAD_2S2, x, None, dy, w4.shape, cout, cin)
            dw = g4[:, :, 0:1, 0:1].contiguous()
        else:  # 1x1 stride 1: centre tap of the 3x3 weight-gradient kernel
            g9 = conv_wgrad(WGRAD_3S1, x, None, dy, (cout, cin, 3, 3), cout, cin)
            dw = g9[:, :, 1:2, 1:2].contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            wb, npad, kpad = PackCache().get(w4, dtype, n_from_d0=False)
            if ctx.stride == 2:
                dx, _, _ = conv_mma(CONV_T2S2, dy, None, wb, npad, kpad, False, None, cin, (x.shape[1], x.shape[2]))
            else:
                dx, _, _ = conv_mma(CONV_G1, dy, None, wb, npad, kpad, False, None, cin, (ho, wo))
        if not need_w:
            return dx, None, None, None, None, None, None
        return dx, dw, nb.dbias, nb.dgamma, nb.dbeta, None, None


class ScaleLReLUFn(torch.autograd.Function):
    """z = LeakyReLU(m[n,c] * v): Dropout2d AFTER the norm followed by the activation (ResidualBlock order
    conv -> norm -> dropout -> lrelu, blocks.py:141); m = None means no dropout."""

    @staticmethod
    def forward(ctx, v, m, slope: float):
        _need_dev(v)
        v = v.contiguous()
        n, h, w, c = v.shape
        coef = torch.zeros((2, n, c), device=v.device, dtype=torch.float32)
        if m is None:
            coef[0].fill_(1.0)
        else:
            coef[0].copy_(m)
        z = _norm_act_fwd(v, coef[0], coef[1], slope)
        ctx.save_for_backward(v, coef)
        ctx.slope = slope
        return z

    @staticmethod
    def backward(ctx, dz):
        v, coef = ctx.saved_tensors
        dz = dz.contiguous()
        n, h, w, c = v.shape
        dev = v.device
        slabs = _slabs_for(h * w)
        part = torch.empty((n, slabs, c, 2), device=dev, dtype=torch.float32)
        cc = torch.empty((2, n, c), device=dev, dtype=torch.float32)
        junk = torch.empty((2, c), device=dev, dtype=torch.float32)
        dv = torch.empty_like(v)
        # frozen statistics: dv = scale * dz * lrelu'(scale*v)
        call("mia_norm_act_bwd", _p(dz), None, _p(v), _p(dv), _dt(v), _p(coef[0]), _p(coef[1]), _p(coef[0]), _p(coef[1]), None, n,
             _c_i64(h * w), c, NORM_INSTANCE, 1, _c_float(ctx.slope), slabs, _p(part), _p(cc[0]), _p(cc[1]), _p(junk[0]), _p(junk[1]),
             None, 0, _p(_amax_new(dv)), _stream())
        return dv, None, None


class AddFn(torch.autograd.Function):
    """residual + out (blocks.py:164)."""

    @staticmethod
    def forward(ctx, a, b):
        _need_dev(a, b)
        a, b = a.contiguous(), b.contiguous()
        if a.shape != b.shape or a.dtype != b.dtype:
            raise RuntimeError(f"The size of tensor a {tuple(a.shape)} must match the size of tensor b {tuple(b.shape)}")
        out = torch.empty_like(a)
        call("mia_add", _p(a), _p(b), _p(out), _dt(a), _c_i64(a.numel()), _stream())
        return out

    @staticmethod
    def backward(ctx, g):
        return g, g
