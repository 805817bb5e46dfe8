"""Fold-ensemble prediction (reference `src/entry/fugc2025/predict.py`, class ``model``): every fold model's ``softmax(1)`` summed,
``argmax``, nearest resize back to the original size, then the morphological mask clean-up.

On the GPU the reduction is one streaming pass per model (``mia_softmax_accum``, csrc/predict.hip) straight from the head's native
logits layout, with the arg-max written by the last pass, and the clean-up is one launch (``mia_mask_denoise``).  CPU tensors take
the same definition as torch ops; the networks themselves run on the GPU only.

``sliding_window_predict`` is the native-resolution path the reference's configs name (``patch_size`` and the inference parameter
``stride``, al_trainer.py:112,167,253) and never got: overlapping windows blended with a Gaussian importance map, optional mirroring
of each window, the fold models on top.  Each (model, mirror combination, window) is one ``mia_window_accum`` pass into a full-size
canvas and ``mia_window_finalize`` takes the arg-max and the separable normalisation."""
from __future__ import annotations

import ctypes
import math
import os
from typing import Optional, Sequence

import numpy as np
import torch

from models.unet import UNet, UnetProcessor

DEFAULT_CHANNELS = (32, 64, 128, 256, 512)  # al_train's widths


def softmax_accum(logits: torch.Tensor, prob_sum: Optional[torch.Tensor], pred: Optional[torch.Tensor], weight: float = 1.0,
                  first: bool = False) -> None:
    """``prob_sum = (0 if first else prob_sum) + weight * logits.softmax(1)`` in place, and ``pred = prob_sum.argmax(1)`` where
    ``pred`` is given (ties to the lowest class).  logits [B,K,H,W] fp32 on the GPU, any strides whose H and W collapse (the head's
    channels-last view included); prob_sum contiguous [B,K,H,W] fp32 or None (only with ``first`` and ``pred``); pred contiguous
    [B,H,W] int64 or None."""
    from mia_hip import call
    from mia_hip.ops import _c_i64, _need_dev, _p, _pix_strides, _stream
    _need_dev(logits, prob_sum, pred)
    if logits.dtype != torch.float32:
        logits = logits.float()
    st = _pix_strides(logits)
    if st is None:
        logits = logits.contiguous()
        st = _pix_strides(logits)
    b, k1, h, w = logits.shape
    if prob_sum is not None and not (prob_sum.dtype == torch.float32 and prob_sum.is_contiguous() and prob_sum.shape == logits.shape):
        raise ValueError("prob_sum must be a contiguous fp32 tensor of the logits' shape")
    if pred is not None and not (pred.dtype == torch.int64 and pred.is_contiguous() and tuple(pred.shape) == (b, h, w)):
        raise ValueError("pred must be a contiguous int64 tensor [B,H,W]")
    call("mia_softmax_accum", _p(logits), _p(prob_sum), _p(pred), b, _c_i64(h * w), k1, _c_i64(st[0]), _c_i64(st[1]), _c_i64(st[2]),
         ctypes.c_float(float(weight)), int(bool(first)), _stream())


def _logits_of(model, x):
    out = model(x)
    return out[0] if isinstance(out, (list, tuple)) else out


def ensemble_predict(models: Sequence[torch.nn.Module], x: torch.Tensor, weights: Optional[Sequence[float]] = None,
                     return_probs: bool = False):
    """Label map [B,H,W] (int64) of ``sum_m weights[m] * models[m](x).softmax(1)`` (predict.py:144-161 with all weights 1).

    Every model runs in eval mode under ``torch.no_grad()`` and gets its train / eval mode back on every exit path.  Models are
    accumulated in order with one logits tensor alive at a time; the result is bit-identical from run to run.
    ``return_probs=True`` returns ``(labels, prob_sum [B,K,H,W] fp32)``."""
    models = list(models)
    if not models:
        raise ValueError("ensemble_predict needs at least one model")
    weights = [1.0] * len(models) if weights is None else [float(v) for v in weights]
    if len(weights) != len(models):
        raise ValueError(f"{len(weights)} weights for {len(models)} models")
    modes = [m.training for m in models]
    prob_sum = pred = None
    try:
        for m in models:
            m.eval()
        with torch.no_grad():
            for i, (m, wt) in enumerate(zip(models, weights)):
                logits = _logits_of(m, x)
                if logits.dim() != 4:
                    raise ValueError(f"model {i} returned shape {tuple(logits.shape)}; expected logits [B,K,H,W]")
                last = i == len(models) - 1
                if logits.is_cuda:
                    b, k1, h, w = logits.shape
                    if prob_sum is None and (len(models) > 1 or return_probs):
                        prob_sum = torch.empty((b, k1, h, w), device=logits.device, dtype=torch.float32)
                    if last:
                        pred = torch.empty((b, h, w), device=logits.device, dtype=torch.int64)
                    if prob_sum is not None and tuple(prob_sum.shape) != tuple(logits.shape):
                        raise ValueError(f"model {i} returned shape {tuple(logits.shape)}, the models before it {tuple(prob_sum.shape)}")
                    softmax_accum(logits, prob_sum, pred, wt, first=i == 0)
                else:  # the same definition in torch ops
                    p = wt * logits.float().softmax(1)
                    prob_sum = p if prob_sum is None else prob_sum + p
                    if last:
                        pred = prob_sum.argmax(1)
                del logits
    finally:
        for m, was in zip(models, modes):
            m.train(was)
    return (pred, prob_sum) if return_probs else pred


def regions_to_labels(prob_sum: torch.Tensor, class_order, threshold: float) -> torch.Tensor:
    """nnU-Net's region-to-label rule in torch ops: ``pred = 0; for i: pred[prob_sum[:, i] > threshold] = class_order[i]`` --
    later regions overwrite earlier ones.  [B,C,H,W] -> int64 [B,H,W]; the definition `mia_sigmoid_accum` follows."""
    pred = torch.zeros((prob_sum.shape[0],) + tuple(prob_sum.shape[2:]), dtype=torch.int64, device=prob_sum.device)
    for i, lab in enumerate(class_order):
        pred[prob_sum[:, i] > threshold] = int(lab)
    return pred


def sigmoid_accum(logits: torch.Tensor, prob_sum: Optional[torch.Tensor], pred: Optional[torch.Tensor],
                  class_order: Optional[torch.Tensor] = None, weight: float = 1.0, threshold: float = 0.5, first: bool = False) -> None:
    """``prob_sum = (0 if first else prob_sum) + weight * logits.sigmoid()`` in place, and where ``pred`` is given the
    region-to-label rule on the updated sum (`regions_to_labels` with ``class_order``, a device int64 tensor of C labels).
    logits [B,C,H,W] fp32 on the GPU, any strides whose H and W collapse (the head's channels-last view included); prob_sum
    contiguous [B,C,H,W] fp32 or None (only with ``first`` and ``pred``); pred contiguous [B,H,W] int64 or None."""
    from mia_hip import call
    from mia_hip.ops import _c_i64, _need_dev, _p, _pix_strides, _stream
    _need_dev(logits, prob_sum, pred, class_order)
    if logits.dtype != torch.float32:
        logits = logits.float()
    st = _pix_strides(logits)
    if st is None:
        logits = logits.contiguous()
        st = _pix_strides(logits)
    b, c, h, w = logits.shape
    if prob_sum is not None and not (prob_sum.dtype == torch.float32 and prob_sum.is_contiguous() and prob_sum.shape == logits.shape):
        raise ValueError("prob_sum must be a contiguous fp32 tensor of the logits' shape")
    if pred is not None:
        if not (pred.dtype == torch.int64 and pred.is_contiguous() and tuple(pred.shape) == (b, h, w)):
            raise ValueError("pred must be a contiguous int64 tensor [B,H,W]")
        if class_order is None or not (class_order.dtype == torch.int64 and class_order.is_contiguous() and class_order.numel() == c):
            raise ValueError(f"class_order must be a contiguous int64 tensor of {c} labels")
    call("mia_sigmoid_accum", _p(logits), _p(prob_sum), _p(pred), _p(class_order), b, _c_i64(h * w), c, _c_i64(st[0]), _c_i64(st[1]),
         _c_i64(st[2]), ctypes.c_float(float(weight)), ctypes.c_float(float(threshold)), int(bool(first)), _stream())


def ensemble_predict_regions(models: Sequence[torch.nn.Module], x: torch.Tensor, class_order: Sequence[int],
                             weights: Optional[Sequence[float]] = None, return_probs: bool = False):
    """Label map [B,H,W] (int64) of region-based models: ``prob_sum = sum_m weights[m] * models[m](x).sigmoid()`` and then
    `regions_to_labels(prob_sum, class_order, 0.5 * sum(weights))`, i.e. the mean probability thresholded at 1/2 and the regions
    written in order, later ones over earlier ones (``class_order[i]`` is the label of output channel i).

    Like `ensemble_predict`: every model runs in eval mode under ``torch.no_grad()`` and gets its train / eval mode back on every
    exit path; models are accumulated in order with one logits tensor alive at a time; bit-identical from run to run; CPU logits
    take the same definition in torch ops.  ``return_probs=True`` returns ``(labels, prob_sum [B,C,H,W] fp32)``."""
    models = list(models)
    if not models:
        raise ValueError("ensemble_predict_regions needs at least one model")
    weights = [1.0] * len(models) if weights is None else [float(v) for v in weights]
    if len(weights) != len(models):
        raise ValueError(f"{len(weights)} weights for {len(models)} models")
    class_order = [int(v) for v in class_order]
    threshold = 0.5 * sum(weights)
    modes = [m.training for m in models]
    prob_sum = pred = order = None
    try:
        for m in models:
            m.eval()
        with torch.no_grad():
            for i, (m, wt) in enumerate(zip(models, weights)):
                logits = _logits_of(m, x)
                if logits.dim() != 4:
                    raise ValueError(f"model {i} returned shape {tuple(logits.shape)}; expected logits [B,C,H,W]")
                if logits.shape[1] != len(class_order):
                    raise ValueError(f"model {i} has {logits.shape[1]} output channels, class_order names {len(class_order)} regions")
                last = i == len(models) - 1
                if logits.is_cuda:
                    b, c, h, w = logits.shape
                    if prob_sum is None and (len(models) > 1 or return_probs):
                        prob_sum = torch.empty((b, c, h, w), device=logits.device, dtype=torch.float32)
                    if last:
                        pred = torch.empty((b, h, w), device=logits.device, dtype=torch.int64)
                        order = torch.tensor(class_order, dtype=torch.int64, device=logits.device)
                    if prob_sum is not None and tuple(prob_sum.shape) != tuple(logits.shape):
                        raise ValueError(f"model {i} returned shape {tuple(logits.shape)}, the models before it {tuple(prob_sum.shape)}")
                    sigmoid_accum(logits, prob_sum, pred, order, wt, threshold, first=i == 0)
                else:  # the same definition in torch ops
                    p = wt * logits.float().sigmoid()
                    prob_sum = p if prob_sum is None else prob_sum + p
                    if last:
                        pred = regions_to_labels(prob_sum, class_order, threshold)
                del logits
    finally:
        for m, was in zip(models, modes):
            m.train(was)
    return (pred, prob_sum) if return_probs else pred


def window_starts(n: int, p: int, overlap: float) -> list:
    """Start offsets of windows of length ``p`` that cover ``n`` pixels with at least ``overlap`` (a fraction of ``p``) between
    neighbours: ``k = ceil((n - p) / (p * (1 - overlap))) + 1`` windows spread evenly, the first at 0 and the last at ``n - p``."""
    n, p = int(n), int(p)
    if p < 1 or n < p:
        raise ValueError(f"window_starts: window {p} does not fit {n} pixels")
    if not 0.0 <= overlap < 1.0:
        raise ValueError(f"window_starts: overlap={overlap} not in [0, 1)")
    if n == p:
        return [0]
    k = int(math.ceil((n - p) / (p * (1.0 - overlap)))) + 1
    return [int(round((n - p) / (k - 1) * i)) for i in range(k)]


def window_weights(p: int, importance: str = "gaussian", sigma_scale: float = 0.125) -> np.ndarray:
    """One axis of the importance map (the map is the outer product of two of these), fp32 [p]: ``"gaussian"`` is
    ``exp(-0.5 * ((i - (p - 1) / 2) / (p * sigma_scale))**2)`` evaluated in float64 and rounded once, ``"constant"`` is all ones."""
    p = int(p)
    if p < 1:
        raise ValueError(f"window_weights: p={p}")
    if importance == "constant":
        return np.ones(p, dtype=np.float32)
    if importance != "gaussian":
        raise ValueError(f"importance={importance!r}: expected 'gaussian' or 'constant'")
    if not sigma_scale > 0:
        raise ValueError(f"window_weights: sigma_scale={sigma_scale}")
    i = np.arange(p, dtype=np.float64)
    return np.exp(-0.5 * ((i - (p - 1) / 2.0) / (p * float(sigma_scale))) ** 2).astype(np.float32)


def coverage_1d(g: np.ndarray, starts: Sequence[int], n: int) -> np.ndarray:
    """``R[y] = sum_a g[y - starts[a]]`` over the windows that hold ``y``, float64 [n].  The window grid is a Cartesian product and
    the importance map an outer product, so the two-dimensional coverage is ``Ry[:, None] * Rx[None, :]``."""
    g = np.asarray(g, dtype=np.float32).astype(np.float64)
    r = np.zeros(int(n), dtype=np.float64)
    for s in starts:
        r[s:s + g.shape[0]] += g
    return r


def window_accum(logits: torch.Tensor, canvas: torch.Tensor, gy: torch.Tensor, gx: torch.Tensor, y0: int, x0: int,
                 weight: float = 1.0, flip_h: bool = False, flip_w: bool = False) -> None:
    """``canvas[:, :, y0:y0+ph, x0:x0+pw] += weight * gy[:, None] * gx[None, :] * flipped(logits.softmax(1))`` in place, where
    ``flipped`` mirrors H / W inside the window as the flags say.  logits [B,K,ph,pw] fp32 on the GPU with any strides whose H and W
    collapse (a batch slice of the head's channels-last view included), canvas contiguous [B,K,H,W] fp32, gy [ph] and gx [pw] fp32
    on the GPU.  A window that does not lie inside the canvas is an error."""
    from mia_hip import call
    from mia_hip.ops import _c_i64, _need_dev, _p, _pix_strides, _stream
    _need_dev(logits, canvas, gy, gx)
    if logits.dim() != 4 or canvas.dim() != 4:
        raise ValueError(f"window_accum: logits {tuple(logits.shape)} and canvas {tuple(canvas.shape)} must be [B,K,*,*]")
    if logits.dtype != torch.float32:
        logits = logits.float()
    st = _pix_strides(logits)
    if st is None:
        logits = logits.contiguous()
        st = _pix_strides(logits)
    b, k1, ph, pw = logits.shape
    if not (canvas.dtype == torch.float32 and canvas.is_contiguous() and tuple(canvas.shape[:2]) == (b, k1)):
        raise ValueError("canvas must be a contiguous fp32 tensor [B,K,H,W] with the logits' B and K")
    for name, g, n in (("gy", gy, ph), ("gx", gx, pw)):
        if not (g.dtype == torch.float32 and g.is_contiguous() and tuple(g.shape) == (n,)):
            raise ValueError(f"{name} must be a contiguous fp32 tensor of {n} elements, got {g.dtype} {tuple(g.shape)}")
    call("mia_window_accum", _p(logits), _p(canvas), _p(gy), _p(gx), b, k1, ph, pw, int(canvas.shape[2]), int(canvas.shape[3]),
         int(y0), int(x0), _c_i64(st[0]), _c_i64(st[1]), _c_i64(st[2]), ctypes.c_float(float(weight)), int(bool(flip_h)),
         int(bool(flip_w)), _stream())


def window_finalize(canvas: torch.Tensor, pred: Optional[torch.Tensor] = None, ry: Optional[torch.Tensor] = None,
                    rx: Optional[torch.Tensor] = None, scale: float = 1.0, normalise: bool = False) -> None:
    """``pred = canvas.argmax(1)`` where ``pred`` is given (ties to the lowest class), taken from the raw canvas; then, with
    ``normalise``, ``canvas *= (scale * ry[:, None]) * rx[None, :]`` in place.  canvas contiguous [B,K,H,W] fp32, pred contiguous
    [B,H,W] int64, ry [H] and rx [W] fp32, all on the GPU."""
    from mia_hip import call
    from mia_hip.ops import _need_dev, _p, _stream
    _need_dev(canvas, pred, ry, rx)
    if not (canvas.dim() == 4 and canvas.dtype == torch.float32 and canvas.is_contiguous()):
        raise ValueError("canvas must be a contiguous fp32 tensor [B,K,H,W]")
    b, k1, h, w = canvas.shape
    if pred is not None and not (pred.dtype == torch.int64 and pred.is_contiguous() and tuple(pred.shape) == (b, h, w)):
        raise ValueError("pred must be a contiguous int64 tensor [B,H,W]")
    if normalise:
        for name, r, n in (("ry", ry, h), ("rx", rx, w)):
            if r is None or not (r.dtype == torch.float32 and r.is_contiguous() and tuple(r.shape) == (n,)):
                raise ValueError(f"{name} must be a contiguous fp32 tensor of {n} elements")
    call("mia_window_finalize", _p(canvas), _p(pred), _p(ry), _p(rx), b, k1, h, w, ctypes.c_float(float(scale)), int(bool(normalise)),
         _stream())


def _mirror_combos(mirror_axes) -> list:
    """``()``, then each axis alone in the order given, then both."""
    axes = [int(a) for a in mirror_axes]
    if len(set(axes)) != len(axes) or any(a not in (2, 3) for a in axes):
        raise ValueError(f"mirror_axes={tuple(mirror_axes)}: expected a subset of (2, 3)")
    return [()] + [(a,) for a in axes] + ([tuple(axes)] if len(axes) == 2 else [])


def sliding_window_predict(models: Sequence[torch.nn.Module], x: torch.Tensor, patch_size, overlap: float = 0.5,
                           mirror_axes: Sequence[int] = (), weights: Optional[Sequence[float]] = None, importance: str = "gaussian",
                           window_batch: int = 1, return_probs: bool = False):
    """Label map [B,H,W] (int64) of x [B,C,H,W] predicted at its own resolution: every model sees windows of ``patch_size`` that
    overlap by at least ``overlap``, each window also mirrored along the combinations of ``mirror_axes`` (a subset of (2, 3)), and
    ``weights[m] * softmax`` of every forward is blended into one canvas under the outer product of two ``window_weights``.

    Each pixel accumulates in a fixed order -- model in list order, then mirror combination (none, each axis in the order given,
    both), then window row-major -- so the result is bit-identical from run to run.  ``window_batch`` stacks that many windows of one
    mirror combination into one forward (``window_batch * B`` patches) and changes nothing else: accumulation stays one pass per
    window.  An axis shorter than the patch is zero-padded to it (evenly, the odd pixel at the end) and the result cropped back.
    Models run in eval mode under ``torch.no_grad()`` and get their mode back on every exit path.  On the GPU a window is one
    ``mia_window_accum`` pass; CPU tensors take the same definition in torch ops.  ``return_probs=True`` returns
    ``(labels, probabilities [B,K,H,W] fp32 that sum to 1 over K)``."""
    models = list(models)
    if not models:
        raise ValueError("sliding_window_predict needs at least one model")
    weights = [1.0] * len(models) if weights is None else [float(v) for v in weights]
    if len(weights) != len(models):
        raise ValueError(f"{len(weights)} weights for {len(models)} models")
    if x.dim() != 4:
        raise ValueError(f"sliding_window_predict expects [B,C,H,W], got shape {tuple(x.shape)}")
    patch = [int(patch_size)] * 2 if isinstance(patch_size, int) else [int(v) for v in patch_size]
    if len(patch) != 2 or min(patch) < 1:
        raise ValueError(f"patch_size={patch_size}: expected one or two positive sizes")
    ph, pw = patch
    combos = _mirror_combos(mirror_axes)
    window_batch = int(window_batch)
    if window_batch < 1:
        raise ValueError(f"window_batch={window_batch}")
    b, _, h0, w0 = x.shape
    top, left = max(ph - h0, 0) // 2, max(pw - w0, 0) // 2
    if h0 < ph or w0 < pw:
        x = torch.nn.functional.pad(x, (left, max(pw - w0, 0) - left, top, max(ph - h0, 0) - top))
    h, w = int(x.shape[2]), int(x.shape[3])
    ys, xs = window_starts(h, ph, overlap), window_starts(w, pw, overlap)
    windows = [(y0, x0) for y0 in ys for x0 in xs]
    gy_np, gx_np = window_weights(ph, importance), window_weights(pw, importance)
    ry_np = (1.0 / coverage_1d(gy_np, ys, h)).astype(np.float32)
    rx_np = (1.0 / coverage_1d(gx_np, xs, w)).astype(np.float32)
    scale = 1.0 / (len(combos) * sum(weights))
    on_gpu = x.is_cuda
    gy, gx, ry, rx = (torch.from_numpy(v).to(x.device) for v in (gy_np, gx_np, ry_np, rx_np))
    if on_gpu:
        from transforms.hip import functional_hip as FH
        x = x.contiguous()
    else:
        g2d = gy[:, None] * gx[None, :]
    modes = [m.training for m in models]
    canvas = None
    try:
        for m in models:
            m.eval()
        with torch.no_grad():
            for i, (m, wt) in enumerate(zip(models, weights)):
                for combo in combos:
                    fh, fw = 2 in combo, 3 in combo
                    # a window of the mirrored image at the mirrored offset is the mirrored window
                    if not combo:
                        xin = x
                    else:
                        xin = FH.rot90_flip(x, 0, fh, fw) if on_gpu else x.flip(combo)
                    for c0 in range(0, len(windows), window_batch):
                        chunk = windows[c0:c0 + window_batch]
                        srcs = [(h - y0 - ph if fh else y0, w - x0 - pw if fw else x0) for y0, x0 in chunk]
                        if on_gpu:
                            patches = [FH.crop(xin, [sy] * b, [sx] * b, ph, pw) for sy, sx in srcs]
                        else:
                            patches = [xin[:, :, sy:sy + ph, sx:sx + pw] for sy, sx in srcs]
                        logits = _logits_of(m, patches[0] if len(patches) == 1 else torch.cat(patches, 0))
                        del patches
                        if logits.dim() != 4 or tuple(logits.shape[0:1] + logits.shape[2:]) != (len(chunk) * b, ph, pw):
                            raise ValueError(f"model {i} returned shape {tuple(logits.shape)} for {len(chunk) * b} patches of {ph}x{pw}")
                        if canvas is None:
                            canvas = torch.zeros((b, logits.shape[1], h, w), device=logits.device, dtype=torch.float32)
                        elif logits.shape[1] != canvas.shape[1]:
                            raise ValueError(f"model {i} returned {logits.shape[1]} classes, the models before it {canvas.shape[1]}")
                        for j, (y0, x0) in enumerate(chunk):
                            part = logits[j * b:(j + 1) * b]
                            if part.is_cuda:
                                window_accum(part, canvas, gy, gx, y0, x0, wt, fh, fw)
                            else:  # the same definition in torch ops
                                p = wt * part.float().softmax(1)
                                canvas[:, :, y0:y0 + ph, x0:x0 + pw] += g2d * (p.flip(combo) if combo else p)
                        del logits
            if canvas.is_cuda:
                pred = torch.empty((b, h, w), device=canvas.device, dtype=torch.int64)
                window_finalize(canvas, pred, ry, rx, scale, normalise=return_probs)
            else:
                pred = canvas.argmax(1)
                if return_probs:
                    canvas = canvas * ((scale * ry)[:, None] * rx[None, :])
    finally:
        for m, was in zip(models, modes):
            m.train(was)
    if (h, w) != (h0, w0):
        pred = pred[:, top:top + h0, left:left + w0].contiguous()
        canvas = canvas[:, :, top:top + h0, left:left + w0].contiguous() if return_probs else None
    return (pred, canvas) if return_probs else pred


class EnsemblePredictor:
    """The reference's ``model`` class (predict.py:15-161) on the GPU.

    ``UNet(2, in_channels, output_classes, channels_list, **unet_kwargs)`` per fold (the reference's ``UNet(3, 3)`` predates that
    signature); ``output_classes`` counts the background, and the clean-up knows labels 0 / 1 / 2 like the reference's.
    ``weights`` (one per fold, default all 1) is one extension.  ``patch_size`` is the other: with it the ensemble runs as
    ``sliding_window_predict`` (windows of that size with ``overlap``, mirrored along ``mirror_axes``, ``window_batch`` windows per
    forward) on the preprocessed batch -- with ``image_size=None`` at the images' own resolution.  Without it nothing changes.
    ``keep_largest`` (None, "foreground", "per_class" or a tuple of classes) and ``min_component_size`` switch on the
    connected-component clean-up of `UnetProcessor.postprocess`, applied last at the images' own size; off by default."""

    def __init__(self, image_size, folds: Sequence[int] = (0, 1, 2, 3, 4), in_channels: int = 3, output_classes: int = 3, device=None,
                 channels_list: Sequence[int] = DEFAULT_CHANNELS, weights: Optional[Sequence[float]] = None, patch_size=None,
                 overlap: float = 0.5, mirror_axes: Sequence[int] = (), window_batch: int = 1, keep_largest=None,
                 min_component_size: int = 0, **unet_kwargs):
        self.folds = list(folds)
        if not self.folds:
            raise ValueError("EnsemblePredictor needs at least one fold")
        self.device = torch.device(device) if device is not None else torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
        self.weights = None if weights is None else [float(v) for v in weights]
        if self.weights is not None and len(self.weights) != len(self.folds):
            raise ValueError(f"{len(self.weights)} weights for {len(self.folds)} folds")
        self.patch_size = None if patch_size is None else ([int(patch_size)] * 2 if isinstance(patch_size, int) else [int(v) for v in patch_size])
        self.overlap, self.mirror_axes, self.window_batch = float(overlap), tuple(mirror_axes), int(window_batch)
        self.keep_largest, self.min_component_size, self.output_classes = keep_largest, int(min_component_size), int(output_classes)
        if self.patch_size is not None:
            window_starts(self.patch_size[0], self.patch_size[0], self.overlap)  # argument errors now, not at the first image
            _mirror_combos(self.mirror_axes)
        self.processor = UnetProcessor(image_size=image_size, dilate_size=5, erode_size=5, smooth_kernel=7)  # predict.py:21-23
        self.image_size = self.processor.image_size
        self.models = [UNet(2, in_channels, output_classes, list(channels_list), **unet_kwargs).to(self.device).eval() for _ in self.folds]

    def load(self, path="./"):
        """``{path}/fold_{k}/checkpoint_best.pth`` -> model k (its ``["model"]`` entry, predict.py:35-41)."""
        from training.checkpoint import load_model_checkpoint
        for m, fold in zip(self.models, self.folds):
            ckpt = os.path.join(os.fspath(path), f"fold_{fold}", "checkpoint_best.pth")
            if not os.path.isfile(ckpt):
                raise FileNotFoundError(f"no checkpoint for fold {fold}: {ckpt}")
            load_model_checkpoint(m, ckpt, map_location=self.device)
        return self

    def preprocess(self, X) -> torch.Tensor:
        """``X / 255`` as fp32 on the device, bilinear resize to ``image_size`` (predict.py:43-53); [C,H,W] or [B,C,H,W]."""
        image = torch.as_tensor(np.asarray(X) if not isinstance(X, torch.Tensor) else X).to(self.device, dtype=torch.float32) / 255.0
        return self.processor.preprocess(image)

    def predict_batch(self, X, do_denoise: bool = True) -> torch.Tensor:
        """[B,C,H,W] images with values 0..255 -> label maps [B,H,W] (int64, on the device) at the images' own size: ensemble
        arg-max at ``image_size`` (over sliding windows where ``patch_size`` is set), nearest resize back, then the mask clean-up
        (predict.py:55-90) unless ``do_denoise`` is off."""
        if X.ndim != 4:
            raise ValueError(f"predict_batch expects [B,C,H,W], got shape {tuple(X.shape)}")
        ori_shape = (int(X.shape[-2]), int(X.shape[-1]))
        if self.patch_size is None:
            pred = ensemble_predict(self.models, self.preprocess(X), self.weights)
        else:
            pred = sliding_window_predict(self.models, self.preprocess(X), self.patch_size, self.overlap, self.mirror_axes, self.weights,
                                          window_batch=self.window_batch)
        return self.processor.postprocess(pred, ori_shape, do_denoise=do_denoise, keep_largest=self.keep_largest,
                                          min_component_size=self.min_component_size, n_classes=self.output_classes)

    def predict(self, X, no_normalization: bool = True) -> np.ndarray:
        """One [C,H,W] image -> numpy label map [H,W] (predict.py:133-151; ``no_normalization`` is accepted and unused there too)."""
        if X.ndim != 3:
            raise ValueError(f"predict expects [C,H,W], got shape {tuple(X.shape)}")
        return self.predict_batch(X[None])[0].cpu().numpy()
