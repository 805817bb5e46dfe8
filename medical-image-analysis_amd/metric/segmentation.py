"""Validation metrics on the GPU: label maps, per-class hard Dice, Jaccard, Hausdorff and average surface distance.

Replaces the CPU work of ``ALTrainer.valid_slices`` / ``valid_volumns`` / ``calculate_metric_percase`` (reference
`src/training/al_trainer.py:1415-1556`: ``softmax -> argmax -> .cpu().numpy()`` then ``medpy.metric.dc``, ``metric.cal_hd``
(SimpleITK), ``medpy.metric.asd`` and ``medpy.metric.jc`` per image and class).  ``percase_metrics`` returns the reference's full
(DSC, HD, ASD, JC) table as device tensors: DSC / JC from the Dice counts (csrc/metrics.hip), HD / ASD from exact Euclidean distance
transforms (csrc/surface.hip), in 2-D for [N,H,W] images and in 3-D for [N,D,H,W] volumes; ``surface_metrics`` and
``percase_metrics(extended=True)`` add HD95, the symmetric surface distance and the surface Dice.  Divergences from the reference
(INTEGRATION.md section D): a spacing applies to HD too (``cal_hd`` returns inf whenever one is passed), the spacing is read in array
axis order for HD and ASD alike, and ASD is +inf for an empty label mask (medpy raises)."""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple, Optional, Sequence, Tuple, Union

import torch

from mia_hip import call, lib
from mia_hip.ops import _c_i64, _need_dev, _p, _pix_strides, _stream


def predict_and_dice(logits: torch.Tensor, labels: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """logits [B,K1,H,W] fp32 (any pixel-collapsible strides) -> (pred [B,H,W] int64, dice [B,K1], counts [B,K1,3]).

    ``dice[b, k]`` = 2|P&G| / (|P|+|G|) for class k (``pred == k`` vs ``label == k``), 0 where the prediction is empty
    -- `calculate_metric_percase` semantics; the trainer's "all foreground" metric is
    ``2*sum_k>0 I / (sum_k>0 P + sum_k>0 G)`` from ``counts``."""
    _need_dev(logits, labels)
    if logits.dtype != torch.float32:
        logits = logits.float()
    st = _pix_strides(logits)
    if st is None:
        logits = logits.contiguous()
        st = _pix_strides(logits)
    b, k1, h, w = logits.shape
    hw = h * w
    slabs = max(1, min(128, hw // 2048))
    dev = logits.device
    pred = torch.empty((b, h, w), device=dev, dtype=torch.long)
    ws = counts = dice = None
    lab = None
    if labels is not None:
        lab = labels.reshape(b, h, w).long().contiguous()
        ws = torch.empty(lib().mia_argmax_dice_workspace(b, k1, slabs), device=dev, dtype=torch.float32)
        counts = torch.empty((b, k1, 3), device=dev, dtype=torch.float32)
        dice = torch.empty((b, k1), device=dev, dtype=torch.float32)
    call("mia_argmax_dice", _p(logits), _p(lab), _p(pred), b, _c_i64(hw), k1, _c_i64(st[0]), _c_i64(st[1]), _c_i64(st[2]), slabs,
         _p(ws), _p(counts), _p(dice), _stream())
    return pred, dice, counts


def label_dice(pred: torch.Tensor, labels: torch.Tensor, k1: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-(image, class) hard Dice of two LABEL MAPS [B,H,W] (int64) -> (dice [B,K1], counts [B,K1,3] = |P&G|, |P|, |G|):
    `calculate_metric_percase` (al_trainer.py:1539-1556) on `pred == k` vs `label == k`, all classes in one pass."""
    _need_dev(pred, labels)
    b, h, w = pred.shape
    hw = h * w
    slabs = max(1, min(128, hw // 2048))
    dev = pred.device
    p = pred.long().contiguous()
    lab = labels.reshape(b, h, w).long().contiguous()
    ws = torch.empty(lib().mia_argmax_dice_workspace(b, k1, slabs), device=dev, dtype=torch.float32)
    counts = torch.empty((b, k1, 3), device=dev, dtype=torch.float32)
    dice = torch.empty((b, k1), device=dev, dtype=torch.float32)
    call("mia_argmax_dice", None, _p(lab), _p(p), b, _c_i64(hw), k1, _c_i64(0), _c_i64(0), _c_i64(0), slabs, _p(ws), _p(counts),
         _p(dice), _stream())
    return dice, counts


def _dice_columns(dice: torch.Tensor, counts: torch.Tensor, n: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(DSC of `pred > 0` vs `label > 0` [B], DSC per class 1..K [B,K]) from `label_dice`'s outputs over n pixels per image."""
    i0, p0, g0 = counts[:, 0, 0], counts[:, 0, 1], counts[:, 0, 2]
    pf, gf = n - p0, n - g0                       # |pred > 0|, |label > 0|
    inter = n - p0 - g0 + i0                      # |pred > 0 & label > 0| = N - |pred == 0 or label == 0|
    metric_all = torch.where(pf > 0, 2.0 * inter / (pf + gf).clamp_min(1.0), torch.zeros_like(pf))
    return metric_all, dice[:, 1:]


def _mask_ndim(pred: torch.Tensor, labels: torch.Tensor) -> int:
    """2 for [N,H,W] images, 3 for [N,D,H,W] volumes; raises on other ranks and on a shape mismatch."""
    if pred.shape != labels.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and labels {tuple(labels.shape)} differ in shape")
    if pred.dim() not in (3, 4):
        raise ValueError(f"expected [N,H,W] images or [N,D,H,W] volumes, got shape {tuple(pred.shape)}")
    return pred.dim() - 1


def _spacing(spacing, ndim: int) -> Tuple[float, float, float]:
    """(sd, sh, sw) for the C ABI from None or `ndim` positive finite host numbers in array axis order (sd = 1 for images)."""
    if spacing is None:
        return 1.0, 1.0, 1.0
    if isinstance(spacing, torch.Tensor):
        if spacing.is_cuda:
            raise ValueError("spacing must be host numbers (a CPU tensor, list or tuple), not a device tensor")
        spacing = spacing.detach().double().numpy()
    s = [float(v) for v in spacing]
    if len(s) != ndim:
        raise ValueError(f"spacing has {len(s)} entries; a {ndim}-D mask needs {ndim} (array axis order)")
    if not all(math.isfinite(v) and v > 0 for v in s):
        raise ValueError(f"spacing {s} must be finite and > 0")
    return (1.0, s[0], s[1]) if ndim == 2 else (s[0], s[1], s[2])


def surface_distances(pred: torch.Tensor, labels: torch.Tensor, k1: int, spacing: Optional[Sequence[float]] = None
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Hausdorff distance and average surface distance of `calculate_metric_percase` (al_trainer.py:1539-1556) for k1 mask pairs:
    mask 0 = (pred > 0, labels > 0), mask c = (pred == c, labels == c).  pred / labels int64 device tensors, [N,H,W] (N images,
    4-neighbour borders) or [N,D,H,W] (N volumes, 6-neighbour borders); spacing None or one positive number per axis in array
    order.  Returns (hd [N,k1], asd [N,k1]) fp32: HD over all pixels of both masks (ITK HausdorffDistanceImageFilter), ASD =
    medpy asd (connectivity 1); NaN where the prediction mask is empty, +inf where only the label mask is."""
    ndim = _mask_ndim(pred, labels)
    sd, sh, sw = _spacing(spacing, ndim)
    _need_dev(pred, labels)
    n, d, h, w = (pred.shape[0], 1) + tuple(pred.shape[1:]) if ndim == 2 else tuple(pred.shape)
    p = pred.long().contiguous()
    lab = labels.long().contiguous()
    nws = lib().mia_surface_distance_workspace(n, d, h, w, k1)
    if nws < 0:
        raise ValueError(f"surface_distances: shape {tuple(pred.shape)} with k1={k1} is outside the kernel's limits "
                         f"(include/mia_hip.h)")
    dev = p.device
    ws = torch.empty(nws, device=dev, dtype=torch.float32)
    hd = torch.empty((n, k1), device=dev, dtype=torch.float32)
    asd = torch.empty((n, k1), device=dev, dtype=torch.float32)
    call("mia_surface_distance", _p(p), _p(lab), n, ndim, d, h, w, k1, ctypes.c_float(sd), ctypes.c_float(sh), ctypes.c_float(sw),
         _p(ws), _p(hd), _p(asd), _stream())
    return hd, asd


class SurfaceMetrics(NamedTuple):
    hd: torch.Tensor
    asd: torch.Tensor
    hd_pct: torch.Tensor
    assd: torch.Tensor
    nsd: torch.Tensor


def _percentile(percentile) -> float:
    q = float(percentile)
    if not 0.0 < q <= 100.0:  # NaN fails too
        raise ValueError(f"percentile {percentile} must be in (0, 100]")
    return q


def _tolerance(tolerance, k1: int):
    """k1 finite host floats >= 0 (a number applies to every mask) as a C array."""
    if isinstance(tolerance, torch.Tensor):
        if tolerance.is_cuda:
            raise ValueError("tolerance must be host numbers (a number, CPU tensor, list or tuple), not a device tensor")
        tolerance = tolerance.detach().double().reshape(-1).tolist()
    t = [float(v) for v in tolerance] if hasattr(tolerance, "__iter__") else [float(tolerance)] * k1
    if len(t) != k1:
        raise ValueError(f"tolerance has {len(t)} entries; one number or {k1} (one per mask, entry 0 = the whole foreground) are needed")
    if not all(math.isfinite(v) and v >= 0 for v in t):
        raise ValueError(f"tolerance {t} must be finite and >= 0")
    return (ctypes.c_float * k1)(*t)


def surface_metrics(pred: torch.Tensor, labels: torch.Tensor, k1: int, spacing: Optional[Sequence[float]] = None,
                    percentile: float = 95.0, tolerance: Union[float, Sequence[float]] = 1.0) -> SurfaceMetrics:
    """`surface_distances` plus the symmetric surface metrics of the same k1 mask pairs, over the border-to-border distances
    S1 = {d(a, dB) : a in dA} and S2 = {d(b, dA) : b in dB}: `hd_pct` = numpy's linear `percentile` of S1 u S2 (medpy hd95 at 95),
    `assd` = (mean S1 + mean S2) / 2 (medpy assd), `nsd` = the share of S1 u S2 that is <= `tolerance` (voxel-count surface Dice;
    one number, or k1 numbers in the units of `spacing`).  Returns (hd, asd, hd_pct, assd, nsd), each [N,k1] fp32 on the device;
    hd / asd are `surface_distances`' bits.  hd_pct = assd = NaN where the prediction mask is empty, +inf where only the label mask
    is; nsd = 0 in both cases.  The percentile is an exact order statistic (integer radix select): bit-identical from run to run.
    No host sync."""
    ndim = _mask_ndim(pred, labels)
    sd, sh, sw = _spacing(spacing, ndim)
    q = _percentile(percentile)
    if not 1 <= k1 <= 8:
        raise ValueError(f"surface_metrics: k1={k1} not in [1, 8]")
    tol = _tolerance(tolerance, k1)
    _need_dev(pred, labels)
    n, d, h, w = (pred.shape[0], 1) + tuple(pred.shape[1:]) if ndim == 2 else tuple(pred.shape)
    p = pred.long().contiguous()
    lab = labels.long().contiguous()
    nws = lib().mia_surface_metrics_workspace(n, d, h, w, k1)
    if nws < 0:
        raise ValueError(f"surface_metrics: shape {tuple(pred.shape)} with k1={k1} is outside the kernel's limits "
                         f"(include/mia_hip.h)")
    dev = p.device
    ws = torch.empty(nws, device=dev, dtype=torch.float32)
    out = [torch.empty((n, k1), device=dev, dtype=torch.float32) for _ in range(5)]
    call("mia_surface_metrics", _p(p), _p(lab), n, ndim, d, h, w, k1, ctypes.c_float(sd), ctypes.c_float(sh), ctypes.c_float(sw),
         ctypes.c_double(q), tol, _p(ws), *[_p(o) for o in out], _stream())
    return SurfaceMetrics(*out)


def percase_metrics(pred: torch.Tensor, labels: torch.Tensor, num_classes: int, spacing: Optional[Sequence[float]] = None,
                    extended: bool = False, percentile: float = 95.0, tolerance: Union[float, Sequence[float]] = 1.0
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The reference's metric arrays of `valid_slices` / `valid_volumns` (al_trainer.py:1463-1472, :1523-1535) as device tensors:
    (metric_all [N,4], metric_per_cls [N,num_classes,4]), columns (DSC, HD, ASD, JC) of `calculate_metric_percase` on
    (pred > 0, label > 0) and (pred == c, label == c).  [N,H,W] = N images (2-D metrics), [N,D,H,W] = N volumes (3-D metrics).
    A row is (0, NaN, NaN, 0) for an empty prediction mask and (0, inf, inf, 0) when only the label mask is empty.
    `extended=True` appends the columns (HD95, ASSD, NSD) of `surface_metrics` -- 7 in all, the first four with the same bits --
    at `percentile` and `tolerance` (one number, or num_classes + 1 with entry 0 for the whole foreground); an empty prediction
    gives (NaN, NaN, 0) there and an empty label alone (inf, inf, 0)."""
    _spacing(spacing, _mask_ndim(pred, labels))
    k1 = num_classes + 1
    if extended:
        _percentile(percentile)
        _tolerance(tolerance, k1)
    _need_dev(pred, labels)
    if extended:
        hd, asd, hd_pct, assd, nsd = surface_metrics(pred, labels, k1, spacing, percentile, tolerance)
    else:
        hd, asd = surface_distances(pred, labels, k1, spacing)
    b, w = pred.shape[0], pred.shape[-1]
    rows = pred.numel() // (b * w)                # a volume's Dice counts are those of one D*H x W image
    dice, counts = label_dice(pred.reshape(b, rows, w), labels.reshape(b, rows, w), k1)
    n = float(rows * w)
    dsc_all, dsc_cls = _dice_columns(dice, counts, n)
    i0, p0, g0 = counts[:, 0, 0], counts[:, 0, 1], counts[:, 0, 2]
    inter_all, union_all = n - p0 - g0 + i0, n - i0   # |pred == 0 & label == 0| = i0, so |pred > 0 or label > 0| = N - i0
    jc_all = torch.where(n - p0 > 0, inter_all / union_all.clamp_min(1.0), torch.zeros_like(p0))
    ic, pc, gc = counts[:, 1:, 0], counts[:, 1:, 1], counts[:, 1:, 2]
    jc_cls = torch.where(pc > 0, ic / (pc + gc - ic).clamp_min(1.0), torch.zeros_like(pc))
    ext_all, ext_cls = ((hd_pct[:, 0], assd[:, 0], nsd[:, 0]), (hd_pct[:, 1:], assd[:, 1:], nsd[:, 1:])) if extended else ((), ())
    metric_all = torch.stack((dsc_all, hd[:, 0], asd[:, 0], jc_all) + ext_all, dim=-1)
    metric_per_cls = torch.stack((dsc_cls, hd[:, 1:], asd[:, 1:], jc_cls) + ext_cls, dim=-1)
    return metric_all, metric_per_cls


def _predict(model, processor, image: torch.Tensor, label: torch.Tensor, loss_fn, do_denoise: bool):
    """preprocess -> eval forward -> argmax -> (loss on labels nearest-resized to the output size) -> postprocess; the model's
    train / eval mode is restored on every exit path.  Returns (loss, pred [B,H,W] at the label size)."""
    from transforms.hip import functional_hip as FH
    was_training = model.training
    model.eval()
    try:
        x = processor.preprocess(image)
        output = model(x)
        pred, _, _ = predict_and_dice(output)
        loss = None
        if loss_fn is not None:
            ll = label
            if pred.shape[-2:] != label.shape[-2:]:
                ll = FH.resize_nearest(label.unsqueeze(1), int(output.shape[-2]), int(output.shape[-1])).squeeze(1)
            loss = loss_fn(output, ll)
        pred = processor.postprocess(pred, label.shape[-2:], do_denoise=do_denoise)
    finally:
        model.train(was_training)
    return loss, pred


@torch.no_grad()
def valid_slices(model, processor, image_batch: torch.Tensor, label_batch: torch.Tensor, num_classes: int, loss_fn=None,
                 do_denoise: bool = False, spacing: Optional[Sequence[float]] = None, full_metrics: bool = False,
                 extended: bool = False, percentile: float = 95.0, tolerance: Union[float, Sequence[float]] = 1.0):
    """One validation step of `ALTrainer.valid_slices` (al_trainer.py:1415-1474) chained on the GPU:
    `processor.preprocess` (bilinear resize to the model size, unet_processor.py:35-47) -> eval forward ->
    `softmax(1).argmax(1)` -> (loss on labels nearest-resized to the output size, :1433-1449) -> `processor.postprocess`
    (nearest resize back to the label size, unet_processor.py:49-70) -> metrics at the ORIGINAL resolution.
    Default: hard Dice only, `metric_all[b]` = Dice(pred > 0, label > 0), `metric_per_cls[b, c-1]` = Dice(pred == c, label == c),
    c = 1..num_classes, 0 for an empty prediction (:1463-1472, :1539-1556): returns (metric_all [B], metric_per_cls
    [B, num_classes], loss, pred).  `full_metrics=True`: the reference's whole (DSC, HD, ASD, JC) table of `percase_metrics`
    in 2-D, metric_all [B,4] and metric_per_cls [B,num_classes,4], with `spacing` = (sh, sw) for HD / ASD (the same DSC bits);
    with `extended=True` also its (HD95, ASSD, NSD) columns at `percentile` / `tolerance`, 7 columns in all.
    Device tensors, no host sync.  `do_denoise` is the reference's `config.postprocess_mask` (al_trainer.py:1445): the
    morphology of unet_processor.py:72-160 as batched tensor ops on the device (`UnetProcessor.denoise_masks`; parity with cv2 itself is
    unpinned -- cv2 is not importable here).  The model's train / eval mode is restored on every exit path."""
    if spacing is not None and not full_metrics:
        raise ValueError("valid_slices: spacing applies to the HD / ASD columns of full_metrics=True")
    if extended and not full_metrics:
        raise ValueError("valid_slices: extended adds columns to the table of full_metrics=True")
    dev = next(model.parameters()).device
    image = image_batch.to(dev, dtype=torch.float32)
    label = label_batch.to(dev).long()
    loss, pred = _predict(model, processor, image, label, loss_fn, do_denoise)
    if full_metrics:
        metric_all, metric_per_cls = percase_metrics(pred, label, num_classes, spacing, extended, percentile, tolerance)
        return metric_all, metric_per_cls, loss, pred
    dice, counts = label_dice(pred, label, num_classes + 1)
    metric_all, metric_per_cls = _dice_columns(dice, counts, float(label.shape[-2] * label.shape[-1]))
    return metric_all, metric_per_cls, loss, pred


@torch.no_grad()
def valid_volumns(model, processor, image: torch.Tensor, label: torch.Tensor, num_classes: int, loss_fn=None, do_denoise: bool = False,
                  spacing: Optional[Sequence[float]] = None, extended: bool = False, percentile: float = 95.0,
                  tolerance: Union[float, Sequence[float]] = 1.0):
    """One validation step of `ALTrainer.valid_volumns` (al_trainer.py:1476-1537, the default `valid_mode`): image [1,C,D,H,W] and
    label [1,D,H,W] (batch 1, asserted as the reference does); the D slices go through the chain of `valid_slices` as one batch and
    the metrics are computed in 3-D on the [D,H,W] prediction, `spacing` = (sd, sh, sw) in array axis order (the trainer's
    `torch.roll(sampled_batch["spacing"][0], 1)`).  Returns (metric_all [1,4], metric_per_cls [1,num_classes,4], loss,
    pred [D,H,W]) -- device tensors, no host sync; `extended=True` appends `percase_metrics`' (HD95, ASSD, NSD) columns
    ([1,7] / [1,num_classes,7]).  The model's train / eval mode is restored on every exit path."""
    assert image.shape[0] == 1 and label.shape[0] == 1, "valid_volumns takes one volume (batch 1)"
    dev = next(model.parameters()).device
    x = image.to(dev, dtype=torch.float32).squeeze(0).permute(1, 0, 2, 3).contiguous()  # [D,C,H,W]
    lab = label.to(dev).long().squeeze(0)                                            # [D,H,W]
    loss, pred = _predict(model, processor, x, lab, loss_fn, do_denoise)
    metric_all, metric_per_cls = percase_metrics(pred.unsqueeze(0), lab.unsqueeze(0), num_classes, spacing, extended, percentile,
                                                 tolerance)
    return metric_all, metric_per_cls, loss, pred
