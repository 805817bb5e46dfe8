"""Fold-ensemble prediction (reference `src/entry/fugc2025/predict.py`, class ``model``): every fold model's ``softmax(1)`` summed,
``argmax``, nearest resize back to the original size, then the morphological mask clean-up.

On the GPU the reduction is one streaming pass per model (``mia_softmax_accum``, csrc/predict.hip) straight from the head's native
logits layout, with the arg-max written by the last pass, and the clean-up is one launch (``mia_mask_denoise``).  CPU tensors take
the same definition as torch ops; the networks themselves run on the GPU only."""
from __future__ import annotations

import ctypes
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


class EnsemblePredictor:
    """The reference's ``model`` class (predict.py:15-161) on the GPU.

    ``UNet(2, in_channels, output_classes, channels_list, **unet_kwargs)`` per fold (the reference's ``UNet(3, 3)`` predates that
    signature); ``output_classes`` counts the background, and the clean-up knows labels 0 / 1 / 2 like the reference's.
    ``weights`` (one per fold, default all 1) is the one extension."""

    def __init__(self, image_size, folds: Sequence[int] = (0, 1, 2, 3, 4), in_channels: int = 3, output_classes: int = 3, device=None,
                 channels_list: Sequence[int] = DEFAULT_CHANNELS, weights: Optional[Sequence[float]] = None, **unet_kwargs):
        self.folds = list(folds)
        if not self.folds:
            raise ValueError("EnsemblePredictor needs at least one fold")
        self.device = torch.device(device) if device is not None else torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
        self.weights = None if weights is None else [float(v) for v in weights]
        if self.weights is not None and len(self.weights) != len(self.folds):
            raise ValueError(f"{len(self.weights)} weights for {len(self.folds)} folds")
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
        arg-max at ``image_size``, nearest resize back, then the mask clean-up (predict.py:55-90) unless ``do_denoise`` is off."""
        if X.ndim != 4:
            raise ValueError(f"predict_batch expects [B,C,H,W], got shape {tuple(X.shape)}")
        ori_shape = (int(X.shape[-2]), int(X.shape[-1]))
        pred = ensemble_predict(self.models, self.preprocess(X), self.weights)
        return self.processor.postprocess(pred, ori_shape, do_denoise=do_denoise)

    def predict(self, X, no_normalization: bool = True) -> np.ndarray:
        """One [C,H,W] image -> numpy label map [H,W] (predict.py:133-151; ``no_normalization`` is accepted and unused there too)."""
        if X.ndim != 3:
            raise ValueError(f"predict expects [C,H,W], got shape {tuple(X.shape)}")
        return self.predict_batch(X[None])[0].cpu().numpy()
