"""Acquisition scores of the active-learning selectors as one fused HIP pass over the logits (softmax + per-image
reduction): entropy (reference `src/activelearning/entropy_selector.py:42-49`), least confidence
(`confidence_selector.py:42-47`), margin (`margin_selector.py:42-48`).  The selectors themselves (pool iteration,
sorting, budget) live in ``activelearning.selectors`` and call ``selector_scores(model(x))``."""
from __future__ import annotations

import ctypes

import torch

from mia_hip import MiaError, call, lib
from mia_hip.ops import _c_i64, _dt, _need_dev, _p, _pix_strides, _stream

ENTROPY, CONFIDENCE, MARGIN = 0, 1, 2
BADGE_MAX_CLASSES, BADGE_MAX_CHANNELS = 8, 128  # mia_badge_embed: 1 <= K1 <= 8, C0 a multiple of 4 up to 128


def badge_shape_supported(k1: int, c0: int) -> bool:
    return 1 <= k1 <= BADGE_MAX_CLASSES and 4 <= c0 <= BADGE_MAX_CHANNELS and c0 % 4 == 0


def badge_slabs(hw: int, k1: int, c0: int, dtype: torch.dtype) -> int:
    """Pixel slabs per image of the `badge_embeddings` kernels (the library's own rule; 0 = unsupported shape)."""
    slabs = ctypes.c_int(0)
    lib().mia_badge_embed_workspace(1, hw, k1, c0, _dt(dtype), ctypes.byref(slabs))
    return slabs.value


def badge_embeddings(logits: torch.Tensor, feat_nhwc: torch.Tensor, smooth: float = 1e-5, do_bg: bool = False,
                     squared: bool = False):
    """BADGE gradient embeddings of a batch in one fused pass (reference `badge_selector.py:19-35` and `:80-96`, one image
    and one autograd backward at a time there): logits [B,K1,H,W] fp32 and the head's input feat_nhwc [B,H,W,C0] (fp32 or
    bf16) -> (embed [B, K1*C0] fp32, loss [B] fp32), embed[b] = d(CE + DiceLoss(smooth, do_bg, squared))(logits[b],
    argmax logits[b]) / d decoder.seg_output.weight, flattened like that weight."""
    _need_dev(logits, feat_nhwc)
    if logits.ndim != 4 or feat_nhwc.ndim != 4 or feat_nhwc.shape[:3] != (logits.shape[0], logits.shape[2], logits.shape[3]):
        raise MiaError(f"badge_embeddings: logits {tuple(logits.shape)} [B,K1,H,W] and features {tuple(feat_nhwc.shape)} "
                       "[B,H,W,C0] do not describe the same pixels")
    if logits.dtype != torch.float32:
        logits = logits.float()
    st = _pix_strides(logits)
    if st is None:
        logits = logits.contiguous()
        st = _pix_strides(logits)
    feat_nhwc = feat_nhwc.contiguous()
    b, k1, h, w = logits.shape
    c0 = feat_nhwc.shape[3]
    dtype = _dt(feat_nhwc)
    words = lib().mia_badge_embed_workspace(b, h * w, k1, c0, dtype, None)
    ws = torch.empty(max(words, 1), device=logits.device, dtype=torch.float32)
    embed = torch.empty((b, k1 * c0), device=logits.device, dtype=torch.float32)
    loss = torch.empty(b, device=logits.device, dtype=torch.float32)
    call("mia_badge_embed", _p(logits), _p(feat_nhwc), dtype, b, _c_i64(h * w), k1, c0, _c_i64(st[0]), _c_i64(st[1]), _c_i64(st[2]),
         ctypes.c_float(smooth), int(bool(do_bg)), int(bool(squared)), _p(ws), _p(embed), _p(loss), _stream())
    return embed, loss


def selector_scores(logits: torch.Tensor, smooth: float = 1e-8) -> torch.Tensor:
    """logits [B,K1,H,W] -> scores [B,3] fp32: (entropy, -max prob, -(top1 - top2)), each averaged like the reference."""
    _need_dev(logits)
    if logits.dtype != torch.float32:
        logits = logits.float()
    st = _pix_strides(logits)
    if st is None:
        logits = logits.contiguous()
        st = _pix_strides(logits)
    b, k1, h, w = logits.shape
    hw = h * w
    slabs = max(1, min(128, hw // 2048))
    ws = torch.empty(lib().mia_selector_scores_workspace(b, slabs), device=logits.device, dtype=torch.float32)
    out = torch.empty((b, 3), device=logits.device, dtype=torch.float32)
    call("mia_selector_scores", _p(logits), b, _c_i64(hw), k1, _c_i64(st[0]), _c_i64(st[1]), _c_i64(st[2]), ctypes.c_float(smooth), slabs, _p(ws), _p(out),
         _stream())
    return out
