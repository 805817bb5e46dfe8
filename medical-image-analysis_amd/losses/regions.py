"""Region-based targets (nnU-Net's region mode): every output channel is a *region*, the set of labels it covers, and regions
may overlap -- e.g. the FUGC post-processing's "object = label > 0" and "anterior lip = label == 1" are `((1, 2), (1,))`."""
from __future__ import annotations

from typing import Optional, Sequence

import torch


def check_regions(regions) -> tuple:
    """`regions` as a tuple of tuples of non-negative ints (one tuple of labels per output channel)."""
    out = tuple(tuple(int(v) for v in ((r,) if isinstance(r, int) else r)) for r in regions)
    if not out:
        raise ValueError("regions: at least one region is needed")
    if any(v < 0 for r in out for v in r):
        raise ValueError("regions: labels must be >= 0")
    return out


def expand_regions(labels: torch.Tensor, regions: Sequence[Sequence[int]], ignore_label: Optional[int] = None) -> torch.Tensor:
    """Dense bool target of a label map: `labels` [B,1,H,W] or [B,H,W] (any integer dtype) -> [B,C,H,W] with channel c true where
    the label belongs to `regions[c]`; with `ignore_label` a last channel is appended that is true where the label equals it (the
    layout `DC_and_BCE_loss(use_ignore_label=True)` expects).  Plain tensor ops, for CPU and GPU tensors alike: this function is
    the definition of what the index form of the loss (`DC_and_BCE_loss(..., regions=...)`) computes."""
    regions = check_regions(regions)
    if labels.ndim == 4:
        if labels.shape[1] != 1:
            raise ValueError(f"expand_regions: label map [B,1,H,W] or [B,H,W] expected, got {tuple(labels.shape)}")
        labels = labels[:, 0]
    chans = []
    for r in regions:
        m = torch.zeros(labels.shape, dtype=torch.bool, device=labels.device)
        for v in r:
            m |= labels == v
        chans.append(m)
    if ignore_label is not None:
        chans.append(labels == ignore_label)
    return torch.stack(chans, 1)
