"""Connected-component clean-up of label maps: nnU-Net's "remove all but the largest component" (per class or for the whole
foreground) and a minimum component size, in 2-D and 3-D.  The reference has only an approximation of it -- ``remove_cc``
(reference `src/models/unet/unet_processor.py:121-125`) is a morphological opening, which cannot remove a false-positive blob
larger than its structuring element.

Two voxels are joined when they are neighbours (``connectivity=1``: face neighbours; ``connectivity=ndim``: all 8 / 26) and hold
the same label in ``[1, n_classes)`` -- with ``foreground``, when both hold any label in that range.  A component's *root* is the
smallest linear index, within its image, of its voxels; the root map holds ``root + 1`` on component voxels and 0 elsewhere, so it
is a function of the input alone.

int64 label maps on the GPU go through the union-find kernels of csrc/components.hip (``mia_cc_label`` / ``mia_cc_filter``).  The
tensor backend is the same definition in tensor ops -- a neighbourhood minimum of linear indices, masked by label equality, iterated
to its fixed point with a hooking step and pointer jumping in between; it serves CPU tensors and everything the kernels do not
cover.  Both give the same bits."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

MAX_CLASSES = 256  # CC_MAX_CLASSES of csrc/components.hip
_BACKENDS = ("auto", "tensor", "kernel")
_JUMPS = 3  # pointer-jumping steps between two neighbourhood passes


def _canon(labels: torch.Tensor, ndim: int) -> torch.Tensor:
    """[nimg, D, H, W] view of the label maps (D = 1 for ndim 2)."""
    if ndim not in (2, 3):
        raise ValueError(f"ndim={ndim}: expected 2 or 3")
    if ndim == 2:
        if labels.ndim not in (2, 3):
            raise ValueError(f"ndim=2 expects [H,W] or [B,H,W], got shape {tuple(labels.shape)}")
        return labels.reshape(-1, 1, labels.shape[-2], labels.shape[-1])
    if labels.ndim not in (3, 4):
        raise ValueError(f"ndim=3 expects [D,H,W] or [B,D,H,W], got shape {tuple(labels.shape)}")
    return labels.reshape((-1,) + tuple(labels.shape[-3:]))


def _check_args(labels, ndim, connectivity, n_classes, backend):
    if backend not in _BACKENDS:
        raise ValueError(f"backend={backend!r}: expected 'auto', 'tensor' or 'kernel'")
    if labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool:
        raise ValueError(f"label maps must hold integers, got {labels.dtype}")
    if connectivity not in (1, ndim):
        raise ValueError(f"connectivity={connectivity}: expected 1 (faces) or {ndim} (full) for ndim={ndim}")
    if n_classes is None:
        n_classes = max(int(labels.max()) + 1, 2) if labels.numel() else 2
    n_classes = int(n_classes)
    if not 1 <= n_classes <= MAX_CLASSES:
        raise ValueError(f"n_classes={n_classes}: expected 1..{MAX_CLASSES}")
    return n_classes


def _use_kernel(lab4: torch.Tensor, ndim: int, n_classes: int, backend: str) -> bool:
    if backend == "tensor":
        return False
    covered = lab4.is_cuda and lab4.dtype == torch.int64 and lab4.numel() > 0
    if covered:
        from mia_hip import lib
        n, d, h, w = lab4.shape
        covered = lib().mia_cc_workspace(n, ndim, d, h, w, n_classes) >= 0
    if backend == "kernel" and not covered:
        raise ValueError(f"the component kernels do not cover {lab4.dtype} label maps of shape {tuple(lab4.shape)} on {lab4.device}")
    return covered


def _raise_on_status(status: torch.Tensor, what: str) -> None:
    s = int(status.item())
    if s:
        from mia_hip import MiaError
        raise MiaError(f"{what}: a union-find walk {'hit its iteration cap' if s & 1 else 'met a parent above its child'} "
                       f"(status {s}); the result is not valid")


# ------------------------------------------------------------------ tensor backend
def _offsets(ndim: int, connectivity: int):
    r = (-1, 0, 1)
    out = []
    for dz in (r if ndim == 3 else (0,)):
        for dy in r:
            for dx in r:
                n = abs(dz) + abs(dy) + abs(dx)
                if n and (connectivity > 1 or n == 1):
                    out.append((dz, dy, dx))
    return out


def _pair(n: int, o: int):
    """Slices (p, p + o) over the positions p of an axis of length n whose neighbour p + o exists."""
    return slice(max(0, -o), n - max(0, o)), slice(max(0, o), n - max(0, -o))


def _tensor_roots(lab4: torch.Tensor, ndim: int, connectivity: int, n_classes: int, foreground: bool):
    """(flat [nimg, vox] int64: the voxel's root, or `vox` where there is no component; fg mask of the same shape)."""
    n, d, h, w = lab4.shape
    vox = d * h * w
    lab = lab4.long()
    valid = (lab >= 1) & (lab < n_classes)
    key = torch.where(valid, torch.ones_like(lab) if foreground else lab, torch.zeros_like(lab))
    idx = torch.arange(vox, device=lab.device, dtype=torch.int64).reshape(1, d, h, w).expand(n, d, h, w)
    L = torch.where(valid, idx, torch.full_like(idx, vox)).contiguous()
    fg = valid.reshape(n, vox)
    if vox == 0 or n == 0:
        return L.reshape(n, vox), fg
    pairs = []
    for dz, dy, dx in _offsets(ndim, connectivity):
        (zd, zs), (yd, ys), (xd, xs) = _pair(d, dz), _pair(h, dy), _pair(w, dx)
        dst, src = (slice(None), zd, yd, xd), (slice(None), zs, ys, xs)
        pairs.append((dst, src, (key[dst] == key[src]) & valid[dst]))
    flat = L.reshape(n, vox)
    zero = torch.zeros_like(flat)
    while True:  # invariant: L[x] <= x names a voxel of x's own component
        before = L.clone()
        for dst, src, same in pairs:
            cur, nb = L[dst], L[src]
            L[dst] = torch.where(same & (nb < cur), nb, cur)
        # hook: what x pointed at learns x's new minimum too -- a minimum that arrives from higher indices (a line that runs
        # backwards in raster order) would otherwise crawl one voxel per round, because pointers only lead to lower indices
        flat.scatter_reduce_(1, torch.where(fg, before.reshape(n, vox), zero), torch.where(fg, flat, torch.full_like(flat, vox)),
                             "amin", include_self=True)
        for _ in range(_JUMPS):  # L[x] <- L[L[x]]
            flat.copy_(torch.where(fg, torch.gather(flat, 1, torch.where(fg, flat, zero)), flat))
        if torch.equal(L, before):
            return flat, fg


# ------------------------------------------------------------------ public interface
def connected_components(labels: torch.Tensor, ndim: int = 2, connectivity: int = 1, n_classes: Optional[int] = None,
                         foreground: bool = False, backend: str = "auto", check: bool = False) -> torch.Tensor:
    """int32 root map of the labels' shape: ``1 + root`` on component voxels, 0 elsewhere.

    labels: integer label maps [H,W] or [B,H,W] (``ndim=2``, every image on its own), [D,H,W] or [B,D,H,W] (``ndim=3``).
    ``n_classes=None`` takes ``labels.max() + 1`` (one synchronisation); labels outside ``[0, n_classes)`` belong to no component.
    backend: "auto" = the kernels for int64 maps on the GPU, else the tensor ops; "tensor"; "kernel" = the kernels or a ValueError.
    ``check=True`` reads the kernels' status word (one synchronisation) and raises if a union-find walk was cut short."""
    n_classes = _check_args(labels, ndim, connectivity, n_classes, backend)
    lab4 = _canon(labels, ndim)
    if _use_kernel(lab4, ndim, n_classes, backend):
        from mia_hip import call
        from mia_hip.ops import _p, _stream
        lab4 = lab4.contiguous()
        n, d, h, w = lab4.shape
        roots = torch.empty(lab4.shape, device=lab4.device, dtype=torch.int32)
        status = torch.empty(1, device=lab4.device, dtype=torch.int32)
        call("mia_cc_label", _p(lab4), _p(roots), n, ndim, d, h, w, int(connectivity), n_classes, int(bool(foreground)), _p(status),
             _stream())
        if check:
            _raise_on_status(status, "mia_cc_label")
        return roots.reshape(labels.shape)
    flat, fg = _tensor_roots(lab4, ndim, connectivity, n_classes, bool(foreground))
    return torch.where(fg, flat + 1, torch.zeros_like(flat)).to(torch.int32).reshape(labels.shape)


def compact_ids(roots: torch.Tensor, ndim: int = 2) -> torch.Tensor:
    """Root map -> components numbered 1..n per image in root order (int32), which is `scipy.ndimage.label`'s numbering for
    one mask: its raster scan meets every component first at its smallest index.  Plain tensor plumbing."""
    r4 = _canon(roots, ndim)
    n = r4.shape[0]
    flat = r4.reshape(n, -1).long()
    vox = flat.shape[1]
    if n == 0 or vox == 0:
        return torch.zeros_like(roots, dtype=torch.int32)
    is_root = flat == torch.arange(1, vox + 1, device=flat.device, dtype=torch.int64)
    rank = torch.cumsum(is_root.to(torch.int64), 1)
    ids = torch.gather(rank, 1, (flat - 1).clamp_(min=0))
    return torch.where(flat > 0, ids, torch.zeros_like(ids)).to(torch.int32).reshape(roots.shape)


def filter_components(labels: torch.Tensor, keep_largest: bool = True, min_size: int = 0, classes: Optional[Sequence[int]] = None,
                      foreground: bool = False, fill: int = 0, ndim: int = 2, connectivity: int = 1,
                      n_classes: Optional[int] = None, backend: str = "auto", check: bool = False) -> torch.Tensor:
    """Label maps with the stray components set to ``fill``: those of fewer than ``min_size`` voxels and, with ``keep_largest``,
    all but the largest of each (image, class) -- of each image with ``foreground``, where a component is a connected piece of the
    object mask and its kept voxels keep their classes.  Ties go to the component met first in raster order.  ``classes`` names the
    classes to filter (default: all of ``1 .. n_classes-1``); it cannot be combined with ``foreground``.  Everything else, labels
    outside ``[0, n_classes)`` included, is copied through; the result has the input's shape and dtype.  Shapes, ``n_classes``,
    ``backend`` and ``check`` as in `connected_components`."""
    n_classes = _check_args(labels, ndim, connectivity, n_classes, backend)
    min_size, fill, foreground, keep_largest = int(min_size), int(fill), bool(foreground), bool(keep_largest)
    if min_size < 0:
        raise ValueError(f"min_size={min_size} is negative")
    if classes is not None:
        if foreground:
            raise ValueError("classes cannot be combined with foreground=True: the foreground is filtered as one mask")
        classes = sorted({int(c) for c in classes})
        if any(not 1 <= c < n_classes for c in classes):
            raise ValueError(f"classes={classes}: expected labels in 1..{n_classes - 1}")
    lab4 = _canon(labels, ndim)
    if _use_kernel(lab4, ndim, n_classes, backend):
        import ctypes
        from mia_hip import call, lib
        from mia_hip.ops import _c_i64, _p, _stream
        lab4 = lab4.contiguous()
        n, d, h, w = lab4.shape
        out = torch.empty_like(lab4)
        ws = torch.empty(lib().mia_cc_workspace(n, ndim, d, h, w, n_classes), device=lab4.device, dtype=torch.float32)
        status = torch.empty(1, device=lab4.device, dtype=torch.int32)
        mask = None
        if classes is not None:
            mask = (ctypes.c_ubyte * n_classes)(*[1 if c in classes else 0 for c in range(n_classes)])
        call("mia_cc_filter", _p(lab4), _p(out), n, ndim, d, h, w, int(connectivity), n_classes, int(foreground), int(keep_largest),
             min_size, mask, _c_i64(fill), _p(ws), _p(status), _stream())
        if check:
            _raise_on_status(status, "mia_cc_filter")
        return out.reshape(labels.shape)
    flat, fg = _tensor_roots(lab4, ndim, connectivity, n_classes, foreground)
    n, vox = flat.shape
    lab = lab4.reshape(n, vox)
    if n == 0 or vox == 0:
        return labels.clone()
    r0 = torch.where(fg, flat, torch.zeros_like(flat))
    sizes = torch.zeros((n, vox), device=flat.device, dtype=torch.int64).scatter_add_(1, r0, fg.to(torch.int64))
    remove = fg & (torch.gather(sizes, 1, r0) < min_size)
    if keep_largest:
        ar = torch.arange(vox, device=flat.device, dtype=torch.int64)
        # (size << 32) | ~root: the largest size wins, ties go to the lowest root
        score = torch.where(fg & (flat == ar), (sizes << 32) | (0xFFFFFFFF - ar), torch.zeros_like(sizes))
        for m in ([fg] if foreground else [fg & (lab == c) for c in (range(1, n_classes) if classes is None else classes)]):
            win = torch.where(m, score, torch.zeros_like(score)).amax(1, keepdim=True)
            remove |= m & (flat != 0xFFFFFFFF - (win & 0xFFFFFFFF))
    if classes is not None:
        sel = torch.zeros_like(fg)
        for c in classes:
            sel |= lab == c
        remove &= sel
    return torch.where(remove, torch.full_like(lab, fill), lab).reshape(labels.shape)


def keep_largest_component(labels: torch.Tensor, **kwargs) -> torch.Tensor:
    """`filter_components` with ``keep_largest=True``: all but the largest component of every class (or of the foreground) go."""
    kwargs.setdefault("keep_largest", True)
    return filter_components(labels, **kwargs)
