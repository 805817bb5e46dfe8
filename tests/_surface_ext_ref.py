"""float64 restatement of the symmetric surface metrics (metric.segmentation.surface_metrics) and brute-force pairwise versions.

With dX = `border(X)` of `_surface_ref` (medpy's `__surface_distances`, connectivity 1) and
  S1 = edt(~dB)[dA]   (d(a, dB) for a in dA),   S2 = edt(~dA)[dB]   (d(b, dA) for b in dB),   n = |dA| + |dB|:
  HD_q   = `medpy.metric.binary.hd95` at q: `np.percentile(np.hstack((S1, S2)), q)`, numpy's default linear method, restated as
           pos = (n - 1) * (q / 100), k = floor(pos), v[k] + (v[min(k + 1, n - 1)] - v[k]) * (pos - k) over the sorted v
  ASSD   = `medpy.metric.binary.assd` = (S1.mean() + S2.mean()) / 2
  NSD(t) = (|S1 <= t| + |S2 <= t|) / n, the voxel-count surface Dice (MONAI `compute_surface_dice`)
medpy and MONAI are not importable on the machines that run this suite; the restatement is their scipy calls, pinned by the brute
versions below.  Empty sets follow the project's rules: empty prediction -> (NaN, NaN, 0); empty label alone -> (inf, inf, 0)."""
import math

import numpy as np
from scipy import ndimage

from _surface_ref import _brute_border, _min_dists, _sampling, border


def percentile_linear(v, q):
    """numpy's default (linear) percentile of the values v, by the formula the kernels restate."""
    v = np.sort(np.asarray(v, dtype=np.float64))
    n = v.size
    pos = float(n - 1) * (float(q) / 100.0)
    k = int(math.floor(pos))
    return float(v[k] + (v[min(k + 1, n - 1)] - v[k]) * (pos - k))


def surface_sets(a, b, spacing=None):
    """(S1, S2) for two non-empty masks."""
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    s = _sampling(spacing, a.ndim)
    da, db = border(a), border(b)
    return ndimage.distance_transform_edt(~db, sampling=s)[da], ndimage.distance_transform_edt(~da, sampling=s)[db]


def brute_sets(a, b, spacing=None):
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    da, db = _brute_border(a), _brute_border(b)
    return _min_dists(da, db, spacing), _min_dists(db, da, spacing)


def _metrics(sets, a, b, spacing, q, tau):
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    if not a.any():
        return float("nan"), float("nan"), 0.0
    if not b.any():
        return float("inf"), float("inf"), 0.0
    s1, s2 = sets(a, b, spacing)
    both = np.hstack((s1, s2))
    return (percentile_linear(both, q), float((s1.mean() + s2.mean()) / 2.0),
            float((np.count_nonzero(s1 <= tau) + np.count_nonzero(s2 <= tau)) / both.size))


def ext_metrics(a, b, spacing=None, q=95.0, tau=1.0):
    """(HD_q, ASSD, NSD(tau)) of one mask pair."""
    return _metrics(surface_sets, a, b, spacing, q, tau)


def brute_ext_metrics(a, b, spacing=None, q=95.0, tau=1.0):
    return _metrics(brute_sets, a, b, spacing, q, tau)


def masks(pred, label, k1):
    pred, label = np.asarray(pred), np.asarray(label)
    return [(pred > 0, label > 0)] + [(pred == c, label == c) for c in range(1, k1)]


def ext_table(pred, label, k1, spacing=None, q=95.0, tau=1.0):
    """(hd_pct [k1], assd [k1], nsd [k1]) for mask 0 = (pred > 0, label > 0) and mask c = (pred == c, label == c); tau is one
    number or k1 numbers."""
    taus = np.broadcast_to(np.asarray(tau, dtype=np.float64), (k1,))
    rows = [ext_metrics(a, b, spacing, q, taus[m]) for m, (a, b) in enumerate(masks(pred, label, k1))]
    return tuple(np.array([r[j] for r in rows]) for j in range(3))
