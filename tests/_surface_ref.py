"""float64 restatement of the surface metrics of `calculate_metric_percase` (src/training/al_trainer.py:1539-1556), and
brute-force pairwise versions for small masks.

ASD is medpy's own scipy calls (`medpy.metric.binary.__surface_distances`, connectivity 1): `generate_binary_structure(ndim, 1)`,
`binary_erosion` (border_value 0), `distance_transform_edt(~border_B, sampling=spacing)[border_A].mean()`.  HD is
`max(edt(~B)[A].max(), edt(~A)[B].max())`: ITK's HausdorffDistanceImageFilter (`metric.cal_hd`) maps each set's signed Maurer
distance, clamped at 0, which is the distance to the nearest pixel of the other set.  medpy and SimpleITK are not importable on the
machines that run this suite, so parity with those libraries themselves is unpinned; the restatement follows their documented
definitions, and `brute_hd` / `brute_asd` pin it to the plain definitions.  Empty sets follow the project's rules: an empty
prediction gives (0, NaN, NaN, 0); an empty label gives (0, inf, inf, 0) (medpy would raise for ASD)."""
import numpy as np
from scipy import ndimage


def _sampling(spacing, ndim):
    return None if spacing is None else tuple(float(s) for s in spacing)[:ndim]


def border(mask):
    """X & ~erode(X) with the face-connected cross; everything outside the array is background."""
    mask = np.asarray(mask, dtype=bool)
    st = ndimage.generate_binary_structure(mask.ndim, 1)
    return mask ^ ndimage.binary_erosion(mask, structure=st, iterations=1, border_value=0)


def hd(a, b, spacing=None):
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    if not a.any():
        return float("nan")
    if not b.any():
        return float("inf")
    s = _sampling(spacing, a.ndim)
    return float(max(ndimage.distance_transform_edt(~b, sampling=s)[a].max(), ndimage.distance_transform_edt(~a, sampling=s)[b].max()))


def asd(a, b, spacing=None):
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    if not a.any():
        return float("nan")
    if not b.any():
        return float("inf")
    s = _sampling(spacing, a.ndim)
    return float(ndimage.distance_transform_edt(~border(b), sampling=s)[border(a)].mean())


def dc(a, b):
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    return 2.0 * np.count_nonzero(a & b) / float(np.count_nonzero(a) + np.count_nonzero(b))


def jc(a, b):
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    return np.count_nonzero(a & b) / float(np.count_nonzero(a | b))


def calculate_metric_percase(pred, gt, spacing=None):
    """(DSC, HD, ASD, JC): nothing is computed when the prediction is empty."""
    pred, gt = np.asarray(pred) > 0, np.asarray(gt) > 0
    if pred.sum() == 0:
        return 0.0, float("nan"), float("nan"), 0.0
    return dc(pred, gt), hd(pred, gt, spacing), asd(pred, gt, spacing), jc(pred, gt)


def percase_table(pred, label, num_classes, spacing=None):
    """The reference's arrays for one image or volume: (metric_all [4], metric_per_cls [num_classes, 4])."""
    pred, label = np.asarray(pred), np.asarray(label)
    m_all = np.array(calculate_metric_percase(pred > 0, label > 0, spacing))
    m_cls = np.array([calculate_metric_percase(pred == c, label == c, spacing) for c in range(1, num_classes + 1)])
    return m_all, m_cls


def surface_table(pred, label, k1, spacing=None):
    """(hd [k1], asd [k1]) for mask 0 = (pred > 0, label > 0) and mask c = (pred == c, label == c)."""
    pred, label = np.asarray(pred), np.asarray(label)
    masks = [(pred > 0, label > 0)] + [(pred == c, label == c) for c in range(1, k1)]
    return np.array([hd(a, b, spacing) for a, b in masks]), np.array([asd(a, b, spacing) for a, b in masks])


def _min_dists(src, dst, spacing):
    """For every True pixel of src, the distance to the nearest True pixel of dst (pairwise, float64)."""
    s = np.ones(src.ndim) if spacing is None else np.asarray(spacing, dtype=np.float64)[:src.ndim]
    p = np.argwhere(src) * s
    q = np.argwhere(dst) * s
    d2 = ((p[:, None, :] - q[None, :, :]) ** 2).sum(-1)
    return np.sqrt(d2.min(1))


def _brute_border(mask):
    """Border by the definition: a set pixel with a face neighbour outside the set or outside the array."""
    out = np.zeros_like(mask)
    for idx in np.argwhere(mask):
        for ax in range(mask.ndim):
            for step in (-1, 1):
                j = idx.copy()
                j[ax] += step
                if j[ax] < 0 or j[ax] >= mask.shape[ax] or not mask[tuple(j)]:
                    out[tuple(idx)] = True
    return out


def brute_hd(a, b, spacing=None):
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    if not a.any():
        return float("nan")
    if not b.any():
        return float("inf")
    return float(max(_min_dists(a, b, spacing).max(), _min_dists(b, a, spacing).max()))


def brute_asd(a, b, spacing=None):
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    if not a.any():
        return float("nan")
    if not b.any():
        return float("inf")
    return float(_min_dists(_brute_border(a), _brute_border(b), spacing).mean())
