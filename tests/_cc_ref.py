"""Connected components restated with scipy: the reference for `inference.components` and csrc/components.hip.

For every image and class (or the foreground): `ndimage.label` with `generate_binary_structure(ndim, connectivity)`; the root map
from `ndimage.minimum(linear_index, cc, index)`; sizes by `bincount`; the winner by `argmax` -- the first maximum is the component
with the lowest root, because scipy numbers components in raster order.  All comparisons against it are exact."""
import numpy as np
from scipy import ndimage


def _images(labels, ndim):
    """[nimg, ...image dims] view of the label maps."""
    a = np.asarray(labels)
    return a.reshape((-1,) + a.shape[a.ndim - ndim:])


def _masks(img, n_classes, foreground, classes=None):
    """[(class or None, mask)] whose components are to be found."""
    valid = (img >= 1) & (img < n_classes)
    if foreground:
        return [(None, valid)]
    return [(c, img == c) for c in (range(1, n_classes) if classes is None else classes)]


def label_one(mask, ndim, connectivity):
    return ndimage.label(mask, structure=ndimage.generate_binary_structure(ndim, connectivity))


def roots(labels, ndim=2, connectivity=1, n_classes=3, foreground=False):
    """int32 root map: 1 + the smallest linear index (within the image) of the voxel's component, 0 elsewhere."""
    imgs = _images(labels, ndim)
    out = np.zeros(imgs.shape, dtype=np.int32)
    for i, img in enumerate(imgs):
        lin = np.arange(img.size, dtype=np.int64).reshape(img.shape)
        for _, mask in _masks(img, n_classes, foreground):
            cc, n = label_one(mask, ndim, connectivity)
            if n == 0:
                continue
            lowest = np.asarray(ndimage.minimum(lin, cc, index=np.arange(1, n + 1)), dtype=np.int64)
            out[i][mask] = (lowest[cc[mask] - 1] + 1).astype(np.int32)
    return out.reshape(np.asarray(labels).shape)


def compact(labels, ndim=2, connectivity=1, n_classes=3):
    """scipy's own numbering of the object mask (all labels in [1, n_classes) as one mask), int32."""
    imgs = _images(labels, ndim)
    out = np.zeros(imgs.shape, dtype=np.int32)
    for i, img in enumerate(imgs):
        out[i] = label_one((img >= 1) & (img < n_classes), ndim, connectivity)[0]
    return out.reshape(np.asarray(labels).shape)


def filtered(labels, keep_largest=True, min_size=0, classes=None, foreground=False, fill=0, ndim=2, connectivity=1, n_classes=3):
    """The label maps with every component below min_size, and with keep_largest every component but the largest of its
    (image, class) -- of its image with `foreground` -- set to `fill`."""
    src = np.asarray(labels)
    imgs = _images(src, ndim)
    out = imgs.copy()
    for i, img in enumerate(imgs):
        for _, mask in _masks(img, n_classes, foreground, classes):
            cc, n = label_one(mask, ndim, connectivity)
            if n == 0:
                continue
            sizes = np.bincount(cc.ravel(), minlength=n + 1)[1:]
            drop = sizes < min_size
            if keep_largest:
                drop |= np.arange(n) != int(np.argmax(sizes))
            out[i][mask & np.concatenate(([False], drop))[cc]] = fill
    return out.reshape(src.shape)


# ------------------------------------------------------------------ inputs shared by the CPU and GPU tests
def random_labels(shape, density, seed, n_labels=3):
    """Labels 0 .. n_labels-1: a voxel is set with probability `density`, its class uniform over the non-zero labels."""
    g = np.random.default_rng(seed)
    on = g.random(shape) < density
    return np.where(on, g.integers(1, n_labels, size=shape), 0).astype(np.int64)
