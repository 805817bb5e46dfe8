"""float64 restatement of the dual-task consistency loss (DTC: Luo et al., AAAI 2021) for the tests of csrc/dtc.hip,
losses/dual_task.py and training.semi.DTCEngine.  The definition is the module text of losses/dual_task.py; this file restates it in
numpy and adds the generators the tests share.

For z [B, K1, H, W], r [B, C, H, W] (C = K1 - 1), the first lb images labelled, phi [lb, C, H, W] the signed distance map of
tests/_boundary_ref.py at unit spacing (scipy) or the device's own map:

    m_out = max phi, m_in = max -phi per (image, class), both >= 0
    T = phi / m_out (phi > 0),  -(1 - phi) / (1 + m_in) (phi < 0),  0 (phi = 0)
    s = softmax(z), t = tanh(r), q = sigmoid(-k t), d_c = q_c - s_{c+1}
    L_cons = mean over all (n, c, p) of d^2,   L_sdf = mean over (n < lb, c, p) of (t - T)^2 (0 when lb = 0)
    L = w0 L_cons + w1 L_sdf
    dL/dz_j = c0 s_j (e_j - sum_i s_i e_i),  e_0 = 0, e_{c+1} = -d_c,  c0 = 2 w0 / (B C HW)
    dL/dr_c = [c0 d_c (-k q_c (1 - q_c)) + [n < lb] c1 (t_c - T_c)] (1 - t_c^2),  c1 = 2 w1 / (lb C HW)

Magnitudes (what a bound of "so many fp32 roundings" multiplies): the sum of the absolute values of each expression's terms, and for
everything that passes through q the first-order sensitivity k q (1 - q) |t| to one relative fp32 rounding of t:

    qm = q + k q (1 - q) |t|                       the magnitude of q
    dm = qm + s_{c+1}                              of d
    cons_mag = mean(d^2 + 2 |d| dm)                the sum's own terms, and every term's sensitivity to its d
    sdf_mag  = mean(e^2 + 2 |e| (|t| + |T|)),  e = t - T
    dz_mag_j = |c0| s_j (em_j + sum_i s_i em_i),   em_0 = 0, em_{c+1} = dm_c
    dr_mag_c = [|c0| k (dm q (1 - q) + |d| k q (1 - q) |1 - 2 q| |t|) + [n < lb] |c1| (|t| + |T|)] (1 - t^2)

(d/dt of q (1 - q) is -k q (1 - q) (1 - 2 q).)  In dr_mag the products q (1 - q) and 1 - t^2 count as ONE term each: that is the bound
for an evaluation that forms them without a subtraction, as csrc/dtc.hip does (a b from exp(-|k t|); 4 (1 + m) / (2 + m)^2 from
expm1).  An evaluation that follows the definition as it is written -- fp32 tensor ops and their autograd: `q * (1 - q)`,
`1 - t * t` -- subtracts, and each difference has the magnitude of its terms, q + q^2 and 1 + t^2; that is dr_mag_ops:

    dr_mag_ops_c = [|c0| k (dm q (1 + q) + |d| k q (1 - q) |1 - 2 q| |t|) + [n < lb] |c1| (|t| + |T|)] (1 + t^2)

dz contains neither product, so it has one magnitude.
"""
import numpy as np

SHAPES = [(1, 1, 1), (2, 1, 7), (4, 37, 61), (2, 336, 544)]
K1S = [2, 3, 8]
K_PUBLISHED = 1500.0


# ---------------------------------------------------------------- generators
def make_labels(nb, k1, h, w, seed=0):
    """int64 [nb, h, w] label maps; image n follows pattern n % 4:
      0  a blob per class; class 1's blob touches the image edge
      1  a one-pixel-wide line of class min(2, k1 - 1) (m_in = 0) on background: with k1 > 2 an image without class 1
      2  the image filled by class 1
      3  random blobs of the classes >= 2 only: an image without class 1 (all background with k1 = 2)"""
    rng = np.random.default_rng(1000 + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((nb, h, w), np.int64)
    for n in range(nb):
        kind = n % 4
        if kind == 0:
            for c in range(1, k1):
                cy, cx = (0, 0) if c == 1 else (h * (c % 3 + 1) // 4, w * c // k1)
                ry, rx = max(h // (3 + c % 2), 1), max(w // (4 + c % 3), 1)
                out[n][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = c
        elif kind == 1:
            out[n, h // 2, w // 5: max(w - w // 5, w // 5 + 1)] = min(2, k1 - 1)
        elif kind == 2:
            out[n] = 1
        else:
            f = rng.standard_normal((h, w))
            for _ in range(3):  # a cheap smoothing: neighbours' mean
                f = (f + np.roll(f, 1, 0) + np.roll(f, -1, 0) + np.roll(f, 1, 1) + np.roll(f, -1, 1)) / 5.0
            f = (f - f.mean()) / (f.std() + 1e-12)
            for c in range(2, k1):
                out[n][(f > 0.3 + 0.2 * c) & (out[n] == 0)] = c
                f = -f
    return out


def make_case(nb, k1, h, w, seed=0):
    """(z, r) fp32: z ~ 2 N(0, 1); r a fixed mix, half of the elements N(0, 1) and half 2e-3 N(0, 1), so that a good share of pixels
    sits in the steep zone of sigmoid(-1500 t) (|r| < 3e-3).  With N(0, 1) alone q is 0 or 1 nearly everywhere and a gradient test
    would show nothing of the k q (1 - q) factor."""
    rng = np.random.default_rng(2000 + seed + 7 * k1 + 13 * h + 17 * w + nb)
    z = (2.0 * rng.standard_normal((nb, k1, h, w))).astype(np.float32)
    wide = rng.standard_normal((nb, k1 - 1, h, w))
    steep = rng.random((nb, k1 - 1, h, w)) < 0.5
    r = np.where(steep, 2e-3 * wide, rng.standard_normal((nb, k1 - 1, h, w))).astype(np.float32)
    return z, r


def saturated_case(nb, k1, h, w, seed=0):
    """|z|, |r| up to 80: exp overflows in a naive soft-max, tanh is +-1 to the last bit and k t is +-1500."""
    rng = np.random.default_rng(3000 + seed + k1 + h + w)
    z = (80.0 * (2.0 * rng.random((nb, k1, h, w)) - 1.0)).astype(np.float32)
    r = (80.0 * (2.0 * rng.random((nb, k1 - 1, h, w)) - 1.0)).astype(np.float32)
    z.reshape(-1)[0] = 80.0
    r.reshape(-1)[0] = -80.0
    return z, r


def phi_scipy(labels, k1):
    """phi [B, k1 - 1, H, W] float64 by scipy (tests/_boundary_ref.py)."""
    import _boundary_ref as BR
    return BR.phi_labels(labels, k1)


# ---------------------------------------------------------------- the definition
def extents(phi):
    """[..., 2] = {max phi, max -phi} over the last two axes, both >= 0."""
    phi = np.asarray(phi, np.float64)
    return np.stack([np.maximum(phi.max((-2, -1)), 0.0), np.maximum((-phi).max((-2, -1)), 0.0)], -1)


def target(phi, ext=None):
    """T of the module text, float64."""
    phi = np.asarray(phi, np.float64)
    ext = extents(phi) if ext is None else np.asarray(ext, np.float64)
    m_out, m_in = ext[..., 0, None, None], ext[..., 1, None, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        outside = phi / np.where(m_out > 0, m_out, 1.0)
    inside = -(1.0 - phi) / (1.0 + m_in)
    return np.where(phi > 0, outside, np.where(phi < 0, inside, 0.0))


def published_sdf(mask):
    """The steps of the published `compute_sdf` for one boolean mask [H, W] with scipy, boundary = (edt == 1); None where the
    published code writes nothing (an empty mask).  Not finite where it divides 0 by 0 (a mask that fills the image)."""
    from scipy.ndimage import distance_transform_edt as distance
    posmask = np.asarray(mask, bool)
    if not posmask.any():
        return None
    negmask = ~posmask
    posdis, negdis = distance(posmask), distance(negmask)
    boundary = posdis == 1
    with np.errstate(divide="ignore", invalid="ignore"):
        sdf = (negdis - negdis.min()) / (negdis.max() - negdis.min()) - (posdis - posdis.min()) / (posdis.max() - posdis.min())
    sdf[boundary] = 0
    return sdf


def softmax(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def sigmoid_parts(x):
    """(q, q (1 - q)) of sigmoid(x) from exp(-|x|): finite for any x."""
    e = np.exp(-np.abs(x))
    a, b = 1.0 / (1.0 + e), e / (1.0 + e)
    return np.where(x >= 0, a, b), a * b


def evaluate(z, r, phi, lb, k=K_PUBLISHED, w0=1.0, w1=1.0):
    """Everything the tests compare, float64: ext, T, cons, sdf, value, their magnitudes, dz, dr and their magnitudes."""
    z, r = np.asarray(z, np.float64), np.asarray(r, np.float64)
    nb, k1, h, w = z.shape
    c = k1 - 1
    n_all = float(nb * c * h * w)
    s = softmax(z)
    t = np.tanh(r)
    sech2 = 1.0 / np.cosh(r) ** 2
    q, qq = sigmoid_parts(-k * t)
    d = q - s[:, 1:]
    qm = q + k * qq * np.abs(t)
    dm = qm + s[:, 1:]
    cons = (d * d).sum() / n_all
    cons_mag = (d * d + 2.0 * np.abs(d) * dm).sum() / n_all
    c0 = 2.0 * w0 / n_all
    ez = np.zeros_like(s)
    ez[:, 1:] = -d
    em = np.zeros_like(s)
    em[:, 1:] = dm
    dz = c0 * s * (ez - (s * ez).sum(1, keepdims=True))
    dz_mag = abs(c0) * s * (em + (s * em).sum(1, keepdims=True))
    a = c0 * d * (-k * qq)
    sens = np.abs(d) * k * qq * np.abs(1.0 - 2.0 * q) * np.abs(t)
    a_mag = abs(c0) * k * (dm * qq + sens)
    a_mag_ops = abs(c0) * k * (dm * q * (1.0 + q) + sens)
    out = {"cons": cons, "cons_mag": cons_mag, "sdf": 0.0, "sdf_mag": 0.0, "ext": None, "T": None}
    if lb > 0:
        phi = np.asarray(phi, np.float64)
        assert phi.shape == (lb, c, h, w)
        n_sdf = float(lb * c * h * w)
        ext = extents(phi)
        T = target(phi, ext)
        e = t[:lb] - T
        out["sdf"] = (e * e).sum() / n_sdf
        out["sdf_mag"] = (e * e + 2.0 * np.abs(e) * (np.abs(t[:lb]) + np.abs(T))).sum() / n_sdf
        c1 = 2.0 * w1 / n_sdf
        a[:lb] += c1 * e
        a_mag[:lb] += abs(c1) * (np.abs(t[:lb]) + np.abs(T))
        a_mag_ops[:lb] += abs(c1) * (np.abs(t[:lb]) + np.abs(T))
        out["ext"], out["T"] = ext, T
    out["value"] = w0 * out["cons"] + w1 * out["sdf"]
    out["value_mag"] = abs(w0) * out["cons_mag"] + abs(w1) * out["sdf_mag"]
    out["dz"], out["dz_mag"] = dz, dz_mag
    out["dr"], out["dr_mag"], out["dr_mag_ops"] = a * sech2, a_mag * sech2, a_mag_ops * (1.0 + t * t)
    out["q"] = q
    return out


def torch_loss(z, r, T, lb, k=K_PUBLISHED, w0=1.0, w1=1.0):
    """The plain formula in float64 torch, for autograd: (L, L_cons, L_sdf)."""
    import torch
    s = torch.softmax(z, 1)
    t = torch.tanh(r)
    q = torch.sigmoid(-k * t)
    cons = ((q - s[:, 1:]) ** 2).mean()
    sdf = ((t[:lb] - torch.as_tensor(T, dtype=torch.float64)) ** 2).mean() if lb > 0 else torch.zeros((), dtype=torch.float64)
    return w0 * cons + w1 * sdf, cons, sdf
