"""Float64 restatement of the normalisation + Dropout2d + LeakyReLU family of csrc/norm.hip (test infrastructure only), the
synthetic conv-epilogue partials its finalize kernels consume, and the seeded case table that tests/test_norm_host.py (CPU)
and tests/test_gpu_norm.py (GPU) share.  Activations are NHWC with the pixels flattened: [N, P, C].

    y' = m[n,c] * y                                         (m = 0 or 1/keep, the Dropout2d channel mask; 1 in eval mode)
    mean', var' = statistics of y' per (n, c) (instance) or per c over the batch (batch); biased variance
    rstd' = 1 / sqrt(var' + eps)
    xhat = (y' - mean') * rstd' = xa * y + xb               xa = m rstd',  xb = -m mean rstd' (instance), -mean'_batch rstd' (batch)
    z = lrelu(gamma * xhat + beta) = lrelu(scale * y + shift)     scale = gamma xa,  shift = gamma xb + beta
    ysum = sum_p y

Frozen statistics (eval-mode batch norm) take mean', var' from the running statistics, which are constants in backward.  Gradients
come from autograd over these float64 expressions; the group means c1 = mean(g), c2 = mean(g * xhat) with g = dz * lrelu'(v) are
restated directly (0 under frozen statistics)."""
import functools

import numpy as np
import torch

EPS = float(np.float32(1e-5))   # the kernels take eps / momentum as C floats
MOM = float(np.float32(0.1))
SLOPE = 0.01
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
NEAR_ZERO = {"f32": 2.0 ** -20, "bf16": 2.0 ** -7}  # |v| below this fraction of max|v| may land on the other LeakyReLU branch
MAX_EXCLUDED = 0.01


def f64(x):
    return None if x is None else torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).detach().to(torch.float64).clone()


def lrelu(v, slope):
    return torch.where(v > 0, v, v * slope)


def coefficients(s1, s2, hw, gamma, beta, mode, m=None, training=True, running=None, eps=EPS, momentum=MOM):
    """The five [N, C] coefficient rows (xa, xb, scale, shift, ysum) from the per-(n, c) sums s1 = sum y, s2 = sum y^2 over hw
    pixels, plus `running` = (mean, unbiased var) after one momentum update (batch mode in training, else None / unchanged)."""
    n, c = s1.shape
    m = torch.ones_like(s1) if (m is None or not training) else m
    new_running = running
    if mode == "instance":
        mean = s1 / hw
        var = torch.clamp(s2 / hw - mean * mean, min=0.0)
        rstd = 1.0 / torch.sqrt(m * m * var + eps)
        xa, xb = m * rstd, -m * mean * rstd
    else:
        assert mode == "batch"
        if training:
            cnt = float(n * hw)
            mean = (m * s1).sum(0) / cnt
            var = torch.clamp((m * m * s2).sum(0) / cnt - mean * mean, min=0.0)
            if running is not None:
                unb = var * cnt / (cnt - 1.0) if cnt > 1 else var
                new_running = ((1.0 - momentum) * running[0] + momentum * mean.detach(),
                               (1.0 - momentum) * running[1] + momentum * unb.detach())
        else:
            mean, var = running
        rstd = 1.0 / torch.sqrt(var + eps)
        xa, xb = m * rstd, (-mean * rstd).expand(n, c)
    return dict(xa=xa, xb=xb, scale=gamma * xa, shift=gamma * xb + beta, ysum=s1, running=new_running)


def norm_act(y, gamma, beta, dz, mode, m=None, dz2=None, slope=SLOPE, training=True, running=None, eps=EPS, momentum=MOM):
    """Forward and backward of one block's Dropout2d -> norm -> LeakyReLU on y [N, P, C]; the output gradient dz comes in one piece
    or two (dz + dz2).  training=False (batch mode only) freezes the statistics at `running`.  Everything returned is float64."""
    y = f64(y).requires_grad_(True)
    gamma, beta = f64(gamma).requires_grad_(True), f64(beta).requires_grad_(True)
    m, dz = f64(m), f64(dz)
    running = None if running is None else (f64(running[0]), f64(running[1]))
    if dz2 is not None:
        dz = dz + f64(dz2)
    n, hw, c = y.shape
    frozen = mode == "batch" and not training
    co = coefficients(y.sum(1), (y * y).sum(1), hw, gamma, beta, mode, m, training, running, eps, momentum)
    v = co["scale"][:, None, :] * y + co["shift"][:, None, :]
    z = lrelu(v, slope)
    z.backward(dz)
    dy = y.grad
    with torch.no_grad():
        g = dz * torch.where(v > 0, torch.ones_like(v), torch.full_like(v, slope))
        gx = g * (co["xa"][:, None, :] * y + co["xb"][:, None, :])
        if frozen:
            c1, c2 = torch.zeros(n, c, dtype=torch.float64), torch.zeros(n, c, dtype=torch.float64)
        elif mode == "instance":
            c1, c2 = g.mean(1), gx.mean(1)
        else:
            c1, c2 = g.mean((0, 1)).expand(n, c).clone(), gx.mean((0, 1)).expand(n, c).clone()
    out = {k: co[k].detach() for k in ("xa", "xb", "scale", "shift", "ysum")}
    out.update(v=v.detach(), z=z.detach(), dy=dy, dgamma=gamma.grad, dbeta=beta.grad, dbias=dy.sum((0, 1)), c1=c1, c2=c2,
               sg=g.sum(1), sgx=gx.sum(1),
               running_mean=None if co["running"] is None else co["running"][0],
               running_var=None if co["running"] is None else co["running"][1])
    return out


def norm_act_world(shards, gamma, beta, slope=SLOPE, running=None, eps=EPS, momentum=MOM):
    """The "world" view of synchronised batch norm: `shards` is a list of dict(y, dz, m[, dz2]), one per rank; the answer is
    norm_act in batch mode on the concatenated batch, plus `slices` (each rank's rows of the batch)."""
    cat = lambda k: None if shards[0].get(k) is None else torch.cat([f64(s[k]) for s in shards], 0)
    out = norm_act(cat("y"), gamma, beta, cat("dz"), "batch", m=cat("m"), dz2=cat("dz2"), slope=slope, training=True,
                   running=running, eps=eps, momentum=momentum)
    edges = np.cumsum([0] + [len(s["y"]) for s in shards])
    out["slices"] = [slice(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]
    return out


def scale_lrelu(v, m, dz, slope=SLOPE):
    """z = lrelu(m * v) and dv = m * dz * lrelu'(m * v): Dropout2d behind the norm (the ScaleLReLUFn call shape)."""
    v, m, dz = f64(v), f64(m), f64(dz)
    mv = m[:, None, :] * v
    return dict(z=lrelu(mv, slope), dv=m[:, None, :] * dz * torch.where(mv > 0, torch.ones_like(mv), torch.full_like(mv, slope)))


def epilogue_partials(y, tiles, seed=0):
    """Synthetic conv-epilogue partials: the P pixels of y [N, P, C] (fp32, or bf16 widened) are cut into `tiles` contiguous,
    non-empty, ragged pieces (seeded cut points, one set per image); returns fp32 [N, tiles, C, 2] (sum, sum of squares), each
    accumulated in float64 and rounded ONCE to fp32 -- the kernel and the reference consume the same fp32 numbers."""
    a = np.asarray(f64(y))
    n, p, c = a.shape
    assert 1 <= tiles <= p, "every tile holds at least one pixel"
    rng = np.random.default_rng(seed)
    out = np.empty((n, tiles, c, 2), dtype=np.float32)
    for i in range(n):
        starts = np.concatenate([[0], np.sort(rng.choice(np.arange(1, p), size=tiles - 1, replace=False))]).astype(np.int64)
        out[i, :, :, 0] = np.add.reduceat(a[i], starts, axis=0).astype(np.float32)
        out[i, :, :, 1] = np.add.reduceat(a[i] * a[i], starts, axis=0).astype(np.float32)
    return torch.from_numpy(out)


def near_zero(v, dt):
    """Elements whose float64 pre-activation is within rounding of the LeakyReLU kink for storage dtype `dt`: the only ones the
    dy comparison may skip (a condition on the REFERENCE, never on what a kernel returned)."""
    return v.abs() < NEAR_ZERO[dt] * v.abs().max()


# ------------------------------------------------------------------ the shared, seeded case table
HW_RAGGED = 37 * 53                       # 1961 pixels: no multiple of any lane count, last slab ragged for slabs = 3, 7
BWD_CHANNELS = (7, 12, 20, 24, 32, 64, 96, 160, 224, 288)
FWD_CHANNELS = (7, 12, 20, 24, 32, 96, 160)
FWD_HW = (3 * 5, 16 * 16, 37 * 53)
LONG_SLAB = dict(n=3, hw=40 * 40, slabs=400, channels=(40, 64))
SYNC_SPLITS = ((1, 3), (2, 2))
SYNC_CHANNELS = (20, 64)
# (images, tiles) of the finalize tests; (5, 250) puts a lane of the 1024-thread sum kernel on its unrolled loop's guard boundary
FINALIZE_NT = ((2, 1), (3, 300), (4, 300), (4, 517), (2, 1025), (5, 250))
FINALIZE_P = 1153                          # pixels behind the synthetic partials: >= the longest tile table, every tile non-empty
KEEP = 0.5                                 # Dropout2d keep probability of the masks: 1/keep = 2 is exact in every dtype


def _key(c, dt, mode, n=3, hw=HW_RAGGED, frozen=False):
    return (c, dt, mode, n, hw, frozen)


def dy_cases():
    """Every input set whose dy a GPU test compares with the restatement: (channels, dtype, mode, images, pixels, frozen)."""
    keys = []
    for c in BWD_CHANNELS:
        for dt in DT:
            for mode in ("instance", "batch"):
                keys.append(_key(c, dt, mode))
    for c in LONG_SLAB["channels"]:
        for dt in DT:
            for mode in ("instance", "batch"):
                keys.append(_key(c, dt, mode, LONG_SLAB["n"], LONG_SLAB["hw"]))
    for c in (20, 64):
        for dt in DT:
            keys.append(_key(c, dt, "batch", frozen=True))
    for c in SYNC_CHANNELS:
        for dt in DT:
            keys.append(_key(c, dt, "batch", 4))
    return keys


def drop_mask(gen, n, c):
    """[N, C] Dropout2d multipliers in {0, 1/keep}; entry (0, 0) is an exact 0 and (1 % n, 0) is 1/keep."""
    m = (torch.rand(n, c, generator=gen) < 0.75).double() / KEEP
    m[0, 0] = 0.0
    m[(1 % n), 0 if n > 1 else c - 1] = 1.0 / KEEP
    return m


def make_inputs(key):
    """Seeded inputs of one dy case, quantised to the storage dtype.  The LeakyReLU branch is decided in fp32 by the kernels and in
    float64 here, so the inputs keep the pre-activations away from zero: y - mu is bimodal (|y - mu| in [0.7, 1.4] times a
    channel scale), |mu| <= 0.3 channel scales, and beta in +-[0.1, 0.2] with the sign opposite to mu, which keeps a DROPPED
    channel's constant pre-activation beta - gamma mean' rstd' away from zero too.  tests/test_norm_host.py checks the outcome."""
    c, dt, mode, n, hw, frozen = key
    assert key in dy_cases(), "a GPU test may only use inputs of the shared case table"
    gen = torch.Generator().manual_seed(1000 * c + 10 * n + hw + (1 if dt == "bf16" else 0) + (2 if mode == "batch" else 0) + (4 if frozen else 0))
    q = lambda t: t.to(DT[dt]).double()
    sgn = lambda *s: torch.where(torch.rand(*s, generator=gen) < 0.5, -1.0, 1.0).double()
    sigma = 0.5 + 1.5 * torch.rand(c, generator=gen).double()
    mu = sgn(c) * (0.1 + 0.2 * torch.rand(c, generator=gen).double())
    y = q(sigma * (mu + sgn(n, hw, c) * (0.7 + 0.7 * torch.rand(n, hw, c, generator=gen).double())))
    dz = q(torch.randn(n, hw, c, generator=gen).double())
    dz2 = q(torch.randn(n, hw, c, generator=gen).double()) if c % 32 == 0 else None  # wherever mia_norm_two_piece_ok holds
    gamma = (0.8 + 0.4 * torch.rand(c, generator=gen).double()).float().double()
    beta = (-torch.sign(mu) * (0.1 + 0.1 * torch.rand(c, generator=gen).double())).float().double()
    m = drop_mask(gen, n, c)
    running = None
    if mode == "batch":
        # running statistics that differ from the batch's own: mean off by 0.1 channel scales, variance 1.5 times larger
        running = ((sigma * (mu + 0.1)).float().double(), (1.5 * sigma * sigma * 1.15).float().double())
    return dict(y=y, dz=dz, dz2=dz2, gamma=gamma, beta=beta, m=m, running=running)


@functools.lru_cache(maxsize=3)
def reference(key, pieces=None):
    """(inputs, norm_act answer) of one case of the table, computed once and shared; callers leave both unchanged.  pieces=1
    ignores the second gradient piece."""
    c, dt, mode, n, hw, frozen = key
    i = make_inputs(key)
    dz2 = None if pieces == 1 else i["dz2"]
    r = norm_act(i["y"], i["gamma"], i["beta"], i["dz"], mode, m=i["m"], dz2=dz2, training=not frozen, running=i["running"])
    return i, r


def finalize_inputs(n, c, r, seed, p=FINALIZE_P):
    """y [n, p, c] fp32-representable with per-channel mean = +-r * std (std in [0.5, 2]), gamma, beta, a Dropout2d mask
    and running statistics for the finalize tests."""
    gen = torch.Generator().manual_seed(seed)
    sigma = 0.5 + 1.5 * torch.rand(c, generator=gen).double()
    sgn = torch.where(torch.rand(c, generator=gen) < 0.5, -1.0, 1.0).double()
    y = (sigma * (r * sgn + torch.randn(n, p, c, generator=gen).double())).float().double()
    gamma = (0.8 + 0.4 * torch.rand(c, generator=gen).double()).float().double()
    beta = (0.3 * torch.randn(c, generator=gen).double()).float().double()
    running = ((0.5 * torch.randn(c, generator=gen).double()).float().double(), (0.5 + torch.rand(c, generator=gen).double()).float().double())
    return dict(y=y, gamma=gamma, beta=beta, m=drop_mask(gen, n, c), running=running)
