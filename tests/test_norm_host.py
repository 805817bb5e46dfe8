"""CPU checks of the float64 restatement of the norm kernels (tests/_norm_ref.py): against torch's own instance / batch norm +
leaky_relu in float64 with autograd, the synthetic conv-epilogue partials against direct sums, and -- for every input set of the
GPU grid in tests/test_gpu_norm.py -- the condition under which the dy comparison may skip an element.  None of it needs a GPU."""
import pytest
import torch
import torch.nn.functional as F

import _norm_ref as R

RTOL = 1e-12


def close(got, want, what, scale=None):
    err = (got - want).abs().max().item() / max(want.abs().max().item() if scale is None else scale, 1e-300)
    assert err < RTOL, f"{what}: {err:.3e}"


def nchw(t, h, w):  # [N, P, C] -> [N, C, H, W]
    n, p, c = t.shape
    return t.reshape(n, h, w, c).permute(0, 3, 1, 2)


def npc(t):  # [N, C, H, W] -> [N, P, C]
    n, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(n, h * w, c)


def _inputs(seed, n=3, h=5, w=7, c=6):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(y=rnd(n, h * w, c) * 1.7 + rnd(c), dz=rnd(n, h * w, c), dz2=rnd(n, h * w, c), gamma=1 + 0.3 * rnd(c), beta=0.3 * rnd(c),
                m=R.drop_mask(g, n, c), running=(rnd(c), 0.5 + torch.rand(c, generator=g, dtype=torch.float64)), h=h, w=w)


@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("mode", ["instance", "batch", "batch_eval"])
@pytest.mark.parametrize("slope", [0.01, 1.0])
def test_restatement_matches_torch_norm_and_leaky_relu(slope, mode, drop, pieces):
    i = _inputs(11 + pieces + 2 * drop)
    h, w = i["h"], i["w"]
    training = mode != "batch_eval"
    m = i["m"] if drop else None
    got = R.norm_act(i["y"], i["gamma"], i["beta"], i["dz"], "instance" if mode == "instance" else "batch", m=m,
                     dz2=i["dz2"] if pieces == 2 else None, slope=slope, training=training, running=i["running"])
    y = nchw(i["y"], h, w).clone().requires_grad_(True)
    gamma, beta = i["gamma"].clone().requires_grad_(True), i["beta"].clone().requires_grad_(True)
    yp = y * i["m"][:, :, None, None] if (drop and training) else y  # Dropout2d is the identity in eval mode
    rm, rv = i["running"][0].clone(), i["running"][1].clone()
    if mode == "instance":
        zn = F.instance_norm(yp, weight=gamma, bias=beta, eps=R.EPS)
    else:
        zn = F.batch_norm(yp, rm, rv, gamma, beta, training, R.MOM, R.EPS)
    z = F.leaky_relu(zn, slope)
    dz = nchw(i["dz"] + (i["dz2"] if pieces == 2 else 0), h, w)
    z.backward(dz)
    close(got["z"], npc(z.detach()), "z")
    close(got["dy"], npc(y.grad), "dy")
    close(got["dgamma"], gamma.grad, "dgamma")
    close(got["dbeta"], beta.grad, "dbeta")
    # analytically 0 while the statistics are live (the mean is removed): relative to the sums of |dy| it is made of
    close(got["dbias"], y.grad.sum((0, 2, 3)), "dbias", scale=y.grad.abs().sum((0, 2, 3)).max().item())
    close(got["ysum"], i["y"].sum(1), "ysum")
    if mode == "batch":
        close(got["running_mean"], rm, "running_mean")
        close(got["running_var"], rv, "running_var")
    if mode == "batch_eval":
        assert torch.equal(got["running_mean"], i["running"][0]) and torch.equal(got["running_var"], i["running"][1])
        assert not got["c1"].any() and not got["c2"].any()
    # the coefficient rows in the kernels' definitions reproduce z, and the group means reproduce dy:
    # dy = scale * (g - c1 - xhat c2)
    v = got["scale"][:, None] * i["y"] + got["shift"][:, None]
    close(R.lrelu(v, slope), got["z"], "z from scale / shift")
    close(i["gamma"] * got["xa"], got["scale"], "scale = gamma xa")
    close(i["gamma"] * got["xb"] + i["beta"], got["shift"], "shift = gamma xb + beta")
    g = (i["dz"] + (i["dz2"] if pieces == 2 else 0)) * torch.where(v > 0, torch.ones_like(v), torch.full_like(v, slope))
    xhat = got["xa"][:, None] * i["y"] + got["xb"][:, None]
    close(got["scale"][:, None] * (g - got["c1"][:, None] - xhat * got["c2"][:, None]), got["dy"], "dy from c1 / c2")


def test_world_view_is_the_batch_of_all_shards():
    i = _inputs(5, n=4)
    whole = R.norm_act(i["y"], i["gamma"], i["beta"], i["dz"], "batch", m=i["m"], dz2=i["dz2"], running=i["running"])
    for split in ((1, 3), (2, 2)):
        edges = [0, split[0], 4]
        shards = [dict(y=i["y"][a:b], dz=i["dz"][a:b], dz2=i["dz2"][a:b], m=i["m"][a:b]) for a, b in zip(edges[:-1], edges[1:])]
        got = R.norm_act_world(shards, i["gamma"], i["beta"], running=i["running"])
        assert got["slices"] == [slice(0, split[0]), slice(split[0], 4)]
        for k in ("z", "dy", "dgamma", "dbeta", "dbias", "scale", "shift", "running_mean", "running_var", "c1", "c2"):
            assert torch.equal(got[k], whole[k]), k


def test_scale_lrelu_matches_autograd():
    i = _inputs(9)
    v = i["y"].clone().requires_grad_(True)
    z = F.leaky_relu(i["m"][:, None] * v, 0.01)
    z.backward(i["dz"])
    got = R.scale_lrelu(i["y"], i["m"], i["dz"], 0.01)
    close(got["z"], z.detach(), "z")
    close(got["dv"], v.grad, "dv")


@pytest.mark.parametrize("tiles", [1, 7, 300, R.FINALIZE_P])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_partials_sum_to_the_direct_sums(tiles, dt):
    i = R.finalize_inputs(3, 20, 2.0, seed=tiles)
    y = i["y"].to(R.DT[dt]).double()
    part = R.epilogue_partials(y, tiles, seed=3)
    assert part.dtype == torch.float32 and tuple(part.shape) == (3, tiles, 20, 2)
    assert bool((part[..., 1] > 0).all()), "every tile holds at least one pixel"
    # each partial is one fp32 rounding of a float64 sum: the total is within tiles half-ulps of its largest partial
    for k, direct in enumerate((y.sum(1), (y * y).sum(1))):
        err = (part[..., k].double().sum(1) - direct).abs()
        bound = 2.0 ** -24 * part[..., k].double().abs().sum(1) + 1e-12
        assert bool((err <= bound).all())
    if tiles == 1:
        assert torch.equal(part[:, 0, :, 0], y.sum(1).float()) and torch.equal(part[:, 0, :, 1], (y * y).sum(1).float())
    again = R.epilogue_partials(y, tiles, seed=3)
    assert torch.equal(part, again), "seeded"


def test_mask_has_a_dropped_and_a_kept_channel():
    for n, c in ((1, 20), (2, 20), (4, 64)):
        m = R.drop_mask(torch.Generator().manual_seed(n), n, c)
        vals = set(m.unique().tolist())
        assert vals == {0.0, 1.0 / R.KEEP}


def test_case_table_is_unique_and_small():
    keys = R.dy_cases()
    assert len(keys) == len(set(keys))
    for c, dt, mode, n, hw, frozen in keys:
        assert n <= 5 and hw <= 2000


@pytest.mark.parametrize("key", R.dy_cases(), ids=lambda k: "-".join(str(x) for x in k))
def test_near_zero_exclusion_stays_under_one_percent(key):
    """The dy comparison of the GPU tests may skip only |v| < 2^-20 max|v| (fp32) or 2^-7 max|v| (bf16) of the REFERENCE
    pre-activation, and at most 1 % of a case: checked here for every input of the GPU grid, from the reference alone."""
    dt = key[1]
    i, r = R.reference(key)
    frac = R.near_zero(r["v"], dt).double().mean().item()
    assert frac <= R.MAX_EXCLUDED, f"{frac:.4f} of the elements sit on the LeakyReLU kink"
    # inputs are exactly representable in the storage dtype, the mask holds both values
    assert torch.equal(i["y"].to(R.DT[dt]).double(), i["y"]) and torch.equal(i["dz"].to(R.DT[dt]).double(), i["dz"])
    assert set(i["m"].unique().tolist()) == {0.0, 1.0 / R.KEEP}
    if i["dz2"] is not None:
        r1 = R.reference(key, 1)[1]
        assert not torch.equal(r1["dy"], r["dy"])
