"""CPU checks of the float64 restatement in tests/_head_loss_ref.py: against torch's conv2d / leaky_relu / autograd and the loss
oracle (oracle/losses_ref.py) in float64, the shared case tables (unique, small), the cap on what the head-fed dy comparison of
tests/test_gpu_head_loss.py may skip, and the hand-built loss inputs.  None of it needs a GPU."""
import pytest
import torch
import torch.nn.functional as F

import _head_loss_ref as R
import _norm_ref as N
from oracle import losses_ref

RTOL = 1e-12


def close(got, want, what):
    err = (got - want).abs().max().item() / max(want.abs().max().item(), 1e-300)
    assert err < RTOL, f"{what}: {err:.3e}"


def nchw(t, h, w):  # [N, P, C] -> [N, C, H, W]
    n, p, c = t.shape
    return t.reshape(n, h, w, c).permute(0, 3, 1, 2)


def npc(t):  # [N, C, H, W] -> [N, P, C]
    n, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(n, h * w, c)


@pytest.mark.parametrize("k1,c0", [(1, 7), (3, 16), (8, 40)])
def test_head_matches_conv2d(k1, c0):
    i = R.head_inputs("f32", c0, k1, 2, 5 * 7)
    got = R.head(i["x"], i["w"], i["b"], i["dl"])
    x, w, b = nchw(i["x"], 5, 7).clone().requires_grad_(True), i["w"].reshape(k1, c0, 1, 1).clone().requires_grad_(True), i["b"].clone().requires_grad_(True)
    out = F.conv2d(x, w, b)
    out.backward(nchw(i["dl"], 5, 7))
    close(got["logits"], npc(out.detach()), "logits")
    close(got["dx"], npc(x.grad), "dx")
    close(got["dw"], w.grad.reshape(k1, c0), "dW")
    close(got["db"], b.grad, "db")


@pytest.mark.parametrize("slope", [0.01, 1.0])
def test_fused_head_matches_leaky_relu_then_conv2d(slope):
    k1, c0, h, w_ = 3, 16, 5, 7
    i = R.fused_inputs("bf16", c0, k1, 2, h * w_)
    got = R.head_norm(i["y"], i["scale"], i["shift"], slope, i["w"], i["b"], i["dl"])
    w, b = i["w"].reshape(k1, c0, 1, 1).clone().requires_grad_(True), i["b"].clone().requires_grad_(True)
    x = F.leaky_relu(nchw(i["y"], h, w_) * i["scale"][:, :, None, None] + i["shift"][:, :, None, None], slope)
    out = F.conv2d(x, w, b)
    out.backward(nchw(i["dl"], h, w_))
    close(got["logits"], npc(out.detach()), "logits")
    close(got["dw"], w.grad.reshape(k1, c0), "dW")
    close(got["db"], b.grad, "db")
    assert bool((i["scale"] == 0).any()), "a dropped channel"


@pytest.mark.parametrize("mode", ["instance", "batch", "batch_eval"])
def test_head_fed_backward_matches_norm_leaky_relu_conv2d(mode):
    """The whole chain conv output -> Dropout2d -> norm -> LeakyReLU -> 1x1 head under autograd."""
    n, h, w_, c, k1 = 3, 5, 7, 6, 3
    g = torch.Generator().manual_seed(4)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    y0, gamma0, beta0, m = rnd(n, h * w_, c) * 1.7 + rnd(c), 1 + 0.3 * rnd(c), 0.3 * rnd(c), N.drop_mask(g, n, c)
    running = (rnd(c), 0.5 + torch.rand(c, generator=g, dtype=torch.float64))
    wh, dl = rnd(k1, c), rnd(n, h * w_, k1)
    training = mode != "batch_eval"
    got = R.head_fed_norm_bwd(y0, gamma0, beta0, wh, dl, "instance" if mode == "instance" else "batch", m=m, training=training, running=running)
    y = nchw(y0, h, w_).clone().requires_grad_(True)
    gamma, beta, w = gamma0.clone().requires_grad_(True), beta0.clone().requires_grad_(True), wh.reshape(k1, c, 1, 1).clone().requires_grad_(True)
    yp = y * m[:, :, None, None] if training else y
    if mode == "instance":
        zn = F.instance_norm(yp, weight=gamma, bias=beta, eps=N.EPS)
    else:
        zn = F.batch_norm(yp, running[0].clone(), running[1].clone(), gamma, beta, training, N.MOM, N.EPS)
    F.conv2d(F.leaky_relu(zn, N.SLOPE), w).backward(nchw(dl, h, w_))
    close(got["dy"], npc(y.grad), "dy")
    close(got["dgamma"], gamma.grad, "dgamma")
    close(got["dbeta"], beta.grad, "dbeta")
    close(got["dw"], w.grad.reshape(k1, c), "head dW")
    close(got["db"], dl.sum((0, 1)), "head db")


@pytest.mark.parametrize("softmax,do_bg,batch,squared", R.LOSS_FLAGS)
@pytest.mark.parametrize("special", [None, "absent", "one_class"])
def test_dice_ce_matches_the_oracle_under_autograd(softmax, do_bg, batch, squared, special):
    nb, h, w_, k1 = 4, 4, 5, 3  # four images: the oracle keeps its one-hot target in fp32, where a batch mean over 4 is exact
    logits, labels = R.loss_inputs(nb, h * w_, k1, softmax=softmax, special=special)
    dice_w, ce_w = 0.6, 0.9
    got = R.dice_ce(logits, labels, softmax, do_bg, batch, squared, dice_w=dice_w, ce_w=ce_w, gout=R.LOSS_GOUT)
    v = nchw(logits, h, w_).clone().requires_grad_(True)
    lab = labels.reshape(nb, h, w_)
    ref = losses_ref.dice_and_ce(v, lab, k1 - 1, dice_w, ce_w, smooth=R.SMOOTH, do_bg=do_bg, softmax=softmax, batch=batch, squared=squared)
    (R.LOSS_GOUT * ref).backward()
    close(got["out"][0], ref.detach(), "loss")
    close(got["out"][1], losses_ref.ce_loss(v.detach(), lab), "ce")
    close(got["out"][2], losses_ref.dice_loss(v.detach(), lab, k1 - 1, R.SMOOTH, do_bg, softmax, batch, squared), "dice")
    close(got["dlogits"], npc(v.grad), "dlogits")
    close(got["sums"][..., 2], F.one_hot(labels, k1).double().sum(1), "label counts")
    # coef is the derivative of the dice term with respect to the sums I and S
    I = got["sums"][..., 0].clone().requires_grad_(True)
    S = got["sums"][..., 1].clone().requires_grad_(True)
    T = got["sums"][..., 2]
    a, b_, c_ = (I.mean(0), S.mean(0), T.mean(0)) if batch else (I, S, T)
    d = (1 - (2 * a + R.SMOOTH) / (b_ + c_ + R.SMOOTH))[..., (0 if do_bg else 1):].mean()
    d.backward()
    close(got["coef"][..., 0], I.grad, "alpha")
    close(got["coef"][..., 1], S.grad, "beta")
    if not do_bg:
        assert not got["coef"][:, 0].any()


@pytest.mark.parametrize("dice_w,ce_w", R.LOSS_WEIGHTS)
def test_dice_ce_weights_and_upstream_scalar(dice_w, ce_w):
    """A weight of exactly 0 (the oracle's dice_and_ce replaces it by its default, so the two terms are combined here)."""
    nb, h, w_, k1 = 2, 4, 5, 4
    logits, labels = R.loss_inputs(nb, h * w_, k1, seed=1)
    got = R.dice_ce(logits, labels, True, False, False, False, dice_w=dice_w, ce_w=ce_w, gout=R.LOSS_GOUT)
    v = nchw(logits, h, w_).clone().requires_grad_(True)
    lab = labels.reshape(nb, h, w_)
    ref = ce_w * losses_ref.ce_loss(v, lab) + dice_w * losses_ref.dice_loss(v, lab, k1 - 1, R.SMOOTH, False, True, False, False)
    (R.LOSS_GOUT * ref).backward()
    close(got["out"][0], ref.detach(), "loss")
    close(got["dlogits"], npc(v.grad), "dlogits")


@pytest.mark.parametrize("softmax,do_bg,batch,squared", R.LOSS_FLAGS)
def test_dense_targets_match_cross_entropy_with_probabilities(softmax, do_bg, batch, squared):
    nb, h, w_, k1 = 2, 4, 5, 3
    logits, soft = R.loss_inputs(nb, h * w_, k1, softmax=softmax, dense=True)
    got = R.dice_ce(logits, soft, softmax, do_bg, batch, squared, dice_w=0.6, ce_w=0.9)
    v = nchw(logits, h, w_).clone().requires_grad_(True)
    t = nchw(soft, h, w_)
    ce = torch.nn.CrossEntropyLoss()(v, t)
    ref = 0.9 * ce + 0.6 * losses_ref.dice_loss(v, t, k1 - 1, R.SMOOTH, do_bg, softmax, batch, squared)
    ref.backward()
    close(got["out"][1], ce.detach(), "ce")
    close(got["out"][0], ref.detach(), "loss")
    close(got["dlogits"], npc(v.grad), "dlogits")
    assert (soft.sum(-1) - 1).abs().max().item() < 1e-6 and bool((soft > 0).all()), "a dense target is a distribution (rounded to fp32)"


def test_case_tables_are_unique_and_small():
    for cases in (R.head_fwd_cases(), R.head_bwd_cases(), R.fused_cases(), R.fed_cases(), R.LOSS_SHAPES):
        assert len(cases) == len(set(cases))
    sizes = R.case_bytes()
    assert max(sizes.values()) <= R.MAX_CASE_BYTES, max(sizes, key=sizes.get)
    dt, c0, k1, n, hw = R.CAPPED  # the one exception: the smallest shape on which the fast forward's paired loop runs twice
    lanes = 256 // (c0 // 4)
    assert n * hw > 3 * 16384 * lanes and (887 - 1) ** 2 <= 3 * 16384 * lanes and n * hw * c0 * 4 < 210e6
    # all 18 fast and 24 fused instantiations are in the tables
    assert len({k[:3] for k in R.head_fwd_cases() if k[5:] == ("cl", False) and k[4] == R.HW and k[1] in R.FAST_C0[k[0]] and k[2] in R.FAST_K1}) == 18
    assert len({k[:3] for k in R.fused_cases()}) == 24
    assert set(R.fed_cases()) >= {R.fed_key(c, dt, "instance", k1) for c in R.FED_CHANNELS for dt in R.DT for k1 in R.FAST_K1}


def test_inputs_are_seeded_and_exact_in_their_storage_types():
    for dt in R.DT:
        a, b = R.head_inputs(dt, 16, 3, 2, 33), R.head_inputs(dt, 16, 3, 2, 33)
        assert all(torch.equal(a[k], b[k]) for k in a)
        assert torch.equal(a["x"].to(R.DT[dt]).double(), a["x"])
        f = R.fused_inputs(dt, 32, 3, 2, 33)
        assert torch.equal(f["y"].to(R.DT[dt]).double(), f["y"])
        for k in ("w", "b", "dl"):
            assert torch.equal(a[k].float().double(), a[k]) and torch.equal(f[k].float().double(), f[k])
        assert torch.equal(f["scale"].float().double(), f["scale"]) and torch.equal(f["shift"].float().double(), f["shift"])
    assert not torch.equal(R.head_inputs("f32", 16, 3, 2, 33)["x"], R.head_inputs("f32", 16, 3, 2, 33, seed=1)["x"])
    logits, labels = R.loss_inputs(3, 36, 3)
    assert torch.equal(logits.float().double(), logits) and labels.dtype == torch.int64


@pytest.mark.parametrize("key", R.fed_cases(), ids=lambda k: "-".join(str(x) for x in k))
def test_near_zero_exclusion_stays_under_one_percent(key):
    """The dy comparison of the head-fed backward may skip only elements whose REFERENCE pre-activation is within rounding of the
    LeakyReLU kink, and at most 1 % of a case: checked here, from the reference alone, for every input of the GPU grid."""
    dt = key[1]
    i, r = R.fed_reference(key)
    frac = N.near_zero(r["v"], dt).double().mean().item()
    assert frac <= N.MAX_EXCLUDED, f"{frac:.4f} of the elements sit on the LeakyReLU kink"
    assert torch.equal(i["y"].to(R.DT[dt]).double(), i["y"]) and torch.equal(i["dl"].float().double(), i["dl"])
    assert set(i["m"].unique().tolist()) == {0.0, 1.0 / N.KEEP}


@pytest.mark.parametrize("k1", [2, 3, 4, 8])
def test_hand_built_loss_inputs_are_what_they_claim(k1):
    nb, hw = 3, 1964
    _, labels = R.loss_inputs(nb, hw, k1, special="absent")
    counts = F.one_hot(labels, k1).sum(1)
    assert counts[0, k1 - 1] == 0 and bool((counts[1:, k1 - 1] > 0).all()) and bool((counts[0, :k1 - 1] > 0).all())
    logits, labels = R.loss_inputs(nb, hw, k1, special="unpredicted")
    assert not bool((logits.argmax(-1) == 0).any()) and bool((labels == 0).any())
    assert torch.equal(logits.float().double(), logits)
    _, labels = R.loss_inputs(nb, hw, k1, special="one_class")
    assert bool((labels[nb - 1] == 1).all()) and labels[0].unique().numel() == k1
    _, clean = R.loss_inputs(nb, hw, k1)
    for which in R.BAD_LABELS:
        bad = R.bad_labels(clean, k1, which)
        diff = (bad != clean).nonzero().tolist()
        assert diff == [[nb - 1, 5]]
        v = int(bad[nb - 1, 5])
        assert v == (k1 if which == "k1" else which) and not 0 <= v < k1
    hi = R.bad_labels(clean, k1, 2 ** 32 + 1)[nb - 1, 5].item()
    assert hi >> 32 == 1 and 0 <= (hi & 0xFFFFFFFF) < k1, "the low word alone is a valid class: only the high word gives it away"
