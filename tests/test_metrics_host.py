"""CPU checks of the float64 restatement in tests/_metrics_ref.py: against torch (argmax, softmax, the selectors'
score expressions) and oracle/losses_ref.hard_dice in float64, and the properties the shared case tables claim -- exact logit ties, exact
p1 == p2 pixels, a ragged multi-slab split, the 128-slab cap.  None of it needs a GPU."""
import numpy as np
import pytest
import torch

import _metrics_ref as M
from oracle import losses_ref

RTOL = 1e-12


@pytest.mark.parametrize("case", M.ARGMAX_CASES, ids=M.case_id)
def test_argmax_dice_matches_torch_and_oracle(case):
    hw_id, k1, nb = case
    z, lab = M.logits_case(hw_id, k1, nb)
    zz = z.reshape(nb, k1, -1)
    pred, counts, dice = M.argmax_dice(zz, lab.reshape(nb, -1))
    tp = torch.from_numpy(z).softmax(1).argmax(1) if np.isfinite(z).all() else torch.from_numpy(z).argmax(1)
    # softmax in fp32 may merge near-ties; the definition takes the argmax of the logits (softmax is monotone): compare to that
    assert np.array_equal(pred, torch.from_numpy(z).argmax(1).reshape(nb, -1).numpy())
    assert (pred.reshape(tp.shape) == tp.numpy()).mean() > 0.99
    for b in range(nb):
        for k in range(k1):
            p, g = torch.from_numpy(pred[b] == k), torch.from_numpy(lab[b].reshape(-1) == k)
            want = float(losses_ref.hard_dice(p, g)) if p.sum() > 0 else 0.0
            assert abs(dice[b, k] - want) < RTOL, (b, k)
            assert counts[b, k].tolist() == [int((p & g).sum()), int(p.sum()), int(g.sum())]
    assert counts.max() < 2 ** 24


def test_label_map_mode_and_hand_built():
    pred = np.array([[0, 0, 1, 1, 2, 2, 2, 0]])
    lab = np.array([[0, 1, 1, 1, 0, 0, 3, 3]])
    counts, dice = M.counts_dice(pred, lab, 4)
    assert counts[0].tolist() == [[1, 3, 3], [2, 2, 3], [0, 3, 0], [0, 0, 2]]
    np.testing.assert_allclose(dice[0], [2 / 6, 4 / 5, 0.0, 0.0], rtol=RTOL)  # class 2 absent from the labels, class 3 never predicted


@pytest.mark.parametrize("case", M.SCORE_CASES, ids=M.case_id)
@pytest.mark.parametrize("scale", [1.0, 80.0])
def test_selector_scores_match_torch(case, scale):
    hw_id, k1, nb = case
    z, _ = M.logits_case(hw_id, k1, nb, scale=scale)
    got = M.selector_scores(z.reshape(nb, k1, -1), 1e-8)
    p = torch.from_numpy(z).double().softmax(1)
    smooth = float(np.float32(1e-8))
    ent = (-p * torch.log2(p + smooth)).mean(dim=(1, 2, 3))  # entropy_selector.py:42-49
    conf = (-p.max(1)[0]).mean(dim=(1, 2))                    # confidence_selector.py:42-47
    top2 = p.topk(2, dim=1)[0]
    marg = (-(top2[:, 0] - top2[:, 1])).mean(dim=(1, 2))      # margin_selector.py:42-48
    np.testing.assert_allclose(got, torch.stack([ent, conf, marg], 1).numpy(), rtol=1e-11, atol=1e-14)
    assert np.isfinite(got).all()


def test_case_tables_hold_what_they_claim():
    assert len(set(map(M.case_id, M.ARGMAX_CASES))) == len(M.ARGMAX_CASES)
    assert {c[1] for c in M.ARGMAX_CASES} == {1, 2, 3, 8} and 8 == M.MAXK and min(c[1] for c in M.SCORE_CASES) == 2
    hw = {k: h * w for k, (h, w) in M.HW.items()}
    assert M.slabs_of(hw["2240"]) == 1 and M.slabs_of(hw["7"]) == 1 and hw["7"] < 256
    ln = M.slab_lengths(hw["65x67"])
    assert len(ln) == 2 and 0 < ln[-1] < ln[0] and sum(ln) == hw["65x67"]                    # >= 2 slabs, ragged last slab
    assert M.slabs_of(hw["512x513"]) == 128 and sum(M.slab_lengths(hw["512x513"])) == hw["512x513"]
    ln = M.slab_lengths(hw["515x517"])
    assert hw["515x517"] // 2048 > 128 and len(ln) == 128 and 0 < ln[-1] < ln[0] and sum(ln) == hw["515x517"]  # the cap, ragged
    for hw_id, k1, nb in M.SCORE_CASES:
        z, lab = M.logits_case(hw_id, k1, nb)
        zz = z.reshape(nb, k1, -1)
        p = zz.shape[2]
        assert (zz[:, :, 0] == zz[:, :1, 0]).all()                                            # all classes equal
        assert (zz[:, k1 - 2, p // 3] == zz[:, k1 - 1, p // 3]).all() and (zz[:, :, p // 3].max(1) == zz[:, k1 - 1, p // 3]).all()  # exact tie for the maximum
        assert (zz[:, 0, p - 1] == zz[:, k1 - 1, p - 1]).all() and (zz[:, :, p - 1].max(1) == zz[:, 0, p - 1]).all()
        pr = np.sort(np.exp(zz.astype(np.float64) - zz.max(1, keepdims=True)), axis=1)
        assert (pr[:, -1, p // 3] == pr[:, -2, p // 3]).all()                                 # an exact p1 == p2 pixel
        pred, counts, _ = M.argmax_dice(zz, lab.reshape(nb, -1))
        assert (pred[:, 0] == 0).all() and (pred[:, p // 3] == k1 - 2).all() and (pred[:, p - 1] == 0).all()  # the first maximum wins
        assert counts[0, 0, 2] == 0 and counts[0, k1 - 1, 1] == 0                             # absent class, never-predicted class
        if nb > 1:
            assert np.isneginf(zz[1, 0, p // 2])
        # a last-maximum-wins argmax would differ
        last = k1 - 1 - np.argmax(zz[:, ::-1], axis=1)
        assert (last != pred).any()
