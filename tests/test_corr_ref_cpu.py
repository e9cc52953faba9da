"""CPU suite for tests/corr_ref.py, the exact-integer references of test_gpu_corr_exact.py: the conditions under which an arg-max kernel
must return the float64 scores and indices bit for bit hold for every case of the GPU file, a correct pass meets the checks under either
tie rule, and each faulty pass — the slips that white-noise features and flip-count allowances let through — fails them."""
import pytest
import torch

import corr_ref as R

FAULT_SHAPE = (20, 30, 20, 30)


@pytest.fixture(scope="module")
def fault_case():
    c = R.case(*FAULT_SHAPE, "copy")
    return c, R.scores(c.lr, c.ref, c.inv_ref)


def test_preconditions_of_every_gpu_case():
    n = 0
    for label, c, fam in R.gpu_cases():
        try:
            R.check_preconditions(c, fam)
        except AssertionError as e:
            raise AssertionError(f"{label}: {e}") from None
        n += 1
    assert n == 3 * 14 + 2 + 8 + 1      # candidate shapes x families, the top-1 shape not among them, the 64-channel forms, the re-score map


@pytest.mark.parametrize("ch", [128, 64])
def test_preconditions_of_the_planted_tie_case(ch):
    """Every query has exactly two equal maxima, the first copy's position and its twin 13 rows below."""
    c = R.tie_case(c=ch)
    hl, wl = c.lr.shape[2:]
    wr = c.ref.shape[3]
    t = R.top3(R.scores(c.lr, c.ref, c.inv_ref))
    assert (t.v1 == t.v2).all() and (t.v2 > t.v3).all()
    assert torch.equal(t.i2 - t.i1, torch.full_like(t.i1, (hl + 1) * wr))
    assert (t.i1 // wr <= hl).all() and hl + 1 > 8                  # the twins lie in different 8-row reference blocks
    R.check_preconditions(c, "random")


def test_copy_share_measured():
    """The figures the share bounds rest on: at amplitude 8 with random exponents nearly every reference position of the copied area is
    some query's winner."""
    for shape, lo in (((20, 30, 20, 30), 0.98), ((37, 45, 37, 45), 0.97), ((29, 51, 37, 45), 0.77)):
        _, share = R.check_preconditions(R.case(*shape, "copy"), "copy")
        assert share >= lo, (shape, share)


def test_preconditions_reject_wrongly_built_cases():
    c = R.case(*FAULT_SHAPE, "random")
    with pytest.raises(AssertionError, match="integers"):
        R.check_preconditions(c._replace(lr=c.lr + 0.5), "random")
    with pytest.raises(AssertionError, match="not exact"):
        R.check_preconditions(c._replace(ref=c.ref * 257), "random")                # 257 k: no bf16 number
    with pytest.raises(AssertionError, match="powers of two"):
        R.check_preconditions(c._replace(inv_ref=c.inv_ref * 0.75), "random")
    with pytest.raises(AssertionError, match="powers of two"):
        R.check_preconditions(c._replace(inv_ref=c.inv_ref * 0), "random")
    with pytest.raises(AssertionError, match="max .D."):
        R.check_preconditions(c._replace(lr=c.lr * 32, ref=c.ref * 32), "random")
    with pytest.raises(AssertionError, match="win a query"):                        # independent maps: far fewer positions ever win
        R.check_preconditions(c, "copy")
    tiled = R.case(*FAULT_SHAPE, "copy")
    tiled = tiled._replace(ref=torch.cat((tiled.ref, tiled.ref), 2), inv_ref=torch.ones(2 * tiled.inv_ref.numel()))
    t = R.top3(R.scores(tiled.lr, tiled.ref, tiled.inv_ref))
    assert (t.v1 == t.v2).float().mean() > 0.5                                      # tiling plants ties: why `maps` does not tile


def test_top2_against_a_loop():
    lr, ref = R.maps(5, 3, 3, 3, 3, "random")
    S = R.scores(lr, ref, R.pow2(6, 9))
    S[4, 2] = S[1, 2] = S[:, 2].max() + 1                                           # an exact tie at the top, one for second place
    S[7, 5] = S[0, 5] = S[:, 5].min()
    v1, i1, v2, i2 = R.top2(S)
    for i in range(9):
        order = sorted(range(9), key=lambda j: (-S[j, i].item(), j))
        assert (i1[i].item(), i2[i].item()) == (order[0], order[1])
        assert (v1[i].item(), v2[i].item()) == (S[order[0], i].item(), S[order[1], i].item())
    assert (i1[2].item(), i2[2].item()) == (1, 4)
    v1, i1, v2, i2 = R.top2(S[3:4])
    assert torch.equal(i1, torch.zeros(9, dtype=torch.int64)) and (i2 == -1).all() and (v2 == float("-inf")).all()
    assert R.top3(S[:2]).v3.eq(float("-inf")).all()


def test_a_correct_pass_meets_the_checks(fault_case):
    c, S = fault_case
    s, a, s2, a2 = R.reference_pass(S)
    R.check_candidates(S, s, a, s2, a2)
    tagged = (R.f32_bits(s) | (63 - (a % 64))).view(torch.float32)                  # keys as the kernels return them
    R.check_candidates(S, tagged, a, s2, a2)
    R.check_top1(S, c.inv_lr, (S.gather(0, a.long()[None])[0] * c.inv_lr.double()).float(), a)
    one = S[5:6]
    R.check_candidates(one, *R.reference_pass(one))


def test_ties_may_go_either_way_in_a_candidate_pass_but_not_in_a_top1_kernel():
    c = R.tie_case()
    S = R.scores(c.lr, c.ref, c.inv_ref)
    s, a, s2, a2 = R.reference_pass(S)
    R.check_candidates(S, s, a, s2, a2)
    R.check_candidates(S, s2, a2, s, a)                                             # the higher position first: allowed
    top = (S.gather(0, a.long()[None])[0] * c.inv_lr.double()).float()
    R.check_top1(S, c.inv_lr, top, a)
    with pytest.raises(AssertionError, match="lowest"):
        R.check_top1(S, c.inv_lr, top, a2)


def both_fail(c, S, bad_scores):
    s, a, s2, a2 = R.reference_pass(bad_scores)
    with pytest.raises(AssertionError):
        R.check_candidates(S, s, a, s2, a2)
    with pytest.raises(AssertionError):
        R.check_top1(S, c.inv_lr, (bad_scores.gather(0, a.long()[None])[0] * c.inv_lr.double()).float(), a)


def test_fault_dropped_tap(fault_case):
    """One product (one channel of one tap) missing from every score."""
    c, S = fault_case
    pl = R.patches(c.lr).reshape(128, 9, -1).clone()
    pl[77, 5] = 0
    both_fail(c, S, (R.patches(c.ref).t() @ pl.reshape(128 * 9, -1)) * c.inv_ref.double()[:, None])


def test_fault_right_edge_halo(fault_case):
    """The reference map's right-edge halo taken from the next row's first pixel instead of zero: only the scores of the reference
    positions in the last column change — winners of some query on the "copy" family, never seen on independent maps."""
    c, S = fault_case
    bad = (R.patches(c.ref, wrap_right=True).t() @ R.patches(c.lr)) * c.inv_ref.double()[:, None]
    rows = (bad != S).any(1).nonzero().reshape(-1)
    assert rows.numel() and (rows % FAULT_SHAPE[3] == FAULT_SHAPE[3] - 1).all()
    both_fail(c, S, bad)
    # on independent maps the same fault changes hardly any query's winner (the reach "copy" adds)
    r = R.case(*FAULT_SHAPE, "random")
    Sr = R.scores(r.lr, r.ref, r.inv_ref)
    badr = (R.patches(r.ref, wrap_right=True).t() @ R.patches(r.lr)) * r.inv_ref.double()[:, None]
    changed = (R.top2(badr)[1] != R.top2(Sr)[1]).float().mean().item()
    assert changed < 0.05


def test_fault_neighbouring_normaliser(fault_case):
    """inv_ref[j + 1] used for j."""
    c, S = fault_case
    both_fail(c, S, R.dots(c.lr, c.ref) * torch.roll(c.inv_ref, -1).double()[:, None])
    flat = c._replace(inv_ref=torch.full_like(c.inv_ref, 0.25))                     # constant exponents cannot see it
    Sf = R.scores(flat.lr, flat.ref, flat.inv_ref)
    assert torch.equal(R.dots(c.lr, c.ref) * torch.roll(flat.inv_ref, -1).double()[:, None], Sf)


def test_fault_runner_up_missing(fault_case):
    _, S = fault_case
    s, a, s2, a2 = R.reference_pass(S)
    with pytest.raises(AssertionError, match="arg2 outside"):
        R.check_candidates(S, s, a, torch.full_like(s2, float("-inf")), torch.full_like(a2, -1))


def test_fault_runner_up_is_the_winner(fault_case):
    _, S = fault_case
    s, a, s2, a2 = R.reference_pass(S)
    with pytest.raises(AssertionError, match="winner again"):
        R.check_candidates(S, s, a, s.clone(), a.clone())


def test_fault_lost_split(fault_case):
    """The winner taken from the first half of the reference rows only (one split's partial result lost in the merge)."""
    c, S = fault_case
    half = S.clone()
    half[S.shape[0] // 2:] = float("-inf")
    both_fail(c, S, half)


def test_fault_low_score_bit(fault_case):
    """Scores with one low bit set: the lowest bit above the tag in a candidate key, the last bit in a top-1 score."""
    c, S = fault_case
    s, a, s2, a2 = R.reference_pass(S)
    with pytest.raises(AssertionError, match="S is not"):
        R.check_candidates(S, (R.f32_bits(s) | 64).view(torch.float32), a, s2, a2)
    with pytest.raises(AssertionError, match="S2 is not"):
        R.check_candidates(S, s, a, (R.f32_bits(s2) | 64).view(torch.float32), a2)
    top = (S.gather(0, a.long()[None])[0] * c.inv_lr.double()).float()
    with pytest.raises(AssertionError, match="S is not"):
        R.check_top1(S, c.inv_lr, (R.f32_bits(top) | 1).view(torch.float32), a)
