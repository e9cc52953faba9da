"""The definition of the geometric self-ensemble without a GPU: speinet_amd/ensemble.py against the numpy restatement in
tests/ensemble_ref.py and against the bookkeeping of the reference's forward_x8 (util/network_utils.py:308-341), restated here as
data; and the argument check of `deblur_clip(..., ensemble=)`, which sits in front of everything else."""
import numpy as np
import pytest
import torch

import ensemble_ref as R
from speinet_amd import ensemble as E
from speinet_amd import video

ARRAYS = [np.arange(15, dtype=np.float32).reshape(3, 5), np.arange(16, dtype=np.float32).reshape(4, 4),
          np.arange(2 * 3 * 5, dtype=np.float32).reshape(2, 3, 5)]


@pytest.mark.parametrize("a", ARRAYS, ids=["3x5", "4x4", "2x3x5"])
def test_apply_and_invert_are_the_restatement(a):
    for g in range(8):
        want = R.t_op(a, g)
        assert want.shape == a.shape[:-2] + R.shape_of(*a.shape[-2:], g)
        assert np.array_equal(E.apply(a, g), want)
        assert np.array_equal(E.apply(torch.from_numpy(a), g).numpy(), want)
        assert np.array_equal(E.invert(want, g), a) and np.array_equal(R.t_inv(want, g), a)
        assert np.array_equal(E.invert(torch.from_numpy(want), g).numpy(), a)
        assert np.array_equal(E.invert(E.apply(a, g), g), a)
        assert E.inverse_member(g) == R.inverse_member(g)
        assert np.array_equal(E.apply(E.apply(a, g), E.inverse_member(g)), a)


def test_members_are_pairwise_different():
    for a in ARRAYS[:2]:                                   # asymmetric under all of D4: a square one included
        seen = [E.apply(a, g) for g in range(8)]
        for g in range(8):
            for h in range(g):
                assert seen[g].shape != seen[h].shape or not np.array_equal(seen[g], seen[h]), (g, h)


def test_shape_of_and_members():
    for g in range(8):
        assert E.shape_of(3, 5, g) == ((5, 3) if g >= 4 else (3, 5)) == R.shape_of(3, 5, g)
    assert sorted(E.MEMBERS) == [1, 2, 4, 8] == list(E.SIZES)
    for k in (1, 2, 4, 8):
        assert tuple(E.MEMBERS[k]) == tuple(range(k))
    assert [E.inverse_member(g) for g in range(8)] == [0, 1, 2, 3, 4, 6, 5, 7]
    for bad in (-1, 8, True, 1.0, "1", None):
        with pytest.raises(ValueError):
            E.apply(ARRAYS[0], bad)
        with pytest.raises(ValueError):
            E.shape_of(3, 5, bad)


# forward_x8's bookkeeping as data.  Its input list doubles three times, by 'v' (columns reversed), 'h' (rows reversed) and 't'
# (transposed), so entry i has had these applied, left to right; its outputs are undone by 't' if i > 3, then 'h' if i % 4 > 1, then 'v'
# if i % 4 is odd.
X8_FORWARD = ["", "v", "h", "vh", "t", "vt", "ht", "vht"]
X8_INVERSE = ["", "v", "h", "hv", "t", "tv", "th", "thv"]
LETTER = {"v": lambda a: a[..., :, ::-1], "h": lambda a: a[..., ::-1, :], "t": lambda a: np.swapaxes(a, -1, -2)}


def _letters(a, word):
    for c in word:
        a = LETTER[c](a)
    return a


def test_enumeration_is_forward_x8s():
    a = np.arange(2 * 3 * 4 * 7, dtype=np.float32).reshape(2, 3, 4, 7)
    for i in range(8):
        fwd = _letters(a, X8_FORWARD[i])
        assert np.array_equal(R.t_op(a, i), fwd) and np.array_equal(E.apply(a, i), fwd)
        assert np.array_equal(_letters(fwd, X8_INVERSE[i]), a)
        assert np.array_equal(R.t_inv(fwd, i), _letters(fwd, X8_INVERSE[i]))
    # with the identity as the model, forward_x8's mean over its list is the input: so is the restatement's
    for k in (1, 2, 4, 8):
        assert np.array_equal(R.mean([R.t_op(a, g) for g in range(k)], list(range(k))), a)


def test_mean_is_sequential():
    """1e8 + 1 - 1e8 is 0 in float32 in that order and 1 in another: the restatement keeps the order it is given."""
    one = lambda v: np.full((1, 2, 2), v, np.float32)
    assert (R.mean([one(1e8), one(1.0), one(-1e8), one(0.0)], [0, 0, 0, 0]) == 0.0).all()
    assert (R.mean([one(1e8), one(-1e8), one(1.0), one(0.0)], [0, 0, 0, 0]) == 0.25).all()
    neg = R.mean([one(-0.0), one(-0.0)], [0, 3])
    assert (neg == 0).all() and np.signbit(neg).all()


@pytest.mark.parametrize("bad", [0, 3, 16, True, 8.0])
def test_deblur_clip_refuses_a_bad_ensemble(bad):
    with pytest.raises(ValueError, match="ensemble must be 1, 2, 4 or 8"):
        video.deblur_clip(None, None, ensemble=bad)          # refused before the model or a frame is looked at
