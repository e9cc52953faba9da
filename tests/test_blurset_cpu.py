"""Host suite: the run plan of speinet_amd.blurset against the reference's own generate_blurry_sequence (golden G25,
tests/golden/make_golden_blurset.py): labels, ground-truth frames and, through an integer mean, the bytes of the blurry frames."""
import os
import random

import numpy as np
import pytest

from speinet_amd import blurset


@pytest.fixture(scope="module")
def g25(golden_dir):
    return np.load(os.path.join(golden_dir, "g25_blurset.npz"))


def test_plan_runs_reproduces_reference(g25):
    frames = g25["frames"]
    for i, (ratio, seed) in enumerate(zip(g25["ratios"], g25["seeds"])):
        starts, lengths, labels = blurset.plan_runs(len(frames), float(ratio), 5, (1, 15), random.Random(int(seed)))
        assert np.array_equal(labels, g25[f"labels_{i}"])
        gt = np.stack([frames[s + n // 2] for s, n in zip(starts, lengths)])
        assert np.array_equal(gt, g25[f"gt_{i}"].transpose(0, 2, 3, 1))
        blur = np.stack([frames[s:s + n].astype(np.int64).sum(axis=0) // n for s, n in zip(starts, lengths)]).astype(np.uint8)
        assert np.array_equal(blur, g25[f"blurry_{i}"].transpose(0, 2, 3, 1).astype(np.uint8))      # mix_choice_dataset.py:104


@pytest.mark.parametrize("n,ratio,seed", [(1, 0.5, 0), (5, 0.0, 1), (6, 0.0, 2), (100, 0.3, 3), (1000, 1.0, 4), (333, 0.1, 5)])
def test_runs_tile_the_clip(n, ratio, seed):
    starts, lengths, labels = blurset.plan_runs(n, ratio, rng=random.Random(seed))
    assert starts[0] == 0 and np.array_equal(starts[1:], np.cumsum(lengths)[:-1]) and lengths.sum() == n
    assert lengths.min() >= 1 and lengths.max() <= 15 and np.isin(labels, (0, 1)).all()
    assert (lengths[labels == 1] <= 5).all()
    assert (lengths[:-1][labels[:-1] == 0] > 5).all()             # only the last run may be cut short by the clip's end


def test_plan_runs_leaves_global_random_state_alone():
    random.seed(99)
    before = random.getstate()
    blurset.plan_runs(200, 0.5, rng=random.Random(1))
    assert random.getstate() == before


@pytest.mark.parametrize("kw", [dict(ratio=1.5), dict(ratio=-0.1), dict(ratio=None), dict(ratio=0.5, threshold=15),
                                dict(ratio=0.5, threshold=0), dict(ratio=0.5, window_range=(1, 16)), dict(ratio=0.5, window_range=(0, 15)),
                                dict(ratio=0.5, n_frames=0), dict(ratio=0.5, rng=None)])
def test_invalid_arguments_raise(kw):
    args = dict(n_frames=60, rng=random.Random(0))
    args.update(kw)
    with pytest.raises(ValueError):
        blurset.plan_runs(**args)


def test_chunks_cover_every_run_within_the_budget():
    starts, lengths, _ = blurset.plan_runs(500, 0.3, rng=random.Random(8))
    seen = []
    for i, j, lo, hi in blurset._chunks(starts, lengths, 64):
        assert hi - lo <= 64 and lo == starts[i] and hi == starts[j - 1] + lengths[j - 1]
        seen += list(range(i, j))
    assert seen == list(range(len(starts)))
