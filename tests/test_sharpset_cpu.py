"""Host suite of training from sharp footage (speinet_amd.data.SharpClipSet, run_records, SharpSampler; blurset.plan_dataset; the
--dir_sharp option of speinet_amd.fit): the plans are blurset.write_dataset's draws, the samples are ClipSet's on the set
write_dataset(seed + epoch) would write (written here with numpy), the record table points at the runs' frames."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from sharpset_ref import moving_clip, replay, write_set_numpy, write_sharp      # noqa: E402

from speinet_amd import blurset, data      # noqa: E402

LENGTHS = {"a": 37, "b": 40, "c": 64}
RATIOS, SEED = (0.3, 0.5), 4


@pytest.fixture(scope="module")
def clips():
    return {name: moving_clip(10 + i, T, 20, 20) for i, (name, T) in enumerate(LENGTHS.items())}


@pytest.fixture(scope="module")
def sharp_dir(clips, tmp_path_factory):
    return write_sharp(str(tmp_path_factory.mktemp("sharp")), clips)


@pytest.fixture(scope="module")
def long_dir(tmp_path_factory):
    """A clip long enough, at ratio 0.1, for sharp runs more than 7 runs apart: zeroed pre references."""
    return write_sharp(str(tmp_path_factory.mktemp("long")), {"a": moving_clip(4, 37, 20, 20), "long": moving_clip(3, 300, 20, 20)})


@pytest.mark.parametrize("ratios", [[0.5], [0.1, 0.3, 0.5], [0.0, 1.0]])
@pytest.mark.parametrize("seed", [0, 1, 11])
def test_plan_dataset_is_write_datasets_draw_sequence(ratios, seed):
    lengths = [37, 40, 64, 500]
    got = blurset.plan_dataset(lengths, ratios, seed, 5, (1, 15))
    want = replay(lengths, ratios, seed)
    assert len(got) == len(want) == 4
    for (ratio, (starts, lens, labels)), (w_ratio, w_starts, w_lens, w_labels) in zip(got, want):
        assert ratio == w_ratio
        assert np.array_equal(starts, w_starts) and np.array_equal(lens, w_lens) and np.array_equal(labels, w_labels)
    # another threshold and window range reach plan_runs
    got = blurset.plan_dataset(lengths, ratios, seed, 3, (2, 9))
    want = replay(lengths, ratios, seed, 3, (2, 9))
    assert all(np.array_equal(g[1][1], w[2]) and g[1][1].max() <= 9 for g, w in zip(got, want))
    with pytest.raises(ValueError):
        blurset.plan_dataset(lengths, [], seed)
    with pytest.raises(ValueError):
        blurset.plan_dataset(lengths, [0.5, 1.5], seed)


@pytest.mark.parametrize("references,n_frames_per_video", [(True, 200), (True, 5), (False, 200), (False, 5)])
def test_samples_equal_clipset_on_the_written_set(clips, sharp_dir, tmp_path, references, n_frames_per_video):
    cs = data.SharpClipSet(sharp_dir, ratios=RATIOS, seed=SEED, n_frames_per_video=n_frames_per_video, references=references, patch=20)
    assert cs.n_seq == 3 and cs.references == references and cs.nbytes() == sum(LENGTHS.values()) * 20 * 20 * 3
    for epoch in (0, 1, 0):
        out = str(tmp_path / f"set{epoch}")
        if not os.path.isdir(out):
            write_set_numpy(out, clips, RATIOS, SEED + epoch)
        ref = data.ClipSet(out, True, n_frames_per_video=n_frames_per_video, references=references, patch=20)
        cs.plan(epoch)
        if n_frames_per_video == 5:
            assert all(c["T"] <= 5 for c in cs.clips) and any(len(os.listdir(os.path.join(out, "blur", n))) > 5 for n in LENGTHS)
        assert len(cs) == len(ref) > 0 and len(cs.clips) == len(ref.clips) == 3
        for a, b in zip(cs.clips, ref.clips):
            for key in ("name", "T", "H", "W", "names", "pre", "sub") + (("labels",) if references else ()):
                assert a[key] == b[key], (epoch, key)
        for idx in range(len(cs)):
            got, want = cs.sample(idx), ref.sample(idx)
            for field in data.Sample._fields:
                assert getattr(got, field) == getattr(want, field), (epoch, idx, field)
        with pytest.raises(IndexError):
            cs.sample(len(cs))


def _stand_in(cs, pad=0):
    """A store of CPU tensors; `pad` bytes between frames."""
    frames = []
    for c in cs.sharp:
        flat = torch.zeros(c["T"], c["H"] * c["W"] * 3 + pad, dtype=torch.uint8)
        frames.append(flat[:, :c["H"] * c["W"] * 3].view(c["T"], c["H"], c["W"], 3))
    return SimpleNamespace(frames=frames, clipset=cs)


@pytest.mark.parametrize("references", [True, False])
def test_run_records(long_dir, references):
    cs = data.SharpClipSet(long_dir, ratios=(0.1,), seed=1, references=references, patch=12)
    store = _stand_in(cs, pad=8)
    sampler = data.SharpSampler(cs, batch=len(cs), patch=12, seed=2, rank=0, world=1)
    (items,) = sampler.epoch()
    rec = data.run_records(cs, store, items)
    F, B = (5 if references else 3), len(items)
    assert rec.dtype == data.RUN_RECORD and rec.dtype.itemsize == 48 and rec.shape == (B * F + B,)
    zeroed = 0
    for b, (idx, s, d) in enumerate(items):
        c = cs.clips[s.clip]
        sharp = store.frames[c["source"]]
        T = sharp.shape[0]
        assert sharp.stride(0) == 20 * 20 * 3 + 8
        flags = (1 if d.hflip else 0) | (2 if d.vflip else 0) | (4 if d.rot90 else 0)
        runs = list(s.frames) + ([s.pre, s.sub] if references else [])
        for k, m in enumerate(runs):
            r = rec[b * F + k]
            start, length = int(c["starts"][m]), int(c["lengths"][m])
            assert r["src"] == sharp.data_ptr() + start * sharp.stride(0) and r["frame_stride"] == sharp.stride(0)
            assert (r["length"], r["avail"]) == (length, T - start) and 1 <= length <= r["avail"]
            zero = references and k == 3 and s.zero_pre
            zeroed += zero
            assert (r["pitch"], r["y0"], r["x0"], r["H"], r["W"], r["flags"]) == (60, d.iy, d.ix, 20, 20, flags | (8 if zero else 0))
        g = rec[B * F + b]
        m = s.frames[1]
        mid = int(c["starts"][m]) + int(c["lengths"][m]) // 2
        assert g["src"] == sharp.data_ptr() + mid * sharp.stride(0) and (g["length"], g["avail"]) == (1, T - mid)
        assert (g["pitch"], g["y0"], g["x0"], g["H"], g["W"], g["flags"], g["frame_stride"]) == (60, d.iy, d.ix, 20, 20, flags, sharp.stride(0))
    assert (zeroed > 0) == references           # the zero flag is exercised, on pre only


def _plan_of(cs):
    return [(c["starts"].tolist(), c["lengths"].tolist(), c["labels"]) for c in cs.clips]


def test_sampler_replans_every_epoch(sharp_dir):
    def make(**kw):
        cs = data.SharpClipSet(sharp_dir, ratios=RATIOS, seed=SEED, patch=12)
        args = dict(batch=4, patch=12, seed=3, rank=0, world=1)
        args.update(kw)
        return cs, data.SharpSampler(cs, **args)

    probe = data.SharpClipSet(sharp_dir, ratios=RATIOS, seed=SEED, patch=12)
    plans = []
    for e in range(4):
        probe.plan(e)
        plans.append(_plan_of(probe))
    assert plans[0] != plans[1] and plans[1] != plans[2] and plans[2] != plans[3]

    (cs1, s1), (cs2, s2) = make(), make()
    for e in range(3):
        b1, b2 = s1.epoch(), s2.epoch()
        assert _plan_of(cs1) == plans[e] == _plan_of(cs2) and cs1.epoch == e
        assert b1 == b2 and sum(len(b) for b in b1) == len(cs1) and len(b1) == len(s1) == s1.n_batches()
    # after k calls the next epoch is plan k: what Fit's resume loop relies on
    cs3, s3 = make()
    for _ in range(2):
        s3.epoch()
    third = s3.epoch()
    assert _plan_of(cs3) == plans[2] and third == b1

    # two ranks: the same number of batches each, in every epoch, though the epochs differ in length
    pairs = [make(rank=r, world=2) for r in (0, 1)]
    for e in range(3):
        got = [s.epoch() for _cs, s in pairs]
        full = -(-len(pairs[0][0]) // 4)
        assert len(got[0]) == len(got[1]) == len(pairs[0][1]) == len(pairs[1][1]) == full // 2
        assert all(s.n_batches() == full - full % 2 and s.n_batches() % 2 == 0 for _cs, s in pairs)
        # rank 0 and rank 1 interleave the one shared order
        whole = make()[1]
        for _ in range(e):
            whole.epoch()
        shared = whole.epoch()
        assert got[0] == shared[:full - full % 2][0::2] and got[1] == shared[:full - full % 2][1::2]

    cs4, s4 = make(replan=False)
    for e in range(3):
        s4.epoch()
        assert _plan_of(cs4) == plans[0] and cs4.epoch == 0


def test_errors(sharp_dir, clips, tmp_path):
    from speinet_amd import fit
    with pytest.raises(ValueError, match="smaller than the 24x24 patch"):
        data.SharpClipSet(sharp_dir, patch=24)
    # 7 frames at ratio 0: the first run takes 6 or 7 of them, so at most two runs, fewer than a window of 3; the error names clip and epoch
    short = write_sharp(str(tmp_path / "short"), {"tiny": clips["a"][:7]})
    with pytest.raises(ValueError, match=r"clip tiny: the plan of epoch 0 .* fewer than one window of 3"):
        data.SharpClipSet(short, ratios=(0.0,), patch=20)
    with pytest.raises(ValueError, match="no clip folder"):
        data.SharpClipSet(str(tmp_path))
    from PIL import Image
    mixed = write_sharp(str(tmp_path / "mixed"), {"m": clips["a"][:20]})
    Image.fromarray(np.zeros((24, 20, 3), np.uint8)).save(os.path.join(mixed, "m", "00007.png"))
    with pytest.raises(ValueError, match="clip m:"):
        data.SharpClipSet(mixed)
    with pytest.raises(ValueError):
        data.SharpClipSet(sharp_dir, ratios=(1.5,))
    base = ["--dir_data_test", "v", "--save", "s"]
    for argv in (base, base + ["--dir_data", "a", "--dir_sharp", "b"]):
        with pytest.raises(SystemExit) as e:
            fit.main(argv)
        assert e.value.code == 2
