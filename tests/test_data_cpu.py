"""speinet_amd.data / speinet_amd.fit on the host: the dataset scan and sample arithmetic against G24 (tests/golden/g24_loader.npz,
recorded from the reference's own training loader by tests/golden/make_golden_data.py), the draws, the error paths, the rank split and
the order of the learning-rate schedule.  `restate` below is the numpy restatement of the reference's crop + flips + rot90 + np2Tensor;
it is required here to reproduce the reference's recorded tensors exactly, and is then the yardstick of the kernel in test_gpu_data.py."""
import os
import random
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g24_loader.npz")
CLIPS = ("000", "001", "002")


def load_g24():
    return np.load(GOLDEN)


def rebuild_tree(root, g=None, label=True) -> str:
    """The G24 data set as a directory tree: blur/<clip>/<number>.png, gt/..., label/<clip>.npy."""
    from PIL import Image
    g = load_g24() if g is None else g
    for name in CLIPS:
        for kind in ("blur", "gt"):
            os.makedirs(os.path.join(root, kind, name), exist_ok=True)
            for t, num in enumerate(g[f"numbers/{name}"]):
                Image.fromarray(g[f"{kind}/{name}"][t]).save(os.path.join(root, kind, name, f"{int(num):08d}.png"))
        if label:
            os.makedirs(os.path.join(root, "label"), exist_ok=True)
            np.save(os.path.join(root, "label", name + ".npy"), g[f"labels/{name}"])
    return str(root)


def restate(img: np.ndarray, iy: int, ix: int, patch: int, hflip: bool, vflip: bool, rot90: bool, rgb_range: float = 1.0,
            zero: bool = False) -> np.ndarray:
    """uint8 [H,W,3] -> float32 [3,P,P]: get_patch's crop, data_augment's hflip / vflip / rot90 in that order, np2Tensor's values
    (float64 -> float32, then one float32 multiply by the float32 value of rgb_range / 255)."""
    c = img[iy:iy + patch, ix:ix + patch]
    if zero:
        c = np.zeros_like(c)
    if hflip:
        c = c[:, ::-1]
    if vflip:
        c = c[::-1]
    if rot90:
        c = np.rot90(c)
    t = np.ascontiguousarray(c.transpose(2, 0, 1)).astype(np.float64).astype(np.float32)
    return t * np.float32(rgb_range / 255)


def expected_sample(g, cs, idx, d, patch, rgb_range=1.0):
    """(input [F,3,P,P], gt [3,P,P]) of sample idx under draw d, by the restatement."""
    s = cs.sample(idx)
    name = cs.clips[s.clip]["name"]
    blur, gt = g[f"blur/{name}"], g[f"gt/{name}"]
    frames = list(s.frames) + ([s.pre, s.sub] if cs.references else [])
    inp = np.stack([restate(blur[f], d.iy, d.ix, patch, d.hflip, d.vflip, d.rot90, rgb_range, zero=(cs.references and k == 3 and s.zero_pre))
                    for k, f in enumerate(frames)])
    return inp, restate(gt[s.frames[cs.n_seq // 2]], d.iy, d.ix, patch, d.hflip, d.vflip, d.rot90, rgb_range)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return rebuild_tree(tmp_path_factory.mktemp("g24"))


def test_clipset_matches_the_reference_loader(tree):
    from speinet_amd.data import ClipSet
    g = load_g24()
    for tag, train in (("train", True), ("eval", False)):
        cs = ClipSet(tree, train, n_sequence=3, n_frames_per_video=int(g["n_frames_per_video"]))
        assert len(cs) == int(g[f"{tag}/len"]) and cs.num_frame == int(g[f"{tag}/num_frame"])
        names, zero = g[f"{tag}/names"], g[f"{tag}/zero_pre"]
        assert len(names) == len(cs)
        for idx in range(len(cs)):
            s = cs.sample(idx)
            assert s.names == list(names[idx]), (tag, idx, s.names, list(names[idx]))
            assert s.zero_pre == bool(zero[idx]), (tag, idx)
        with pytest.raises(IndexError):
            cs.sample(len(cs))
    assert zero.any() and not zero.all()
    # training reads clip 001 truncated to 13 frames, evaluation all 14; the labels are truncated with it
    assert ClipSet(tree, True, n_frames_per_video=13).clips[1]["T"] == 13 and ClipSet(tree, False, n_frames_per_video=13).clips[1]["T"] == 14
    # without references: the same windows, three names, no labels needed
    plain = ClipSet(tree, True, n_frames_per_video=13, references=False)
    ref = ClipSet(tree, True, n_frames_per_video=13)
    assert len(plain) == len(ref)
    for idx in (0, 5, len(plain) - 1):
        assert plain.sample(idx).names == ref.sample(idx).names[:3] and plain.sample(idx).pre is None


def test_draw_and_restatement_reproduce_the_recorded_tensors(tree):
    """The restatement reproduces every recorded tensor exactly under exactly one (offsets, flags), and `draw` under
    random.Random(seed) yields those offsets and flags in the recorded order."""
    from speinet_amd.data import ClipSet, Draw, draw
    g = load_g24()
    patch, seed = int(g["patch"]), int(g["seed"])
    cs = ClipSet(tree, True, n_frames_per_video=int(g["n_frames_per_video"]), patch=patch)
    seen, zeros = set(), set()
    for tag, augment in (("aug", True), ("plain", False)):
        rng = random.Random(seed)
        for k, idx in enumerate(g[f"{tag}_idx"]):
            idx = int(idx)
            c = cs.clips[cs.sample(idx).clip]
            hits = []
            for h in (False, True):
                for v in (False, True):
                    for r in (False, True):
                        for iy in range(c["H"] - patch + 1):
                            for ix in range(c["W"] - patch + 1):
                                d = Draw(ix, iy, h, v, r)
                                if np.array_equal(expected_sample(g, cs, idx, d, patch)[1], g[f"{tag}_gt"][k]):
                                    hits.append(d)
            assert len(hits) == 1, (tag, idx, hits)
            inp, gt = expected_sample(g, cs, idx, hits[0], patch)
            assert inp.dtype == np.float32 and np.array_equal(inp, g[f"{tag}_input"][k]) and np.array_equal(gt, g[f"{tag}_gt"][k])
            got = draw(rng, c["H"], c["W"], patch, augment)
            assert got == hits[0], (tag, idx, got, hits[0])
            if augment:
                seen.add(tuple(got[2:]))
                zeros.add(cs.sample(idx).zero_pre)
            else:
                assert tuple(got[2:]) == (False, False, False)
    assert len(seen) == 8 and zeros == {True, False}


def test_error_paths(tmp_path):
    from PIL import Image
    from speinet_amd.data import ClipSet, ClipStore
    g = load_g24()
    root = rebuild_tree(tmp_path / "nolabel", g, label=False)
    with pytest.raises(ValueError, match="speinet_amd.video"):
        ClipSet(root, True)
    assert len(ClipSet(root, True, references=False)) > 0
    root = rebuild_tree(tmp_path / "mixed", g)
    Image.fromarray(np.zeros((40, 64, 3), np.uint8)).save(os.path.join(root, "blur", "001", "00000003.png"))
    with pytest.raises(ValueError, match="mixed frame sizes"):
        ClipSet(root, True)
    root = rebuild_tree(tmp_path / "ok", g)
    with pytest.raises(ValueError, match="smaller than the 56x56 patch"):
        ClipSet(root, True, patch=56)
    np.save(os.path.join(root, "label", "002.npy"), g["labels/002"][:-1])
    with pytest.raises(ValueError, match="11 labels"):
        ClipSet(root, True)
    np.save(os.path.join(root, "label", "002.npy"), g["labels/002"])
    cs = ClipSet(root, True)
    assert cs.nbytes() == 2 * 3 * 48 * 64 * (9 + 14 + 12)
    with pytest.raises(MemoryError, match=r"(?s)%d bytes.*budget.*1 bytes.*residency='host'" % cs.nbytes()):
        ClipStore(cs, residency="device", budget_bytes=1)
    with pytest.raises(ValueError):
        ClipStore(cs, residency="managed")


def test_new_entries_declared_with_their_reference_lines():
    from speinet_amd import _lib
    from speinet_amd.build import sources
    from speinet_amd.data import RECORD
    for name in ("spei_train_batch_u8", "spei_psnr_f32"):
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES
    text = open(_lib.HEADER_PATH).read()
    assert "util/utils.py:8-65" in text and "data/videodata_nfs.py:180-207" in text
    assert "train_batch.hip" in sources()
    assert RECORD.itemsize == 32 and RECORD.names == ("src", "pitch", "y0", "x0", "flags", "H", "W")


def _split_worker(rank, world, port, root, ret):
    import torch.distributed as dist
    from speinet_amd.data import ClipSet, Sampler
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cs = ClipSet(root, True, n_frames_per_video=13)
        sm = Sampler(cs, batch=5, patch=40, seed=3)             # rank and world from the process group
        epochs = [[[(idx, tuple(d)) for idx, _s, d in b] for b in sm.epoch()] for _ in range(2)]
        ret[rank] = (sm.rank, sm.world, len(sm), epochs)
    finally:
        dist.destroy_process_group()


def test_rank_split_of_the_epoch_order(tree):
    from speinet_amd.data import ClipSet, Sampler
    world = 2
    port = 31500 + (os.getpid() % 2000)
    ret = mp.Manager().dict()
    mp.spawn(_split_worker, args=(world, port, tree, ret), nprocs=world, join=True)
    cs = ClipSet(tree, True, n_frames_per_video=13)
    whole = Sampler(cs, batch=5, patch=40, seed=3, rank=0, world=1)
    assert whole.n_batches() == 12 and len(cs) == 56             # 11 full batches and one of 1
    for e in range(2):
        full = [[(idx, tuple(d)) for idx, _s, d in b] for b in whole.epoch()]
        parts = [ret[r][3][e] for r in range(world)]
        assert [ret[r][:2] for r in range(world)] == [(0, 2), (1, 2)]
        assert abs(len(parts[0]) - len(parts[1])) <= 1 and [len(p) for p in parts] == [ret[r][2] for r in range(world)]
        assert parts[0] == full[0::2] and parts[1] == full[1::2]              # every world-th batch of the shared plan: same draws
        idx = [[i for b in p for i, _d in b] for p in parts]
        assert not set(idx[0]) & set(idx[1]) and sorted(idx[0] + idx[1]) == list(range(len(cs)))      # disjoint and covering


def test_schedule_steps_before_the_epoch_as_the_reference():
    """The learning rate each epoch trains at, against the reference's call order restated with plain torch: scheduler.step() first,
    then the epoch's optimizer steps (trainer_swint_hsa_nsf.py:18-24); epoch = scheduler.last_epoch."""
    import warnings
    from speinet_amd.fit import Schedule
    lr0, lr_decay, gamma = 1e-4, 5, 0.5

    def opt():
        return torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr0)
    ref_opt = opt()
    ref_sched = torch.optim.lr_scheduler.StepLR(ref_opt, step_size=lr_decay, gamma=gamma)
    ref = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(2 * lr_decay + 1):
            ref_sched.step()
            ref[ref_sched.last_epoch] = ref_opt.param_groups[0]["lr"]
            ref_opt.step()
    o = opt()
    sch = Schedule(o, lr_decay, gamma)
    got = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")                           # the order warning is silenced inside Schedule, nothing else is raised
        for _ in range(2 * lr_decay + 1):
            epoch, lr = sch.begin_epoch()
            got[epoch] = lr
            assert o.param_groups[0]["lr"] == lr
            o.step()
    for epoch in (1, lr_decay - 1, lr_decay, lr_decay + 1, 2 * lr_decay):
        assert got[epoch] == ref[epoch], (epoch, got[epoch], ref[epoch])
    assert got[1] == lr0 and got[lr_decay - 1] == lr0 and got[lr_decay] == lr0 * gamma and got[lr_decay + 1] == lr0 * gamma
    # resume: fast-forward by the number of finished epochs, the next epoch is the one after
    o2 = opt()
    s2 = Schedule(o2, lr_decay, gamma)
    s2.fast_forward(lr_decay - 1)
    assert s2.begin_epoch() == (lr_decay, lr0 * gamma)
