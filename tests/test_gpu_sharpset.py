"""Training from sharp footage, on the device: spei_train_batch_runs_u8 (csrc/train_batch.hip) bit for bit against the numpy restatement
tests/sharpset_ref.py, against spei_train_batch_u8 at length 1 and against blurset.synthesize + spei_train_batch_u8; a whole epoch of
data.SharpTrainLoader against TrainLoader on the set blurset.write_dataset writes; speinet_amd.fit on sharp footage.  No tolerance is
involved: the run's mean is an integer quotient, uint8 -> float32 is exact and the one float32 multiply is the reference's."""
import ctypes as C
import itertools
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from sharpset_ref import moving_clip, run_patch, write_sharp      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS = (1, 2, 3, 7, 15)
T = 16


def _contents(H, W):
    """random bytes; all 255 (the largest sums); ramps of k mod 256, every frame with another step, so that the sums of a run take
    every residue modulo its length."""
    rs = np.random.RandomState(H * 100 + W)
    k = np.arange(H * W * 3, dtype=np.int64).reshape(H, W, 3)
    ramps = np.stack([(k * (t % 3 + 1) + 5 * t) % 256 for t in range(T)]).astype(np.uint8)
    return {"random": rs.randint(0, 256, (T, H, W, 3)).astype(np.uint8), "full": np.full((T, H, W, 3), 255, np.uint8), "ramps": ramps}


def _resident(frames, pitch, frame_stride, shift=0):
    """The clip on the device with the given row pitch and frame stride (bytes), its first byte `shift` bytes past an aligned address."""
    n, H, W, _ = frames.shape
    host = np.zeros(shift + n * frame_stride + 16, np.uint8)
    for t in range(n):
        rows = np.lib.stride_tricks.as_strided(host[shift + t * frame_stride:], (H, W * 3), (pitch, 1))
        rows[...] = frames[t].reshape(H, W * 3)
    dev = torch.from_numpy(host).to(DEV)
    return dev, dev.data_ptr() + shift


def _launch_runs(rec, n_in, n_gt, P, rgb_range=1.0):
    from speinet_amd import ops
    host = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())
    inp = torch.full((n_in, 3, P, P), -7.0, device=DEV)
    gt = torch.full((max(n_gt, 1), 3, P, P), -7.0, device=DEV)[:n_gt]
    with torch.cuda.device(DEV):
        ops.Ctx(device=DEV).train_batch_runs(host.to(DEV), host, n_in, n_gt, inp, gt, P, rgb_range)
    torch.cuda.synchronize()
    return inp.cpu().numpy(), gt.cpu().numpy()


@pytest.mark.parametrize("P", [32, 36])
@pytest.mark.parametrize("H,W", [(40, 48), (41, 47)])
def test_kernel_against_the_numpy_restatement(H, W, P):
    """Per frame size (40x48: rows on dwords, the dword path where x0 % 4 == 0; 41x47 with pitch 141: the byte path) and patch size
    (32: one full tile; 36: a full tile and 4-wide partial tiles on both axes): lengths 1, 2, 3, 7, 15 x all eight flag combinations x
    three crop origins x three clips x three layouts of the clip in memory (packed; a wider pitch and frame stride, multiples of 4; a
    frame stride that is no multiple of 4), runs at the start and at the very end of their clip, some records zeroed, the last eight
    records written to gt; rgb_range 1 and 255."""
    from speinet_amd.data import RUN_RECORD
    clips = _contents(H, W)
    for n in LENGTHS:                                          # the ramps do what they are there for
        sums = clips["ramps"][:n, :P, :P].astype(np.int64).sum(axis=0)
        assert set((sums % n).reshape(-1).tolist()) == set(range(n)), n
    frame = H * W * 3
    wide = (W * 3 + 3) // 4 * 4 + 4
    layouts = [(W * 3, frame), (wide, (H * wide + 11) // 4 * 4), (W * 3, frame + (5 if (frame + 5) % 4 else 6))]
    assert layouts[1][1] % 4 == 0 and layouts[1][1] > H * layouts[1][0] and layouts[2][1] % 4 != 0
    origins = [(0, 0), (H - P, W - P), (1, 3)]
    assert all(y + P <= H and x + P <= W for y, x in origins)
    keep, rows, want_of = [], [], []
    for (name, frames), (pitch, fstride) in itertools.product(clips.items(), layouts):
        dev, base = _resident(frames, pitch, fstride)
        keep.append(dev)
        for i, (n, (h, v, r), (y0, x0)) in enumerate(itertools.product(LENGTHS, itertools.product((False, True), repeat=3), origins)):
            start = 0 if i % 2 else T - n                      # every other run ends with its clip: avail == length
            zero = i % 17 == 5
            flags = (1 if h else 0) | (2 if v else 0) | (4 if r else 0) | (8 if zero else 0)
            rows.append((base + start * fstride, fstride, pitch, y0, x0, flags, H, W, n, T - start))
            want_of.append((name, start, n, y0, x0, h, v, r, zero))
    rec = np.array(rows, dtype=RUN_RECORD)
    n_gt = 8
    n_in = rec.size - n_gt
    assert rec.size == 3 * 3 * 5 * 8 * 3
    for rgb_range in (1.0, 255.0):
        inp, gt = _launch_runs(rec, n_in, n_gt, P, rgb_range)
        got = np.concatenate([inp, gt])
        for k, (name, start, n, y0, x0, h, v, r, zero) in enumerate(want_of):
            want = run_patch(clips[name], start, n, y0, x0, P, h, v, r, zero, rgb_range)
            assert np.array_equal(got[k], want), (rgb_range, k, name, start, n, (y0, x0), (h, v, r), zero, tuple(rec[k])[1:3])


def test_length_one_equals_train_batch_u8():
    """Runs of length 1 are spei_train_batch_u8's rectangles: the same tensors, on both access paths."""
    from speinet_amd import ops
    from speinet_amd.data import RECORD, RUN_RECORD
    P = 36
    for H, W in ((40, 48), (41, 47)):
        frames = np.random.RandomState(W).randint(0, 256, (4, H, W, 3)).astype(np.uint8)
        dev, base = _resident(frames, W * 3, H * W * 3)
        crops, runs = [], []
        for i, ((h, v, r), (y0, x0)) in enumerate(itertools.product(itertools.product((False, True), repeat=3), [(0, 0), (H - P, W - P), (1, 3)])):
            flags = (1 if h else 0) | (2 if v else 0) | (4 if r else 0) | (8 if i == 4 else 0)
            t = i % 4
            crops.append((base + t * H * W * 3, W * 3, y0, x0, flags, H, W))
            runs.append((base + t * H * W * 3, H * W * 3, W * 3, y0, x0, flags, H, W, 1, 4 - t))
        crops, runs = np.array(crops, dtype=RECORD), np.array(runs, dtype=RUN_RECORD)
        n_in, n_gt = len(crops) - 5, 5
        for rgb_range in (1.0, 255.0):
            got = np.concatenate(_launch_runs(runs, n_in, n_gt, P, rgb_range))
            host = torch.from_numpy(crops.view(np.uint8).reshape(-1).copy())
            inp, gt = torch.full((n_in, 3, P, P), -7.0, device=DEV), torch.full((n_gt, 3, P, P), -7.0, device=DEV)
            with torch.cuda.device(DEV):
                ops.Ctx(device=DEV).train_batch(host.to(DEV), host, n_in, n_gt, inp, gt, P, rgb_range)
            torch.cuda.synchronize()
            assert np.array_equal(got, torch.cat([inp, gt]).cpu().numpy()), (H, W, rgb_range)


def test_composition_with_synthesize():
    """train_batch_runs on the sharp clip == blurset.synthesize, then train_batch_u8 on the synthesized blur / gt frames: for every run of
    a plan, and for the gt records."""
    from speinet_amd import blurset, ops
    from speinet_amd.data import RECORD, RUN_RECORD
    H, W, P, n = 40, 48, 36, 40
    frames = moving_clip(7, n, H, W)
    starts, lengths, _ = blurset.plan_runs(n, 0.5, rng=random.Random(1))
    M = len(starts)
    assert M >= 4 and lengths.max() > 5 and lengths.min() <= 5
    sharp = torch.from_numpy(frames).to(DEV)
    blur, mid = blurset.synthesize(sharp, (starts, lengths), DEV)
    rng = random.Random(2)
    crops, runs = np.zeros(2 * M, dtype=RECORD), np.zeros(2 * M, dtype=RUN_RECORD)
    for m in range(M):
        y0, x0, flags = rng.randrange(H - P + 1), rng.randrange(W - P + 1), rng.randrange(8)
        s, ln = int(starts[m]), int(lengths[m])
        crops[m] = (blur.data_ptr() + m * H * W * 3, W * 3, y0, x0, flags, H, W)
        crops[M + m] = (mid.data_ptr() + m * H * W * 3, W * 3, y0, x0, flags, H, W)
        runs[m] = (sharp.data_ptr() + s * H * W * 3, H * W * 3, W * 3, y0, x0, flags, H, W, ln, n - s)
        runs[M + m] = (sharp.data_ptr() + (s + ln // 2) * H * W * 3, H * W * 3, W * 3, y0, x0, flags, H, W, 1, n - s - ln // 2)
    got_in, got_gt = _launch_runs(runs, M, M, P)
    host = torch.from_numpy(crops.view(np.uint8).reshape(-1).copy())
    inp, gt = torch.full((M, 3, P, P), -7.0, device=DEV), torch.full((M, 3, P, P), -7.0, device=DEV)
    with torch.cuda.device(DEV):
        ops.Ctx(device=DEV).train_batch(host.to(DEV), host, M, M, inp, gt, P, 1.0)
    torch.cuda.synchronize()
    assert np.array_equal(got_in, inp.cpu().numpy()) and np.array_equal(got_gt, gt.cpu().numpy())
    assert not np.array_equal(got_in, got_gt)


def test_whole_epochs_equal_the_written_sets(tmp_path):
    """Epochs 0 and 1 of SharpTrainLoader == TrainLoader over ClipSet on what blurset.write_dataset(seed = seed + epoch) writes from the
    same clips: the same (input, gt) tensors in the same order, with prefetch on and off.  The written set's sampler is put into the
    state the sharp loader's is in at that epoch (one generator pair serves all epochs, and the epochs differ in length)."""
    from speinet_amd import blurset
    from speinet_amd.data import ClipSet, ClipStore, SharpClipSet, SharpStore, SharpTrainLoader, TrainLoader
    src = write_sharp(str(tmp_path / "sharp"), {f"clip{c}": moving_clip(20 + c, 40, 48, 52) for c in range(3)})
    seed, sampler_seed, patch, batch = 5, 3, 32, 4
    got = {}
    for prefetch in (True, False):
        cs = SharpClipSet(src, ratios=(0.3, 0.5), seed=seed, patch=patch)
        store = SharpStore(cs, device=DEV, log=None)
        assert store.nbytes == cs.nbytes() == 3 * 40 * 48 * 52 * 3 and store.frames[2].shape == (40, 48, 52, 3) and store.frames[2].is_cuda
        loader = SharpTrainLoader(cs, store, batch, patch, seed=sampler_seed, prefetch=prefetch, rank=0, world=1)
        got[prefetch] = [[(i.clone(), g.clone()) for i, g in loader] for _ in range(2)]
        assert cs.epoch == 1
    state = None
    for epoch in (0, 1):
        out = str(tmp_path / f"set{epoch}")
        blurset.write_dataset(src, out, ratios=(0.3, 0.5), seed=seed + epoch, device=DEV)
        ref_set = ClipSet(out, True, patch=patch)
        ref = TrainLoader(ref_set, ClipStore(ref_set, device=DEV, log=None), batch, patch, seed=sampler_seed, rank=0, world=1)
        if state is not None:
            ref.sampler.gen.set_state(state[0])
            ref.sampler.rng.setstate(state[1])
        want = [(i.clone(), g.clone()) for i, g in ref]
        state = (ref.sampler.gen.get_state(), ref.sampler.rng.getstate())
        assert len(want) == -(-len(ref_set) // batch) > 3
        for prefetch in (True, False):
            assert len(got[prefetch][epoch]) == len(want), (epoch, prefetch)
            for k, ((i, g), (wi, wg)) in enumerate(zip(got[prefetch][epoch], want)):
                assert i.shape == wi.shape and i.shape[1:] == (5, 3, patch, patch) and torch.equal(i, wi) and torch.equal(g, wg), (epoch, prefetch, k)
    assert not torch.equal(got[True][0][0][0], got[True][1][0][0])
    with pytest.raises(MemoryError, match=r"python -m speinet_amd\.blurset.*--dir_data"):
        SharpStore(SharpClipSet(src, patch=patch), device=DEV, budget_bytes=1000, log=None)


def test_bad_arguments_launch_nothing():
    from speinet_amd import _lib
    from speinet_amd.data import RUN_RECORD
    lib = _lib.lib()
    P, H, W, n = 40, 48, 64, 4
    clip = torch.zeros((n, H, W, 3), dtype=torch.uint8, device=DEV) + 9
    inp = torch.full((1, 3, P, P), -7.0, device=DEV)
    gt = torch.full((1, 3, P, P), -7.0, device=DEV)

    def call(y0=0, x0=0, P=P, flags=0, length=2, avail=n, fstride=H * W * 3, pitch=W * 3, host=True, dev=True):
        rec = np.zeros(2, dtype=RUN_RECORD)
        rec[0] = (clip.data_ptr(), H * W * 3, W * 3, 0, 0, 0, H, W, 1, n)
        rec[1] = (clip.data_ptr(), fstride, pitch, y0, x0, flags, H, W, length, avail)
        h = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())
        d = h.to(DEV)
        with torch.cuda.device(DEV):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc = lib.spei_train_batch_runs_u8(C.c_void_p(d.data_ptr() if dev else 0), C.c_void_p(h.data_ptr() if host else 0), 1, 1,
                                              C.c_void_p(inp.data_ptr()), C.c_void_p(gt.data_ptr()), P, 1.0, st)
        torch.cuda.synchronize()
        return rc, lib.spei_last_error().decode()

    for kw, text in (({"host": False}, "null record table"), ({"dev": False}, "null record table"), ({"length": 0}, "record 1 has a run of length 0"),
                     ({"length": 16, "avail": 16}, "record 1 has a run of length 16"), ({"length": 3, "avail": 2}, "record 1: a run of 3 frames where 2 are left"),
                     ({"y0": 9}, "record 1: the 40x40 rectangle at (y 9, x 0) leaves its"), ({"x0": 25}, "leaves its"), ({"y0": -1}, "leaves its"),
                     ({"flags": 16}, "record 1 has unknown flag bits"), ({"fstride": H * W * 3 - 1}, "record 1: frame stride"),
                     ({"pitch": W * 3 - 1}, "record 1: frame 64x48 with a row pitch"), ({"P": 38}, "multiple of 4")):
        rc, msg = call(**kw)
        assert rc != 0 and text in msg and msg.startswith("spei_train_batch_runs_u8: "), (kw, rc, msg)
        assert bool((inp == -7.0).all()) and bool((gt == -7.0).all()), kw         # nothing was launched
    rc, msg = call(y0=8, x0=24, length=n, avail=n)                                # the maximal rectangle and the whole clip are fine
    assert rc == 0, msg
    rc, msg = call(length=1, avail=1, fstride=0)                                  # a single frame needs no stride
    assert rc == 0, msg
    assert bool((inp == np.float32(9) * np.float32(1 / 255)).all()) and bool((gt == inp[0]).all())


def test_fit_from_sharp_footage(tmp_path):
    from speinet_amd.data import SharpClipSet, SharpStore, SharpTrainLoader
    from speinet_amd.fit import Fit, build_model
    from speinet_amd.loss import Loss
    src = write_sharp(str(tmp_path / "sharp"), {f"clip{c}": moving_clip(30 + c, 30, 40, 40) for c in range(2)})
    save = str(tmp_path / "exp")

    def make(resume, epochs):
        net = build_model("swint", DEV, train_precision="f32", synthetic_seed=1 if resume else 0)
        cs = SharpClipSet(src, ratios=(0.5,), seed=2, references=False, patch=40)
        loader = SharpTrainLoader(cs, SharpStore(cs, device=DEV, log=None), batch=2, patch=40, seed=1)
        lines = []
        return Fit(net, Loss("1*L1+2*HEM", device=DEV), loader, None, save=save, lr=1e-4, lr_decay=3, epochs=epochs, print_every=1000,
                   resume=resume, seed=1, log=lines.append), cs, lines

    fit, cs, lines = make(False, 2)
    log = fit.run()
    print("\n".join(lines))
    plans = [ln for ln in lines if ln.startswith("Plan ")]
    assert len(plans) == 2 and plans[0].startswith("Plan 0 of ") and plans[1].startswith("Plan 1 of ") and "labelled sharp" in plans[0]
    assert plans[0].split(":", 1)[1] != plans[1].split(":", 1)[1] and cs.epoch == 1       # the two epochs trained on different runs
    assert log == [0.0, 0.0] and len(fit.loss_log) == 2 and all(np.isfinite(fit.loss_log))
    for name in ("model/model_latest.pt", "model/model_best.pt", "optimizer.pt", "psnr_log.pt"):
        assert os.path.isfile(os.path.join(save, name)), name
    fit2, cs2, lines2 = make(True, 3)
    assert cs2.epoch == 1                                                                 # fast-forwarded over plans 0 and 1
    fit2.run()
    print("\n".join(lines2))
    plans2 = [ln for ln in lines2 if ln.startswith("Plan ")]
    assert len(plans2) == 1 and plans2[0].startswith("Plan 2 of ") and cs2.epoch == 2 and np.isfinite(fit2.loss_log[-1])
