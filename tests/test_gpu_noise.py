"""Sensor noise of blur synthesis on the device: spei_window_mean_noise_u8 (csrc/blurset.hip) and spei_train_batch_runs_noise_u8
(csrc/train_batch.hip) bit for bit against the numpy restatement tests/noise_ref.py, against the light entries where they must agree,
blurset.synthesize across chunk sizes, whole epochs of data.SharpTrainLoader against TrainLoader on the sets blurset.write_dataset
writes with the same noise, and the checks that refuse a launch.  Equality throughout: the arithmetic is integer."""
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

import light_ref  # noqa: E402
import noise_ref  # noqa: E402
from sharpset_ref import moving_clip, write_sharp  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 20
SEED = (7 << 32) | 11                                       # both key words in use
STARTS, LENGTHS = np.array([0, 1, 3, 5, 19, 18, 6]), np.array([1, 2, 7, 15, 1, 2, 7])
FIRST_RUN, CLIP = 5, 3


def _records(runs, clip, A, B):
    from speinet_amd import light
    rec = np.zeros(len(runs), dtype=light.NOISE_RECORD)
    rec["run"], rec["clip"], rec["A"], rec["B"] = runs, clip, A, B
    return rec


def _clips(H, W):
    """random bytes; and a clip whose pixels are 0 or 255 in every frame (L = 0 or S: the clamp at both ends), a few frames flipped so
    that the runs also hold mid-range means."""
    rs = np.random.RandomState(H * 100 + W)
    ends = np.repeat((rs.randint(0, 2, (1, H, W, 3)) * 255).astype(np.uint8), T, axis=0)
    ends[::3] = 255 - ends[::3]
    ends[:, : H // 2] = ends[:1, : H // 2]
    return {"random": rs.randint(0, 256, (T, H, W, 3)).astype(np.uint8), "ends": ends}


def _on_device(frames, shift, frame_stride):
    """The clip as a uint8 [T,H,W,3] device tensor whose first byte lies `shift` bytes past an aligned address, frames frame_stride apart."""
    n, H, W, _ = frames.shape
    host = np.zeros(shift + n * frame_stride + 16, np.uint8)
    for t in range(n):
        host[shift + t * frame_stride:shift + t * frame_stride + H * W * 3] = frames[t].reshape(-1)
    buf = torch.from_numpy(host).to(DEV)
    view = torch.as_strided(buf, (n, H, W, 3), (frame_stride, W * 3, 3, 1), storage_offset=shift)
    assert view.data_ptr() % 16 == shift % 16
    return view


@pytest.mark.parametrize("spec", ["srgb", "gamma:2.2"])
def test_window_mean_against_the_numpy_restatement(spec):
    """16x16: the 16-byte path; 9x7: the pixel path; 16x16 one byte past an aligned address: the pixel path forced.  20 frames, runs of
    1, 2, 7 and 15 frames at the start, inside and at the very end of the clip, run ids from 5, moderate and the largest levels."""
    from speinet_amd import ops
    M = len(STARTS)
    runs = FIRST_RUN + np.arange(M)
    for (H, W, shift, extra), (a, r) in itertools.product(((16, 16, 0, 0), (9, 7, 0, 0), (16, 16, 1, 7)), ((5e-3, 1e-2), (0.05, 0.1))):
        A, B = noise_ref.levels(a, r)
        for name, frames in _clips(H, W).items():
            src = _on_device(frames, shift, H * W * 3 + extra)
            blur, gt, gray = ops.window_mean_u8(src, STARTS, LENGTHS, gray=True, light=spec, noise=(_records(runs, CLIP, A, B), SEED))
            torch.cuda.synchronize()
            want = np.stack([noise_ref.run_mean(frames[s:s + n], spec, run, CLIP, SEED, A, B) for s, n, run in zip(STARTS, LENGTHS, runs)])
            assert np.array_equal(blur.cpu().numpy(), want), (H, W, shift, a, name)
            assert np.array_equal(gt.cpu().numpy(), np.stack([frames[s + n // 2] for s, n in zip(STARTS, LENGTHS)])), (H, W, shift, name)
            _, _, gray_of_blur = ops.window_mean_u8(blur, np.arange(M), np.ones(M, np.int64), gray=True)
            assert torch.equal(gray, gray_of_blur), (H, W, shift, name)          # the gray plane of the noisy encoded bytes
            for m in np.flatnonzero(LENGTHS == 1):                              # a run of length 1 returns its bytes
                assert np.array_equal(want[m], frames[STARTS[m]])
            clean = np.stack([light_ref.run_mean(frames[s:s + n], spec) for s, n in zip(STARTS, LENGTHS)])
            assert not np.array_equal(want[LENGTHS > 1], clean[LENGTHS > 1])     # the noise is there
            assert not np.array_equal(want[2][H // 2:], want[6][H // 2:])        # other frames and another run id


def _resident(frames):
    dev = torch.from_numpy(np.ascontiguousarray(frames)).to(DEV)
    return dev, dev.data_ptr()


def _launch_runs(rec, n_in, n_gt, P, rgb_range=1.0, light=None, noise=None):
    from speinet_amd import ops
    host = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())
    inp = torch.full((n_in, 3, P, P), -7.0, device=DEV)
    gt = torch.full((max(n_gt, 1), 3, P, P), -7.0, device=DEV)[:n_gt]
    if noise is not None:
        nhost = torch.from_numpy(noise[0].view(np.uint8).reshape(-1).copy())
        noise = (nhost.to(DEV), nhost, noise[1])
    with torch.cuda.device(DEV):
        ops.Ctx(device=DEV).train_batch_runs(host.to(DEV), host, n_in, n_gt, inp, gt, P, rgb_range, light=light, noise=noise)
    torch.cuda.synchronize()
    return inp.cpu().numpy(), gt.cpu().numpy()


def _batch_case(H, W, P):
    """Two clips at different levels; per clip lengths 1, 2, 7, 15 x eight flag combinations, origins cycling over three, runs at the
    start or at the very end of the clip, some records zeroed; then one gt record (a run of length 1) per clip."""
    from speinet_amd.data import RUN_RECORD
    clips = [moving_clip(3, T, H, W), np.random.RandomState(H + W).randint(0, 256, (T, H, W, 3)).astype(np.uint8)]
    levels = [noise_ref.levels(5e-3, 1e-2), noise_ref.levels(2e-2, 0.0)]
    origins = [(0, 0), (H - P, W - P), (1, 3)]
    keep, rows, nrows, what = [], [], [], []
    frame = H * W * 3
    for c, frames in enumerate(clips):
        dev, base = _resident(frames)
        keep.append(dev)
        for i, (n, (h, v, r)) in enumerate(itertools.product((1, 2, 7, 15), itertools.product((False, True), repeat=3))):
            y0, x0 = origins[i % 3]
            start = 0 if i % 2 else T - n
            zero = i % 9 == 5
            flags = (1 if h else 0) | (2 if v else 0) | (4 if r else 0) | (8 if zero else 0)
            run = 40 + n + (i % 2)
            rows.append((base + start * frame, frame, W * 3, y0, x0, flags, H, W, n, T - start))
            nrows.append((run, 10 + c) + levels[c])
            what.append((c, start, n, run, y0, x0, h, v, r, zero))
    n_in = len(rows)
    for c, frames in enumerate(clips):
        rows.append((keep[c].data_ptr() + 9 * frame, frame, W * 3, 2, 4, 5, H, W, 1, T - 9))
        nrows.append((3, 10 + c) + levels[c])
        what.append((c, 9, 1, 3, 2, 4, True, False, True, False))
    rec = np.array(rows, dtype=RUN_RECORD)
    nrec = np.zeros(len(nrows), dtype=_records([0], 0, 0, 0).dtype)
    for k, (run, clip, A, B) in enumerate(nrows):
        nrec[k] = (run, clip, A, 0, B)
    return clips, levels, keep, rec, nrec, what, n_in


@pytest.mark.parametrize("P", [32, 36])
@pytest.mark.parametrize("H,W", [(40, 48), (41, 47)])
def test_batch_kernel_against_the_numpy_restatement(H, W, P):
    """40x48 (dword loads) and 41x47 (byte loads), P = 32 (one full tile) and 36 (partial tiles): every output frame is the crop, flip
    and rotation of the restatement's FULL noisy frame — the counter is the pixel in its frame, whatever the crop — in srgb and gamma:2.2."""
    clips, levels, keep, rec, nrec, what, n_in = _batch_case(H, W, P)
    assert any(w[9] for w in what) and len({w[6:9] for w in what}) == 8 and {w[2] for w in what} == {1, 2, 7, 15}
    for spec, rgb_range in (("srgb", 1.0), ("gamma:2.2", 255.0)):
        full = {}
        got = np.concatenate(_launch_runs(rec, n_in, len(what) - n_in, P, rgb_range, spec, (nrec, SEED)))
        for k, (c, start, n, run, y0, x0, h, v, r, zero) in enumerate(what):
            if zero:
                want = np.zeros((3, P, P), np.float32)
            else:
                if (c, start, n, run) not in full:
                    full[c, start, n, run] = noise_ref.run_mean(clips[c][start:start + n], spec, run, 10 + c, SEED, *levels[c])
                want = noise_ref.place(full[c, start, n, run], y0, x0, P, h, v, r, rgb_range)
            assert np.array_equal(got[k], want), (spec, k, what[k])
        for k in range(n_in, len(what)):                                         # the gt records equal their frames
            c, start = what[k][:2]
            assert np.array_equal(got[k], noise_ref.place(clips[c][start], 2, 4, P, True, False, True, rgb_range))
        clean = np.concatenate(_launch_runs(rec, n_in, len(what) - n_in, P, rgb_range, spec))
        longer = [k for k, w in enumerate(what) if w[2] > 1 and not w[9]]
        assert not np.array_equal(clean[longer], got[longer])


def test_zero_levels_are_the_light_entries():
    """A = B = 0: d = 0 for every byte, so both noise entries return the light entries' bytes (and gray planes)."""
    from speinet_amd import ops
    for spec in ("srgb", "gamma:2.2"):
        for H, W in ((16, 16), (9, 7)):
            frames = _clips(H, W)["random"]
            src = torch.from_numpy(frames).to(DEV)
            want = ops.window_mean_u8(src, STARTS, LENGTHS, gray=True, light=spec)
            got = ops.window_mean_u8(src, STARTS, LENGTHS, gray=True, light=spec, noise=(_records(np.arange(len(STARTS)), 1, 0, 0), SEED))
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (spec, H, W)
        for H, W, P in ((40, 48, 36), (41, 47, 32)):
            _clips_, _levels, keep, rec, nrec, what, n_in = _batch_case(H, W, P)
            nrec["A"], nrec["B"] = 0, 0
            got = _launch_runs(rec, n_in, len(what) - n_in, P, 1.0, spec, (nrec, SEED))
            want = _launch_runs(rec, n_in, len(what) - n_in, P, 1.0, spec)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (spec, H, W)


@pytest.mark.parametrize("k", [1000, 2 ** 20])
def test_isqrt_at_and_below_a_perfect_square(k):
    """A = 0, n = 2: V = B / 2 = k^2 and k^2 - 1, whose integer roots are k and k - 1, on both window-mean paths and in the batch kernel."""
    from speinet_amd import ops
    from speinet_amd.data import RUN_RECORD
    for B in (2 * k * k, 2 * k * k - 2):
        assert int(noise_ref.isqrt(np.array([B // 2]))[0]) == (k if B == 2 * k * k else k - 1)
        for H, W in ((16, 16), (9, 7)):
            frames = _clips(H, W)["random"]
            blur, _, _ = ops.window_mean_u8(torch.from_numpy(frames).to(DEV), [4], [2], light="srgb", noise=(_records([2], 1, 0, B), SEED))
            want = noise_ref.run_mean(frames[4:6], "srgb", 2, 1, SEED, 0, B)
            assert np.array_equal(blur.cpu().numpy()[0], want), (k, B, H, W)
        H, W, P = 40, 48, 32
        frames = _clips(H, W)["random"]
        dev, base = _resident(frames)
        rec = np.array([(base + 4 * H * W * 3, H * W * 3, W * 3, 5, 7, 0, H, W, 2, T - 4)], dtype=RUN_RECORD)
        got, _ = _launch_runs(rec, 1, 0, P, 255.0, "srgb", (_records([2], 1, 0, B), SEED))
        assert np.array_equal(got[0], noise_ref.place(noise_ref.run_mean(frames[4:6], "srgb", 2, 1, SEED, 0, B), 5, 7, P, 0, 0, 0, 255.0)), (k, B)
    # sigma = k or k - 1 moves d by at most |z| / 4096 < 4 of 2^24: a byte changes only where L' lies that close to a boundary between
    # two codes.  A 256 x 256 frame holds a few such bytes (three for k = 1000, four for k = 2^20), so a root that is off by one shows
    big = np.random.RandomState(1).randint(0, 256, (2, 256, 256, 3)).astype(np.uint8)
    src = torch.from_numpy(big).to(DEV)
    want = [noise_ref.run_mean(big, "srgb", 2, 1, SEED, 0, B) for B in (2 * k * k, 2 * k * k - 2)]
    assert 0 < int((want[0] != want[1]).sum()) < 10
    for B, w in zip((2 * k * k, 2 * k * k - 2), want):
        blur, _, _ = ops.window_mean_u8(src, [0], [2], light="srgb", noise=(_records([2], 1, 0, B), SEED))
        assert np.array_equal(blur.cpu().numpy()[0], w), (k, B)


def test_synthesize_does_not_depend_on_the_chunk():
    """blurset.synthesize with chunks of 15 frames (the smallest; asked for as 4) and of 64: identical bytes and gray planes, those of the
    restatement; the run id is global across chunks."""
    from speinet_amd import blurset, light
    H, W, n = 20, 24, 60
    frames = moving_clip(9, n, H, W)
    starts, lengths, _ = blurset.plan_runs(n, 0.5, rng=random.Random(1))
    assert len(list(blurset._chunks(starts, lengths, 15))) > 2 and len(list(blurset._chunks(starts, lengths, 64))) == 1
    spec, noise = "srgb", "5e-3..2e-2:1e-2"
    outs = [blurset.synthesize(frames, (starts, lengths), DEV, gray=True, chunk_frames=c, light=spec, noise=light.ClipNoise(noise, 21, 2))
            for c in (4, 64)]
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    A, B = light.noise_levels(noise, 21, 2)
    want = np.stack([noise_ref.run_mean(frames[s:s + k], spec, m, 2, 21, A, B) for m, (s, k) in enumerate(zip(starts, lengths))])
    assert np.array_equal(outs[0][0].cpu().numpy(), want)
    other = blurset.synthesize(frames, (starts, lengths), DEV, light=spec, noise=light.ClipNoise(noise, 21, 2, 1))[0]
    assert not torch.equal(other, outs[0][0])
    with pytest.raises(ValueError, match="--light / --blur_light"):
        blurset.synthesize(frames, (starts, lengths), DEV, noise=light.ClipNoise(noise, 21, 2))


def test_epochs_equal_the_written_sets(tmp_path):
    """Epochs 0 and 1 of SharpTrainLoader(noise) == TrainLoader over ClipSet on what blurset.write_dataset(seed + e, light, noise) writes
    from the same clips, tensor for tensor; the written set's sampler is put into the state the sharp loader's is in at that epoch.  The
    two epochs differ, and so do the noisy and the clean loader."""
    from speinet_amd import blurset, light
    from speinet_amd.data import ClipSet, ClipStore, SharpClipSet, SharpStore, SharpTrainLoader, TrainLoader
    src = write_sharp(str(tmp_path / "sharp"), {f"clip{c}": moving_clip(40 + c, 40, 40, 48) for c in range(2)})
    seed, sampler_seed, patch, batch = 4, 3, 32, 2
    spec, noise = "srgb", "2e-3..2e-2:5e-3"
    got = {}
    for nz in (noise, None):
        cs = SharpClipSet(src, ratios=(0.5,), seed=seed, patch=patch, light=spec, noise=nz)
        loader = SharpTrainLoader(cs, SharpStore(cs, device=DEV, log=None), batch, patch, seed=sampler_seed, rank=0, world=1)
        got[nz] = [[(i.clone(), g.clone()) for i, g in loader] for _ in range(2)]
        assert cs.epoch == 1 and (("noise " + light.noise_name(noise)) in cs.summary()) == (nz is not None)
    state = None
    for epoch in (0, 1):
        out = str(tmp_path / f"set{epoch}")
        lines = []
        done = blurset.write_dataset(src, out, ratios=(0.5,), seed=seed + epoch, device=DEV, light=spec, noise=noise, log=lines.append)
        for k, (d, ln) in enumerate(zip(done, lines)):
            assert (d["shot"], d["read"]) == light.noise_draw(noise, seed + epoch, k) and d["read"] == 5e-3
            assert ln.endswith(f"light srgb, noise shot {d['shot']:.3g} read 0.005)")
        ref_set = ClipSet(out, True, patch=patch)
        ref = TrainLoader(ref_set, ClipStore(ref_set, device=DEV, log=None), batch, patch, seed=sampler_seed, rank=0, world=1)
        if state is not None:
            ref.sampler.gen.set_state(state[0])
            ref.sampler.rng.setstate(state[1])
        want = [(i.clone(), g.clone()) for i, g in ref]
        state = (ref.sampler.gen.get_state(), ref.sampler.rng.getstate())
        assert len(want) == len(got[noise][epoch]) == len(got[None][epoch]) > 3
        for k, ((i, g), (wi, wg), (ci, cg)) in enumerate(zip(got[noise][epoch], want, got[None][epoch])):
            assert i.shape == wi.shape and i.shape[1:] == (5, 3, patch, patch) and torch.equal(i, wi) and torch.equal(g, wg), (epoch, k)
            assert torch.equal(g, cg), (epoch, k)                                # the ground truth carries no noise
        assert any(not torch.equal(i, ci) for (i, _), (ci, _) in zip(got[noise][epoch], got[None][epoch]))
    assert not torch.equal(got[noise][0][0][0], got[noise][1][0][0])


class _Spy:
    """The library handle with every entry point that is fetched from it written down."""

    def __init__(self, real):
        self.real, self.seen = real, []

    def __getattr__(self, name):
        self.seen.append(name)
        return getattr(self.real, name)


def test_none_reaches_only_the_existing_entry_points(monkeypatch):
    from speinet_amd import _lib, blurset, light, ops
    from speinet_amd.data import RUN_RECORD
    H, W, P = 40, 48, 32
    frames = _clips(H, W)["random"]
    sharp = torch.from_numpy(frames).to(DEV)
    rec = np.array([(sharp.data_ptr(), H * W * 3, W * 3, 3, 5, 0, H, W, 7, T)], dtype=RUN_RECORD)
    light.device_tables("srgb", DEV)
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", spy)
    for spec, entries in ((None, {"spei_window_mean_u8", "spei_train_batch_runs_u8"}),
                          ("code", {"spei_window_mean_u8", "spei_train_batch_runs_u8"}),
                          ("srgb", {"spei_window_mean_light_u8", "spei_train_batch_runs_light_u8"})):
        spy.seen.clear()
        ops.window_mean_u8(sharp, STARTS, LENGTHS, gray=True, light=spec, noise=None)
        blurset.synthesize(sharp, (STARTS, LENGTHS), DEV, light=spec, noise=None)
        _launch_runs(rec, 1, 0, P, 1.0, spec, None)
        assert set(spy.seen) == entries, (spec, spy.seen)
    spy.seen.clear()
    noise = (_records([0], 0, 5, 5), 1)
    ops.window_mean_u8(sharp, [0], [7], light="srgb", noise=noise)
    _launch_runs(rec, 1, 0, P, 1.0, "srgb", noise)
    assert set(spy.seen) == {"spei_window_mean_noise_u8", "spei_train_batch_runs_noise_u8"}
    for spec in (None, "code"):                                                  # noise needs a linear light
        with pytest.raises(ValueError, match="--light / --blur_light"):
            ops.window_mean_u8(sharp, [0], [7], light=spec, noise=noise)
        with pytest.raises(ValueError, match="--light / --blur_light"):
            _launch_runs(rec, 1, 0, P, 1.0, spec, noise)


def test_invalid_arguments_launch_nothing():
    """A bad gauss table, bad records or a missing pointer handed straight to either entry point: non-zero, the text names the entry
    point, nothing is written."""
    from speinet_amd import _lib, light
    from speinet_amd.data import RUN_RECORD
    lib = _lib.lib()
    H, W, n, P = 8, 16, 4, 8
    clip = torch.zeros((n, H, W, 3), dtype=torch.uint8, device=DEV) + 9
    tab_host = torch.from_numpy(np.concatenate(light.tables("srgb")).astype(np.int32))
    tab = tab_host.to(DEV)
    good_gauss = light.gauss_table()
    flat = good_gauss.copy()
    flat[700] = flat[699]
    tall = good_gauss.copy()
    tall[1024] = 2 ** 15
    cases = [("a gauss table that does not increase", flat, (0, 0, 0), "invalid gauss table at word 700"),
             ("a gauss word of 2^15", tall, (0, 0, 0), "invalid gauss table"),
             ("A = 2^20", good_gauss, (2 ** 20, 0, 0), "A = 1048576"),
             ("B = 2^42", good_gauss, (0, 2 ** 42, 0), "B = 4398046511104"),
             ("reserved = 1", good_gauss, (0, 0, 1), "reserved = 1"),
             ("null noise records", good_gauss, None, "null noise records"),
             ("null noise host copy", good_gauss, "host", "null noise records"),
             ("null gauss table", None, (0, 0, 0), "null gauss table"),
             ("valid", good_gauss, (2 ** 20 - 1, 2 ** 42 - 1, 0), None)]
    runs = torch.tensor([[0, 2]], dtype=torch.int32)
    rec = np.array([(clip.data_ptr(), H * W * 3, W * 3, 0, 0, 0, H, W, 2, n)], dtype=RUN_RECORD)
    rec_host = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())
    runs_dev, rec_dev = runs.to(DEV), rec_host.to(DEV)
    for what, gauss, level, text in cases:
        gs_host = torch.from_numpy((good_gauss if gauss is None else gauss).copy())
        gs = gs_host.to(DEV)
        nrec = _records([0], 0, 0, 0)
        if isinstance(level, tuple):
            nrec["A"], nrec["B"], nrec["reserved"] = level
        nz_host = torch.from_numpy(nrec.view(np.uint8).copy())
        nz = nz_host.to(DEV)
        g_ptrs = (0, 0) if gauss is None else (gs.data_ptr(), gs_host.data_ptr())
        n_ptrs = (0, nz_host.data_ptr()) if level is None else (nz.data_ptr(), 0) if level == "host" else (nz.data_ptr(), nz_host.data_ptr())
        blur = torch.full((1, H, W, 3), 77, dtype=torch.uint8, device=DEV)
        gt = torch.full((1, H, W, 3), 77, dtype=torch.uint8, device=DEV)
        inp = torch.full((1, 3, P, P), -7.0, device=DEV)
        with torch.cuda.device(DEV):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc_w = lib.spei_window_mean_noise_u8(C.c_void_p(clip.data_ptr()), H * W * 3, n, C.c_void_p(runs_dev.data_ptr()),
                                                 C.c_void_p(runs.data_ptr()), 1, C.c_void_p(tab.data_ptr()), C.c_void_p(tab_host.data_ptr()),
                                                 C.c_void_p(g_ptrs[0]), C.c_void_p(g_ptrs[1]), C.c_void_p(n_ptrs[0]), C.c_void_p(n_ptrs[1]), 3, 4,
                                                 C.c_void_p(blur.data_ptr()), C.c_void_p(gt.data_ptr()), C.c_void_p(0), H, W, st)
            msg_w = lib.spei_last_error().decode()
            rc_b = lib.spei_train_batch_runs_noise_u8(C.c_void_p(rec_dev.data_ptr()), C.c_void_p(rec_host.data_ptr()), 1, 0,
                                                      C.c_void_p(tab.data_ptr()), C.c_void_p(tab_host.data_ptr()), C.c_void_p(g_ptrs[0]),
                                                      C.c_void_p(g_ptrs[1]), C.c_void_p(n_ptrs[0]), C.c_void_p(n_ptrs[1]), 3, 4,
                                                      C.c_void_p(inp.data_ptr()), C.c_void_p(0), P, 1.0, st)
            msg_b = lib.spei_last_error().decode()
        torch.cuda.synchronize()
        if text is None:                                                         # identical frames of code 9 at the largest levels: written
            assert rc_w == 0 and rc_b == 0, (msg_w, msg_b)
            assert bool((gt == 9).all()) and bool((blur != 77).any()) and not bool((inp == -7.0).any())
            continue
        assert rc_w != 0 and msg_w.startswith("spei_window_mean_noise_u8: ") and text in msg_w, (what, rc_w, msg_w)
        assert rc_b != 0 and msg_b.startswith("spei_train_batch_runs_noise_u8: ") and text in msg_b, (what, rc_b, msg_b)
        assert bool((blur == 77).all()) and bool((gt == 77).all()) and bool((inp == -7.0).all()), what       # nothing was launched
    # every check of the light entries stays: an invalid light table is refused by the noise entries as well
    bad_tab_host = tab_host.clone()
    bad_tab_host[100] = bad_tab_host[99]
    gs_host = torch.from_numpy(good_gauss.copy())
    gs, nz_host = gs_host.to(DEV), torch.from_numpy(_records([0], 0, 0, 0).view(np.uint8).copy())
    nz = nz_host.to(DEV)
    inp = torch.full((1, 3, P, P), -7.0, device=DEV)
    with torch.cuda.device(DEV):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = lib.spei_train_batch_runs_noise_u8(C.c_void_p(rec_dev.data_ptr()), C.c_void_p(rec_host.data_ptr()), 1, 0, C.c_void_p(tab.data_ptr()),
                                                C.c_void_p(bad_tab_host.data_ptr()), C.c_void_p(gs.data_ptr()), C.c_void_p(gs_host.data_ptr()),
                                                C.c_void_p(nz.data_ptr()), C.c_void_p(nz_host.data_ptr()), 3, 4, C.c_void_p(inp.data_ptr()),
                                                C.c_void_p(0), P, 1.0, st)
        assert rc != 0 and "invalid light tables at code 100" in lib.spei_last_error().decode()
    torch.cuda.synchronize()
    assert bool((inp == -7.0).all())
