"""Averaging in linear light on the device: spei_window_mean_light_u8 (csrc/blurset.hip) and spei_train_batch_runs_light_u8
(csrc/train_batch.hip) bit for bit against the numpy restatement tests/light_ref.py, against each other, against the unchanged
code-value calls where they must agree, and a whole epoch of data.SharpTrainLoader against TrainLoader on the set
blurset.write_dataset writes in the same light.  No tolerance anywhere: the arithmetic is integer, uint8 -> float32 is exact."""
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
from sharpset_ref import moving_clip, write_sharp  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS = (1, 2, 3, 7, 15)
LIGHTS = ("srgb", "gamma:2.2", "gamma:1.0", "gamma:2.6")
T = 16
S = 2 ** 24 - 1


def _clips(H, W):
    """random; all 255 (the largest sums); all 0; frames alternating 0 / 255; frame t = (k + 17 t) mod 256, so that every code is
    decoded; k mod 256 in every frame, so that runs of 2..15 identical frames take every code through decode, quotient and encode."""
    rs = np.random.RandomState(H * 100 + W)
    k = np.arange(H * W * 3, dtype=np.int64).reshape(H, W, 3)
    alt = np.zeros((T, H, W, 3), np.uint8)
    alt[1::2] = 255
    return {"random": rs.randint(0, 256, (T, H, W, 3)).astype(np.uint8), "full": np.full((T, H, W, 3), 255, np.uint8),
            "zero": np.zeros((T, H, W, 3), np.uint8), "alternating": alt,
            "ramps": np.stack([(k + 17 * t) % 256 for t in range(T)]).astype(np.uint8),
            "still": np.stack([k % 256 for _ in range(T)]).astype(np.uint8)}


def _runs():
    """Every length at the start and at the very end of the clip."""
    starts = [0] * len(LENGTHS) + [T - n for n in LENGTHS]
    return np.asarray(starts), np.asarray(LENGTHS + LENGTHS)


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


@pytest.mark.parametrize("spec", LIGHTS)
def test_window_mean_against_the_numpy_restatement(spec):
    """8x16: the 16-byte path; 7x9: the pixel path; 8x16 one byte past an aligned address with a frame stride that is no multiple of
    16: the pixel path forced.  blur against light_ref, gt the middle frame, gray the plane the code-value launch makes of the blur."""
    from speinet_amd import ops
    starts, lengths = _runs()
    M = len(starts)
    for H, W, shift, extra in ((8, 16, 0, 0), (7, 9, 0, 0), (8, 16, 1, 7)):
        vector_path = H * W % 16 == 0 and shift % 16 == 0 and (H * W * 3 + extra) % 16 == 0
        assert vector_path == ((H, W, shift) == (8, 16, 0))
        for name, frames in _clips(H, W).items():
            if name in ("ramps", "still"):
                assert set(frames[:, :, :, :].reshape(-1).tolist()) == set(range(256)) or (name == "still" and H * W * 3 < 256)
            src = _on_device(frames, shift, H * W * 3 + extra)
            assert np.array_equal(src.cpu().numpy(), frames)
            blur, gt, gray = ops.window_mean_u8(src, starts, lengths, gray=True, light=spec)
            torch.cuda.synchronize()
            want = np.stack([light_ref.run_mean(frames[s:s + n], spec) for s, n in zip(starts, lengths)])
            assert np.array_equal(blur.cpu().numpy(), want), (H, W, shift, name)
            assert np.array_equal(gt.cpu().numpy(), np.stack([frames[s + n // 2] for s, n in zip(starts, lengths)])), (H, W, shift, name)
            again, _, gray_of_blur = ops.window_mean_u8(blur, np.arange(M), np.ones(M, np.int64), gray=True)
            assert torch.equal(again, blur) and torch.equal(gray, gray_of_blur), (H, W, shift, name)
            for m in np.flatnonzero(lengths == 1):                         # a run of length 1 returns its bytes
                assert np.array_equal(want[m], frames[starts[m]])
            if name in ("full", "zero", "still"):                            # ... and so does a run of identical frames
                assert np.array_equal(want, frames[:M])
    edge = np.zeros((2, 8, 16, 3), np.uint8)
    edge[1] = 255
    blur, _, _ = ops.window_mean_u8(torch.from_numpy(edge).to(DEV), [0], [2], light=spec)
    value = int(light_ref.run_mean(edge, spec)[0, 0, 0])                     # a black / white edge: far brighter than mid-gray
    assert set(blur.cpu().numpy().reshape(-1).tolist()) == {value} and value == {"srgb": 188, "gamma:2.2": 186, "gamma:1.0": 127}.get(spec, value)


def _resident(frames, pitch, frame_stride):
    n, H, W, _ = frames.shape
    host = np.zeros(n * frame_stride + 16, np.uint8)
    for t in range(n):
        rows = np.lib.stride_tricks.as_strided(host[t * frame_stride:], (H, W * 3), (pitch, 1))
        rows[...] = frames[t].reshape(H, W * 3)
    dev = torch.from_numpy(host).to(DEV)
    return dev, dev.data_ptr()


def _launch_runs(rec, n_in, n_gt, P, rgb_range=1.0, light=None):
    from speinet_amd import ops
    host = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())
    inp = torch.full((n_in, 3, P, P), -7.0, device=DEV)
    gt = torch.full((max(n_gt, 1), 3, P, P), -7.0, device=DEV)[:n_gt]
    with torch.cuda.device(DEV):
        ops.Ctx(device=DEV).train_batch_runs(host.to(DEV), host, n_in, n_gt, inp, gt, P, rgb_range, light=light)
    torch.cuda.synchronize()
    return inp.cpu().numpy(), gt.cpu().numpy()


def _place(img, y0, x0, P, h, v, r, rgb_range):
    img = img[y0:y0 + P, x0:x0 + P].astype(np.int64)
    if h:
        img = img[:, ::-1]
    if v:
        img = img[::-1, :]
    if r:
        img = np.rot90(img)
    return np.ascontiguousarray(img.transpose(2, 0, 1)).astype(np.float32) * np.float32(rgb_range / 255)


@pytest.mark.parametrize("spec", LIGHTS)
@pytest.mark.parametrize("P", [32, 36])
@pytest.mark.parametrize("H,W", [(40, 48), (41, 47)])
def test_batch_kernel_against_the_numpy_restatement(H, W, P, spec):
    """The cases of tests/test_gpu_sharpset.py's restatement test — 40x48 (dword path) and 41x47 (byte path), P = 32 (one full tile) and
    36 (partial tiles), lengths 1, 2, 3, 7, 15 x eight flag combinations x three origins x three layouts in memory, runs at the start
    and at the very end of their clip, some records zeroed, the last eight written to gt, rgb_range 1 and 255 — in a light."""
    from speinet_amd.data import RUN_RECORD
    clips = {k: v for k, v in _clips(H, W).items() if k in ("random", "full", "ramps")}
    frame = H * W * 3
    wide = (W * 3 + 3) // 4 * 4 + 4
    layouts = [(W * 3, frame), (wide, (H * wide + 11) // 4 * 4), (W * 3, frame + (5 if (frame + 5) % 4 else 6))]
    assert layouts[1][1] % 4 == 0 and layouts[1][1] > H * layouts[1][0] and layouts[2][1] % 4 != 0
    origins = [(0, 0), (H - P, W - P), (1, 3)]
    mean = {(name, start, n): light_ref.run_mean(frames[start:start + n], spec)
            for name, frames in clips.items() for n in LENGTHS for start in (0, T - n)}
    keep, rows, want_of = [], [], []
    for (name, frames), (pitch, fstride) in itertools.product(clips.items(), layouts):
        dev, base = _resident(frames, pitch, fstride)
        keep.append(dev)
        for i, (n, (h, v, r), (y0, x0)) in enumerate(itertools.product(LENGTHS, itertools.product((False, True), repeat=3), origins)):
            start = 0 if i % 2 else T - n
            zero = i % 17 == 5
            flags = (1 if h else 0) | (2 if v else 0) | (4 if r else 0) | (8 if zero else 0)
            rows.append((base + start * fstride, fstride, pitch, y0, x0, flags, H, W, n, T - start))
            want_of.append((name, start, n, y0, x0, h, v, r, zero))
    rec = np.array(rows, dtype=RUN_RECORD)
    n_gt = 8
    n_in = rec.size - n_gt
    assert rec.size == 3 * 3 * 5 * 8 * 3
    for rgb_range in (1.0, 255.0):
        got = np.concatenate(_launch_runs(rec, n_in, n_gt, P, rgb_range, spec))
        for k, (name, start, n, y0, x0, h, v, r, zero) in enumerate(want_of):
            want = np.zeros((3, P, P), np.float32) if zero else _place(mean[name, start, n], y0, x0, P, h, v, r, rgb_range)
            assert np.array_equal(got[k], want), (rgb_range, k, name, start, n, (y0, x0), (h, v, r), zero, tuple(rec[k])[1:3])
    k = next(k for k, w in enumerate(want_of) if w[2] == 7 and not w[8])   # _place is the restatement's own run_patch
    name, start, n, y0, x0, h, v, r, zero = want_of[k]
    assert np.array_equal(got[k], light_ref.run_patch(clips[name], start, n, y0, x0, P, h, v, r, zero, 255.0, spec))


@pytest.mark.parametrize("spec", LIGHTS)
def test_composition_with_synthesize(spec):
    """train_batch_runs(light) on the sharp clip == blurset.synthesize(light), then train_batch_u8 on the synthesized blur / gt frames,
    for every run of a plan; a gt record (a run of length 1) is the source crop; and the light matters."""
    from speinet_amd import blurset, ops
    from speinet_amd.data import RECORD, RUN_RECORD
    H, W, P, n = 40, 48, 36, 40
    frames = moving_clip(7, n, H, W)
    starts, lengths, _ = blurset.plan_runs(n, 0.5, rng=random.Random(1))
    M = len(starts)
    assert M >= 4 and lengths.max() > 5 and lengths.min() <= 5
    sharp = torch.from_numpy(frames).to(DEV)
    blur, mid = blurset.synthesize(sharp, (starts, lengths), DEV, light=spec)
    assert np.array_equal(blur.cpu().numpy(), np.stack([light_ref.run_mean(frames[s:s + k], spec) for s, k in zip(starts, lengths)]))
    assert torch.equal(mid, blurset.synthesize(sharp, (starts, lengths), DEV)[1])
    rng = random.Random(2)
    crops, runs = np.zeros(2 * M, dtype=RECORD), np.zeros(2 * M, dtype=RUN_RECORD)
    draws = []
    for m in range(M):
        y0, x0, flags = rng.randrange(H - P + 1), rng.randrange(W - P + 1), rng.randrange(8)
        draws.append((y0, x0, flags))
        s, ln = int(starts[m]), int(lengths[m])
        crops[m] = (blur.data_ptr() + m * H * W * 3, W * 3, y0, x0, flags, H, W)
        crops[M + m] = (mid.data_ptr() + m * H * W * 3, W * 3, y0, x0, flags, H, W)
        runs[m] = (sharp.data_ptr() + s * H * W * 3, H * W * 3, W * 3, y0, x0, flags, H, W, ln, n - s)
        runs[M + m] = (sharp.data_ptr() + (s + ln // 2) * H * W * 3, H * W * 3, W * 3, y0, x0, flags, H, W, 1, n - s - ln // 2)
    got_in, got_gt = _launch_runs(runs, M, M, P, light=spec)
    host = torch.from_numpy(crops.view(np.uint8).reshape(-1).copy())
    inp, gt = torch.full((M, 3, P, P), -7.0, device=DEV), torch.full((M, 3, P, P), -7.0, device=DEV)
    with torch.cuda.device(DEV):
        ops.Ctx(device=DEV).train_batch(host.to(DEV), host, M, M, inp, gt, P, 1.0)
    torch.cuda.synchronize()
    assert np.array_equal(got_in, inp.cpu().numpy()) and np.array_equal(got_gt, gt.cpu().numpy())
    for m, (y0, x0, flags) in enumerate(draws):
        src = frames[int(starts[m]) + int(lengths[m]) // 2]
        assert np.array_equal(got_gt[m], _place(src, y0, x0, P, flags & 1, flags & 2, flags & 4, 1.0)), m
    code_in, code_gt = _launch_runs(runs, M, M, P)
    assert np.array_equal(code_gt, got_gt) and not np.array_equal(code_in, got_in)


def test_code_and_none_are_the_unchanged_calls():
    from speinet_amd import blurset, ops
    from speinet_amd.data import RUN_RECORD
    H, W, P = 40, 48, 32
    frames = _clips(H, W)["random"]
    sharp = torch.from_numpy(frames).to(DEV)
    starts, lengths = _runs()
    plain = ops.window_mean_u8(sharp, starts, lengths, gray=True)
    for light in ("code", None):
        got = ops.window_mean_u8(sharp, starts, lengths, gray=True, light=light)
        assert all(torch.equal(a, b) for a, b in zip(got, plain)), light
        got = blurset.synthesize(sharp, (starts, lengths), DEV, gray=True, light=light)
        assert all(torch.equal(a, b) for a, b in zip(got, plain)), light
    assert np.array_equal(plain[0].cpu().numpy(), np.stack([light_ref.run_mean(frames[s:s + n], "code") for s, n in zip(starts, lengths)]))
    assert not torch.equal(ops.window_mean_u8(sharp, starts, lengths, light="srgb")[0], plain[0])
    rec = np.array([(sharp.data_ptr() + s * H * W * 3, H * W * 3, W * 3, 3, 5, m % 8, H, W, n, T - s)
                    for m, (s, n) in enumerate(zip(starts, lengths))], dtype=RUN_RECORD)
    host = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())
    outs = {}
    for light in ("plain", "code", None, "srgb"):
        inp = torch.full((len(rec), 3, P, P), -7.0, device=DEV)
        with torch.cuda.device(DEV):
            kw = {} if light == "plain" else {"light": light}
            ops.Ctx(device=DEV).train_batch_runs(host.to(DEV), host, len(rec), 0, inp, inp[:0], P, 1.0, **kw)
        torch.cuda.synchronize()
        outs[light] = inp
    assert torch.equal(outs["code"], outs["plain"]) and torch.equal(outs[None], outs["plain"]) and not torch.equal(outs["srgb"], outs["plain"])


def test_one_epoch_equals_the_written_set(tmp_path):
    """One epoch of SharpTrainLoader(light = srgb) == TrainLoader over ClipSet on what blurset.write_dataset(light = srgb) writes from the
    same clips: identical input and gt tensors in the same order — and not those of the code-value set."""
    from speinet_amd import blurset
    from speinet_amd.data import ClipSet, ClipStore, SharpClipSet, SharpStore, SharpTrainLoader, TrainLoader
    src = write_sharp(str(tmp_path / "sharp"), {f"clip{c}": moving_clip(40 + c, 24, 40, 48) for c in range(2)})
    seed, sampler_seed, patch, batch = 4, 3, 32, 2
    got = {}
    for light in ("srgb", "code"):
        cs = SharpClipSet(src, ratios=(0.5,), seed=seed, patch=patch, light=light)
        assert "light " + light in cs.summary()
        loader = SharpTrainLoader(cs, SharpStore(cs, device=DEV, log=None), batch, patch, seed=sampler_seed, rank=0, world=1)
        got[light] = [(i.clone(), g.clone()) for i, g in loader]
    out = str(tmp_path / "set")
    lines = []
    blurset.write_dataset(src, out, ratios=(0.5,), seed=seed, device=DEV, light="srgb", log=lines.append)
    assert len(lines) == 2 and all(ln.endswith("light srgb)") for ln in lines)
    ref_set = ClipSet(out, True, patch=patch)
    want = [(i.clone(), g.clone()) for i, g in
            TrainLoader(ref_set, ClipStore(ref_set, device=DEV, log=None), batch, patch, seed=sampler_seed, rank=0, world=1)]
    assert len(want) == len(got["srgb"]) == len(got["code"]) == -(-len(ref_set) // batch) > 3
    for k, ((i, g), (wi, wg), (ci, cg)) in enumerate(zip(got["srgb"], want, got["code"])):
        assert i.shape == wi.shape and i.shape[1:] == (5, 3, patch, patch) and torch.equal(i, wi) and torch.equal(g, wg), k
        assert torch.equal(g, cg), k
    assert any(not torch.equal(i, ci) for (i, _), (ci, _) in zip(got["srgb"], got["code"]))


def test_invalid_tables_launch_nothing():
    """An invalid pair handed straight to either entry point: non-zero, the text names the entry point, nothing is written."""
    from speinet_amd import _lib, light
    from speinet_amd.data import RUN_RECORD
    lib = _lib.lib()
    H, W, n, P = 8, 16, 4, 8
    clip = torch.zeros((n, H, W, 3), dtype=torch.uint8, device=DEV) + 9
    lin, thr = (a.astype(np.int64) for a in light.tables("srgb"))

    def edited(fn):
        l, t = lin.copy(), thr.copy()
        fn(l, t)
        return np.concatenate([l, t]).astype(np.uint32)

    cases = [("lin not increasing", edited(lambda l, t: l.__setitem__(100, l[99])), "code 100"),
             ("thr above lin", edited(lambda l, t: t.__setitem__(7, l[7] + 1)), "code 7"),
             ("lin[255] above S", edited(lambda l, t: l.__setitem__(255, S + 1)), "lin[255]"),
             ("lin[0] not 0", edited(lambda l, t: l.__setitem__(0, 1)), "lin[0]"),
             ("valid", edited(lambda l, t: None), None)]
    runs = torch.tensor([[0, 2]], dtype=torch.int32)
    rec = np.array([(clip.data_ptr(), H * W * 3, W * 3, 0, 0, 0, H, W, 2, n)], dtype=RUN_RECORD)
    rec_host = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())
    runs_dev, rec_dev = runs.to(DEV), rec_host.to(DEV)
    for what, words, text in cases:
        tab_host = torch.from_numpy(words.view(np.int32).copy())
        tab = tab_host.to(DEV)
        blur = torch.full((1, H, W, 3), 77, dtype=torch.uint8, device=DEV)
        gt = torch.full((1, H, W, 3), 77, dtype=torch.uint8, device=DEV)
        inp = torch.full((1, 3, P, P), -7.0, device=DEV)
        with torch.cuda.device(DEV):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc_w = lib.spei_window_mean_light_u8(C.c_void_p(clip.data_ptr()), H * W * 3, n, C.c_void_p(runs_dev.data_ptr()),
                                                 C.c_void_p(runs.data_ptr()), 1, C.c_void_p(tab.data_ptr()), C.c_void_p(tab_host.data_ptr()),
                                                 C.c_void_p(blur.data_ptr()), C.c_void_p(gt.data_ptr()), C.c_void_p(0), H, W, st)
            msg_w = lib.spei_last_error().decode()
            rc_b = lib.spei_train_batch_runs_light_u8(C.c_void_p(rec_dev.data_ptr()), C.c_void_p(rec_host.data_ptr()), 1, 0,
                                                      C.c_void_p(tab.data_ptr()), C.c_void_p(tab_host.data_ptr()), C.c_void_p(inp.data_ptr()),
                                                      C.c_void_p(0), P, 1.0, st)
            msg_b = lib.spei_last_error().decode()
        torch.cuda.synchronize()
        if text is None:
            assert rc_w == 0 and rc_b == 0, (msg_w, msg_b)
            assert bool((blur == 9).all()) and bool((gt == 9).all()) and bool((inp == np.float32(9) * np.float32(1 / 255)).all())
            continue
        assert rc_w != 0 and msg_w.startswith("spei_window_mean_light_u8: invalid light tables") and text in msg_w, (what, rc_w, msg_w)
        assert rc_b != 0 and msg_b.startswith("spei_train_batch_runs_light_u8: invalid light tables") and text in msg_b, (what, rc_b, msg_b)
        assert bool((blur == 77).all()) and bool((gt == 77).all()) and bool((inp == -7.0).all()), what       # nothing was launched
    # a missing host copy or device table is refused as well
    tab_host = torch.from_numpy(cases[-1][1].view(np.int32).copy())
    tab = tab_host.to(DEV)
    with torch.cuda.device(DEV):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for d, h in ((0, tab_host.data_ptr()), (tab.data_ptr(), 0)):
            rc = lib.spei_train_batch_runs_light_u8(C.c_void_p(rec_dev.data_ptr()), C.c_void_p(rec_host.data_ptr()), 1, 0, C.c_void_p(d),
                                                    C.c_void_p(h), C.c_void_p(inp.data_ptr()), C.c_void_p(0), P, 1.0, st)
            assert rc != 0 and "null light tables" in lib.spei_last_error().decode()
    torch.cuda.synchronize()
