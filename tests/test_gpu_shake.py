"""Camera-shake blur of blur synthesis on the device: spei_window_mean_shake_u8 and spei_train_batch_runs_shake_u8 (csrc/shake.hip)
bit for bit against the numpy restatement tests/shake_ref.py, against the light and noise entries where they must agree,
blurset.synthesize across chunk sizes, the checks that refuse a launch, and blurset.write_dataset / data.SharpTrainLoader end to end.
Equality throughout: the arithmetic is integer."""
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

import noise_ref  # noqa: E402
import shake_ref  # noqa: E402
from sharpset_ref import moving_clip, write_sharp  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 32                                                   # csrc/shake.hip: one workgroup per 32 x 32 output tile
T = 17
STARTS, LENGTHS = np.array([0, 1, 2]), np.array([1, 2, 15])  # runs of 1, 2 and 15 frames
SEED = (7 << 32) | 11
CLIP, FIRST_RUN = 3, 5
# 13 x 21: both smaller than the radius 16, so both clamps act inside one tap window; 70 x 150: more than two tiles each way, no multiple
# of the tile, rows of 450 bytes (the byte path); 68 x 148: the same with W % 4 == 0 (the 12-byte / 16-byte path)
SIZES = [(13, 21), (70, 150), (68, 148)]
assert all(H > 2 * TILE and W > 2 * TILE and H % TILE and W % TILE for H, W in SIZES[1:])


def _psfs():
    """name -> (table int64 [33,33], radius): fixed tables, and one generated trajectory PSF."""
    from speinet_amd import shake
    traj = shake.psf("4..24", 5, 1, 2)
    assert traj[1] > 4
    return {"delta": (shake_ref.delta(), 0), "tap(-16,+16)": (shake_ref.tap(-16, 16), 16), "tap(+3,-7)": (shake_ref.tap(3, -7), 7),
            "dense16": (shake_ref.dense(16, 1), 16), "dense1": (shake_ref.dense(1, 2), 1), "dense7": (shake_ref.dense(7, 3), 7),
            "trajectory": (traj[0].astype(np.int64), traj[1])}


PSFS = _psfs()
_REF = {}                                                   # the restatement's full frames of test_batch_kernel


def _table(names):
    """(uint32 [n,33,33] of the named PSFs with a radius above 0, name -> record fields (psf, radius, q16, 0))."""
    tabs, fields = [], {}
    for name in names:
        w, radius = PSFS[name]
        if radius == 0:
            fields[name] = (0, 0, 65536, 0)
        else:
            fields[name] = (len(tabs), radius, shake_ref.q16_of(w), 0)
            tabs.append(w)
    return (np.stack(tabs).astype(np.uint32) if tabs else np.zeros((0, 33, 33), np.uint32)), fields


def _shake_records(fields):
    from speinet_amd import shake
    rec = np.zeros(len(fields), dtype=shake.SHAKE_RECORD)
    for i, f in enumerate(fields):
        rec[i] = f
    return rec


def _noise_records(runs, clip, A, B):
    from speinet_amd import light
    rec = np.zeros(len(runs), dtype=light.NOISE_RECORD)
    rec["run"], rec["clip"], rec["A"], rec["B"] = runs, clip, A, B
    return rec


def _clip(H, W, content):
    rs = np.random.RandomState(H * 1000 + W)
    if content == "random":
        return rs.randint(0, 256, (T, H, W, 3)).astype(np.uint8)
    frames = np.zeros((T, H, W, 3), np.uint8)                 # a black / white edge that moves one column per frame
    for t in range(T):
        frames[t, :, (W // 3 + t) % W:] = 255
    return frames


def _window_case(H, W, content, spec, names, noise):
    """Every run under every named PSF in ONE launch -> (frames, got blur / gt / gray, want blur)."""
    from speinet_amd import ops
    frames = _clip(H, W, content)
    table, fields = _table(names)
    starts, lengths = np.tile(STARTS, len(names)), np.tile(LENGTHS, len(names))
    rec = _shake_records([fields[n] for n in names for _ in STARTS])
    runs = FIRST_RUN + np.arange(starts.size)
    nz = None if noise is None else (_noise_records(runs, CLIP, *noise), SEED)
    got = ops.window_mean_u8(torch.from_numpy(frames).to(DEV), starts, lengths, gray=True, light=spec, noise=nz, shake=(rec, table))
    torch.cuda.synchronize()
    want = np.stack([shake_ref.run_mean(frames[s:s + n], spec, *PSFS[name], None if noise is None else (run, CLIP, SEED) + noise)
                     for (name, (s, n)), run in zip(itertools.product(names, zip(STARTS, LENGTHS)), runs)])
    return frames, starts, lengths, got, want


@pytest.mark.parametrize("spec", ["srgb", "gamma:2.2"])
@pytest.mark.parametrize("H,W", SIZES)
def test_window_mean_against_the_numpy_restatement(H, W, spec):
    """Runs of 1, 2 and 15 frames under each of the seven PSFs in one launch, random bytes and a black / white edge: blur bit for bit,
    gt the run's middle frame, the gray plane that of the encoded bytes.  The delta returns the light entry's bytes."""
    from speinet_amd import ops
    names = list(PSFS)
    for content in ("random", "edge"):
        frames, starts, lengths, (blur, gt, gray), want = _window_case(H, W, content, spec, names, None)
        got = blur.cpu().numpy()
        for m in range(starts.size):
            assert np.array_equal(got[m], want[m]), (H, W, spec, content, names[m // 3], int(lengths[m]))
        assert np.array_equal(gt.cpu().numpy(), np.stack([frames[s + n // 2] for s, n in zip(starts, lengths)]))
        _, _, gray_of_blur = ops.window_mean_u8(blur, np.arange(starts.size), np.ones(starts.size, np.int64), gray=True)
        assert torch.equal(gray, gray_of_blur)
        plain = ops.window_mean_u8(torch.from_numpy(frames).to(DEV), STARTS, LENGTHS, light=spec)[0].cpu().numpy()
        assert np.array_equal(got[:3], plain) and not np.array_equal(got[3:6], plain)


def test_white_stays_white():
    """The overflow guard: an all-255 clip under the dense radius-16 PSF returns 255 (the exact sum reaches 65536 S)."""
    from speinet_amd import ops
    table, fields = _table(["dense16"])
    for H, W in SIZES[:2]:
        src = torch.full((T, H, W, 3), 255, dtype=torch.uint8, device=DEV)
        for noise in (None, (_noise_records(np.arange(3), 0, 0, 0), SEED)):
            blur, gt, _ = ops.window_mean_u8(src, STARTS, LENGTHS, light="srgb", noise=noise, shake=(_shake_records([fields["dense16"]] * 3), table))
            assert bool((blur == 255).all()) and bool((gt == 255).all())


@pytest.mark.parametrize("H,W", SIZES)
def test_noise_composed(H, W):
    """A, B non-zero, lengths 1, 2 and 15, the dense and the trajectory PSF (and the delta: the noise entry's bytes): blur and the gray
    plane of the noisy bytes.  A run of length 1 under a PSF carries noise (q16 < 65536); under the delta it returns its bytes."""
    from speinet_amd import ops
    levels = noise_ref.levels(5e-3, 1e-2)
    names = ["dense16", "trajectory", "delta", "dense1"]
    frames, starts, lengths, (blur, gt, gray), want = _window_case(H, W, "random", "srgb", names, levels)
    got = blur.cpu().numpy()
    for m in range(starts.size):
        assert np.array_equal(got[m], want[m]), (H, W, names[m // 3], int(lengths[m]))
    _, _, gray_of_blur = ops.window_mean_u8(blur, np.arange(starts.size), np.ones(starts.size, np.int64), gray=True)
    assert torch.equal(gray, gray_of_blur)
    assert np.array_equal(got[6], frames[0])                                     # delta, length 1
    clean = shake_ref.run_mean(frames[0:1], "srgb", *PSFS["dense16"])
    assert not np.array_equal(got[0], clean)                                     # dense, length 1: the noise is there
    if (H, W) == SIZES[0]:                                                       # the largest levels and gamma:2.2 once, at the small size
        top = noise_ref.levels(0.05, 0.1)
        _f, _s, lengths, (blur, _g, _y), want = _window_case(H, W, "random", "gamma:2.2", names, top)
        assert np.array_equal(blur.cpu().numpy(), want)


def _launch_runs(rec, n_in, n_gt, P, rgb_range, light, noise, shake):
    from speinet_amd import ops
    from speinet_amd.shake import device_psfs
    host = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())
    inp = torch.full((n_in, 3, P, P), -7.0, device=DEV)
    gt = torch.full((max(n_gt, 1), 3, P, P), -7.0, device=DEV)[:n_gt]
    if noise is not None:
        nhost = torch.from_numpy(noise[0].view(np.uint8).reshape(-1).copy())
        noise = (nhost.to(DEV), nhost, noise[1])
    if shake is not None:
        shost = torch.from_numpy(shake[0].view(np.uint8).reshape(-1).copy())
        shake = (shost.to(DEV), shost, device_psfs(shake[1], DEV))
    with torch.cuda.device(DEV):
        ops.Ctx(device=DEV).train_batch_runs(host.to(DEV), host, n_in, n_gt, inp, gt, P, rgb_range, light=light, noise=noise, shake=shake)
    torch.cuda.synchronize()
    return inp.cpu().numpy(), gt.cpu().numpy()


def test_all_radius_zero_is_the_light_and_noise_entries():
    """Every record at radius 0: the shake entries return the noise entries' output (with gauss) and the light entries' (without)."""
    from speinet_amd import ops
    from speinet_amd.data import RUN_RECORD
    H, W, P = 70, 150, 40
    frames = _clip(H, W, "random")
    src = torch.from_numpy(frames).to(DEV)
    still = (_shake_records([(0, 0, 65536, 0)] * 3), np.zeros((0, 33, 33), np.uint32))
    nz = (_noise_records(FIRST_RUN + np.arange(3), CLIP, *noise_ref.levels(5e-3, 1e-2)), SEED)
    for noise in (None, nz):
        want = ops.window_mean_u8(src, STARTS, LENGTHS, gray=True, light="srgb", noise=noise)
        got = ops.window_mean_u8(src, STARTS, LENGTHS, gray=True, light="srgb", noise=noise, shake=still)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    frame = H * W * 3
    rows = [(src.data_ptr() + s * frame, frame, W * 3, 7, 9, f, H, W, n, T - s) for f, (s, n) in enumerate(zip(STARTS, LENGTHS))]
    rows.append((src.data_ptr() + 9 * frame, frame, W * 3, 7, 9, 0, H, W, 1, T - 9))
    rec = np.array(rows, dtype=RUN_RECORD)
    nz4 = (_noise_records([5, 6, 7, 7], CLIP, *noise_ref.levels(5e-3, 1e-2)), SEED)
    still4 = (_shake_records([(0, 0, 65536, 0)] * 4), np.zeros((0, 33, 33), np.uint32))
    for noise in (None, nz4):
        want = _launch_runs(rec, 3, 1, P, 1.0, "srgb", noise, None)
        got = _launch_runs(rec, 3, 1, P, 1.0, "srgb", noise, still4)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # a delta beside shaken records (the mixed launch's radius-0 path) still returns the light / noise entries' bytes
    table, fields = _table(["dense7"])
    mixed = (_shake_records([(0, 0, 65536, 0), (0, 0, 65536, 0), (0, 0, 65536, 0), fields["dense7"]]), table)
    for noise in (None, nz4):
        want = _launch_runs(rec, 3, 1, P, 1.0, "srgb", noise, None)
        got = _launch_runs(rec, 4, 0, P, 1.0, "srgb", noise, mixed)
        assert np.array_equal(got[0][:3], want[0])


@pytest.mark.parametrize("P", [8, 40])
@pytest.mark.parametrize("H,W", SIZES[1:])
def test_batch_kernel(H, W, P):
    """All eight flag combinations and a zero record; crops at the frame's two far corners (the halo clamps to the frame) and in the
    interior (the halo reads the real neighbours outside the crop: random bytes, so they differ from the border); lengths 1, 2, 15;
    the dense, trajectory and single-tap PSFs and the delta; with and without noise.  Every output frame is scale * the bytes the
    window-mean shake entry gives for the same run, cropped and augmented, and those are the restatement's."""
    from speinet_amd import ops
    from speinet_amd.data import RUN_RECORD
    frames = _clip(H, W, "random")
    src = torch.from_numpy(frames).to(DEV)
    names = ["dense16", "trajectory", "tap(-16,+16)", "tap(+3,-7)", "delta"]
    table, fields = _table(names)
    origins = [(0, 0), (H - P, W - P), ((H - P) // 2, (W - P) // 2)]
    levels = noise_ref.levels(5e-3, 1e-2)
    frame = H * W * 3
    rows, srec, nrec, what = [], [], [], []
    for i, (h, v, r) in enumerate(itertools.product((False, True), repeat=3)):
        for j, (y0, x0) in enumerate(origins):
            k = 3 * i + j
            name, (s, n) = names[k % 5], (int(STARTS[k % 3]), int(LENGTHS[k % 3]))
            zero = k == 13
            flags = (1 if h else 0) | (2 if v else 0) | (4 if r else 0) | (8 if zero else 0)
            rows.append((src.data_ptr() + s * frame, frame, W * 3, y0, x0, flags, H, W, n, T - s))
            srec.append(fields[name])
            nrec.append(40 + k % 3)
            what.append((name, s, n, 40 + k % 3, y0, x0, h, v, r, zero))
    n_in = len(rows)
    rows.append((src.data_ptr() + 9 * frame, frame, W * 3, 2, 4, 5, H, W, 1, T - 9))     # a gt record: length 1, radius 0
    srec.append((0, 0, 65536, 0))
    nrec.append(41)
    rec, srec = np.array(rows, dtype=RUN_RECORD), _shake_records(srec)
    assert len({w[6:9] for w in what}) == 8 and {w[0] for w in what} == set(names) and {w[2] for w in what} == {1, 2, 15}
    for noise in (None, levels):
        nz = None if noise is None else (_noise_records(nrec, CLIP, *noise), SEED)
        inp, gt = _launch_runs(rec, n_in, 1, P, 255.0, "srgb", nz, (srec, table))
        full, full_ref = {}, {}
        for k, (name, s, n, run, y0, x0, h, v, r, zero) in enumerate(what):
            key = (name, s, n, run)
            if key not in full and not zero:
                one = (_shake_records([fields[name]]), table)
                nz1 = None if noise is None else (_noise_records([run], CLIP, *noise), SEED)
                full[key] = ops.window_mean_u8(src, [s], [n], light="srgb", noise=nz1, shake=one)[0][0].cpu().numpy()
                if (H, W, key, noise) not in _REF:                                # computed once, shared by both patch sizes
                    _REF[H, W, key, noise] = shake_ref.run_mean(frames[s:s + n], "srgb", *PSFS[name],
                                                                None if noise is None else (run, CLIP, SEED) + noise)
                full_ref[key] = _REF[H, W, key, noise]
                assert np.array_equal(full[key], full_ref[key]), (key, noise)
            want = shake_ref.run_patch(None if zero else full[key], y0, x0, P, h, v, r, zero, 255.0)
            assert np.array_equal(inp[k], want), (k, what[k], noise)
        assert np.array_equal(gt[0], noise_ref.place(frames[9], 2, 4, P, True, False, True, 255.0))
    # the interior crop under the far tap shows pixels from outside the crop, not its clamped border
    k = next(k for k, w in enumerate(what) if w[0] == "tap(-16,+16)" and (w[4], w[5]) == origins[2] and not w[9])
    name, s, n, run, y0, x0, h, v, r, zero = what[k]
    inside = shake_ref.run_mean(frames[s:s + n, y0:y0 + P, x0:x0 + P], "srgb", *PSFS[name])
    assert not np.array_equal(_REF[H, W, (name, s, n, run), None][y0:y0 + P, x0:x0 + P], inside)


def test_synthesize_does_not_depend_on_the_chunk():
    """blurset.synthesize(shake=) with chunks of 15 frames and of 64: identical bytes and gray planes, those of the restatement with
    the PSF of every label-0 run drawn from (seed, clip, global run id); with noise on top."""
    from speinet_amd import blurset, light, shake
    H, W, n = 20, 24, 60
    frames = moving_clip(9, n, H, W)
    runs = blurset.plan_runs(n, 0.5, rng=random.Random(1))
    starts, lengths, labels = runs
    assert len(list(blurset._chunks(starts, lengths, 15))) > 2 and len(list(blurset._chunks(starts, lengths, 64))) == 1
    assert (labels == 0).sum() > 2 and (labels == 1).sum() > 2
    spec, noise, sk = "srgb", "5e-3..2e-2:1e-2", "4..12"
    outs = [blurset.synthesize(frames, runs, DEV, gray=True, chunk_frames=c, light=spec, noise=light.ClipNoise(noise, 21, 2),
                               shake=shake.ClipShake(sk, 21, 2)) for c in (15, 64)]
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    A, B = light.noise_levels(noise, 21, 2)
    want = []
    for m, (s, k, lab) in enumerate(zip(starts, lengths, labels)):
        w, radius, _ = shake.psf(sk, 21, 2, m) if lab == 0 else (None, 0, 0)
        want.append(shake_ref.run_mean(frames[s:s + k], spec, w, radius, (m, 2, 21, A, B)))
    assert np.array_equal(outs[0][0].cpu().numpy(), np.stack(want))
    plain = blurset.synthesize(frames, runs, DEV, light=spec, noise=light.ClipNoise(noise, 21, 2))[0].cpu().numpy()
    assert all(np.array_equal(plain[m], want[m]) == bool(lab) for m, lab in enumerate(labels))
    with pytest.raises(ValueError, match="--light / --blur_light"):
        blurset.synthesize(frames, runs, DEV, shake=shake.ClipShake(sk, 21, 2))
    with pytest.raises(ValueError, match="labels"):
        blurset.synthesize(frames, runs[:2], DEV, light=spec, shake=shake.ClipShake(sk, 21, 2))


def test_invalid_records_launch_nothing():
    """Each bad shake record, second of two, handed straight to either entry point: non-zero, the text names the entry point and the
    record, and the outputs, pre-filled with a sentinel, are untouched."""
    from speinet_amd import _lib, light
    from speinet_amd.data import RUN_RECORD
    lib = _lib.lib()
    H, W, n, P = 8, 16, 4, 8
    clip = torch.zeros((n, H, W, 3), dtype=torch.uint8, device=DEV) + 9
    tab_host = torch.from_numpy(np.concatenate(light.tables("srgb")).astype(np.int32))
    tab = tab_host.to(DEV)
    good = shake_ref.dense(7, 3)
    top = np.unravel_index(np.argmax(good), good.shape)
    short = good.copy()
    short[top] -= 1
    outside = good.copy()
    outside[top] -= 1
    outside[16 + 8, 16] += 1
    q = shake_ref.q16_of(good)
    cases = [("the sum is not 65536", short, (0, 7, shake_ref.q16_of(short), 0), "sum to 65535"),
             ("a weight outside the radius", outside, (0, 7, shake_ref.q16_of(outside), 0), "outside its radius 7"),
             ("radius 17", good, (0, 17, q, 0), "radius 17"),
             ("psf >= n_psf", good, (1, 7, q, 0), "PSF 1 of 1"),
             ("a wrong q16", good, (0, 7, q + 1, 0), f"q16 = {q + 1}"),
             ("reserved != 0", good, (0, 7, q, 1), "reserved = 1"),
             ("radius 0 with q16 != 65536", good, (0, 0, q, 0), "must be 65536"),
             ("valid", good, (0, 7, q, 0), None)]
    runs = torch.tensor([[0, 2], [1, 2]], dtype=torch.int32)
    rec = np.array([(clip.data_ptr(), H * W * 3, W * 3, 0, 0, 0, H, W, 2, n)] * 2, dtype=RUN_RECORD)
    rec_host = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())
    runs_dev, rec_dev = runs.to(DEV), rec_host.to(DEV)
    null = C.c_void_p(0)
    for what, table, fields, text in cases:
        psf_host = torch.from_numpy(table.astype(np.uint32).view(np.int32).copy())
        psf = psf_host.to(DEV)
        srec = _shake_records([(0, 0, 65536, 0), fields])
        s_host = torch.from_numpy(srec.view(np.uint8).copy())
        s_dev = s_host.to(DEV)
        blur = torch.full((2, H, W, 3), 77, dtype=torch.uint8, device=DEV)
        gt = torch.full((2, H, W, 3), 77, dtype=torch.uint8, device=DEV)
        inp = torch.full((2, 3, P, P), -7.0, device=DEV)
        with torch.cuda.device(DEV):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc_w = lib.spei_window_mean_shake_u8(C.c_void_p(clip.data_ptr()), H * W * 3, n, C.c_void_p(runs_dev.data_ptr()),
                                                 C.c_void_p(runs.data_ptr()), 2, C.c_void_p(tab.data_ptr()), C.c_void_p(tab_host.data_ptr()),
                                                 null, null, null, null, 0, 0, C.c_void_p(psf.data_ptr()), C.c_void_p(psf_host.data_ptr()), 1,
                                                 C.c_void_p(s_dev.data_ptr()), C.c_void_p(s_host.data_ptr()), C.c_void_p(blur.data_ptr()),
                                                 C.c_void_p(gt.data_ptr()), null, H, W, st)
            msg_w = lib.spei_last_error().decode()
            rc_b = lib.spei_train_batch_runs_shake_u8(C.c_void_p(rec_dev.data_ptr()), C.c_void_p(rec_host.data_ptr()), 2, 0,
                                                      C.c_void_p(tab.data_ptr()), C.c_void_p(tab_host.data_ptr()), null, null, null, null, 0, 0,
                                                      C.c_void_p(psf.data_ptr()), C.c_void_p(psf_host.data_ptr()), 1,
                                                      C.c_void_p(s_dev.data_ptr()), C.c_void_p(s_host.data_ptr()), C.c_void_p(inp.data_ptr()),
                                                      null, P, 1.0, st)
            msg_b = lib.spei_last_error().decode()
        torch.cuda.synchronize()
        if text is None:                                                         # identical frames of code 9 under any PSF: code 9
            assert rc_w == 0 and rc_b == 0, (msg_w, msg_b)
            assert bool((gt == 9).all()) and bool((blur == 9).all()) and bool((inp == float(np.float32(9) * np.float32(1 / 255))).all())
            continue
        assert rc_w != 0 and msg_w.startswith("spei_window_mean_shake_u8: shake record 1: ") and text in msg_w, (what, rc_w, msg_w)
        assert rc_b != 0 and msg_b.startswith("spei_train_batch_runs_shake_u8: shake record 1: ") and text in msg_b, (what, rc_b, msg_b)
        assert bool((blur == 77).all()) and bool((gt == 77).all()) and bool((inp == -7.0).all()), what       # nothing was launched
    # every check of the light entries stays: a run that leaves the clip and an invalid light table are refused before the shake
    bad_tab_host = tab_host.clone()
    bad_tab_host[100] = bad_tab_host[99]
    blur = torch.full((2, H, W, 3), 77, dtype=torch.uint8, device=DEV)
    inp = torch.full((2, 3, P, P), -7.0, device=DEV)
    with torch.cuda.device(DEV):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = lib.spei_train_batch_runs_shake_u8(C.c_void_p(rec_dev.data_ptr()), C.c_void_p(rec_host.data_ptr()), 2, 0, C.c_void_p(tab.data_ptr()),
                                                C.c_void_p(bad_tab_host.data_ptr()), null, null, null, null, 0, 0, C.c_void_p(psf.data_ptr()),
                                                C.c_void_p(psf_host.data_ptr()), 1, C.c_void_p(s_dev.data_ptr()), C.c_void_p(s_host.data_ptr()),
                                                C.c_void_p(inp.data_ptr()), null, P, 1.0, st)
        assert rc != 0 and "invalid light tables at code 100" in lib.spei_last_error().decode()
        far = torch.tensor([[0, 2], [3, 2]], dtype=torch.int32)
        rc = lib.spei_window_mean_shake_u8(C.c_void_p(clip.data_ptr()), H * W * 3, n, C.c_void_p(runs_dev.data_ptr()), C.c_void_p(far.data_ptr()),
                                           2, C.c_void_p(tab.data_ptr()), C.c_void_p(tab_host.data_ptr()), null, null, null, null, 0, 0,
                                           C.c_void_p(psf.data_ptr()), C.c_void_p(psf_host.data_ptr()), 1, C.c_void_p(s_dev.data_ptr()),
                                           C.c_void_p(s_host.data_ptr()), C.c_void_p(blur.data_ptr()), C.c_void_p(gt.data_ptr()), null, H, W, st)
        assert rc != 0 and "leaves the clip" in lib.spei_last_error().decode()
    torch.cuda.synchronize()
    assert bool((inp == -7.0).all()) and bool((blur == 77).all())


def test_write_dataset_single_frames_and_the_loader(tmp_path):
    """blurset.write_dataset(frames="single", shake="4..12") on 6-frame 40 x 40 clips writes the blur / gt / label layout: gt is the
    source byte for byte, label-1 frames have blur == gt, label-0 frames are the restatement's shaken frames.  One epoch of
    SharpTrainLoader with the same shake equals TrainLoader over that written set, tensor for tensor."""
    from speinet_amd import blurset, shake
    from speinet_amd.data import ClipSet, ClipStore, SharpClipSet, SharpStore, SharpTrainLoader, TrainLoader
    from speinet_amd.video import _imread
    clips = {f"clip{c}": moving_clip(50 + c, 6, 40, 40) for c in range(2)}
    src = write_sharp(str(tmp_path / "sharp"), clips)
    seed, spec, sk, patch, batch = 2, "srgb", "4..12", 32, 2
    out = str(tmp_path / "set")
    done = blurset.write_dataset(src, out, ratios=(0.5,), seed=seed, device=DEV, light=spec, shake=sk, frames="single")
    plans = blurset.plan_dataset([6, 6], [0.5], seed, frames="single")
    assert sorted(os.listdir(out)) == ["blur", "gt", "label"]
    all_labels = []
    for k, (name, frames) in enumerate(sorted(clips.items())):
        labels = np.load(os.path.join(out, "label", name + ".npy"))
        assert labels.tolist() == plans[k][1][2].tolist() == done[k]["labels"].tolist() and labels.size == 6
        all_labels += labels.tolist()
        for m in range(6):
            blur, gt = (_imread(os.path.join(out, d, name, f"{m:06d}.png")) for d in ("blur", "gt"))
            assert np.array_equal(gt, frames[m])
            w, radius, _ = shake.psf(sk, seed, k, m) if labels[m] == 0 else (None, 0, 0)
            assert np.array_equal(blur, shake_ref.run_mean(frames[m:m + 1], spec, w, radius))
            assert np.array_equal(blur, gt) == bool(labels[m])
    assert 0 in all_labels and 1 in all_labels
    cs = SharpClipSet(src, ratios=(0.5,), seed=seed, patch=patch, light=spec, shake=sk, frames="single")
    loader = SharpTrainLoader(cs, SharpStore(cs, device=DEV, log=None), batch, patch, seed=3, rank=0, world=1)
    got = [(i.clone(), g.clone()) for i, g in loader]
    ref_set = ClipSet(out, True, patch=patch)
    ref = TrainLoader(ref_set, ClipStore(ref_set, device=DEV, log=None), batch, patch, seed=3, rank=0, world=1)
    want = [(i.clone(), g.clone()) for i, g in ref]
    assert len(got) == len(want) > 1
    for (i, g), (wi, wg) in zip(got, want):
        assert i.shape == wi.shape and torch.equal(i, wi) and torch.equal(g, wg)
    with pytest.raises(ValueError, match="single"):
        blurset.write_dataset(src, str(tmp_path / "none"), ratios=(0.5,), seed=seed, device=DEV, light=spec, frames="single")
