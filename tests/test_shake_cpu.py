"""Camera-shake blur of blur synthesis on the host: the numpy restatement tests/shake_ref.py against itself, speinet_amd.shake's PSF
generator, records, parser and plans, the C-ABI's declaration and the command lines.  No GPU."""
import math
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import light_ref  # noqa: E402
import noise_ref  # noqa: E402
import shake_ref  # noqa: E402
from shake_ref import S  # noqa: E402

SEEDS = [0, 1, (7 << 32) | 11, 2 ** 63 + 5]


def test_radius_zero_is_the_light_and_noise_restatement():
    """Radius 0 (the delta) returns light_ref's / noise_ref's bytes; the delta pushed through the correlation and the generalised
    variance does too: Lb = Lm and V = floor(X (n - 1) / n)."""
    rs = np.random.RandomState(3)
    frames = rs.randint(0, 256, (15, 9, 7, 3)).astype(np.uint8)
    A, B = noise_ref.levels(5e-3, 1e-2)
    for spec in ("srgb", "gamma:2.2"):
        lin, thr = light_ref.tables(spec)
        for n in (1, 2, 15):
            noise = (4, 2, 9, A, B)
            assert np.array_equal(shake_ref.run_mean(frames[:n], spec, shake_ref.delta(), 0), light_ref.run_mean(frames[:n], spec))
            assert np.array_equal(shake_ref.run_mean(frames[:n], spec, shake_ref.delta(), 0, noise), noise_ref.run_mean(frames[:n], spec, *noise))
            Lm = lin[frames[:n]].sum(axis=0) // n
            assert np.array_equal(shake_ref.correlate(Lm, shake_ref.delta()), Lm)
            z = noise_ref.z_of(noise_ref.words(9, 7, 4, 2, 9))
            assert np.array_equal(shake_ref.apply_noise(Lm, z, A, B, n, 65536), noise_ref.apply(Lm, z, A, B, n))
            assert np.array_equal(light_ref.encode(thr, shake_ref.apply_noise(Lm, z, A, B, n, 65536)).astype(np.uint8),
                                  noise_ref.run_mean(frames[:n], spec, *noise))


def test_white_stays_white_and_taps_shift():
    """The overflow guard: an all-255 frame under any valid PSF stays 255 (the sum reaches 65536 S).  A single tap at (dy, dx) returns
    the frame shifted so that the output pixel shows the one dy rows below and dx columns to the right, the edges repeated."""
    white = np.full((2, 13, 21, 3), 255, np.uint8)
    for w, r in ((shake_ref.dense(16, 1), 16), (shake_ref.dense(1, 2), 1), (shake_ref.tap(-16, 16), 16)):
        assert shake_ref.valid(w, r) and shake_ref.q16_of(w) <= 65536
        for spec in ("srgb", "gamma:2.2"):
            assert (shake_ref.run_mean(white, spec, w, r) == 255).all()
            assert int(shake_ref.correlate(np.full((5, 5, 3), S, np.int64), w).max()) == S
    frame = np.random.RandomState(0).randint(0, 256, (1, 13, 21, 3)).astype(np.uint8)
    for dy, dx in ((-16, 16), (3, -7)):
        got = shake_ref.run_mean(frame, "srgb", shake_ref.tap(dy, dx), 16)
        y, x = np.clip(np.arange(13) + dy, 0, 12), np.clip(np.arange(21) + dx, 0, 20)
        assert np.array_equal(got, frame[0][y][:, x])
    assert shake_ref.q16_of(shake_ref.delta()) == 65536 and shake_ref.q16_of(shake_ref.tap(3, -7)) == 65536


def test_generalised_variance():
    """V = X - ceil(X q16 / (n 2^16)) against Python's big integers, up to the largest X = A S + B; z = 1 (Q12 4096) makes d = isqrt(V)."""
    for A, L, B, q16, n in ((2 ** 20 - 1, S, 2 ** 42 - 1, 65536, 15), (2 ** 20 - 1, S, 2 ** 42 - 1, 65535, 1), (0, 0, 12345678901, 732, 7),
                            (0, 0, 1, 1, 1), (0, 0, 0, 5, 3), (1000, 2 ** 20, 7, 40000, 2), (5, 1, 0, 65536, 1)):
        X, D = A * L + B, n * 65536
        V = X - (X * q16 + D - 1) // D
        assert 0 <= V <= X < 2 ** 45
        got = shake_ref.apply_noise(np.array([L], np.int64), np.array([4096], np.int64), A, B, n, q16)
        assert int(got[0]) == min(L + math.isqrt(V), S), (A, L, B, q16, n)
        if q16 == 65536:
            assert V == X * (n - 1) // n


@pytest.mark.parametrize("seed", SEEDS)
def test_psf_generator(seed):
    from speinet_amd import shake
    ys, xs = np.mgrid[-16:17, -16:17]
    seen = []
    for clip, run in ((0, 0), (0, 1), (3, 0), (2, 77)):
        w, radius, q16 = shake.psf("2..30", seed, clip, run)
        L = shake.extent("2..30", seed, clip, run)
        assert w.dtype == np.uint32 and w.shape == (33, 33) and int(w.sum(dtype=np.int64)) == 65536
        assert 2 <= L <= 30 and radius == math.floor(L / 2) + 1 <= 16
        assert shake_ref.valid(w, radius) and q16 == shake_ref.q16_of(w) == shake.q16_of(w)
        assert np.count_nonzero(w) > 1
        cy, cx = (w * ys).sum() / 65536, (w * xs).sum() / 65536
        assert abs(cy) <= 0.5 and abs(cx) <= 0.5
        # every sample lies within L / 2 of the centre: nothing beyond the bilinear footprint of that disc
        assert not w[np.hypot(np.maximum(np.abs(ys) - 1, 0), np.maximum(np.abs(xs) - 1, 0)) > L / 2 + 1e-9].any()
        again = shake._psf.__wrapped__(2.0, 30.0, seed, clip, run)
        assert np.array_equal(again[0], w) and again[1:] == (radius, q16)
        seen.append(w.tobytes())
    assert len(set(seen)) == len(seen)                                  # another run or clip: another table
    assert not np.array_equal(shake.psf("2..30", seed, 0, 0)[0], shake.psf("2..30", seed + 1, 0, 0)[0])
    w, radius, _ = shake.psf("7", seed, 1, 2)
    assert shake.extent("7", seed, 1, 2) == 7.0 and radius == 4


def test_degenerate_trajectory_and_quantiser():
    from speinet_amd import shake
    w, radius, q16 = shake.rasterise([(0.0, 0.0)] * 129, 12.0)
    assert np.array_equal(w, shake_ref.delta()) and radius == 0 and q16 == 65536
    w, radius, q16 = shake.rasterise([(1.5, -2.5)] * 129, 12.0)
    assert np.array_equal(w, shake_ref.delta()) and radius == 0
    # a straight horizontal path of extent 8: a line of taps in the centre row, symmetric
    w, radius, q16 = shake.rasterise([(0.0, float(k)) for k in range(129)], 8.0)
    assert radius == 5 and int(w.sum(dtype=np.int64)) == 65536 and not np.delete(w, 16, axis=0).any()
    assert np.abs(w[16, 12:21].astype(np.int64) - w[16, 12:21][::-1].astype(np.int64)).max() <= 1 and not w[16, :11].any()
    # thirds: 21845 each, the one unit of shortfall to the first in raster order
    a = np.zeros((33, 33))
    a[16, 15:18] = 1.0
    assert shake.quantise(a)[16, 15:18].tolist() == [21846, 21845, 21845]
    a[16, 15:18] = (0.5, 0.25, 0.25)
    assert shake.quantise(a)[16, 15:18].tolist() == [32768, 16384, 16384]
    pts = shake.trajectory(5, 1, 2)
    assert len(pts) == 129 and pts[0] == (0.0, 0.0) and pts == shake.trajectory(5, 1, 2) and pts != shake.trajectory(5, 1, 3)


def test_spec_and_records():
    from speinet_amd import shake
    assert shake.SHAKE_RECORD.itemsize == 16 and shake.SHAKE_RECORD.names == ("psf", "radius", "q16", "reserved")
    assert shake.parse("4") == (4.0, 4.0) and shake.parse("4..24") == (4.0, 24.0) and shake.parse("2..30") == (2.0, 30.0)
    assert shake.parse(None) is None and shake.name(None) is None and shake.name("4..24") == "4.0..24.0" and shake.name(" 4 ") == "4.0"
    for bad in ("1..5", "5..31", "8..4", "", "a", "4..", "4..5..6", "nan", 1.0):
        with pytest.raises(ValueError, match="shake"):
            shake.parse(bad)
    shake.check("srgb", "4..24")
    shake.check("code", None)
    shake.check("gamma:2.2", "4", "single")
    for light_spec in ("code", None):
        with pytest.raises(ValueError, match="--light / --blur_light"):
            shake.check(light_spec, "4..24")
    with pytest.raises(ValueError, match="single"):
        shake.check("srgb", None, "single")
    with pytest.raises(ValueError, match="frames"):
        shake.check("srgb", "4", "pairs")
    runs, labels = np.array([5, 6, 7, 8]), np.array([0, 1, 0, 1])
    rec = shake.records("4..24", 9, 2, runs, labels, base=10)
    tab = shake.psf_table("4..24", 9, 2, runs, labels)
    assert rec.dtype == shake.SHAKE_RECORD and tab.dtype == np.uint32 and tab.shape == (2, 33, 33)
    assert rec["radius"][[1, 3]].tolist() == [0, 0] and rec["q16"][[1, 3]].tolist() == [65536, 65536] and not rec["reserved"].any()
    for i, run in ((0, 5), (1, 7)):
        w, radius, q16 = shake.psf("4..24", 9, 2, run)
        assert np.array_equal(tab[i], w) and tuple(rec[2 * i]) == (10 + i, radius, q16, 0) and radius > 0
    assert shake.psf_table("4", 9, 2, [1, 2], [1, 1]).shape == (0, 33, 33)


def test_plans():
    """plan_dataset is what it was, with and without shake (it takes none); runs mode shakes exactly the label-0 runs; plan_single gives
    lengths 1 and the labels of the draw sequence."""
    import inspect
    from speinet_amd import blurset, shake
    assert "shake" not in inspect.signature(blurset.plan_dataset).parameters
    want = blurset.plan_dataset([40, 33], [0.3, 0.5], 5)
    again = blurset.plan_dataset([40, 33], [0.3, 0.5], 5, frames="runs")
    rng = random.Random(5)
    for n, (r, (s, k, lab)), (r2, (s2, k2, lab2)) in zip((40, 33), want, again):
        ratio = rng.choice([0.3, 0.5])
        s0, k0, lab0 = blurset.plan_runs(n, ratio, rng=rng)
        assert r == r2 == ratio and s.tolist() == s2.tolist() == s0.tolist() and k.tolist() == k2.tolist() == k0.tolist()
        assert lab.tolist() == lab2.tolist() == lab0.tolist()
        rec = shake.records("4..12", 5, 0, np.arange(lab.size), lab)
        assert ((rec["radius"] > 0) == (lab == 0)).all() and (lab == 0).any() and (lab == 1).any()
    rng, mirror = random.Random(8), random.Random(8)
    s, k, lab = blurset.plan_single(25, 0.4, rng)
    assert s.tolist() == list(range(25)) and k.tolist() == [1] * 25 and lab.tolist() == [int(mirror.random() < 0.4) for _ in range(25)]
    assert rng.random() == mirror.random()
    single = blurset.plan_dataset([25, 9], [0.4], 8, frames="single")
    mirror = random.Random(8)
    for n, (r, (s, k, lab)) in zip((25, 9), single):
        assert r == 0.4 and k.tolist() == [1] * n and lab.tolist() == [int(mirror.random() < 0.4) for _ in range(n)]
    with pytest.raises(ValueError):
        blurset.plan_single(5, 0.5)
    with pytest.raises(ValueError):
        blurset.plan_single(0, 0.5, random.Random(0))
    with pytest.raises(ValueError, match="frames"):
        blurset.plan_dataset([5], [0.5], 0, frames="pairs")


def test_sharp_clip_set_carries_its_shake(tmp_path):
    from sharpset_ref import moving_clip, write_sharp
    from speinet_amd import blurset, data, shake
    src = write_sharp(str(tmp_path / "sharp"), {f"clip{c}": moving_clip(c, 30, 40, 40) for c in range(2)})
    plain = data.SharpClipSet(src, references=False, seed=3, light="srgb")
    shaken = data.SharpClipSet(src, references=False, seed=3, light="srgb", shake="4..12")
    assert plain.shake is None and plain.psfs is None and shaken.shake == "4.0..12.0" and "shake" not in plain.summary()
    assert "shake 4.0..12.0 on " in shaken.summary() and plain.frames == shaken.frames == "runs"
    for epoch in (0, 1):
        plain.plan(epoch)
        shaken.plan(epoch)
        base = 0
        for k, (p, q) in enumerate(zip(plain.clips, shaken.clips)):
            assert p["starts"].tolist() == q["starts"].tolist() and p["labels"] == q["labels"] and "shake" not in p
            want = shake.records("4..12", 3 + epoch, k, np.arange(len(q["labels"])), q["labels"], base=base)
            assert np.array_equal(q["shake"], want)
            tab = shake.psf_table("4..12", 3 + epoch, k, np.arange(len(q["labels"])), q["labels"])
            assert np.array_equal(shaken.psfs[base:base + tab.shape[0]], tab)
            base += tab.shape[0]
        assert shaken.psfs.shape == (base, 33, 33)
    single = data.SharpClipSet(src, references=True, seed=3, light="srgb", shake="4", frames="single")
    want = blurset.plan_dataset([30, 30], [0.5], 3, frames="single")
    for c, (_r, (starts, lengths, labels)) in zip(single.clips, want):
        assert c["lengths"].tolist() == [1] * 30 and c["labels"] == labels.tolist() and "frames single" in single.summary()
    items = [(0, single.sample(1), None), (1, single.sample(len(single) - 1), None)]
    rec = data.run_shake_records(single, items)
    assert rec.shape == (2 * 5 + 2,) and rec["radius"][10:].tolist() == [0, 0] and rec["q16"][10:].tolist() == [65536, 65536]
    for b, (_i, s, _d) in enumerate(items):
        runs = list(s.frames) + [s.pre, s.sub]
        assert np.array_equal(rec[5 * b:5 * b + 5], single.clips[s.clip]["shake"][runs])
    for light_spec in ("code", None):
        with pytest.raises(ValueError, match="--light / --blur_light"):
            data.SharpClipSet(src, references=False, light=light_spec, shake="4..12")
    with pytest.raises(ValueError, match="single"):
        data.SharpClipSet(src, references=False, light="srgb", frames="single")
    with pytest.raises(ValueError, match="shake"):
        data.SharpClipSet(src, references=False, light="srgb", shake="1..5")


def test_c_abi_declares_the_entries():
    from speinet_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    assert "uint32_t psf;" in text and "} spei_shake_record;" in text
    for name, after in (("spei_window_mean_shake_u8", "spei_window_mean_noise_u8"), ("spei_train_batch_runs_shake_u8", "spei_train_batch_runs_noise_u8")):
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        _res, base = _lib.SIGNATURES[after]
        assert res is _res and len(args) == len(base) + 5
    assert os.path.exists(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "shake.hip"))


def test_command_lines(capsys):
    from speinet_amd import blurset, fit
    base = ["--dir_data_test", "v", "--save", "s"]
    io = ["--input", "a", "--output", "b"]
    a = blurset.parser().parse_args(io)
    assert a.shake is None and a.frames == "runs"
    a = blurset.parser().parse_args(io + ["--light", "srgb", "--shake", "4..24", "--frames", "single"])
    assert a.shake == "4..24" and a.frames == "single"
    a = fit.parser().parse_args(base + ["--dir_sharp", "a"])
    assert a.blur_shake is None and a.blur_frames == "runs"
    a = fit.parser().parse_args(base + ["--dir_sharp", "a", "--blur_light", "srgb", "--blur_shake", "4", "--blur_frames", "single"])
    assert a.blur_shake == "4" and a.blur_frames == "single"
    for main, argv, text in ((blurset.main, io + ["--shake", "4..24"], "--light"),
                             (blurset.main, io + ["--light", "code", "--shake", "4..24"], "--light"),
                             (blurset.main, io + ["--light", "srgb", "--shake", "1..5"], "--shake"),
                             (blurset.main, io + ["--light", "srgb", "--shake", "5..31"], "--shake"),
                             (blurset.main, io + ["--light", "srgb", "--shake", "8..4"], "--shake"),
                             (blurset.main, io + ["--light", "srgb", "--frames", "single"], "--shake"),
                             (blurset.main, io + ["--light", "srgb", "--shake", "4", "--frames", "pairs"], "--frames"),
                             (fit.main, base + ["--dir_sharp", "a", "--blur_shake", "4..24"], "--blur_light"),
                             (fit.main, base + ["--dir_sharp", "a", "--blur_light", "srgb", "--blur_shake", "1..5"], "--blur_shake"),
                             (fit.main, base + ["--dir_sharp", "a", "--blur_light", "srgb", "--blur_frames", "single"], "--blur_shake"),
                             (fit.main, base + ["--dir_data", "a", "--blur_shake", "4..24"], "--dir_sharp"),
                             (fit.main, base + ["--dir_data", "a", "--blur_frames", "single"], "--dir_sharp")):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert e.value.code == 2 and text in capsys.readouterr().err, argv
