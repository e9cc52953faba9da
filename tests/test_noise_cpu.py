"""Sensor noise of blur synthesis on the host: the generator's known answers, the gauss table, the statistics of the deviates and of
the noise step on the numpy restatement tests/noise_ref.py, speinet_amd.light's levels and parser, the command lines, and that the plan
is untouched.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import light_ref  # noqa: E402
import noise_ref  # noqa: E402
from noise_ref import S  # noqa: E402

VECTORS = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def test_philox_known_answers():
    """Philox4x32-10's published vectors, on the restatement's generator and on speinet_amd.light's (the host's draws)."""
    from speinet_amd import light
    for ctr, k, want in VECTORS:
        got = noise_ref.philox(*ctr, *k)
        assert " ".join("%08x" % int(w) for w in got) == want
        assert " ".join("%08x" % w for w in light.philox(ctr, k)) == want
    # vectorised == one at a time, and the key of a seed
    x = np.arange(5)
    many = noise_ref.philox(x, 7, 3, 1, *noise_ref.key((9 << 32) | 5))
    assert noise_ref.key((9 << 32) | 5) == (5, 9) == light.key_of((9 << 32) | 5)
    for i in range(5):
        assert [int(w[i]) for w in many] == list(light.philox((i, 7, 3, 1), (5, 9)))


def test_gauss_table():
    from speinet_amd import light
    t = light.gauss_table()
    assert t.dtype == np.int32 and t.shape == (1025,) and np.array_equal(t.astype(np.int64), noise_ref.GAUSS)
    assert light.gauss_valid(t) and noise_ref.gauss_valid(noise_ref.GAUSS)
    assert np.all(np.diff(noise_ref.GAUSS) > 0) and np.array_equal(noise_ref.GAUSS, -noise_ref.GAUSS[::-1])
    assert noise_ref.GAUSS[512] == 0 and np.abs(noise_ref.GAUSS).max() == 15025
    bad = t.copy()
    bad[100] = bad[99]
    assert not light.gauss_valid(bad) and not light.gauss_valid(t[:-1]) and not light.gauss_valid(np.where(np.arange(1025) == 0, -2 ** 15, t))


def test_deviates_are_standard_normal():
    """2^20 pixels (x, y < 1024) of one frame: mean, deviation, fourth moment of z / 4096 and its correlations along x and between
    channels.  The standard error of each is about 0.001; the bounds are conditions several errors wide."""
    from speinet_amd import light
    z = noise_ref.z_of(noise_ref.words(1024, 1024, 3, 1, 12345), light.gauss_table().astype(np.int64)) / 4096.0
    mean, std = float(z.mean()), float(z.std())
    m4 = float((((z - mean) / std) ** 4).mean())
    u = (z - mean) / std
    lag = [float((u[:, :-1, c] * u[:, 1:, c]).mean()) for c in range(3)]
    cross = [float((u[..., a] * u[..., b]).mean()) for a, b in ((0, 1), (0, 2), (1, 2))]
    print(f"mean {mean:.4f} std {std:.4f} m4 {m4:.4f} lag-1 {lag} channels {cross}")
    assert abs(mean) < 0.005 and abs(std - 1) < 0.005 and abs(m4 - 3) < 0.05
    assert max(abs(v) for v in lag + cross) < 0.01


def test_flat_run_has_the_stated_deviation():
    """n = 7, L = 0.2 S, a = 1e-3, r = 2e-3: std(d) / S within 1 % of sqrt((a 0.2 + r^2) 6 / 7) = 0.013223."""
    from speinet_amd import light
    a, r, n = 1e-3, 2e-3, 7
    A, B = light.noise_levels(f"{a}:{r}", 0, 0)
    assert (A, B) == noise_ref.levels(a, r)
    L = np.full((512, 512, 3), int(0.2 * S), np.int64)
    out = noise_ref.apply(L, noise_ref.z_of(noise_ref.words(512, 512, 0, 0, 1)), A, B, n)
    got = float((out - L).std()) / S
    want = float(np.sqrt((a * 0.2 + r * r) * 6 / 7))
    print(f"std(d) / S = {got:.6f}, expected {want:.6f}")
    assert abs(want - 0.013223) < 1e-6 and abs(got / want - 1) < 0.01
    assert out.min() > 0 and out.max() < S                                  # nothing was clamped


def test_noise_levels():
    from speinet_amd import light
    for a, r in ((1e-3, 2e-3), (0.0, 0.0), (0.05, 0.1), (0.0123, 0.0)):
        A, B = light.noise_levels(f"{a}:{r}", 5, 2)
        assert (A, B) == (int(np.rint(a * S)), int(np.rint(r * r * float(S) * float(S)))) == noise_ref.levels(a, r)
        assert A < 2 ** 20 and B < 2 ** 42
        assert light.noise_levels(f"{a}:{r}", 6, 3) == (A, B)              # a fixed spec is the same for every clip and seed
    spec = "1e-4..1e-2:1e-3..5e-2"
    seen = {}
    for seed in (0, 1, (1 << 32) + 1):
        for clip in range(6):
            a, r = light.noise_draw(spec, seed, clip)
            assert 1e-4 <= a <= 1e-2 and 1e-3 <= r <= 5e-2
            assert light.noise_draw(spec, seed, clip) == (a, r)            # deterministic
            assert light.noise_levels(spec, seed, clip) == noise_ref.levels(a, r)
            w = [int(v) for v in noise_ref.philox(0xffffffff, 0xffffffff, 0, clip, *noise_ref.key(seed))]
            assert a == pytest.approx(1e-4 * 100 ** (w[0] / 2.0 ** 32), rel=1e-12) and r == pytest.approx(1e-3 * 50 ** (w[1] / 2.0 ** 32), rel=1e-12)
            seen[seed, clip] = (a, r)
    assert len(set(seen.values())) == len(seen)                             # differs between clips and between seeds
    a, r = light.noise_draw("2e-3:1e-3..5e-2", 0, 0)                        # one side fixed, one drawn
    assert a == 2e-3 and r == seen[0, 0][1]
    assert light.noise_draw("3e-3..3e-3:0", 4, 1) == (3e-3, 0.0)


def test_parser():
    from speinet_amd import light
    assert light.parse_noise(None) is None and light.noise_name(None) is None
    assert light.parse_noise("1e-3:2e-3") == ((1e-3, 1e-3), (2e-3, 2e-3))
    assert light.parse_noise("1e-3..1e-2:0") == ((1e-3, 1e-2), (0.0, 0.0))
    assert light.noise_name("1.0e-3..0.010:0.0020") == "0.001..0.01:0.002" and light.noise_name("0:0") == "0.0:0.0"
    assert light.noise_name(light.noise_name("1e-3..1e-2:2e-3..3e-3")) == light.noise_name("1e-3..1e-2:2e-3..3e-3")
    for bad in ("", "1e-3", "1e-3:2e-3:3", "x:1e-3", "1e-3:y", "nan:0", "0.06:0", "0:0.11", "-1e-3:0", "0:-1e-3",      # out of range
                "1e-2..1e-3:0", "0:5e-2..1e-3",                                                                      # lo > hi
                "0..1e-3:0", "0:0..1e-3", "0.0..0.0:0",                                                              # lo = 0 in a range
                "1e-3..0.06:0", "0:1e-3..0.2", "1e-3..x:0", 0.001):
        with pytest.raises(ValueError, match="noise"):
            light.parse_noise(bad)
    # `code` plus noise: a ValueError that names --light / --blur_light
    for light_spec in ("code", None):
        with pytest.raises(ValueError, match="--light / --blur_light"):
            light.check_noise(light_spec, "1e-3:2e-3")
    light.check_noise("srgb", "1e-3:2e-3")
    light.check_noise("code", None)
    with pytest.raises(ValueError, match="noise"):
        light.check_noise("srgb", "1:1")


def test_command_lines(capsys):
    from speinet_amd import blurset, fit
    base = ["--dir_data_test", "v", "--save", "s"]
    assert blurset.parser().parse_args(["--input", "a", "--output", "b"]).noise is None
    assert blurset.parser().parse_args(["--input", "a", "--output", "b", "--light", "srgb", "--noise", "1e-3:2e-3"]).noise == "1e-3:2e-3"
    assert fit.parser().parse_args(base + ["--dir_sharp", "a"]).blur_noise is None
    assert fit.parser().parse_args(base + ["--dir_sharp", "a", "--blur_noise", "1e-3..1e-2:0"]).blur_noise == "1e-3..1e-2:0"
    for main, argv, text in ((blurset.main, ["--input", "a", "--output", "b", "--noise", "1e-3:2e-3"], "--light"),
                             (blurset.main, ["--input", "a", "--output", "b", "--light", "code", "--noise", "1e-3:2e-3"], "--light"),
                             (blurset.main, ["--input", "a", "--output", "b", "--light", "srgb", "--noise", "0.06:0"], "--noise"),
                             (blurset.main, ["--input", "a", "--output", "b", "--light", "srgb", "--noise", "1e-2..1e-3:0"], "lo <= hi"),
                             (fit.main, base + ["--dir_sharp", "a", "--blur_noise", "1e-3:2e-3"], "--blur_light"),
                             (fit.main, base + ["--dir_sharp", "a", "--blur_light", "srgb", "--blur_noise", "0..1e-3:0"], "--blur_noise"),
                             (fit.main, base + ["--dir_data", "a", "--blur_noise", "1e-3:2e-3"], "--dir_sharp")):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert e.value.code == 2 and text in capsys.readouterr().err, argv


def test_the_plan_is_untouched(tmp_path):
    """plan_dataset takes no noise and SharpClipSet's runs are the same with and without it; the levels follow the plan's seed."""
    import inspect
    from sharpset_ref import moving_clip, write_sharp
    from speinet_amd import blurset, data, light
    assert "noise" not in inspect.signature(blurset.plan_dataset).parameters
    src = write_sharp(str(tmp_path / "sharp"), {f"clip{c}": moving_clip(c, 30, 40, 40) for c in range(2)})
    plain = data.SharpClipSet(src, references=False, seed=3, light="srgb")
    noisy = data.SharpClipSet(src, references=False, seed=3, light="srgb", noise="1.0e-3..1e-2:2e-3")
    assert plain.noise is None and noisy.noise == "0.001..0.01:0.002" and plain.noise_lines() == []
    assert plain.summary().endswith("light srgb") and noisy.summary().endswith("light srgb, noise 0.001..0.01:0.002")
    for epoch in (0, 1):
        plain.plan(epoch)
        noisy.plan(epoch)
        want = blurset.plan_dataset([30, 30], [0.5], 3 + epoch)
        for k, (p, q, (_r, (starts, lengths, labels))) in enumerate(zip(plain.clips, noisy.clips, want)):
            assert p["starts"].tolist() == q["starts"].tolist() == starts.tolist() and p["lengths"].tolist() == q["lengths"].tolist()
            assert p["labels"] == q["labels"] == labels.tolist() and "noise" not in p
            assert q["noise"] == light.noise_draw(noisy.noise, 3 + epoch, k) + light.noise_levels(noisy.noise, 3 + epoch, k)
        assert len(noisy.noise_lines()) == 2 and noisy.noise_lines()[0].startswith("> clip0: noise shot ")
    for light_spec in ("code", None):
        with pytest.raises(ValueError, match="--light / --blur_light"):
            data.SharpClipSet(src, references=False, light=light_spec, noise="1e-3:2e-3")
    with pytest.raises(ValueError, match="noise"):
        data.SharpClipSet(src, references=False, light="srgb", noise="1:1")


def test_identities_on_the_restatement():
    """A run of length 1 returns its bytes; A = B = 0 returns the light's bytes; a non-zero level changes them."""
    from speinet_amd import light
    rs = np.random.RandomState(5)
    frames = rs.randint(0, 256, (15, 9, 7, 3)).astype(np.uint8)
    assert light.noise_levels("0:0", 9, 1) == (0, 0) and light.noise_levels("1e-3:2e-3", 9, 1) == noise_ref.levels(1e-3, 2e-3)
    for spec in ("srgb", "gamma:2.2"):
        for start in (0, 14):
            assert np.array_equal(noise_ref.run_mean(frames[start:start + 1], spec, 2, 1, 9, 1000, 10 ** 9), frames[start])
        for n in (2, 7, 15):
            assert np.array_equal(noise_ref.run_mean(frames[:n], spec, 2, 1, 9, 0, 0), light_ref.run_mean(frames[:n], spec))
            noisy = noise_ref.run_mean(frames[:n], spec, 2, 1, 9, *noise_ref.levels(1e-3, 2e-3))
            assert not np.array_equal(noisy, light_ref.run_mean(frames[:n], spec))
            assert not np.array_equal(noisy, noise_ref.run_mean(frames[:n], spec, 3, 1, 9, *noise_ref.levels(1e-3, 2e-3)))
    assert [int(v) for v in noise_ref.isqrt(np.array([0, 1, 3, 4, 10 ** 12 - 1, 10 ** 12, 2 ** 45 - 1]))] == [0, 1, 1, 2, 999999, 10 ** 6, 5931641]
