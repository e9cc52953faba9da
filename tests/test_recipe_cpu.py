"""speinet_amd.recipe on the host: one table of recipes, valid and invalid, through every front end — Recipe.of, blurset.write_dataset,
data.SharpClipSet, blurset.main and fit.main — which must accept or refuse the same rows, the library ones with the identical message,
the command lines naming the offending flag with their own prefix; canonical form, equality and immutability; and the per-clip draws
of SharpClipSet.plan and write_dataset against the per-module functions."""
import contextlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from sharpset_ref import moving_clip, write_sharp      # noqa: E402

NOISE, SHAKE, CODEC = "1e-3..1e-2:2e-3", "4..12", "30..90"
# (the recipe's keywords, the field a refusal names or None for a valid recipe)
ROWS = [({"noise": NOISE}, "noise"),                                             # noise on code
        ({"shake": SHAKE}, "shake"),                                             # shake on code
        ({"light": None, "shake": SHAKE}, "shake"),                              # ... and on None, which is code
        ({"light": "srgb", "frames": "single"}, "frames"),                       # single without shake
        ({"light": "srgb", "shake": "1..5"}, "shake"),
        ({"light": "srgb", "shake": "5..31"}, "shake"),
        ({"light": "srgb", "shake": "8..4"}, "shake"),
        ({"codec": "0"}, "codec"),
        ({"codec": "101"}, "codec"),
        ({"light": "srgb", "codec": "90..30"}, "codec"),
        ({"light": "linear"}, "light"),
        ({"light": "gamma:2.8"}, "light"),                                       # a light without valid tables
        ({"light": "srgb", "noise": "0.06:0"}, "noise"),                         # above the caps
        ({"light": "srgb", "noise": "1e-3:0.2"}, "noise"),
        ({}, None),
        ({"light": "srgb"}, None),
        ({"light": "gamma:2.2", "noise": NOISE}, None),
        ({"light": "srgb", "shake": SHAKE}, None),
        ({"light": "srgb", "shake": "6", "frames": "single"}, None),
        ({"codec": CODEC}, None),
        ({"light": "srgb", "noise": NOISE, "shake": SHAKE, "codec": CODEC}, None),
        ({"light": "srgb", "noise": NOISE, "shake": SHAKE, "codec": CODEC, "frames": "single"}, None)]
IDS = ["-".join(f"{k}={v}" for k, v in kw.items()) or "reference" for kw, _ in ROWS]


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("recipe")
    os.makedirs(root / "empty")
    return {"empty": str(root / "empty"), "out": str(root / "out"),
            "sharp": write_sharp(str(root / "sharp"), {f"clip{c}": moving_clip(c, 30, 24, 32) for c in range(2)})}


def _flags(kw, prefix):
    return [w for k, v in kw.items() if v is not None for w in (f"--{prefix}{k}", v)]


@pytest.mark.parametrize("kw,field", ROWS, ids=IDS)
def test_every_front_end_takes_or_refuses_the_same_rows(kw, field, dirs, capsys):
    from speinet_amd import blurset, data, fit
    from speinet_amd.recipe import Recipe
    lines = ((blurset.main, ["--input", dirs["empty"], "--output", dirs["out"]] + _flags(kw, ""), ""),
             (fit.main, ["--dir_data_test", "v", "--save", "s", "--dir_sharp", dirs["empty"]] + _flags(kw, "blur_"), "blur_"))
    if field is None:
        recipe = Recipe.of(**kw)
        assert recipe == Recipe(**kw) and data.SharpClipSet(dirs["sharp"], references=False, **kw).recipe == recipe
        with pytest.raises(ValueError, match="no clip folder"):                  # accepted: it stops at the empty directory
            blurset.write_dataset(dirs["empty"], dirs["out"], ratio=0.5, **kw)
        for main, argv, _prefix in lines:
            with pytest.raises(ValueError, match="no clip folder"):
                main(argv)
        return
    with pytest.raises(ValueError) as e:
        Recipe.of(**kw)
    text = str(e.value)
    assert e.value.field == field
    for front in (lambda: blurset.write_dataset(dirs["empty"], dirs["out"], ratio=0.5, **kw),
                  lambda: data.SharpClipSet(dirs["sharp"], references=False, **kw)):
        with pytest.raises(ValueError) as e:
            front()
        assert str(e.value) == text
    for main, argv, prefix in lines:
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert e.value.code == 2 and f"error: --{prefix}{field}: {text}" in capsys.readouterr().err, argv
    assert not os.path.exists(dirs["out"])


def test_dir_data_names_every_flag_that_is_not_the_reference(capsys):
    from speinet_amd import fit
    base = ["--dir_data_test", "v", "--save", "s", "--dir_data", "a"]
    for kw in ({"light": "srgb"}, {"frames": "single"}, {"light": "srgb", "noise": NOISE, "shake": SHAKE, "codec": CODEC}):
        with pytest.raises(SystemExit) as e:
            fit.main(base + _flags(kw, "blur_"))
        err = capsys.readouterr().err.split("error: ")[1]
        assert e.value.code == 2 and "--dir_sharp" in err and "(--dir_data) holds its blur already" in err
        assert all(f"--blur_{k} {v}" in err and f"--{k}" in err.split("speinet_amd.blurset")[1] for k, v in kw.items())
        assert not any(f"--blur_{k}" in err for k in ("light", "noise", "shake", "frames", "codec") if k not in kw)


def test_canonical_equal_and_immutable():
    from speinet_amd import codec, light, shake
    from speinet_amd.recipe import Recipe
    assert Recipe() == Recipe.of() == ("code", None, None, "runs", None) and Recipe(None) == Recipe("code")
    loose = Recipe.of("gamma:2.20", " 1.0e-3..1e-2 : 2e-3", " 4..12 ", "runs", " 30..90 ")
    assert loose == Recipe("gamma:2.2", "0.001..0.01:0.002", "4.0..12.0", "runs", "30..90") and hash(loose) == hash(Recipe(*loose))
    assert loose == (light.name("gamma:2.20"), light.noise_name(" 1.0e-3..1e-2 : 2e-3"), shake.name(" 4..12 "), "runs", codec.name(" 30..90 "))
    assert Recipe(light="srgb", codec=75).codec == "75" and Recipe("srgb", shake=6).shake == "6.0"
    assert loose != Recipe("gamma:2.2") and len({loose, Recipe(*loose), Recipe()}) == 2
    for spelt in (" SRGB ", "sRGB", " srgb"):                                    # a spelling light.name refuses is refused here alike
        with pytest.raises(ValueError) as want:
            light.name(spelt)
        with pytest.raises(ValueError) as got:
            Recipe.of(spelt)
        assert str(got.value) == str(want.value)
    for field in Recipe._fields:
        with pytest.raises(AttributeError):
            setattr(loose, field, "srgb")
    with pytest.raises(AttributeError):
        loose.extra = 1
    assert Recipe().describe() == "light code"
    assert loose.describe() == "light gamma:2.2, noise 0.001..0.01:0.002, shake 4.0..12.0, codec 30..90"
    assert loose.describe(shake=lambda: "S", codec=lambda: "C") == "light gamma:2.2, noise 0.001..0.01:0.002, shake S, codec C"


def test_the_draws_of_a_clip_are_the_modules(dirs, monkeypatch):
    """With every stage on, SharpClipSet.plan(e) carries per clip k what light.noise_draw / noise_levels, shake.records / psf_table and
    codec.quality give for (seed + e, k), and write_dataset hands synthesize_chunks ClipNoise, ClipShake and ClipCodec of the same
    (spec, seed, k) and reports the same levels and quality."""
    from speinet_amd import blurset, codec, data, light, shake
    from speinet_amd.recipe import Recipe
    kw = {"light": "srgb", "noise": NOISE, "shake": SHAKE, "codec": CODEC}
    recipe = Recipe.of(**kw)
    seed = 3
    cs = data.SharpClipSet(dirs["sharp"], ratios=(0.5,), seed=seed, references=False, **kw)
    assert (cs.light, cs.noise, cs.shake, cs.frames, cs.codec) == tuple(recipe)
    for e in (0, 1, 2):
        cs.plan(e)
        tables, n_psf = [], 0
        for k, clip in enumerate(cs.clips):
            ids, labels = np.arange(clip["T"]), clip["labels"]
            assert clip["noise"] == light.noise_draw(recipe.noise, seed + e, k) + light.noise_levels(recipe.noise, seed + e, k)
            assert np.array_equal(clip["shake"], shake.records(recipe.shake, seed + e, k, ids, labels, base=n_psf))
            assert clip["quality"] == codec.quality(recipe.codec, seed + e, k)
            tables.append(shake.psf_table(recipe.shake, seed + e, k, ids, labels))
            n_psf += tables[-1].shape[0]
        assert n_psf > 0 and np.array_equal(cs.psfs, np.concatenate(tables))
        draws = [recipe.clip(seed + e, k) for k in range(len(cs.clips))]
        assert [d.noise for d in draws] == [c["noise"] for c in cs.clips] and [d.quality for d in draws] == [c["quality"] for c in cs.clips]
    seen = []

    def record(fr, runs, dev, gray, chunk_frames, light, noise, shake, codec):      # synthesize_chunks' spelling; no frame is made
        seen.append((light, noise, shake, codec))
        return iter(())

    monkeypatch.setattr(blurset, "synthesize_chunks", record)
    monkeypatch.setattr(blurset.torch.cuda, "device", lambda dev: contextlib.nullcontext())
    lines = []
    done = blurset.write_dataset(dirs["sharp"], dirs["out"] + "_draws", ratio=0.5, seed=seed, log=lines.append, **kw)
    assert seen == [("srgb", light.ClipNoise(recipe.noise, seed, k), shake.ClipShake(recipe.shake, seed, k), codec.ClipCodec(recipe.codec, seed, k))
                    for k in range(2)]
    for k, (d, line) in enumerate(zip(done, lines)):
        assert (d["shot"], d["read"]) == light.noise_draw(recipe.noise, seed, k) and d["quality"] == codec.quality(recipe.codec, seed, k)
        assert line.endswith(f"(ratio 0.5, light srgb, noise shot {d['shot']:.3g} read {d['read']:.3g}, shake 4.0..12.0 on "
                             f"{int((d['labels'] == 0).sum())} frames, codec quality {d['quality']})")
    seen.clear()
    blurset.write_dataset(dirs["sharp"], dirs["out"] + "_plain", ratio=0.5, seed=seed)
    assert seen == [("code", None, None, None)] * 2
