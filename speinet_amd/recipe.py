"""The blur-synthesis recipe, stated once: the light the runs are averaged in and the stages on top of the average.

    light   "code" (the reference's average of code values), "srgb" or "gamma:<g>" (linear light)        speinet_amd.light
    noise   None, or "<shot>:<read>": sensor noise in the linear light, levels drawn per clip            speinet_amd.light
    shake   None, or "<len>" / "<lo>..<hi>": a camera-shake PSF per frame labelled blurry, linear light  speinet_amd.shake
    frames  "runs" (runs of 1..15 frames are averaged) or "single" (every frame its own run; needs shake)
    codec   None, or "<q>" / "<lo>..<hi>": a JPEG-style round trip of every blur frame, any light         speinet_amd.codec

`Recipe` validates and canonicalises the five; `Recipe()` is the reference's path.  Everything else here is the one copy of what the
front ends share: the command-line options (`add_arguments`, `from_args`: `blurset` without a prefix, `fit` with `blur_`), the draws
of one clip (`Recipe.clip` -> `Clip`: `blurset.write_dataset` and `data.SharpClipSet.plan` take the same quantities from it) and the
text of a log line (`Recipe.describe`).  The arithmetic stays in the three modules above."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import codec as _codec
from . import light as _light
from . import shake as _shake

FIELDS = ("light", "noise", "shake", "frames", "codec")
STAGES = ("noise", "shake", "codec")


class Recipe(namedtuple("Recipe", FIELDS)):
    """An immutable (light, noise, shake, frames, codec) in canonical spelling — what `light.name`, `light.noise_name`, `shake.name` and
    `codec.name` return.  Constructing one is the validation: a ValueError carries the offending field's name as `field`."""
    __slots__ = ()

    def __new__(cls, light="code", noise=None, shake=None, frames="runs", codec=None):
        field = "light"
        try:
            light = _light.name(light)
            if light != _light.CODE:
                _light.tables(light)                          # a light without valid tables
            field = "noise"
            _light.check_noise(light, noise)                  # a spec that does not parse, noise on code values
            noise = _light.noise_name(noise)
            field = "shake" if shake is not None and frames in _shake.FRAMES else "frames"
            _shake.check(light, shake, frames)                # ... shake on code values, `single` without shake
            shake = _shake.name(shake)
            field = "codec"
            codec = _codec.name(codec)
        except ValueError as e:
            e.field = field
            raise
        return super().__new__(cls, light, noise, shake, frames, codec)

    of = classmethod(lambda cls, *a, **kw: cls(*a, **kw))

    def clip(self, seed: int, clip: int, first_run: int = 0) -> "Clip":
        """The draws of clip number `clip` under `seed`, every stage keyed alike."""
        return Clip(self, {s: (seed, clip, first_run) for s in STAGES})

    def describe(self, **say) -> str:
        """"light <light>" and ", <stage> <text>" per active stage: the stage's spec, or `say[stage]()` where the caller has more to say."""
        return f"light {self.light}" + "".join(f", {s} {say[s]() if s in say else getattr(self, s)}" for s in STAGES
                                               if getattr(self, s) is not None)


class Clip:
    """What a recipe draws for one clip: each active stage under its own (seed, clip, first run id) — `blurset.synthesize`'s
    `light.ClipNoise`, `shake.ClipShake` and `codec.ClipCodec` minus their specs, which are the recipe's."""

    def __init__(self, recipe: Recipe, keys: dict):
        self.recipe, self.keys = recipe, {s: k for s, k in keys.items() if getattr(recipe, s) is not None}

    @classmethod
    def of(cls, light="code", noise=None, shake=None, codec=None) -> "Clip":
        """From `synthesize`'s keywords: a light and per stage None or its (spec, seed, clip[, first_run])."""
        given = {"noise": noise and _light.ClipNoise(*noise), "shake": shake and _shake.ClipShake(*shake), "codec": codec and _codec.ClipCodec(*codec)}
        specs = {s: t and t.spec for s, t in given.items()}
        return cls(Recipe(light, **specs), {s: (t.seed, t.clip, getattr(t, "first_run", 0)) for s, t in given.items() if t})

    def stages(self) -> dict:
        """`synthesize`'s keywords back."""
        made = {"noise": _light.ClipNoise, "shake": _shake.ClipShake, "codec": _codec.ClipCodec}     # a ClipCodec has no first run
        return {"light": self.recipe.light, **{s: None for s in STAGES},
                **{s: made[s](getattr(self.recipe, s), *k[:len(made[s]._fields) - 1]) for s, k in self.keys.items()}}

    @property
    def noise(self):
        """(a, r, A, B): the clip's shot coefficient and read deviation and their integer levels; None without noise."""
        if "noise" not in self.keys:
            return None
        seed, clip, _ = self.keys["noise"]
        return _light.noise_draw(self.recipe.noise, seed, clip) + _light.noise_levels(self.recipe.noise, seed, clip)

    def noise_records(self, runs):
        """(NOISE_RECORD per run of `runs`, counted from the first run handed over; the seed that keys the generator); None without noise."""
        if "noise" not in self.keys:
            return None
        seed, clip, first = self.keys["noise"]
        return _light.noise_records(np.asarray(runs) + first, clip, *self.noise[2:]), seed

    def shake(self, runs, labels, base: int = 0):
        """(SHAKE_RECORD per run, their uint32 [n,33,33] PSFs; the records index them from `base`): one PSF per run labelled 0; None
        without shake."""
        if "shake" not in self.keys:
            return None
        seed, clip, first = self.keys["shake"]
        ids = np.asarray(runs) + first
        return (_shake.records(self.recipe.shake, seed, clip, ids, labels, base=base),
                _shake.psf_table(self.recipe.shake, seed, clip, ids, labels))

    @property
    def quality(self):
        """The clip's one JPEG quality; None without a codec."""
        if "codec" not in self.keys:
            return None
        seed, clip, _ = self.keys["codec"]
        return _codec.quality(self.recipe.codec, seed, clip)

    def drawn(self) -> dict:
        """What a report says of the clip: `shot` and `read` with noise, `quality` with a codec."""
        noise, quality = self.noise, self.quality
        return {**({} if noise is None else {"shot": noise[0], "read": noise[1]}), **({} if quality is None else {"quality": quality})}


# ---- the command line ----

_HELP = {"light": "the light the runs are averaged in: code (code values, the reference's sets), srgb or gamma:<g> (linear light, as an "
                  "exposure; speinet_amd.light)",
         "noise": "sensor noise added in the linear --{p}light: <shot>:<read>, the shot coefficient (at most 0.05) and the read deviation (at "
                  "most 0.1) at full scale 1, each a number or lo..hi (drawn log-uniformly per clip); not fitted to any camera",
         "shake": "camera-shake blur applied in the linear --{p}light to the frames labelled blurry: the blur extent in pixels, <len> or "
                  "<lo>..<hi> within 2..30 (one trajectory PSF is drawn per frame); not fitted to any camera (speinet_amd.shake)",
         "frames": "runs: average runs of 1..15 frames (high-frame-rate footage); single: every frame is its own output frame, shaken unless "
                   "drawn steady with probability --{p}ratio (ordinary footage; needs --{p}shake)",
         "codec": "JPEG-style codec artefacts on every blur frame (never on the ground truth), as the last step: the quality, <q> or "
                  "<lo>..<hi> within 1..100 (one is drawn per clip); goes with any --{p}light; untuned (speinet_amd.codec)"}


def add_arguments(parser, prefix: str = "", note: str = "") -> None:
    """The recipe's five options `--<prefix>light` .. `--<prefix>codec`, defaults `Recipe()`'s; `note` opens every help text."""
    for field, default in zip(FIELDS, Recipe()):
        parser.add_argument(f"--{prefix}{field}", default=default, help=note + _HELP[field].format(p=prefix),
                            **({"choices": _shake.FRAMES} if field == "frames" else {}))


def from_args(parser, args, prefix: str = "") -> Recipe:
    """The recipe of a parsed namespace; a refusal goes through `parser.error`, naming the flag."""
    try:
        return Recipe(*(getattr(args, prefix + f) for f in FIELDS))
    except ValueError as e:
        parser.error(f"--{prefix}{e.field}: {e}")
