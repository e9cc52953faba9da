"""The light a run of sharp frames is averaged in (blurset.py, data.SharpTrainLoader; csrc/light.h).

The reference's data-set scripts average code values: the gamma-encoded bytes.  That is the light `code`, the default, and it selects
the kernels that sum bytes.  A sensor integrates LIGHT and applies its transfer curve afterwards, so an exposure over a black / white
edge is far brighter than mid-gray; the GoPro set's `blur_gamma` variant is made that way, through an inverse gamma 2.2 curve (Nah et
al., CVPR 2017).  A light other than `code` does the same in integer arithmetic, defined bit for bit:

    spec      "code" | "srgb" | "gamma:<g>"
    f         the forward transfer, code value in [0, 1] -> linear light in [0, 1]:
              srgb      IEC 61966-2-1: c / 12.92 for c <= 0.04045, else ((c + 0.055) / 1.055) ** 2.4
              gamma:g   c ** g
    S         2 ** 24 - 1
    lin[c]    rint(S * f(c / 255)), c = 0..255              the linear value of code c
    thr[c]    rint(S * f((c - 0.5) / 255)), c = 1..255      the linear value of the boundary between codes c - 1 and c; thr[0] = 0

both tables built here, once, in float64.  Per byte position of a run of n frames (1..15):

    L    = floor(sum of lin[byte] over the run / n)
    blur = #{c in 1..255 : thr[c] <= L}                      the largest code whose lower boundary is at or below L

A pair of tables is VALID iff lin[0] == 0, lin[255] <= S and lin[c - 1] < thr[c] <= lin[c] for c = 1..255.  Then both increase
strictly and encode(lin[c]) == c: a run of length 1, or of identical frames, returns its bytes, which the ground-truth records rely
on.  No range of gamma is written down anywhere: the tables are validated (`gamma:2.8` fails, its thr[1] rounds to 0), here and again
by the C entry points on the host copy they are handed.

`srgb` and `gamma:2.2` are the conventional approximations of a camera curve that is not known; no model has been trained here on
either.

SENSOR NOISE (opt-in; `noise=` / `--noise` / `--blur_noise`).  The mean of n frames carries 1 / n of one frame's noise variance, so a
long run comes out almost noise-free where a real exposure has the noise of any other frame.  With a noise spec the variance that the
average lost is added back in linear light, between the average and the encode, again bit for bit in integers.  Noise needs a linear
light: `code` plus noise is a ValueError.

    words     Philox4x32-10 (Salmon et al., SC'11): multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85, ten
              rounds.  For the pixel at column x, row y of the full source frame (before any crop, flip or rotation) of output frame
              `run` of clip `clip`: counter (x, y, run, clip), key (seed & 0xffffffff, (seed >> 32) & 0xffffffff); output words 0, 1, 2
              serve the R, G and B bytes, word 3 is unused.  Nothing depends on launch geometry, chunking, crop position or augmentation.
    t[i]      round(4096 * statistics.NormalDist().inv_cdf(min(max(i / 1024, 2^-13), 1 - 2^-13))), i = 0..1024     (`gauss_table`)
              VALID iff strictly increasing and |t[i]| < 2^15.
    z         for a word w: i = w >> 22, f = (w >> 10) & 4095, z = (t[i] (4096 - f) + t[i + 1] f + 2048) >> 12   (arithmetic shift, Q12)
    V         floor((A L + B) (n - 1) / n)            per byte, with L as above and the clip's integers A < 2^20, B < 2^42
    sigma     isqrt(V)
    d         (sigma z + 2048) >> 12
    L'        clamp(L + d, 0, S);   blur = encode(L')

(n - 1) / n tops the average's noise up to the level of ONE source frame, so a run of length 1 — every ground-truth record — has d = 0
and still returns its bytes.  The gray plane is that of the noisy encoded bytes; a `zero` record stays zero.

    levels    one shot coefficient a and one read deviation r per clip: full scale 1, variance a x + r^2; 0 <= a <= 0.05, 0 <= r <= 0.1;
              A = rint(a S), B = rint(r^2 S^2)
    spec      "<shot>:<read>", each side a number or "lo..hi" with 0 < lo <= hi: a range is drawn log-uniformly per clip and per seed,
              on the host: w = philox((0xffffffff, 0xffffffff, 0, clip), key), a = lo (hi / lo) ** (w0 / 2^32), r likewise from w1.
    ids       clip: the clip's index in blurset.clip_folders order (SharpClipSet's `source`); run: the run's index in the clip's plan,
              the number in the six-digit file name, global across synthesize_chunks' chunks; seed: write_dataset's, seed + e in epoch e.

The plan's random.Random stream is not touched: plan_dataset's output is the same with and without noise.  One level per clip, not
one per frame: a clip is shot at one gain.  The levels are NOT fitted to any camera, and no model has been trained with them here.

CAMERA SHAKE (opt-in; `shake=` / `--shake` / `--blur_shake`) correlates L with a point-spread function between the average and the
noise, and generalises V to X - ceil(X q16 / (n 2^16)): speinet_amd/shake.py has that contract.
"""
from __future__ import annotations

import math
import statistics
import threading
from collections import namedtuple
from typing import Optional, Tuple

import numpy as np

S = 2 ** 24 - 1
CODE = "code"

MAX_SHOT, MAX_READ = 0.05, 0.1
GAUSS_WORDS = 1025
# spei_noise_record
NOISE_RECORD = np.dtype([("run", "<u4"), ("clip", "<u4"), ("A", "<u4"), ("reserved", "<u4"), ("B", "<u8")])
assert NOISE_RECORD.itemsize == 24
# the noise of one clip for blurset.synthesize: its spec, write_dataset's seed, the clip's index and the id of the first run handed over
ClipNoise = namedtuple("ClipNoise", "spec seed clip first_run", defaults=(0,))

_cache = {}
_cache_lock = threading.Lock()


def parse(spec) -> Tuple[str, Optional[float]]:
    """`spec` -> ("code", None), ("srgb", None) or ("gamma", g); None is "code".  Anything else raises ValueError.  Whether a gamma
    makes usable tables is `tables`' question, not asked here."""
    if spec is None or spec == CODE:
        return CODE, None
    if spec == "srgb":
        return "srgb", None
    if isinstance(spec, str) and spec.startswith("gamma:"):
        try:
            g = float(spec[len("gamma:"):])
        except ValueError:
            g = math.nan
        if math.isfinite(g):
            return "gamma", g
    raise ValueError(f"light {spec!r}: expected 'code', 'srgb' or 'gamma:<number>'")


def name(spec) -> str:
    """The canonical spelling of a spec: "code", "srgb" or "gamma:<repr of the float>"."""
    kind, g = parse(spec)
    return kind if g is None else f"gamma:{g!r}"


def is_code(spec) -> bool:
    return parse(spec)[0] == CODE


def first_invalid(lin, thr) -> Optional[int]:
    """The first code at which the pair fails the validity conditions (0 for lin[0] != 0, 255 for lin[255] > S), or None."""
    lin, thr = np.asarray(lin).astype(np.int64).reshape(-1), np.asarray(thr).astype(np.int64).reshape(-1)
    if lin.size != 256 or thr.size != 256:
        raise ValueError(f"light tables hold 256 words each; got {lin.size} and {thr.size}")
    if lin[0] != 0:
        return 0
    bad = np.flatnonzero(~((lin[:-1] < thr[1:]) & (thr[1:] <= lin[1:])))
    if bad.size:
        return int(bad[0]) + 1
    return 255 if lin[255] > S else None


def check(lin, thr) -> bool:
    """Is (lin, thr) a valid pair?"""
    return first_invalid(lin, thr) is None


def tables(spec) -> Tuple[np.ndarray, np.ndarray]:
    """(lin, thr) of a light as uint32 [256] each; ValueError for `code` (no light at all) and for a pair that is not valid."""
    kind, g = parse(spec)
    if kind == CODE:
        raise ValueError("light 'code' averages code values: it has no tables")
    c = np.arange(256, dtype=np.float64)
    with np.errstate(all="ignore"):
        if kind == "srgb":
            def f(v):
                return np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
        else:
            def f(v):
                return v ** g
        lin = np.rint(S * f(c / 255.0))
        thr = np.rint(S * f(np.maximum(c - 0.5, 0.0) / 255.0))
    thr[0] = 0.0
    both = np.concatenate([lin, thr])
    if not np.all(np.isfinite(both)) or both.min() < 0 or both.max() >= 2.0 ** 32:
        code = int(np.flatnonzero(~((both >= 0) & (both < 2.0 ** 32)))[0]) % 256
        raise ValueError(f"light {name(spec)}: the tables are not valid at code {code}: its transfer is not a 32-bit value there")
    bad = first_invalid(lin, thr)
    if bad is not None:
        raise ValueError(f"light {name(spec)}: the tables are not valid at code {bad} (lin[{max(bad - 1, 0)}] = {int(lin[max(bad - 1, 0)])}, "
                         f"thr[{bad}] = {int(thr[bad])}, lin[{bad}] = {int(lin[bad])}; need lin[0] == 0, lin[255] <= {S} and "
                         f"lin[c-1] < thr[c] <= lin[c])")
    return lin.astype(np.uint32), thr.astype(np.uint32)


def device_tables(spec, device):
    """(device, host) int32 tensors of the 512 words lin[256], thr[256] (all below 2^24) for the C entry points, made once per light and
    device and kept; the upload has completed when this returns, so any stream may read them."""
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("light tables live on an MI355X (HIP kernels); there is no CPU path")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (name(spec), dev.index)
    with _cache_lock:
        if key not in _cache:
            lin, thr = tables(spec)
            host = torch.from_numpy(np.concatenate([lin, thr]).astype(np.int32))
            on = host.to(dev)
            torch.cuda.current_stream(dev).synchronize()
            _cache[key] = (on, host)
        return _cache[key]


# ---- sensor noise ----

def philox(counter, key) -> Tuple[int, int, int, int]:
    """Philox4x32-10 of four counter words under two key words, in Python integers (the host's draws; the kernels have their own)."""
    c0, c1, c2, c3 = (int(v) & 0xffffffff for v in counter)
    k0, k1 = (int(v) & 0xffffffff for v in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xffffffff, (p0 >> 32) ^ c3 ^ k1, p0 & 0xffffffff
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return c0, c1, c2, c3


def key_of(seed: int) -> Tuple[int, int]:
    """(key0, key1) of a seed."""
    return int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff


def gauss_table() -> np.ndarray:
    """The 1025 Q12 quantiles of the standard normal distribution the kernels interpolate in, int32."""
    nd = statistics.NormalDist()
    lo = 2.0 ** -13
    return np.array([round(4096 * nd.inv_cdf(min(max(i / 1024, lo), 1 - lo))) for i in range(GAUSS_WORDS)], dtype=np.int32)


def gauss_valid(t) -> bool:
    """Is `t` a table the C entry points accept: 1025 words, strictly increasing, every |t[i]| < 2^15?"""
    t = np.asarray(t).astype(np.int64).reshape(-1)
    return bool(t.size == GAUSS_WORDS and np.all(t[:-1] < t[1:]) and np.all(np.abs(t) < 2 ** 15))


def _side(text: str, what: str, top: float):
    def number(v):
        try:
            x = float(v)
        except ValueError:
            x = math.nan
        if not math.isfinite(x):
            raise ValueError(f"noise: {what} {v!r} is not a number")
        if not 0 <= x <= top:
            raise ValueError(f"noise: {what} {x!r} lies outside [0, {top}]")
        return x
    if ".." in text:
        lo, hi = (number(v) for v in text.split("..", 1))
        if not 0 < lo <= hi:
            raise ValueError(f"noise: the {what} range {text!r} needs 0 < lo <= hi (it is drawn log-uniformly)")
        return lo, hi
    x = number(text)
    return x, x


def parse_noise(spec):
    """`spec` "<shot>:<read>", each side a number or "lo..hi" -> ((shot lo, shot hi), (read lo, read hi)); None -> None.  ValueError
    for anything else, for a level outside 0 <= shot <= 0.05, 0 <= read <= 0.1 and for a range without 0 < lo <= hi."""
    if spec is None:
        return None
    if not isinstance(spec, str) or spec.count(":") != 1:
        raise ValueError(f"noise {spec!r}: expected '<shot>:<read>', each a number or 'lo..hi'")
    shot, read = spec.split(":")
    return _side(shot.strip(), "shot coefficient", MAX_SHOT), _side(read.strip(), "read deviation", MAX_READ)


def noise_text(parsed) -> str:
    return ":".join(repr(lo) if lo == hi else f"{lo!r}..{hi!r}" for lo, hi in parsed)


def noise_name(spec) -> Optional[str]:
    """The canonical spelling of a noise spec (the reprs of its floats), or None for None."""
    return None if spec is None else noise_text(parse_noise(spec))


def check_noise(light, noise) -> None:
    """ValueError for a noise spec that does not parse and for noise on the light `code`."""
    if noise is None:
        return
    parse_noise(noise)
    if is_code(light):
        raise ValueError("noise is added in linear light: give a light 'srgb' or 'gamma:<g>' beside it (--light / --blur_light), not 'code'")


def noise_draw(spec, seed: int, clip: int) -> Tuple[float, float]:
    """(a, r) of clip `clip` under `seed`: a side that is a number is that number, a range is drawn log-uniformly from the Philox words
    of the counter (0xffffffff, 0xffffffff, 0, clip) — no pixel has that counter."""
    (a_lo, a_hi), (r_lo, r_hi) = parse_noise(spec)
    w = philox((0xffffffff, 0xffffffff, 0, clip), key_of(seed))
    a = a_lo if a_lo == a_hi else min(max(a_lo * (a_hi / a_lo) ** (w[0] / 2.0 ** 32), a_lo), a_hi)
    r = r_lo if r_lo == r_hi else min(max(r_lo * (r_hi / r_lo) ** (w[1] / 2.0 ** 32), r_lo), r_hi)
    return a, r


def noise_levels(spec, seed: int, clip: int) -> Tuple[int, int]:
    """(A, B) = (rint(a S), rint(r^2 S^2)) of clip `clip` under `seed`."""
    a, r = noise_draw(spec, seed, clip)
    return int(np.rint(a * S)), int(np.rint(r * r * float(S) * float(S)))


def noise_records(runs, clip: int, A: int, B: int) -> np.ndarray:
    """NOISE_RECORD [len(runs)] of one clip: the run ids `runs` at the levels (A, B)."""
    runs = np.asarray(runs, np.int64).reshape(-1)
    rec = np.zeros(runs.size, dtype=NOISE_RECORD)
    rec["run"], rec["clip"], rec["A"], rec["B"] = runs, clip, A, B
    return rec


def device_gauss(device):
    """(device, host) int32 tensors of the gauss table for the C entry points, made once per device and kept, as `device_tables`."""
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("the gauss table lives on an MI355X (HIP kernels); there is no CPU path")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = ("gauss", dev.index)
    with _cache_lock:
        if key not in _cache:
            host = torch.from_numpy(gauss_table())
            on = host.to(dev)
            torch.cuda.current_stream(dev).synchronize()
            _cache[key] = (on, host)
        return _cache[key]
