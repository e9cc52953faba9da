"""Camera-shake blur in blur synthesis (blurset.py, data.SharpTrainLoader; csrc/shake.hip): the blur a hand-held camera adds inside ONE
exposure, as a random trajectory point-spread function (PSF) the sharp frame is correlated with (Boracchi & Foi, "Modeling the
performance of image restoration from motion blur", IEEE TIP 2012; the training sets of DeblurGAN, Kupyn et al., CVPR 2018).  It sits
where the run mean, the light and the noise already are (speinet_amd/light.py): linear light, integer arithmetic, defined bit for bit.
Shake needs a linear light: `code` plus shake is a ValueError.

THE ARITHMETIC.  Take an output frame made from a run of n frames (1..15).  Lm(y, x, c) is light.py's linear mean, floor(sum of lin[byte]
/ n), at pixel (y, x) of the FULL source frame [H][W].  The frame's PSF is w[dy][dx], -r <= dy, dx <= r, radius r in 0..16: unsigned Q16
weights that sum to exactly 65536.

    Lb(y, x, c) = (sum over dy, dx of w[dy][dx] Lm(clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1), c) + 2^15) >> 16

The sum is exact (below 2^40 + 2^15).  It is a correlation, not a flipped convolution: the weight at (dy, dx) multiplies the pixel dy
rows below and dx columns to the right.  Coordinates clamp to the FRAME, never to a crop: a training crop's halo reads the real
neighbours outside the crop.  r = 0 (the delta PSF) gives Lb = Lm: such a record returns the light / noise entry's bytes.  Without
noise blur = encode(Lb).  With noise light.py's formulas run on Lb, with the top-up factor generalised — the PSF averages noise away
too: X = A Lb + B, q16 = floor(sum of w^2 / 2^16) (at most 65536),

    V = X - ceil(X q16 / (n 2^16))          (64-bit; X q16 < 2^61)

which for the delta PSF is floor(X (n - 1) / n), light.py's V, bit for bit.  sigma, z, d, L', the Philox counter (x, y, run, clip) of
the OUTPUT pixel in its full frame and encode are unchanged; ground-truth records stay length 1, unshaken, on the copy path; the gray
plane is that of the final encoded bytes; a `zero` record stays zero.

THE PSFS (host, here).  Spec "<lo>..<hi>" or "<len>": the blur extent in pixels, 2 <= lo <= hi <= 30.  Everything is drawn from
light.philox on the counter (k, 0xfffffffe, run, clip) under light.key_of(seed) — row 0xfffffffe is no pixel's, 0xffffffff is the noise
levels' — so the plan's random.Random stream is untouched and a PSF depends on (seed, clip, run) alone.  Only IEEE-exact float64
operations (+ - * / sqrt, floor, ceil) and Gaussians from light.gauss_table by the kernels' `gauss_z` rule: reproducible across machines.

    extent      L = lo + (hi - lo) w0 / 2^32 from k = 0
    trajectory  128 steps, k = 1..128: g_k = (z(w0), z(w1)) / 4096;  v_k = INERTIA v_{k-1} + IMPULSE g_k - PULL p_{k-1}, v_0 = 0;
                p_k = p_{k-1} + v_k, p_0 = 0.  INERTIA = 0.9, IMPULSE = 0.3 and PULL = 0.02 (inertia, Gaussian impulse, pull towards
                the start) are UNTUNED design parameters.
    centre      c = the time-weighted centroid of the path: every step lasts 1 / 128 of the exposure, so c is the mean of the 128
                segment midpoints (p_{k-1} + p_k) / 2
    scale       s = (L / 2) / max_k |p_k - c| over the 129 step points; a maximum of 0 gives the delta.  Every sample then lies within
                L / 2 <= 15 of the centre, bilinear splatting touches at most offset 16, and radius = floor(L / 2) + 1
    samples     segment k is cut into ceil(4 |p_k - p_{k-1}| s) (at least 1) equal parts; each part's midpoint, minus c, times s, is
                splatted bilinearly with the weight (1 / 128) / parts: exposure is uniform in time, dwell points come out brighter
    quantise    w = floor(a 65536 / sum a); the shortfall to 65536 goes one unit each to the taps with the largest fractional parts,
                ties in raster order; q16 from the integers

WHICH FRAMES.  Runs mode (blurset.plan_runs, unchanged): only the runs labelled blurry (label 0) are shaken; sharp runs get radius 0.
`frames="single"` (blurset.plan_single, for ordinary-frame-rate footage): every source frame is its own run of length 1, label 1
(steady, radius 0) with probability `ratio`, label 0 (shaken) otherwise.  One PSF is drawn per output frame, independently: a camera
path that is continuous across frames is out of scope.  The extents and the three constants are NOT fitted to any camera, and no model
has been trained with them here.
"""
from __future__ import annotations

import math
from collections import namedtuple
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np

from . import light as _light

MAX_RADIUS = 16
SIDE = 2 * MAX_RADIUS + 1
MIN_EXTENT, MAX_EXTENT = 2.0, 30.0
STEPS = 128
INERTIA, IMPULSE, PULL = 0.9, 0.3, 0.02              # untuned design parameters
ROW = 0xfffffffe                                     # the counter row of the PSF draws
FRAMES = ("runs", "single")
# spei_shake_record
SHAKE_RECORD = np.dtype([("psf", "<u4"), ("radius", "<u4"), ("q16", "<u4"), ("reserved", "<u4")])
assert SHAKE_RECORD.itemsize == 16
# the shake of one clip for blurset.synthesize: its spec, write_dataset's seed, the clip's index and the id of the first run handed over
ClipShake = namedtuple("ClipShake", "spec seed clip first_run", defaults=(0,))


def parse(spec) -> Optional[Tuple[float, float]]:
    """`spec` "<lo>..<hi>" or "<len>" -> (lo, hi) with 2 <= lo <= hi <= 30; None -> None.  ValueError for anything else."""
    if spec is None:
        return None

    def number(v):
        try:
            x = float(v)
        except (TypeError, ValueError):
            x = math.nan
        if not math.isfinite(x):
            raise ValueError(f"shake {spec!r}: expected '<len>' or '<lo>..<hi>', the blur extent in pixels")
        return x
    text = spec.strip() if isinstance(spec, str) else spec
    lo, hi = (number(v) for v in text.split("..", 1)) if isinstance(text, str) and ".." in text else (number(text),) * 2
    if not MIN_EXTENT <= lo <= hi <= MAX_EXTENT:
        raise ValueError(f"shake {spec!r}: the extent needs {MIN_EXTENT:g} <= lo <= hi <= {MAX_EXTENT:g} pixels")
    return lo, hi


def name(spec) -> Optional[str]:
    """The canonical spelling of a shake spec (the reprs of its floats), or None for None."""
    p = parse(spec)
    return None if p is None else (repr(p[0]) if p[0] == p[1] else f"{p[0]!r}..{p[1]!r}")


def check(light, spec, frames: str = "runs") -> None:
    """ValueError for a shake spec that does not parse, for shake on the light `code`, for an unknown `frames` and for `single`
    without shake (every frame would come out sharp)."""
    if frames not in FRAMES:
        raise ValueError(f"frames {frames!r}: expected 'runs' or 'single'")
    if spec is None:
        if frames == "single":
            raise ValueError("frames 'single' makes every source frame its own run: without a shake spec (--shake / --blur_shake) every "
                             "frame would come out sharp")
        return
    parse(spec)
    if _light.is_code(light):
        raise ValueError("shake is applied in linear light: give a light 'srgb' or 'gamma:<g>' beside it (--light / --blur_light), not 'code'")


def _z(w: int, t) -> int:
    """light.h's gauss_z in Python integers."""
    i, f = w >> 22, (w >> 10) & 4095
    return (int(t[i]) * (4096 - f) + int(t[i + 1]) * f + 2048) >> 12


@lru_cache(maxsize=1)
def _gauss():
    return [int(v) for v in _light.gauss_table()]


def trajectory(seed: int, clip: int, run: int) -> list:
    """The 129 step points p_0 .. p_128 of the camera path of output frame `run` of clip `clip` under `seed`, as (y, x) float pairs."""
    key, t = _light.key_of(seed), _gauss()
    p, v, pts = (0.0, 0.0), (0.0, 0.0), [(0.0, 0.0)]
    for k in range(1, STEPS + 1):
        w = _light.philox((k, ROW, run, clip), key)
        g = (_z(w[0], t) / 4096.0, _z(w[1], t) / 4096.0)
        v = tuple(INERTIA * v[i] + IMPULSE * g[i] - PULL * p[i] for i in range(2))
        p = (p[0] + v[0], p[1] + v[1])
        pts.append(p)
    return pts


def quantise(a: np.ndarray) -> np.ndarray:
    """Non-negative float64 [33, 33] with a positive sum -> uint32 weights that sum to exactly 65536: floor(a 65536 / sum a), the shortfall
    one unit each to the largest fractional parts, ties in raster order."""
    flat = [float(v) for v in np.asarray(a, np.float64).reshape(-1)]
    total = 0.0
    for v in flat:
        total += v
    scaled = [v * 65536.0 / total for v in flat]
    w = [int(math.floor(v)) for v in scaled]
    short = 65536 - sum(w)
    order = sorted(range(len(flat)), key=lambda i: (-(scaled[i] - w[i]), i))
    assert 0 <= short <= len(order), short
    for i in order[:short]:
        w[i] += 1
    return np.asarray(w, np.uint32).reshape(SIDE, SIDE)


def q16_of(w) -> int:
    """floor(sum of w^2 / 2^16) of integer weights."""
    return sum(int(v) * int(v) for v in np.asarray(w).reshape(-1)) >> 16


def delta() -> np.ndarray:
    w = np.zeros((SIDE, SIDE), np.uint32)
    w[MAX_RADIUS, MAX_RADIUS] = 65536
    return w


def rasterise(pts, extent: float):
    """The step points of a path and the extent L -> (w uint32 [33, 33], radius, q16); a path that never leaves its centroid gives the
    delta with radius 0."""
    n = len(pts) - 1
    mids = [((pts[k][0] + pts[k + 1][0]) / 2.0, (pts[k][1] + pts[k + 1][1]) / 2.0) for k in range(n)]
    cy = cx = 0.0
    for m in mids:
        cy, cx = cy + m[0], cx + m[1]
    cy, cx = cy / n, cx / n
    far = 0.0
    for p in pts:
        far = max(far, math.sqrt((p[0] - cy) * (p[0] - cy) + (p[1] - cx) * (p[1] - cx)))
    if far == 0.0:
        return delta(), 0, 65536
    s = (extent / 2.0) / far
    a = [[0.0] * SIDE for _ in range(SIDE)]
    for k in range(n):
        (y0, x0), (y1, x1) = pts[k], pts[k + 1]
        dy, dx = y1 - y0, x1 - x0
        parts = max(1, int(math.ceil(4.0 * math.sqrt(dy * dy + dx * dx) * s)))
        share = (1.0 / n) / parts
        for j in range(parts):
            f = (j + 0.5) / parts
            qy, qx = (y0 + f * dy - cy) * s, (x0 + f * dx - cx) * s
            iy, ix = int(math.floor(qy)), int(math.floor(qx))
            fy, fx = qy - iy, qx - ix
            for oy, wy in ((iy, 1.0 - fy), (iy + 1, fy)):
                for ox, wx in ((ix, 1.0 - fx), (ix + 1, fx)):
                    if wy * wx > 0.0:
                        a[oy + MAX_RADIUS][ox + MAX_RADIUS] += share * wy * wx
    w = quantise(np.asarray(a))
    return w, int(math.floor(extent / 2.0)) + 1, q16_of(w)


def extent(spec, seed: int, clip: int, run: int) -> float:
    """L of output frame `run` of clip `clip` under `seed`: lo + (hi - lo) w0 / 2^32 from the counter (0, 0xfffffffe, run, clip)."""
    return _extent(*parse(spec), seed, clip, run)


def _extent(lo: float, hi: float, seed: int, clip: int, run: int) -> float:
    return lo + (hi - lo) * _light.philox((0, ROW, run, clip), _light.key_of(seed))[0] / 2.0 ** 32


@lru_cache(maxsize=8192)
def _psf(lo: float, hi: float, seed: int, clip: int, run: int):
    w, radius, q16 = rasterise(trajectory(seed, clip, run), _extent(lo, hi, seed, clip, run))
    w.setflags(write=False)
    return w, radius, q16


def psf(spec, seed: int, clip: int, run: int):
    """(w uint32 [33, 33] (read-only), radius, q16) of output frame `run` of clip `clip` under `seed`; centre at [16][16]."""
    lo, hi = parse(spec)
    return _psf(lo, hi, int(seed), int(clip), int(run))


def _shaken(runs, labels):
    runs, labels = np.asarray(runs, np.int64).reshape(-1), np.asarray(labels, np.int64).reshape(-1)
    if runs.size != labels.size:
        raise ValueError(f"shake: {runs.size} run ids for {labels.size} labels")
    return runs, labels == 0


def records(spec, seed: int, clip: int, runs, labels, base: int = 0) -> np.ndarray:
    """SHAKE_RECORD [len(runs)] of one clip: the run ids `runs` with their labels; a run labelled 0 carries its PSF's radius and q16 and
    the PSF's index in `psf_table` of the same arguments plus `base`, any other run the delta (radius 0, q16 65536)."""
    runs, shaken = _shaken(runs, labels)
    rec = np.zeros(runs.size, dtype=SHAKE_RECORD)
    rec["q16"] = 65536
    at = 0
    for i in np.flatnonzero(shaken):
        _, radius, q16 = psf(spec, seed, clip, int(runs[i]))
        rec[i] = (base + at if radius else 0, radius, q16, 0)
        at += 1
    return rec


def psf_table(spec, seed: int, clip: int, runs, labels) -> np.ndarray:
    """uint32 [n, 33, 33]: the PSFs of the runs labelled 0, in the order of `runs` (what `records`' psf indices count)."""
    runs, shaken = _shaken(runs, labels)
    tabs = [psf(spec, seed, clip, int(runs[i]))[0] for i in np.flatnonzero(shaken)]
    return np.stack(tabs).astype(np.uint32) if tabs else np.zeros((0, SIDE, SIDE), np.uint32)


def device_psfs(table: np.ndarray, device):
    """(device, host) int32-typed tensors of a uint32 [n, 33, 33] PSF table for the C entry points; the upload is issued on the current
    stream of `device`."""
    import torch
    host = torch.from_numpy(np.ascontiguousarray(table, dtype=np.uint32).reshape(-1, SIDE, SIDE).view(np.int32).copy())
    return host.to(torch.device(device)), host
