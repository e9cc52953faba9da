"""Numpy restatement of averaging in linear light (speinet_amd/light.py, csrc/light.h), independent of both: the tables rebuilt from
the formulas, decode, floor-mean and encode.  Not a test."""
import numpy as np

S = 2 ** 24 - 1
LIGHTS = ("srgb", "gamma:1.0", "gamma:1.8", "gamma:2.2", "gamma:2.4", "gamma:2.6")


def forward(spec):
    """The forward transfer f of a light: code value in [0, 1] -> linear light in [0, 1], float64."""
    if spec == "srgb":
        return lambda c: np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    g = float(spec.split(":")[1])
    return lambda c: c ** g


def inverse(spec):
    """f's inverse, float64."""
    if spec == "srgb":
        return lambda v: np.where(v <= 0.04045 / 12.92, v * 12.92, 1.055 * v ** (1 / 2.4) - 0.055)
    g = float(spec.split(":")[1])
    return lambda v: v ** (1.0 / g)


def tables(spec):
    """lin[c] = rint(S f(c / 255)); thr[0] = 0, thr[c] = rint(S f((c - 0.5) / 255)).  -> two int64 [256]."""
    f = forward(spec)
    c = np.arange(256, dtype=np.float64)
    lin = np.rint(S * f(c / 255)).astype(np.int64)
    thr = np.rint(S * f(np.maximum(c - 0.5, 0) / 255)).astype(np.int64)
    thr[0] = 0
    return lin, thr


def valid(lin, thr):
    lin, thr = np.asarray(lin, np.int64), np.asarray(thr, np.int64)
    return bool(lin[0] == 0 and lin[255] <= S and np.all(lin[:-1] < thr[1:]) and np.all(thr[1:] <= lin[1:]))


def encode(thr, L):
    """#{c in 1..255 : thr[c] <= L}"""
    return np.searchsorted(np.asarray(thr, np.int64)[1:], np.asarray(L, np.int64), side="right")


def run_mean(window_u8, spec):
    """window_u8 uint8 [n, ...] -> uint8 [...]: the run averaged in the light `spec`; "code" (or None): floor of the mean of the bytes."""
    w = np.asarray(window_u8)
    n = w.shape[0]
    if spec in (None, "code"):
        return (w.astype(np.int64).sum(axis=0) // n).astype(np.uint8)
    lin, thr = tables(spec)
    L = lin[w].sum(axis=0) // n
    return encode(thr, L).astype(np.uint8)


def run_mean_f64(window_u8, spec):
    """255 f^-1(mean f(c / 255)) in float64: what the integer result approximates."""
    w = np.asarray(window_u8).astype(np.float64)
    return 255.0 * inverse(spec)(forward(spec)(w / 255.0).mean(axis=0))


def run_patch(frames_u8, start, length, y0, x0, P, hflip, vflip, rot90, zero, rgb_range, spec):
    """tests/sharpset_ref.run_patch with the run averaged in the light `spec`: one output frame of spei_train_batch_runs_light_u8."""
    if zero:
        return np.zeros((3, P, P), np.float32)
    img = run_mean(frames_u8[start:start + length], spec).astype(np.int64)[y0:y0 + P, x0:x0 + P]
    if hflip:
        img = img[:, ::-1]
    if vflip:
        img = img[::-1, :]
    if rot90:
        img = np.rot90(img)
    return np.ascontiguousarray(img.transpose(2, 0, 1)).astype(np.float32) * np.float32(rgb_range / 255)
