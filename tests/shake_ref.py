"""Numpy restatement of the camera-shake blur of blur synthesis (speinet_amd/shake.py "THE ARITHMETIC", csrc/shake.hip), independent
of both, in int64: the correlation with a Q16 PSF on the linear mean of the FULL frame, clamped at the frame's edges, the generalised
noise variance, and the window-mean and train-batch forms.  The mean, the encode, Philox, the gauss table and the crop / flip / rotate
are tests/light_ref.py's and tests/noise_ref.py's.  Not a test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import light_ref  # noqa: E402
import noise_ref  # noqa: E402

S = light_ref.S
R, SIDE = 16, 33


def delta():
    w = np.zeros((SIDE, SIDE), np.int64)
    w[R, R] = 65536
    return w


def tap(dy, dx):
    """All of the weight at (dy, dx): the output pixel is the one dy rows below and dx columns to the right."""
    w = np.zeros((SIDE, SIDE), np.int64)
    w[R + dy, R + dx] = 65536
    return w


def dense(radius, seed):
    """A random table with every tap inside `radius` set, the sum forced to 65536."""
    rs = np.random.RandomState(seed)
    n = 2 * radius + 1
    a = rs.randint(1, 1000, (n, n)).astype(np.int64)
    a = a * 65536 // a.sum()
    a[rs.randint(n), rs.randint(n)] += 65536 - a.sum()
    w = np.zeros((SIDE, SIDE), np.int64)
    w[R - radius:R + radius + 1, R - radius:R + radius + 1] = a
    return w


def radius_of(w):
    ys, xs = np.nonzero(np.asarray(w))
    return int(max(np.abs(ys - R).max(), np.abs(xs - R).max()))


def q16_of(w):
    return int((np.asarray(w, np.int64) ** 2).sum()) >> 16


def valid(w, radius):
    w = np.asarray(w, np.int64)
    inside = np.zeros((SIDE, SIDE), bool)
    inside[R - radius:R + radius + 1, R - radius:R + radius + 1] = True
    return bool(w.shape == (SIDE, SIDE) and w.min() >= 0 and w.sum() == 65536 and not w[~inside].any() and 0 <= radius <= R)


def correlate(Lm, w):
    """Lb of Lm int64 [H, W, 3] under the weights w [33, 33]: exact sum over the clamped neighbours, + 2^15, >> 16."""
    Lm, w = np.asarray(Lm, np.int64), np.asarray(w, np.int64)
    H, W = Lm.shape[:2]
    acc = np.zeros_like(Lm)
    for ty, tx in zip(*np.nonzero(w)):
        y = np.clip(np.arange(H) + (ty - R), 0, H - 1)
        x = np.clip(np.arange(W) + (tx - R), 0, W - 1)
        acc += w[ty, tx] * Lm[y][:, x]
    return (acc + 2 ** 15) >> 16


def apply_noise(L, z, A, B, n, q16):
    """noise_ref.apply with V = X - ceil(X q16 / (n 2^16))."""
    L = np.asarray(L, np.int64)
    assert 0 <= A < 2 ** 20 and 0 <= B < 2 ** 42 and 0 <= q16 <= 65536 and L.min() >= 0 and L.max() <= S
    X = A * L + B
    V = X - -((-X * q16) // (n * 65536))
    d = (noise_ref.isqrt(V) * z + 2048) >> 12
    return np.clip(L + d, 0, S)


def run_mean(window_u8, spec, w, radius, noise=None):
    """window_u8 uint8 [n, H, W, 3] (FULL frames) -> uint8 [H, W, 3]: the run averaged in the light `spec`, correlated with the PSF w of
    `radius`, with the noise (run, clip, seed, A, B) or none.  Radius 0 is the light / noise restatement itself."""
    win = np.asarray(window_u8)
    n, H, W, _ = win.shape
    if radius == 0:
        return light_ref.run_mean(win, spec) if noise is None else noise_ref.run_mean(win, spec, *noise)
    assert valid(w, radius)
    lin, thr = light_ref.tables(spec)
    Lb = correlate(lin[win].sum(axis=0) // n, w)
    if noise is not None:
        run, clip, seed, A, B = noise
        Lb = apply_noise(Lb, noise_ref.z_of(noise_ref.words(H, W, run, clip, seed)), A, B, n, q16_of(w))
    return light_ref.encode(thr, Lb).astype(np.uint8)


def run_patch(full_u8, y0, x0, P, hflip, vflip, rot90, zero, rgb_range):
    """One output frame of the train-batch form from `run_mean`'s FULL frame: crop, flips, rotation, scale; zeros for a zero record."""
    if zero:
        return np.zeros((3, P, P), np.float32)
    return noise_ref.place(full_u8, y0, x0, P, hflip, vflip, rot90, rgb_range)
