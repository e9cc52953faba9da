"""Numpy restatement of the sensor noise of blur synthesis (speinet_amd/light.py "SENSOR NOISE", csrc/light.h), independent of both:
its own Philox4x32-10, gauss table, levels and noise step; the mean and the encode are tests/light_ref.py's.  Not a test."""
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import light_ref  # noqa: E402

S = light_ref.S
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10, vectorised: counters (broadcast against each other) and scalar key words -> four uint64 arrays of 32-bit words."""
    c = [np.asarray(v, np.uint64) & MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xffffffff, int(k1) & 0xffffffff
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]              # 32 x 32 bits: no overflow in 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return c


def key(seed):
    return int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff


def gauss_table():
    nd = statistics.NormalDist()
    return np.array([round(4096 * nd.inv_cdf(min(max(i / 1024, 2.0 ** -13), 1 - 2.0 ** -13))) for i in range(1025)], dtype=np.int64)


GAUSS = gauss_table()


def gauss_valid(t):
    t = np.asarray(t, np.int64)
    return bool(t.shape == (1025,) and np.all(np.diff(t) > 0) and np.all(np.abs(t) < 2 ** 15))


def z_of(w, t=GAUSS):
    """The Q12 deviate of 32-bit words w (any integer array)."""
    w = np.asarray(w).astype(np.int64)
    i, f = w >> 22, (w >> 10) & 4095
    return (t[i] * (4096 - f) + t[i + 1] * f + 2048) >> 12               # numpy's >> on int64 is arithmetic


def isqrt(v):
    """The mathematical integer square root of non-negative int64 values, by Python's math.isqrt."""
    v = np.asarray(v, np.int64)
    return np.array([math.isqrt(int(x)) for x in v.reshape(-1)], dtype=np.int64).reshape(v.shape)


def words(H, W, run, clip, seed):
    """int64 [H, W, 3]: output words 0, 1, 2 of the counter (x, y, run, clip) for every pixel of an H x W frame."""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = philox(x, y, run, clip, *key(seed))
    return np.stack(out[:3], axis=-1).astype(np.int64)


def apply(L, z, A, B, n):
    """L' of linear means L (int64) under deviates z for a run of n frames at the levels A, B."""
    L = np.asarray(L, np.int64)
    assert 0 <= A < 2 ** 20 and 0 <= B < 2 ** 42 and L.min() >= 0 and L.max() <= S
    V = (A * L + B) * (n - 1) // n
    d = (isqrt(V) * z + 2048) >> 12
    return np.clip(L + d, 0, S)


def run_mean(window_u8, spec, run, clip, seed, A, B, t=GAUSS):
    """window_u8 uint8 [n, H, W, 3] (FULL frames) -> uint8 [H, W, 3]: output frame `run` of clip `clip` in the light `spec` with noise."""
    w = np.asarray(window_u8)
    n, H, W, _ = w.shape
    if n == 1:
        return w[0].copy()
    lin, thr = light_ref.tables(spec)
    L = lin[w].sum(axis=0) // n
    return light_ref.encode(thr, apply(L, z_of(words(H, W, run, clip, seed), t), A, B, n)).astype(np.uint8)


def levels(a, r):
    return int(np.rint(a * S)), int(np.rint(r * r * float(S) * float(S)))


def place(img, y0, x0, P, hflip, vflip, rot90, rgb_range):
    """The crop / flip / rotate of a batch record applied to a full uint8 frame -> float32 [3, P, P]."""
    img = img[y0:y0 + P, x0:x0 + P].astype(np.int64)
    if hflip:
        img = img[:, ::-1]
    if vflip:
        img = img[::-1, :]
    if rot90:
        img = np.rot90(img)
    return np.ascontiguousarray(img.transpose(2, 0, 1)).astype(np.float32) * np.float32(rgb_range / 255)
