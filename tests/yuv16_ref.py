"""The deep (10- and 12-bit) planar-YUV conversions of the clip API restated in numpy, from the definition in include/speinet_hip.h
(not from the kernel): int64 arithmetic, the literal Q14 tables, `>>` floors.  Depth d, s = d - 8, D = 2^d - 1; a sample is a 16-bit
word and a word above D is read as D.  The resampling is `yuv_ref`'s.  A helper of the deep y4m tests."""
from fractions import Fraction

import numpy as np

import yuv_ref as R8
from yuv_ref import BT601, BT709, CENTER, FULL, LEFT, LIMITED, P444, chroma_shape        # noqa: F401

DEPTHS = (10, 12)
_NAMES = R8._NAMES
# limited range per (depth, matrix); full range reuses the 8-bit full rows at every depth
TABLE = {
    (10, BT601): (4195, 8236, 1599, -2421, -4754, 7175, 7175, -6008, -1167, 64, 19133, 26226, -6438, -13359, 33148),
    (10, BT709): (2983, 10034, 1013, -1644, -5531, 7175, 7175, -6517, -658, 64, 19133, 29459, -3504, -8757, 34711),
    (12, BT601): (4192, 8229, 1598, -2420, -4750, 7170, 7170, -6004, -1166, 256, 19147, 26245, -6442, -13369, 33172),
    (12, BT709): (2981, 10026, 1012, -1643, -5527, 7170, 7170, -6513, -657, 256, 19147, 29480, -3507, -8763, 34737),
}
KR_KB = {BT601: (Fraction(299, 1000), Fraction(114, 1000)), BT709: (Fraction(2126, 10000), Fraction(722, 10000))}


def rule(depth, matrix, rng) -> tuple:
    """The row of (depth, matrix, range) from the rule, in exact rationals rounded to nearest (an exact half raises)."""
    s, D = depth - 8, (1 << depth) - 1
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    if rng == FULL:
        ly = lc = Fraction(1)
        yo = 0
    else:
        ly, lc, yo = Fraction(219 << s, D), Fraction(224 << s, D), 16 << s

    def rnd(x):
        x = Fraction(x)
        assert (2 * x).denominator != 1 or x.denominator == 1, f"{x} is an exact half"
        return int((x + Fraction(1, 2)).__floor__())

    q = 16384
    yr, yb = rnd(q * kr * ly), rnd(q * kb * ly)
    yg = rnd(q * ly) - yr - yb
    ub = vr = rnd(q * lc / 2)
    ur = -rnd(q * lc * kr / (2 * (1 - kb)))
    ug = -ub - ur
    vb = -rnd(q * lc * kb / (2 * (1 - kr)))
    vg = -vr - vb
    cy = rnd(q / ly)
    rv, bu = rnd(q * 2 * (1 - kr) / lc), rnd(q * 2 * (1 - kb) / lc)
    gu = -rnd(q * 2 * kb * (1 - kb) / (kg * lc))
    gv = -rnd(q * 2 * kr * (1 - kr) / (kg * lc))
    return (yr, yg, yb, ur, ug, ub, vr, vg, vb, yo, cy, rv, gu, gv, bu)


def coef(depth, matrix, rng) -> dict:
    assert depth in DEPTHS
    return dict(zip(_NAMES, R8.TABLE[(matrix, FULL)] if rng == FULL else TABLE[(depth, matrix)]))


def frame_samples(h, w, layout) -> int:
    return R8.frame_bytes(h, w, layout)


def _words(a, depth):
    """16-bit words as int64 samples: a word above D reads as D."""
    return np.minimum(np.asarray(a).astype(np.int64) & 0xffff, (1 << depth) - 1)


def split(planar, h, w, layout, depth):
    """Y, U, V planes (int64, at most D) of one planar frame of uint16 words."""
    ch, cw = chroma_shape(h, w, layout)
    p = _words(np.asarray(planar, dtype=np.uint16).reshape(-1), depth)
    assert p.size == frame_samples(h, w, layout)
    return p[:h * w].reshape(h, w), p[h * w:h * w + ch * cw].reshape(ch, cw), p[h * w + ch * cw:].reshape(ch, cw)


def yuv_to_rgb_sums(Y, U16, V16, depth, matrix, rng):
    """The three sums before `>> 18` (int64, last axis R G B): what must not be taken in 32 bits."""
    k, s = coef(depth, matrix, rng), depth - 8
    Y, U16, V16 = (np.asarray(a, dtype=np.int64) for a in (Y, U16, V16))
    yy = k["cy"] * 16 * (Y - k["yo"])
    u, v = U16 - (2048 << s), V16 - (2048 << s)
    return np.stack([yy + k["rv"] * v + (1 << 17), yy + k["gu"] * u + k["gv"] * v + (1 << 17), yy + k["bu"] * u + (1 << 17)], axis=-1)


def yuv_to_rgb_values(Y, U16, V16, depth, matrix, rng):
    """RGB (uint16, last axis) from luma and 16-fold chroma arrays of one shape (samples at most D)."""
    return np.clip(yuv_to_rgb_sums(Y, U16, V16, depth, matrix, rng) >> 18, 0, (1 << depth) - 1).astype(np.uint16)


def yuv_to_rgb(planar, h, w, layout, matrix, rng, depth):
    """One planar frame of uint16 words -> uint16 [h,w,3]."""
    y, u, v = split(planar, h, w, layout, depth)
    return yuv_to_rgb_values(y, R8.upsample16(u, h, w, layout), R8.upsample16(v, h, w, layout), depth, matrix, rng)


def _limits(depth, rng):
    s, D = depth - 8, (1 << depth) - 1
    return ((16 << s, 235 << s), (16 << s, 240 << s)) if rng == LIMITED else ((0, D), (0, D))


def _yuv(k, r, g, b, depth, rng, shift):
    (ylo, yhi), (clo, chi) = _limits(depth, rng)
    rnd, mid = 1 << (shift - 1), 128 << (depth - 8)
    u = np.clip(((k["ur"] * r + k["ug"] * g + k["ub"] * b + rnd) >> shift) + mid, clo, chi)
    v = np.clip(((k["vr"] * r + k["vg"] * g + k["vb"] * b + rnd) >> shift) + mid, clo, chi)
    return u, v


def rgb_to_yuv_values(rgb, depth, matrix, rng):
    """Per-pixel Y, U, V (the 4:4:4 rule) of an array of words whose last axis is RGB: three int64 arrays."""
    k = coef(depth, matrix, rng)
    (ylo, yhi), _ = _limits(depth, rng)
    c = _words(rgb, depth)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    y = np.clip(((k["yr"] * r + k["yg"] * g + k["yb"] * b + (1 << 13)) >> 14) + k["yo"], ylo, yhi)
    u, v = _yuv(k, r, g, b, depth, rng, 14)
    return y, u, v


def rgb_to_yuv(rgb, layout, matrix, rng, depth):
    """uint16 [h,w,3] -> one planar frame (uint16, flat)."""
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    y, u, v = rgb_to_yuv_values(rgb, depth, matrix, rng)
    if layout != P444:
        k = coef(depth, matrix, rng)
        ch, cw = chroma_shape(h, w, layout)
        c = _words(rgb, depth)
        j, i = np.arange(ch), np.arange(cw)
        rows = c[np.clip(2 * j, 0, h - 1)] + c[np.clip(2 * j + 1, 0, h - 1)]          # [ch, w, 3]

        def col(x):
            return rows[:, np.clip(x, 0, w - 1)]

        if layout == CENTER:
            sm, shift = col(2 * i) + col(2 * i + 1), 16
        else:
            sm, shift = col(2 * i - 1) + 2 * col(2 * i) + col(2 * i + 1), 17
        u, v = _yuv(k, sm[..., 0], sm[..., 1], sm[..., 2], depth, rng, shift)
    return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).astype(np.uint16)


def luma(rgb, depth):
    """The depth-bit integer luma of the pair statistics: (77 R + 150 G + 29 B + 128) >> 8."""
    c = _words(rgb, depth)
    return (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8
