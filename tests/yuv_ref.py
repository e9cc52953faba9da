"""The planar-YUV conversions of the clip API restated in numpy, from the definition in include/speinet_hip.h (not from the kernel):
integer arithmetic, Q14 coefficients, `>>` floors (numpy's shift of a signed integer is arithmetic).  A helper of the y4m tests."""
import numpy as np

CENTER, LEFT, P444 = 0, 1, 2               # SPEI_YUV_420_CENTER, SPEI_YUV_420_LEFT, SPEI_YUV_444
BT601, BT709 = 0, 1
FULL, LIMITED = 0, 1

_NAMES = "yr yg yb ur ug ub vr vg vb yo cy rv gu gv bu".split()
TABLE = {
    (BT601, FULL): (4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332, 0, 16384, 22970, -5638, -11700, 29032),
    (BT601, LIMITED): (4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170, 16, 19077, 26149, -6419, -13320, 33050),
    (BT709, FULL): (3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751, 0, 16384, 25802, -3069, -7670, 30402),
    (BT709, LIMITED): (2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660, 16, 19077, 29372, -3494, -8731, 34610),
}


def coef(matrix, rng) -> dict:
    return dict(zip(_NAMES, TABLE[(matrix, rng)]))


def chroma_shape(h, w, layout):
    return (h, w) if layout == P444 else ((h + 1) // 2, (w + 1) // 2)


def frame_bytes(h, w, layout) -> int:
    ch, cw = chroma_shape(h, w, layout)
    return h * w + 2 * ch * cw


def split(planar, h, w, layout):
    """Y, U, V planes (int64) of one planar frame."""
    ch, cw = chroma_shape(h, w, layout)
    p = np.asarray(planar, dtype=np.uint8).reshape(-1)
    assert p.size == frame_bytes(h, w, layout)
    y = p[:h * w].reshape(h, w)
    u = p[h * w:h * w + ch * cw].reshape(ch, cw)
    v = p[h * w + ch * cw:].reshape(ch, cw)
    return y.astype(np.int64), u.astype(np.int64), v.astype(np.int64)


def upsample16(c, h, w, layout):
    """A chroma plane at full resolution, times 16 (U16 / V16): int64 [h,w]."""
    c = np.asarray(c, dtype=np.int64)
    if layout == P444:
        return 16 * c
    ch, cw = c.shape
    y, x = np.arange(h), np.arange(w)
    j = y >> 1
    jo = np.clip(np.where(y % 2 == 0, j - 1, j + 1), 0, ch - 1)
    rows = 3 * c[j] + c[jo]                                # [h, cw], weights 3 : 1
    i = x >> 1
    if layout == CENTER:
        io = np.clip(np.where(x % 2 == 0, i - 1, i + 1), 0, cw - 1)
        return 3 * rows[:, i] + rows[:, io]
    i1 = np.clip(i + 1, 0, cw - 1)
    return np.where(x % 2 == 0, 4 * rows[:, i], 2 * rows[:, i] + 2 * rows[:, i1])


def yuv_to_rgb_values(Y, U16, V16, matrix, rng):
    """RGB (uint8, last axis) from luma and 16-fold chroma arrays of one shape."""
    k = coef(matrix, rng)
    Y, U16, V16 = (np.asarray(a, dtype=np.int64) for a in (Y, U16, V16))
    yy = k["cy"] * 16 * (Y - k["yo"])
    u, v = U16 - 2048, V16 - 2048
    r = (yy + k["rv"] * v + (1 << 17)) >> 18
    g = (yy + k["gu"] * u + k["gv"] * v + (1 << 17)) >> 18
    b = (yy + k["bu"] * u + (1 << 17)) >> 18
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def yuv_to_rgb(planar, h, w, layout, matrix, rng):
    """One planar frame -> uint8 [h,w,3]."""
    y, u, v = split(planar, h, w, layout)
    return yuv_to_rgb_values(y, upsample16(u, h, w, layout), upsample16(v, h, w, layout), matrix, rng)


def _limits(rng):
    return ((16, 235), (16, 240)) if rng == LIMITED else ((0, 255), (0, 255))


def rgb_to_yuv_values(rgb, matrix, rng):
    """Per-pixel Y, U, V (the 4:4:4 rule) of an int / uint8 array whose last axis is RGB: three int64 arrays."""
    k = coef(matrix, rng)
    (ylo, yhi), (clo, chi) = _limits(rng)
    rgb = np.asarray(rgb).astype(np.int64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    y = np.clip(((k["yr"] * r + k["yg"] * g + k["yb"] * b + (1 << 13)) >> 14) + k["yo"], ylo, yhi)
    u = np.clip(((k["ur"] * r + k["ug"] * g + k["ub"] * b + (1 << 13)) >> 14) + 128, clo, chi)
    v = np.clip(((k["vr"] * r + k["vg"] * g + k["vb"] * b + (1 << 13)) >> 14) + 128, clo, chi)
    return y, u, v


def rgb_to_yuv(rgb, layout, matrix, rng):
    """uint8 [h,w,3] -> one planar frame (uint8, flat)."""
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    y, u, v = rgb_to_yuv_values(rgb, matrix, rng)
    if layout != P444:
        k = coef(matrix, rng)
        _, (clo, chi) = _limits(rng)
        ch, cw = chroma_shape(h, w, layout)
        c = rgb.astype(np.int64)
        j, i = np.arange(ch), np.arange(cw)
        rows = c[np.clip(2 * j, 0, h - 1)] + c[np.clip(2 * j + 1, 0, h - 1)]          # [ch, w, 3]

        def col(x):
            return rows[:, np.clip(x, 0, w - 1)]

        if layout == CENTER:
            s, shift = col(2 * i) + col(2 * i + 1), 16
        else:
            s, shift = col(2 * i - 1) + 2 * col(2 * i) + col(2 * i + 1), 17
        rnd = 1 << (shift - 1)
        u = np.clip(((k["ur"] * s[..., 0] + k["ug"] * s[..., 1] + k["ub"] * s[..., 2] + rnd) >> shift) + 128, clo, chi)
        v = np.clip(((k["vr"] * s[..., 0] + k["vg"] * s[..., 1] + k["vb"] * s[..., 2] + rnd) >> shift) + 128, clo, chi)
    return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).astype(np.uint8)
