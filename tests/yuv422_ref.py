"""The 4:2:2 and mono planar-YUV conversions of the clip API restated in numpy, from the definition in include/speinet_hip.h (not
from the kernel): int64 arithmetic, the Q14 tables of `yuv_ref` (8 bits) and `yuv16_ref` (10 and 12 bits, each row made by its
`rule`), `>>` floors.  Depth d in (8, 10, 12), s = d - 8, D = 2^d - 1; a deep sample is a 16-bit word and a word above D is read as
D.  A helper of the 4:2:2 / mono y4m tests."""
import numpy as np

import yuv16_ref as R16
import yuv_ref as R8
from yuv_ref import BT601, BT709, CENTER, FULL, LEFT, LIMITED, P444        # noqa: F401

P422, MONO = 3, 4                          # SPEI_YUV_422, SPEI_YUV_MONO
DEPTHS = (8, 10, 12)


def coef(depth, matrix, rng) -> dict:
    return R8.coef(matrix, rng) if depth == 8 else R16.coef(depth, matrix, rng)


def dtype_of(depth):
    return np.uint8 if depth == 8 else np.uint16


def chroma_shape(h, w, layout):
    return {P422: (h, (w + 1) // 2), MONO: (0, 0)}[layout]


def frame_samples(h, w, layout) -> int:
    ch, cw = chroma_shape(h, w, layout)
    return h * w + 2 * ch * cw


def split(planar, h, w, layout, depth=8):
    """Y, U, V planes (int64, at most D) of one planar frame; U and V are empty for mono."""
    ch, cw = chroma_shape(h, w, layout)
    p = np.minimum(np.asarray(planar, dtype=dtype_of(depth)).reshape(-1).astype(np.int64), (1 << depth) - 1)
    assert p.size == frame_samples(h, w, layout)
    return p[:h * w].reshape(h, w), p[h * w:h * w + ch * cw].reshape(ch, cw), p[h * w + ch * cw:].reshape(ch, cw)


def upsample16(c, w):
    """A 4:2:2 chroma plane [h, ceil(w/2)] at full width, times 16: 16 c[y][i] at even x, 8 (c[y][i] + c[y][i+1]) at odd x, i = x >> 1,
    i + 1 clamped to the plane."""
    c = np.asarray(c, dtype=np.int64)
    x = np.arange(w)
    i = x >> 1
    i1 = np.minimum(i + 1, c.shape[1] - 1)
    return np.where(x % 2 == 0, 16 * c[:, i], 8 * (c[:, i] + c[:, i1]))


def yuv_to_rgb_values(Y, U16, V16, depth, matrix, rng):
    """RGB (last axis; uint8, or uint16 for a deep frame) from luma and 16-fold chroma arrays of one shape."""
    return R8.yuv_to_rgb_values(Y, U16, V16, matrix, rng) if depth == 8 else R16.yuv_to_rgb_values(Y, U16, V16, depth, matrix, rng)


def yuv_to_rgb(planar, h, w, layout, matrix, rng, depth=8):
    """One planar 4:2:2 or mono frame -> [h,w,3] (uint8, or uint16 for a deep frame)."""
    y, u, v = split(planar, h, w, layout, depth)
    if layout == MONO:
        u16 = v16 = np.full((h, w), 2048 << (depth - 8), np.int64)
    else:
        u16, v16 = upsample16(u, w), upsample16(v, w)
    return yuv_to_rgb_values(y, u16, v16, depth, matrix, rng)


def limits(depth, rng):
    """((Y lo, Y hi), (chroma lo, chroma hi))"""
    s, D = depth - 8, (1 << depth) - 1
    return ((16 << s, 235 << s), (16 << s, 240 << s)) if rng == LIMITED else ((0, D), (0, D))


def rgb_to_yuv(rgb, layout, matrix, rng, depth=8):
    """[h,w,3] (uint8, or uint16 words of a deep frame) -> one planar 4:2:2 or mono frame (flat, same dtype)."""
    k, s, D = coef(depth, matrix, rng), depth - 8, (1 << depth) - 1
    (ylo, yhi), (clo, chi) = limits(depth, rng)
    c = np.minimum(np.asarray(rgb, dtype=dtype_of(depth)).astype(np.int64), D)
    h, w = c.shape[:2]
    y = np.clip(((k["yr"] * c[..., 0] + k["yg"] * c[..., 1] + k["yb"] * c[..., 2] + (1 << 13)) >> 14) + k["yo"], ylo, yhi)
    if layout == MONO:
        return y.reshape(-1).astype(dtype_of(depth))
    i = np.arange((w + 1) // 2)
    S = c[:, np.clip(2 * i - 1, 0, w - 1)] + 2 * c[:, 2 * i] + c[:, np.clip(2 * i + 1, 0, w - 1)]          # [h, cw, 3]
    assert int(np.abs(S).max()) * 8192 < 1 << 31
    u = np.clip(((k["ur"] * S[..., 0] + k["ug"] * S[..., 1] + k["ub"] * S[..., 2] + (1 << 15)) >> 16) + (128 << s), clo, chi)
    v = np.clip(((k["vr"] * S[..., 0] + k["vg"] * S[..., 1] + k["vb"] * S[..., 2] + (1 << 15)) >> 16) + (128 << s), clo, chi)
    return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).astype(dtype_of(depth))


# ---- the 4:2:0 / 4:4:4 conversions of yuv_ref / yuv16_ref behind one signature: what the identities compare against --------------
def old_samples(h, w, layout) -> int:
    return R8.frame_bytes(h, w, layout)


def old_yuv_to_rgb(planar, h, w, layout, matrix, rng, depth=8):
    return R8.yuv_to_rgb(planar, h, w, layout, matrix, rng) if depth == 8 else R16.yuv_to_rgb(planar, h, w, layout, matrix, rng, depth)


def old_rgb_to_yuv(rgb, layout, matrix, rng, depth=8):
    return R8.rgb_to_yuv(rgb, layout, matrix, rng) if depth == 8 else R16.rgb_to_yuv(rgb, layout, matrix, rng, depth)
