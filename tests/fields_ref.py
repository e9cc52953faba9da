"""Interlaced frames of the clip API (`deblur_clip(..., fields="split")`) restated in numpy, from the definition in
include/speinet_hip.h (not from the kernel).  A woven frame f of even height is two fields, field p = f[p::2]; the planar picture of
field p of a y4m frame is its Y rows p::2 and, for 4:2:0, its chroma-plane rows p::2 (chroma row j belongs to field j & 1); the other
layouts have one chroma row per luma row, so there the chroma rows p::2 are the field's as well.  The conversions are those of
`yuv_ref` / `yuv16_ref` / `yuv422_ref`, applied to each field's picture.  A helper of the fields tests; it holds no kernel code."""
import numpy as np

import yuv422_ref as R422
import yuv_ref as R8
from yuv_ref import BT601, BT709, CENTER, FULL, LEFT, LIMITED, P444        # noqa: F401
from yuv422_ref import MONO, P422                                          # noqa: F401

LAYOUTS = (CENTER, LEFT, P444, P422, MONO)


def split(f, p):
    """Field p (0 = top, 1 = bottom) of a woven frame [H, ...] (or of a clip [T, H, ...] with axis=1 in mind: use f[:, p::2])."""
    return f[p::2]


def weave(a, b):
    """The frame whose top field is a and whose bottom field is b: rows 0, 2, ... from a, rows 1, 3, ... from b."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    out = np.empty((2 * a.shape[0],) + a.shape[1:], a.dtype)
    out[0::2], out[1::2] = a, b
    return out


def chroma_shape(h, w, layout):
    return R8.chroma_shape(h, w, layout) if layout in (CENTER, LEFT, P444) else R422.chroma_shape(h, w, layout)


def planes(planar, h, w, layout):
    """The Y, U, V planes of one planar frame as they lie in the record (views, any dtype)."""
    ch, cw = chroma_shape(h, w, layout)
    p = np.asarray(planar).reshape(-1)
    assert p.size == h * w + 2 * ch * cw
    return p[:h * w].reshape(h, w), p[h * w:h * w + ch * cw].reshape(ch, cw), p[h * w + ch * cw:].reshape(ch, cw)


def field_planar(planar, h, w, layout, p):
    """The planar picture of field p of one planar frame: a frame of h / 2 rows in the same layout."""
    assert h % 2 == 0 and (layout not in (CENTER, LEFT) or h % 4 == 0)
    return np.concatenate([np.ascontiguousarray(a[p::2]).reshape(-1) for a in planes(planar, h, w, layout)])


def weave_planar(top, bottom, h, w, layout):
    """The planar frame whose field pictures are `top` and `bottom` (planar frames of h / 2 rows)."""
    tp, bp = planes(top, h // 2, w, layout), planes(bottom, h // 2, w, layout)
    return np.concatenate([weave(a, b).reshape(-1) for a, b in zip(tp, bp)])


def _to_rgb(planar, h, w, layout, matrix, rng, depth):
    if layout in (P422, MONO):
        return R422.yuv_to_rgb(planar, h, w, layout, matrix, rng, depth)
    return R422.old_yuv_to_rgb(planar, h, w, layout, matrix, rng, depth)


def _from_rgb(rgb, layout, matrix, rng, depth):
    if layout in (P422, MONO):
        return R422.rgb_to_yuv(rgb, layout, matrix, rng, depth)
    return R422.old_rgb_to_yuv(rgb, layout, matrix, rng, depth)


def yuv_to_rgb(planar, h, w, layout, matrix, rng, depth=8):
    """The progressive conversion of one planar frame (every layout) -> [h,w,3]."""
    return _to_rgb(planar, h, w, layout, matrix, rng, depth)


def rgb_to_yuv(rgb, layout, matrix, rng, depth=8):
    return _from_rgb(rgb, layout, matrix, rng, depth)


def yuv_fields_to_rgb(planar, h, w, layout, matrix, rng, depth=8):
    """One planar INTERLACED frame -> the woven RGB frame [h,w,3] whose field p is the conversion of field p's planar picture."""
    return weave(*[_to_rgb(field_planar(planar, h, w, layout, p), h // 2, w, layout, matrix, rng, depth) for p in (0, 1)])


def rgb_to_yuv_fields(rgb, layout, matrix, rng, depth=8):
    """One woven RGB frame [h,w,3] -> the planar frame whose field pictures are the conversions of the RGB fields."""
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    return weave_planar(*[_from_rgb(np.ascontiguousarray(rgb[p::2]), layout, matrix, rng, depth) for p in (0, 1)], h, w, layout)
