"""A numpy restatement of the region-of-interest kernels (csrc/roi_io.hip; the definitions in include/speinet_hip.h): `requant`, the
paste (hard and feathered) and the extent maxima, for the tests of `deblur_clip(..., roi=)`.  The hard paste is plain float32
arithmetic, one rounding per step.  The feathered paste has the float32 weights of the definition and is evaluated twice: in float32
step by step, with the one fused multiply-add taken as the float32 rounding of the float64 sum of the exact product and the addend
(`value`), and in float64, where every sample gets the band [lo, hi] that a float32 evaluation within 8 units of 2^-24 * max(1,
|operands|) of the exact value may land in: the acceptance rule of the feathered tile seams (tests/tiles_feather_ref.py).  No device."""
import numpy as np

import tiles_ref as R
from tiles_feather_ref import quantise64

FEATHER_MAX = 200


def requant(v, in_depth: int, out_depth: int) -> np.ndarray:
    """Samples of `in_depth` bits at `out_depth` bits: (min(v, D_in) * 2 * D_out + D_in) // (2 * D_in), D = 2^depth - 1, in integers."""
    din, dout = R.scale_of(in_depth), R.scale_of(out_depth)
    return (np.minimum(np.asarray(v).astype(np.int64), din) * 2 * dout + din) // (2 * din)


def luma(frames, depth=8) -> np.ndarray:
    """Packed [..., 3] samples of `depth` bits (a word above D reads as D) -> the integer luma (77 R + 150 G + 29 B + 128) >> 8."""
    f = np.minimum(np.asarray(frames).astype(np.int64), R.scale_of(depth))
    return (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8


def extent(frames, depth=8):
    """Packed frames [N,H,W,3] -> (rowmax [H], colmax [W]) of the integer luma over all N frames."""
    y = luma(frames, depth)
    return y.max(axis=(0, 2)), y.max(axis=(0, 1))


def axis_weights(n: int, lo: int, hi: int, feather: int) -> np.ndarray:
    """float32 [n]: the weight of the model's output along an axis of n pixels with ramps of lo / hi pixels (0 or `feather`) inside its
    two ends: fl32(fl32(2 d + 1) * fl32(1 / (2 N))) at distance d from the end, 1 elsewhere."""
    w = np.ones(n, np.float32)
    if feather:
        ramp = (np.arange(feather, dtype=np.int64) * 2 + 1).astype(np.float32) * np.float32(1.0 / (2.0 * feather))
        assert lo + hi <= n and (ramp < 1).all()
        w[:lo] = ramp[:lo]
        w[n - hi:] = ramp[:hi][::-1]
    return w


def weights(H: int, W: int, roi, feather: int):
    """(wy float32 [h, 1], wx float32 [1, w]) of the rectangle `roi` of an H x W frame: a side on the frame's border gets no ramp."""
    y0, x0, h, w = roi
    assert 0 <= feather <= min(FEATHER_MAX, h // 2, w // 2)
    wy = axis_weights(h, feather if y0 > 0 else 0, feather if y0 + h < H else 0, feather)
    wx = axis_weights(w, feather if x0 > 0 else 0, feather if x0 + w < W else 0, feather)
    return wy[:, None], wx[None, :]


def paste(src: np.ndarray, frame: np.ndarray, roi, in_depth=8, out_depth=8, feather=0) -> dict:
    """float32 [3, hp, wp] and the packed frame [H, W, 3] -> dict of
      out    [H, W, 3] the pasted frame: `requant(frame)` outside the rectangle; inside it the egress quantisation of the model's value
             m where the weight wt = fl32(wy * wx) is 1, and of fma(wt, m - o, o) elsewhere, o = fl32(min(v, D_in) * fl32(1 / D_in)),
             0 where m is not finite,
      bad    whether a value of src inside the h x w crop is not finite,
      ramp   [H, W] the pixels with wt != 1,
      lo, hi [H, W, 3] the band of the float64 evaluation (equal to `out` off the ramps and where m is not finite)."""
    y0, x0, h, w = roi
    H, W = frame.shape[:2]
    hp, wp = R.up20(h), R.up20(w)
    assert src.shape == (3, hp, wp) and src.dtype == np.float32 and frame.shape == (H, W, 3)
    assert 0 <= y0 and 0 <= x0 and y0 + h <= H and x0 + w <= W and h >= 1 and w >= 1
    din, dout = R.scale_of(in_depth), R.scale_of(out_depth)
    dtype = np.uint8 if out_depth == 8 else np.uint16
    m = src[:, :h, :w].transpose(1, 2, 0)                                          # [h, w, 3]: the pad is never read
    fin = np.isfinite(m)
    wy, wx = weights(H, W, roi, feather)
    wt = (wy * wx)[..., None]                                                      # float32 [h, w, 1]
    o = np.minimum(frame[y0:y0 + h, x0:x0 + w].astype(np.int64), din).astype(np.float32) * np.float32(1.0 / din)
    with np.errstate(invalid="ignore", over="ignore"):
        d = m - o                                                                  # float32
        fma = (wt.astype(np.float64) * d.astype(np.float64) + o.astype(np.float64)).astype(np.float32)
    value = np.where(wt == 1, m, fma)
    inner = R.quantise(np.where(fin, value, np.float32(np.nan)), out_depth)       # 0 where m is not finite
    out = requant(frame, in_depth, out_depth).astype(dtype)
    out[y0:y0 + h, x0:x0 + w] = inner
    ramp = np.zeros((H, W), bool)
    ramp[y0:y0 + h, x0:x0 + w] = wt[..., 0] != 1
    lo, hi = out.astype(np.int64), out.astype(np.int64)
    if feather:
        m64, o64 = np.where(fin, m, 0).astype(np.float64), o.astype(np.float64)
        u = o64 + wt.astype(np.float64) * (m64 - o64)
        delta = 8.0 * 2.0 ** -24 * np.maximum.reduce([np.ones_like(u), np.abs(m64), np.abs(o64)])
        on = np.broadcast_to(wt != 1, fin.shape) & fin
        for band, edge in ((lo, u - delta), (hi, u + delta)):
            sub = band[y0:y0 + h, x0:x0 + w]
            sub[on] = quantise64(edge, dout)[on]
    return {"out": out, "bad": bool((~fin).any()), "ramp": ramp, "lo": lo, "hi": hi}
