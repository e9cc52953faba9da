"""A numpy restatement of the feathered tile stitch (spei_tiles_u8_blend / spei_tiles_u16_blend, csrc/tile_io.hip; the definition in
include/speinet_hip.h), for the tests of `deblur_clip(..., tiles=, feather=)`.  The ramps come from the plan's tables through
`tiles.seam_ramps` (the one statement of the clip rule in Python), the weights are the float32 numbers of the definition, the blend
itself is evaluated in float64, and every sample gets the band [lo, hi] that a float32 evaluation within 8 units of 2^-24 *
max(1, |operands|) of the exact value may land in.  No device."""
import numpy as np

import tiles_ref as R
from speinet_amd import tiles as T


def ramps(plan):
    """(row half-widths [rows - 1], column half-widths [cols - 1]): f_s of inner seam s = 1 .. r-1 at index s - 1."""
    return T.seam_ramps(plan)


def weights(f: int) -> np.ndarray:
    """float32 [2 f]: the weight of the high tile at p = b - f .. b + f - 1, fl32(fl32(2 (p - b + f) + 1) * fl32(1 / (4 f)))."""
    r = np.float32(1.0 / (4.0 * f))                        # double, rounded once
    return (np.arange(2 * f, dtype=np.int64) * 2 + 1).astype(np.float32) * r


def axis(n: int, b, f):
    """Per coordinate p of an axis of n pixels with band bounds b[r + 1] and half-widths f[r - 1]: (low tile [n], high tile [n],
    float32 weight of the high tile [n], in a ramp [n]).  Outside the ramps low == high == the band's owner and the weight is 0."""
    r = len(b) - 1
    lo = np.zeros(n, np.int64)
    for i in range(r):
        lo[b[i]:b[i + 1]] = i
    hi, w, inside = lo.copy(), np.zeros(n, np.float32), np.zeros(n, bool)
    for s in range(1, r):
        fs = f[s - 1]
        if fs > 0:
            sl = slice(b[s] - fs, b[s] + fs)
            assert not inside[sl].any(), "two ramps overlap"
            lo[sl], hi[sl], w[sl], inside[sl] = s - 1, s, weights(fs), True
    return lo, hi, w, inside


def corners(plan):
    """The four contributing places of every pixel, as index arrays that broadcast to [H, W]: a list of (tile k, tile row, tile column)
    for (low row, low column), (low row, high column), (high row, low column), (high row, high column), then the weights wy [H, 1],
    wx [1, W] (float32) and the ramp mask [H, W].  Outside the ramps the places coincide."""
    fy, fx = ramps(plan)
    ilo, ihi, wy, iny = axis(plan.H, plan.yb, fy)
    jlo, jhi, wx, inx = axis(plan.W, plan.xb, fx)
    y0, x0 = np.asarray(plan.y0), np.asarray(plan.x0)
    y, x = np.arange(plan.H), np.arange(plan.W)
    places = []
    for i in (ilo, ihi):
        for j in (jlo, jhi):
            ry, cx = y - y0[i], x - x0[j]
            assert (ry >= 0).all() and (ry < plan.th).all() and (cx >= 0).all() and (cx < plan.tw).all(), "a ramp leaves the real pixels"
            places.append(((i[:, None] * plan.cols + j[None, :]), np.broadcast_to(ry[:, None], (plan.H, plan.W)),
                           np.broadcast_to(cx[None, :], (plan.H, plan.W))))
    return places, wy[:, None], wx[None, :], iny[:, None] | inx[None, :]


def contributing(plan) -> np.ndarray:
    """bool [plan.n, thp, twp]: the places of each tile that some pixel of the frame is made from."""
    thp, twp = R.up20(plan.th), R.up20(plan.tw)
    m = np.zeros((plan.rows * plan.cols, thp, twp), bool)
    for k, ry, cx in corners(plan)[0]:
        m[k, ry, cx] = True
    return m


def quantise64(v: np.ndarray, D: int) -> np.ndarray:
    """float64 -> round_half_even(clamp(v * D, 0, D)) as int64."""
    return np.rint(np.clip(v * float(D), 0.0, float(D))).astype(np.int64)


def blend(tiles: np.ndarray, plan, depth=8) -> dict:
    """float32 [plan.n, 3, thp, twp] -> dict of [H, W, 3] arrays (ramp: [H, W]):
      u     the blend lerp(lerp(a, b, wx), lerp(c, d, wx), wy) in float64 with the float32 weights (0 where `bad`),
      mid   quantise64(u); lo, hi = quantise64(u - delta), quantise64(u + delta), delta = 8 * 2^-24 * max(1, |a|, |b|, |c|, |d|),
      bad   a contributing value is a NaN or an infinity: lo = mid = hi = 0 there,
      ramp  the pixel lies in a row or a column ramp."""
    D = R.scale_of(depth)
    places, wy, wx, ramp = corners(plan)
    a, b, c, d = (tiles[k, :, ry, cx].astype(np.float64) for k, ry, cx in places)          # each [H, W, 3]: the index arrays lead
    bad = ~(np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & np.isfinite(d))
    a, b, c, d = (np.where(bad, 0.0, v) for v in (a, b, c, d))
    wy, wx = wy.astype(np.float64)[..., None], wx.astype(np.float64)[..., None]
    top, bot = a + wx * (b - a), c + wx * (d - c)
    u = top + wy * (bot - top)
    delta = 8.0 * 2.0 ** -24 * np.maximum.reduce([np.ones_like(a), np.abs(a), np.abs(b), np.abs(c), np.abs(d)])
    out = {"u": u, "mid": quantise64(u, D), "lo": quantise64(u - delta, D), "hi": quantise64(u + delta, D), "bad": bad, "ramp": ramp}
    for key in ("mid", "lo", "hi"):
        out[key][bad] = 0
    return out
