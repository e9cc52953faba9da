"""A numpy restatement of the tile ingest and the tile stitch (csrc/tile_io.hip; the definitions in include/speinet_hip.h), for the
tests of the clip API's large-frame mode.  Plain float32 arithmetic, one rounding per step, no device."""
import numpy as np


def up20(n: int) -> int:
    return -(-n // 20) * 20


def reflect_index(n: int, n_pad: int) -> np.ndarray:
    """Source index of each of n_pad padded positions of an axis of n: i < n reads i, n + j reads n - 2 - j (torch "reflect")."""
    assert n_pad - n < n
    i = np.arange(n_pad)
    return np.where(i < n, i, 2 * n - 2 - i)


def scale_of(depth) -> int:
    return 255 if depth in (None, 8) else (1 << depth) - 1


def ingest(frame: np.ndarray, plan, depth=None) -> np.ndarray:
    """Packed [H,W,3] uint8 (or uint16 of `depth` bits) -> float32 [plan.n, 3, thp, twp]: tile k = i * cols + j is the crop at
    (y0[i], x0[j]) of th x tw pixels, each sample min(v, D) * float32(1 / D), reflect-padded at the bottom and right to multiples
    of 20."""
    D = scale_of(depth)
    assert frame.shape == (plan.H, plan.W, 3)
    thp, twp = up20(plan.th), up20(plan.tw)
    ry, rx = reflect_index(plan.th, thp), reflect_index(plan.tw, twp)
    out = np.empty((plan.rows * plan.cols, 3, thp, twp), np.float32)
    for i in range(plan.rows):
        for j in range(plan.cols):
            crop = frame[plan.y0[i]:plan.y0[i] + plan.th, plan.x0[j]:plan.x0[j] + plan.tw]
            assert crop.shape == (plan.th, plan.tw, 3), "a tile leaves the frame"
            v = np.minimum(crop.astype(np.int64), D).astype(np.float32) * np.float32(1.0 / D)
            out[i * plan.cols + j] = v[ry][:, rx].transpose(2, 0, 1)
    return out


def quantise(x: np.ndarray, depth=8) -> np.ndarray:
    """float32 -> round_half_even(clamp(x * D, 0, D)) in float32, 0 for a non-finite value; uint8 for depth 8, else uint16."""
    D = np.float32(scale_of(depth))
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.rint(np.minimum(np.maximum(x.astype(np.float32) * D, np.float32(0)), D))
    q = np.where(np.isfinite(x), q, np.float32(0))
    return q.astype(np.uint8 if depth == 8 else np.uint16)


def owned(plan) -> np.ndarray:
    """bool [plan.n, thp, twp]: the pixels of each tile that lie in the band the tile owns."""
    thp, twp = up20(plan.th), up20(plan.tw)
    m = np.zeros((plan.rows * plan.cols, thp, twp), bool)
    for i in range(plan.rows):
        for j in range(plan.cols):
            m[i * plan.cols + j, plan.yb[i] - plan.y0[i]:plan.yb[i + 1] - plan.y0[i], plan.xb[j] - plan.x0[j]:plan.xb[j + 1] - plan.x0[j]] = True
    return m


def stitch(tiles, plan) -> np.ndarray:
    """Tiles as packed frames [plan.n][>= th, >= tw, 3] (any dtype) -> [H,W,3]: band (i, j) is copied from tile i * cols + j.  Hard
    seams."""
    t0 = np.asarray(tiles[0])
    out = np.empty((plan.H, plan.W, 3), t0.dtype)
    for i in range(plan.rows):
        for j in range(plan.cols):
            t = np.asarray(tiles[i * plan.cols + j])
            out[plan.yb[i]:plan.yb[i + 1], plan.xb[j]:plan.xb[j + 1]] = t[plan.yb[i] - plan.y0[i]:plan.yb[i + 1] - plan.y0[i],
                                                                            plan.xb[j] - plan.x0[j]:plan.xb[j + 1] - plan.x0[j]]
    return out


def egress(tiles: np.ndarray, plan, depth=8):
    """float32 [plan.n, 3, thp, twp] -> (the stitched frame [H,W,3] of `quantise`d values, whether an owned value was non-finite)."""
    frame = stitch([quantise(t, depth).transpose(1, 2, 0) for t in tiles], plan)
    bad = bool((~np.isfinite(tiles) & owned(plan)[:, None]).any())
    return frame, bad
