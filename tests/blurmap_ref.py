"""The numpy statement of the clip API's automatic blur mattes (`deblur_clip(..., matte="auto")`, csrc/blur_map.hip,
speinet_amd/blurmap.py): the re-blur measure per cell, the verdict, the hold and the dilation, the integer bilinear expansion, and
the rules for an empty matte and for the box of `roi="matte"`.  Integers throughout; the kernels match it bit for bit."""
import numpy as np

CELL = 16
REACH = 8                                # pixels the ramp of a lit cell reaches past the cell


def cell_shape(H: int, W: int):
    return (H + CELL - 1) // CELL, (W + CELL - 1) // CELL


def luma(frame, depth: int = 8) -> np.ndarray:
    """[..., H, W, 3] samples -> the integer luma (77 R + 150 G + 29 B + 128) >> 8 as int64; a word above D = 2^depth - 1 reads as D."""
    f = np.minimum(np.asarray(frame).astype(np.int64), (1 << depth) - 1)
    return (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8


def _shift(Y, dy: int, dx: int) -> np.ndarray:
    """Y(y + dy, x + dx) at the clamped index."""
    H, W = Y.shape
    yi = np.clip(np.arange(H) + dy, 0, H - 1)
    xi = np.clip(np.arange(W) + dx, 0, W - 1)
    return Y[yi][:, xi]


def pixel_terms(Y):
    """Y int64 [H,W] -> (D_h, V_h, D_v, V_v), int64 [H,W] each."""
    out = []
    for (ay, ax) in ((0, 1), (1, 0)):
        d = 9 * (Y - _shift(Y, -ay, -ax))
        b = _shift(Y, 4 * ay, 4 * ax) - _shift(Y, -5 * ay, -5 * ax)
        out += [d * d, np.maximum(0, d * d - b * b)]
    return tuple(out)


def cell_sums(frame, depth: int = 8) -> np.ndarray:
    """One frame [H,W,3] -> int64 [ch,cw,4]: (sum D_h, sum V_h, sum D_v, sum V_v) over the pixels of every cell."""
    Y = luma(frame, depth)
    H, W = Y.shape
    ch, cw = cell_shape(H, W)
    S = np.zeros((ch, cw, 4), np.int64)
    for k, t in enumerate(pixel_terms(Y)):
        pad = np.zeros((ch * CELL, cw * CELL), np.int64)
        pad[:H, :W] = t
        S[..., k] = pad.reshape(ch, CELL, cw, CELL).sum((1, 3))
    return S


def cell_pixels(H: int, W: int) -> np.ndarray:
    """int64 [ch,cw]: the number of pixels of every cell."""
    ch, cw = cell_shape(H, W)
    hs = np.minimum(CELL, H - CELL * np.arange(ch))
    ws = np.minimum(CELL, W - CELL * np.arange(cw))
    return hs[:, None].astype(np.int64) * ws[None, :]


def verdict(S, H: int, W: int, depth: int = 8, thr: int = 192, flat: int = 2) -> np.ndarray:
    """The sums [ch,cw,4] of an H x W frame -> uint8 [ch,cw], 255 where either direction is blurred."""
    S = np.asarray(S).astype(np.int64)
    floor = (81 * flat * flat * cell_pixels(H, W)) << (2 * (depth - 8))
    lit = np.zeros(S.shape[:2], bool)
    for k in (0, 2):
        D, V = S[..., k], S[..., k + 1]
        lit |= (D >= floor) & (256 * V < thr * D)
    return np.where(lit, 255, 0).astype(np.uint8)


def cells_of(frames, depth: int = 8, thr: int = 192, flat: int = 2):
    """[N,H,W,3] -> (cells uint8 [N,ch,cw], sums int64 [N,ch,cw,4])."""
    frames = np.asarray(frames)
    H, W = frames.shape[1:3]
    S = np.stack([cell_sums(f, depth) for f in frames])
    return np.stack([verdict(s, H, W, depth, thr, flat) for s in S]), S


def dilate(c, grow: int) -> np.ndarray:
    """[ch,cw] -> the maximum over a (2 grow + 1)^2 neighbourhood, zeros outside."""
    c = np.asarray(c)
    ch, cw = c.shape
    pad = np.zeros((ch + 2 * grow, cw + 2 * grow), c.dtype)
    pad[grow:grow + ch, grow:grow + cw] = c
    out = np.zeros_like(c)
    for p in range(2 * grow + 1):
        for q in range(2 * grow + 1):
            out = np.maximum(out, pad[p:p + ch, q:q + cw])
    return out


def cell_map(maps, grow: int = 1) -> np.ndarray:
    """Verdict maps [n,ch,cw] -> the held (their maximum) and dilated cell map [ch,cw]."""
    return dilate(np.asarray(maps).max(0), grow)


def _axis(n: int, nc: int):
    u = 2 * np.arange(n) + 17
    i0 = u // 32 - 1
    return np.clip(i0, 0, nc - 1), np.clip(i0 + 1, 0, nc - 1), u % 32


def expand(c, H: int, W: int) -> np.ndarray:
    """A cell map [ch,cw] -> the pixel matte uint8 [H,W]: bilinear between cell centres, in exact integers."""
    c = np.asarray(c).astype(np.int64)
    i0, i1, wy = _axis(H, c.shape[0])
    j0, j1, wx = _axis(W, c.shape[1])
    wy, wx = wy[:, None], wx[None, :]
    m = ((32 - wy) * (32 - wx) * c[i0][:, j0] + (32 - wy) * wx * c[i0][:, j1] + wy * (32 - wx) * c[i1][:, j0] + wy * wx * c[i1][:, j1]
         + 512) // 1024
    return m.astype(np.uint8)


def matte_of(maps, H: int, W: int, grow: int = 1) -> np.ndarray:
    return expand(cell_map(maps, grow), H, W)


def clip_mattes(cells, plan, H: int, W: int, grow: int = 1, hold: int = 1) -> np.ndarray:
    """The verdict maps of a clip [T,ch,cw] and its window plan (`plan[k]["window"]`: the frames window k reads) -> the mattes
    [T,H,W]: frame k's from the maps of its window's frames under `hold`, from its own otherwise."""
    cells = np.asarray(cells)
    return np.stack([matte_of(cells[sorted(set(plan[k]["window"]))] if hold else cells[k:k + 1], H, W, grow) for k in range(len(cells))])


def clip_cell_maps(cells, plan, grow: int = 1, hold: int = 1) -> np.ndarray:
    cells = np.asarray(cells)
    return np.stack([cell_map(cells[sorted(set(plan[k]["window"]))] if hold else cells[k:k + 1], grow) for k in range(len(cells))])


def empty(cmap) -> bool:
    """Is the matte of this (held and dilated) cell map 0 everywhere?  A lit cell has m > 0 at its centre."""
    return not np.asarray(cmap).any()


def cell_box(cmaps, H: int, W: int):
    """Cell maps [T,ch,cw] (or [ch,cw]) -> the half-open pixel box (ya, yb, xa, xb) around every non-zero cell, moved out by 8 pixels
    on each side and clamped; None when no cell is lit."""
    c = np.asarray(cmaps)
    lit = (c.reshape(-1, *c.shape[-2:]) != 0).any(0)
    if not lit.any():
        return None
    ys, xs = np.flatnonzero(lit.any(1)), np.flatnonzero(lit.any(0))
    return (max(0, CELL * int(ys[0]) - REACH), min(H, CELL * (int(ys[-1]) + 1) + REACH),
            max(0, CELL * int(xs[0]) - REACH), min(W, CELL * (int(xs[-1]) + 1) + REACH))


def box9(frame, axis: int = 1) -> np.ndarray:
    """A frame through a 9-tap box along `axis` (edge-clamped), rounded half up: the blur of the tests' scenes."""
    f = np.asarray(frame)
    a = np.moveaxis(f.astype(np.int64), axis, 0)
    n = a.shape[0]
    acc = sum(a[np.clip(np.arange(n) + k, 0, n - 1)] for k in range(-4, 5))
    return np.moveaxis((acc + 4) // 9, 0, axis).astype(f.dtype)
