"""The tile plan of the clip API's large-frame mode (`video.deblur_clip(..., tiles=)`): a frame cut into a grid of overlapping tiles of
ONE shape, each run through the net on its own, the results stitched with hard seams (or, with `feather`, blended over a ramp around
every seam: `seam_ramps`).  The reference's `forward_chop`
(inference_SPEINet.py:545-607, trainer/trainer_swint_hsa_nsf.py:96) is the 2x2 case: four quadrants that overlap by `shave` = 20
pixels, seams at h // 2 and w // 2, recursion while a piece has 6 * 160000 pixels or more (`MAX_TILE_PIXELS`).

Pure host arithmetic: nothing here touches a device.  Per axis of n pixels cut into r bands:
  * band i owns [b[i], b[i+1]) with b[i] = (i * n) // r; with r > 1 every band is at least max(40, 2 * shave) pixels;
  * the tile length t is the longest band grown by `shave` on both sides (clipped to the frame), rounded up to a multiple of 20: the
    same for every tile of the axis, so one set of captured graphs serves the whole grid;
  * t >= n: the tile spans the axis (t = n, every origin 0) and the ingest pads it to the next multiple of 20 by reflection, as the
    untiled path does;
  * otherwise tile i starts at min(max(b[i] - shave, 0), n - t): a tile at the far edge slides inward and sees real pixels instead of
    a reflected pad.
Every tile then lies inside the frame, every band inside its tile, with at least `shave` pixels of margin on every side that is not a
frame edge.  For r = 2 and n a multiple of 40 these are the reference's slices."""
from __future__ import annotations

import dataclasses
from typing import Optional, Tuple, Union

MULT = 20                        # the model's frame sizes are multiples of 20 (ops.padded_size)
MAX_GRID = 8                     # rows, cols <= 8: the tile tables travel to the kernels by value (csrc/tile_io.hip)
MAX_SHAVE = 200
MIN_BAND = 40
MAX_TILE_PIXELS = 6 * 160000     # the reference's recursion threshold (inference_SPEINet.py:545, min_size=160000 times 6)


def up20(n: int) -> int:
    return -(-n // MULT) * MULT


@dataclasses.dataclass(frozen=True)
class TilePlan:
    """A grid of rows x cols tiles of th x tw pixels on an H x W frame: tile (i, j) covers [y0[i], y0[i] + th) x [x0[j], x0[j] + tw) and
    owns the band [yb[i], yb[i+1]) x [xb[j], xb[j+1]) of the output.  Tile k = i * cols + j."""
    H: int
    W: int
    rows: int
    cols: int
    th: int
    tw: int
    y0: Tuple[int, ...]
    x0: Tuple[int, ...]
    yb: Tuple[int, ...]
    xb: Tuple[int, ...]
    shave: int = 20
    feather: int = 0                 # half-width of the blend ramp around every inner seam (0: hard seams); see `seam_ramps`

    @property
    def n(self) -> int:
        return self.rows * self.cols

    @property
    def padded(self) -> Tuple[int, int]:
        """The tile's size in the model: (th, tw) rounded up to multiples of 20."""
        return up20(self.th), up20(self.tw)


def axis_plan(n: int, r: int, shave: int = 20):
    """One axis of n pixels in r bands: (tile length, origins [r], band bounds [r + 1]).  Raises ValueError with the reason."""
    if not 1 <= r <= MAX_GRID:
        raise ValueError(f"a tile grid has 1..{MAX_GRID} rows and columns, got {r}")
    if not 0 <= shave <= MAX_SHAVE:
        raise ValueError(f"shave must be 0..{MAX_SHAVE}, got {shave}")
    if n < 1:
        raise ValueError(f"an axis of {n} pixels cannot be tiled")
    b = [(i * n) // r for i in range(r + 1)]
    if r > 1:
        need = max(MIN_BAND, 2 * shave)
        small = min(b[i + 1] - b[i] for i in range(r))
        if small < need:
            raise ValueError(f"{n} pixels in {r} bands leave a band of {small}: with shave {shave} a band needs at least {need}")
    t = up20(max(min(b[i + 1] + shave, n) - max(b[i] - shave, 0) for i in range(r)))
    if t >= n:
        return n, [0] * r, b
    return t, [min(max(b[i] - shave, 0), n - t) for i in range(r)], b


def _auto(H: int, W: int, shave: int):
    if H * W <= MAX_TILE_PIXELS:
        return 1, 1
    best = None
    for r in range(1, MAX_GRID + 1):
        for c in range(1, MAX_GRID + 1):
            try:
                th, tw = axis_plan(H, r, shave)[0], axis_plan(W, c, shave)[0]
            except ValueError:
                continue
            if th * tw <= MAX_TILE_PIXELS:
                rank = (r * c, abs(th - tw), r)
                if best is None or rank < best[0]:
                    best = (rank, r, c)
    if best is None:
        raise ValueError(f"no grid of up to {MAX_GRID}x{MAX_GRID} tiles brings a {W}x{H} frame down to tiles of {MAX_TILE_PIXELS} "
                         f"pixels with shave {shave}")
    return best[1], best[2]


def tile_plan(H: int, W: int, tiles: Union[str, Tuple[int, int]], shave: int = 20, feather: int = 0) -> TilePlan:
    """The plan for an H x W frame.  `tiles`: (rows, cols), 1..8 each, or "auto": a 1x1 grid for a frame of at most MAX_TILE_PIXELS
    pixels, otherwise the grid of the fewest tiles whose tile has at most that many (ties: the squarer tile, then fewer rows).  `shave`
    (0..200): the margin a tile keeps around the band it owns.  `feather` (0..shave): the half-width of the ramp over which the
    egress blends the two tiles of a seam (0: hard seams); within the margin every seam gets the whole of it (`seam_ramps`).  Raises
    ValueError with the reason."""
    if isinstance(shave, bool) or not isinstance(shave, int) or not 0 <= shave <= MAX_SHAVE:
        raise ValueError(f"shave must be a whole number 0..{MAX_SHAVE}, got {shave!r}")
    if isinstance(feather, bool) or not isinstance(feather, int) or not 0 <= feather <= shave:
        raise ValueError(f"feather must be a whole number 0..shave ({shave}): the ramp is blended from the margin the tiles keep, "
                         f"got {feather!r}")
    if isinstance(H, bool) or isinstance(W, bool) or not isinstance(H, int) or not isinstance(W, int) or H < 1 or W < 1:
        raise ValueError(f"a frame is H x W pixels, got {H!r} x {W!r}")
    if isinstance(tiles, str):
        if tiles != "auto":
            raise ValueError(f"tiles must be (rows, cols) or \"auto\", got {tiles!r}")
        rows, cols = _auto(H, W, shave)
    else:
        try:
            rows, cols = tiles
        except (TypeError, ValueError):
            raise ValueError(f"tiles must be (rows, cols) or \"auto\", got {tiles!r}") from None
        for v in (rows, cols):
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= MAX_GRID:
                raise ValueError(f"a tile grid has 1..{MAX_GRID} rows and columns, got {tiles!r}")
    th, y0, yb = axis_plan(H, rows, shave)
    tw, x0, xb = axis_plan(W, cols, shave)
    return TilePlan(H, W, rows, cols, th, tw, tuple(y0), tuple(x0), tuple(yb), tuple(xb), shave, feather)


def axis_ramps(o, b, t: int, feather: int) -> Tuple[int, ...]:
    """The half-widths f_s of the inner seams s = 1 .. r-1 of one axis: origins o[r], band bounds b[r + 1], real tile length t.  The
    ramp [b[s] - f_s, b[s] + f_s) lies inside the real pixels [o, o + t) of the low tile s-1 and the high tile s (never in a reflect
    pad) and inside the two bands next to the seam: a band with a seam on both sides gives each at most half of itself, a band at
    the frame's edge all of itself, so the ramps of an axis never overlap and none leaves the frame:
        f_s = max(0, min(feather, b[s] - o[s], o[s-1] + t - b[s],
                         (b[s] - b[s-1]) // 2 where s > 1, else b[1] - b[0];  (b[s+1] - b[s]) // 2 where s < r-1, else b[r] - b[r-1]))
    (and b[s] - o[s-1], o[s] + t - b[s], which bind only in a hand-made table whose origins do not increase).  0 is a hard seam.  The
    rule of include/speinet_hip.h, which csrc/tile_io.hip applies to the tables it is given."""
    r = len(o)
    out = []
    for s in range(1, r):
        f = min(feather, *(v for k in (s - 1, s) for v in (b[s] - o[k], o[k] + t - b[s])))
        f = min(f, (b[s] - b[s - 1]) // 2 if s > 1 else b[s] - b[s - 1])
        f = min(f, (b[s + 1] - b[s]) // 2 if s < r - 1 else b[s + 1] - b[s])
        out.append(max(f, 0))
    return tuple(out)


def seam_ramps(plan) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """(row half-widths [rows - 1], column half-widths [cols - 1]) of the blend ramps of `plan` (a `TilePlan`, or anything with its
    fields; no `feather` field means 0).  For every plan of `tile_plan` each is `plan.feather`: every band is at least 2 * shave
    pixels and every inner seam has shave pixels of margin on both sides."""
    f = int(getattr(plan, "feather", 0))
    return axis_ramps(plan.y0, plan.yb, plan.th, f), axis_ramps(plan.x0, plan.xb, plan.tw, f)


def parse_tiles(text: str) -> Optional[Union[str, Tuple[int, int]]]:
    """The command line's `none | auto | RxC` -> None, "auto" or (R, C).  Raises ValueError with the reason."""
    s = str(text).strip().lower()
    if s == "none":
        return None
    if s == "auto":
        return "auto"
    r, sep, c = s.partition("x")
    if not sep or not r.isdigit() or not c.isdigit():
        raise ValueError(f"tiles must be none, auto or RxC (rows x columns, such as 2x2), got {text!r}")
    return int(r), int(c)
