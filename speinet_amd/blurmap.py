"""Automatic blur mattes (`deblur_clip(..., matte="auto")`): where in every frame is the picture blurred?  The measurement is GPU work
(csrc/blur_map.hip: `ops.blur_cells` per analysis batch, `ops.blur_matte` per matted frame); this module holds its parameters, the
host rules on cell bytes (is a matte empty, the box of `roi="matte"`), and `AutoMattes`, the matte source with the interface of
`clip.Mattes` that the clip loop reads.  An extension beyond the reference.

The definition (integers throughout; tests/blurmap_ref.py is its numpy statement).  On the luma Y = (77 R + 150 G + 29 B + 128) >> 8
at the frame's depth d, taken at the clamped index outside the frame, per pixel and direction the RE-BLUR measure: how much of the
adjacent-pixel variation a 9-tap box removes.  Horizontally D = (9 (Y(y,x) - Y(y,x-1)))^2 and V = max(0, D - (Y(y,x+4) -
Y(y,x-5))^2), the second difference being that of the box sums centred on x and x - 1; vertically alike.  The frame is cut into
cells of 16x16 pixels (edge cells partial, n pixels).  A direction of a cell is textured iff sum D >= 81 flat^2 n << 2 (d - 8),
blurred iff textured and 256 sum V < thr sum D, and the cell is lit (255) iff either direction is blurred: a horizontal motion blur
counts although vertical detail survives it.  An isolated linear edge of width w <= 5 (every box of 9 taps around one of its pixels
spans it whole) has sum V / sum D = 1 - w^2 / 81, so thr = 192 draws the line at 4.5 pixels; a wider edge has 1 - sum_j c_j^2 / (81
w) with c_j the number of its w steps inside the box of step j, which falls more slowly (0.60 at w = 6, 0.37 at w = 10).  Frame k's
cell map is the maximum of the verdict maps of the frames of plan entry k's window (`hold`; else frame k's own), dilated by `grow`
cells; its pixel matte is the bilinear interpolation between cell centres (`ops.blur_matte`), so the ramp between a lit and an unlit
cell is 16 pixels wide and reaches 8 pixels past the lit cell.

`thr`, `flat`, `grow` and `hold` are design parameters, not measurements: nobody has tuned them on footage, which is why they are
keywords (`matte_params=`).  Blind spots: grain lying on top of a blurred region reads as sharp; a defocused background is "blurred"
and gets deblurred; a cell below `flat` is never lit; interlaced clips (`fields=`) are not served."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import ops

CELL = ops.BLUR_CELL
REACH = CELL // 2                        # pixels the ramp of a lit cell reaches past the cell
MATTE_PARAMS = ("thr", "flat", "grow", "hold")     # `matte_params`: BlurParams' fields
_RANGES = {"thr": (0, 257), "flat": (0, 255), "grow": (0, ops.BLUR_GROW_MAX), "hold": (0, 1)}


@dataclass(frozen=True)
class BlurParams:
    """The four design parameters of the blur map: `thr` 0..257 (a textured direction is blurred iff 256 sum V < thr sum D; 0 lights
    nothing), `flat` 0..255 (the RMS adjacent difference, in 8-bit levels, below which a direction is not judged), `grow` 0..4 (cells
    of dilation) and `hold` 0 or 1 (join the verdicts of the frames of the plan entry's window).  Untuned defaults."""
    thr: int = 192
    flat: int = 2
    grow: int = 1
    hold: int = 1

    def __post_init__(self):
        for name, (lo, hi) in _RANGES.items():
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError(f"matte_params: {name} must be a whole number in {lo}..{hi}, got {v!r}")
            object.__setattr__(self, name, int(v))

    @staticmethod
    def of(matte_params: Optional[dict]) -> "BlurParams":
        """`matte_params` (a dict over MATTE_PARAMS, or None) as BlurParams; ValueError for an unknown key or a value out of range."""
        if matte_params is None:
            return BlurParams()
        if not isinstance(matte_params, dict):
            raise ValueError(f"matte_params must be a dict over {', '.join(MATTE_PARAMS)}, got {type(matte_params).__name__}")
        if set(matte_params) - set(MATTE_PARAMS):
            raise ValueError(f"matte_params holds {sorted(set(matte_params) - set(MATTE_PARAMS), key=str)}: it takes thr, flat, grow and hold")
        return BlurParams(**matte_params)

    def describe(self) -> str:
        return f"thr={self.thr},flat={self.flat},grow={self.grow},hold={self.hold}"


def parse_params(text: str) -> dict:
    """`--matte_params`: 'thr=192,flat=2' -> dict(thr=192, flat=2).  ValueError with the reason; the values are checked by BlurParams."""
    out = {}
    for part in text.split(","):
        name, eq, value = part.partition("=")
        name, value = name.strip(), value.strip()
        if not eq or name not in MATTE_PARAMS or not value.lstrip("+-").isdigit():
            raise ValueError(f"{part!r} is not NAME=N with NAME one of {', '.join(MATTE_PARAMS)} and N a whole number")
        if name in out:
            raise ValueError(f"{name} is given twice")
        out[name] = int(value)
    return out


cell_shape = ops.blur_cell_shape


def lit(cells) -> bool:
    """Does a verdict map (or a stack of them) hold a lit cell?"""
    return bool(np.asarray(cells).any())


def empty(cells, window, hold: int, k: int) -> bool:
    """Is frame k's matte 0 everywhere?  `cells`: the verdict maps by frame; `window`: the frames of plan entry k.  Its cell map is the
    dilated maximum of its window's maps (its own without `hold`), a dilation lights a cell only beside a lit one, and a lit cell has
    m > 0 at its centre: so the matte is empty iff none of those maps holds a lit cell."""
    return not any(lit(cells[f]) for f in (set(window) if hold else (k,)))


def cell_box(cells, H: int, W: int, grow: int):
    """The half-open pixel box (ya, yb, xa, xb) of `roi="matte"` from the verdict maps of every frame [T,ch,cw]: around every non-zero
    cell of every frame's cell map, moved out by 8 pixels on each side (as far as the ramp reaches) and clamped.  Every frame lies in
    its own window and a dilation moves a bounding box out by `grow` cells, so the box of all cell maps is that of all verdict maps
    grown by `grow` cells, with or without the hold.  None when no cell is lit."""
    c = np.asarray(cells)
    ch, cw = c.shape[-2:]
    on = (c.reshape(-1, ch, cw) != 0).any(0)
    if not on.any():
        return None
    ys, xs = np.flatnonzero(on.any(1)), np.flatnonzero(on.any(0))
    i0, i1 = max(0, int(ys[0]) - grow), min(ch - 1, int(ys[-1]) + grow)
    j0, j1 = max(0, int(xs[0]) - grow), min(cw - 1, int(xs[-1]) + grow)
    return max(0, CELL * i0 - REACH), min(H, CELL * (i1 + 1) + REACH), max(0, CELL * j0 - REACH), min(W, CELL * (j1 + 1) + REACH)


class AutoMattes:
    """The matte source behind `matte="auto"`, with the interface of `clip.Mattes`: one matte per frame (`static` False), made on the
    device (`on_device` True).  `feed(i0, maps)` takes the verdict maps of an analysis batch (`detector.clip_analysis(..., blur=)`:
    uint8 [n,ch,cw] on the device) and brings their bytes to the host, once per batch; `cells` holds them as a host uint8 [T,ch,cw]
    array, as far as the analysis has come.  `device(i)` runs `ops.blur_matte` on the verdict maps of plan entry i's window (frame i's
    alone without `hold`), `empty(i)` and `bbox()` decide from the cell bytes on the host, with no sync per frame.  A whole clip that
    nobody has measured by the time a matte is asked for (labels and cuts were given, or the labelling pass saw a region of
    interest) is measured then, in one `detector.clip_batches` pass of its own over the full frames: one more upload of a host clip.
    `bind(run)` ties it to its `video.ClipRun`, whose frames it measures and whose plan entries name the windows."""
    static, invert, kind = False, False, "auto"

    def __init__(self, params: BlurParams, H: int, W: int):
        self.params, self.H, self.W = params, H, W
        self.ch, self.cw = cell_shape(H, W)
        self.run = None
        self._host = []                  # per batch: host uint8 [n,ch,cw]
        self._dev = []                   # per batch: (first frame, device uint8 [n,ch,cw]); a stream gives up those long behind
        self._lit = []                   # per frame: does its verdict map hold a lit cell
        self.fed = 0

    def bind(self, run) -> None:
        self.run = run

    @property
    def T(self) -> Optional[int]:
        T = self.run.frames.T
        return self.fed if T is None else T

    @property
    def cells(self) -> np.ndarray:
        return np.concatenate(self._host) if self._host else np.zeros((0, self.ch, self.cw), np.uint8)

    def describe(self) -> str:
        return f"{self.params.describe()}, cells of {CELL}x{CELL}: a grid of {self.cw}x{self.ch} for {self.W}x{self.H}"

    def key(self, i: int) -> int:
        return i

    def on_device(self, i: int) -> bool:
        return True

    def prefetch(self, pool, indices) -> None:
        """Nothing to decode: the mattes are made on the device."""

    def feed(self, i0: int, maps: torch.Tensor) -> None:
        assert i0 == self.fed and tuple(maps.shape[1:]) == (self.ch, self.cw)
        host = maps.cpu().numpy()                          # the verdict bytes come to the host once per batch
        self._host.append(host)
        self._dev.append((i0, maps))
        self._lit += [lit(m) for m in host]
        self.fed += len(host)

    def measure(self) -> None:
        """The pass of its own, over the full frames of a clip whose length is known, if no analysis pass has fed the cells."""
        run = self.run
        if self.fed or run.horizon is not None:          # fed already; or a stream, whose analysis feeds the cells as it goes
            return
        from . import detector
        with torch.no_grad(), torch.cuda.device(run.device):
            for i0, _, _, maps in detector.clip_analysis(run.frames, run.device, features=False, pair_stats=False, blur=self.params):
                self.feed(i0, maps)

    def _window(self, i: int) -> list:
        return sorted(set(self.run.plan[i]["window"])) if self.params.hold else [i]

    def empty(self, i: int) -> bool:
        self.measure()
        return not any(self._lit[f] for f in self._window(i))

    def bbox(self, grow: Optional[int] = None):
        """The rectangle (y0, x0, h, w) of `roi="matte"`: `cell_box` of every frame's cells through `clip.grow_box`; None: all empty."""
        from .clip import MATTE_GROW, grow_box
        self.measure()
        return grow_box(cell_box(self.cells, self.H, self.W, self.params.grow), self.H, self.W, MATTE_GROW if grow is None else grow)

    def _maps(self, frames: list) -> torch.Tensor:
        """The verdict maps of `frames` (increasing) as one device tensor [n,ch,cw]: a slice of a batch's where they are neighbours in
        one batch, gathered otherwise."""
        rows = []
        for f in frames:
            i0, t = next((i0, t) for i0, t in reversed(self._dev) if i0 <= f)
            rows.append((i0, t, f - i0))
        if all(r[0] == rows[0][0] for r in rows) and [r[2] for r in rows] == list(range(rows[0][2], rows[0][2] + len(rows))):
            return rows[0][1][rows[0][2]:rows[0][2] + len(rows)]
        return torch.stack([t[j] for _, t, j in rows])

    def device(self, i: int) -> torch.Tensor:
        self.measure()
        frames = self._window(i)
        if self.run.horizon is not None:                   # a stream: no later window reaches back to the batches long behind this one
            while len(self._dev) > 1 and self._dev[1][0] <= frames[0] - 8:
                self._dev.pop(0)
        return ops.blur_matte(self._maps(frames), self.H, self.W, self.params.grow)

    def host(self, i: int) -> np.ndarray:
        return self.device(i).cpu().numpy()
