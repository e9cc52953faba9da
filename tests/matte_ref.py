"""The numpy statement of the clip API's mattes (`deblur_clip(..., matte=)`, csrc/matte_io.hip): the blend of the input frame with the
deblurred one in exact integers, and the region of interest that `roi="matte"` takes from the mattes."""
import numpy as np

GROW = 20                                # the project's `shave` default
LEAST = 20                               # the smallest frame (and rectangle) the clip API takes


def blend(a, b, m, invert: bool = False) -> np.ndarray:
    """a: the input samples at the output depth [..., H, W, 3]; b: the deblurred samples there, already clamped to D_out; m: the
    matte bytes [..., H, W] -> (a * (255 - m) + b * m + 127) // 255 in int64, with 255 - m for m under `invert`."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    m = np.asarray(m).astype(np.int64)[..., None]
    if invert:
        m = 255 - m
    return (a * (255 - m) + b * m + 127) // 255


def bbox(mattes, H: int, W: int, grow: int = GROW, least: int = LEAST):
    """mattes: [T,H,W] or [H,W], as in effect (inverted already) -> the rectangle (y0, x0, h, w): the bounding box of the non-zero
    samples of all of them, grown by `grow` on every side, then symmetrically to at least `least` per axis (an odd pixel at the far
    side), then clamped to the frame; an axis the clamp left shorter than `least` reaches `least` pixels from the frame edge it lies on.
    None when every sample is zero."""
    m = np.asarray(mattes).reshape(-1, H, W)
    lit = (m != 0).any(0)
    if not lit.any():
        return None
    out = []
    for line, n in ((lit.any(1), H), (lit.any(0), W)):
        at = np.flatnonzero(line)
        lo, hi = int(at[0]) - grow, int(at[-1]) + 1 + grow
        if hi - lo < least:
            d = least - (hi - lo)
            lo, hi = lo - d // 2, hi + (d - d // 2)
        lo, hi = max(lo, 0), min(hi, n)
        if hi - lo < least:
            lo, hi = (0, min(n, least)) if lo == 0 else (max(0, hi - least), hi)
        out.append((lo, hi - lo))
    return out[0][0], out[1][0], out[0][1], out[1][1]
