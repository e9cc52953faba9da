"""Codec artefacts in blur synthesis (blurset.py, data.SharpTrainLoader; csrc/codec.hip): a JPEG-style round trip — YCbCr 4:2:0, 8x8 DCT,
quantisation by quality-scaled tables, dequantisation, inverse DCT, back to RGB — on the INPUT frames of the synthesis, as the last
link of exposure -> shake -> noise -> codec.  It runs on the final encoded bytes, after the average, the shake, the noise and the
encode, so it needs no linear light and works with the light `code` too.  Ground truth is never coded.  Every frame under `blur/`
(sharp-labelled ones included) and every input record of a training batch (reference frames included) is coded.  Everything is int32,
`>>` floors, and the result is defined bit for bit.  No entropy coding happens: nothing is lost in it.

THE MCU GRID.  MCUs are 16 x 16 pixels.  One corner of the grid sits at (-oy, -ox) of the frame or rectangle, 0 <= oy, ox < 16.  A sample
outside the frame or rectangle is the nearest one inside (coordinates clamp, as an encoder pads a frame that is no multiple of 16).  An
MCU reads and writes only its own pixels: the whole-frame pass is in place.

COLOUR.  JFIF is BT.601 full range: the Q14 constants of csrc/yuv_io.hip's `601 full` row and its CENTER 4:2:0 rule.  Per pixel
Y = (4899 R + 9617 G + 1868 B + 2^13) >> 14 (0..255); per 2 x 2 cell of the MCU, on the channel sums S_c,
Cb = clip(((-2765 S_R - 5427 S_G + 8192 S_B + 2^15) >> 16) + 128, 0, 255) and Cr likewise with (8192, -6860, -1332).  On the way back chroma
is REPLICATED, U16 = 16 Cb[y >> 1][x >> 1], with no bilinear taps (an MCU stays self-contained), then yuv_io.hip's inverse: yy = 262144 Y,
u = U16 - 2048, v = V16 - 2048, R = clip((yy + 22970 v + 2^17) >> 18), G = clip((yy - 5638 u - 11700 v + 2^17) >> 18),
B = clip((yy + 29032 u + 2^17) >> 18), clipped to 0..255.  Every intermediate stays below 1.3e8.

THE TRANSFORM.  D[u][x] = rint(8192 a(u) cos((2x + 1) u pi / 16)), a(0) = sqrt(1/8), a(u > 0) = 1/2: the literal table `D` below.  The
largest sum of |D| over a row is 23168, over a column 21641.  Per 8 x 8 block (four of Y, one of Cb, one of Cr per MCU) of samples
s = value - 128, |s| <= 128:

    forward rows     T[y][u] = (sum_x D[u][x] s[y][x] + 2^9) >> 10          |sum| <= 2 965 504,   |T| <= 2896
    forward columns  F[v][u] = (sum_y D[v][y] T[y][u] + 2^12) >> 13         |sum| <= 67 094 528,  |F| <= 8190: the coefficient in Q3
    quantise         q = sign(F) ((|F| + 4 Q) / (8 Q)), truncating division: halves round away from zero
    dequantise       G = q Q                                                 |G| <= (8190 + 4 * 255) / 8 = 1151
    inverse columns  U[y][u] = (sum_v D[v][y] G[v][u] + 2^9) >> 10          |sum| <= 24 908 791,  |U| <= 24325
    inverse rows     r[y][x] = (sum_u D[u][x] U[y][u] + 2^15) >> 16         |sum| <= 526 417 325 < 2^29
    sample           clip(r + 128, 0, 255)

so every sum fits int32 with room to spare; tests/codec_ref.py asserts these bounds in int64.  Measured on the fixed inputs of
tests/test_codec_cpu.py (a smooth pattern, that pattern with noise, saturated checker edges, uniform noise, an odd 37 x 51 frame;
qualities 10, 30, 50, 75, 90, 100): F / 8 lies within 0.25 of the float64 orthonormal DCT before quantisation, and the PSNR to the source
of this integer pipeline lies within 0.66 dB of the same pipeline in float64 — that largest gap at quality 100 on the smooth pattern,
49.9 dB against 50.6 dB, where every table entry is 1 and the transform's own rounding is all the loss there is; below quality 100 the
gap is at most 0.08 dB.  Against PIL's JPEG at the same quality with subsampling=2 the PSNR to the source lies between 0.53 dB below
and 0.37 dB above.  Single pixels differ from float64 by tens of levels wherever a coefficient sits on a rounding boundary.

THE TABLES.  Base tables: the luminance and chrominance tables of ITU-T T.81 Annex K (`BASE`).  Scaling: libjpeg's rule — for a quality
q in 1..100, scale = 5000 // q if q < 50 else 200 - 2 q, Q = clamp((base scale + 50) // 100, 1, 255).  `quant_tables(q)` -> uint16 [2][64],
luma then chroma, row-major [v][u].

THE QUALITY.  Spec "<q>" or "<lo>..<hi>", integers with 1 <= lo <= hi <= 100.  One quality per clip and seed (a clip is encoded at one
setting): q = lo + floor((hi - lo + 1) w0 / 2^32), w0 the first word of light.philox on the counter (0xffffffff, 0xfffffffd, 0, clip)
under light.key_of(seed).  Row 0xfffffffd is no pixel's (rows are below 2^24), 0xffffffff is the noise levels', 0xfffffffe the PSFs'.  The
plan's random.Random stream is not touched: blurset.plan_dataset gives the same plan with and without a codec.

THE TRAINING CROP.  spei_train_batch_codec_f32 runs on the P x P rectangle in SOURCE orientation with oy = y0 % 16, ox = x0 % 16, so the
grid is the FULL frame's: every MCU that lies wholly inside the crop equals the whole-frame pass on the synthesised frame bit for bit.
The partial MCUs on the crop's border ring differ: they replicate the CROP's edge, not the frame's real neighbours.  This is the one
place where a training crop is not the crop of `blurset`'s frame.

The range of qualities and the JPEG proxy itself (no entropy coding, no inter-frame prediction, no deblocking filter, 4:2:0 only) are
UNTUNED, and no model has been trained with them here.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional, Tuple

import numpy as np

from . import light as _light

MCU = 16
ROW = 0xfffffffd                                     # the counter row of the quality draw
SKIP = 16                                            # SPEI_CODEC_SKIP: the record's frame is left alone
# spei_codec_record
CODEC_RECORD = np.dtype([("qtab", "<u4"), ("oy", "<u4"), ("ox", "<u4"), ("flags", "<u4")])
assert CODEC_RECORD.itemsize == 16
# the codec of one clip for blurset.synthesize: its spec, write_dataset's seed and the clip's index
ClipCodec = namedtuple("ClipCodec", "spec seed clip")

# rint(8192 a(u) cos((2x + 1) u pi / 16)), [u][x]
D = np.array([[2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896],
              [4017, 3406, 2276, 799, -799, -2276, -3406, -4017],
              [3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784],
              [3406, -799, -4017, -2276, 2276, 4017, 799, -3406],
              [2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896],
              [2276, -4017, 799, 3406, -3406, -799, 4017, -2276],
              [1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567],
              [799, -2276, 3406, -4017, 4017, -3406, 2276, -799]], dtype=np.int32)
D.setflags(write=False)

# ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), [v][u]
BASE = np.array([[16, 11, 10, 16, 24, 40, 51, 61,
                  12, 12, 14, 19, 26, 58, 60, 55,
                  14, 13, 16, 24, 40, 57, 69, 56,
                  14, 17, 22, 29, 51, 87, 80, 62,
                  18, 22, 37, 56, 68, 109, 103, 77,
                  24, 35, 55, 64, 81, 104, 113, 92,
                  49, 64, 78, 87, 103, 121, 120, 101,
                  72, 92, 95, 98, 112, 100, 103, 99],
                 [17, 18, 24, 47, 99, 99, 99, 99,
                  18, 21, 26, 66, 99, 99, 99, 99,
                  24, 26, 56, 99, 99, 99, 99, 99,
                  47, 66, 99, 99, 99, 99, 99, 99,
                  99, 99, 99, 99, 99, 99, 99, 99,
                  99, 99, 99, 99, 99, 99, 99, 99,
                  99, 99, 99, 99, 99, 99, 99, 99,
                  99, 99, 99, 99, 99, 99, 99, 99]], dtype=np.int64)
BASE.setflags(write=False)


def parse(spec) -> Optional[Tuple[int, int]]:
    """`spec` "<q>" or "<lo>..<hi>" (or an int) -> (lo, hi), integers with 1 <= lo <= hi <= 100; None -> None.  ValueError for anything else."""
    if spec is None:
        return None

    def number(v):
        try:
            if isinstance(v, bool) or not isinstance(v, (int, str, np.integer)):
                raise ValueError
            return int(v.strip(), 10) if isinstance(v, str) else int(v)
        except ValueError:
            raise ValueError(f"codec {spec!r}: expected '<q>' or '<lo>..<hi>', the JPEG quality as integers") from None
    text = spec.strip() if isinstance(spec, str) else spec
    lo, hi = (number(v) for v in text.split("..", 1)) if isinstance(text, str) and ".." in text else (number(text),) * 2
    if not 1 <= lo <= hi <= 100:
        raise ValueError(f"codec {spec!r}: the quality needs 1 <= lo <= hi <= 100")
    return lo, hi


def name(spec) -> Optional[str]:
    """The canonical spelling of a codec spec, or None for None."""
    p = parse(spec)
    return None if p is None else (str(p[0]) if p[0] == p[1] else f"{p[0]}..{p[1]}")


def check(spec) -> None:
    """ValueError for a codec spec that does not parse.  Any light goes with a codec: it runs on the encoded bytes."""
    parse(spec)


def quality(spec, seed: int, clip: int) -> int:
    """The quality of clip `clip` under `seed`: lo + floor((hi - lo + 1) w0 / 2^32) from the counter (0xffffffff, 0xfffffffd, 0, clip)."""
    lo, hi = parse(spec)
    return lo + (((hi - lo + 1) * _light.philox((0xffffffff, ROW, 0, clip), _light.key_of(seed))[0]) >> 32)


def quant_tables(q: int) -> np.ndarray:
    """uint16 [2][64] of the quality q in 1..100: Annex K's luminance table, then its chrominance table, scaled by libjpeg's rule;
    row-major [v][u]."""
    if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 1 <= q <= 100:
        raise ValueError(f"codec: quality {q!r} is no integer in 1..100")
    scale = 5000 // int(q) if q < 50 else 200 - 2 * int(q)
    return np.clip((BASE * scale + 50) // 100, 1, 255).astype(np.uint16)


def all_tables() -> np.ndarray:
    """uint16 [100][2][64]: `quant_tables` of every quality, quality q at index q - 1 (the training loader's one table)."""
    return np.stack([quant_tables(q) for q in range(1, 101)])


def records(n: int, qtab: int = 0, oy=0, ox=0, flags=0) -> np.ndarray:
    """CODEC_RECORD [n]: `qtab`, `oy`, `ox` and `flags` are scalars or arrays of n."""
    rec = np.zeros(int(n), dtype=CODEC_RECORD)
    rec["qtab"], rec["oy"], rec["ox"], rec["flags"] = qtab, oy, ox, flags
    return rec


def device_qtabs(tables: np.ndarray, device):
    """(device, host) int16-typed tensors of uint16 [n][2][64] quantisation tables for the C entry points; the upload is issued on the
    current stream of `device`."""
    import torch
    host = torch.from_numpy(np.ascontiguousarray(tables, dtype=np.uint16).reshape(-1, 2, 64).view(np.int16).copy())
    return host.to(torch.device(device)), host
