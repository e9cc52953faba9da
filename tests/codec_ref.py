"""speinet_amd/codec.py's contract in numpy int64, for the tests: the JPEG-style round trip of a uint8 [H][W][3] frame or rectangle.  Every sum
is held to the int32 bound codec.py's docstring states for it."""
import numpy as np

from speinet_amd import codec

D = codec.D.astype(np.int64)
# |sum| of the four matrix passes, before the rounding constant is added (codec.py)
BOUNDS = (2965504, 67094528, 24908791, 526417325)
F_HFLIP, F_VFLIP, F_ROT90, F_ZERO, F_SKIP = 1, 2, 4, 8, 16


def _bounded(v, bound):
    assert np.abs(v).max() <= bound < 2 ** 31 - 2 ** 15, (int(np.abs(v).max()), bound)
    return v


def forward(s):
    """int64 [..., 8, 8] samples (value - 128) -> F [..., v, u], the coefficients in Q3."""
    T = (_bounded(np.einsum("ux,...yx->...yu", D, s), BOUNDS[0]) + 2 ** 9) >> 10
    return (_bounded(np.einsum("vy,...yu->...vu", D, T), BOUNDS[1]) + 2 ** 12) >> 13


def quantise(F, Q):
    """F [..., 8, 8] and a table Q [8, 8] -> G = q Q."""
    q = np.sign(F) * ((np.abs(F) + 4 * Q) // (8 * Q))
    return q * Q


def inverse(G):
    """G [..., v, u] -> samples 0..255 [..., y, x]."""
    U = (_bounded(np.einsum("vy,...vu->...yu", D, G), BOUNDS[2]) + 2 ** 9) >> 10
    r = (_bounded(np.einsum("ux,...yu->...yx", D, U), BOUNDS[3]) + 2 ** 15) >> 16
    return np.clip(r + 128, 0, 255)


def _blocks(p):
    """[H8, W8] -> [H8 / 8, W8 / 8, 8, 8]"""
    h, w = p.shape
    return p.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def _plane(b):
    ny, nx = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(ny * 8, nx * 8)


def code_plane(p, Q):
    """A plane of values 0..255 whose sides are multiples of 8 through the block round trip with the table Q [64]."""
    return _plane(inverse(quantise(forward(_blocks(p.astype(np.int64)) - 128), np.asarray(Q, np.int64).reshape(8, 8))))


def to_ycc(rgb):
    """int64 [H16, W16, 3] (sides multiples of 2) -> Y [H16, W16], Cb and Cr [H16 / 2, W16 / 2]."""
    R, G, B = (rgb[..., c] for c in range(3))
    Y = np.clip((4899 * R + 9617 * G + 1868 * B + 2 ** 13) >> 14, 0, 255)
    S = [c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] for c in (R, G, B)]
    Cb = np.clip(((-2765 * S[0] - 5427 * S[1] + 8192 * S[2] + 2 ** 15) >> 16) + 128, 0, 255)
    Cr = np.clip(((8192 * S[0] - 6860 * S[1] - 1332 * S[2] + 2 ** 15) >> 16) + 128, 0, 255)
    return Y, Cb, Cr


def to_rgb(Y, Cb, Cr):
    yy = 16384 * 16 * Y
    u = 16 * np.repeat(np.repeat(Cb, 2, 0), 2, 1) - 2048
    v = 16 * np.repeat(np.repeat(Cr, 2, 0), 2, 1) - 2048
    for t in (yy + 22970 * v, yy - 5638 * u - 11700 * v, yy + 29032 * u):
        assert np.abs(t).max() + 2 ** 17 < 2 ** 31
    return np.stack([np.clip((yy + 22970 * v + 2 ** 17) >> 18, 0, 255), np.clip((yy - 5638 * u - 11700 * v + 2 ** 17) >> 18, 0, 255),
                     np.clip((yy + 29032 * u + 2 ** 17) >> 18, 0, 255)], axis=-1)


def pad(rgb, oy=0, ox=0):
    """uint8 [H, W, 3] -> int64 [16 ny, 16 nx, 3]: the MCUs that cover it from a grid corner at (-oy, -ox), coordinates clamped."""
    H, W = rgb.shape[:2]
    assert 0 <= oy < 16 and 0 <= ox < 16
    ys = np.clip(np.arange(-oy, -oy + 16 * -(-(H + oy) // 16)), 0, H - 1)
    xs = np.clip(np.arange(-ox, -ox + 16 * -(-(W + ox) // 16)), 0, W - 1)
    return rgb.astype(np.int64)[ys][:, xs]


def round_trip(rgb, qtabs, oy=0, ox=0):
    """The contract: uint8 [H, W, 3] -> uint8 [H, W, 3] through the tables `qtabs` [2][64] on the MCU grid with a corner at (-oy, -ox)."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    qtabs = np.asarray(qtabs, np.int64).reshape(2, 64)
    assert qtabs.min() >= 1 and qtabs.max() <= 255
    H, W = rgb.shape[:2]
    Y, Cb, Cr = to_ycc(pad(rgb, oy, ox))
    out = to_rgb(code_plane(Y, qtabs[0]), code_plane(Cb, qtabs[1]), code_plane(Cr, qtabs[1]))
    return out[oy:oy + H, ox:ox + W].astype(np.uint8)


def augment(a, flags):
    """train_batch.hip's geometry on a [P, P, ...] array in source orientation: rot90 (counter-clockwise) of the flipped crop."""
    if flags & F_HFLIP:
        a = a[:, ::-1]
    if flags & F_VFLIP:
        a = a[::-1]
    if flags & F_ROT90:
        a = np.rot90(a)
    return np.ascontiguousarray(a)


def unaugment(a, flags):
    """The inverse of `augment`."""
    if flags & F_ROT90:
        a = np.rot90(a, -1)
    if flags & F_VFLIP:
        a = a[::-1]
    if flags & F_HFLIP:
        a = a[:, ::-1]
    return np.ascontiguousarray(a)


def train_batch_codec(inp, rgb_range, recs, qtabs):
    """spei_train_batch_codec_f32 on float32 [n, 3, P, P] whose values are (float)u * (float)(rgb_range / 255): a new array."""
    s, inv = np.float32(rgb_range / 255.0), np.float32(255.0 / rgb_range)
    out = inp.copy()
    for r in range(inp.shape[0]):
        flags = int(recs["flags"][r])
        if flags & (F_ZERO | F_SKIP):
            continue
        u8 = (inp[r] * inv + np.float32(0.5)).astype(np.int64).astype(np.uint8).transpose(1, 2, 0)
        coded = round_trip(unaugment(u8, flags), qtabs[int(recs["qtab"][r])], int(recs["oy"][r]), int(recs["ox"][r]))
        out[r] = augment(coded, flags).transpose(2, 0, 1).astype(np.float32) * s
    return out
