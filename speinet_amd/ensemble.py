"""Geometric self-ensemble (the "+" variant of a restoration model): the eight flips and transpositions of a frame, the reference's
`forward_x8` (util/network_utils.py:308-341).  This is the Python statement of the definition; the C statement is in
include/speinet_hip.h, the kernels are in csrc/ensemble_io.hip (`ops.planes_d4`, `ops.d4_mean`) and the clip API uses them
(`video.deblur_clip(..., ensemble=)`).

Member `op` in 0..7, the reference's enumeration: bit 0 reverses the columns (`a[..., :, ::-1]`, its 'v'), bit 1 reverses the rows
(`a[..., ::-1, :]`, its 'h'), bit 2 transposes the last two axes; `apply` (T_op) does them in that order, `invert` (T_op^-1)
transposes first and then flips.  An ensemble of K uses the members 0..K-1: 2 is the frame and its mirror, 4 the flips (one frame
shape), 8 adds the four transposed members of shape [W][H].  The result is the float32 sum of m_k = T_k^-1(model(T_k(x))) in member
order, starting from m_0, times 2^-log2 K."""
from __future__ import annotations

import numbers

SIZES = (1, 2, 4, 8)
MEMBERS = {k: tuple(range(k)) for k in SIZES}


def check_op(op) -> int:
    if isinstance(op, bool) or not isinstance(op, numbers.Integral) or not 0 <= op <= 7:
        raise ValueError(f"an ensemble member is a whole number 0..7, got {op!r}")
    return int(op)


def _flip(a, axis: int):
    if hasattr(a, "flip"):                                 # a torch tensor: no negative strides
        return a.flip(axis)
    idx = [slice(None)] * a.ndim
    idx[axis] = slice(None, None, -1)
    return a[tuple(idx)]


def _transpose(a):
    return a.transpose(-1, -2) if hasattr(a, "flip") else a.swapaxes(-1, -2)


def apply(a, op: int):
    """T_op of a numpy array or torch tensor, on its last two axes (a view where the type allows one)."""
    op = check_op(op)
    if op & 1:
        a = _flip(a, -1)
    if op & 2:
        a = _flip(a, -2)
    return _transpose(a) if op & 4 else a


def invert(a, op: int):
    """T_op^-1: `invert(apply(a, op), op)` is a."""
    op = check_op(op)
    if op & 4:
        a = _transpose(a)
    if op & 2:
        a = _flip(a, -2)
    return _flip(a, -1) if op & 1 else a


def shape_of(h: int, w: int, op: int) -> tuple:
    """The (rows, columns) of T_op of an h x w plane."""
    return (w, h) if check_op(op) & 4 else (h, w)


def inverse_member(op: int) -> int:
    """The member g with T_g = T_op^-1: a flip is its own inverse; behind a transposition the two flips change places."""
    op = check_op(op)
    return 4 | ((op & 1) << 1) | ((op >> 1) & 1) if op & 4 else op


def check_size(k) -> int:
    """`ensemble=` of the clip API: 1, 2, 4 or 8 as an int (not True, not 8.0)."""
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or k not in SIZES:
        raise ValueError(f"ensemble must be 1, 2, 4 or 8 (members 0..K-1 of the eight flips and transpositions), got {k!r}")
    return int(k)
