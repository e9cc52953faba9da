"""A numpy restatement of the geometric self-ensemble (include/speinet_hip.h, speinet_amd/ensemble.py), written from the definition and
independent of the package: member `op` in 0..7, bit 0 reverses the columns, bit 1 the rows, bit 2 then transposes the last two axes;
the mean is the sequential float32 sum of the inverse-transformed members, starting from the first, times 2^-log2 K."""
import numpy as np


def t_op(a: np.ndarray, op: int) -> np.ndarray:
    """T_op on the last two axes."""
    assert 0 <= op <= 7
    if op & 1:
        a = a[..., :, ::-1]
    if op & 2:
        a = a[..., ::-1, :]
    if op & 4:
        a = np.swapaxes(a, -1, -2)
    return np.ascontiguousarray(a)


def t_inv(a: np.ndarray, op: int) -> np.ndarray:
    """T_op^-1: the transposition first, then the flips."""
    assert 0 <= op <= 7
    if op & 4:
        a = np.swapaxes(a, -1, -2)
    if op & 2:
        a = a[..., ::-1, :]
    if op & 1:
        a = a[..., :, ::-1]
    return np.ascontiguousarray(a)


def shape_of(h: int, w: int, op: int) -> tuple:
    return (w, h) if op & 4 else (h, w)


def inverse_member(op: int) -> int:
    """The g with T_g = T_op^-1, found by trying all eight on an asymmetric array."""
    a = np.arange(12.0).reshape(3, 4)
    b = t_op(a, op)
    (g,) = [g for g in range(8) if t_op(b, g).shape == a.shape and np.array_equal(t_op(b, g), a)]
    return g


def mean(members, ops) -> np.ndarray:
    """float32 (((m_0 + m_1) + m_2) + ...) * (1 / K) with m_k = T_ops[k]^-1(members[k]); K = 1: m_0 itself, bits kept."""
    k = len(members)
    assert k in (1, 2, 4, 8) and len(ops) == k
    terms = [t_inv(np.asarray(m, np.float32), g) for m, g in zip(members, ops)]
    if k == 1:
        return terms[0]
    with np.errstate(invalid="ignore", over="ignore"):
        acc = terms[0].copy()
        for t in terms[1:]:
            acc = (acc + t).astype(np.float32)
        return acc * np.float32(1.0 / k)


def same_bits_or_nan(got: np.ndarray, want: np.ndarray) -> bool:
    """Bit for bit where `want` is not NaN, NaN where it is."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return (got.shape == want.shape and bool(np.isnan(got[nan]).all())
            and np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32)))
