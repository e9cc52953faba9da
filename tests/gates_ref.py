"""Float64 statement of the inference ResBlock epilogue (csrc/resblock.hip): the SE vector, the two gate maps and the gated sum, with
a derived bound on what an fp32 evaluation of them may differ by, the contents and the case table of tests/test_gpu_gates.py, and
the defect models with which tests/test_gates_ref_cpu.py shows that those cases see a subtly wrong kernel.  numpy only.

    s[c]      = sigmoid(W2 relu(W1 mean_hw(x1) + b1) + b2)
    g1[y][c]  = scale1 * corr7x7([max_w x1, mean_w x1])[y][c] + shift1      on the (H, C) plane, zero padding 3
    g2[x][c]  = scale2 * corr5x5([max_h x1, mean_h x1])[c][x] + shift2      on the (C, W) plane, zero padding 2
    out       = x + (x1*s + (x1*g1[y] + x1*g2[x])) (+ extra)

The bound (u = 2**-24, first order in u).  The values of x1 are taken as given (a 16-bit map converts to fp32 exactly) and the maxima
are exact, so every error is one of
  * a length-n fp32 sum, in ANY order:  at most (n-1) u sum|terms|   (each term passes through at most n-1 additions)
  * one division:                       u |quotient|
  * a length-n chain of fused multiply-adds (or of products and additions):  at most (n+1) u sum|w_k||z_k|, the inputs' own errors
    e_k entering with sum|w_k| e_k.
g1: the line mean of W values errs by at most (W-1) u m + u m <= (W+1) u m with m = mean_w|x1| (|mean| <= m); the 98-term chain and the
BatchNorm fma (one more rounding of scale * acc) give 100 u (sum|w_max||zmax| + sum|w_mean| m); the last rounding and that of the shift
are covered by 2u |g1|:

    tol_g1 = u |scale1| (100 sum|w_max||zmax| + (W + 1 + 100) sum|w_mean| mean_w|x1|) + 2u |g1|

g2: 50 terms, so 52 for 100, and H for W.  s: the mean errs by e_mean = (H*W + 1) u mean_hw|x1|; the first layer gives
e_hid = sum|W1| e_mean + (C + 1) u (|b1| + sum|W1||mean|) (ReLU does not enlarge it), the second e_a = sum|W2| e_hid + (C/4 + 1) u (|b2| +
sum|W2| hid); the sigmoid has slope at most 1/4, and expf, the addition and the reciprocal together are allowed 4u of s:

    tol_s = e_a / 4 + 4u s

exact_sums=True is for integer-valued content whose every partial sum is an integer below 2**24: all fp32 sums are exact in any order,
the (n-1) terms go, and only the division's rounding stays: (W + 1 + 100) becomes (2 + 100) and e_mean becomes u |mean_hw x1|.

apply: b*v, two fmas, the addition of x and that of `extra` are five roundings of values bounded by the sum of the absolute terms:

    tol_out = 5u (|x| + |x1| (|s| + |g1| + |g2|) + |extra|)
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
FORMATS = ("fp32", "bf16", "f16")
CHANNELS = (32, 64, 128)

Stats = namedtuple("Stats", "rowmax rowmean rowabs colmax colmean colabs mean meanabs")
Gates = namedtuple("Gates", "s g1 g2 tol_s tol_g1 tol_g2")


# ---- the kernel's tiling, restated (csrc/resblock.hip: GATE_TR16 / GATE_TR32, gate_tc) ----------------------------------------------
def tile_rows(fmt: str) -> int:
    return 8 if fmt == "fp32" else 16


def tile_cols(c: int) -> int:
    return 2048 // c


def tiles(h: int, w: int, c: int, fmt: str):
    """(row tiles, column tiles) of the statistics pass."""
    return -(-h // tile_rows(fmt)), -(-w // tile_cols(c))


# ---- number formats -----------------------------------------------------------------------------------------------------------------
def round_to(x: np.ndarray, fmt: str) -> np.ndarray:
    """x rounded (to nearest, ties to even) to `fmt`, returned as float64."""
    x32 = np.asarray(x, np.float64).astype(np.float32)
    if fmt == "fp32":
        return x32.astype(np.float64)
    if fmt == "f16":
        return x32.astype(np.float16).astype(np.float64)
    assert fmt == "bf16"
    b = x32.view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def pk64(pk: dict) -> dict:
    """The gate parameters of `pack.resblock` as float64 numpy arrays."""
    keys = ("se_w1", "se_b1", "se_w2", "se_b2", "cw_w", "cw_bn", "hc_w", "hc_bn")
    return {k: np.asarray(pk[k].detach().cpu().double().numpy() if hasattr(pk[k], "detach") else pk[k], np.float64) for k in keys}


# ---- the statement ------------------------------------------------------------------------------------------------------------------
def stats_f64(x1: np.ndarray) -> Stats:
    """Line maxima and means of a map [H, W, C]: row* [H, C] over w, col* [W, C] over h, mean [C]; *abs are the means of |x1|."""
    x1 = np.asarray(x1, np.float64)
    a = np.abs(x1)
    return Stats(x1.max(axis=1), x1.mean(axis=1), a.mean(axis=1), x1.max(axis=0), x1.mean(axis=0), a.mean(axis=0),
                 x1.mean(axis=(0, 1)), a.mean(axis=(0, 1)))


def _corr(zmax, zmean, zabs, wk, k):
    """Zero-padded k x k correlation of the two planes [L0, L1] with wk [2, k, k] (taps over axis 0, then axis 1), and the sums
    sum|w_max||zmax| and sum|w_mean| zabs over the same window."""
    p = k // 2
    pad = [np.pad(z, p) for z in (zmax, zmean, np.abs(zmax), zabs)]
    n0, n1 = zmax.shape
    acc, amax, amean = (np.zeros((n0, n1)) for _ in range(3))
    for d0 in range(k):
        for d1 in range(k):
            sl = (slice(d0, d0 + n0), slice(d1, d1 + n1))
            acc += wk[0, d0, d1] * pad[0][sl] + wk[1, d0, d1] * pad[1][sl]
            amax += abs(wk[0, d0, d1]) * pad[2][sl]
            amean += abs(wk[1, d0, d1]) * pad[3][sl]
    return acc, amax, amean


def gates_from_stats(st: Stats, pk: dict, h: int, w: int, exact_sums: bool = False) -> Gates:
    c = st.mean.shape[0]
    # SE
    w1, b1, w2, b2 = pk["se_w1"], pk["se_b1"], pk["se_w2"], pk["se_b2"]
    e_mean = U * np.abs(st.mean) if exact_sums else (h * w + 1) * U * st.meanabs
    pre = w1 @ st.mean + b1
    hid = np.maximum(pre, 0.0)
    e_hid = np.abs(w1) @ e_mean + (c + 1) * U * (np.abs(b1) + np.abs(w1) @ np.abs(st.mean))
    a = w2 @ hid + b2
    e_a = np.abs(w2) @ e_hid + (c // 4 + 1) * U * (np.abs(b2) + np.abs(w2) @ hid)
    s = 1.0 / (1.0 + np.exp(-a))
    tol_s = e_a / 4 + 4 * U * s
    # row gate: (H, C) plane, taps [dy][dc]
    acc, amax, amean = _corr(st.rowmax, st.rowmean, st.rowabs, pk["cw_w"].reshape(2, 7, 7), 7)
    g1 = acc * pk["cw_bn"][0] + pk["cw_bn"][1]
    tol_g1 = U * abs(pk["cw_bn"][0]) * (100 * amax + ((2 if exact_sums else w + 1) + 100) * amean) + 2 * U * np.abs(g1)
    # column gate: (C, W) plane, taps [dc][dx]; the planes here are [W, C], so the taps are transposed
    acc, amax, amean = _corr(st.colmax, st.colmean, st.colabs, pk["hc_w"].reshape(2, 5, 5).transpose(0, 2, 1), 5)
    g2 = acc * pk["hc_bn"][0] + pk["hc_bn"][1]
    tol_g2 = U * abs(pk["hc_bn"][0]) * (52 * amax + ((2 if exact_sums else h + 1) + 52) * amean) + 2 * U * np.abs(g2)
    return Gates(s, g1, g2, tol_s, tol_g1, tol_g2)


def gates_f64(x1: np.ndarray, pk: dict, exact_sums: bool = False) -> Gates:
    """s [C], g1 [H, C], g2 [W, C] of the map x1 [H, W, C] and the bound on each element (module docstring).  pk: `pk64`."""
    h, w, _ = x1.shape
    return gates_from_stats(stats_f64(x1), pk, h, w, exact_sums)


def apply_f64(x, x1, s, g1, g2, extra=None):
    """out [H, W, C] = x + (x1*s + (x1*g1[y] + x1*g2[x])) (+ extra), and its bound."""
    x, x1 = np.asarray(x, np.float64), np.asarray(x1, np.float64)
    s, g1, g2 = (np.asarray(t, np.float64) for t in (s, g1, g2))
    e = np.zeros_like(x) if extra is None else np.asarray(extra, np.float64)
    out = x + (x1 * s + (x1 * g1[:, None, :] + x1 * g2[None, :, :])) + e
    tol = 5 * U * (np.abs(x) + np.abs(x1) * (np.abs(s) + np.abs(g1)[:, None, :] + np.abs(g2)[None, :, :]) + np.abs(e))
    return out, tol


def apply_i64(x, x1, s, g1, g2, extra=None):
    """The gated sum of integer-valued operands in int64: exact, so any fp32 evaluation order must give these very values."""
    x, x1, s, g1, g2 = (np.asarray(t).astype(np.int64) for t in (x, x1, s, g1, g2))
    out = x + x1 * s + x1 * g1[:, None, :] + x1 * g2[None, :, :]
    return out if extra is None else out + np.asarray(extra).astype(np.int64)


# ---- contents -----------------------------------------------------------------------------------------------------------------------
def content(family: str, h: int, w: int, c: int, fmt: str, seed: int) -> np.ndarray:
    """A map [H, W, C] (float64) of values representable in `fmt`.
    gauss    randn * 0.7 + 0.1
    neg      -|randn| - 0.5: every line maximum is negative, so a zero that enters a maximum changes it
    ints     integers in [-8, 8]: every partial sum is exact in fp32 (|sum| < 2**24 up to 2 000 000 summands)
    planted  neg with one value per checked line raised to -1/8, -1/4 or -3/8, the line's only value above -1/2.  Even channels check
             the row lines (y, c): the value sits in the last column, in the first column of the last column tile or in column 0,
             in turn; odd channels check the column lines (x, c) likewise with the last row, the first row of the last row tile and row 0.
             Every thread of the statistics pass owns 8 adjacent channels, so each sees both kinds.
    flat     one constant per channel (of either sign): all values of a line tie and its mean equals its maximum"""
    r = np.random.RandomState(seed)
    if family == "gauss":
        return round_to(r.randn(h, w, c) * 0.7 + 0.1, fmt)
    if family == "ints":
        return r.randint(-8, 9, size=(h, w, c)).astype(np.float64)
    if family == "flat":
        v = round_to(r.randn(c) * 0.7 + 0.1, fmt)
        assert (v < 0).any() and (v > 0).any()
        return np.broadcast_to(v, (h, w, c)).copy()
    x = round_to(-np.abs(r.randn(h, w, c)) - 0.5, fmt)
    if family == "neg":
        return x
    assert family == "planted"
    nty, ntx = tiles(h, w, c, fmt)
    xs = (w - 1, (ntx - 1) * tile_cols(c), 0)
    ys = (h - 1, (nty - 1) * tile_rows(fmt), 0)
    for ch in range(c):
        if ch % 2 == 0:
            for y in range(h):
                k = (y + ch // 2) % 3
                x[y, xs[k], ch] = -0.125 * (1 + (y + ch) % 3)
        else:
            for xx in range(w):
                k = (xx + ch // 2) % 3
                x[ys[k], xx, ch] = -0.125 * (1 + (xx + ch) % 3)
    return x


def apply_ints(b: int, h: int, w: int, c: int, seed: int, extra: bool):
    """Integer-valued operands in [-4, 4] of the gated sum on `b` maps: x, x1 [B, H, W, C], s [B, C], g1 [B, H, C], g2 [B, W, C], extra
    (or None).  Independent draws: s depends on (map, channel) only, g1 on (map, row, channel), g2 on (map, column, channel), so an
    exchange of two indices changes the result (tests/test_gates_ref_cpu.py checks that it does)."""
    r = np.random.RandomState(seed)
    draw = lambda *shape: r.randint(-4, 5, size=shape).astype(np.float64)          # noqa: E731
    return draw(b, h, w, c), draw(b, h, w, c), draw(b, c), draw(b, h, c), draw(b, w, c), (draw(b, h, w, c) if extra else None)


def apply_gauss(b: int, h: int, w: int, c: int, fmt: str, seed: int, extra: bool):
    """Gaussian operands of the gated sum, fp32 values (x1 rounded to `fmt`); the gates have the size of real ones."""
    r = np.random.RandomState(seed)
    f32 = lambda t: round_to(t, "fp32")                                            # noqa: E731
    return (f32(r.randn(b, h, w, c)), round_to(r.randn(b, h, w, c) * 0.7, fmt), f32(0.5 + 0.2 * r.randn(b, c)), f32(0.3 * r.randn(b, h, c)),
            f32(0.3 * r.randn(b, w, c)), (f32(r.randn(b, h, w, c)) if extra else None))


# ---- the case table of the gate kernels -----------------------------------------------------------------------------------------------
# row name -> (families, shapes(c, fmt)); TR / TC are the tile's rows (per format) and columns (per channel count)
def _degenerate(c, fmt):
    return [(1, 1), (1, 5), (5, 1), (3, 4), (6, 4)]


def _one_tile(c, fmt):
    tr, tc = tile_rows(fmt), tile_cols(c)
    return [(tr, tc), (tr + 1, tc + 1)]


def _column_tiles(c, fmt):
    tc = tile_cols(c)
    return [(9, 2 * tc + 1), (9, 4 * tc), (9, 4 * tc + 1)]


def _row_tiles(c, fmt):
    tr = tile_rows(fmt)
    return [(2 * tr + 1, 7), (4 * tr, 7), (4 * tr + 1, 7)]


def _block_boundary(c, fmt):
    return [(2 * (256 // c) + 3, tile_cols(c) + 3)]


def _se_walk(c, fmt):
    tr, tc = tile_rows(fmt), tile_cols(c)
    return [{128: (65, 200), 64: (8 * tr + 1, 15 * tc + 1), 32: (15 * tr + 1, 15 * tc + 1)}[c]]


ROWS = {
    "degenerate": (("gauss", "neg", "flat"), _degenerate),
    "one_tile": (("neg", "planted"), _one_tile),
    "column_tiles": (("gauss", "planted"), _column_tiles),
    "row_tiles": (("gauss", "planted"), _row_tiles),
    "block_boundary": (("neg",), _block_boundary),
    # ints: at 200 000 summands the order-free bound on the SE mean would hide a dropped tile, exact sums do not.  neg: the masks and
    # the maxima of the partials at 9 to 16 tiles per line (two to four rounds of reduce_partials' unrolled loop)
    "se_walk": (("ints", "neg"), _se_walk),
}
# two ragged shapes of the table for the batched entry point: (row, index into its shapes)
BATCHED = (("one_tile", 1), ("column_tiles", 2))
BATCHED_FAMILIES = ("gauss", "neg", "planted")


def cases(row: str, c: int, fmt: str):
    """[(h, w, family, exact_sums, seed)] of one row of the table."""
    fams, shapes = ROWS[row]
    out = []
    for i, (h, w) in enumerate(shapes(c, fmt)):
        for j, fam in enumerate(fams):
            out.append((h, w, fam, fam == "ints", 1000 * c + 100 * list(ROWS).index(row) + 10 * i + j))
    return out


def se_unrolled(h: int, w: int, c: int, fmt: str) -> bool:
    """The SE block's 8-way unrolled tile walk runs: more than 7 * (1024 / C) tiles."""
    nty, ntx = tiles(h, w, c, fmt)
    return nty * ntx > 7 * (1024 // c)


# ---- defect models: a wrong kernel, stated on the float64 statistics ----------------------------------------------------------------
def _zeros_in_column_maxima(st, x1, c, fmt):
    """The out-of-map rows of the last row tile (loaded as zeros) enter the column maxima: `y0 + r < H` lost."""
    return st._replace(colmax=np.maximum(st.colmax, 0.0)) if x1.shape[0] % tile_rows(fmt) else st


def _zeros_in_row_maxima(st, x1, c, fmt):
    """The out-of-map columns of the last column tile enter the row maxima: `c2 < ncol` lost."""
    return st._replace(rowmax=np.maximum(st.rowmax, 0.0)) if x1.shape[1] % tile_cols(c) else st


def _row_mean_drops_last_column(st, x1, c, fmt):
    w = x1.shape[1]
    return st._replace(rowmean=st.rowmean - x1[:, w - 1, :] / w)


def _column_mean_drops_last_row(st, x1, c, fmt):
    h = x1.shape[0]
    return st._replace(colmean=st.colmean - x1[h - 1, :, :] / h)


def _denominators_swapped(st, x1, c, fmt):
    h, w = x1.shape[:2]
    return st._replace(rowmean=st.rowmean * w / h, colmean=st.colmean * h / w)


def _se_drops_last_tile(st, x1, c, fmt):
    """The last tile's channel sums never reach the SE mean (the tail of the tile walk)."""
    h, w = x1.shape[:2]
    nty, ntx = tiles(h, w, c, fmt)
    t = x1[(nty - 1) * tile_rows(fmt):, (ntx - 1) * tile_cols(c):, :]
    return st._replace(mean=st.mean - t.sum(axis=(0, 1)) / (h * w))


DEFECTS = {                      # name -> (model, the content family that exposes it, applies to this shape)
    "zeros_in_column_maxima": (_zeros_in_column_maxima, "neg", lambda h, w, c, fmt: h % tile_rows(fmt) != 0),
    "zeros_in_row_maxima": (_zeros_in_row_maxima, "neg", lambda h, w, c, fmt: w % tile_cols(c) != 0),
    "row_mean_drops_last_column": (_row_mean_drops_last_column, "planted", lambda h, w, c, fmt: True),
    "column_mean_drops_last_row": (_column_mean_drops_last_row, "planted", lambda h, w, c, fmt: True),
    "denominators_swapped": (_denominators_swapped, "gauss", lambda h, w, c, fmt: h != w),
    "se_drops_last_tile": (_se_drops_last_tile, "ints", lambda h, w, c, fmt: True),
    "halo_minus_one_reads_line_zero": (None, "gauss", lambda h, w, c, fmt: True),
}


def gates_with_defect(name: str, x1: np.ndarray, pk: dict, c: int, fmt: str) -> Gates:
    h, w = x1.shape[:2]
    if name == "halo_minus_one_reads_line_zero":
        return _gates_halo_defect(x1, pk)
    return gates_from_stats(DEFECTS[name][0](stats_f64(x1), x1, c, fmt), pk, h, w)


def _gates_halo_defect(x1, pk):
    """Line -1 of the reduced rows / columns (outside the map: zero padding) is read as line 0."""
    h, w, c = x1.shape
    st = stats_f64(x1)

    def corr(zmax, zmean, wk, k):
        p = k // 2
        pads = []
        for z in (zmax, zmean):
            zp = np.pad(z, p)
            zp[p - 1, p:p + z.shape[1]] = z[0]
            pads.append(zp)
        acc = np.zeros(zmax.shape)
        for d0 in range(k):
            for d1 in range(k):
                acc += wk[0, d0, d1] * pads[0][d0:d0 + zmax.shape[0], d1:d1 + zmax.shape[1]]
                acc += wk[1, d0, d1] * pads[1][d0:d0 + zmax.shape[0], d1:d1 + zmax.shape[1]]
        return acc
    good = gates_from_stats(st, pk, h, w)
    g1 = corr(st.rowmax, st.rowmean, pk["cw_w"].reshape(2, 7, 7), 7) * pk["cw_bn"][0] + pk["cw_bn"][1]
    g2 = corr(st.colmax, st.colmean, pk["hc_w"].reshape(2, 5, 5).transpose(0, 2, 1), 5) * pk["hc_bn"][0] + pk["hc_bn"][1]
    return good._replace(g1=g1, g2=g2)


def exceeds(got: Gates, ref: Gates) -> float:
    """Largest |got - ref| / tol over the three outputs."""
    return max(float((np.abs(getattr(got, n) - getattr(ref, n)) / getattr(ref, "tol_" + n)).max()) for n in ("s", "g1", "g2"))


# ---- fp32 evaluation in another order: sequential sums over each line, products and additions unfused ----------------------------------
def gates_fp32_sequential(x1: np.ndarray, pk: dict):
    f = np.float32
    x = np.asarray(x1, np.float64).astype(f)
    h, w, c = x.shape
    p = {k: v.astype(f) for k, v in pk.items()}
    rowsum = np.cumsum(x, axis=1, dtype=f)[:, -1, :]
    colsum = np.cumsum(x, axis=0, dtype=f)[-1]
    total = np.cumsum(x.reshape(h * w, c), axis=0, dtype=f)[-1]
    mean = total / f(h * w)

    def dense(wt, b, v):
        acc = b.copy()
        for k in range(wt.shape[1]):
            acc = acc + wt[:, k] * v[k]
        return acc
    a = dense(p["se_w2"], p["se_b2"], np.maximum(dense(p["se_w1"], p["se_b1"], mean), f(0)))
    s = f(1) / (f(1) + np.exp(-a))

    def corr(zmax, zmean, wk, k):
        pd = k // 2
        zp = [np.pad(z, pd) for z in (zmax, zmean)]
        acc = np.zeros(zmax.shape, f)
        for ch in range(2):
            for d0 in range(k):
                for d1 in range(k):
                    acc = acc + wk[ch, d0, d1] * zp[ch][d0:d0 + zmax.shape[0], d1:d1 + zmax.shape[1]]
        return acc
    g1 = corr(x.max(axis=1), rowsum / f(w), p["cw_w"].reshape(2, 7, 7), 7) * p["cw_bn"][0] + p["cw_bn"][1]
    g2 = corr(x.max(axis=0), colsum / f(h), p["hc_w"].reshape(2, 5, 5).transpose(0, 2, 1), 5) * p["hc_bn"][0] + p["hc_bn"][1]
    assert s.dtype == f and g1.dtype == f and g2.dtype == f
    return s.astype(np.float64), g1.astype(np.float64), g2.astype(np.float64)
