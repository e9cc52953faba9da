"""Exact-integer operands and float64 references for the conv and GEMM kernels (helper of test_exact_ref_cpu.py and
test_gpu_exact_gemm.py; no GPU).

The operands are small integers (bias: multiples of 0.5), exactly representable in bf16 AND f16, with the sum of |x||w| over a receptive
field far below 2^24: every product and every partial sum is exact in fp32 in whatever order a kernel adds them, so every arithmetic mode
("f32", "bf16x3", "bf16", "f16") of every kernel has to return the float64 result itself, and a 16-bit output has to be that value
rounded once to nearest even (csrc/common.h).  The tests compare with torch.equal: no tolerance.  `check_exact_preconditions` states what
makes that legitimate; it reads the operands and the reference only, never a kernel's output.

References are NCHW float64, cached per argument tuple, so the modes and in / out formats of one shape share one reference."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

# (|x| <=, |w| <=).  "narrow": small results; "wide": results that need rounding in both 16-bit formats, and often land on ties;
# "wider": the same for outputs of fewer than 128 terms, whose sums over the wide set mostly stay below 2048, where f16 holds every
# integer (`amp_for`)
SETS = {"narrow": (4, 3), "wide": (16, 16), "wider": (32, 32)}
BIAS_MAX, RES_MAX, ROWSCALES = 4.0, 64, (0.0, 0.5, 1.0, 2.0)
LP = {"bf16": torch.bfloat16, "f16": torch.float16}
SIG_BITS = {torch.bfloat16: 8, torch.float16: 11}          # significand bits, the hidden one included
MIN_INEXACT, MIN_TIES, MAX_ABS = 0.10, 0.01, 60000.0

Operands = namedtuple("Operands", "x w bias residual rowscale")


def amps(amp):
    return SETS[amp] if isinstance(amp, str) else ((amp, amp) if isinstance(amp, int) else tuple(amp))


def amp_for(terms):
    """The set for a case with 16-bit outputs of `terms` products each (the fewest, where outputs differ)."""
    return "wide" if terms >= 128 else "wider"


def out_hw(k, h, w, stride=1, transposed=False):
    if transposed:
        return h * stride, w * stride
    p = k // 2
    return (h + 2 * p - k) // stride + 1, (w + 2 * p - k) // stride + 1


@functools.lru_cache(maxsize=64)
def operands(seed, batch, cin, cout, k, h, w, amp, stride=1, transposed=False):
    """Integer-valued float32 tensors: x [batch,cin,h,w] in [-ax, ax]; w [cout,cin,k,k] ([cin,cout,k,k] for a transposed conv) in
    [-aw, aw]; bias [cout], multiples of 0.5 in [-4, 4]; for epilogue cases residual [batch,cout,ho,wo], integers in [-64, 64], and a
    per-pixel rowscale [ho,wo] from {0, 0.5, 1, 2}.  `amp`: a set name of SETS, one integer, or (ax, aw).  Do not modify the result."""
    ax, aw = amps(amp)
    g = torch.Generator().manual_seed(seed)
    ho, wo = out_hw(k, h, w, stride, transposed)
    x = torch.randint(-ax, ax + 1, (batch, cin, h, w), generator=g).float()
    wt = torch.randint(-aw, aw + 1, (cin, cout, k, k) if transposed else (cout, cin, k, k), generator=g).float()
    bias = torch.randint(-int(2 * BIAS_MAX), int(2 * BIAS_MAX) + 1, (cout,), generator=g).float() * 0.5
    res = torch.randint(-RES_MAX, RES_MAX + 1, (batch, cout, ho, wo), generator=g).float()
    rs = torch.tensor(ROWSCALES)[torch.randint(0, len(ROWSCALES), (ho, wo), generator=g)]
    return Operands(x, wt, bias, res, rs)


def epilogue64(y, o, relu=False, rowscale=False, residual=False):
    """act(conv + bias) * rowscale + residual on a float64 NCHW result that already holds conv + bias."""
    if relu:
        y = F.relu(y)
    if rowscale:
        y = y * o.rowscale.double()
    if residual:
        y = y + o.residual.double()
    return y


@functools.lru_cache(maxsize=32)
def _conv64(seed, batch, cin, cout, k, h, w, amp, stride, transposed, split):
    o = operands(seed, batch, cin, cout, k, h, w, amp, stride, transposed)
    x = torch.cat((o.x[:, :split], o.x[:, split:]), 1) if split else o.x
    if transposed:
        assert (k, stride) == (3, 2)
        return F.conv_transpose2d(x.double(), o.w.double(), o.bias.double(), stride=2, padding=1, output_padding=1)
    return F.conv2d(x.double(), o.w.double(), o.bias.double(), stride=stride, padding=k // 2)


def conv_ref(seed, batch, cin, cout, k, h, w, amp, stride=1, transposed=False, relu=False, rowscale=False, residual=False, split=0):
    """float64 reference [batch,cout,ho,wo] of the operands of the same arguments: conv2d (padding k//2) or the 3x3 stride-2
    conv_transpose2d (padding 1, output_padding 1), cached, then `epilogue64`.  split > 0: the input arrives as two sources, channels
    [0, split) and [split, cin), concatenated here as the kernels concatenate them.  Do not modify the result."""
    o = operands(seed, batch, cin, cout, k, h, w, amp, stride, transposed)
    return epilogue64(_conv64(seed, batch, cin, cout, k, h, w, amp, stride, transposed, split), o, relu, rowscale, residual)


def linear_operands(seed, m, kdim, n, amp):
    """A token list [m, kdim] -> [m, n] as the 1x1 conv on an m x 1 map that Ctx.linear launches."""
    return operands(seed, 1, kdim, n, 1, m, 1, amp)


@functools.lru_cache(maxsize=16)
def linear_ref(seed, m, kdim, n, amp, relu=False, residual=False):
    """float64 F.linear on `linear_operands`, [m, n]; the residual is the operands' residual as [m, n]."""
    o = linear_operands(seed, m, kdim, n, amp)
    y = F.linear(rows(o.x).double(), o.w.reshape(n, kdim).double(), o.bias.double())
    if relu:
        y = F.relu(y)
    return y + rows(o.residual).double() if residual else y


def rows(x):
    """NCHW -> the kernels' layout: pixels as rows, [batch*h*w, c]."""
    b, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(b * h * w, c).contiguous()


def rounded(y64, dtype):
    """The float64 result rounded ONCE to bf16 / f16 (nearest even): .float() is exact on these values (asserted), so the only rounding
    is the 16-bit one."""
    f = y64.float()
    assert torch.equal(f.double(), y64), "the reference is not exact in fp32: the case is built wrongly"
    return f if dtype == torch.float32 else f.to(dtype)


def _half_ulp(y64, dtype):
    """Half the spacing of `dtype` in the binade of |y| (normal numbers)."""
    _, e = torch.frexp(y64.abs())                           # |y| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(y64), e - SIG_BITS[dtype] - 1)


def rounding_shares(y64, dtype):
    """(share of the outputs that `dtype` cannot hold exactly, share that lie exactly midway between two neighbours)."""
    d = (rounded(y64, dtype).double() - y64).abs()
    inexact = d != 0
    ties = inexact & (d == _half_ulp(y64, dtype))
    return inexact.double().mean().item(), ties.double().mean().item()


def _step_magnitude(r, mask, step):
    """r (16-bit) with the magnitude of the masked elements moved by `step` units in the last place."""
    bits = r.clone().view(torch.int16)
    bits[mask] += step
    return bits.view(r.dtype)


def truncated(y64, dtype):
    """FAULTY rounding: toward zero instead of to nearest even."""
    r = rounded(y64, dtype)
    return _step_magnitude(r, r.double().abs() > y64.abs(), -1)


def ties_away(y64, dtype):
    """FAULTY rounding: nearest, ties away from zero."""
    r = rounded(y64, dtype)
    d = (r.double() - y64).abs()
    return _step_magnitude(r, (d != 0) & (d == _half_ulp(y64, dtype)) & (r.double().abs() < y64.abs()), 1)


def check_exact_preconditions(o, y64, out_dtypes=(), epilogue=False, fan_in=None):
    """What makes `torch.equal` against float64 a fair demand of every mode and summation order.  o: Operands; y64: the reference of the
    case; out_dtypes: the 16-bit output formats the case is run with; epilogue: row scale and residual are part of the case; fan_in:
    terms per output over the full receptive field (default cin * k * k of o.w)."""
    used = [o.x, o.w, o.bias] + ([o.residual, o.rowscale] if epilogue else [])
    for t in used:
        for dt in LP.values():
            assert torch.equal(t.to(dt).float(), t), f"an operand is not exact in {dt}"
    if fan_in is None:
        fan_in = o.w[0].numel() if o.w.dim() == 4 else o.w.shape[-1]
    bound = o.x.abs().max().item() * o.w.abs().max().item() * fan_in + o.bias.abs().max().item()
    if epilogue:
        bound = bound * o.rowscale.abs().max().item() + o.residual.abs().max().item()
    # every intermediate is a multiple of 1/4 (bias 1/2, row scale 1/2): below 2^24 / 4 such values are exact in fp32
    assert bound < 2 ** 24 and bound < 2 ** 22, f"sum |x||w| + |bias| + |residual| can reach {bound}"
    assert y64.dtype == torch.float64 and y64.abs().max().item() <= MAX_ABS, f"max |y| = {y64.abs().max().item()}"
    rounded(y64, torch.float32)
    for dt in out_dtypes:
        inexact, ties = rounding_shares(y64, dt)
        assert inexact >= MIN_INEXACT and ties >= MIN_TIES, f"{dt}: {inexact:.3f} of the outputs inexact, {ties:.4f} ties"


# ---- deliberately wrong references (test_exact_ref_cpu.py shows that torch.equal sees each of them) ----------------------------------
def conv_taps(x, wt, bias, dtype=torch.float32, reverse=False, chunk=16, drop=None, wrap_right=False):
    """Stride-1 conv (padding k//2) accumulated tap by tap and channel chunk by channel chunk in `dtype`, bias last; reverse: taps,
    chunks and the channels inside a chunk in reversed order.  drop = (cout, cin, ky, kx): FAULT, that one product is left out of that
    output channel at every pixel.  wrap_right: FAULT, no zero fill at the right edge — a tap right of the map reads on into the next
    row of the same channel (zero after the last row)."""
    b, c, h, w = x.shape
    co, _, k, _ = wt.shape
    p = k // 2
    wt = wt.to(dtype).clone()
    if drop is not None:
        wt[drop] = 0
    xp = F.pad(x.to(dtype), (p, p, p, p))
    if wrap_right:
        flat = F.pad(x.to(dtype), (0, 0, p, p + 1)).reshape(b, c, -1)             # rows only; one spare row for the last wrap
    y = torch.zeros(b, co, h, w, dtype=dtype)
    taps = [(ky, kx) for ky in range(k) for kx in range(k)]
    chunks = [slice(c0, min(c0 + chunk, c)) for c0 in range(0, c, chunk)]
    if reverse:
        taps, chunks = taps[::-1], chunks[::-1]
    for ky, kx in taps:
        if wrap_right and kx > p:
            idx = (torch.arange(h)[:, None] + ky) * w + torch.arange(w)[None, :] + (kx - p)
            xs = flat[:, :, idx.reshape(-1)].reshape(b, c, h, w)
        else:
            xs = xp[:, :, ky:ky + h, kx:kx + w]
        for ch in chunks:
            xc, wc = xs[:, ch], wt[:, ch, ky, kx]
            if reverse:
                xc, wc = xc.flip(1), wc.flip(1)
            y += torch.einsum("oc,bchw->bohw", wc, xc)
    return y + bias.to(dtype).view(1, -1, 1, 1)


def conv_stack_halo_leak(x, wt, bias):
    """FAULT: in a stack of maps, the top halo of map b > 0 reads the last rows of map b - 1 instead of zeros."""
    p = wt.shape[2] // 2
    out = []
    for m in range(x.shape[0]):
        top = x[m - 1:m, :, -p:] if m else torch.zeros_like(x[:1, :, :p])
        xs = F.pad(torch.cat((top, x[m:m + 1]), 2).double(), (p, p, 0, p))
        out.append(F.conv2d(xs, wt.double(), bias.double()))
    return torch.cat(out)


def conv_stale_tile(x, wt, bias, tile_rows=6, tile=1):
    """FAULT: the output rows of tile `tile` (tiles of `tile_rows` rows) are computed from the input rows of the tile before it."""
    y = F.conv2d(x.double(), wt.double(), bias.double(), padding=wt.shape[2] // 2)
    r0 = tile * tile_rows
    n = min(tile_rows, y.shape[2] - r0)
    y[:, :, r0:r0 + n] = y[:, :, r0 - tile_rows:r0 - tile_rows + n].clone()
    return y


# ---- the case tables, shared by the CPU and the GPU file -------------------------------------------------------------------------------
MI355X_CUS = 256          # the CPU file checks the walk shapes of this CU count; the GPU file builds them from the device's own

# (cin, cout, k, stride, h, w): test_gpu_bf16.py::test_igemm_conv's twelve, then the stride-2 head convs run with 16-bit input too
IGEMM_CASES = [(32, 32, 5, 1, 20, 24), (64, 64, 5, 1, 13, 17), (128, 128, 5, 1, 10, 15), (32, 64, 5, 2, 40, 60),
               (64, 128, 5, 2, 22, 18), (128, 256, 3, 1, 10, 15), (256, 256, 3, 1, 9, 11), (256, 128, 3, 1, 10, 15),
               (384, 128, 1, 1, 10, 15), (64, 32, 1, 1, 21, 19), (96, 32, 3, 1, 21, 19), (512, 256, 1, 1, 33, 7)]
HEAD_CASES = [(32, 64, 5, 2, 11, 13), (64, 128, 5, 2, 34, 66)]
CONCAT_CASE = (64, 32, 64, 3, 14, 22)                                              # (cin0, cin1, cout, k, h, w)
LINEAR_CASES = [(77, 256, 256), (150, 512, 256), (200, 256, 512)]                  # (M, K, N)
BATCHED_LAYERS = [(32, 5), (64, 5), (256, 3)]                                      # (channels, k)
BATCHED_SHAPES = [(3, 7, 33), (3, 37, 50)]                                         # (maps, h, w)
WS_SMALL = [(2, 5, 7), (1, 7, 33), (3, 37, 50)]                                    # (maps, h, w)
WS_TILES = {32: (16, 32), 64: (6, 32)}                                             # channels -> tile (rows, columns)
PIPE_TILE = (6, 16)
PIPE_SHAPES = [(1, 6, 16), (3, 18, 32)]
PIPE_FALLBACK = (1, 10, 16)
PIPE_SETS = ("narrow", "wide")
CONVT_CASES = [(128, 64, 10, 15), (64, 32, 21, 19), (64, 32, 5, 33)]               # (cin, cout, h, w)
IO_SHAPES = [(17, 35), (40, 60)]
SEED = 20


def tiles_of(maps, h, w, tile):
    return maps * -(-h // tile[0]) * -(-w // tile[1])


def walk_shape(cus, tile, maps, ragged=True):
    """(maps, h, w): the smallest narrow stack on which a persistent kernel of `cus` workgroups and `tile` = (rows, columns) pixel tiles
    walks: more than 2 * cus tiles (some workgroups take three: the LDS buffer index returns to 0), not a multiple of cus, fewer tiles
    per map than workgroups (a workgroup's consecutive tiles lie in different maps).  ragged: two tile columns, the second one pixel
    wide, and a last tile row short of 3 rows; else whole tiles, one tile column."""
    cols = 2 if ragged else 1
    r = 2 * cus // (maps * cols) + 1
    while (maps * r * cols) % cus == 0:
        r += 1
    h, w = r * tile[0] - (3 if ragged else 0), tile[1] + (1 if ragged else 0)
    n = tiles_of(maps, h, w, tile)
    assert n == maps * r * cols and n > 2 * cus and n % cus and r * cols < cus and maps >= 2
    return maps, h, w


def ws_walk_shape(channels, cus):
    return walk_shape(cus, WS_TILES[channels], 7 if channels == 32 else 5)


def pipe_walk_shape(cus):
    return walk_shape(cus, PIPE_TILE, 6, ragged=False)


# the argument tuples of `operands` / `conv_ref` per case: test_gpu_exact_gemm.py and `gpu_cases` below both build them here
def igemm_args(cin, cout, k, stride, h, w):
    return (SEED, 1, cin, cout, k, h, w, amp_for(cin * k * k), stride)


def concat_args():
    c0, c1, cout, k, h, w = CONCAT_CASE
    return (SEED + 1, 1, c0 + c1, cout, k, h, w, "wide")


def linear_args(m, kdim, n):
    return (SEED + 2, m, kdim, n, "wide")


def batched_args(c, k, maps, h, w):
    return (SEED + 3, maps, c, c, k, h, w, "wide")


def ws_args(c, maps, h, w):
    return (SEED + 4, maps, c, c, 5, h, w, "wide")


def pipe_args(amp, maps, h, w):
    return (SEED + 5, maps, 256, 256, 3, h, w, amp)


def convt_args(cin, cout, h, w):
    return (SEED + 6, 1, cin, cout, 3, h, w, amp_for(cin), 2, True)          # the output class of one tap has cin terms


def conv5_in_args(h, w):
    return (SEED + 7, 1, 3, 32, 5, h, w, "wide")


def conv5_out_args(h, w):
    return (SEED + 8, 1, 32, 3, 5, h, w, "wide")


def gpu_cases(cus=MI355X_CUS):
    """Every reference that test_gpu_exact_gemm.py compares a kernel with, as (label, Operands, float64 reference, the 16-bit formats it
    is rounded to, row scale and residual in the case, terms per output)."""
    both = tuple(LP.values())
    for case in IGEMM_CASES + HEAD_CASES:
        a = igemm_args(*case)
        yield f"igemm {case} {a[7]}", operands(*a), conv_ref(*a), both, False, case[0] * case[2] ** 2
    a = concat_args()
    yield "concat", operands(*a), conv_ref(*a, relu=True, rowscale=True, residual=True, split=CONCAT_CASE[0]), both, True, a[2] * a[4] ** 2
    for m, kd, n in LINEAR_CASES:
        a = linear_args(m, kd, n)
        yield f"linear {m, kd, n}", linear_operands(*a), linear_ref(*a, residual=True).t().reshape(1, n, m, 1), both, True, kd
    for c, k in BATCHED_LAYERS:
        for maps, h, w in BATCHED_SHAPES:
            a = batched_args(c, k, maps, h, w)
            yield f"batched {a[1:]}", operands(*a), conv_ref(*a), both, False, c * k * k
            yield f"batched {a[1:]} residual", operands(*a), conv_ref(*a, residual=True), (), True, c * k * k
    for c in WS_TILES:
        for maps, h, w in WS_SMALL + [ws_walk_shape(c, cus)]:
            a = ws_args(c, maps, h, w)
            for relu in (False, True):
                yield f"ws {a[1:]} relu {relu}", operands(*a), conv_ref(*a, relu=relu), both, False, c * 25
    for amp in PIPE_SETS:
        for maps, h, w in PIPE_SHAPES + [PIPE_FALLBACK, pipe_walk_shape(cus)]:
            a = pipe_args(amp, maps, h, w)
            yield f"pipe {a[1:]}", operands(*a), conv_ref(*a), (), False, 256 * 9
            yield f"pipe {a[1:]} residual", operands(*a), conv_ref(*a, residual=True), (), True, 256 * 9
    for cin, cout, h, w in CONVT_CASES:
        a = convt_args(cin, cout, h, w)
        for relu in (False, True):
            yield f"convT {a[2:8]} relu {relu}", operands(*a), conv_ref(*a, relu=relu), both, False, cin * 9
    for h, w in IO_SHAPES:
        a = conv5_in_args(h, w)
        yield f"conv5_in {h, w}", operands(*a), conv_ref(*a, relu=True), (), False, 75
        a = conv5_out_args(h, w)
        yield f"conv5_out {h, w}", operands(*a), conv_ref(*a), (), False, 800
