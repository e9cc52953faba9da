"""Float64 references, operand builders and the case tables of the fp32 glue kernels: csrc/stencil.hip (RL prior, bicubic upsampling) and
csrc/swin.hip (LayerNorm(256), the f32 window-attention core).  tests/test_gpu_glue_f64.py holds the kernels to these on the MI355X;
tests/test_glue_ref_cpu.py pins the references themselves (golden vectors, the oracle) and shows that the case tables see each mistake
of `wrong_variants()`.

Every reference is generic in dtype: evaluated in float64 it is the "want" side, evaluated in float32 on the host ("host fp32") it
gives the error that an honest fp32 evaluation of the same formula has.  The bound of an operation comes from that alone:

    e_host(op) = max over the operation's cases of  max|host fp32 - float64| / max|float64|
    a kernel passes a case when  max|kernel - float64| / max|float64|  <=  FACTOR * e_host(op),      FACTOR = 4

FACTOR allows for another, equally valid order of summation and other fused multiply-adds than the host's; no figure in it comes
from a kernel.  A 16-bit output adds half a unit of the format at |float64| (`ulp16`): the rounding contract of csrc/common.h.
The operations are `OPS`: each operand set of the attention is one of its own (see ATTN_OPS).  e_host is pooled over the small cases
on the host; the three grid-stride maps of the bicubic kernels and the 32773-row LayerNorm case hold the same kind of content and are
held to the same bound without adding to it.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import speinet_oracle as O
from speinet_amd.synth import _shift_mask

FACTOR = 4
WS, NH, HD, DIM = 5, 8, 32, 256
F64 = torch.float64
LP_BITS = {torch.bfloat16: (8, -126), torch.float16: (11, -14)}        # significand bits, smallest normal exponent


def rng(seed):
    return np.random.RandomState(seed)


def f32(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


# ------------------------------------------------------------------------------------------------------------------------------
# error measures
# ------------------------------------------------------------------------------------------------------------------------------
def nerr(got: torch.Tensor, want: torch.Tensor) -> float:
    """max|got - want| over the case's max|want|; a NaN or inf in `got` counts as an infinite error."""
    d = torch.nan_to_num((got.to(F64) - want).abs(), nan=math.inf, posinf=math.inf).max().item()
    scale = want.abs().max().item()
    return d / scale if scale > 0 else (0.0 if d == 0 else math.inf)


def ulp16(want: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of the 16-bit format `dtype` at |want| (float64): 2^(floor(log2|want|) - (p - 1)), subnormal spacing below 2^emin."""
    p, emin = LP_BITS[dtype]
    e = torch.frexp(want.abs())[1].to(F64) - 1                       # |want| = m * 2^(e + 1), m in [0.5, 1)
    e = torch.where(want == 0, torch.full_like(e, emin), e)          # frexp(0) has exponent 0
    return torch.exp2(torch.clamp(e, min=emin) - (p - 1))


def lp_excess(got: torch.Tensor, want: torch.Tensor, dtype, e_host: float) -> float:
    """max of |got - want| / (ulp16(want) / 2 + FACTOR * e_host * max|want|): at most 1 when the 16-bit output keeps its contract."""
    allowed = ulp16(want, dtype) / 2 + FACTOR * e_host * want.abs().max()
    d = torch.nan_to_num((got.to(F64) - want).abs(), nan=math.inf, posinf=math.inf)
    return (d / allowed).max().item()


# ------------------------------------------------------------------------------------------------------------------------------
# RL prior  (csrc/stencil.hip rl_iter_kernel: 32 x 32 tile + halo 2, one launch per iteration, ping-pong)
# ------------------------------------------------------------------------------------------------------------------------------
RL_SIZES = ((1, 1), (1, 7), (2, 3), (5, 5), (31, 34), (32, 32), (33, 65), (66, 63))
RL_ITERS, RL_PLANES, RL_LAMS = (1, 2, 3, 5), (1, 3, 4), (0.0, 0.01, 0.1)
RL_ZERO_SIZES = ((33, 65), (66, 63))
RL_SIGNED_SIZES = ((5, 5), (33, 65))


def rl_cases():
    """(h, w, planes, iters, lam, content): every size with every iteration count; planes and lam cycle so that all nine pairs of
    them occur.  "zeros": exact-zero blocks (9 x 11 inside, 6 x 7 in the bottom right corner) and plane 1 scaled by 0.02.  "signed":
    isolated negative pixels (one in 35), the only content here on which I / b is negative, so the only one that needs the clamp."""
    out = []
    for i, (h, w) in enumerate(RL_SIZES):
        for j, it in enumerate(RL_ITERS):
            out.append((h, w, RL_PLANES[(i + j) % 3], it, RL_LAMS[(i + 2 * j) % 3], "uniform"))
    for i, (h, w) in enumerate(RL_ZERO_SIZES):
        for j, it in enumerate(RL_ITERS):
            out.append((h, w, 3, it, RL_LAMS[(i + j + 1) % 3], "zeros"))
    for i, (h, w) in enumerate(RL_SIGNED_SIZES):
        for j, it in enumerate(RL_ITERS):
            out.append((h, w, 3, it, RL_LAMS[(i + j + 2) % 3], "signed"))
    return out


def rl_image(h, w, c, content) -> torch.Tensor:
    x = rng(1000 + 131 * h + 7 * w + c).uniform(0.2, 1.0, size=(c, h, w))
    if content == "zeros":
        x[:, 10:19, 12:23] = 0.0
        x[:, h - 6:, w - 7:] = 0.0
        x[1] *= 0.02
    if content == "signed":
        x[:, 3::7, 2::5] *= -1.0
    return f32(x)


def rl_prior64(img: torch.Tensor, iters: int, lam: float, dtype=F64) -> torch.Tensor:
    """[C,H,W] -> [C,H,W]: `oracle.speinet_oracle.rl_prior` evaluated in `dtype`."""
    return O.rl_prior(img[None].to(dtype), iters, lam)[0]


def _rl_variant(img, iters, lam, box_valid=False, clamp=True, lap_on_img=False):
    x = img[:, None].to(F64)
    box = torch.ones(1, 1, 5, 5, dtype=F64)
    lap = torch.tensor([[0, -1, 0], [-1, 4, -1], [0, -1, 0]], dtype=F64).view(1, 1, 3, 3)
    count = F.conv2d(torch.ones_like(x), box, padding=2) if box_valid else 25.0
    d = x.clone()
    for _ in range(iters):
        corr = x / (F.conv2d(d, box, padding=2) / count)
        corr = torch.where(corr != corr, torch.zeros_like(corr), corr)
        if clamp:
            corr = torch.where(corr < 0, torch.zeros_like(corr), corr)
        d = corr * (d + lam * F.conv2d(x if lap_on_img else d, lap, padding=1))
    return d[:, 0]


# ------------------------------------------------------------------------------------------------------------------------------
# bicubic upsampling  (bicubic2x_kernel: s = 2 and C % 4 == 0; bicubic_kernel<4>: s = 4 and C % 4 == 0; bicubic_kernel<1>: the rest)
# ------------------------------------------------------------------------------------------------------------------------------
BICUBIC_SIZES = ((1, 1), (1, 7), (3, 1), (2, 3), (9, 7))
BICUBIC_KERNELS = {"2x": ((8, 2),), "vec4": ((8, 4),), "vec1": ((1, 2), (1, 4), (6, 2), (6, 4))}        # (C, s) per kernel
BICUBIC_LP_SIZES = ((2, 3), (9, 7))
BICUBIC_STRIDE = {"2x": (258, 255, 128, 2), "vec4": (129, 128, 32, 4), "vec1": (363, 362, 1, 4)}       # just past 8192 x 256 threads


def bicubic_cases():
    """(kernel, h, w, c, s, relu) of the dense fp32 cases."""
    return [(k, h, w, c, s, relu) for k, cs in BICUBIC_KERNELS.items() for c, s in cs for h, w in BICUBIC_SIZES for relu in (False, True)]


def bicubic_map(h, w, c, seed=0) -> torch.Tensor:
    """[H*W, C] N(0, 1): signed, so that the ReLU epilogue cuts about half of the outputs."""
    return f32(rng(2000 + 97 * h + 13 * w + c + seed).randn(h * w, c))


def bicubic64(x: torch.Tensor, h: int, w: int, s: int, relu: bool, dtype=F64) -> torch.Tensor:
    """[H*W, C] -> [sH*sW, C]: F.interpolate(bicubic, align_corners=False) (+ ReLU) evaluated in `dtype` (on x's device)."""
    c = x.shape[1]
    y = F.interpolate(x.to(dtype).view(h, w, c).permute(2, 0, 1)[None], scale_factor=s, mode="bicubic", align_corners=False)[0]
    y = F.relu(y) if relu else y
    return y.permute(1, 2, 0).reshape(s * h * s * w, c)


def _cubic_matrix(n, s, A, border, flip):
    """[s*n, n] float64: row o holds the four tap weights of output o (aten UpSampleBicubic2d: src = (o + 0.5) / s - 0.5)."""
    m = torch.zeros(s * n, n, dtype=F64)
    for o in range(s * n):
        src = (o + 0.5) / s - 0.5
        fl = math.floor(src)
        t = src - fl
        if flip:
            t = 1.0 - t
        near = lambda x: ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
        far = lambda x: ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
        for a, cf in enumerate((far(t + 1.0), near(t), near(1.0 - t), far(2.0 - t))):
            i = fl - 1 + a
            if border == "clamp" or n == 1:
                i = min(max(i, 0), n - 1)
            else:                                                       # reflect about the first / last sample
                i = abs(i) % (2 * (n - 1))
                i = 2 * (n - 1) - i if i >= n else i
            m[o, i] += cf
    return m


def bicubic_taps64(x, h, w, s, relu, A=-0.75, border="clamp", flip=False) -> torch.Tensor:
    """The same upsampling written out as two tap matrices; with its defaults it equals `bicubic64` (checked on the CPU)."""
    y = torch.einsum("ah,hwc,bw->abc", _cubic_matrix(h, s, A, border, flip), x.to(F64).view(h, w, -1), _cubic_matrix(w, s, A, border, flip))
    y = F.relu(y) if relu else y
    return y.reshape(s * h * s * w, -1)


# ------------------------------------------------------------------------------------------------------------------------------
# LayerNorm(256)  (one wave per row; the launch has at most 8192 x 4 waves)
# ------------------------------------------------------------------------------------------------------------------------------
LN_ROWS = (1, 3, 4, 5, 1000, 32773)
LN_HOST_ROWS = (1, 3, 4, 5, 1000)             # e_host is pooled over these; 32773 repeats their row kinds
LN_KINDS = ("gauss", "zero", "const7", "offset100", "tiny", "huge", "single")
assert LN_ROWS[-1] > 8192 * 4


def ln_rows(m: int, seed=0) -> torch.Tensor:
    """[M, 256]; row i is of kind LN_KINDS[i % 7]: N(0.5, 3), all zero, constant 7, mean 100 std 1, std 1e-4 (eps dominates), std 1e4,
    one nonzero element."""
    r = rng(3000 + m + seed)
    x = r.randn(m, DIM)
    k = np.arange(m) % len(LN_KINDS)
    x[k == 0] = x[k == 0] * 3.0 + 0.5
    x[k == 1] = 0.0
    x[k == 2] = 7.0
    x[k == 3] += 100.0
    x[k == 4] *= 1e-4
    x[k == 5] *= 1e4
    for i in np.nonzero(k == 6)[0]:
        x[i] = 0.0
        x[i, (37 * i) % DIM] = 3.0
    return f32(x)


def ln_affine():
    r = rng(3999)
    return f32(r.randn(DIM) * 0.2 + 1.0), f32(r.randn(DIM) * 0.1)


def layernorm64(x, g=None, b=None, dtype=F64, eps=1e-5) -> torch.Tensor:
    cast = lambda t: None if t is None else t.to(dtype)
    return F.layer_norm(x.to(dtype), (DIM,), cast(g), cast(b), eps)


def layernorm_twice64(x, g, b, dtype=F64) -> torch.Tensor:
    """LN(LN(x) * g + b) without a second affine: what spei_layernorm256_twice computes."""
    return layernorm64(layernorm64(x, g, b, dtype), None, None, dtype)


def _ln_onepass_fp32(x, g=None, b=None):
    """Wrong on purpose: var = E[x^2] - E[x]^2 with fp32 moments, each a running sum over the row (np.cumsum adds in sequence, so the
    figure does not depend on how a library vectorises a reduction)."""
    a = x.float().numpy()
    mean = np.cumsum(a, axis=1, dtype=np.float32)[:, -1:] / np.float32(DIM)
    var = np.cumsum(a * a, axis=1, dtype=np.float32)[:, -1:] / np.float32(DIM) - mean * mean
    assert mean.dtype == var.dtype == np.float32
    with np.errstate(invalid="ignore"):
        y = torch.from_numpy((a - mean) / np.sqrt(var + np.float32(1e-5))).to(F64)
    return y if g is None else y * g.to(F64) + b.to(F64)


@functools.lru_cache(maxsize=None)
def ln_case(m: int, affine: bool):
    """(x, g, b, float64 LayerNorm, float64 double LayerNorm) of one case; shared by every test of that case."""
    x = ln_rows(m)
    g, b = ln_affine()
    return x, g, b, (layernorm64(x, g, b) if affine else layernorm64(x)), layernorm_twice64(x, g, b)


# ------------------------------------------------------------------------------------------------------------------------------
# window attention core  (window_attention_kernel<float>: the attention of the f32 and bf16x3 modes)
# ------------------------------------------------------------------------------------------------------------------------------
ATTN_SIZES = ((5, 5), (5, 10), (10, 5), (10, 15))
ATTN_SHIFTS = (0, 1, 2, 3, 4)
ATTN_SETS = ("plain", "bias_only", "peaked", "offset", "uniform")
ATTN_LP_SIZES, ATTN_LP_SHIFTS = ((5, 5), (10, 15)), (0, 2)


def _regions(n, shift, edge=0):
    r = torch.zeros(n, dtype=torch.long)
    r[n - WS:n - shift - edge] = 1
    r[n - shift - edge:] = 2
    return r


def _window_regions(h, w, shift, edge=0):
    """[nW, 25] region id of every token of the shifted frame (edge: the wrong variant's boundary at n - shift - 1)."""
    reg = 3 * _regions(h, shift, edge)[:, None] + _regions(w, shift, edge)[None, :]
    return reg.view(h // WS, WS, w // WS, WS).permute(0, 2, 1, 3).reshape(-1, WS * WS)


def _attention(q, kv, relbias, h, w, shift, dtype, bias_t=False, head_xor=0, edge=0, roll_sign=-1, masked=True, swap_kv=False):
    nw = (h // WS) * (w // WS)

    def windows(t):                                    # [H*W, C] -> roll by -shift -> [nW, 25, C]
        c = t.shape[1]
        t = t.to(dtype).view(h, w, c)
        if shift:
            t = torch.roll(t, (roll_sign * shift, roll_sign * shift), (0, 1))
        return t.view(h // WS, WS, w // WS, WS, c).permute(0, 2, 1, 3, 4).reshape(nw, WS * WS, c)

    qw = windows(q).view(nw, 25, NH, HD).permute(0, 2, 1, 3)                        # [nW, 8, 25, 32]
    k, v = windows(kv).view(nw, 25, 2, NH, HD).permute(2, 0, 3, 1, 4)                # K then V, head-major
    if swap_kv:
        k, v = v, k
    rb = relbias.to(dtype)
    if bias_t:
        rb = rb.transpose(1, 2)
    if head_xor:
        rb = rb[torch.arange(NH) ^ head_xor]
    attn = qw @ k.transpose(-2, -1) + rb[None]
    if shift and masked:
        if edge:
            reg = _window_regions(h, w, shift, edge)
            differ = reg[:, None, :] != reg[:, :, None]
        else:
            differ = _shift_mask(h, w, WS, shift) != 0
        attn = attn + torch.where(differ, -100.0, 0.0).to(dtype)[:, None]
    out = (torch.softmax(attn, dim=-1) @ v).permute(0, 2, 1, 3).reshape(nw, WS, WS, DIM)
    out = out.view(h // WS, w // WS, WS, WS, DIM).permute(0, 2, 1, 3, 4).reshape(h, w, DIM)
    if shift:
        out = torch.roll(out, (-roll_sign * shift, -roll_sign * shift), (0, 1))
    return out.reshape(h * w, DIM)


def window_attention64(q, kv, relbias, h, w, shift, dtype=F64) -> torch.Tensor:
    """The core on the kernel's own operands: q [H*W][256] pre-scaled, kv [H*W][512] = K | V head-major, relbias [8][25][25].  Roll by
    -shift, 5 x 5 windows, 8 heads of 32, softmax(q k^T + relbias + mask) v, reverse, roll back; the mask is -100 between different
    regions of `speinet_amd.synth._shift_mask`."""
    return _attention(q, kv, relbias, h, w, shift, dtype)


def attn_operands(name: str, h: int, w: int, seed=0):
    """(q, kv, relbias) fp32 of one operand set.
    plain: N(0,1) q / kv, 0.3 sigma bias.  bias_only: q = 0 and a 3 sigma bias that is neither symmetric in (i, j) nor equal across
    heads: the probabilities are softmax(relbias + mask).  peaked: q x 2, no bias.  offset: q and K around 1.8, so that the mean score
    is 32 * 1.8^2 = 104 and exp overflows in fp32 without the max subtraction.  uniform: q = 0, no bias: the mean of V over the region."""
    r = rng(4000 + 31 * h + w + 1009 * ATTN_SETS.index(name) + seed)
    n = h * w
    q, kv, rb = r.randn(n, DIM), r.randn(n, 2 * DIM), r.randn(NH, 25, 25)
    if name == "plain":
        rb *= 0.3
    elif name == "bias_only":
        q[:], rb = 0.0, rb * 3.0
    elif name == "peaked":
        q, rb = q * 2.0, rb * 0.0
    elif name == "offset":
        q = 1.8 + 0.25 * q
        kv[:, :DIM] = 1.8 + 0.25 * kv[:, :DIM]
        rb *= 0.3
    elif name == "uniform":
        q[:], rb = 0.0, rb * 0.0
    return f32(q), f32(kv), f32(rb)


def attn_op(name: str) -> str:
    return "window_attention/" + name


def attn_cases():
    return [(name, h, w, shift) for name in ATTN_SETS for h, w in ATTN_SIZES for shift in ATTN_SHIFTS]


ATTN_BATCH_SIZES, ATTN_BATCH_SHIFTS, ATTN_BATCH = ((5, 10), (10, 15)), (0, 3), 3


def attn_batch_operands(name: str, h: int, w: int):
    """Three maps of one operand set stored one after the other (q [3*H*W, 256], kv [3*H*W, 512]) and the relbias they share."""
    maps = [attn_operands(name, h, w, seed=500 * i) for i in range(ATTN_BATCH)]
    return torch.cat([m[0] for m in maps]), torch.cat([m[1] for m in maps]), maps[0][2]


def attn_batch_cases():
    return [(name, h, w, shift) for name in ATTN_SETS for h, w in ATTN_BATCH_SIZES for shift in ATTN_BATCH_SHIFTS]


def region_mean64(kv, h, w, shift) -> torch.Tensor:
    """The `uniform` set's output written directly: every query gets the mean of V over the tokens of its window that lie in its
    own mask region.  (Through the softmax the other tokens weigh exp(-100) = 3.7e-44 each, far below any bound here.)"""
    v = kv[:, DIM:].to(F64).view(h, w, DIM)
    if shift:
        v = torch.roll(v, (-shift, -shift), (0, 1))
    out = torch.empty_like(v)
    reg = (3 * _regions(h, shift)[:, None] + _regions(w, shift)[None, :]) if shift else torch.zeros(h, w, dtype=torch.long)
    for y0 in range(0, h, WS):
        for x0 in range(0, w, WS):
            vw, rw = v[y0:y0 + WS, x0:x0 + WS], reg[y0:y0 + WS, x0:x0 + WS]
            ow = out[y0:y0 + WS, x0:x0 + WS]
            for r in rw.unique():
                ow[rw == r] = vw[rw == r].mean(dim=0)
    if shift:
        out = torch.roll(out, (shift, shift), (0, 1))
    return out.reshape(h * w, DIM)


# ------------------------------------------------------------------------------------------------------------------------------
# the pooled host-fp32 error of each operation
# ------------------------------------------------------------------------------------------------------------------------------
# The attention's error follows the size of its scores (the `offset` set's are near 104, and its host error is 70 times the
# `uniform` set's), so every operand set is an operation of its own here: pooled over all five, the `offset` figure would be the bound
# of the four well-conditioned sets.
ATTN_OPS = tuple("window_attention/" + name for name in ATTN_SETS)
OPS = ("rl_prior", "bicubic", "layernorm", "layernorm_twice") + ATTN_OPS


def host_errors(op: str) -> dict:
    """{case: max|host fp32 - float64| / max|float64|} over the operation's cases."""
    out = {}
    if op == "rl_prior":
        for case in rl_cases():
            h, w, c, it, lam, content = case
            x = rl_image(h, w, c, content)
            out[case] = nerr(rl_prior64(x, it, lam, torch.float32), rl_prior64(x, it, lam))
    elif op == "bicubic":
        for case in bicubic_cases():
            _, h, w, c, s, relu = case
            x = bicubic_map(h, w, c)
            out[case] = nerr(bicubic64(x, h, w, s, relu, torch.float32), bicubic64(x, h, w, s, relu))
    elif op in ("layernorm", "layernorm_twice"):
        for m in LN_HOST_ROWS:
            for affine in ((True, False) if op == "layernorm" else (True,)):
                x, g, b, want1, want2 = ln_case(m, affine)
                if op == "layernorm":
                    out[(m, affine)] = nerr(layernorm64(x, g, b, torch.float32) if affine else layernorm64(x, dtype=torch.float32), want1)
                else:
                    out[(m, affine)] = nerr(layernorm_twice64(x, g, b, torch.float32), want2)
    elif op in ATTN_OPS:
        for case in attn_cases():
            name, h, w, shift = case
            if attn_op(name) != op:
                continue
            q, kv, rb = attn_operands(name, h, w)
            out[case] = nerr(window_attention64(q, kv, rb, h, w, shift, torch.float32), window_attention64(q, kv, rb, h, w, shift))
        for name, h, w, shift in attn_batch_cases():
            if attn_op(name) == op:
                q, kv, rb = attn_batch_operands(name, h, w)
                for i in range(1, ATTN_BATCH):                           # map 0 is the single-map case above
                    qi, kvi = q[i * h * w:(i + 1) * h * w], kv[i * h * w:(i + 1) * h * w]
                    out[(name, h, w, shift, "map", i)] = nerr(window_attention64(qi, kvi, rb, h, w, shift, torch.float32),
                                                              window_attention64(qi, kvi, rb, h, w, shift))
    else:
        raise KeyError(op)
    return out


@functools.lru_cache(maxsize=None)
def e_host(op: str) -> float:
    return max(host_errors(op).values())


def bound(op: str) -> float:
    return FACTOR * e_host(op)


# ------------------------------------------------------------------------------------------------------------------------------
# deliberately wrong float64 versions: what the case tables must be able to see
# ------------------------------------------------------------------------------------------------------------------------------
def wrong_variants() -> dict:
    """{name: (operation, function with the signature of that operation's reference)}."""
    att = lambda **kw: (lambda q, kv, rb, h, w, shift: _attention(q, kv, rb, h, w, shift, F64, **kw))
    bic = lambda **kw: (lambda x, h, w, s, relu: bicubic_taps64(x, h, w, s, relu, **kw))
    rl = lambda **kw: (lambda img, iters, lam: _rl_variant(img, iters, lam, **kw))
    return {
        "attention: bias indexed [h][j][i]": ("window_attention", att(bias_t=True)),
        "attention: bias of head h ^ 1": ("window_attention", att(head_xor=1)),
        "attention: mask region boundary at n - shift - 1": ("window_attention", att(edge=1)),
        "attention: roll with the wrong sign": ("window_attention", att(roll_sign=1)),
        "attention: no mask": ("window_attention", att(masked=False)),
        "attention: K and V halves swapped": ("window_attention", att(swap_kv=True)),
        "layernorm: one-pass fp32 variance": ("layernorm", _ln_onepass_fp32),
        "layernorm: no eps": ("layernorm", lambda x, g=None, b=None: layernorm64(x, g, b, eps=0.0)),
        "bicubic: even / odd coefficient sets swapped": ("bicubic", bic(flip=True)),
        "bicubic: reflect instead of clamp": ("bicubic", bic(border="reflect")),
        "bicubic: A = -0.5": ("bicubic", bic(A=-0.5)),
        "rl_prior: box weights over the valid count": ("rl_prior", rl(box_valid=True)),
        "rl_prior: no negative clamp": ("rl_prior", rl(clamp=False)),
        "rl_prior: Laplacian on img instead of d": ("rl_prior", rl(lap_on_img=True)),
    }
