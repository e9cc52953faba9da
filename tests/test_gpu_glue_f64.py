"""GPU suite: the fp32 glue kernels that every precision mode runs on every frame -- csrc/stencil.hip (RL prior, bicubic upsampling,
add, the routing flag, rot90) and csrc/swin.hip (LayerNorm(256), the f32 window-attention core) -- against float64 statements of the
same operations (tests/glue_ref.py), at the shapes where each kernel changes path and on operands chosen so that every term of the
formula dominates somewhere.  tests/test_glue_ref_cpu.py shows that these cases see each of fourteen plausible mistakes.

Bound (after test_gpu_corr_exact.py::test_patch_invnorm_against_float64): with e_host the largest error of the same formula in fp32 on
the host over the operation's cases, each error over its case's max|float64|, a kernel's error is at most 4 e_host in every case.
The 4 allows for another order of summation and other fused multiply-adds; every bound is computed when the test runs and none
comes from a kernel.  A 16-bit output is within ulp16(float64) / 2 + 4 e_host max|float64| of float64: the rounding contract of
csrc/common.h held against float64, not against the kernel's own fp32 value.  add, any_nonzero and rot90 are exact (torch.equal).

Measured on the MI355X, largest kernel error as a multiple of e_host (the figures are in each test's docstring): RL prior 0.88, bicubic 1.16,
LayerNorm 1.08, double LayerNorm 1.26, attention 1.02 / 1.11 / 1.00 / 1.00 / 1.00 (plain, bias_only, peaked, offset, uniform).  No factor was raised
above 4, and no test found a fault in a kernel.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import glue_ref as R                                          # noqa: E402
from speinet_amd import _lib                                  # noqa: E402
from speinet_amd.ops import ACT_NONE, ACT_RELU, Ctx, FMap    # noqa: E402
from speinet_amd.pack import fmt_of                           # noqa: E402

DEV = "cuda:0"
LP = (torch.bfloat16, torch.float16)
ops = Ctx("f32", "bf16x3", device=DEV)


class Tally:
    """The errors of one operation's cases: prints e_host beside the largest, then holds every case to the bound."""

    def __init__(self, op: str, what: str = ""):
        self.what, self.e_host, self.rows, self.lp_rows = what or op, R.e_host(op), [], []
        assert self.e_host > 0

    def add(self, case, got: torch.Tensor, want: torch.Tensor):
        assert got.dtype == torch.float32 and got.shape == want.shape, (case, got.dtype, got.shape, want.shape)
        self.rows.append((R.nerr(got.cpu() if want.device.type == "cpu" else got, want), case))

    def add_lp(self, case, got: torch.Tensor, want: torch.Tensor, dtype):
        """A 16-bit output: the largest |got - want| / (ulp16(want) / 2 + 4 e_host max|want|) of the case, at most 1."""
        assert got.dtype == dtype and got.shape == want.shape, (case, got.dtype, got.shape, want.shape)
        self.lp_rows.append((R.lp_excess(got.cpu(), want, dtype, self.e_host), case))

    def check(self):
        bad = []
        if self.rows:
            err, case = max(self.rows, key=lambda r: r[0])
            print(f"{self.what}: e_host {self.e_host:.3e} (bound {R.FACTOR * self.e_host:.3e}); largest kernel error {err:.3e} = "
                  f"{err / self.e_host:.2f} e_host at {case}; {len(self.rows)} cases")
            bad += [f"{c}: {e:.3e} = {e / self.e_host:.2f} e_host" for e, c in self.rows if not e <= R.FACTOR * self.e_host]
        if self.lp_rows:
            ratio, case = max(self.lp_rows, key=lambda r: r[0])
            print(f"{self.what}: largest |kernel - float64| / (ulp16 / 2 + {R.FACTOR} e_host max|float64|) {ratio:.4f} at {case}; "
                  f"{len(self.lp_rows)} cases")
            bad += [f"{c}: {r:.4f} of the 16-bit allowance" for r, c in self.lp_rows if not r <= 1.0]
        assert self.rows or self.lp_rows
        assert not bad, f"{self.what}: over {R.FACTOR} e_host = {R.FACTOR * self.e_host:.3e}:\n" + "\n".join(bad)


def _vp(t):
    return C.c_void_p(t if isinstance(t, int) else t.data_ptr())


# ------------------------------------------------------------------------------------------------------------------------------
# RL prior
# ------------------------------------------------------------------------------------------------------------------------------
def rl_prior_into_nan(img: torch.Tensor, iters: int, lam: float) -> torch.Tensor:
    """spei_rl_prior with `out` and `scratch` both NaN before the launch."""
    c, h, w = img.shape
    out, scratch = torch.full_like(img, float("nan")), torch.full_like(img, float("nan"))
    _lib.check(_lib.lib().spei_rl_prior(_vp(img), _vp(out), _vp(scratch), c, h, w, iters, lam, ops._stream()), "spei_rl_prior")
    return out


@pytest.mark.parametrize("content", ["uniform", "zeros", "signed"])
def test_rl_prior(content):
    """Sizes that cut the 32 + 4 halo tile at every edge, both ping-pong parities of `iters` (the buffers start as NaN, so a result
    left in the scratch buffer shows), 1 / 3 / 4 planes, lam 0 / 0.01 / 0.1; the input stays as it was.  "zeros": out == 0 exactly
    where img == 0 (0 / 0 -> NaN -> 0 inside the 9 x 11 and 6 x 7 blocks) and finite everywhere.  "signed": 0 at the negative pixels.
    Measured on the MI355X: e_host 3.11e-7 (66 x 63, 3 iterations, lam 0.1), kernel 2.02e-7 on uniform content, 2.74e-7 with the zero blocks (33 x 65, 5 iterations; 0.88 e_host), 1.62e-7 on signed content."""
    tally = Tally("rl_prior", f"rl_prior[{content}]")
    for case in R.rl_cases():
        h, w, c, iters, lam, kind = case
        if kind != content:
            continue
        x = R.rl_image(h, w, c, kind)
        img = x.to(DEV)
        got = rl_prior_into_nan(img, iters, lam).cpu()
        assert torch.equal(img.cpu(), x), case
        assert torch.isfinite(got).all(), case
        if kind == "zeros":
            assert torch.equal(got == 0, x == 0), case
        if kind == "signed":
            assert (got[x < 0] == 0).all(), case
        tally.add(case, got, R.rl_prior64(x, iters, lam))
        assert torch.equal(ops.rl_prior(img, iters, lam).cpu(), got), case
    tally.check()


# ------------------------------------------------------------------------------------------------------------------------------
# bicubic upsampling
# ------------------------------------------------------------------------------------------------------------------------------
def upsample_into(src: FMap, dst: FMap, s: int, act: int):
    """spei_upsample_bicubic into an fp32 map the caller owns (`Ctx.upsample` allocates a dense one)."""
    assert src.t.dtype == dst.t.dtype == torch.float32 and (dst.H, dst.W, dst.C) == (s * src.H, s * src.W, src.C)
    _lib.check(_lib.lib().spei_upsample_bicubic(_vp(src.ptr), src.ld, _vp(dst.ptr), dst.ld, src.H, src.W, src.C, s, act, ops._stream()),
               "spei_upsample_bicubic")


def kernel_of(c, ldi, ldo, s):
    """The kernel `upsample_bicubic_run` picks for an fp32 output of 16-byte aligned maps (csrc/stencil.hip)."""
    v4 = c % 4 == 0 and ldi % 4 == 0 and ldo % 4 == 0
    return "2x" if v4 and s == 2 else ("vec4" if v4 else "vec1")


@pytest.mark.parametrize("kernel", list(R.BICUBIC_KERNELS))
def test_bicubic(kernel):
    """Each of the three kernels with and without its ReLU epilogue, at sizes where the clamped taps collapse (1 x 1: all of them;
    1 x 7, 3 x 1: one axis; 2 x 3) and at 9 x 7; the one-channel-per-thread kernel at C = 1 and C = 6.
    Measured on the MI355X: e_host 1.67e-7 (1 x 1, C = 6), kernel 1.06e-7 (bicubic2x_kernel), 1.94e-7 (bicubic_kernel<4>, 3 x 1 at s = 4; 1.16 e_host), 1.67e-7 (bicubic_kernel<1>)."""
    tally = Tally("bicubic", f"bicubic[{kernel}]")
    for case in R.bicubic_cases():
        k, h, w, c, s, relu = case
        if k != kernel:
            continue
        assert kernel_of(c, c, c, s) == kernel
        x = R.bicubic_map(h, w, c)
        got = ops.upsample(FMap(x.to(DEV), h, w, c), s, act=ACT_RELU if relu else ACT_NONE)
        assert (got.H, got.W, got.C) == (s * h, s * w, c)
        tally.add(case, got.t, R.bicubic64(x, h, w, s, relu))
    tally.check()


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("relu", [False, True])
def test_bicubic_channel_slice(s, relu):
    """Read channels [32, 96) of a 128-wide map, write channels [64, 128) of a 192-wide buffer (bicubic2x_kernel at s = 2,
    bicubic_kernel<4> at s = 4): the rest of that buffer keeps its bits."""
    h, w, c = 9, 7, 64
    tally = Tally("bicubic", f"bicubic slice s={s}")
    big = R.bicubic_map(h, w, 128, seed=5)
    buf = torch.from_numpy(R.rng(6).randn(s * h * s * w, 192).astype(np.float32))
    src = FMap(big.to(DEV), h, w, 128).view(32, c)
    dst = FMap(buf.to(DEV), s * h, s * w, 192).view(64, c)
    assert kernel_of(c, src.ld, dst.ld, s) == ("2x" if s == 2 else "vec4") and src.ptr % 16 == 0 and dst.ptr % 16 == 0
    upsample_into(src, dst, s, ACT_RELU if relu else ACT_NONE)
    after = dst.t.cpu()
    tally.add((h, w, c, s, relu), after[:, 64:128].contiguous(), R.bicubic64(big[:, 32:96], h, w, s, relu))
    assert torch.equal(after[:, :64].view(torch.int32), buf[:, :64].view(torch.int32))
    assert torch.equal(after[:, 128:].view(torch.int32), buf[:, 128:].view(torch.int32))
    tally.check()


@pytest.mark.parametrize("dtype", LP)
def test_bicubic_16bit_output_vs_float64(dtype):
    """bicubic2x_kernel<bf16 / f16> at 2 x 3 and 9 x 7, with and without ReLU: within half a unit of the format (+ 4 e_host) of float64.
    Measured on the MI355X: the largest |kernel - float64| is 0.998 of that allowance for bf16 and 0.994 for f16."""
    tally = Tally("bicubic", f"bicubic 16-bit {dtype}")
    for h, w in R.BICUBIC_LP_SIZES:
        for relu in (False, True):
            x = R.bicubic_map(h, w, 8)
            got = ops.upsample(FMap(x.to(DEV), h, w, 8), 2, act=ACT_RELU if relu else ACT_NONE, out_dtype=dtype)
            tally.add_lp((h, w, relu), got.t, R.bicubic64(x, h, w, 2, relu), dtype)
    tally.check()


@pytest.mark.parametrize("kernel", list(R.BICUBIC_STRIDE))
def test_bicubic_grid_stride(kernel):
    """One map per kernel just past 8192 blocks of 256 threads, so that the grid-stride loop takes a second step; float64 by torch on
    the device.  Measured on the MI355X: 1.47e-7 (2x), 1.51e-7 (VEC4), 1.52e-7 (VEC1; 0.91 e_host)."""
    h, w, c, s = R.BICUBIC_STRIDE[kernel]
    assert kernel_of(c, c, c, s) == kernel
    threads = h * w * (c // 4) if kernel == "2x" else s * h * s * w * (c // 4 if kernel == "vec4" else c)
    assert 8192 * 256 < threads < 8192 * 256 * 1.01
    tally = Tally("bicubic", f"bicubic grid stride [{kernel}]")
    x = torch.randn(h * w, c, generator=torch.Generator().manual_seed(h)).to(DEV)
    got = ops.upsample(FMap(x, h, w, c), s, act=ACT_RELU)
    tally.add((h, w, c, s), got.t, R.bicubic64(x, h, w, s, True))
    tally.check()


# ------------------------------------------------------------------------------------------------------------------------------
# LayerNorm(256), plain and twice
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("m", R.LN_ROWS)
def test_layernorm(m, out_dtype):
    """Rows of seven kinds in one tensor (N(0.5, 3); zero; constant 7; mean 100 std 1, where a one-pass variance is 0.4 % off; std 1e-4,
    where eps dominates; std 1e4; one nonzero element), with and without gamma / beta, to every output format; 32773 rows are past the
    launch's 8192 x 4 waves.  A zero or constant row gives exactly beta (0 without affine).  `layernorm_twice` against float64
    LN(LN(x) g + b).  Measured on the MI355X: layernorm e_host 1.54e-6, kernel 1.66e-6 (M = 5 with affine; 1.08 e_host); twice e_host 4.47e-7, kernel 5.62e-7 (M = 5; 1.26 e_host);
    16-bit outputs at most 0.9985 of their allowance (bf16, twice, M = 1000 and 32773)."""
    flat = torch.isin(torch.arange(m) % len(R.LN_KINDS), torch.tensor([R.LN_KINDS.index("zero"), R.LN_KINDS.index("const7")]))
    one, two = Tally("layernorm", f"layernorm {out_dtype}"), Tally("layernorm_twice", f"layernorm_twice {out_dtype}")
    for affine in (True, False):
        x, g, b, want1, want2 = R.ln_case(m, affine)
        xd, gd, bd = x.to(DEV), g.to(DEV), b.to(DEV)
        got = ops.layernorm(xd, gd, bd, out_dtype=out_dtype) if affine else ops.layernorm(xd, out_dtype=out_dtype)
        assert torch.equal(xd.cpu(), x)
        flat_want = (b if affine else torch.zeros(256)).to(out_dtype).expand(int(flat.sum()), 256)
        assert torch.equal(got.cpu()[flat], flat_want), (m, affine)
        if out_dtype == torch.float32:
            one.add((m, affine), got, want1)
        else:
            one.add_lp((m, affine), got, want1, out_dtype)
        if affine:
            got2 = ops.layernorm_twice(xd, gd, bd, out_dtype=out_dtype)
            if out_dtype == torch.float32:
                two.add((m,), got2, want2)
            else:
                two.add_lp((m,), got2, want2, out_dtype)
    one.check()
    two.check()


# ------------------------------------------------------------------------------------------------------------------------------
# window attention, f32 core
# ------------------------------------------------------------------------------------------------------------------------------
def attention(q, kv, rb, h, w, shift, batch=None):
    """spei_window_attention, or the batched entry on `batch` maps stored one after the other."""
    out = torch.full_like(q, float("nan"))
    lib, fmt = _lib.lib(), fmt_of(q.dtype)
    assert q.is_contiguous() and kv.is_contiguous() and rb.dtype == torch.float32 and q.dtype == kv.dtype
    if batch is None:
        assert q.shape == (h * w, 256) and kv.shape == (h * w, 512)
        _lib.check(lib.spei_window_attention(_vp(q), _vp(kv), fmt, _vp(rb), _vp(out), h, w, shift, ops._stream()), "spei_window_attention")
    else:
        assert q.shape == (batch * h * w, 256) and kv.shape == (batch * h * w, 512)
        _lib.check(lib.spei_window_attention_batched(_vp(q), _vp(kv), fmt, _vp(rb), _vp(out), h, w, shift, batch, ops._stream()),
                   "spei_window_attention_batched")
    return out


@pytest.mark.parametrize("name", R.ATTN_SETS)
def test_window_attention(name):
    """One operand set at 5 x 5 (one window), 5 x 10, 10 x 5 and 10 x 15 (all nine mask regions) with shifts 0 .. 4.  `uniform` is also
    held to the mean of V over the query's mask region, written without a softmax.
    Measured on the MI355X (e_host, which includes the maps of the batched test; kernel over both tests): plain 1.51e-6; 1.55e-6 (1.02 e_host).
    bias_only 3.39e-7; 3.77e-7 (1.11 e_host).  peaked 2.37e-6; 2.37e-6.  offset 1.37e-5; 1.37e-5.  uniform 1.91e-7; 1.91e-7, the same
    against the region mean."""
    tally, direct = Tally(R.attn_op(name)), Tally(R.attn_op(name), "uniform against the region mean")
    for case in R.attn_cases():
        _, h, w, shift = case
        if case[0] != name:
            continue
        q, kv, rb = R.attn_operands(name, h, w)
        got = attention(q.to(DEV), kv.to(DEV), rb.to(DEV), h, w, shift)
        tally.add(case, got, R.window_attention64(q, kv, rb, h, w, shift))
        if name == "uniform":
            direct.add(case, got, R.region_mean64(kv, h, w, shift))
        assert torch.equal(ops.window_attention(q.to(DEV), kv.to(DEV), rb.to(DEV), h, w, shift), got), case
    tally.check()
    if name == "uniform":
        direct.check()


@pytest.mark.parametrize("name", R.ATTN_SETS)
def test_window_attention_batched(name):
    """Three maps in one launch (blockIdx.y only offsets the pointers): every map has the bits of its own single-map call, and is
    within the bound."""
    tally = Tally(R.attn_op(name), f"{R.attn_op(name)} batched")
    for case in R.attn_batch_cases():
        _, h, w, shift = case
        if case[0] != name:
            continue
        q, kv, rb = R.attn_batch_operands(name, h, w)
        qd, kvd, rbd = q.to(DEV), kv.to(DEV), rb.to(DEV)
        got = attention(qd, kvd, rbd, h, w, shift, batch=R.ATTN_BATCH)
        n = h * w
        for i in range(R.ATTN_BATCH):
            rows = slice(i * n, (i + 1) * n)
            alone = attention(qd[rows].contiguous(), kvd[rows].contiguous(), rbd, h, w, shift)
            assert torch.equal(got[rows].view(torch.int32), alone.view(torch.int32)), (case, i)
            tally.add(case + (i,), got[rows], R.window_attention64(q[rows], kv[rows], rb, h, w, shift))
    tally.check()


@pytest.mark.parametrize("dtype", LP)
@pytest.mark.parametrize("name", R.ATTN_SETS)
def test_window_attention_16bit_io(name, dtype):
    """io_fmt bf16 / f16 at 5 x 5 and 10 x 15, shifts 0 and 2: operands rounded to the format first, float64 on the rounded operands,
    the output within half a unit of the format (+ 4 e_host) of it.  Measured on the MI355X: at most 0.9997 of that allowance (uniform, bf16, 10 x 15, shift 2)."""
    tally = Tally(R.attn_op(name), f"{R.attn_op(name)} {dtype}")
    for h, w in R.ATTN_LP_SIZES:
        for shift in R.ATTN_LP_SHIFTS:
            q, kv, rb = R.attn_operands(name, h, w)
            q, kv = q.to(dtype), kv.to(dtype)
            got = attention(q.to(DEV), kv.to(DEV), rb.to(DEV), h, w, shift)
            tally.add_lp((h, w, shift), got, R.window_attention64(q, kv, rb, h, w, shift), dtype)
    tally.check()


# ------------------------------------------------------------------------------------------------------------------------------
# exact glue
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4_195_507])
def test_add_equals_torch(n):
    """The scalar tail (n % 4) and, at 4 195 507 = 4 (4096 x 256 + 192) + 3, the loop past 4096 blocks with a 3-element tail; once with
    `out` aliasing `a`."""
    assert n < 6 or (n // 4 > 4096 * 256 and n % 4 == 3)
    gen = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=gen).to(DEV), torch.randn(n, generator=gen).to(DEV)
    want = a + b
    assert torch.equal(ops.add(a, b), want)
    a2 = a.clone()
    assert ops.add(a2, b, out=a2) is a2 and torch.equal(a2, want)


def flag_of(x: np.ndarray) -> int:
    t = torch.from_numpy(x).to(DEV)
    assert torch.equal(t.view(torch.int32).cpu(), torch.from_numpy(x).view(torch.int32))        # the copy kept every bit
    flag = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ops.any_nonzero(t, flag)
    return flag.item()


@pytest.mark.parametrize("n", [1, 4095, 8_392_707])
def test_any_nonzero_lone_last_element(n):
    """A lone nonzero in the last element; 8 392 707 is past the launch's 2048 x 256 x 16 elements.  All zeros, and all -0.0, give 0."""
    x = np.zeros(n, np.float32)
    assert flag_of(x) == 0
    assert flag_of(-x) == 0 and np.signbit(-x).all()
    x[-1] = 0.5
    assert flag_of(x) == 1


@pytest.mark.parametrize("value,want", [(np.float32(1e-40), 1), (-np.float32(1e-40), 1), (np.float32(1.4e-45), 1), (np.float32(np.inf), 1),
                                        (np.float32(-np.inf), 1), (np.float32(np.nan), 1)])
def test_any_nonzero_special_values(value, want):
    """The reference routes on torch.all(x == 0), which is false for a denormal: the kernel's compare must not flush it."""
    x = np.zeros(4095, np.float32)
    x[1234] = value
    assert x.view(np.int32)[1234] != 0
    assert flag_of(x) == want


def test_rot90_equals_torch():
    """258 x 255 x 128 is past 8192 blocks of 256 threads; then a channel-slice input (ldi 128, C 64)."""
    h, w, c = 258, 255, 128
    assert h * w * (c // 4) > 8192 * 256
    x = torch.randn(h * w, c, generator=torch.Generator().manual_seed(3)).to(DEV)

    def want(t, c_):                                                       # out[a][b] = in[b][W - 1 - a]
        return t.view(h, w, c_).transpose(0, 1).flip(0).reshape(w * h, c_)
    got = ops.rot90(FMap(x, h, w, c))
    assert (got.H, got.W, got.C) == (w, h, c) and torch.equal(got.t, want(x, c))
    got = ops.rot90(FMap(x, h, w, c).view(32, 64))
    assert (got.H, got.W, got.C) == (w, h, 64) and torch.equal(got.t, want(x[:, 32:96].contiguous(), 64))
