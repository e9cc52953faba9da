"""GPU suite: every entry point of csrc/resblock.hip but the routed apply -- spei_resblock_gates, _gates_batched, _apply, _apply_batched,
called through the C-ABI as ops.Ctx calls them -- against the float64 statement of tests/gates_ref.py, for x1 stored as fp32, bf16 and
f16 and C = 32, 64, 128.  The bound on |kernel - float64| is derived there from the fp32 roundings, not fitted; the shapes are the
smallest that reach each path of the kernels (gates_ref.ROWS: degenerate maps, one tile and one line over, 3 / 4 / 5 column and row
tiles, a gate-map block boundary, the SE block's unrolled tile walk) and the contents are those on which a lost mask, a dropped line
or tile, a wrong denominator or halo line leaves the bound (tests/test_gates_ref_cpu.py shows that on the float64 statement; no kernel
is mutated here).  The gated sum is held bit for bit on integer operands and to its five roundings on Gaussian ones, and one ResBlock
of `ops.resblock_batched` is held to the float64 gates and sum of the kernel's own x1.  (The routed apply is tied bit for bit to the
dense one by test_gpu_handoff16.py::test_routed_apply.)

Largest |kernel - float64| / tol measured on an MI355X over all cases of this file, per output and x1 format:

    x1       s        g1       g2       apply    resblock_batched
    fp32     0.187    0.056    0.070    0.458    -
    bf16     0.217    0.061    0.064    0.463    0.138
    f16      0.217    0.055    0.071    0.505    0.147

s: the figures come from the integer content of the SE row at C = 32, whose bound has no length terms and is little more than the 4u s
allowed for expf, the addition and the reciprocal -- one rounding of s is a quarter of it; on every other case s stays under 0.04.
g1, g2: as the fp32 evaluation on the CPU (0.05 to 0.1).  apply: the kernel rounds four times (five with `extra`) and the bound
allows five roundings of the full magnitude, so over some 10^5 Gaussian elements the largest comes to half of it; no term is missing.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gates_ref as R                                            # noqa: E402
from speinet_amd import _lib, pack                               # noqa: E402
from speinet_amd.ops import ACT_RELU, BMap, Ctx                  # noqa: E402

DEV = "cuda:0"
BLOCK = {32: "recons_net.inBlock.1.", 64: "recons_net.encoder_first.1.", 128: "recons_net.encoder_second.1."}
DTYPE = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
FMT = {"fp32": pack.F32, "bf16": pack.BF16, "f16": pack.F16}
GATE_KEYS = ("se_w1", "se_b1", "se_w2", "se_b2", "cw_w", "cw_bn", "hc_w", "hc_bn")
OUTPUTS = ("s", "g1", "g2")


def vp(t):
    assert t is None or (t.is_cuda and t.is_contiguous())
    return C.c_void_p(0 if t is None else t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(x: np.ndarray, fmt: str = "fp32") -> torch.Tensor:
    """x on the device in `fmt`; the values must be representable (the reference sees the bits the kernel sees)."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV).to(DTYPE[fmt])
    assert torch.equal(t.double().cpu(), torch.from_numpy(np.ascontiguousarray(x))), f"content is not exact in {fmt}"
    return t


@pytest.fixture(scope="module")
def gate_params(synth_sd):
    """c -> (the gate parameters on the device, the same as float64 numpy)."""
    out = {}
    for c in R.CHANNELS:
        pk = pack.resblock(synth_sd, BLOCK[c])
        out[c] = ({k: pk[k].to(DEV).contiguous() for k in GATE_KEYS}, R.pk64(pk))
    return out


def run_gates(maps, fmt, pkd, batched):
    """s [B, C], g1 [B, H, C], g2 [B, W, C] of the maps [B, H, W, C]; outputs and workspace start as NaN."""
    b, h, w, c = maps.shape
    lib = _lib.lib()
    x1 = dev(maps, fmt)
    wsf = lib.spei_gate_ws_floats(h, w, c)
    assert wsf > 0
    nan = float("nan")
    ws = torch.full((b * wsf,), nan, device=DEV)
    s, g1, g2 = (torch.full(sh, nan, device=DEV) for sh in ((b, c), (b, h, c), (b, w, c)))
    par = [vp(pkd[k]) for k in GATE_KEYS]
    if batched:
        _lib.check(lib.spei_resblock_gates_batched(vp(x1), FMT[fmt], b, h, w, c, *par, vp(s), vp(g1), vp(g2), vp(ws), stream()),
                   "spei_resblock_gates_batched")
    else:
        assert b == 1
        _lib.check(lib.spei_resblock_gates(vp(x1), FMT[fmt], h, w, c, *par, vp(s), vp(g1), vp(g2), vp(ws), stream()), "spei_resblock_gates")
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (s, g1, g2))


def gate_ratios(got, ref, what):
    """|kernel - float64| / tol per output; asserts that every value is finite and within its bound."""
    out = {}
    for g, n in zip(got, OUTPUTS):
        assert np.isfinite(g).all(), f"{what}: {n} is not finite"
        want, tol = getattr(ref, n), getattr(ref, "tol_" + n)
        assert g.shape == want.shape
        ratio = np.abs(g.astype(np.float64) - want) / tol
        out[n] = float(ratio.max())
        i = np.unravel_index(ratio.argmax(), ratio.shape)
        assert out[n] <= 1.0, f"{what}: {n}{list(i)} kernel {g[i]!r} float64 {want[i]!r} |difference| / tol = {out[n]:.3g}"
    return out


def report(fmt, what, ratios):
    print(f"RATIO {fmt} {what}: " + " ".join(f"{n}={v:.4f}" for n, v in ratios.items()))


@pytest.mark.parametrize("row", list(R.ROWS))
@pytest.mark.parametrize("c", R.CHANNELS)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_gates_vs_float64(gate_params, fmt, c, row):
    pkd, pk = gate_params[c]
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for h, w, fam, exact, seed in R.cases(row, c, fmt):
        if row == "se_walk":
            # the unrolled tile walk must run: fail loudly if the tiling moves the case below the threshold
            nty, ntx = R.tiles(h, w, c, fmt)
            nty32 = R.tiles(h, w, c, "fp32")[0]
            assert _lib.lib().spei_gate_ws_floats(h, w, c) == 2 * ntx * h * c + 2 * nty32 * w * c + ntx * nty32 * c, "the statistics tiling changed"
            assert R.se_unrolled(h, w, c, fmt) and nty * ntx > 7 * (1024 // c), (nty, ntx)
        x1 = R.content(fam, h, w, c, fmt, seed)
        s, g1, g2 = run_gates(x1[None], fmt, pkd, batched=False)
        rt = gate_ratios((s[0], g1[0], g2[0]), R.gates_f64(x1, pk, exact), f"{h}x{w}x{c} {fmt} {fam}")
        worst = {n: max(worst[n], rt[n]) for n in OUTPUTS}
    report(fmt, f"gates C={c} {row}", worst)


@pytest.mark.parametrize("row,idx", R.BATCHED)
@pytest.mark.parametrize("c", R.CHANNELS)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_gates_batched(gate_params, fmt, c, row, idx):
    """Three maps of different content in one launch: each within the bound of its own float64 gates, and bit for bit what the
    single-map entry point gives on that map alone (the partials are combined in a fixed order)."""
    pkd, pk = gate_params[c]
    h, w = R.ROWS[row][1](c, fmt)[idx]
    maps = np.stack([R.content(fam, h, w, c, fmt, 50 + j) for j, fam in enumerate(R.BATCHED_FAMILIES)])
    got = run_gates(maps, fmt, pkd, batched=True)
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for b in range(len(maps)):
        rt = gate_ratios([g[b] for g in got], R.gates_f64(maps[b], pk), f"map {b} of {h}x{w}x{c} {fmt}")
        worst = {n: max(worst[n], rt[n]) for n in OUTPUTS}
        alone = run_gates(maps[b:b + 1], fmt, pkd, batched=False)
        for n, g, a in zip(OUTPUTS, got, alone):
            assert np.array_equal(g[b].view(np.int32), a[0].view(np.int32)), f"map {b}: {n} differs from the single-map launch"
    report(fmt, f"gates batched C={c} {h}x{w}", worst)


# ---- the gated sum ------------------------------------------------------------------------------------------------------------------
SENTINEL = 7.0


def run_apply(ops_, fmt, batched=False, ldo=None, off=0):
    """The gated sum of x, x1 [B, H, W, C], s [B, C], g1 [B, H, C], g2 [B, W, C], extra: out [B, H, W, C], and the columns of the
    destination rows outside [off, off + C) (sentinels)."""
    x, x1, s, g1, g2, extra = ops_
    b, h, w, c = x.shape
    lib = _lib.lib()
    ldo = c if ldo is None else ldo
    buf = torch.full((b * h * w, ldo), SENTINEL, device=DEV)
    dst = C.c_void_p(buf.data_ptr() + 4 * off)
    t = [dev(x), dev(x1, fmt), dev(s), dev(g1), dev(g2), None if extra is None else dev(extra)]
    if batched:
        assert extra is None and ldo == c and off == 0
        _lib.check(lib.spei_resblock_apply_batched(vp(t[0]), vp(t[1]), FMT[fmt], vp(t[2]), vp(t[3]), vp(t[4]), dst, b, h, w, c, stream()),
                   "spei_resblock_apply_batched")
    else:
        assert b == 1
        _lib.check(lib.spei_resblock_apply(vp(t[0]), vp(t[1]), FMT[fmt], vp(t[2]), vp(t[3]), vp(t[4]), vp(t[5]), dst, ldo, h, w, c, stream()),
                   "spei_resblock_apply")
    torch.cuda.synchronize()
    full = buf.cpu().numpy()
    rest = np.concatenate([full[:, :off], full[:, off + c:]], axis=1)
    return full[:, off:off + c].reshape(b, h, w, c), rest


def exact_sum(ops_):
    x, x1, s, g1, g2, extra = ops_
    return np.stack([R.apply_i64(x[m], x1[m], s[m], g1[m], g2[m], None if extra is None else extra[m]) for m in range(len(x))]).astype(np.float32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


@pytest.mark.parametrize("extra", [False, True])
@pytest.mark.parametrize("h,w", [(3, 5), (17, 33)])
@pytest.mark.parametrize("c", R.CHANNELS)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_apply_exact(fmt, c, h, w, extra):
    """Integer operands in [-4, 4]: every evaluation order is exact, so the kernel must give the int64 statement's values bit for bit."""
    ops_ = R.apply_ints(1, h, w, c, 11 * c + h, extra)
    out, _ = run_apply(ops_, fmt)
    assert same_bits(out, exact_sum(ops_))


@pytest.mark.parametrize("c", R.CHANNELS)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_apply_exact_strided_destination(fmt, c):
    """Destination rows of 384 floats, the map at column 128 of them, `extra` given: the other columns keep their sentinel."""
    ops_ = R.apply_ints(1, 17, 33, c, 13 * c, True)
    out, rest = run_apply(ops_, fmt, ldo=384, off=128)
    assert same_bits(out, exact_sum(ops_))
    assert rest.shape == (17 * 33, 384 - c) and (rest == SENTINEL).all()


@pytest.mark.parametrize("c", R.CHANNELS)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_apply_exact_batched(fmt, c):
    ops_ = R.apply_ints(3, 17, 33, c, 17 * c, False)
    out, _ = run_apply(ops_, fmt, batched=True)
    assert same_bits(out, exact_sum(ops_))


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_apply_exact_grid_stride(fmt):
    """One 260 x 260 x 128 map: 2 163 200 thread quads, more than the launch's 8192 x 256 threads, so the grid-stride loop runs."""
    h = w = 260
    assert h * w * 32 > 8192 * 256
    ops_ = R.apply_ints(1, h, w, 128, 19, False)
    out, _ = run_apply(ops_, fmt)
    assert same_bits(out, exact_sum(ops_))


@pytest.mark.parametrize("h,w", [(3, 5), (17, 33)])
@pytest.mark.parametrize("c", R.CHANNELS)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_apply_vs_float64(fmt, c, h, w):
    """Gaussian operands, with and without `extra`, and three maps through the batched entry point."""
    worst = 0.0
    for b, extra, batched in ((1, False, False), (1, True, False), (3, False, True)):
        ops_ = R.apply_gauss(b, h, w, c, fmt, 23 * c + w + b, extra)
        out, _ = run_apply(ops_, fmt, batched=batched)
        assert np.isfinite(out).all()
        x, x1, s, g1, g2, e = ops_
        for m in range(b):
            want, tol = R.apply_f64(x[m], x1[m], s[m], g1[m], g2[m], None if e is None else e[m])
            ratio = float((np.abs(out[m].astype(np.float64) - want) / tol).max())
            assert ratio <= 1.0, (b, extra, m, ratio)
            worst = max(worst, ratio)
    report(fmt, f"apply C={c} {h}x{w}", {"apply": worst})


# ---- one ResBlock through the wrapper -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_resblock_batched_vs_float64(synth_sd, mode):
    """`ops.resblock_batched` on two maps: the float64 gates and gated sum of the kernel's own x1 (read back with the two conv calls
    the wrapper makes, so the convolutions' rounding is not part of the bound).  The bound is that of the sum plus what the gates'
    own bounds contribute through it, |x1| (tol_s + tol_g1 + tol_g2)."""
    b, h, w, c = 2, 17, 33, 64
    ctx = Ctx(mode, device=DEV)
    raw = pack.resblock(synth_sd, BLOCK[c])
    pkd = {k: (pack.PackedW(v.t, DEV) if isinstance(v, pack.GemmW) else v.to(DEV).contiguous()) for k, v in raw.items()}
    pk = R.pk64(raw)
    xs = R.round_to(np.random.RandomState(31).randn(b, h, w, c), "fp32")
    x = BMap(dev(xs.reshape(b * h * w, c)), b, h, w, c)
    out = ctx.resblock_batched(x, pkd).t.cpu().numpy().reshape(b, h, w, c)
    idt = ctx.inter_dtype()
    t = ctx.igemm_batched(x, pkd["w1"], pkd["b1"], c, 5, act=ACT_RELU, out_dtype=idt)
    x1 = ctx.igemm_batched(t, pkd["w2"], pkd["b2"], c, 5, out_dtype=idt)
    assert x1.t.dtype == DTYPE[mode] and (x1.B, x1.H, x1.W, x1.C) == (b, h, w, c)
    x1s = x1.t.double().cpu().numpy().reshape(b, h, w, c)
    assert np.isfinite(out).all() and len({m.tobytes() for m in x1s}) == b and np.abs(x1s).max() > 0.01
    worst = 0.0
    for m in range(b):
        g = R.gates_f64(x1s[m], pk)
        want, tol = R.apply_f64(xs[m], x1s[m], g.s, g.g1, g.g2)
        tol = tol + np.abs(x1s[m]) * (g.tol_s + g.tol_g1[:, None, :] + g.tol_g2[None, :, :])
        ratio = float((np.abs(out[m].astype(np.float64) - want) / tol).max())
        assert ratio <= 1.0, (m, ratio)
        worst = max(worst, ratio)
    report(mode, "resblock_batched", {"out": worst})
