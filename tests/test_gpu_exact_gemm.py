"""GPU suite: the conv and GEMM kernels bit for bit on exact integer operands (tests/exact_ref.py).

The operands are integers that bf16 and f16 hold exactly, with every partial sum exact in fp32, so every arithmetic mode of every kernel
must return the float64 convolution itself, and a 16-bit output must be that value rounded once to nearest even.  Every comparison is
torch.equal on values: a dropped, doubled or misplaced term, a wrong zero fill, a stale tile or a wrong rounding fails at any seam, where
the max-norm tolerances of the older tests only bound operand rounding on real-valued data.  test_exact_ref_cpu.py checks the conditions
of every case of this file, and that torch.equal sees each such fault.  Each case asserts which C-ABI entry point took the call."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import exact_ref as E                             # noqa: E402
from speinet_amd import _lib, pack                # noqa: E402
from speinet_amd.ops import BMap, Ctx, FMap       # noqa: E402

DEV = "cuda:0"
LP = E.LP


class Spy:
    """Counts the launches of one C-ABI entry point."""
    def __init__(self, monkeypatch, name):
        lib = _lib.lib()
        self.n, fn = 0, getattr(lib, name)

        def call(*a):
            self.n += 1
            return fn(*a)
        monkeypatch.setattr(lib, name, call)


class took:
    """The block makes exactly `n` launches of the spied entry point (and none of `others`)."""
    def __init__(self, spy, n=1, others=()):
        self.spy, self.n, self.others = spy, n, others

    def __enter__(self):
        self.n0, self.o0 = self.spy.n, [o.n for o in self.others]

    def __exit__(self, et, ev, tb):
        if et is None:
            assert self.spy.n == self.n0 + self.n, "the intended kernel did not take the call"
            assert [o.n for o in self.others] == self.o0, "another kernel took a call"
        return False


def cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def dev_rows(x, dtype=torch.float32):
    """NCHW on the host -> the kernels' [batch*h*w, c] rows on the device, in `dtype` (exact: the operands fit every format)."""
    return E.rows(x).to(DEV).to(dtype)


def exact(got_rows, y64, width, label):
    """got_rows [maps*h*w, c] (any of the three formats) equals the float64 reference [maps,c,h,w] rounded once to that format."""
    got = got_rows.detach().cpu()
    want = E.rows(E.rounded(y64, got.dtype))
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape)
    if torch.equal(got, want):
        return
    bad = ~(got == want)
    idx = bad.nonzero()
    h = y64.shape[2]
    lines = []
    for r, c in idx[:12].tolist():
        m, p = divmod(r, h * width)
        lines.append(f"  map {m} y {p // width} x {p % width} channel {c}: got {got[r, c].item()} want {want[r, c].item()}")
    rws = idx[:, 0]
    ys = torch.unique((rws % (h * width)) // width)[:24].tolist()
    xs = torch.unique(rws % width)[:24].tolist()
    print(f"{label}: {int(bad.sum())} of {bad.numel()} values differ; rows y {ys} columns x {xs}\n" + "\n".join(lines))
    raise AssertionError(f"{label}: {int(bad.sum())} of {bad.numel()} values differ from the float64 result")


def formats(mode):
    """(input dtype, output dtype) pairs of a mode: the 16-bit modes take and write fp32 and their own format."""
    if mode in LP:
        return [(i, o) for i in (torch.float32, LP[mode]) for o in (torch.float32, LP[mode])]
    return [(torch.float32, torch.float32)]


MODES = ("f32", "bf16x3", "bf16", "f16")


def slab_ctx(mode):
    """The slab kernel (the f32 MFMA kernel in "f32") for every layer: the persistent kernels off."""
    return Ctx(mode, device=DEV, conv32_ws=False, conv3_pipe=False)


def igemm_spies(monkeypatch):
    return {"f32": Spy(monkeypatch, "spei_igemm_f32"), "slab": Spy(monkeypatch, "spei_conv_slab16")}


# ---- a. slab kernel and f32 MFMA kernel through Ctx.igemm --------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,k,stride,h,w", E.IGEMM_CASES + E.HEAD_CASES)
def test_igemm_conv_exact(cin, cout, k, stride, h, w, monkeypatch):
    """test_gpu_bf16.py::test_igemm_conv's shapes and the stride-2 head convs in all four modes, fp32 and 16-bit maps in and out: all
    equal the float64 conv, and so one another."""
    args = E.igemm_args(cin, cout, k, stride, h, w)
    o, y = E.operands(*args), E.conv_ref(*args)
    ho, wo = y.shape[2:]
    pw, b = pack.PackedW(pack.conv_w(o.w), DEV), o.bias.to(DEV)
    spies = igemm_spies(monkeypatch)
    for mode in MODES:
        ops = slab_ctx(mode)
        spy, other = (spies["f32"], spies["slab"]) if mode == "f32" else (spies["slab"], spies["f32"])
        for idt, odt in formats(mode):
            with took(spy, 1, (other,)):
                out = ops.igemm(FMap(dev_rows(o.x, idt), h, w, cin), pw, b, cout, ksize=k, stride=stride, out_dtype=odt)
            assert (out.H, out.W, out.t.dtype) == (ho, wo, odt)
            exact(out.t, y, wo, f"{mode} in {idt} out {odt}")


def test_igemm_concat_epilogue_exact(monkeypatch):
    """Two concatenated sources, ReLU, row scale and residual: act(conv + bias) * rowscale + residual."""
    c0, c1, cout, k, h, w = E.CONCAT_CASE
    args = E.concat_args()
    o = E.operands(*args)
    y = E.conv_ref(*args, relu=True, rowscale=True, residual=True, split=c0)
    pw, b = pack.PackedW(pack.conv_w(o.w), DEV), o.bias.to(DEV)
    res, rs = FMap(dev_rows(o.residual), h, w, cout), o.rowscale.reshape(-1).to(DEV)
    spies = igemm_spies(monkeypatch)
    for mode in MODES:
        ops = slab_ctx(mode)
        spy, other = (spies["f32"], spies["slab"]) if mode == "f32" else (spies["slab"], spies["f32"])
        for idt, odt in formats(mode):
            a0, a1 = FMap(dev_rows(o.x[:, :c0], idt), h, w, c0), FMap(dev_rows(o.x[:, c0:], idt), h, w, c1)
            with took(spy, 1, (other,)):
                out = ops.igemm(a0, pw, b, cout, ksize=k, a1=a1, act=ops.ACT_RELU, residual=res, rowscale=rs, out_dtype=odt)
            exact(out.t, y, w, f"{mode} in {idt} out {odt}")


@pytest.mark.parametrize("m,kdim,n", E.LINEAR_CASES)
def test_linear_exact(m, kdim, n, monkeypatch):
    """Token-list linears with a residual (Ctx.linear: a 1x1 conv on an m x 1 map), ragged last row tiles."""
    args = E.linear_args(m, kdim, n)
    o = E.linear_operands(*args)
    y = E.linear_ref(*args, residual=True).t().reshape(1, n, m, 1)
    pw, b, res = pack.PackedW(o.w.reshape(1, n, kdim), DEV), o.bias.to(DEV), dev_rows(o.residual)
    spies = igemm_spies(monkeypatch)
    for mode in MODES:
        ops = slab_ctx(mode)
        spy, other = (spies["f32"], spies["slab"]) if mode == "f32" else (spies["slab"], spies["f32"])
        for idt, odt in formats(mode):
            with took(spy, 1, (other,)):
                out = ops.linear(dev_rows(o.x, idt), pw, b, residual=res, out_dtype=odt)
            assert out.dtype == odt
            exact(out, y, 1, f"{mode} in {idt} out {odt}")


# ---- b. igemm_batched on the slab kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("maps,h,w", E.BATCHED_SHAPES)
@pytest.mark.parametrize("c,k", E.BATCHED_LAYERS)
def test_batched_slab_exact(mode, maps, h, w, c, k, monkeypatch):
    """Several maps per launch of the slab kernel, with the residual aliased to the output and without a residual: every map equals the
    float64 conv and its own single-map launch."""
    args = E.batched_args(c, k, maps, h, w)
    o = E.operands(*args)
    y, yres = E.conv_ref(*args), E.conv_ref(*args, residual=True)
    ops = slab_ctx(mode)
    pw, b, n = pack.PackedW(pack.conv_w(o.w), DEV), o.bias.to(DEV), h * w
    batched, single = Spy(monkeypatch, "spei_conv_slab16_batched"), Spy(monkeypatch, "spei_conv_slab16")
    persistent = [Spy(monkeypatch, s) for s in ("spei_conv32_ws16", "spei_conv64_ws16", "spei_conv3x3_256_pipe16")]
    for idt, odt in formats(mode):
        xin = dev_rows(o.x, idt)
        with took(batched, 1, persistent):
            out = ops.igemm_batched(BMap(xin, maps, h, w, c), pw, b, c, k, out_dtype=odt)
        exact(out.t, y, w, f"{mode} in {idt} out {odt}")
        with took(single, maps, persistent):
            for m in range(maps):
                one = ops.igemm(FMap(xin[m * n:(m + 1) * n], h, w, c), pw, b, c, ksize=k, out_dtype=odt)
                assert torch.equal(one.t, out.t[m * n:(m + 1) * n]), f"map {m} differs from its own launch"
        if odt != torch.float32:
            continue
        res = dev_rows(o.residual)
        rb = BMap(res.clone(), maps, h, w, c)
        with took(batched, 1, persistent):
            out = ops.igemm_batched(BMap(xin, maps, h, w, c), pw, b, c, k, residual=rb, out=rb)        # in place on the residual
        exact(out.t, yres, w, f"{mode} in {idt} residual in place")
        with took(single, maps, persistent):
            for m in range(maps):
                one = ops.igemm(FMap(xin[m * n:(m + 1) * n], h, w, c), pw, b, c, ksize=k, residual=FMap(res[m * n:(m + 1) * n], h, w, c))
                assert torch.equal(one.t, out.t[m * n:(m + 1) * n]), f"map {m} with residual differs from its own launch"


# ---- c. weight-stationary kernels ---------------------------------------------------------------------------------------------------------
def ws_case(mode, c, maps, h, w, monkeypatch):
    args = E.ws_args(c, maps, h, w)
    o = E.operands(*args)
    ops = Ctx(mode, device=DEV)
    pw, b = pack.PackedW(pack.conv_w(o.w), DEV), o.bias.to(DEV)
    ws = Spy(monkeypatch, f"spei_conv{c}_ws16")
    slab = [Spy(monkeypatch, s) for s in ("spei_conv_slab16_batched", "spei_conv_slab16")]
    for relu in (False, True):
        y = E.conv_ref(*args, relu=relu)
        for idt, odt in formats(mode):
            with took(ws, 1, slab):
                out = ops.igemm_batched(BMap(dev_rows(o.x, idt), maps, h, w, c), pw, b, c, 5, act=ops.ACT_RELU if relu else ops.ACT_NONE,
                                        out_dtype=odt)
            exact(out.t, y, w, f"conv{c}_ws16 {mode} {maps}x{h}x{w} in {idt} out {odt} relu {relu}")


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("maps,h,w", E.WS_SMALL)
@pytest.mark.parametrize("c", [32, 64])
def test_weight_stationary_exact(mode, c, maps, h, w, monkeypatch):
    """spei_conv32_ws16 / spei_conv64_ws16: a map smaller than a tile, one pixel past a tile column, ragged both ways over several maps."""
    ws_case(mode, c, maps, h, w, monkeypatch)


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("c", [32, 64])
def test_weight_stationary_walk_exact(mode, c, monkeypatch):
    """The persistent workgroups' tile walk: more than twice as many tiles as the device has CUs and no multiple of them, so workgroups
    take two or three tiles from different maps, prefetch into both LDS buffers and return to the first; ragged last tile row and column."""
    n = cus()
    maps, h, w = E.ws_walk_shape(c, n)
    tiles = E.tiles_of(maps, h, w, E.WS_TILES[c])
    assert tiles > 2 * n and tiles % n and maps >= 3 and h % E.WS_TILES[c][0] and w % E.WS_TILES[c][1]
    ws_case(mode, c, maps, h, w, monkeypatch)


# ---- d. the persistent 3x3 / 256-channel kernel -------------------------------------------------------------------------------------------
def pipe_case(mode, amp, maps, h, w, monkeypatch, fallback=False):
    args = E.pipe_args(amp, maps, h, w)
    o = E.operands(*args)
    ops = Ctx(mode, device=DEV)
    pw, b = pack.PackedW(pack.conv_w(o.w), DEV), o.bias.to(DEV)
    pipe, slab = Spy(monkeypatch, "spei_conv3x3_256_pipe16"), Spy(monkeypatch, "spei_conv_slab16_batched")
    spy, other = (slab, pipe) if fallback else (pipe, slab)
    xin = BMap(dev_rows(o.x), maps, h, w, 256)
    rb = BMap(dev_rows(o.residual), maps, h, w, 256)
    with took(spy, 1, (other,)):
        out = ops.igemm_batched(xin, pw, b, 256, 3, residual=rb, out=rb)             # in place on the residual, as engine.swin_multi calls it
    exact(out.t, E.conv_ref(*args, residual=True), w, f"{mode} {amp} {maps}x{h}x{w} residual in place")
    with took(spy, 1, (other,)):
        out = ops.igemm_batched(xin, pw, b, 256, 3)
    exact(out.t, E.conv_ref(*args), w, f"{mode} {amp} {maps}x{h}x{w} no residual")


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("amp", E.PIPE_SETS)
@pytest.mark.parametrize("maps,h,w", E.PIPE_SHAPES)
def test_conv3_pipe_exact(mode, amp, maps, h, w, monkeypatch):
    pipe_case(mode, amp, maps, h, w, monkeypatch)


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("amp", E.PIPE_SETS)
def test_conv3_pipe_fallback_exact(mode, amp, monkeypatch):
    """6 x 16 tiles do not cover a 10-row map: the slab kernel takes the call and is exact too."""
    pipe_case(mode, amp, *E.PIPE_FALLBACK, monkeypatch, fallback=True)


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("amp", E.PIPE_SETS)
def test_conv3_pipe_walk_exact(mode, amp, monkeypatch):
    """The tile walk of the pipelined kernel (the next tile's halo is staged inside the current tile's k-steps): more than 2 * CUs whole
    tiles, no multiple of the CUs, several maps."""
    n = cus()
    maps, h, w = E.pipe_walk_shape(n)
    tiles = E.tiles_of(maps, h, w, E.PIPE_TILE)
    assert tiles > 2 * n and tiles % n and maps >= 2 and h % 6 == 0 and w % 16 == 0
    pipe_case(mode, amp, maps, h, w, monkeypatch)


# ---- e. transposed conv ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,h,w", E.CONVT_CASES)
def test_conv_transpose_exact(cin, cout, h, w, monkeypatch):
    """3x3 stride-2 transposed conv: the four-class kernel in bf16 / f16 (fp32 and 16-bit maps in and out), its split form in bf16x3 and
    the f32 kernel's CONV_T path, with and without ReLU, against conv_transpose2d in float64."""
    args = E.convt_args(cin, cout, h, w)
    o = E.operands(*args)
    pw, b = pack.PackedW(pack.convT_w(o.w), DEV), o.bias.to(DEV)
    names = {"f32": "spei_igemm_f32", "bf16x3": "spei_convt2_slab16x3", "bf16": "spei_convt2_slab16", "f16": "spei_convt2_slab16"}
    spies = {n: Spy(monkeypatch, n) for n in set(names.values()) | {"spei_conv_slab16"}}
    for relu in (False, True):
        y = E.conv_ref(*args, relu=relu)
        for mode in MODES:
            ops = Ctx(mode, device=DEV)
            spy = spies[names[mode]]
            for idt, odt in formats(mode):
                with took(spy, 1, [s for s in spies.values() if s is not spy]):
                    out = ops.igemm(FMap(dev_rows(o.x, idt), h, w, cin), pw, b, cout, ksize=3, stride=2, mode=ops.CONV_T,
                                    act=ops.ACT_RELU if relu else ops.ACT_NONE, out_dtype=odt)
                assert (out.H, out.W) == (2 * h, 2 * w)
                exact(out.t, y, 2 * w, f"{mode} in {idt} out {odt} relu {relu}")


# ---- f. first and last conv -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", E.IO_SHAPES)
def test_conv5_in_exact(h, w, monkeypatch):
    """3 -> 32 channels, NCHW planes in, NHWC out, bias and ReLU (spei_conv5_in)."""
    args = E.conv5_in_args(h, w)
    o = E.operands(*args)
    spy = Spy(monkeypatch, "spei_conv5_in")
    with took(spy):
        out = Ctx("f32", device=DEV).conv5_in(o.x[0].to(DEV), pack.conv_w(o.w).to(DEV), o.bias.to(DEV))
    exact(out.t, E.conv_ref(*args, relu=True), w, "conv5_in")


@pytest.mark.parametrize("h,w", E.IO_SHAPES)
def test_conv5_out_exact(h, w, monkeypatch):
    """32 -> 3 channels, NHWC in, three NCHW planes out: the fp32 kernel, and the slab kernel in bf16 / f16 on fp32 and 16-bit maps with the
    weights zero-padded to 32 output channels as pack._pack_common builds them."""
    args = E.conv5_out_args(h, w)
    o = E.operands(*args)
    y = E.rounded(E.conv_ref(*args), torch.float32)[0]
    tail_w, tail_b = pack.conv_w(o.w), o.bias
    w32 = pack.PackedW(torch.cat((tail_w, torch.zeros(25, 29, tail_w.shape[2])), 1), DEV)
    b32 = torch.cat((tail_b, torch.zeros(29))).to(DEV)
    f32k, slab = Spy(monkeypatch, "spei_conv5_out"), Spy(monkeypatch, "spei_conv5_out_slab16")

    def same(out, label):
        got = out.cpu()
        bad = ~(got == y)
        if bad.any():
            print(f"{label}: {int(bad.sum())} of {bad.numel()} differ; first (channel, y, x, got, want): "
                  + ", ".join(str((*i, got[tuple(i)].item(), y[tuple(i)].item())) for i in bad.nonzero()[:12].tolist()))
        assert not bad.any(), label

    out = torch.full((3, h, w), float("nan"), device=DEV)
    with took(f32k, 1, (slab,)):
        Ctx("f32", device=DEV).conv5_out(FMap(dev_rows(o.x), h, w, 32), tail_w.to(DEV), tail_b.to(DEV), out)
    same(out, "conv5_out f32")
    for mode in ("bf16", "f16"):
        for idt in (torch.float32, LP[mode]):
            out = torch.full((3, h, w), float("nan"), device=DEV)
            with took(slab, 1, (f32k,)):
                Ctx(mode, device=DEV).conv5_out(FMap(dev_rows(o.x, idt), h, w, 32), tail_w.to(DEV), tail_b.to(DEV), out, w32, b32)
            same(out, f"conv5_out_slab16 {mode} in {idt}")
