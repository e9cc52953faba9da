"""GPU suite: `Ctx.handoff16` — maps whose every reader stages them as the operand of a single-product 16-bit conv are written in 16 bits
by their producer.  The consumer rounds the same fp32 values to the same format while staging, so every check here is
bit for bit (torch.equal): the routed batched apply (csrc/resblock.hip) against the dense one followed by `.to(16-bit)` and `spei_add`,
the batched stride-2 head conv on 16-bit maps against fp32 maps holding the rounded values, the bicubic x2 upsampler's 16-bit output
against its fp32 output rounded, the double LayerNorm against two launches, and whole frames with the knob on against off."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from speinet_amd import _lib, pack                         # noqa: E402
from speinet_amd.ops import ACT_NONE, ACT_RELU, BMap, Ctx, FMap  # noqa: E402
from speinet_amd.speinet import SPEINet, default_args      # noqa: E402
from speinet_amd.synth import synth_frames                 # noqa: E402

DEV = "cuda:0"
LPD = {"bf16": torch.bfloat16, "f16": torch.float16}
BLOCK = {32: "recons_net.inBlock.1.", 64: "recons_net.encoder_first.1.", 128: "recons_net.encoder_second.1."}


def rnd(seed, *shape, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).randn(*shape) * scale).astype(np.float32))


class Spy:
    """Counts the launches of one C-ABI entry point."""
    def __init__(self, monkeypatch, name):
        lib = _lib.lib()
        self.n, fn = 0, getattr(lib, name)

        def call(*a):
            self.n += 1
            return fn(*a)
        monkeypatch.setattr(lib, name, call)


def gate_params(synth_sd, c):
    return {k: v.to(DEV).contiguous() for k, v in pack.resblock(synth_sd, BLOCK[c]).items() if torch.is_tensor(v)}


def apply_inputs(mode, b, h, w, c, seed, x1_dtype=None):
    x = BMap(rnd(seed, b * h * w, c).to(DEV), b, h, w, c)
    x1 = BMap(rnd(seed + 1, b * h * w, c, scale=0.7).to(DEV).to(LPD[mode] if x1_dtype is None else x1_dtype), b, h, w, c)
    return x, x1


@pytest.mark.parametrize("mode", ["f16", "bf16"])
@pytest.mark.parametrize("c", [32, 64, 128])
@pytest.mark.parametrize("h,w", [(3, 5), (17, 33)])
def test_routed_apply(synth_sd, mode, c, h, w):
    """Seven maps as the encoder hands them over: the pair sums (1 -> 0), (3 -> 2), (5 -> 4) and map 6 to an fp32 and a 16-bit
    destination; six maps without a reference; every map to a 16-bit destination of its own with fp32 for one of them (levels 1 and
    2); an fp32 destination with row stride 384 at C = 128; an fp32 x1.  Reference: the dense batched apply, `.to(16-bit)`, spei_add."""
    ctx = Ctx(mode, device=DEV)
    lp, pk = LPD[mode], gate_params(synth_sd, c)
    x, x1 = apply_inputs(mode, 7, h, w, c, 100 + c)
    dense = ctx._gates_apply_batched(x, x1, pk)
    sums = [ctx.add(dense.map(2 * k + 1).t, dense.map(2 * k).t) for k in range(3)]
    # level 3, with and without the reference map
    for nmaps in (7, 6):
        xs, x1s = (BMap(t.t[:nmaps * h * w], nmaps, h, w, c) for t in (x, x1))
        dst = [FMap.empty(h, w, c, DEV) for _ in range(3)]
        cat = FMap(torch.full((h * w, 384), 7.0, device=DEV), h, w, 384)
        if c == 128:
            dst[0] = cat.view(0, 128)
        routes = [(2 * k + 1, 2 * k, dst[k], None) for k in range(3)]
        if nmaps == 7:
            o32, o16 = FMap.empty(h, w, c, DEV), FMap.empty(h, w, c, DEV, lp)
            routes.append((6, None, o32, o16))
        assert ctx._gates_apply_batched(xs, x1s, pk, routes) is None
        for k in range(3):
            assert torch.equal(dst[k].t[:, :c], sums[k]), (nmaps, k)
        if c == 128:
            assert (cat.t[:, 128:] == 7.0).all()            # the strided destination's neighbours are untouched
        if nmaps == 7:
            assert torch.equal(o32.t, dense.map(6).t) and torch.equal(o16.t, dense.map(6).t.to(lp))
    # levels 1 and 2: 16-bit for every map, fp32 for the reference pass only
    nxt, keep = BMap.empty(7, h, w, c, DEV, lp), FMap.empty(h, w, c, DEV)
    ctx._gates_apply_batched(x, x1, pk, [(i, None, keep if i == 6 else None, nxt.map(i)) for i in range(7)])
    assert torch.equal(nxt.t, dense.t.to(lp)) and torch.equal(keep.t, dense.map(6).t)
    # fp32 x1 (x1_bf16 off)
    xf, x1f = apply_inputs(mode, 2, h, w, c, 300 + c, torch.float32)
    densef = ctx._gates_apply_batched(xf, x1f, pk)
    o32, o16 = FMap.empty(h, w, c, DEV), FMap.empty(h, w, c, DEV, lp)
    ctx._gates_apply_batched(xf, x1f, pk, [(1, 0, o32, o16)])
    want = ctx.add(densef.map(1).t, densef.map(0).t)
    assert torch.equal(o32.t, want) and torch.equal(o16.t, want.to(lp))


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_routed_apply_grid_stride(synth_sd, mode):
    """One 260 x 260 x 128 map: 2 163 200 thread quads, more than the launch's 8192 x 256 threads, so the grid-stride loop runs."""
    ctx = Ctx(mode, device=DEV)
    h = w = 260
    assert h * w * 32 > 8192 * 256
    pk = gate_params(synth_sd, 128)
    x, x1 = apply_inputs(mode, 1, h, w, 128, 500)
    dense = ctx._gates_apply_batched(x, x1, pk)
    o32, o16 = FMap.empty(h, w, 128, DEV), FMap.empty(h, w, 128, DEV, LPD[mode])
    ctx._gates_apply_batched(x, x1, pk, [(0, None, o32, o16)])
    assert torch.equal(o32.t, dense.t) and torch.equal(o16.t, dense.t.to(LPD[mode]))


@pytest.mark.parametrize("mode", ["f16", "bf16"])
@pytest.mark.parametrize("cin,cout", [(32, 64), (64, 128)])
@pytest.mark.parametrize("h,w", [(11, 13), (34, 66)])
def test_head_conv_16bit_input(mode, cin, cout, h, w):
    """The batched stride-2 5x5 head conv of an encoder stage on three 16-bit maps against fp32 maps holding the same rounded values:
    the same tile choice and accumulation order, so the same bits (34 x 66 crosses an output tile edge)."""
    ctx = Ctx(mode, device=DEV)
    wt = pack.PackedW(pack.conv_w(rnd(1, cout, cin, 5, 5, scale=1.0 / np.sqrt(cin * 25))), DEV)
    b = rnd(2, cout, scale=0.1).to(DEV)
    a16 = BMap(rnd(3, 3 * h * w, cin).to(DEV).to(LPD[mode]), 3, h, w, cin)
    a32 = BMap(a16.t.float(), 3, h, w, cin)
    got = ctx.igemm_batched(a16, wt, b, cout, 5, stride=2, act=ACT_RELU)
    want = ctx.igemm_batched(a32, wt, b, cout, 5, stride=2, act=ACT_RELU)
    assert got.t.dtype == torch.float32 and torch.equal(got.t, want.t)


@pytest.mark.parametrize("mode", ["f16", "bf16"])
@pytest.mark.parametrize("c", [32, 64])
@pytest.mark.parametrize("h,w", [(2, 3), (5, 7), (17, 33)])
@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU])
def test_bicubic2x_16bit_output(mode, c, h, w, act):
    ctx = Ctx(mode, device=DEV)
    f = FMap(rnd(7, h * w, c).to(DEV), h, w, c)
    got = ctx.upsample(f, 2, act=act, out_dtype=LPD[mode])
    want = ctx.upsample(f, 2, act=act)
    assert got.t.dtype == LPD[mode] and (got.H, got.W, got.C) == (2 * h, 2 * w, c)
    assert torch.equal(got.t, want.t.to(LPD[mode]))


@pytest.mark.parametrize("out_dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1000])
def test_layernorm_twice(rows, out_dtype):
    ctx = Ctx("f16", device=DEV)
    x = (rnd(11, rows, 256) * 1.3 + 0.2).to(DEV)
    g, b = (rnd(12, 256) * 0.2 + 1.0).to(DEV), rnd(13, 256, scale=0.1).to(DEV)
    got = ctx.layernorm_twice(x, g, b, out_dtype=out_dtype)
    want = ctx.layernorm(ctx.layernorm(x, g, b), out_dtype=out_dtype)
    assert got.dtype == out_dtype and torch.equal(got, want)


@pytest.fixture(scope="module")
def net(synth_sd):
    n = SPEINet(args=default_args())
    n.load_state_dict(synth_sd, strict=True)
    return n.to(DEV).eval()


@pytest.mark.parametrize("mode", ["f16", "bf16"])
@pytest.mark.parametrize("b,h,w,zero_ref", [(2, 40, 60, (1,)), (1, 100, 100, ())])
def test_frame_bit_identical(net, monkeypatch, mode, b, h, w, zero_ref):
    """Whole frames with `handoff16` on (the default) against off: the outputs and what SearchTransfer decided (arg-max, S) are equal,
    eager and as a hipGraph; the routed apply and the double LayerNorm run only with the knob on."""
    x = synth_frames(b, h, w, seed=91, zero_ref=zero_ref).to(DEV)
    routed, twice = Spy(monkeypatch, "spei_resblock_apply_routed"), Spy(monkeypatch, "spei_layernorm256_twice")
    net.precision, net.corr_precision = mode, "top2"
    try:
        outs, caps = {}, {}
        for on in (False, True):
            net.knobs = {} if on else {"handoff16": False}
            caps[on] = {}
            with torch.no_grad():
                outs[on] = net(x, capture=caps[on]).clone()
            assert (routed.n > 0 and twice.n > 0) == on
        assert torch.equal(outs[True], outs[False]), (outs[True] - outs[False]).abs().max().item()
        assert caps[True].keys() == caps[False].keys() and len(caps[True]) > 0
        for k in caps[True]:
            assert torch.equal(caps[True][k], caps[False][k]), k
        net.knobs, net.use_graph = {}, True
        with torch.no_grad():
            net(x)
            assert torch.equal(net(x), outs[False])
    finally:
        net.knobs, net.use_graph = {}, False
        net.precision, net.corr_precision = "f32", "bf16x3"


def test_consumer_ctx_decides(net, monkeypatch):
    """The decode maps follow the consumer's Ctx: with the `glue1` stage overridden to split (bf16x3) arithmetic its operands stay fp32 (no
    16-bit upsampler launch) while the encoder hand-offs, whose consumers are unchanged, stay routed — and the frame is still the one
    with the knob off.  An f32-grade frame takes none of the new launches."""
    x = synth_frames(1, 40, 60, seed=92).to(DEV)
    up16, routed, twice = (Spy(monkeypatch, n) for n in ("spei_upsample_bicubic_fmt", "spei_resblock_apply_routed", "spei_layernorm256_twice"))
    split_glue1 = {"stage": {"glue1": {"precision": "bf16x3"}}}
    net.precision, net.corr_precision = "f16", "top2"
    try:
        with torch.no_grad():
            net.knobs = dict(split_glue1, handoff16=False)
            off = net(x).clone()
            assert (up16.n, routed.n, twice.n) == (0, 0, 0)
            net.knobs = split_glue1
            on = net(x).clone()
            assert up16.n == 0 and routed.n == 3 and twice.n == 1
            assert torch.equal(on, off)
            net.knobs = {}
            net(x)
            assert up16.n == 2                      # upsample(f_lv2) and s13
            net.precision, net.corr_precision = "bf16x3", "bf16x3"
            net(x)
            assert (up16.n, routed.n, twice.n) == (2, 6, 2)
    finally:
        net.knobs = {}
        net.precision, net.corr_precision = "f32", "bf16x3"
