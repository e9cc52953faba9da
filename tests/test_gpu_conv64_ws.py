"""GPU suite: the weight-stationary 64 -> 64 channel 5x5 kernel (csrc/conv64_ws16.hip, the ResBlock convs at half resolution).

Against the float64 convolution of what the kernel sees (16-bit operands where the mode rounds them) and against the slab kernel it
replaces (same operand rounding, other summation order); every map of a multi-map launch must equal its own single-map launch bit for
bit, because the frame's encoder passes run batched and the decoder runs single maps (test_batched_encoder_bit_identical).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from speinet_amd import _lib, pack                # noqa: E402
from speinet_amd.ops import BMap, Ctx, FMap       # noqa: E402

DEV = "cuda:0"
TOL = {"bf16": 1.5e-2, "f16": 2e-3}
LPD = {"bf16": torch.bfloat16, "f16": torch.float16}


def rnd(seed, *shape, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).randn(*shape) * scale).astype(np.float32))


def relerr(a, b):
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    assert a.shape == b.shape and torch.isfinite(a).all()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def layer(seed):
    wt = rnd(seed, 64, 64, 5, 5, scale=1.0 / np.sqrt(64 * 25))
    b = rnd(seed + 1, 64, scale=0.1)
    return wt, b, pack.PackedW(pack.conv_w(wt), DEV)


def ref_rows(x, wt, b, r0, r1, relu):
    """float64 conv (padding 2) of NCHW maps x, output rows [r0, r1) only."""
    H = x.shape[2]
    lo, hi = max(r0 - 2, 0), min(r1 + 2, H)
    xs = F.pad(x[:, :, lo:hi].double(), (2, 2, 2 - (r0 - lo), 2 - (hi - r1)))
    y = F.conv2d(xs, wt.double(), b.double())
    return (F.relu(y) if relu else y).float()


class Spy:
    """Counts the launches of one C-ABI entry point."""
    def __init__(self, monkeypatch, name):
        lib = _lib.lib()
        self.n, fn = 0, getattr(lib, name)

        def call(*a):
            self.n += 1
            return fn(*a)
        monkeypatch.setattr(lib, name, call)


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("h,w,batch", [(6, 32, 1), (12, 64, 2), (7, 33, 1), (5, 7, 2), (37, 50, 3), (40, 150, 2)])
def test_conv64_weight_stationary(mode, h, w, batch, monkeypatch):
    """Whole and ragged tiles, maps smaller than a tile, several maps per launch, fp32 and 16-bit inputs and outputs, ReLU on and off."""
    ops, slab = Ctx(mode, device=DEV), Ctx(mode, device=DEV, conv64_ws=False)
    lp = LPD[mode]
    x = rnd(80 + h, batch, 64, h, w)
    wt, b, pw = layer(81)
    bd = b.to(DEV)
    rows = x.permute(0, 2, 3, 1).reshape(batch * h * w, 64).contiguous().to(DEV)
    ws_calls = Spy(monkeypatch, "spei_conv64_ws16")
    for in16 in (False, True):
        xin = rows.to(lp) if in16 else rows
        xr = xin.float().view(batch, h, w, 64).permute(0, 3, 1, 2).cpu()               # what the kernel sees
        for relu in (False, True):
            ref = ref_rows(xr, wt, b, 0, h, relu)
            act = ops.ACT_RELU if relu else ops.ACT_NONE
            for o16 in (True, False):
                odt = lp if o16 else torch.float32
                n0 = ws_calls.n
                out = ops.igemm_batched(BMap(xin, batch, h, w, 64), pw, bd, 64, 5, act=act, out_dtype=odt)
                assert ws_calls.n == n0 + 1
                got = out.t.float().view(batch, h, w, 64).permute(0, 3, 1, 2)
                e = relerr(got, ref)
                assert e < TOL[mode], f"{mode} in16={in16} relu={relu} o16={o16}: rel err {e:.2e}"
                old = slab.igemm_batched(BMap(xin, batch, h, w, 64), pw, bd, 64, 5, act=act, out_dtype=odt)
                assert ws_calls.n == n0 + 1
                assert relerr(out.t.float(), old.t.float()) < TOL[mode]
                for m in range(batch):                                                   # each map as it comes out alone
                    one = ops.igemm(FMap(xin[m * h * w:(m + 1) * h * w].contiguous(), h, w, 64), pw, bd, 64, ksize=5, act=act,
                                    out_dtype=odt)
                    assert torch.equal(one.t, out.t[m * h * w:(m + 1) * h * w])
                assert ws_calls.n == n0 + 1 + batch


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_conv64_weight_stationary_720p_level(mode):
    """The frame's shape: 7 stacked 360 x 640 maps (the half-resolution encoder level of a 720p frame's passes).  float64 rows at the
    top, middle and bottom of the first and last map; the whole launch against the slab kernel; maps 0 and 6 against their own launch."""
    h, w, batch = 360, 640, 7
    ops, slab = Ctx(mode, device=DEV), Ctx(mode, device=DEV, conv32_ws=False)
    lp = LPD[mode]
    wt, b, pw = layer(91)
    bd = b.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(92)
    xin = torch.randn(batch * h * w, 64, device=DEV, generator=g).to(lp)
    out = ops.igemm_batched(BMap(xin, batch, h, w, 64), pw, bd, 64, 5, act=ops.ACT_RELU, out_dtype=lp)
    old = slab.igemm_batched(BMap(xin, batch, h, w, 64), pw, bd, 64, 5, act=ops.ACT_RELU, out_dtype=lp)
    assert relerr(out.t.float(), old.t.float()) < TOL[mode]
    for m in (0, batch - 1):
        xm = xin[m * h * w:(m + 1) * h * w]
        one = ops.igemm(FMap(xm.contiguous(), h, w, 64), pw, bd, 64, ksize=5, act=ops.ACT_RELU, out_dtype=lp)
        assert torch.equal(one.t, out.t[m * h * w:(m + 1) * h * w])
        xr = xm.float().view(1, h, w, 64).permute(0, 3, 1, 2).cpu()
        got = out.t[m * h * w:(m + 1) * h * w].float().view(1, h, w, 64).permute(0, 3, 1, 2).cpu()
        for r0, r1 in ((0, 8), (175, 185), (352, 360)):
            e = relerr(got[:, :, r0:r1], ref_rows(xr, wt, b, r0, r1, True))
            assert e < TOL[mode], f"{mode} map {m} rows [{r0}, {r1}): rel err {e:.2e}"


@pytest.mark.parametrize("knobs", [{"conv64_ws": False}, {"conv32_ws": False}, {"conv32_ws": False, "conv64_ws": True}])
def test_conv64_ws_routing(knobs, monkeypatch):
    """conv64_ws=False, and conv32_ws=False with conv64_ws left at None, put the 64-channel 5x5 layers on the slab kernel (one map and
    batched); conv64_ws=True overrides conv32_ws=False."""
    ctx = Ctx("f16", device=DEV, **knobs)
    want_ws = knobs.get("conv64_ws", knobs.get("conv32_ws", True))
    assert ctx.conv64_ws_available() == want_ws
    ws, sl, sl1 = (Spy(monkeypatch, n) for n in ("spei_conv64_ws16", "spei_conv_slab16_batched", "spei_conv_slab16"))
    wt, b, pw = layer(95)
    x = torch.randn(2 * 20 * 40, 64, device=DEV).half()
    ctx.igemm_batched(BMap(x, 2, 20, 40, 64), pw, b.to(DEV), 64, 5, act=ctx.ACT_RELU, out_dtype=torch.float16)
    ctx.igemm(FMap(x[:800].contiguous(), 20, 40, 64), pw, b.to(DEV), 64, ksize=5, out_dtype=torch.float16)
    assert ws.n == (2 if want_ws else 0)
    assert sl.n + sl1.n == (0 if want_ws else 2)
