"""GPU suite, 16-bit matrix-pipe modes of the GEMM-shaped kernels.

  bf16x3  split-bf16 products (3 MFMAs): f32-grade.  Tolerance 2e-5 * max|ref| per kernel; end to end the same
          bounds as the f32 path (1e-3 absolute, PSNR delta <= 1e-3 dB) and bit-exact arg-max on the golden cases.
  f16     single IEEE-half products, fp32 accumulate — the THROUGHPUT configuration (bench.py's default, with the "top2"
          correlation): per kernel 2^-11-ish relative error of each operand, tolerance 2e-3 * max|ref|; end to end
          |dPSNR| <= 1e-3 dB against the reference's own outputs (the north-star bound) at every golden size.
  bf16    single bf16 products: per kernel tolerance 1.5e-2 * max|ref|; end to end 0.05 absolute on an O(1) image and
          1e-2 dB (measured 3e-3 dB at 720p: 8-bit significands of weights and activations).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import speinet_oracle as O           # noqa: E402
from speinet_amd import engine, pack             # noqa: E402
from speinet_amd.ops import Ctx                  # noqa: E402
from speinet_amd.ops import FMap                 # noqa: E402
from speinet_amd.speinet import SPEINet, default_args  # noqa: E402
from speinet_amd.synth import synth_frames       # noqa: E402

DEV = "cuda:0"
TOL = {"bf16x3": 2e-5, "bf16": 1.5e-2, "f16": 2e-3}
LPD = {"bf16": torch.bfloat16, "f16": torch.float16}


def g(golden_dir, name):
    d = np.load(os.path.join(golden_dir, name + ".npz"))
    return {k: (torch.from_numpy(d[k]) if d[k].ndim > 0 else d[k].item()) for k in d.files}


def rnd(seed, *shape, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).randn(*shape) * scale).astype(np.float32))


def fm(x):
    return FMap.from_nchw(x.to(DEV))


def relerr(a, b):
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    assert a.shape == b.shape and torch.isfinite(a).all()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16", "f16"])
@pytest.mark.parametrize("cin,cout,k,stride,h,w", [
    (32, 32, 5, 1, 20, 24), (64, 64, 5, 1, 13, 17), (128, 128, 5, 1, 10, 15), (32, 64, 5, 2, 40, 60),
    (64, 128, 5, 2, 22, 18), (128, 256, 3, 1, 10, 15), (256, 256, 3, 1, 9, 11), (256, 128, 3, 1, 10, 15),
    (384, 128, 1, 1, 10, 15), (64, 32, 1, 1, 21, 19), (96, 32, 3, 1, 21, 19), (512, 256, 1, 1, 33, 7)])
def test_igemm_conv(mode, cin, cout, k, stride, h, w):
    ops = Ctx(mode, device=DEV)
    x = rnd(1, 1, cin, h, w)
    wt = rnd(2, cout, cin, k, k, scale=1.0 / np.sqrt(cin * k * k))
    b = rnd(3, cout, scale=0.1)
    ref = F.conv2d(x.double(), wt.double(), b.double(), stride=stride, padding=k // 2).float()
    out = ops.igemm(fm(x), pack.conv_w(wt).to(DEV), b.to(DEV), cout, ksize=k, stride=stride)
    e = relerr(out.nchw(), ref)
    assert e < TOL[mode], f"{mode}: rel err {e:.2e}"


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("h,w,batch", [(16, 32, 1), (20, 36, 1), (37, 50, 3), (5, 7, 2), (48, 160, 2), (180, 320, 1)])
def test_conv32_weight_stationary(mode, h, w, batch):
    """The weight-stationary 32 -> 32 channel 5x5 kernel (csrc/conv32_ws16.hip: the ResBlock convs at full resolution) against the
    float64 convolution and against the slab kernel it replaces (same operand rounding, other summation order): whole and ragged
    tiles, maps smaller than a tile, several maps per launch (each as it comes out alone), fp32 and 16-bit inputs and outputs, ReLU."""
    from speinet_amd.ops import BMap
    ops, slab = Ctx(mode, device=DEV), Ctx(mode, device=DEV, conv32_ws=False)
    lp = LPD[mode]
    x = rnd(70 + h, batch, 32, h, w)
    wt = rnd(71, 32, 32, 5, 5, scale=1.0 / np.sqrt(32 * 25))
    b = rnd(72, 32, scale=0.1)
    pw = pack.PackedW(pack.conv_w(wt), DEV)
    rows = x.permute(0, 2, 3, 1).reshape(batch * h * w, 32).contiguous().to(DEV)
    for in16 in (False, True):
        xin = rows.to(lp) if in16 else rows
        xr = xin.float().view(batch, h, w, 32).permute(0, 3, 1, 2).cpu()               # what the kernel sees
        for relu in (False, True):
            ref = F.conv2d(xr.double(), wt.double(), b.double(), padding=2)
            ref = (F.relu(ref) if relu else ref).float()
            act = ops.ACT_RELU if relu else ops.ACT_NONE
            for o16 in (True, False):
                odt = lp if o16 else torch.float32
                out = ops.igemm_batched(BMap(xin, batch, h, w, 32), pw, b.to(DEV), 32, 5, act=act, out_dtype=odt)
                got = out.t.float().view(batch, h, w, 32).permute(0, 3, 1, 2)
                e = relerr(got, ref)
                assert e < TOL[mode], f"{mode} in16={in16} relu={relu} o16={o16}: rel err {e:.2e}"
                old = slab.igemm_batched(BMap(xin, batch, h, w, 32), pw, b.to(DEV), 32, 5, act=act, out_dtype=odt)
                assert relerr(out.t.float(), old.t.float()) < TOL[mode]
                one = ops.igemm(FMap(xin[:h * w], h, w, 32), pw, b.to(DEV), 32, ksize=5, act=act, out_dtype=odt)   # map 0 alone
                assert torch.equal(one.t, out.t[:h * w])
                if batch > 1:
                    last = ops.igemm(FMap(xin[-h * w:].contiguous(), h, w, 32), pw, b.to(DEV), 32, ksize=5, act=act, out_dtype=odt)
                    assert torch.equal(last.t, out.t[-h * w:])


@pytest.mark.parametrize("mode", ["bf16x3", "bf16", "f16"])
def test_igemm_concat_transpose_epilogue(mode):
    ops = Ctx(mode, device=DEV)
    h, w = 14, 22
    xa, xb = rnd(4, 1, 64, h, w), rnd(5, 1, 32, h, w)
    wt, b, res = rnd(6, 64, 96, 3, 3, scale=0.05), rnd(7, 64, scale=0.1), rnd(8, 1, 64, h, w)
    rs = torch.rand(h * w, generator=torch.Generator().manual_seed(9))
    ref = F.gelu(F.conv2d(torch.cat((xa, xb), 1), wt, b, padding=1)) * rs.view(1, 1, h, w) + res
    out = ops.igemm(fm(xa), pack.conv_w(wt).to(DEV), b.to(DEV), 64, ksize=3, a1=fm(xb), act=ops.ACT_GELU, residual=fm(res), rowscale=rs.to(DEV))
    assert relerr(out.nchw(), ref) < TOL[mode]
    x = rnd(12, 1, 128, 10, 15)
    wtt, bt = rnd(13, 128, 64, 3, 3, scale=0.05), rnd(14, 64, scale=0.1)
    ref = F.relu(F.conv_transpose2d(x, wtt, bt, stride=2, padding=1, output_padding=1))
    out = ops.igemm(fm(x), pack.convT_w(wtt).to(DEV), bt.to(DEV), 64, ksize=3, stride=2, mode=ops.CONV_T, act=ops.ACT_RELU)
    assert relerr(out.nchw(), ref) < TOL[mode]
    # second decoder tail shape (64 -> 32), odd map, no activation; in "bf16" mode both run as four parity-class convs on the slab kernel
    x = rnd(15, 1, 64, 21, 19)
    wtt, bt = rnd(16, 64, 32, 3, 3, scale=0.05), rnd(17, 32, scale=0.1)
    ref = F.conv_transpose2d(x, wtt, bt, stride=2, padding=1, output_padding=1)
    out = ops.igemm(fm(x), pack.convT_w(wtt).to(DEV), bt.to(DEV), 32, ksize=3, stride=2, mode=ops.CONV_T)
    assert relerr(out.nchw(), ref) < TOL[mode]


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_conv3x3_256_pipe_vs_conv2d(mode):
    """The persistent 3x3 / 256-channel kernel of the Swin body (spei_conv3x3_256_pipe16; RSTB tail and conv_after_body, reference
    model/swinir.py:467,483-484,742) against F.conv2d in fp32: one tile, several tiles per workgroup's walk across map borders, two stacked
    maps, the residual aliasing the output (as engine.swin_multi calls it), and the fall-back to the slab kernel where 6 x 16 tiles do not
    cover the map."""
    from speinet_amd.ops import BMap
    ops = Ctx(mode, device=DEV)
    slab = ops.replace(conv3_pipe=False)
    wt, b = rnd(31, 256, 256, 3, 3, scale=0.03), rnd(32, 256, scale=0.1)
    pw = pack.PackedW(pack.conv_w(wt), DEV)
    for (batch, h, w) in ((1, 6, 16), (1, 12, 48), (3, 18, 32), (2, 180, 320), (1, 10, 16)):
        x = rnd(33 + h, batch, 256, h, w)
        r = rnd(34 + w, batch, 256, h, w)
        ref = F.conv2d(x, wt, b, padding=1) + r
        xin = x.permute(0, 2, 3, 1).reshape(batch * h * w, 256).contiguous().to(DEV)
        rin = r.permute(0, 2, 3, 1).reshape(batch * h * w, 256).contiguous().to(DEV)
        rb = BMap(rin.clone(), batch, h, w, 256)
        out = ops.igemm_batched(BMap(xin, batch, h, w, 256), pw, b.to(DEV), 256, 3, residual=rb, out=rb)       # in place on the residual
        got = out.t.view(batch, h, w, 256).permute(0, 3, 1, 2).cpu()
        e = relerr(got, ref)
        assert torch.isfinite(got).all() and e < TOL[mode], f"{mode} {batch}x{h}x{w}: rel err {e:.2e}"
        old = slab.igemm_batched(BMap(xin, batch, h, w, 256), pw, b.to(DEV), 256, 3, residual=BMap(rin, batch, h, w, 256))
        assert relerr(out.t, old.t) < TOL[mode]
        # one map alone through igemm (the x-side call of a frame), no residual, fresh output
        one = ops.igemm(FMap(xin[:h * w], h, w, 256), pw, b.to(DEV), 256, ksize=3)
        assert relerr(one.nchw().cpu(), F.conv2d(x[:1], wt, b, padding=1)) < TOL[mode]
        if h % 6 == 0 and batch > 1:                  # a map's result does not depend on its place in the batch
            last = ops.igemm(FMap(xin[-h * w:].contiguous(), h, w, 256), pw, b.to(DEV), 256, ksize=3, residual=FMap(rin[-h * w:].contiguous(), h, w, 256))
            assert torch.equal(last.t, out.t[-h * w:])


@pytest.mark.parametrize("name", ["g07_search", "g07_search_tie"])
def test_search_bf16x3_argmax_exact(golden_dir, name):
    """With split-bf16 scores the arg-max of the golden cases (incl. the exact-tie one) stays bit exact."""
    ops = Ctx("bf16x3", "bf16x3", device=DEV)
    d = g(golden_dir, name)
    s, t3, t2, t1, arg = engine.search_transfer(ops, fm(d["lr3"]), fm(d["rf1"]), fm(d["rf2"]), fm(d["rf3"]), return_arg=True)
    assert torch.equal(arg.cpu().long(), d["arg"][0])
    assert relerr(s.view(1, 1, 10, 15), d["s"]) < 2e-5
    assert relerr(t1.nchw(), d["t1"]) < 1e-6


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_search_single_flip_rate(mode):
    """Single 16-bit scores: the winner may flip between near-tied candidates; measure it on a 20x30 map."""
    ops = Ctx(mode, "single", device=DEV)
    lr3, rf3 = rnd(32, 1, 128, 20, 30), rnd(33, 1, 128, 20, 30)
    rf2, rf1 = rnd(34, 1, 64, 40, 60), rnd(35, 1, 32, 80, 120)
    s0, _, _, _, arg0 = O.search_transfer(lr3, rf3, rf1, rf2, rf3, return_arg=True)
    s, t3, t2, t1, arg = engine.search_transfer(ops, fm(lr3), fm(rf1), fm(rf2), fm(rf3), return_arg=True)
    flips = (arg.cpu().long() != arg0[0]).float().mean().item()
    serr = (s.cpu() - s0.reshape(-1)).abs().max().item()
    print(f"{mode} correlation: flip rate {flips:.3%}, max |S err| {serr:.2e}")
    assert serr < (5e-3 if mode == "bf16" else 7e-4)          # the weight map S itself stays accurate
    assert flips < (0.25 if mode == "bf16" else 0.05)         # random (structure-free) features are the worst case for near-ties


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["g07_search", "g07_search_tie"])
def test_search_top2_argmax_exact(golden_dir, name, mode):
    """16-bit pass keeping two candidates + exact fp64 re-score ("top2"): the reference's arg-max bit for bit on the golden
    cases incl. the crafted exact-tie one (many bit-identical reference patches: the lowest index must win), and S to fp32
    round-off — the winner no longer depends on 16-bit rounding."""
    ops = Ctx(mode, "top2", device=DEV)
    d = g(golden_dir, name)
    s, t3, t2, t1, arg = engine.search_transfer(ops, fm(d["lr3"]), fm(d["rf1"]), fm(d["rf2"]), fm(d["rf3"]), return_arg=True)
    assert torch.equal(arg.cpu().long(), d["arg"][0])
    assert relerr(s.view(1, 1, 10, 15), d["s"]) < 2e-6
    assert relerr(t1.nchw(), d["t1"]) < 1e-6


def test_search_top2_ragged_vs_oracle():
    """top-2 + re-score on a ragged map (partial query tiles, partial reference blocks, out-of-map rows in the edge blocks)
    with a reference map of another size than the query map: arg-max equal to the oracle's except on fp32 near-ties."""
    lr3, rf3 = rnd(61, 1, 128, 37, 45), rnd(62, 1, 128, 29, 51)
    rf2, rf1 = rnd(63, 1, 64, 58, 102), rnd(64, 1, 32, 116, 204)
    lu = F.normalize(F.unfold(lr3, (3, 3), padding=1), dim=1)
    ru = F.normalize(F.unfold(rf3, (3, 3), padding=1).permute(0, 2, 1), dim=2)
    r = torch.bmm(ru.double(), lu.double())[0]                       # [Nr, Nl]
    top = torch.topk(r, 2, dim=0)
    for mode in ("bf16", "f16"):
        ops = Ctx(mode, "top2", device=DEV)
        inv_l, inv_r = ops.patch_invnorm(fm(lr3)), ops.patch_invnorm(fm(rf3))
        s, arg = ops.corr_argmax(fm(lr3), fm(rf3), inv_l, inv_r)
        diff = arg.cpu().long() != top.indices[0]
        margin = (top.values[0] - top.values[1])[diff]
        assert diff.sum().item() <= 2 and (margin < 1e-6).all(), (mode, diff.sum().item(), margin)
        assert (s.cpu().double() - top.values[0]).abs().max().item() < 1e-6


@pytest.fixture(scope="module")
def net(synth_sd):
    n = SPEINet(args=default_args())
    n.load_state_dict(synth_sd, strict=True)
    return n.to(DEV).eval()


@pytest.mark.parametrize("name,b,h,w", [("g10_fwd_40x60_mixed", 2, 40, 60), ("g10_fwd_100x100", 1, 100, 100),
                                        ("g10_fwd_200x200", 1, 200, 200), ("g10_fwd_200x200_noref", 1, 200, 200)])
def test_forward_bf16x3_golden(golden_dir, net, name, b, h, w):
    d = g(golden_dir, name)
    zr = tuple(int(i) for i in d["zero_ref"]) if "zero_ref" in d else ()
    x = synth_frames(b, h, w, seed=int(d["seed"]), zero_ref=zr)
    net.precision, net.corr_precision = "bf16x3", "bf16x3"
    with torch.no_grad():
        out = net(x.to(DEV)).cpu()
    net.precision = "f32"
    err = (out - d["out"]).abs().max().item()
    assert err < 1e-3, f"max abs err {err:.3e}"
    for i in range(b):
        tgt = O.to_uint8(x[i:i + 1, 1])
        dp = abs(O.psnr_uint8(O.to_uint8(out[i:i + 1]), tgt) - O.psnr_uint8(O.to_uint8(d["out"][i:i + 1]), tgt))
        assert dp <= 1e-3, f"PSNR delta {dp:.2e} dB"


@pytest.mark.parametrize("mode,corr,tol_err,tol_db", [("f16", "top2", 3e-3, 1e-3), ("bf16", "top2", 0.05, 1e-2)])
@pytest.mark.parametrize("name,b,h,w", [("g10_fwd_40x60_mixed", 2, 40, 60), ("g10_fwd_100x100", 1, 100, 100),
                                        ("g10_fwd_200x200", 1, 200, 200), ("g10_fwd_200x200_noref", 1, 200, 200)])
def test_forward_16bit_golden(golden_dir, net, name, b, h, w, mode, corr, tol_err, tol_db):
    """The single-product 16-bit modes against the reference's own outputs.  f16 / top2 is what bench.py times: it must hold
    the north-star bound (|dPSNR| <= 1e-3 dB); its largest pixel errors (3e-3 bound, 1.4e-3 measured) sit where a near-tied
    arg-max resolved differently, not in the arithmetic (rms 1.2e-4); bf16 holds its documented bound."""
    d = g(golden_dir, name)
    zr = tuple(int(i) for i in d["zero_ref"]) if "zero_ref" in d else ()
    x = synth_frames(b, h, w, seed=int(d["seed"]), zero_ref=zr)
    net.precision, net.corr_precision = mode, corr
    with torch.no_grad():
        out = net(x.to(DEV)).cpu()
    net.precision, net.corr_precision = "f32", "bf16x3"
    err = (out - d["out"]).abs().max().item()
    rms = (out - d["out"]).pow(2).mean().sqrt().item()
    dps = [abs(O.psnr_uint8(O.to_uint8(out[i:i + 1]), O.to_uint8(x[i:i + 1, 1])) -
               O.psnr_uint8(O.to_uint8(d["out"][i:i + 1]), O.to_uint8(x[i:i + 1, 1]))) for i in range(b)]
    print(f"{name} {mode}/{corr}: max abs err {err:.3e}, rms {rms:.3e}, |dPSNR vs target| {max(dps):.2e} dB")
    assert err < tol_err
    for i in range(b):
        assert dps[i] <= tol_db, (i, dps[i])           # no per-branch slack (round 3): the north-star bound on `_forwardb` too


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_mlp_fused_vs_oracle(synth_sd, mode):
    """Fused LN -> fc1 -> GELU -> fc2 -> +x kernel against the fp32 formula (tolerance of the mode, relative to the branch)."""
    ops = Ctx(mode, device=DEV)
    p = "swin.layers.1.residual_group.blocks.2."
    bk = pack.swin_block(synth_sd, p, 8, 5)
    w1, w2 = pack.PackedW(bk["w1"].t, DEV), pack.PackedW(bk["w2"].t, DEV)
    for m in (1, 64, 127, 1000, 2500, 57600, 115200):   # one token, half a tile, a ragged tile, ragged tail, many tiles, the 720p token count, two calls' worth
        x = rnd(40 + m, m, 256, scale=1.5) + 0.3
        ref = x + F.linear(F.gelu(F.linear(F.layer_norm(x, (256,), synth_sd[p + "norm2.weight"], synth_sd[p + "norm2.bias"], 1e-5),
                                           synth_sd[p + "mlp.fc1.weight"], synth_sd[p + "mlp.fc1.bias"])),
                           synth_sd[p + "mlp.fc2.weight"], synth_sd[p + "mlp.fc2.bias"])
        xd = x.to(DEV)
        out = ops.mlp_fused(xd, w1, bk["b1"].to(DEV), w2, bk["b2"].to(DEV), out=torch.empty_like(xd))
        e = ((out.cpu() - ref).abs().max() / (ref - x).abs().max()).item()      # relative to the MLP branch itself
        assert e < TOL[mode], f"M={m}: rel err {e:.2e}"
        inplace = ops.mlp_fused(xd, w1, bk["b1"].to(DEV), w2, bk["b2"].to(DEV), out=xd)
        assert torch.equal(inplace, out)


@pytest.mark.parametrize("h,w,shift", [(5, 5, 0), (5, 5, 2), (10, 15, 0), (10, 15, 2), (15, 25, 2), (20, 35, 0), (20, 35, 2),
                                       (180, 320, 2)])       # last: the 720p token map (2304 windows), oracle on the CPU
@pytest.mark.parametrize("win4", [True, False])
@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_attn_fused_vs_oracle(synth_sd, h, w, shift, mode, win4):
    """Fused LN -> q/kv -> shifted-window attention -> proj -> +x kernel against the oracle's attention branch
    (model/swinir.py:238-278); window counts that are not a multiple of a workgroup's windows leave its last slots empty.  win4: the
    four-window kernel of round 4 (spei_attn_win4_16, the default; also run on TWO stacked maps, as the engine calls it for the two Swin
    calls of a frame: each map must come out as it does alone) / round 2's two-window kernel."""
    ops = Ctx(mode, device=DEV, attn_win4=win4)
    p = "swin.layers.2.residual_group.blocks.1."
    bk = pack._to_device(pack.swin_block(synth_sd, p, 8, 5), DEV)
    m = h * w
    x = rnd(300 + m + shift, 1, m, 256, scale=1.3) + 0.2
    y = rnd(400 + m + shift, 1, m, 256, scale=0.9) - 0.1
    ln = lambda t: F.layer_norm(t, (256,), synth_sd[p + "norm1.weight"], synth_sd[p + "norm1.bias"], 1e-5).view(1, h, w, 256)
    xn, yn = ln(x), ln(y)
    if shift:
        xn, yn = (torch.roll(t, shifts=(-shift, -shift), dims=(1, 2)) for t in (xn, yn))
    xw, yw = (O.window_partition(t, 5).view(-1, 25, 256) for t in (xn, yn))
    mask = O.shift_mask(h, w, 5, shift) if shift else None
    branch = O.window_reverse(O.window_attention(xw, yw, synth_sd, p + "attn.", 8, 5, mask).view(-1, 5, 5, 256), 5, h, w)
    if shift:
        branch = torch.roll(branch, shifts=(shift, shift), dims=(1, 2))
    branch = branch.reshape(m, 256)
    xd = x[0].to(DEV).contiguous()
    yhat = ops.layernorm(y[0].to(DEV).contiguous(), out_dtype=LPD[mode])
    out = ops.attn_fused(xd, yhat, bk, h, w, shift, out=torch.empty_like(xd))
    e = ((out.cpu() - x[0] - branch).abs().max() / branch.abs().max()).item()
    assert torch.isfinite(out).all() and e < TOL[mode], f"{h}x{w} shift {shift}: rel err {e:.2e}"
    if win4:
        # two maps in one launch: map 0 = this case, map 1 = other tokens; map 0's rows must be bit-identical to the single-map launch
        x2 = torch.cat((xd, xd.flip(0) * 0.7 + 0.1))
        y2 = torch.cat((yhat, yhat.flip(0)))
        both = ops.attn_fused(x2, y2, bk, h, w, shift, out=torch.empty_like(x2))
        assert torch.equal(both[:m], out) and torch.isfinite(both).all()
        alone = ops.attn_fused(x2[m:].contiguous(), y2[m:].contiguous(), bk, h, w, shift, out=torch.empty_like(xd))
        assert torch.equal(both[m:], alone)
    inplace = ops.attn_fused(xd, yhat, bk, h, w, shift, out=xd)
    assert torch.equal(inplace, out)


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_streams_bit_identical(net, mode, graph):
    """Issuing the neighbour-frame / reference branches on 2 or 3 HIP streams (eagerly or captured into the frame's
    hipGraph) must not change a single bit: same kernels, same operands, only the schedule differs."""
    x = synth_frames(2, 100, 120, seed=77, zero_ref=(1,)).to(DEV)       # sample 0 SearchTransfer, sample 1 SelfTransfer
    net.precision, net.corr_precision = mode, "bf16x3"
    outs = []
    try:
        for streams in (1, 2, 3):
            net.streams, net.use_graph = streams, graph
            with torch.no_grad():
                outs.append(net(x).clone())
                outs.append(net(x).clone())                                 # second call: graph replay / warm allocator
    finally:
        net.streams, net.use_graph, net.precision = 1, False, "f32"
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all()
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


def test_graph_trim_recapture_bit_identical(net):
    """More frame shapes than the model keeps graphs for (`GRAPH_LIMIT`, lowered to 2 on this instance): the graphs are dropped and
    captured again as the shapes come round, and every call — capture, replay, replay after a trim — gives the bits of the eager call."""
    shapes = [(20, 20), (20, 40), (40, 40)]
    xs = [synth_frames(1, h, w, seed=90 + i).to(DEV) for i, (h, w) in enumerate(shapes)]
    net.precision, net.corr_precision, net.streams, net.GRAPH_LIMIT = "f16", "top2", 2, 2
    try:
        with torch.no_grad():
            refs = [net(x).clone() for x in xs]
            net.use_graph = True
            for i in (0, 0, 1, 1, 2, 2, 0):                 # the third shape's capture trims; then the first shape is captured again
                out = net(xs[i])
                assert len(net._graphs) <= 2
                assert torch.equal(out, refs[i]), shapes[i]
    finally:
        net.streams, net.use_graph, net.precision, net.corr_precision = 1, False, "f32", "bf16x3"
        del net.GRAPH_LIMIT
    torch.cuda.synchronize()
    assert all(torch.isfinite(r).all() for r in refs)


@pytest.mark.parametrize("h,w,b,zero_ref", [(480, 640, 2, (1,)), (720, 1280, 1, ())])
def test_forward_large_sizes_modes_agree(net, h, w, b, zero_ref):
    """480x640 (the BSD frame size, BASELINE.json configs[3]; 768 windows, lv3 map 120x160 -> partial tiles in every tiled
    kernel, both routing branches) and 720x1280 (the bench configuration): no oracle run at these sizes, so the three
    arithmetic modes are checked against each other.  bf16x3 and f16 / top2 (the bench configuration) must stay within
    the f32-grade bound of the f32 path, bf16 within its documented bound."""
    x = synth_frames(b, h, w, seed=4242, zero_ref=zero_ref).to(DEV)
    outs = {}
    try:
        for mode, corr in (("f32", "bf16x3"), ("bf16x3", "bf16x3"), ("f16", "top2"), ("bf16", "single" if h == 720 else "bf16x3")):
            net.precision, net.corr_precision = mode, corr
            with torch.no_grad():
                outs[mode] = net(x).cpu()
    finally:
        net.precision, net.corr_precision = "f32", "bf16x3"
    assert all(torch.isfinite(o).all() for o in outs.values())
    e3 = (outs["bf16x3"] - outs["f32"]).abs().max().item()
    e1 = (outs["bf16"] - outs["f32"]).abs().max().item()
    eh = (outs["f16"] - outs["f32"]).abs().max().item()
    print(f"{h}x{w}: max |bf16x3 - f32| {e3:.2e}, max |f16 - f32| {eh:.2e}, max |bf16 - f32| {e1:.2e}")
    assert e3 < (1e-3 if h < 720 else 2e-3) and e1 < 0.05      # 720p: the max is over 2.8 M values (9.3e-4 measured)
    assert eh < 3e-3


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_conv5_out_slab(mode):
    """Last conv (32 -> 3 channels, NCHW planes out) on the slab kernel in the 16-bit modes; odd sizes -> partial tiles."""
    ops = Ctx(mode, device=DEV)
    f = rnd(21, 1, 32, 27, 45)
    wo, bo = rnd(22, 3, 32, 5, 5, scale=0.05), rnd(23, 3, scale=0.1)
    w = pack.conv_w(wo)
    w32 = pack.PackedW(torch.cat((w, torch.zeros(25, 29, 32)), 1), DEV)
    b32 = torch.cat((bo, torch.zeros(29))).to(DEV)
    o = torch.full((3, 27, 45), float("nan"), device=DEV)
    ops.conv5_out(fm(f), w.to(DEV), bo.to(DEV), o, w32, b32)
    assert relerr(o, F.conv2d(f, wo, bo, padding=2)[0]) < TOL[mode]


def test_up_conv1x1_relu_commuted():
    """relu(conv1x1(bicubic_up(x))): the "bf16" mode runs the conv before the upsampling (ReLU fused into the upsampler);
    same function up to the bf16 products, checked against the reference's order in fp32."""
    x = rnd(31, 1, 128, 9, 13)
    wt, b = rnd(32, 64, 128, 1, 1, scale=0.08), rnd(33, 64, scale=0.2)
    ref = F.relu(F.conv2d(F.interpolate(x, scale_factor=2, mode="bicubic"), wt, b))
    for mode in ("bf16x3", "bf16", "f16"):
        ops = Ctx(mode, device=DEV)
        out = ops.up_conv1x1_relu(fm(x), pack.conv_w(wt).to(DEV), b.to(DEV), 64)
        assert relerr(out.nchw(), ref) < TOL[mode], mode


@pytest.mark.parametrize("mode,corr", [("f32", "bf16x3"), ("bf16", "bf16x3"), ("bf16", "single"), ("bf16", "top2"), ("f16", "single"),
                                       ("f16", "top2")])
def test_full_size_search_properties(mode, corr):
    """Size-independent properties at the 720p map size (180 x 320 positions, 128 channels; no oracle run at this size):
    a map correlated with itself finds every position at itself with a normalised score of 1, a shifted copy is found at the
    shift, and gathering with the identity indices reproduces the map (fold(unfold(x)) / 9: exactly x away from the border)."""
    ops = Ctx(mode, corr, device=DEV)
    h, w = 180, 320
    gen = torch.Generator().manual_seed(5)
    f = FMap(torch.randn(h * w, 128, generator=gen).to(DEV), h, w, 128)
    inv = ops.patch_invnorm(f)
    s, arg = ops.corr_argmax(f, f, inv, inv)
    ident = torch.arange(h * w, device=DEV, dtype=torch.int32)
    assert torch.equal(arg, ident)
    assert (s - 1).abs().max().item() < (1e-5 if mode == "f32" or corr == "top2" else 1e-4 if corr == "bf16x3" else 2e-2 if mode == "bf16" else 3e-3)
    # query = reference shifted by (3, 5) pixels: interior positions (whose whole 3x3 patch moved along) point back by the shift
    g = FMap(torch.roll(f.t.view(h, w, 128), shifts=(3, 5), dims=(0, 1)).reshape(h * w, 128).contiguous(), h, w, 128)
    _, arg2 = ops.corr_argmax(g, f, ops.patch_invnorm(g), inv)
    yy, xx = torch.meshgrid(torch.arange(5, h - 1, device=DEV), torch.arange(7, w - 1, device=DEV), indexing="ij")
    assert torch.equal(arg2.view(h, w)[5:h - 1, 7:w - 1].long(), (yy - 3) * w + (xx - 5))
    for scale, c in ((1, 128), (2, 64), (4, 32)):
        ref = FMap(torch.randn(h * scale * w * scale, c, generator=gen).to(DEV), h * scale, w * scale, c)
        t = ops.gather_fold(ref, ident, h, w, h, w, scale)
        a, b = t.t.view(h * scale, w * scale, c)[scale:-scale, scale:-scale], ref.t.view(h * scale, w * scale, c)[scale:-scale, scale:-scale]
        assert (a - b).abs().max().item() < 1e-5


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
def test_full_size_conv_identity(mode):
    """Identity kernels at the 720p layer sizes (no oracle run at these sizes): a centre-tap identity convolution must return
    its input exactly (bf16-rounded in "bf16" mode: x * 1 + zeros is exact) at every pixel incl. the map border and every
    partial tile; stride 2 returns the even pixels; the transposed conv writes the input to the even output pixels."""
    # (16-bit modes: x * 1 + zeros is exact, so the output is the input rounded to the mode's format)
    ops = Ctx(mode, device=DEV)
    gen = torch.Generator().manual_seed(9)
    rnd_in = lambda x: x.to(LPD[mode]).float() if mode in LPD else x
    for c, h, w, ks in ((32, 720, 1280, 5), (64, 360, 640, 5), (128, 180, 320, 5), (256, 180, 320, 3)):
        x = torch.randn(h * w, c, generator=gen).to(DEV)
        wt = torch.zeros(ks * ks, c, c)
        wt[ks * ks // 2] = torch.eye(c)
        out = ops.igemm(FMap(x, h, w, c), pack.PackedW(wt, DEV), torch.zeros(c, device=DEV), c, ksize=ks)
        assert torch.equal(out.t, rnd_in(x)), (c, h, w, ks)
    for c, n, h, w in ((32, 64, 720, 1280), (64, 128, 360, 640)):                    # stride-2 heads: out[y][x] = in[2y][2x], channels 0..c-1
        x = torch.randn(h * w, c, generator=gen).to(DEV)
        wt = torch.zeros(25, n, c)
        wt[12, :c] = torch.eye(c)
        out = ops.igemm(FMap(x, h, w, c), pack.PackedW(wt, DEV), torch.zeros(n, device=DEV), n, ksize=5, stride=2)
        assert torch.equal(out.t.view(h // 2, w // 2, n)[:, :, :c], rnd_in(x).view(h, w, c)[::2, ::2])
        assert out.t.view(h // 2, w // 2, n)[:, :, c:].abs().max().item() == 0
    for c, n, h, w in ((128, 64, 180, 320), (64, 32, 360, 640)):                     # decoder tails
        x = torch.randn(h * w, c, generator=gen).to(DEV)
        wt = torch.zeros(9, n, c)
        wt[4] = torch.eye(c)[:n]
        out = ops.igemm(FMap(x, h, w, c), pack.PackedW(wt, DEV), torch.zeros(n, device=DEV), n, ksize=3, stride=2, mode=ops.CONV_T)
        o = out.t.view(2 * h, 2 * w, n)
        assert torch.equal(o[::2, ::2], rnd_in(x).view(h, w, c)[:, :, :n])
        assert o[1::2].abs().max().item() == 0 and o[:, 1::2].abs().max().item() == 0


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_full_size_swin_properties(synth_sd, mode):
    """Size-independent properties of the fused Swin kernels at the 720p token count (180 x 320 = 57600 tokens, 2304
    windows): (i) MLP with fc2 = 0 returns x exactly; (ii) attention with proj = 0 returns x exactly; (iii) with V = a
    constant vector c (zero V weights, bias c) and proj = identity, softmax rows summing to 1 give x + c for every token
    of every (shifted, masked) window, up to the 16-bit rounding of the probabilities."""
    ops = Ctx(mode, device=DEV)
    h, w = 180, 320
    m = h * w
    gen = torch.Generator().manual_seed(13)
    x = (torch.randn(m, 256, generator=gen) * 1.2 + 0.3).to(DEV)
    yhat = ops.layernorm(torch.randn(m, 256, generator=gen).to(DEV), out_dtype=LPD[mode])
    p = "swin.layers.3.residual_group.blocks.1."
    raw = pack.swin_block(synth_sd, p, 8, 5)
    bk = pack._to_device(raw, DEV)
    # (i)
    out = ops.mlp_fused(x, bk["w1"], bk["b1"], pack.PackedW(torch.zeros(1, 256, 512), DEV), torch.zeros(256, device=DEV), out=torch.empty_like(x))
    assert torch.equal(out, x)
    for shift in (0, 2):
        # (ii)
        b0 = dict(bk, wproj=pack.PackedW(torch.zeros(1, 256, 256), DEV), bproj=torch.zeros(256, device=DEV))
        assert torch.equal(ops.attn_fused(x, yhat, b0, h, w, shift, out=torch.empty_like(x)), x)
        # (iii)
        c = torch.linspace(-1.5, 2.0, 256)
        wkv = raw["wkv"].t.clone()
        wkv[0, 256:] = 0
        bkv = raw["bkv"].clone()
        bkv[256:] = c
        b1 = dict(bk, wkv=pack.PackedW(wkv, DEV), bkv=bkv.to(DEV), wproj=pack.PackedW(torch.eye(256).unsqueeze(0), DEV),
                  bproj=torch.zeros(256, device=DEV))
        out = ops.attn_fused(x, yhat, b1, h, w, shift, out=torch.empty_like(x))
        err = (out - x - c.to(DEV)).abs().max().item()
        assert err < (2e-2 if mode == "bf16" else 3e-3), (shift, err)


@pytest.mark.parametrize("mode", ["f16", "bf16"])
@pytest.mark.parametrize("b,h,w,zero_ref", [(2, 40, 60, (1,)), (1, 100, 100, ()), (1, 140, 220, (0,)), (1, 360, 640, ())])
def test_batched_encoder_bit_identical(net, mode, b, h, w, zero_ref):
    """`batch_enc` (default): the frame's 7 / 6 encoder passes as ONE launch per layer (gridDim.y = pass) give the bits of one launch
    per pass and layer — same tiles, same arithmetic, same partial-sum order per map — at ragged sizes (tiles cut by the border,
    tile grids that differ per level), both branches, eager and as a hipGraph."""
    x = synth_frames(b, h, w, seed=77, zero_ref=zero_ref).to(DEV)
    net.precision, net.corr_precision = mode, "top2"
    try:
        outs = {}
        for be in (True, False):
            net.knobs = {"batch_enc": be}
            with torch.no_grad():
                outs[be] = net(x).clone()
        assert torch.equal(outs[True], outs[False]), (outs[True] - outs[False]).abs().max().item()
        net.knobs, net.use_graph = {"batch_enc": True}, True
        with torch.no_grad():
            net(x)
            assert torch.equal(net(x), outs[False])
    finally:
        net.knobs, net.use_graph = {}, False
        net.precision, net.corr_precision = "f32", "bf16x3"


@pytest.mark.parametrize("graph", [False, True])
def test_batch_bit_identical_to_per_sample(net, graph):
    """B > 1 (the reference processes [B, ...] natively, model/speinet.py:150-168): the encoder passes of all samples are batched per
    layer (engine.forward_batch_steps: 13 maps here, two launch groups at the 16-map budget for the larger batch); every sample's frame
    has the bits of the same sample run alone — mixed routing, eager and hipGraph."""
    net.precision, net.corr_precision, net.use_graph = "f16", "top2", graph
    try:
        for b, h, w, zr in ((2, 100, 140, (1,)), (4, 60, 80, (0, 3))):
            x = synth_frames(b, h, w, seed=50 + b, zero_ref=zr).to(DEV)
            with torch.no_grad():
                whole = net(x).clone()
                if graph:
                    whole = net(x).clone()                 # the replay, not the capture run
                for i in range(b):
                    assert torch.equal(net(x[i:i + 1])[0], whole[i]), (b, i)
    finally:
        net.precision, net.corr_precision, net.use_graph = "f32", "bf16x3", False


def _golden_case(golden_dir, name):
    from speinet_amd.synth import synth_frames_edges
    d = np.load(os.path.join(golden_dir, name + ".npz"))
    b, h, w = d["sub"].shape[0], d["sub"].shape[2] * 8, d["sub"].shape[3] * 8
    zr = tuple(int(i) for i in d["zero_ref"])
    if str(d["kind"]) == "edges":
        x, gt = synth_frames_edges(b, h, w, seed=int(d["seed"]), zero_ref=zr)
    else:
        x = synth_frames(b, h, w, seed=int(d["seed"]), zero_ref=zr)
        gt = x[:, 1]
    return d, x, gt


@pytest.mark.parametrize("name", ["g14_fwd_720p", "g15_fwd_720p_noref", "g16_fwd_480x640_mixed", "g17_fwd_720p_edges"])
def test_forward_full_size_reference_golden(golden_dir, net, name):
    """The full sizes against the REFERENCE's own outputs (tests/golden/make_golden_720p.py: every 8th pixel of its frames,
    per-channel statistics, its PSNR, and what its SearchTransfer decided: arg-max, S, top-2 margin): the bench configuration
    (720p, `_forwardbs`), the same through `_forwardb`, a mixed-routing batch at the BSD size and an edge-dominated 720p window.
    Every mode that claims PSNR parity — exact fp32, bf16x3 and f16 / top2, the configuration bench.py times — must hold the
    north-star bound |dPSNR| <= 1e-3 dB and 1e-3 absolute on the grid; bf16 its documented bound.  The PSNR bound is asserted twice:
    against the stand-in target the fixture was made with (the reference scores 7-12 dB there) and against a synthesised ground
    truth where the reference scores ~32 dB (~28 dB at the BSD size) — the operating point of its published logs.
    Arg-max: positions that differ from the reference's own arg-max are counted; for the f32-grade modes every one of them
    must be a reference near-tie (top-2 margin < 1e-5 in the reference's own fp32 scores: another summation order decides)."""
    d, x, gt = _golden_case(golden_dir, name)
    tgt = np.load(os.path.join(golden_dir, name + "_target.npz"))        # synthesised ~32 / ~28 dB ground truth + the reference's PSNR
    b = x.shape[0]
    sub, mean, std = (torch.from_numpy(d[k]) for k in ("sub", "mean", "std"))
    ref_arg = torch.from_numpy(d["arg"]).long() if "arg" in d.files else None
    xd = x.to(DEV)
    try:
        for mode, corr, tol, tol_db in (("f32", "bf16x3", 1e-3, 1e-3), ("bf16x3", "bf16x3", 1e-3, 1e-3), ("f16", "top2", 3e-3, 1e-3),
                                        ("bf16", "top2", 0.05, 1e-2)):
            net.precision, net.corr_precision = mode, corr
            outs, flips, hard, serr, si = [], 0, 0, 0.0, 0
            with torch.no_grad():
                for i in range(b):
                    cap = {}
                    outs.append(net(xd[i:i + 1], capture=cap).cpu())
                    if "arg" in cap and ref_arg is not None:
                        diff = cap["arg"].cpu().long() != ref_arg[si]
                        flips += int(diff.sum())
                        hard += int((diff & (torch.from_numpy(d["margin"][si]) >= 1e-5)).sum())
                        serr = max(serr, (cap["s"].cpu() - torch.from_numpy(d["s"][si])).abs().max().item())
                        si += 1
                    elif "s_self" in cap:
                        serr = max(serr, (cap["s_self"].cpu() - torch.from_numpy(d["s_self"][0])).abs().max().item())
            out = torch.cat(outs)
            err = (out[:, :, ::8, ::8] - sub).abs().max().item()
            dm = (out.mean(dim=(2, 3)) - mean).abs().max().item()
            ds = (out.std(dim=(2, 3)) - std).abs().max().item()
            dps = [abs(O.psnr_uint8(O.to_uint8(out[i:i + 1]), O.to_uint8(gt[i:i + 1])) - float(d["psnr"][i])) for i in range(b)]
            print(f"{name} vs reference, {mode}/{corr}: max |err| on the 8x8 grid {err:.2e}, |d mean| {dm:.1e}, |d std| {ds:.1e}, "
                  f"|dPSNR| {max(dps):.1e} dB, arg-max flips {flips} (not reference near-ties: {hard}), max |dS| {serr:.1e}")
            # a flip at a reference near-tie (other fp32 summation order upstream of the scores) swaps one 3x3x128 patch for an
            # equally-scored one: pixels under it move by up to ~1e-3 — the grid bound is then the 16-bit modes' 3e-3, the PSNR
            # bound stays (one patch in 57600)
            grid_tol = tol if flips == 0 else max(tol, 3e-3)
            assert err < grid_tol and dm < tol / 10 and ds < tol / 10, mode
            zr = [int(i) for i in d["zero_ref"]]
            for i in range(b):
                assert dps[i] <= tol_db, (mode, i, dps[i])
            # the same bound at a REALISTIC operating point: against the synthesised ground truth of <case>_target.npz the reference
            # scores ~32 dB (G16, the BSD frame size: ~28 dB) — the range of its own GoPro / BSD logs — where a given output error
            # weighs ~10x more in dB than against the 7-12 dB stand-in targets above (tests/golden/make_golden_720p.py)
            dpt = [abs(O.psnr_uint8(O.to_uint8(out[i:i + 1]), torch.from_numpy(tgt["target"][i]).permute(1, 2, 0)) - float(tgt["psnr"][i]))
                   for i in range(b)]
            print(f"{name} vs reference at its {float(tgt['psnr'].mean()):.1f} dB operating point, {mode}/{corr}: |dPSNR| {max(dpt):.1e} dB")
            # bf16 ("configs[1] to the letter", 8-bit significands) is not a PSNR-parity mode: its 1e-2 dB bound was stated against the
            # stand-in targets; at the realistic operating point its error weighs up to 2.1e-2 dB (G15) — asserted at 3e-2, documented
            for i in range(b):
                assert dpt[i] <= (tol_db if mode != "bf16" else 3e-2), (mode, "realistic target", i, dpt[i])
            if mode in ("f32", "bf16x3"):
                assert hard == 0 and flips <= 40 and serr < 1e-5, (mode, flips, hard, serr)
    finally:
        net.precision, net.corr_precision = "f32", "bf16x3"


def test_two_models_two_threads_bit_identical(synth_sd):
    """SURVEY.md §8b threading row (the reference's nn.DataParallel calls forward from one Python thread per replica,
    model/__init__.py:19-20): two SPEINet instances with DIFFERENT arithmetic modes driven from two threads at once give
    the bits they give when run one after the other — the mode lives in the per-call context, not in the process."""
    import threading
    nets = []
    for mode, corr in (("f32", "bf16x3"), ("f16", "top2")):
        n = SPEINet(args=default_args())
        n.load_state_dict(synth_sd, strict=True)
        n = n.to(DEV).eval()
        n.precision, n.corr_precision = mode, corr
        nets.append(n)
    x = synth_frames(2, 60, 80, seed=91, zero_ref=(1,)).to(DEV)
    with torch.no_grad():
        serial = [n(x).clone() for n in nets]
    torch.cuda.synchronize()
    results, errors = [None, None], []

    def work(i):
        try:
            with torch.no_grad(), torch.cuda.stream(torch.cuda.Stream(device=DEV)):
                outs = [nets[i](x).clone() for _ in range(6)]
            torch.cuda.synchronize()
            results[i] = outs
        except Exception as e:           # noqa: BLE001
            errors.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for i in range(2):
        for o in results[i]:
            assert torch.equal(o, serial[i]), f"model {i} differs when run concurrently"
    assert not torch.equal(serial[0], serial[1])          # the two modes really are different arithmetic
