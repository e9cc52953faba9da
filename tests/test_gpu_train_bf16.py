"""`train_precision = "bf16"`: the training step with every GEMM in single bf16 products (speinet_amd/train.py).

The contract these tests pin, op by op: each GEMM operand rounded ONCE to bf16 (round to nearest even), exact products, fp32 sums.
So every forward / data-gradient / weight-gradient result is compared with float64 arithmetic on the same operands rounded to bf16
in torch (`t.float().bfloat16().double()`): only the fp32 summation order separates the two (bound 2e-5 x max|ref|).  Window attention
also rounds P and dS, which it computes in fp32: the reference rounds its float64 P / dS, and an entry can land one bf16 step away
(bound 1e-3 x max|ref|).  Every case also has
  * the bound of the inference bf16 mode against unrounded float64 (1.5e-2 x max|ref|), and
  * a negative control: the bf16 result differs from the "f32" result by more than 1e-5 x max|ref| (a path that quietly ran fp32
    would not).
Then the whole step (swint and the full model) against the f32 step, the G22 loss curve, reproducibility and the weight cache.
"""
import contextlib
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONTRACT, ATTN, INFER, CONTROL = 2e-5, 1e-3, 1.5e-2, 1e-5


def _bf(t: torch.Tensor) -> torch.Tensor:
    """The operand the kernels multiply: fp32 value rounded to bf16 (nearest even), as float64."""
    return t.float().bfloat16().double()


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.float().double()


@contextlib.contextmanager
def _prec(p: str):
    from speinet_amd import train as T
    tok = T._PREC.set(p)
    try:
        yield
    finally:
        T._PREC.reset(tok)


def _err(a, ref) -> float:
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return (a - ref).abs().max().item() / ref.abs().max().clamp_min(1e-30).item()


def _check(name, got, ref_rounded, ref_exact, got_f32, bound=CONTRACT):
    e, e64 = _err(got, ref_rounded), _err(got, ref_exact)
    ctl = (got.detach().double().cpu() - got_f32.detach().double().cpu()).abs().max().item() / ref_rounded.abs().max().item()
    assert e < bound, f"{name}: {e:.2e} from the bf16-operand float64 reference (bound {bound:.0e})"
    assert e64 < INFER, f"{name}: {e64:.2e} from unrounded float64"
    assert ctl > CONTROL, f"{name}: bf16 result within {ctl:.1e} of the f32 result: not bf16 arithmetic"
    return e


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _leaf(t):
    return t.to(DEV).float().requires_grad_(True)


@pytest.mark.parametrize("B,H,W,k,n,ks,stride,res", [
    (2, 12, 37, 32, 32, 5, 1, False),        # ragged width, batch
    (3, 10, 10, 256, 256, 3, 1, True),       # the Swin-body 3x3 with its residual
    (2, 14, 33, 128, 64, 1, 1, False),       # 1x1
    (2, 9, 21, 64, 128, 5, 2, False),        # stride 2, odd sizes (the adjoint's crop)
    (1, 20, 20, 32, 64, 5, 2, False),        # an encoder head
    (2, 12, 10, 64, 32, 3, 2, False),        # 3x3 stride 2
])
def test_conv2d_bf16_contract(B, H, W, k, n, ks, stride, res):
    from speinet_amd import train as T
    gen = torch.Generator().manual_seed(B * 1000 + H * 10 + ks + stride)
    x = _f32(torch.randn(B, k, H, W, generator=gen, dtype=torch.float64))
    w = _f32(torch.randn(n, k, ks, ks, generator=gen, dtype=torch.float64) / math.sqrt(k * ks * ks))
    b = _f32(torch.randn(n, generator=gen, dtype=torch.float64) * 0.1)
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    r = _f32(torch.randn(B, n, ho, wo, generator=gen, dtype=torch.float64)) if res else None
    g = _f32(torch.randn(B, n, ho, wo, generator=gen, dtype=torch.float64))
    refs = {}
    for name, rnd in (("rounded", _bf), ("exact", lambda t: t)):
        lx, lw = rnd(x).clone().requires_grad_(True), rnd(w).clone().requires_grad_(True)
        y = F.conv2d(lx, lw, b, stride=stride, padding=ks // 2) + (r if res else 0)
        (y * rnd(g)).sum().backward()
        refs[name] = (_rows(y.detach()), _rows(lx.grad), lw.grad, g.sum(dim=(0, 2, 3)))
    got = {}
    for prec in ("bf16", "f32"):
        dx, dw, db = _leaf(_rows(x)), _leaf(w), _leaf(b)
        with _prec(prec):
            y = T._Conv2d.apply(dx, dw, db, _rows(r).to(DEV).float() if res else None, B, H, W, ks, stride, False)
        y.backward(_rows(g).to(DEV).float())
        got[prec] = (y, dx.grad, dw.grad, db.grad)
    for i, what in enumerate(("forward", "data gradient", "weight gradient")):
        _check(what, got["bf16"][i], refs["rounded"][i], refs["exact"][i], got["f32"][i])
    assert _err(got["bf16"][3], refs["exact"][3]) < CONTRACT, "bias gradient: an fp32 column sum"


@pytest.mark.parametrize("B,H,W,k,n", [(2, 5, 5, 128, 64), (1, 10, 15, 64, 32), (3, 6, 7, 64, 32)])
def test_conv_transpose2d_bf16_contract(B, H, W, k, n):
    from speinet_amd import train as T
    gen = torch.Generator().manual_seed(B * 100 + H + W)
    x = _f32(torch.randn(B, k, H, W, generator=gen, dtype=torch.float64))
    w = _f32(torch.randn(k, n, 3, 3, generator=gen, dtype=torch.float64) / math.sqrt(k * 9 / 4))
    b = _f32(torch.randn(n, generator=gen, dtype=torch.float64) * 0.1)
    g = _f32(torch.randn(B, n, 2 * H, 2 * W, generator=gen, dtype=torch.float64))
    got = {}
    for prec in ("bf16", "f32"):
        dx, dw, db = _leaf(_rows(x)), _leaf(w), _leaf(b)
        with _prec(prec):
            y = T._ConvT2d.apply(dx, dw, db, B, H, W)
        y.backward(_rows(g).to(DEV).float())
        got[prec] = (y, dx.grad, dw.grad, db.grad)
    # the ReLU mask is an fp32 elementwise decision, not part of the GEMM contract: the references take the bf16 run's own mask
    mask = (got["bf16"][0].detach().cpu().double() > 0).double().view(B, 2 * H, 2 * W, n).permute(0, 3, 1, 2)
    gz = g * mask
    refs = {}
    for name, rnd in (("rounded", _bf), ("exact", lambda t: t)):
        lx, lw = rnd(x).clone().requires_grad_(True), rnd(w).clone().requires_grad_(True)
        z = F.conv_transpose2d(lx, lw, b, stride=2, padding=1, output_padding=1)
        (z * rnd(gz)).sum().backward()
        refs[name] = (_rows(F.relu(z.detach())), _rows(lx.grad), lw.grad, gz.sum(dim=(0, 2, 3)))
    for i, what in enumerate(("forward", "data gradient", "weight gradient")):
        _check(what, got["bf16"][i], refs["rounded"][i], refs["exact"][i], got["f32"][i])
    assert _err(got["bf16"][3], refs["exact"][3]) < CONTRACT, "bias gradient"


@pytest.mark.parametrize("m,k,n", [(200, 256, 512), (150, 512, 256), (77, 256, 256)])
def test_linear_bf16_contract_with_residual_and_rowscale(m, k, n):
    from speinet_amd import train as T
    gen = torch.Generator().manual_seed(m + k + n)
    x = _f32(torch.randn(m, k, generator=gen, dtype=torch.float64))
    w = _f32(torch.randn(n, k, generator=gen, dtype=torch.float64) * 0.05)
    b = _f32(torch.randn(n, generator=gen, dtype=torch.float64))
    res = _f32(torch.randn(m, n, generator=gen, dtype=torch.float64))
    rs32 = torch.tensor([0.0, 1.0 / 0.9], dtype=torch.float32)[torch.randint(0, 2, (m,), generator=gen)]
    g = _f32(torch.randn(m, n, generator=gen, dtype=torch.float64))
    gs = (g.float() * rs32[:, None]).double()             # spei_scale_rows: the DropPath factor on the branch gradient, fp32
    rs = rs32.double()
    refs = {}
    for name, rnd in (("rounded", _bf), ("exact", lambda t: t)):
        y = res + rs[:, None] * (rnd(x) @ rnd(w).t() + b)
        refs[name] = (y, rnd(gs) @ rnd(w), rnd(gs).t() @ rnd(x), gs.sum(0))
    got = {}
    for prec in ("bf16", "f32"):
        dl = [_leaf(t) for t in (x, w, b, res)]
        with _prec(prec):
            y = T._Linear.apply(dl[0], dl[1], dl[2], dl[3], rs32.to(DEV))
        y.backward(g.to(DEV).float())
        got[prec] = (y, dl[0].grad, dl[1].grad, dl[2].grad, dl[3].grad)
    for i, what in enumerate(("forward", "data gradient", "weight gradient")):
        _check(what, got["bf16"][i], refs["rounded"][i], refs["exact"][i], got["f32"][i])
    assert _err(got["bf16"][3], refs["exact"][3]) < CONTRACT, "bias gradient"
    assert torch.equal(got["bf16"][4].cpu().double(), g), "residual gradient passes through"


def _tie_slack(t: torch.Tensor, tol: torch.Tensor) -> torch.Tensor:
    """bf16 ulp of `t` where `t` lies within `tol` of a round-to-nearest tie (the kernel's fp32 value may round the other way), else 0."""
    f = t.float()
    lo = (f.view(torch.int32) & ~0xFFFF).view(torch.float32).double()                   # truncated to bf16
    ulp = (((f.abs().view(torch.int32) & ~0xFFFF) + 0x10000).view(torch.float32).double() - lo.abs())
    mid = lo + torch.sign(t) * ulp / 2
    return torch.where(((t - mid).abs() <= tol) & (t != 0), ulp, torch.zeros_like(ulp))


def _attn_ref(q, kv, rb, g, B, H, W, shift, rnd):
    """Window attention forward and backward (model/swinir.py:115-149 with the shifted-window partition / mask) in float64, with
    `rnd` applied to every GEMM operand: q, k, v, dO, P, dS.  Returns out, dq, dkv, drelbias and, per result, the slack that P / dS
    entries within fp32 round-off of a bf16 rounding tie allow (their ulp times the other operand's magnitude; zero elsewhere)."""
    ws, heads = 5, 8
    nwh, nww = H // ws, W // ws

    def part(t, c):
        t = t.view(B, H, W, c)
        if shift:
            t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))
        t = t.view(B, nwh, ws, nww, ws, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, c)
        return t.view(-1, 25, c // 32, 32).permute(0, 2, 1, 3)                         # [nb, heads, 25, 32]

    def unpart(t):
        t = t.permute(0, 2, 1, 3).reshape(B, nwh, nww, ws, ws, -1).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, -1)
        if shift:
            t = torch.roll(t, shifts=(shift, shift), dims=(1, 2))
        return t.reshape(B * H * W, -1)

    qh, kh, vh, gh = part(q, 256), part(kv[:, :256], 256), part(kv[:, 256:], 256), part(g, 256)
    s = rnd(qh) @ rnd(kh).transpose(-2, -1) + rb.unsqueeze(0)
    if shift:
        from speinet_amd.speinet import _shift_mask
        mask = _shift_mask(H, W, ws, shift).double().to(s.device)
        s = (s.view(B, -1, heads, 25, 25) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, 25, 25)
    p = s.softmax(-1)
    o = rnd(p) @ rnd(vh)
    dp = rnd(gh) @ rnd(vh).transpose(-2, -1)
    dv = rnd(p).transpose(-2, -1) @ rnd(gh)
    rq = (p * dp).sum(-1, keepdim=True)
    ds = p * (dp - rq)
    dq = rnd(ds) @ rnd(kh)
    dk = rnd(ds).transpose(-2, -1) @ rnd(qh)
    sp = _tie_slack(p, 1e-5 * p.abs())
    sd = _tie_slack(ds, 1e-5 * p * (dp.abs() + rq.abs()))
    a = lambda t: rnd(t).abs()
    slack = (unpart(sp @ a(vh)), unpart(sd @ a(kh)),
             torch.cat([unpart(sd.transpose(-2, -1) @ a(qh)), unpart(sp.transpose(-2, -1) @ a(gh))], dim=1), torch.zeros_like(rb))
    return (unpart(o), unpart(dq), torch.cat([unpart(dk), unpart(dv)], dim=1), ds.sum(0)), slack


@pytest.mark.parametrize("shift", [0, 2])
def test_window_attention_bf16_contract(shift):
    """A non-square map whose window count (3 x 7 = 21 per sample) is not a multiple of the workgroup tiling, two samples.  q at 0.35
    (logits of std ~2): the distance to UNROUNDED float64 grows with the logit spread (|dS| ~ 2^-8 |q| |k| per logit), the contract
    bound against the rounded-operand reference does not."""
    from speinet_amd import train as T
    B, H, W = 2, 15, 35
    gen = torch.Generator().manual_seed(40 + shift)
    m = B * H * W
    q = _f32(torch.randn(m, 256, generator=gen, dtype=torch.float64) * 0.35)
    kv = _f32(torch.randn(m, 512, generator=gen, dtype=torch.float64))
    rb = _f32(torch.randn(8, 25, 25, generator=gen, dtype=torch.float64) * 0.5)
    g = _f32(torch.randn(m, 256, generator=gen, dtype=torch.float64))
    rr, slack = _attn_ref(q, kv, rb, g, B, H, W, shift, _bf)
    re, _ = _attn_ref(q, kv, rb, g, B, H, W, shift, lambda t: t)
    got = {}
    for prec in ("bf16", "f32"):
        dl = [_leaf(t) for t in (q, kv, rb)]
        with _prec(prec):
            out = T._WindowAttention.apply(*dl, B, H, W, shift)
        out.backward(g.to(DEV).float())
        got[prec] = (out, dl[0].grad, dl[1].grad, dl[2].grad)
    for i, what in enumerate(("out", "dq", "dkv", "drelbias")):
        # an fp32 P / dS within round-off of a bf16 tie may round the other way than the float64 reference's: that entry's ulp times
        # the other operand is allowed on top of the bound (a few entries in 10^5; zero slack everywhere else)
        d = ((got["bf16"][i].detach().double().cpu() - rr[i]).abs() - slack[i]).clamp_min(0)
        print(f"{what}: {_err(got['bf16'][i], rr[i]):.1e} from the rounded-operand reference, {d.max().item() / rr[i].abs().max().item():.1e} "
              f"beyond the tie slack ({int((slack[i] > 0).sum())} elements with slack)")
        _check(what, rr[i] + (got["bf16"][i].detach().double().cpu() - rr[i]).sign() * d, rr[i], re[i], got["f32"][i], bound=ATTN)


def _net(which, b, h, w, seed_x, content="smooth"):
    from speinet_amd.speinet import default_args
    from speinet_amd.synth import synth_frames as smooth_frames, synth_frames_flat, synth_state_dict
    synth_frames = smooth_frames if content == "smooth" else synth_frames_flat
    from speinet_amd import train as T
    args = default_args()
    args.n_sequence = 3
    if which == "swint":
        from speinet_amd.swint import SPEINet
        net = SPEINet(n_sequence=3, args=args)
        x = synth_frames(b, h, w, seed=seed_x)[:, :3].contiguous().to(DEV)
        scales = T.drop_path_scales(net.cfg.depths, b, 2, generator=torch.Generator().manual_seed(3))
    else:
        from speinet_amd.speinet import SPEINet
        net = SPEINet(args=args)
        x = synth_frames(b, h, w, seed=seed_x, zero_ref=(b - 1,)).contiguous().to(DEV)
        zero = [i == b - 1 for i in range(b)]
        scales = T.speinet_drop_path_scales(net.cfg.depths, zero, 3, generator=torch.Generator().manual_seed(3))
    net.load_state_dict(synth_state_dict(net.state_dict(), seed=0), strict=True)
    return net.to(DEV).train(), x, scales


def _step(net, x, gt, scales, loss_fn, prec):
    net.train_precision = prec
    net.zero_grad()
    np.random.seed(5)
    out = net(x, drop_path_scales=scales)
    loss = loss_fn(out, gt)
    loss.backward()
    return out.detach().clone(), loss.item(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("which,content", [pytest.param("swint", "smooth", id="swint"), pytest.param("speinet", "smooth", id="speinet"),
                                           pytest.param("speinet", "flat", id="speinet-flat")])
def test_training_step_bf16_vs_f32(which, content):
    """The bf16 step against the f32 step on the batch of test_training_step_bf16x3_vs_f32 (B = 3 at 60x40, the full model's last
    sample reference-less, the same DropPath factors and HEM seed).  Output within 1.5e-2 of its range (the inference bf16 bound),
    loss within 5e-3 relative.  Gradients, relative L2 per parameter: median <= 1.2e-1, worst <= 3e-1.
    The first estimate (median 3e-2, worst 1.5e-1) held for the full model (measured 2.6e-2 / 1.2e-1) but not for swint (8e-2 /
    2.2e-1).  No single op is responsible: every op meets its contract (the tests above, <= 2e-5 beyond rounding ties), and with the
    loss reduced to plain L1 (no hard-example selection) the swint distances stay the same (8.1e-2 / 2.2e-1).  What remains is the
    contract itself compounding: every forward GEMM rounds its operands (2^-9 relative), every backward GEMM rounds dY and the saved
    activations again, and swint's gradient crosses the encoder, 2 x 6 Swin blocks and the decoder, so the parameters far from the
    loss sit furthest from the f32 gradient (outBlock 1.5e-2, encoder / Swin 8e-2 to 9e-2); the largest are the relative-position
    bias tables, sums of dS over every window, where P (dP - r_q) cancels.  bf16x3 (2^-16 products) measures 2.7e-3 / 8e-3 on the
    same batch.  Bounds: measured x 1.5.  content "flat": the full model on synth_frames_flat (letterbox bars, a clipped highlight,
    one sample faded to near-black: tied maxima in the gates, which use the same kernels in both modes), under the same bounds."""
    from speinet_amd.loss import Loss
    from speinet_amd.synth import synth_frames
    b, h, w = 3, 60, 40
    net, x, scales = _net(which, b, h, w, 91 if which == "swint" else 92, content)
    gt = synth_frames(b, h, w, seed=93)[:, 1].contiguous().to(DEV)
    loss_fn = Loss("1*L1+2*HEM", device=DEV)
    o32, l32, g32 = _step(net, x, gt, scales, loss_fn, "f32")
    o16, l16, g16 = _step(net, x, gt, scales, loss_fn, "bf16")
    net.train_precision = "f32"
    eo = (o16 - o32).abs().max().item() / (o32.max() - o32.min()).item()
    errs = sorted((g16[k] - g32[k]).norm().item() / max(g32[k].norm().item(), 1e-20) for k in g32 if g32[k].numel() > 4)
    med, worst = errs[len(errs) // 2], errs[-1]
    print(f"{which}: bf16 vs f32 step: output {eo:.1e}, loss {abs(l16 - l32) / abs(l32):.1e} rel, gradients median {med:.1e} worst {worst:.1e}")
    assert set(g16) == set(g32)
    assert eo < 1.5e-2 and abs(l16 - l32) < 5e-3 * abs(l32)
    assert med <= 1.2e-1 and worst <= 3e-1


def test_loss_curve_bf16(golden_dir):
    """G22 (swint, two 40x40 windows, 1*L1 + 2*HEM, Adam 1e-4, DropPath off, 6 steps) in bf16: the first loss within 5e-3 relative of
    the reference's float64 curve, every step within 2e-2, and the curve goes down."""
    from speinet_amd.loss import Loss
    from speinet_amd.swint import SPEINet
    from speinet_amd.speinet import default_args
    from speinet_amd.synth import synth_frames, synth_state_dict
    d = np.load(os.path.join(golden_dir, "g22_losscurve_swint_40x40.npz"))
    seed, b, h, w = (int(d[k]) for k in ("seed", "b", "h", "w"))
    args = default_args()
    args.n_sequence = 3
    net = SPEINet(n_sequence=3, args=args)
    net.load_state_dict(synth_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.to(DEV).train()
    net.train_precision = "bf16"
    x = synth_frames(b, h, w, seed=seed)[:, :3].contiguous().to(DEV)
    gt = synth_frames(b, h, w, seed=seed + 500)[:, 1].contiguous().to(DEV)
    no_drop = [[None] * sum(net.cfg.depths) for _ in range(2)]
    loss_fn = Loss("1*L1+2*HEM", device=DEV)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, weight_decay=0.0)
    np.random.seed(seed)
    losses = []
    for _ in range(len(d["losses"])):
        out = net(x, drop_path_scales=no_drop)
        opt.zero_grad()
        loss = loss_fn(out, gt)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    ref64 = [float(v) for v in d["losses64"]]
    rel = [abs(a - c) / abs(c) for a, c in zip(losses, ref64)]
    print("bf16   :", ", ".join(f"{v:.6f}" for v in losses))
    print("float64:", ", ".join(f"{v:.6f}" for v in ref64))
    print("relative:", ", ".join(f"{v:.1e}" for v in rel))
    assert rel[0] < 5e-3 and max(rel) < 2e-2
    assert losses[-1] < losses[0]


def test_bf16_step_is_reproducible():
    """Two bf16 steps from the same state give bit-identical gradients (fixed-order two-stage sums everywhere)."""
    from speinet_amd.loss import Loss
    from speinet_amd.synth import synth_frames
    net, x, scales = _net("swint", 2, 40, 40, 31)
    gt = synth_frames(2, 40, 40, seed=32)[:, 1].contiguous().to(DEV)
    loss_fn = Loss("1*L1+2*HEM", device=DEV)
    o1, l1, g1 = _step(net, x, gt, scales, loss_fn, "bf16")
    o2, l2, g2 = _step(net, x, gt, scales, loss_fn, "bf16")
    assert torch.equal(o1, o2) and l1 == l2 and set(g1) == set(g2)
    assert all(torch.equal(g1[k], g2[k]) for k in g1), [k for k in g1 if not torch.equal(g1[k], g2[k])]


def test_inplace_data_edit_reaches_the_bf16_weights():
    """The single bf16 fragments are cached on the parameters like the split halves: after `p.data.mul_()` (invisible to `_version`)
    the bf16 step must follow the f32 step, not the stale fragments."""
    from speinet_amd.speinet import default_args
    from speinet_amd.swint import SPEINet
    from speinet_amd.synth import synth_frames, synth_state_dict
    from speinet_amd import train as T
    args = default_args()
    args.n_sequence = 3
    net = SPEINet(n_sequence=3, args=args)
    net.load_state_dict(synth_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.to(DEV).train()
    x = synth_frames(2, 40, 40, seed=17)[:, :3].contiguous().to(DEV)
    scales = T.drop_path_scales(net.cfg.depths, 2, 2, generator=torch.Generator().manual_seed(1))
    net.train_precision = "bf16"
    with torch.no_grad():
        before = net(x, drop_path_scales=scales).clone()
        assert any(any(isinstance(k, tuple) and k[1] == "bf16" for k in (getattr(p, "_spei_split", None) or {})) for p in net.parameters()), \
            "the bf16 fragment cache is in use"
        for name, p in net.named_parameters():
            if name.endswith("weight") and p.dim() in (2, 4):
                p.data.mul_(1.25)
        after16 = net(x, drop_path_scales=scales).clone()
        net.train_precision = "f32"
        after32 = net(x, drop_path_scales=scales).clone()
    scale = after32.abs().max().item()
    moved = (after16 - before).abs().max().item() / scale
    apart = (after16 - after32).abs().max().item() / scale
    print(f"in-place edit: bf16 output moved by {moved:.2e}, bf16 vs f32 after the edit {apart:.1e}")
    assert moved > 1e-2 and apart < moved / 10           # stale fragments: after16 stays near `before`, apart ~ moved
