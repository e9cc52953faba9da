"""SURVEY.md §8 f3 / BASELINE.json config 5: the training step of the swint model on the HIP kernels.

Two layers of checks:
  * every new backward kernel against torch's own autograd of the same operation evaluated in float64 on the CPU (LayerNorm,
    GELU, linear with residual + DropPath factor, window attention with shift masks, Conv2d / ConvTranspose2d data, weight and
    bias gradients);
  * G20 (tests/golden/make_golden_train.py): one full training step of the REFERENCE's model/swint.py — train() mode
    (BatchNorm(1) batch statistics, DropPath), loss 1*L1 + 2*HEM, backward, Adam — output, loss, every parameter's gradient,
    the BatchNorm buffers and the updated parameters.
Tolerances are written where they are used: fp32 kernels against fp32 / fp64 references, summation orders differ.
"""
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


def _rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _leaf(t, dev):
    return t.to(dev).float().requires_grad_(True)


def test_layernorm_gelu_backward():
    from speinet_amd import train as T
    gen = torch.Generator().manual_seed(1)
    for m in (7, 100, 2500):
        x = torch.randn(m, 256, generator=gen, dtype=torch.float64) * 1.7 + 0.3
        g, b = torch.randn(256, generator=gen, dtype=torch.float64), torch.randn(256, generator=gen, dtype=torch.float64)
        r = torch.randn(m, 256, generator=gen, dtype=torch.float64)
        xr, gr, br = (t.clone().requires_grad_(True) for t in (x, g, b))
        (F.layer_norm(xr, (256,), gr, br) * r).sum().backward()
        xd, gd, bd = _leaf(x, DEV), _leaf(g, DEV), _leaf(b, DEV)
        y = T._LayerNorm.apply(xd, gd, bd)
        assert _rel(y, F.layer_norm(x, (256,), g, b)) < 2e-6
        (y * r.to(DEV).float()).sum().backward()
        assert _rel(xd.grad, xr.grad) < 5e-6 and _rel(gd.grad, gr.grad) < 5e-6 and _rel(bd.grad, br.grad) < 5e-6, m
    pre = torch.randn(400, 512, generator=gen, dtype=torch.float64) * 2.5
    r = torch.randn(400, 512, generator=gen, dtype=torch.float64)
    pr = pre.clone().requires_grad_(True)
    (F.gelu(pr) * r).sum().backward()
    pd = _leaf(pre, DEV)
    y = T._Gelu.apply(pd)
    assert _rel(y, F.gelu(pre)) < 2e-6
    (y * r.to(DEV).float()).sum().backward()
    assert _rel(pd.grad, pr.grad) < 2e-6


def test_linear_backward_with_residual_and_droppath():
    from speinet_amd import train as T
    gen = torch.Generator().manual_seed(2)
    for m, k, n in ((200, 256, 512), (150, 512, 256), (64, 384, 128)):
        x = torch.randn(m, k, generator=gen, dtype=torch.float64)
        w = torch.randn(n, k, generator=gen, dtype=torch.float64) * 0.05
        b = torch.randn(n, generator=gen, dtype=torch.float64)
        res = torch.randn(m, n, generator=gen, dtype=torch.float64)
        rs = torch.tensor([0.0, 1.0 / 0.9])[torch.randint(0, 2, (m,), generator=gen)].double()
        r = torch.randn(m, n, generator=gen, dtype=torch.float64)
        for use in (False, True):
            leaves = [t.clone().requires_grad_(True) for t in (x, w, b, res)]
            y = F.linear(leaves[0], leaves[1], leaves[2])
            y = leaves[3] + rs[:, None] * y if use else y
            (y * r).sum().backward()
            dl = [_leaf(t, DEV) for t in (x, w, b, res)]
            yd = T._Linear.apply(dl[0], dl[1], dl[2], dl[3] if use else None, rs.to(DEV).float() if use else None)
            assert _rel(yd, y) < 3e-6
            (yd * r.to(DEV).float()).sum().backward()
            for a, e in zip(dl[:3] + (dl[3:] if use else []), leaves):
                assert _rel(a.grad, e.grad) < 5e-6, (m, k, n, use)


def _window_attention_ref(q, kv, relbias, B, H, W, shift):
    """model/swinir.py:115-149 + :238-275 partition / roll / mask, float64 on the CPU; q pre-scaled."""
    ws, heads = 5, 8
    def part(t, c):
        t = t.view(B, H, W, c)
        if shift:
            t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))
        return t.view(B, H // ws, ws, W // ws, ws, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, c)
    qw, kvw = part(q, 256), part(kv, 512)
    nb = qw.shape[0]
    qh = qw.view(nb, 25, heads, 32).permute(0, 2, 1, 3)
    kh = kvw[..., :256].reshape(nb, 25, heads, 32).permute(0, 2, 1, 3)
    vh = kvw[..., 256:].reshape(nb, 25, heads, 32).permute(0, 2, 1, 3)
    attn = qh @ kh.transpose(-2, -1) + relbias.unsqueeze(0)
    if shift:
        from speinet_amd.speinet import _shift_mask
        mask = _shift_mask(H, W, ws, shift).double()                                     # [nW, 25, 25]
        attn = attn.view(B, -1, heads, 25, 25) + mask.unsqueeze(1).unsqueeze(0)
        attn = attn.view(-1, heads, 25, 25)
    o = (attn.softmax(-1) @ vh).transpose(1, 2).reshape(nb, 25, 256)
    o = o.view(B, H // ws, W // ws, ws, ws, 256).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, 256)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o.reshape(B * H * W, 256)


@pytest.mark.parametrize("shift", [0, 2])
def test_window_attention_backward(shift):
    from speinet_amd import train as T
    gen = torch.Generator().manual_seed(3 + shift)
    for B, H, W in ((1, 10, 10), (2, 10, 15), (1, 50, 50)):
        m = B * H * W
        q = torch.randn(m, 256, generator=gen, dtype=torch.float64) * 0.6
        kv = torch.randn(m, 512, generator=gen, dtype=torch.float64)
        rb = torch.randn(8, 25, 25, generator=gen, dtype=torch.float64) * 0.5
        r = torch.randn(m, 256, generator=gen, dtype=torch.float64)
        leaves = [t.clone().requires_grad_(True) for t in (q, kv, rb)]
        ref = _window_attention_ref(*leaves, B, H, W, shift)
        (ref * r).sum().backward()
        dl = [_leaf(t, DEV) for t in (q, kv, rb)]
        out = T._WindowAttention.apply(*dl, B, H, W, shift)
        assert _rel(out, ref) < 3e-6, (B, H, W)
        (out * r.to(DEV).float()).sum().backward()
        for a, e, name in zip(dl, leaves, ("dq", "dkv", "dbias")):
            assert _rel(a.grad, e.grad) < 1e-5, (name, B, H, W, _rel(a.grad, e.grad))


def test_conv_family_backward():
    from speinet_amd import train as T
    gen = torch.Generator().manual_seed(5)
    def nchw(rows, B, H, W):
        return rows.view(B, H, W, -1).permute(0, 3, 1, 2)
    def rows(t):
        return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    for B, H, W, k, n, ks, stride, relu, res in ((2, 12, 10, 32, 32, 5, 1, True, False), (1, 20, 20, 32, 64, 5, 2, True, False),
                                                 (2, 10, 10, 256, 256, 3, 1, False, True), (1, 11, 13, 64, 128, 5, 2, True, False),
                                                 (1, 8, 8, 32, 32, 5, 1, False, False)):
        x = torch.randn(B, k, H, W, generator=gen, dtype=torch.float64)
        w = torch.randn(n, k, ks, ks, generator=gen, dtype=torch.float64) * (1.0 / math.sqrt(k * ks * ks))
        b = torch.randn(n, generator=gen, dtype=torch.float64) * 0.1
        lx, lw, lb = (t.clone().requires_grad_(True) for t in (x, w, b))
        y = F.conv2d(lx, lw, lb, stride=stride, padding=ks // 2)
        rr = torch.randn(y.shape, generator=gen, dtype=torch.float64)
        lr_ = rr.clone().requires_grad_(True) if res else None
        if relu:
            y = F.relu(y)
        if res:
            y = y + lr_
        g = torch.randn(y.shape, generator=gen, dtype=torch.float64)
        (y * g).sum().backward()
        dx, dw, db = _leaf(rows(x), DEV), _leaf(w, DEV), _leaf(b, DEV)
        dres = _leaf(rows(rr), DEV) if res else None
        yd = T._Conv2d.apply(dx, dw, db, dres, B, H, W, ks, stride, relu)
        assert _rel(yd, rows(y)) < 3e-6
        (yd * rows(g).to(DEV).float()).sum().backward()
        assert _rel(dx.grad, rows(lx.grad)) < 5e-6 and _rel(dw.grad, lw.grad) < 5e-6 and _rel(db.grad, lb.grad) < 5e-6, (B, H, W, k, n, ks, stride)
        if res:
            assert _rel(dres.grad, rows(lr_.grad)) < 1e-6
    for B, H, W, k, n in ((2, 5, 5, 128, 64), (1, 10, 15, 64, 32)):
        x = torch.randn(B, k, H, W, generator=gen, dtype=torch.float64)
        w = torch.randn(k, n, 3, 3, generator=gen, dtype=torch.float64) * (1.0 / math.sqrt(k * 9 / 4))
        b = torch.randn(n, generator=gen, dtype=torch.float64) * 0.1
        lx, lw, lb = (t.clone().requires_grad_(True) for t in (x, w, b))
        y = F.relu(F.conv_transpose2d(lx, lw, lb, stride=2, padding=1, output_padding=1))
        g = torch.randn(y.shape, generator=gen, dtype=torch.float64)
        (y * g).sum().backward()
        dx, dw, db = _leaf(rows(x), DEV), _leaf(w, DEV), _leaf(b, DEV)
        yd = T._ConvT2d.apply(dx, dw, db, B, H, W)
        assert _rel(yd, rows(y)) < 3e-6
        (yd * rows(g).to(DEV).float()).sum().backward()
        assert _rel(dx.grad, rows(lx.grad)) < 5e-6 and _rel(dw.grad, lw.grad) < 5e-6 and _rel(db.grad, lb.grad) < 5e-6, (B, H, W, k, n)


def _search_transfer_ref(lr, ref3, ref2, ref1):
    """model/SearchTransfer.py:24-50 restated on NCHW float64 tensors: cosine correlation of 3x3 patches, arg-max over the reference
    positions, S and the three gathered + overlap-added maps."""
    n, c, h, w = lr.shape
    a = F.normalize(F.unfold(lr, 3, padding=1), dim=1)                        # [n, 9c, hw]
    bq = F.normalize(F.unfold(ref3, 3, padding=1).transpose(1, 2), dim=2)     # [n, hrwr, 9c]
    s, arg = torch.bmm(bq, a).max(dim=1)                                      # [n, hw]
    outs = []
    for rf, sc in ((ref3, 1), (ref2, 2), (ref1, 4)):
        if rf is None:
            outs.append(None)
            continue
        u = F.unfold(rf, 3 * sc, padding=sc, stride=sc)                       # [n, c k k, hrwr]
        t = torch.gather(u, 2, arg.unsqueeze(1).expand(-1, u.shape[1], -1))
        outs.append(F.fold(t, (h * sc, w * sc), 3 * sc, padding=sc, stride=sc) / 9.0)
    return s.view(n, h, w), outs[0], outs[1], outs[2], arg


def test_search_transfer_bicubic_rowscale_backward():
    """The SearchTransfer Function (S through the normalised correlation at the arg-max, the three gathers), the bicubic adjoint
    and the row scale against float64 torch autograd of the same operations; also the SelfTransfer form (rotated reference,
    S only) on a non-square map."""
    from speinet_amd import train as T
    gen = torch.Generator().manual_seed(9)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    for B, H, W in ((1, 10, 10), (2, 10, 15)):
        lr = torch.randn(B, 128, H, W, generator=gen, dtype=torch.float64)
        r3 = torch.randn(B, 128, H, W, generator=gen, dtype=torch.float64)
        r2 = torch.randn(B, 64, 2 * H, 2 * W, generator=gen, dtype=torch.float64)
        r1 = torch.randn(B, 32, 4 * H, 4 * W, generator=gen, dtype=torch.float64)
        leaves = [t.clone().requires_grad_(True) for t in (lr, r3, r2, r1)]
        s, t3, t2, t1, arg = _search_transfer_ref(*leaves)
        gs = [torch.randn(t.shape, generator=gen, dtype=torch.float64) for t in (s, t3, t2, t1)]
        (s * gs[0]).sum().backward(retain_graph=True)
        ((t3 * gs[1]).sum() + (t2 * gs[2]).sum() + (t1 * gs[3]).sum()).backward()
        dl = [_leaf(rows(t), DEV) for t in (lr, r3, r2, r1)]
        S, T3, T2, T1, A = T._SearchTransfer.apply(*dl, B, H, W, H, W)
        assert torch.equal(A.cpu().long().view(B, -1), arg), "arg-max differs from float64 torch"
        assert _rel(S, s.reshape(-1)) < 3e-6 and _rel(T3, rows(t3)) < 1e-6 and _rel(T2, rows(t2)) < 1e-6 and _rel(T1, rows(t1)) < 1e-6
        tot = (S * gs[0].reshape(-1).to(DEV).float()).sum() + sum((a * rows(g).to(DEV).float()).sum() for a, g in zip((T3, T2, T1), gs[1:]))
        tot.backward()
        for a, e, nm in zip(dl, leaves, ("d lr", "d ref3", "d ref2", "d ref1")):
            assert _rel(a.grad, rows(e.grad)) < 2e-5, (nm, B, H, W, _rel(a.grad, rows(e.grad)))
        # SelfTransfer: reference = the query map transposed and flipped; S only
        l2 = lr.clone().requires_grad_(True)
        s2 = _search_transfer_ref(l2, l2.transpose(2, 3).flip(2), None, None)[0]
        (s2 * gs[0]).sum().backward()
        xd = _leaf(rows(lr), DEV)
        ref = xd.view(B, H, W, -1).transpose(1, 2).flip(1).reshape(B * H * W, -1)
        S2 = T._SearchTransfer.apply(xd, ref, None, None, B, H, W, W, H)[0]
        assert _rel(S2, s2.reshape(-1)) < 3e-6
        (S2 * gs[0].reshape(-1).to(DEV).float()).sum().backward()
        assert _rel(xd.grad, rows(l2.grad)) < 2e-5, ("self", B, H, W, _rel(xd.grad, rows(l2.grad)))
    for B, H, W, c, sc in ((2, 10, 15, 128, 2), (1, 7, 9, 64, 2), (2, 10, 10, 1, 2), (1, 10, 12, 1, 4), (1, 6, 5, 32, 4)):
        x = torch.randn(B, c, H, W, generator=gen, dtype=torch.float64)
        xr = x.clone().requires_grad_(True)
        y = F.interpolate(xr, scale_factor=sc, mode="bicubic")
        g = torch.randn(y.shape, generator=gen, dtype=torch.float64)
        (y * g).sum().backward()
        xd = _leaf(rows(x), DEV)
        yd = T._Bicubic.apply(xd, B, H, W, sc)
        assert _rel(yd, rows(y)) < 2e-6
        (yd * rows(g).to(DEV).float()).sum().backward()
        assert _rel(xd.grad, rows(xr.grad)) < 3e-6, (B, H, W, c, sc, _rel(xd.grad, rows(xr.grad)))
    x = torch.randn(300, 128, generator=gen, dtype=torch.float64)
    sv = torch.randn(300, generator=gen, dtype=torch.float64)
    g = torch.randn(300, 128, generator=gen, dtype=torch.float64)
    xr, sr = x.clone().requires_grad_(True), sv.clone().requires_grad_(True)
    (xr * sr[:, None] * g).sum().backward()
    xd, sd = _leaf(x, DEV), _leaf(sv, DEV)
    y = T._RowScale.apply(xd, sd)
    assert _rel(y, x * sv[:, None]) < 1e-6
    (y * g.to(DEV).float()).sum().backward()
    assert _rel(xd.grad, xr.grad) < 1e-6 and _rel(sd.grad, sr.grad) < 3e-6


def _scales_from_draws(draws: np.ndarray, depths, n_calls: int) -> list:
    """The fixture's flat DropPath draws [n_draws, B] -> train.drop_path_scales' nesting."""
    from speinet_amd.train import drop_path_rates
    rates = drop_path_rates(depths)
    it = iter(torch.from_numpy(draws))
    out = []
    for _ in range(n_calls):
        out.append([None if r <= 0 else (next(it), next(it)) for r in rates])
    assert next(it, None) is None
    return out


@pytest.mark.parametrize("name", ["g20_train_swint_40x40", "g20_train_swint_n1_40x60"])
def test_training_step_vs_reference(golden_dir, name):
    """One full training step against the reference's own (G20): output, loss 1*L1 + 2*HEM, all 828 parameter gradients, the
    BatchNorm(1) running buffers and the parameters after Adam(lr 1e-4).step().

    Tolerances: output 2e-5 abs (values up to 0.6; measured 6e-7), loss 2e-6.  Gradients: every parameter's L2 norm and its
    subsample (every 97th element; G23 every 997th) within 5e-3 of the parameter's gradient norm, against the reference's fp32 run AND against
    the same step run by the reference in float64 (`sub64/*` in the fixture), median below 1e-3 — see the comment at the
    assertion for what was measured and why.  Parameters with a gradient norm below 1e-5 of the largest are compared on an
    absolute scale."""
    from speinet_amd import train as T
    from speinet_amd.loss import Loss
    from speinet_amd.swint import SPEINet
    from speinet_amd.speinet import default_args
    from speinet_amd.synth import state_dict_template, synth_frames, synth_state_dict
    d = np.load(os.path.join(golden_dir, name + ".npz"))
    seed, n_seq, b, h, w = (int(d[k]) for k in ("seed", "n_sequence", "b", "h", "w"))
    args = default_args()
    args.n_sequence = n_seq
    net = SPEINet(n_sequence=n_seq, args=args)
    net.load_state_dict(synth_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.to(DEV).train()
    x = synth_frames(b, h, w, seed=seed)[:, :n_seq].contiguous().to(DEV)
    gt = synth_frames(b, h, w, seed=seed + 500)[:, 1].contiguous().to(DEV)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, weight_decay=0.0)
    scales = _scales_from_draws(d["draws"], net.cfg.depths, 1 if n_seq == 1 else n_seq - 1)
    # the same factors come out of the restated DropPath generator from the same seed
    torch.manual_seed(seed)
    mine = T.drop_path_scales(net.cfg.depths, b, 1 if n_seq == 1 else n_seq - 1)
    for ca, cb in zip(mine, scales):
        for pa, pb in zip(ca, cb):
            assert (pa is None) == (pb is None)
            if pa is not None:
                assert torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1])
    _check_step(name, d, net, x, gt, scales, opt, seed)


def _check_step(name, d, net, x, gt, scales, opt, seed):
    """Run one step on the HIP model and compare output, loss, gradients, BatchNorm buffers and the Adam update with fixture d."""
    from speinet_amd.loss import Loss
    np.random.seed(seed)
    loss_fn = Loss("1*L1+2*HEM", device=DEV)
    out = net(x, drop_path_scales=scales)
    opt.zero_grad()
    err = (out.detach().cpu() - torch.from_numpy(d["out"])).abs().max().item()
    assert err < 2e-5
    # HEM's hard mask is a threshold decision (the pixels above the median residual): an output that differs from the reference's by
    # 1e-6 can move ONE pixel across it — 1e-4 of the loss of a 40x60 crop, and a visible step in the gradients of the last layers.
    # The step is therefore taken under the REFERENCE's mask (the mask of its own output, same numpy draws) whenever the two differ,
    # by at most a few pixels; with equal masks this is exactly `loss_fn(out, gt)`.
    hem = [fn for _, kind, fn in loss_fn.terms if kind == "HEM"][0]
    state = np.random.get_state()
    m_out = hem.hard_mining_mask(out.detach(), gt)
    np.random.set_state(state)
    m_ref = hem.hard_mining_mask(torch.from_numpy(d["out"]).to(DEV), gt)
    flips = int((m_ref != m_out).sum().item())
    assert flips <= 3, flips
    hem_term = 2.0 * (out * m_ref - gt * m_ref).abs().mean()
    loss = (out - gt).abs().mean() + hem_term
    if flips == 0:
        np.random.set_state(state)
        assert abs(loss_fn(out, gt).item() - loss.item()) < 1e-7
    loss.backward()
    print(f"{name}: max |out - ref| {err:.2e}; loss {loss.item():.6f} vs {float(d['loss']):.6f}; {flips} pixel(s) of the hard-example mask differ")
    assert abs(loss.item() - float(d["loss"])) < 2e-6 and abs(hem_term.item() - 2.0 * float(d["hem"])) < 2e-6
    gmax = max(float(d[k]) for k in d.files if k.startswith("norm/"))
    st = int(d["stride"]) if "stride" in d.files else 97          # the fixture's subsample stride (gradients and Adam update)
    rows = []
    unused = set(str(u) for u in d["unused"]) if "unused" in d.files else set()
    for k, p in net.named_parameters():
        if k in unused:                   # parameters the reference's forward never touches (model/speinet.py: search23, connect, ...)
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert p.grad is not None, k
        g = p.grad.detach().reshape(-1).cpu()
        ref_norm = float(d["norm/" + k])
        scale = max(ref_norm, 1e-5 * gmax)
        if ".bn." in k:
            # a one-number gradient (the BatchNorm(1) affine of a gate) is a sum of ~10^3..10^4 signed terms that can cancel to
            # 1e-3 of their size: measured against the gradient norm of the SAME gate's convolution weight (test_gpu_grad.py)
            scale = max(scale, float(d["norm/" + k.rsplit(".bn.", 1)[0] + ".conv.weight"]))
        sub32, sub64 = torch.from_numpy(d["sub/" + k]), torch.from_numpy(d["sub64/" + k])
        e_norm = abs(g.norm().item() - ref_norm) / scale
        e32 = (g[::st] - sub32).norm().item() / scale            # HIP fp32 vs the reference's fp32
        e64 = (g[::st] - sub64).norm().item() / scale            # HIP fp32 vs the reference in float64
        r64 = (sub32 - sub64).norm().item() / scale              # the reference's fp32 vs its own float64: fp32 summation noise
        r64 = max(r64, abs(ref_norm - float(d["norm64/" + k])) / scale)
        rows.append((k, e_norm, e32, e64, r64))
    top = lambda i: ", ".join(f"{r[0]} {r[i]:.1e}" for r in sorted(rows, key=lambda r: -r[i])[:4])
    print(f"{name}: {len(rows)} gradients.  HIP vs reference fp32, worst: {top(2)}\n   HIP vs reference float64, worst: {top(3)}\n"
          f"   reference fp32 vs its own float64, worst: {top(4)}")
    groups = {}
    for k, e_norm, e32, e64, r64 in rows:
        parts = k.split(".")
        gk = ".".join(parts[:3]) if parts[0] == "swin" and parts[1] == "layers" else ".".join(parts[:2])
        groups.setdefault(gk, []).append((e64, r64))
    print("   per stage, median over its parameters of (HIP vs float64, reference fp32 vs float64): "
          + "; ".join(f"{gk} {np.median([a for a, _ in v]):.1e}/{np.median([b for _, b in v]):.1e}" for gk, v in groups.items()))
    # Measured (40x40, B = 2): the last stage before the loss (outBlock) agrees with the float64 gradients to 1e-7, the reference's
    # own fp32 run to 7e-8; from decoder_first upstream BOTH runs sit at a uniform distance from float64 (reference fp32 2e-5
    # median / 2e-4 worst, HIP 2e-4 median / 2e-3 worst on the cancellation-prone BatchNorm scalars): the signature of ReLU /
    # max-pool / hard-mask decisions on elements within fp32 round-off of their threshold resolving differently under another
    # summation order — one element in 10^5 moves every upstream sum by that much (test_gpu_grad.py saw the same at 40x60), while
    # every kernel on its own matches float64 autograd to 1e-6 (the tests above, tools/diag_resblock_train.py).
    med = float(np.median([r[3] for r in rows]))
    assert med < 1e-3, med
    for k, e_norm, e32, e64, r64 in rows:
        # (the n_sequence 1, B = 1 case: the reference's float64 run itself sits up to 1.2e-2 from its fp32 run on the gate
        # parameters — a batch of one map — so there the bound is relative to the reference's own fp32-to-float64 distance)
        bound = max(5e-3, 2.0 * r64 + 1e-3)
        if x.shape[0] == 1 and ".te." in k:
            # ... and on the triplet-gate parameters of that case by the worst such distance of the case (1.2e-2: a gate's BatchNorm
            # normalises ONE small plane there, every decision flip upstream moves all of its sums)
            bound = max(bound, 1.5e-2)
        assert e32 < bound and e_norm < bound and e64 < bound, (k, e_norm, e32, e64, r64)
    opt.step()
    sd = net.state_dict()
    for k in d.files:
        if k.startswith("bn/"):
            ref = torch.from_numpy(np.asarray(d[k]))
            got = sd[k[3:]].cpu()
            if "num_batches" in k:
                assert int(got) == int(ref), k
            else:
                assert (got - ref).abs().max().item() < 1e-5 * max(1.0, ref.abs().max().item()), k
        elif k.startswith("adam/"):
            ref = torch.from_numpy(d[k])
            got = sd[k[5:]].reshape(-1)[::st].cpu()
            # Adam's first step moves every element by lr * g / (|g| + eps): +-1e-4 wherever |g| >> eps = 1e-8; an element whose
            # gradient is within rounding of zero can land on the other side, so compare in units of the step
            frac_bad = ((got - ref).abs() > 2e-5).float().mean().item()
            assert frac_bad < 0.02, (k, frac_bad)




def test_training_step_speinet_vs_reference(golden_dir):
    """G21: one full training step of the reference's `model/speinet.py` (trainer/trainer_swint_hsa_nsf.py:27-40) on a batch of
    three 40x40 windows, the second with an all-zero frame 3: `_forwardb` (SelfTransfer) on a sub-batch of one, `_forwardbs`
    (SearchTransfer: correlation arg-max, S and the three gathered maps, all differentiated) on the other two.  Same checks
    and bounds as G20: output, loss, 850 gradients (fp32 and float64 reference runs), BatchNorm buffers, Adam update; the 8
    parameters the reference's forward never uses get no gradient."""
    from speinet_amd import train as T
    from speinet_amd.speinet import SPEINet, default_args
    from speinet_amd.synth import synth_frames, synth_state_dict
    name = "g21_train_speinet_40x40"
    d = np.load(os.path.join(golden_dir, name + ".npz"))
    seed, b, h, w = (int(d[k]) for k in ("seed", "b", "h", "w"))
    net = SPEINet(args=default_args())
    net.load_state_dict(synth_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.to(DEV).train()
    x = synth_frames(b, h, w, seed=seed, zero_ref=(1,)).contiguous().to(DEV)
    gt = synth_frames(b, h, w, seed=seed + 500)[:, 1].contiguous().to(DEV)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, weight_decay=0.0)
    zero_ref = [False, True, False]
    torch.manual_seed(seed)
    scales = T.speinet_drop_path_scales(net.cfg.depths, zero_ref, 3)
    # the restated DropPath stream equals the reference run's recorded draws: first the no-reference sub-batch, then the other
    flat = [t for has_ref in (False, True) for call in scales[has_ref] for pair in call if pair is not None for t in pair]
    assert len(flat) == d["draws"].shape[0]
    for t, row, n in zip(flat, d["draws"], d["draw_len"]):
        assert t.numel() == int(n) and torch.equal(t, torch.from_numpy(row[:int(n)]))
    _check_step(name, d, net, x, gt, scales, opt, seed)


def test_training_step_speinet_flat_vs_reference(golden_dir):
    """G23: the G21 step on flat content (synth_frames_flat: letterbox bars, a clipped highlight, sample 0 faded to near-black, sample 1
    without a reference), whose feature maps hold exact ties at the ResBlock gates' row / column maxima.  The reference's ZPool
    (torch.max(dim)) hands a tied maximum's gradient to its first index only.  Same checks and bounds as G20 / G21."""
    from speinet_amd import train as T
    from speinet_amd.speinet import SPEINet, default_args
    from speinet_amd.synth import synth_frames_flat, synth_state_dict
    from oracle.fixtures import load_train_fixture
    name = "g23_train_speinet_flat_40x40"
    d = load_train_fixture(os.path.join(golden_dir, name + ".npz"))
    seed, b, h, w = (int(d[k]) for k in ("seed", "b", "h", "w"))
    net = SPEINet(args=default_args())
    net.load_state_dict(synth_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.to(DEV).train()
    x = synth_frames_flat(b, h, w, seed=seed, zero_ref=(1,)).contiguous().to(DEV)
    gt = synth_frames_flat(b, h, w, seed=seed + 500)[:, 1].contiguous().to(DEV)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, weight_decay=0.0)
    torch.manual_seed(seed)
    scales = T.speinet_drop_path_scales(net.cfg.depths, [False, True, False], 3)
    flat = [t for has_ref in (False, True) for call in scales[has_ref] for pair in call if pair is not None for t in pair]
    assert len(flat) == d["draws"].shape[0]
    for t, row, n in zip(flat, d["draws"], d["draw_len"]):
        assert t.numel() == int(n) and torch.equal(t, torch.from_numpy(row[:int(n)]))
    _check_step(name, d, net, x, gt, scales, opt, seed)


def test_trainer_steps_reduce_the_loss():
    """speinet_amd.trainer.Trainer on the HIP model: five Adam steps on one fixed batch of 40x40 crops lower the loss (train()
    mode, DropPath drawn from torch's generator, HEM masks from numpy's), and every parameter moved."""
    from speinet_amd.loss import Loss
    from speinet_amd.swint import SPEINet
    from speinet_amd.speinet import default_args
    from speinet_amd.synth import synth_frames, synth_state_dict
    from speinet_amd.trainer import Trainer
    args = default_args()
    args.n_sequence = 3
    net = SPEINet(n_sequence=3, args=args)
    net.load_state_dict(synth_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.to(DEV)
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    x = synth_frames(2, 40, 40, seed=31)[:, :3].contiguous().to(DEV)
    gt = synth_frames(2, 40, 40, seed=32)[:, 1].contiguous().to(DEV)
    torch.manual_seed(5)
    np.random.seed(5)
    tr = Trainer(net, Loss("1*L1+2*HEM", device=DEV), lr=1e-4)
    losses = [tr.step(x, gt) for _ in range(5)]
    print("losses:", ", ".join(f"{v:.5f}" for v in losses))
    assert losses[-1] < losses[0] and all(np.isfinite(losses))
    moved = sum(int(not torch.equal(before[k], v.detach())) for k, v in net.named_parameters())
    assert moved == len(before), (moved, len(before))
    # evaluation after training (Trainer.test in the reference: model.eval() under no_grad): the inference path must see the UPDATED
    # parameters — its packed weights were dropped by the training forward
    net.eval()
    net.precision = "f32"
    with torch.no_grad():
        ev = net(x)
    net.autograd = True                            # opt in: eval() + recording alone stays on the inference kernels
    ev2 = net(x)                                   # the differentiable graph reads the live parameters
    assert ev2.requires_grad
    assert (ev - ev2.detach()).abs().max().item() < 2e-5
    del net.autograd                               # intent not stated: inference path, and a warning at the call site
    with pytest.warns(UserWarning, match="INFERENCE kernels"):
        ev3 = net(x)
    assert not ev3.requires_grad and torch.equal(ev3, ev)
    net.autograd = False                           # stated: inference path, silent
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ev4 = net(x)
    assert not ev4.requires_grad and torch.equal(ev4, ev)


@pytest.mark.parametrize("which", ["swint", "speinet"])
def test_training_graph_matches_inference_path_at_crop_size(which):
    """Size-independent tie between the two paths at the training crop size (200x200, option/template.py:6): in eval() mode the
    differentiable graph (running BatchNorm statistics, no DropPath) must give the frames the f32 inference path gives —
    the path the full-size goldens G14-G18 pin — and a backward pass through it must reach every parameter the forward uses."""
    from speinet_amd.speinet import default_args
    from speinet_amd.synth import synth_frames, synth_state_dict
    args = default_args()
    args.n_sequence = 3
    if which == "swint":
        from speinet_amd.swint import SPEINet
        net = SPEINet(n_sequence=3, args=args)
        x = synth_frames(2, 200, 200, seed=41)[:, :3].contiguous().to(DEV)
    else:
        from speinet_amd.speinet import SPEINet
        net = SPEINet(args=args)
        x = synth_frames(2, 200, 200, seed=42, zero_ref=(1,)).contiguous().to(DEV)
    net.load_state_dict(synth_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.to(DEV).eval()
    net.precision = "f32"
    with torch.no_grad():
        ref = net(x)
    net.autograd = True                             # eval() + opt-in -> the differentiable graph, eval-mode semantics
    out = net(x)
    assert out.requires_grad
    err = (out.detach() - ref).abs().max().item()
    print(f"{which}: max |training-graph output - inference output| at 200x200: {err:.2e} (values up to {ref.abs().max().item():.2f})")
    assert err < 2e-5 * max(1.0, ref.abs().max().item())
    out.square().mean().backward()
    missing = [k for k, p in net.named_parameters() if p.grad is None]
    allowed = ("search23", "connect", "SearchTransfer.search") if which == "speinet" else ()
    assert all(any(a in k for a in allowed) for k in missing), missing


@pytest.mark.parametrize("which", ["swint", "speinet"])
def test_training_step_bf16x3_vs_f32(which):
    """`train_precision = "bf16x3"` (forward and stride-1 data-gradient GEMMs as split products on the 16-bit matrix pipe) against the
    fp32 step G20 / G21 pin: same batch, same DropPath factors and HEM draws — output within 2e-4 of its range (7e-6 measured), loss
    to 1e-4.  Gradients: median 2.5e-3, worst 1e-2 of a parameter's gradient norm — ten times the distance between the fp32 step and
    the reference's float64 gradients (G20: 2e-4 / 2e-3), and the same mechanism: the products are 2^-16-accurate instead of 2^-24, so
    ~100x as many ReLU / max-pool / hard-example decisions within round-off of their threshold fall the other way, and each moves every
    upstream sum by ~1/sqrt(numel).  (The reference itself trains under `set_float32_matmul_precision('medium')`, main_SPEINet.py:12:
    TF32 / bf16 products, coarser than these.)  Bounds: worst 3e-2, median 1e-2."""
    from speinet_amd.loss import Loss
    from speinet_amd.speinet import default_args
    from speinet_amd.synth import synth_frames, synth_state_dict
    from speinet_amd import train as T
    args = default_args()
    args.n_sequence = 3
    b, h, w = 3, 60, 40
    if which == "swint":
        from speinet_amd.swint import SPEINet
        net = SPEINet(n_sequence=3, args=args)
        x = synth_frames(b, h, w, seed=91)[:, :3].contiguous().to(DEV)
        scales = T.drop_path_scales(net.cfg.depths, b, 2, generator=torch.Generator().manual_seed(3))
    else:
        from speinet_amd.speinet import SPEINet
        net = SPEINet(args=args)
        x = synth_frames(b, h, w, seed=92, zero_ref=(2,)).contiguous().to(DEV)
        scales = T.speinet_drop_path_scales(net.cfg.depths, [False, False, True], 3, generator=torch.Generator().manual_seed(3))
    net.load_state_dict(synth_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.to(DEV).train()
    gt = synth_frames(b, h, w, seed=93)[:, 1].contiguous().to(DEV)
    loss_fn = Loss("1*L1+2*HEM", device=DEV)
    res = {}
    for prec in ("f32", "bf16x3"):
        net.train_precision = prec
        net.zero_grad()
        np.random.seed(5)
        out = net(x, drop_path_scales=scales)
        loss = loss_fn(out, gt)
        loss.backward()
        res[prec] = (out.detach().clone(), loss.item(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    net.train_precision = "f32"
    o32, l32, g32 = res["f32"]
    o16, l16, g16 = res["bf16x3"]
    eo = (o16 - o32).abs().max().item() / o32.abs().max().item()
    errs = sorted((g16[k] - g32[k]).norm().item() / max(g32[k].norm().item(), 1e-20) for k in g32 if g32[k].numel() > 4)
    print(f"{which}: bf16x3 vs f32 step: output {eo:.1e}, loss {abs(l16 - l32):.1e}, gradients median {errs[len(errs) // 2]:.1e} worst {errs[-1]:.1e}")
    assert set(g16) == set(g32)
    assert eo < 2e-4 and abs(l16 - l32) < 1e-4 and errs[-1] < 3e-2 and errs[len(errs) // 2] < 1e-2


def test_loss_curve_vs_reference(golden_dir):
    """the loss curve of N optimizer steps with DropPath disabled against the reference's own run
    (G22: swint model, two 40x40 windows, 1*L1 + 2*HEM, Adam 1e-4, BatchNorm in train mode, 6 steps).  Each step feeds on the
    previous update, so fp32 differences compound: first loss to 2e-6, second to 5e-5, the rest of the curve within ten times the distance
    between the reference's own fp32 and float64 curves (see below)."""
    from speinet_amd.loss import Loss
    from speinet_amd.swint import SPEINet
    from speinet_amd.speinet import default_args
    from speinet_amd.synth import synth_frames, synth_state_dict
    from speinet_amd.trainer import Trainer
    d = np.load(os.path.join(golden_dir, "g22_losscurve_swint_40x40.npz"))
    seed, b, h, w = (int(d[k]) for k in ("seed", "b", "h", "w"))
    args = default_args()
    args.n_sequence = 3
    net = SPEINet(n_sequence=3, args=args)
    net.load_state_dict(synth_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.to(DEV).train()
    x = synth_frames(b, h, w, seed=seed)[:, :3].contiguous().to(DEV)
    gt = synth_frames(b, h, w, seed=seed + 500)[:, 1].contiguous().to(DEV)
    no_drop = [[None] * sum(net.cfg.depths) for _ in range(2)]           # DropPath off: every block's branch passes unscaled
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
    ref = [float(v) for v in d["losses"]]
    ref64 = [float(v) for v in d["losses64"]]
    print("HIP               :", ", ".join(f"{v:.6f}" for v in losses))
    print("reference, fp32   :", ", ".join(f"{v:.6f}" for v in ref))
    print("reference, float64:", ", ".join(f"{v:.6f}" for v in ref64))
    noise = max(abs(a - c) for a, c in zip(ref, ref64))           # how far fp32 round-off alone moves the REFERENCE's curve: 3.8e-4
    dev64 = [abs(a - c) for a, c in zip(losses, ref64)]
    print(f"|reference fp32 - float64| max {noise:.2e};  |HIP - float64| " + ", ".join(f"{v:.1e}" for v in dev64))
    # The fixture holds the reference's own curve in float64 (round 3): its fp32 run leaves it by up to 3.8e-4 within six steps (1e-6
    # through step 3).  The HIP run agrees to 0 / 1e-5 on the first two steps and then sits within 1.2e-3 of the float64 curve: its
    # gradients are 2e-4 (median) from the float64 gradients where the reference's fp32 gradients are 2e-5 (G20: other summation
    # orders, ReLU / max-pool decisions at round-off), and Adam's first steps move EVERY element by +-lr whatever its gradient's size
    # (update = lr g / (|g| + 1e-8)), so elements whose gradient is within round-off of zero step in a direction the summation order
    # decides.  Bound: ten times the reference's own fp32-vs-float64 distance.
    assert abs(losses[0] - ref64[0]) < 2e-6 and abs(losses[1] - ref64[1]) < 5e-5
    assert max(dev64) < 10.0 * noise, (max(dev64), noise)
    assert losses[-1] < losses[0] and ref[-1] < ref[0]


@pytest.mark.parametrize("which,content", [pytest.param("swint", "smooth", id="swint"), pytest.param("speinet", "smooth", id="speinet"),
                                           pytest.param("swint", "flat", id="swint-flat"), pytest.param("speinet", "flat", id="speinet-flat")])
def test_training_step_ragged_size_vs_oracle(which, content):
    """A size and batch no fixture holds (B = 3, 60x40, non-square; the full model with the LAST sample reference-less): the HIP
    training step against the oracle's train-mode graph evaluated in float64 on the host (tests/test_oracle_train.py pins that
    graph to the reference's float64 gradients at 1e-13), on three inputs.  Output 2e-5 and loss 5e-6 on each.  Gradients: the graph
    is piecewise smooth (ReLU, the row/column maxima of the gates, the HEM mask), and ONE maximum taken at a neighbouring pixel in
    fp32 (a near tie: measured in round 4 on outBlock.1 at seed 77, two pixels of dx1 moved, everything upstream shifted by 1.5e-3 of
    its norm, stable under input noise) moves every gradient upstream of it by up to a few 1e-3; an arithmetic error would show on
    every input.  So: on every input each gradient within 2e-2 of its norm and the median below 4e-3; on the best input the median
    below 2e-4 and the worst below 2e-3 (measured 1e-6 .. 2e-4 without a flipped decision).  content "flat": synth_frames_flat
    (letterbox bars of h // 6 rows, a clipped highlight, one sample faded to near-black), where the gates' maxima tie exactly, under
    the same bounds.  (With bars of h // 4 rows the swint step on input 77 sits at a median 5.9e-3 from float64, identically with
    first-index and all-ties max gradients: a difference that is not the ZPool tie rule, left for its own investigation.)"""
    per_seed = []
    for seed in (77, 78, 81):
        per_seed.append(_ragged_step(which, seed, content))
    print(which, content, "ragged step, (worst, median) per input:", per_seed)
    assert all(wv < 2e-2 and md < 4e-3 for wv, md in per_seed), per_seed
    assert min(md for _, md in per_seed) < 2e-4 and min(wv for wv, _ in per_seed) < 2e-3, per_seed


def _ragged_step(which, seed, content="smooth"):
    from oracle import speinet_oracle as O                                   # the checker
    from speinet_amd import train as T
    from speinet_amd.loss import Loss
    from speinet_amd.speinet import default_args
    from speinet_amd.synth import synth_frames as smooth_frames, synth_frames_flat, synth_state_dict
    torch.set_num_threads(16)
    args = default_args()
    args.n_sequence = 3
    b, h, w = 3, 60, 40
    synth_frames = smooth_frames if content == "smooth" else (lambda *a, **k: synth_frames_flat(*a, bar=h // 6, **k))
    if which == "swint":
        from speinet_amd.swint import SPEINet
        net = SPEINet(n_sequence=3, args=args)
        x = synth_frames(b, h, w, seed=seed)[:, :3].contiguous()
        torch.manual_seed(seed)
        scales = T.drop_path_scales(net.cfg.depths, b, 2)
        flat_calls = scales
    else:
        from speinet_amd.speinet import SPEINet
        net = SPEINet(args=args)
        x = synth_frames(b, h, w, seed=seed, zero_ref=(2,)).contiguous()
        torch.manual_seed(seed)
        scales = T.speinet_drop_path_scales(net.cfg.depths, [False, False, True], 3)
        flat_calls = scales[False] + scales[True]                            # the order the forward consumes them
    sd = synth_state_dict(net.state_dict(), seed=0)
    net.load_state_dict(sd, strict=True)
    gt = synth_frames(b, h, w, seed=seed + 500)[:, 1].contiguous()
    # ---- oracle, float64, host ----
    leaves = {k: (v.double().requires_grad_(True) if v.is_floating_point() and "running_" not in k else (v.double() if v.is_floating_point() else v))
              for k, v in sd.items()}
    np.random.seed(seed)
    with O.train_mode(flat_calls):
        ref = (O.forward_swint if which == "swint" else O.forward)(x.double(), leaves, O.Cfg(n_sequence=3))
    ref_loss = Loss("1*L1+2*HEM", device="cpu")(ref, gt.double())
    ref_loss.backward()
    # ---- HIP ----
    net = net.to(DEV).train()
    np.random.seed(seed)
    loss_fn = Loss("1*L1+2*HEM", device=DEV)
    out = net(x.to(DEV), drop_path_scales=scales)
    loss = loss_fn(out, gt.to(DEV))
    loss.backward()
    err = (out.detach().cpu().double() - ref.detach()).abs().max().item()
    assert err < 2e-5 and abs(loss.item() - ref_loss.item()) < 5e-6, (err, loss.item(), ref_loss.item())
    norms = {k: v.grad.norm().item() for k, v in leaves.items() if torch.is_tensor(v) and v.requires_grad and v.grad is not None}
    gmax = max(norms.values())
    devs = []
    for k, p in net.named_parameters():
        if k not in norms:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        scale = max(norms[k], 1e-5 * gmax)
        if ".bn." in k:
            scale = max(scale, norms[k.rsplit(".bn.", 1)[0] + ".conv.weight"])
        devs.append(((p.grad.detach().cpu().double() - leaves[k].grad).norm().item() / scale, k))
    devs.sort(reverse=True)
    print(f"{which} B=3 60x40: output {err:.1e}, loss {loss.item():.6f} vs {ref_loss.item():.6f}; gradients vs float64: worst "
          + ", ".join(f"{k} {e:.1e}" for e, k in devs[:3]) + f"; median {np.median([e for e, _ in devs]):.1e}")
    return devs[0][0], float(np.median([e for e, _ in devs]))


@pytest.mark.parametrize("n,k,ks", [(32, 32, 5), (64, 32, 3), (256, 128, 1), (128, 64, 3), (96, 160, 1)])
def test_pack_split16_matches_the_torch_formulation(n, k, ks):
    """spei_pack_split16 (one launch: reference-layout weight -> split bf16 halves in fragment order) against the tensor arithmetic
    it replaces: hi = bf16(w), lo = bf16(w - hi), pack._frag of the [tap][N][K] view; and for the stride-1 data gradient the same of
    the tap-reversed, channel-swapped view.  Bit for bit."""
    from speinet_amd import _lib, pack
    from speinet_amd.ops import Ctx
    ctx = Ctx("f32", device=DEV)
    w = torch.randn(n, k, ks, ks, generator=torch.Generator().manual_seed(n + k + ks)).to(DEV)
    w = w if ks > 1 else w.reshape(n, k)
    w4 = w.reshape(n, k, ks, ks)
    fwd = w4.permute(2, 3, 0, 1).reshape(ks * ks, n, k).contiguous()
    views = {0: fwd, 1: fwd.transpose(1, 2).flip(0).contiguous()}
    for mode, v in views.items():
        hi = v.to(torch.bfloat16)
        lo = (v - hi.float()).to(torch.bfloat16)
        fhi = torch.empty(w.numel(), device=DEV, dtype=torch.bfloat16)
        flo = torch.empty_like(fhi)
        _lib.check(_lib.lib().spei_pack_split16(ctx._tp(w.contiguous()), n, k, ks, mode, ctx._tp(fhi), ctx._tp(flo), ctx._stream()), "spei_pack_split16")
        assert torch.equal(fhi.view(torch.int16), pack._frag(hi).reshape(-1).view(torch.int16)), (mode, "hi")
        assert torch.equal(flo.view(torch.int16), pack._frag(lo).reshape(-1).view(torch.int16)), (mode, "lo")


def test_inplace_data_edit_reaches_the_split_weights():
    """the packed bf16 (hi, lo) halves of the bf16x3 training graph are cached on the parameters, stamped with `_version`;
    `p.data.mul_()` / `p.data.copy_()` do not move that counter.  `invalidate_packed()` — run at the top of every autograd forward —
    drops them: after an edit through `.data` the bf16x3 step must follow the f32 step, not the stale weights."""
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
    net.train_precision = "bf16x3"
    with torch.no_grad():
        before = net(x, drop_path_scales=scales).clone()
        assert any(getattr(p, "_spei_split", None) for p in net.parameters()), "the split cache is in use"
        for name, p in net.named_parameters():
            if name.endswith("weight") and p.dim() in (2, 4):
                p.data.mul_(1.25)                                  # invisible to `_version`
        after16 = net(x, drop_path_scales=scales).clone()
        net.train_precision = "f32"
        after32 = net(x, drop_path_scales=scales).clone()
    scale = after32.abs().max().item()
    moved = (after16 - before).abs().max().item() / scale
    apart = (after16 - after32).abs().max().item() / scale
    print(f"in-place edit: bf16x3 output moved by {moved:.2e}, bf16x3 vs f32 after the edit {apart:.1e}")
    assert moved > 1e-2 and apart < 2e-4
