"""Training step, first slice: HIP forward + backward of the recons_net encoder stack through
speinet_amd.train (the one set of autograd Functions the product ships), against (a) torch.autograd of the same op in fp64 on the CPU, per op, and (b) the REFERENCE's own
gradients (tests/golden/make_golden_grad.py, G19: its modules, its autograd) for every parameter of inBlock /
encoder_first / encoder_second.  Tolerances are fp32 round-off of re-ordered sums relative to the gradient's norm."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from speinet_amd import train as T                       # noqa: E402
from speinet_amd.speinet import SPEINet, default_args    # noqa: E402
from speinet_amd.synth import synth_frames               # noqa: E402

DEV = "cuda:0"


def rnd(seed, *shape, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).randn(*shape) * scale).astype(np.float32))


def rows(x):          # [1,C,H,W] -> [H*W, C]
    return x[0].permute(1, 2, 0).reshape(-1, x.shape[1]).contiguous()


def rel(a, b):
    return (a.detach().cpu().double() - b.double()).norm().item() / max(b.double().norm().item(), 1e-30)


import contextlib


@contextlib.contextmanager
def train_prec(prec):
    """The arithmetic the training graph's GEMMs are built in (train._PREC: read when a Function's forward runs, kept for its backward)."""
    tok = T._PREC.set(prec)
    try:
        yield
    finally:
        T._PREC.reset(tok)


# bf16x3 (split products on the 16-bit pipe: each operand carried as hi + lo bf16, 16 significant bits, fp32 accumulation): a dropped
# tap, edge segment or bias partial is an O(1/taps) error, five orders above these bounds
TOL = {"f32": (1e-5, 2e-5), "bf16x3": (3e-5, 1e-4)}

CONV_CASES = [(32, 32, 5, 1, 20, 24, True, 1), (64, 64, 5, 1, 13, 17, False, 1), (32, 64, 5, 2, 40, 60, True, 1),
              (64, 128, 5, 2, 22, 18, True, 1), (128, 128, 5, 1, 10, 15, False, 1), (64, 32, 3, 1, 21, 19, False, 1),
              (128, 64, 1, 1, 9, 11, True, 1),
              # batch > 1 (blockIdx.z / .y = sample), Wout not a multiple of 16, k = 1 / 3 / 5, stride 2 on odd sizes
              (32, 32, 5, 1, 11, 23, True, 3), (64, 64, 3, 1, 7, 37, False, 2), (256, 256, 1, 1, 5, 25, False, 2),
              (32, 64, 5, 2, 21, 27, True, 2), (128, 128, 5, 1, 6, 50, True, 2), (32, 32, 3, 1, 9, 33, True, 2)]


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("cin,cout,k,stride,h,w,relu,batch", CONV_CASES)
def test_conv_forward_backward(cin, cout, k, stride, h, w, relu, batch, prec):
    """Forward, data, weight and bias gradients against float64 autograd.  With a ReLU the float64 backward uses the mask the HIP
    forward produced: an output within round-off of zero may fall on the other side there (one such element in 10^5 moves a
    gradient by 1/sqrt(numel) — seen at 9e-3 in bf16x3, whose products are 2^-16-accurate), which says nothing about the
    gradient kernels under test."""
    x, wt, b = rnd(1, batch, cin, h, w), rnd(2, cout, cin, k, k, scale=1.0 / np.sqrt(cin * k * k)), rnd(3, cout, scale=0.1)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, wt, b))
    y_lin = F.conv2d(xd, wd, bd, stride=stride, padding=k // 2)
    y = F.relu(y_lin) if relu else y_lin
    g = rnd(4, *y.shape)
    brows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()
    xg = brows(x).to(DEV).requires_grad_(True)
    wg, bg = wt.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    tf, tb = TOL[prec]
    with train_prec(prec):
        out = T._Conv2d.apply(xg, wg, bg, None, batch, h, w, k, stride, relu)
    assert rel(out, brows(y.detach().float())) < tf
    gd = g.double()
    if relu:
        mask = (out.detach().cpu() > 0).view(batch, y.shape[2], y.shape[3], cout).permute(0, 3, 1, 2)
        flips = int((mask != (y_lin.detach() > 0)).sum())
        assert flips <= max(2, y.numel() // 20000), f"{flips} ReLU decisions differ from float64"
        gd = gd * mask
    y_lin.backward(gd)
    out.backward(brows(g).to(DEV))
    assert rel(xg.grad, brows(xd.grad.float())) < tb, "data gradient"
    assert rel(wg.grad, wd.grad.float()) < tb, "weight gradient"
    assert rel(bg.grad, bd.grad.float()) < tb, "bias gradient"


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("m,k,n", [(50, 256, 512), (137, 512, 256), (75, 256, 256)])
def test_linear_forward_backward(m, k, n, prec):
    """`train._Linear` (the Swin linears: 1x1 GEMMs over token rows) against float64 autograd in both arithmetics."""
    x, wt, b = rnd(31, m, k), rnd(32, n, k, scale=1.0 / np.sqrt(k)), rnd(33, n, scale=0.1)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, wt, b))
    y = F.linear(xd, wd, bd)
    g = rnd(34, m, n)
    y.backward(g.double())
    xg, wg, bg = x.to(DEV).requires_grad_(True), wt.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    tf, tb = TOL[prec]
    with train_prec(prec):
        out = T._Linear.apply(xg, wg, bg, None, None)
    assert rel(out, y.detach().float()) < tf
    out.backward(g.to(DEV))
    assert rel(xg.grad, xd.grad.float()) < tb and rel(wg.grad, wd.grad.float()) < tb and rel(bg.grad, bd.grad.float()) < tb


def test_conv_in_backward():
    x, wt, b = torch.rand(3, 28, 36), rnd(5, 32, 3, 5, 5, scale=0.1), rnd(6, 32, scale=0.1)
    wd, bd = wt.double().requires_grad_(True), b.double().requires_grad_(True)
    y = F.relu(F.conv2d(x[None].double(), wd, bd, padding=2))
    g = rnd(7, *y.shape)
    y.backward(g.double())
    wg, bg = wt.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    out = T._ConvIn.apply(x.to(DEV)[None], wg, bg)
    assert rel(out, rows(y.detach().float())) < 1e-5
    out.backward(rows(g).to(DEV))
    assert rel(wg.grad, wd.grad.float()) < 2e-5 and rel(bg.grad, bd.grad.float()) < 2e-5


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("c,h,w", [(32, 20, 24), (64, 33, 17), (128, 10, 45)])
def test_resblock_backward_vs_torch(synth_sd, c, h, w, prec):
    """One ResBlock (conv-relu-conv, SE + triplet gates, skip) forward and backward against a plain-torch fp64 statement of
    model/block.py:127-140 with the same parameters: output, data gradient and every parameter gradient."""
    net = SPEINet(args=default_args())
    net.load_state_dict(synth_sd, strict=True)
    stage = {32: net.recons_net.inBlock, 64: net.recons_net.encoder_first, 128: net.recons_net.encoder_second}[c]
    blk = stage[2].to(DEV)
    x = rnd(10 + c, 1, c, h, w)
    # torch fp64 statement
    ref = SPEINet(args=default_args())
    ref.load_state_dict(synth_sd, strict=True)
    rb = {32: ref.recons_net.inBlock, 64: ref.recons_net.encoder_first, 128: ref.recons_net.encoder_second}[c][2].double().eval()
    xd = x.double().requires_grad_(True)
    x1 = rb.main[1].main[0](F.relu(rb.main[0].main[0](xd)))
    y = rb.se.fc(x1.mean(dim=(2, 3))).view(1, c, 1, 1)
    xp = x1.permute(0, 3, 2, 1)
    z = torch.cat((xp.max(dim=1)[0].unsqueeze(1), xp.mean(dim=1).unsqueeze(1)), dim=1)
    g1 = rb.te.cw.conv.bn(rb.te.cw.conv.conv(z)).permute(0, 3, 2, 1)
    xp = x1.permute(0, 2, 1, 3)
    z = torch.cat((xp.max(dim=1)[0].unsqueeze(1), xp.mean(dim=1).unsqueeze(1)), dim=1)
    g2 = rb.te.hc.conv.bn(rb.te.hc.conv.conv(z)).permute(0, 2, 1, 3)
    out_ref = xd + x1 * (y + g1 + g2)
    g = rnd(20 + c, *out_ref.shape)
    out_ref.backward(g.double())
    # HIP
    xg = rows(x).to(DEV).requires_grad_(True)
    with train_prec(prec):
        out = T.resblock(xg, blk, 1, h, w, False)       # eval-mode gates: BatchNorm(1) on its running statistics
    # split products carry 2^-16 per operand instead of 2^-24: ~100x as many ReLU / max-pool decisions fall within round-off of their
    # threshold, and ONE that falls the other way moves a gradient by ~1/sqrt(numel) (4.9e-4 seen on the 128-channel case): the
    # bf16x3 bounds leave room for a few of those — a dropped tap or edge segment is still 10x above them (the per-kernel bounds of
    # test_conv_forward_backward, where the float64 side takes the HIP forward's ReLU mask, are the tight ones)
    fo, fd, fp = (1.0, 1.0, 1.0) if prec == "f32" else (4.0, 40.0, 40.0)
    assert rel(out, rows(out_ref.detach().float())) < 1e-5 * fo
    out.backward(rows(g).to(DEV))
    assert rel(xg.grad, rows(xd.grad.float())) < 5e-5 * fd, "data gradient"
    refp = dict(rb.named_parameters())
    for k, p in blk.named_parameters():
        assert p.grad is not None, k
        assert rel(p.grad, refp[k].grad.float()) < 1e-4 * fp, k


# ---- the gate maps of a ResBlock (csrc/gates_train.hip) against their torch statement in float64 -------------------------------------
def gate_maps_torch(rowmax, rowmean, colmax, colmean, mean, prm, bn_train: bool, update_running: bool):
    """s [B,C], g1 [B,H,C], g2 [B,W,C] from the plane statistics (model/block.py:8-24 SE, :75-96 the two gates without their
    sigmoid, :49-68 BasicConv1 = 2->1 conv + BatchNorm2d(1); TripletAttention sums the gates, :116-119).  prm: se_w1, se_b1, se_w2,
    se_b2, cw_w, cw_bn_w, cw_bn_b, cw_rm, cw_rv, hc_w, hc_bn_w, hc_bn_b, hc_rm, hc_rv.  bn_train: normalise with the batch
    statistics; update_running: also move the running buffers (momentum 0.01), as nn.BatchNorm2d.forward does in train()."""
    se_w1, se_b1, se_w2, se_b2, cw_w, cw_g, cw_b, cw_rm, cw_rv, hc_w, hc_g, hc_b, hc_rm, hc_rv = prm
    s = torch.sigmoid(F.linear(F.relu(F.linear(mean, se_w1, se_b1)), se_w2, se_b2))

    def bn(t, g, b, rm, rv):
        # nn.BatchNorm2d(1, eps 1e-5, momentum 0.01) written out (plain tensor arithmetic: no library batch-norm kernels to
        # compile per shape): train() normalises with the biased batch variance and moves the buffers with the unbiased one
        if not bn_train:
            return (t - rm) / torch.sqrt(rv + 1e-5) * g + b
        mean = t.mean()
        var = ((t - mean) ** 2).mean()
        if update_running:
            with torch.no_grad():
                n = t.numel()
                rm.mul_(1.0 - 0.01).add_(0.01 * mean)
                rv.mul_(1.0 - 0.01).add_(0.01 * var * (n / max(n - 1, 1)))
        return (t - mean) / torch.sqrt(var + 1e-5) * g + b

    def conv21(z, w, k):
        # the 2 -> 1 channel k x k convolution as unfold + one matrix product: the library convolution's weight gradient is not
        # bitwise reproducible for these shapes (atomics), this form is
        # torch's im2col runs one launch per batch element (60 maps per ResBlock at batch 20: 2 900 launches per step): the batch is laid out
        # as ONE tall map, each sample between its own zero rows, so the whole batch is one unfold and one product
        bsz, _, a, b = z.shape
        pd = k // 2
        tall = F.pad(z, (0, 0, pd, pd)).permute(1, 0, 2, 3).reshape(1, 2, bsz * (a + 2 * pd), b)
        cols = F.unfold(tall, k, padding=(0, pd))                              # [1, 2 k k, (bsz (a + 2 pd) - k + 1) * b]
        out = (w.reshape(1, -1) @ cols).view(bsz * (a + 2 * pd) - 2 * pd, b)
        out = F.pad(out, (0, 0, 0, 2 * pd)).view(bsz, a + 2 * pd, b)[:, :a]     # row r of sample i sits at i (a + 2 pd) + r
        return out.reshape(bsz, 1, a, b)

    z1 = torch.stack((rowmax, rowmean), dim=1)                              # [B, 2, H, C]: conv "height" = H, "width" = C
    g1 = bn(conv21(z1, cw_w, 7), cw_g, cw_b, cw_rm, cw_rv)[:, 0]            # [B, H, C]
    z2 = torch.stack((colmax.transpose(1, 2), colmean.transpose(1, 2)), dim=1)   # [B, 2, C, W]: conv "height" = C, "width" = W
    g2 = bn(conv21(z2, hc_w, 5), hc_g, hc_b, hc_rm, hc_rv)[:, 0].transpose(1, 2)  # [B, W, C]
    return s.contiguous(), g1.contiguous(), g2.contiguous()


@pytest.mark.parametrize("bn_train", [True, False])
@pytest.mark.parametrize("c,h,w,b,groups", [(32, 20, 24, 2, 1), (64, 13, 17, 3, 1), (128, 10, 15, 1, 1), (32, 9, 31, 6, 3), (64, 12, 8, 4, 2),
                                            (32, 60, 40, 3, 1), (64, 30, 20, 3, 1), (128, 15, 10, 3, 1), (32, 200, 200, 4, 2)])
def test_gate_maps_fwd_bwd_vs_torch(c, h, w, b, groups, bn_train):
    """spei_gate_maps_fwd / _bwd (SE MLP, the two 2 -> 1 channel convolutions, BatchNorm2d(1) on batch or running statistics; per
    group of samples) against torch.autograd of the same formulas in float64 — round 3's implementation of this glue, kept here as
    the oracle: outputs, the gradients of the five statistics and of the ten parameters, and the running buffers after the call."""
    import ctypes as C
    from speinet_amd import _lib
    g = torch.Generator().manual_seed(c * 100 + h)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    stats = [rn(b, h, c), rn(b, h, c), rn(b, w, c), rn(b, w, c), rn(b, c)]
    r = c // 4
    prm = [rn(r, c, sc=0.2), rn(r, sc=0.1), rn(c, r, sc=0.3), rn(c, sc=0.1), rn(1, 2, 7, 7, sc=0.15), rn(1).abs() + 0.5, rn(1, sc=0.1),
           rn(1, sc=0.1), rn(1).abs() + 0.7, rn(1, 2, 5, 5, sc=0.2), rn(1).abs() + 0.5, rn(1, sc=0.1), rn(1, sc=0.1), rn(1).abs() + 0.6]
    douts = [rn(b, c), rn(b, h, c), rn(b, w, c)]
    # float64 oracle, group by group (the statistics of BatchNorm are per group; the running buffers move once per group, in order)
    st64 = [t.double().requires_grad_(True) for t in stats]
    p64 = [t.double().requires_grad_(t.is_floating_point() and i not in (7, 8, 12, 13)) for i, t in enumerate(prm)]
    bs = b // groups
    outs = [[], [], []]
    for gi in range(groups):
        sl = slice(gi * bs, (gi + 1) * bs)
        o = gate_maps_torch(*[t[sl] for t in st64], p64, bn_train, update_running=bn_train)
        for k in range(3):
            outs[k].append(o[k])
    outs = [torch.cat(o) for o in outs]
    leaves = st64 + [t for t in p64 if t.requires_grad]
    grads = torch.autograd.grad(outs, leaves, [t.double() for t in douts])
    # HIP
    ctx = T._ctx(torch.device(DEV))
    lib = _lib.lib()
    dv = lambda t: t.float().contiguous().to(DEV)
    sd, pd, dd = [dv(t) for t in stats], [dv(t) for t in prm], [dv(t) for t in douts]
    prm_p, run_p, keep = T._gate_ptrs(ctx, pd)
    s_, g1, g2 = torch.empty(b, c, device=DEV), torch.empty(b, h, c, device=DEV), torch.empty(b, w, c, device=DEV)
    saved = torch.empty(lib.spei_gate_train_saved_floats(b, groups, h, w, c), device=DEV)
    ws = torch.empty(lib.spei_gate_train_ws_floats(b, groups, h, w, c) // 2 + 1, device=DEV, dtype=torch.float64)
    P = lambda t: T._p(ctx, t)
    with torch.cuda.device(DEV):
        _lib.check(lib.spei_gate_maps_fwd(*[P(t) for t in sd], prm_p, run_p, b, groups, h, w, c, int(bn_train), int(bn_train), P(s_), P(g1), P(g2),
                                          P(saved), C.c_void_p(ws.data_ptr()), ctx._stream()), "fwd")
        for got, ref, nm in zip((s_, g1, g2), outs, ("s", "g1", "g2")):
            assert rel(got, ref.detach().float()) < 2e-6, nm
        for i in (7, 8, 12, 13):                                     # running buffers: moved (train) or untouched (eval)
            assert (keep[i].cpu() - p64[i].detach().float()).abs().max().item() < 1e-6, i
        d_stats = [torch.empty_like(t) for t in sd]
        dprm = torch.empty(lib.spei_gate_train_nparams(c), device=DEV)
        _lib.check(lib.spei_gate_maps_bwd(*[P(t) for t in sd], prm_p, run_p, b, groups, h, w, c, int(bn_train), P(s_), P(saved), *[P(t) for t in dd],
                                          *[P(t) for t in d_stats], P(dprm), C.c_void_p(ws.data_ptr()), ctx._stream()), "bwd")
    for got, ref, nm in zip(d_stats, grads[:5], ("d_rowmax", "d_rowmean", "d_colmax", "d_colmean", "d_mean")):
        assert rel(got, ref.float()) < 5e-6, nm
    sizes = (r * c, r, c * r, c, 98, 1, 1, 50, 1, 1)
    names = ("se_w1", "se_b1", "se_w2", "se_b2", "cw_w", "cw_g", "cw_b", "hc_w", "hc_g", "hc_b")
    for got, ref, nm in zip(torch.split(dprm, sizes), grads[5:], names):
        scale = max(ref.norm().item(), 1e-3 * max(gq.norm().item() for gq in grads[5:]))
        assert (got.cpu().double() - ref.reshape(-1)).norm().item() / scale < 2e-5, nm


@pytest.mark.parametrize("name,h,w", [("g19_enc_grad_40x60", 40, 60), ("g19_enc_grad_100x100", 100, 100)])
def test_encoder_gradients_vs_reference(golden_dir, synth_sd, name, h, w):
    """Every parameter gradient of the three encoder stages against the reference's own autograd (G19): L2 norm and a strided
    sample of each gradient; bitwise reproducible from run to run (fixed-order reductions)."""
    d = np.load(os.path.join(golden_dir, name + ".npz"))
    seed = int(d["seed"])
    net = SPEINet(args=default_args())
    net.load_state_dict(synth_sd, strict=True)
    net = net.to(DEV)
    x = synth_frames(1, h, w, seed=seed)[0, 1].to(DEV)

    def run():
        net.zero_grad()
        lv1, lv2, lv3 = T.encoder(x[None], net.recons_net, False, pyramid=True)
        g = torch.Generator().manual_seed(seed + 1000)
        r1, r2, r3 = (torch.randn(*s, generator=g) for s in ((1, 32, h, w), (1, 64, h // 2, w // 2), (1, 128, h // 4, w // 4)))
        loss = (lv3 * rows(r3).to(DEV)).sum() + 0.5 * (lv2 * rows(r2).to(DEV)).sum() + 0.25 * (lv1 * rows(r1).to(DEV)).sum()
        loss.backward()
        return loss.item(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}

    loss, grads = run()
    assert abs(loss - float(d["loss"])) < 1e-3 * max(1.0, abs(float(d["loss"])))
    keys = [k[5:] for k in d.files if k.startswith("norm/")]
    assert len(keys) == 132 and set(keys) == set(grads), set(keys) ^ set(grads)
    worst, errs = 0.0, []
    for k in keys:
        g = grads[k].cpu().reshape(-1)
        n_ref = float(d["norm/" + k])
        sub = torch.from_numpy(d["sub/" + k])
        e_norm = abs(g.norm().item() - n_ref) / max(n_ref, 1e-12)
        # the sample's error is measured against the gradient's typical magnitude (norm / sqrt(numel) per element), not against the
        # sampled elements' own size: a single sampled element can be a near-cancelling sum
        e_sub = (g[::61] - sub).norm().item() / max(sub.norm().item(), n_ref * (sub.numel() / g.numel()) ** 0.5, 1e-12)
        if g.numel() > 4:
            worst = max(worst, e_norm, e_sub)
            errs.append((max(e_norm, e_sub), k))
        if g.numel() <= 4:
            # a one-number gradient (the BatchNorm(1) affine of a gate) is a sum of ~10^4 signed terms that can cancel to 1e-3 of
            # their size (values from 0.04 to 44 across blocks): its error is measured against the gradient norm of the SAME gate's
            # convolution weight (sums of the same terms), not against its own, possibly near-cancelled, value
            scale = max(n_ref, float(d["norm/" + k.rsplit(".bn.", 1)[0] + ".conv.weight"]))
            assert abs(g.norm().item() - n_ref) < 2e-3 * scale, (k, g.norm().item(), n_ref, scale)
            continue
        # 100x100: every gradient within 4e-6.  40x60: a uniform ~4e-4 on ALL 132 gradients at once — the signature of ONE ReLU /
        # arg-max decision on an element within fp32 round-off of its threshold resolving differently from the CPU's summation
        # order (one element of 76 800 moves every downstream sum by ~1/sqrt(numel)), not of an arithmetic difference
        assert e_norm < 2e-3 and e_sub < 2e-3, (k, e_norm, e_sub)
    print(f"{name}: 132 parameter gradients, worst relative deviation from the reference {worst:.1e}; largest: "
          + ", ".join(f"{k[11:]} {e:.1e}" for e, k in sorted(errs, reverse=True)[:6]))
    loss2, grads2 = run()
    assert loss2 == loss and all(torch.equal(grads[k], grads2[k]) for k in grads), "gradients are not bitwise reproducible"


# ---- ZPool ties: the gated sum's backward on planes with exact ties at the row / column maxima ---------------------------------------
# torch.max(dim) hands the gradient of a maximum to ONE element, the first maximal index (lowest x of a row, lowest y of a column);
# flat content (letterbox bars, clipped highlights, fades to black) gives x1 planes with many bit-identical maxima.
def _tie_planes(b, h, w, c, seed):
    """x1 [b, h, w, c] float32 with exact ties built in, channel pattern (c + sample) % 8: 0 whole constant rows (k = W, and ties down
    the columns), 1 whole constant columns (k = H), 2 a constant rectangle above everything else (row AND column maxima), 3 the same
    rectangle below everything (ties, none at a maximum), 4 two equal row maxima at xa < xb (different 16-wide tiles when W > 70),
    5 equal row maxima at x = 0 and x = W-1, 6 two equal column maxima at ya < yb, 7 at y = 0 and y = H-1.  Channels with
    (c // 8) odd are shifted by -20: all-negative planes with the same ties.  Returns x1 and the checks (pattern -> mask of the
    lines that must hold a tie at their maximum)."""
    r = np.random.RandomState(seed)
    x1 = r.randn(b, h, w, c).astype(np.float32)
    xa, xb = (10, 70) if w > 70 else (1, w - 3)
    ya, yb = (10, 70) if h > 70 else (1, h - 3)
    r0, r1, q0, q1 = h // 4, max(h // 2, h // 4 + 2), w // 3, max(2 * w // 3, w // 3 + 2)
    for bi in range(b):
        for ch in range(c):
            p = x1[bi, :, :, ch]
            k = (ch + bi) % 8
            if k == 0:
                p[1::4, :] = 6.0
            elif k == 1:
                p[:, 2::5] = 6.0
            elif k == 2:
                p[r0:r1, q0:q1] = 6.0
            elif k == 3:
                p[r0:r1, q0:q1] = -6.0
            elif k in (4, 5):
                m = (6.0 + r.rand(h)).astype(np.float32)
                p[:, xa if k == 4 else 0] = m
                p[:, xb if k == 4 else w - 1] = m
            else:
                m = (6.0 + r.rand(w)).astype(np.float32)
                p[ya if k == 6 else 0, :] = m
                p[yb if k == 6 else h - 1, :] = m
            if (ch // 8) % 2 == 1:
                p -= np.float32(20.0)
    return torch.from_numpy(x1), (xa, xb, ya, yb)


def _assert_ties(x1, pos):
    """Every constructed tie is present in x1 (so the test cannot pass on planes without them): per pattern, the lines whose maximum
    is shared."""
    b, h, w, c = x1.shape
    xa, xb, ya, yb = pos
    rmax, cmax = x1.amax(dim=2), x1.amax(dim=1)                   # [b, h, c], [b, w, c]
    rk, ck = (x1 == rmax[:, :, None]).sum(2), (x1 == cmax[:, None]).sum(1)   # number of maxima per row / per column
    n = 0
    for bi in range(b):
        for ch in range(c):
            k = (ch + bi) % 8
            if k == 0:
                assert (rk[bi, 1::4, ch] == w).all() and (ck[bi, :, ch] == len(range(1, h, 4))).all(), (bi, ch)
            elif k == 1:
                assert (ck[bi, 2::5, ch] == h).all() and (rk[bi, :, ch] == len(range(2, w, 5))).all(), (bi, ch)
            elif k == 2:
                r0, r1, q0, q1 = h // 4, max(h // 2, h // 4 + 2), w // 3, max(2 * w // 3, w // 3 + 2)
                assert (rk[bi, r0:r1, ch] == q1 - q0).all() and (ck[bi, q0:q1, ch] == r1 - r0).all(), (bi, ch)
            elif k == 3:
                assert (rk[bi, :, ch] == 1).all() and (ck[bi, :, ch] == 1).all(), (bi, ch)
            elif k in (4, 5):
                a, z = (xa, xb) if k == 4 else (0, w - 1)
                assert (x1[bi, :, a, ch] == rmax[bi, :, ch]).all() and (x1[bi, :, z, ch] == rmax[bi, :, ch]).all() and (rk[bi, :, ch] == 2).all()
            else:
                a, z = (ya, yb) if k == 6 else (0, h - 1)
                assert (x1[bi, a, :, ch] == cmax[bi, :, ch]).all() and (x1[bi, z, :, ch] == cmax[bi, :, ch]).all() and (ck[bi, :, ch] == 2).all()
            n += 1
    assert n == b * c and (x1[..., 8:16] < 0).all()
    return int((rk > 1).sum()), int((ck > 1).sum())


def _gate_params(c, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    r = c // 4
    return [rn(r, c, sc=0.2), rn(r, sc=0.1), rn(c, r, sc=0.3), rn(c, sc=0.1), rn(1, 2, 7, 7, sc=0.15), rn(1).abs() + 0.5, rn(1, sc=0.1),
            rn(1, sc=0.1), rn(1).abs() + 0.7, rn(1, 2, 5, 5, sc=0.2), rn(1).abs() + 0.5, rn(1, sc=0.1), rn(1, sc=0.1), rn(1).abs() + 0.6]


def _gated_sum_torch(x, x1, prm, groups, bn_train):
    """float64 statement of the gated sum on [B, H, W, C] maps: ZPool by torch.max(dim)[0] (first maximal index gets the gradient)."""
    stats = [x1.max(dim=2)[0], x1.mean(dim=2), x1.max(dim=1)[0], x1.mean(dim=1), x1.mean(dim=(1, 2))]
    bs = x1.shape[0] // groups
    outs = [[], [], []]
    for gi in range(groups):
        sl = slice(gi * bs, (gi + 1) * bs)
        o = gate_maps_torch(*[t[sl] for t in stats], prm, bn_train, update_running=bn_train)
        for k in range(3):
            outs[k].append(o[k])
    s, g1, g2 = (torch.cat(o) for o in outs)
    return x + x1 * (s[:, None, None, :] + g1[:, :, None, :] + g2[:, None, :, :]), stats, (s, g1, g2)


TIE_CASES = [(32, 37, 130, 2, 1), (64, 130, 23, 3, 1), (128, 19, 29, 4, 2), (32, 200, 200, 2, 1), (64, 45, 75, 6, 3), (128, 75, 130, 2, 2)]


@pytest.mark.parametrize("bn_train", [True, False])
@pytest.mark.parametrize("c,h,w,b,groups", TIE_CASES)
def test_gated_sum_backward_with_tied_maxima(c, h, w, b, groups, bn_train):
    """train._GatedSum (spei_plane_stats_batched -> spei_gate_maps_fwd / _bwd -> spei_resblock_apply_bwd_batched) on x1 planes with
    exact ties at the row and column maxima (_tie_planes), x1 a leaf so both sides see the same values and the same ties: output,
    dx, dx1, every gate-parameter gradient and the running buffers against float64 autograd of the reference's statement, whose
    ZPool is torch.max(dim)[0].  The gradient of a tied maximum belongs to the FIRST maximal element; handing it to every tied
    element multiplies it by the number of ties (W on a constant row)."""
    x1, pos = _tie_planes(b, h, w, c, seed=c + h + w)
    nr, nc = _assert_ties(x1, pos)
    x = rnd(300 + c, b, h, w, c)
    dout = rnd(400 + c, b, h, w, c)
    prm = _gate_params(c, c * 10 + w)
    # float64
    x64, x164 = x.double().requires_grad_(True), x1.double().requires_grad_(True)
    p64 = [t.double().requires_grad_(i not in (7, 8, 12, 13)) for i, t in enumerate(prm)]
    out64 = _gated_sum_torch(x64, x164, p64, groups, bn_train)[0]
    leaves = [x64, x164] + [t for t in p64 if t.requires_grad]
    grads = torch.autograd.grad(out64, leaves, dout.double())
    # HIP
    flat = lambda t: t.reshape(-1, c).contiguous().to(DEV)
    xg, x1g = flat(x).requires_grad_(True), flat(x1).requires_grad_(True)
    pd = [t.clone().to(DEV).requires_grad_(i not in (7, 8, 12, 13)) for i, t in enumerate(prm)]
    out = T._GatedSum.apply(xg, x1g, b, h, w, bn_train, groups, *pd)
    assert rel(out, out64.detach().reshape(-1, c)) < 2e-6, "output"
    out.backward(flat(dout))
    assert torch.equal(xg.grad.cpu(), dout.reshape(-1, c)), "dx"
    e_dx1 = rel(x1g.grad, grads[1].reshape(-1, c))
    errs = [e_dx1]
    names = ("se_w1", "se_b1", "se_w2", "se_b2", "cw_w", "cw_g", "cw_b", "hc_w", "hc_g", "hc_b")
    gp = grads[2:]
    gscale = max(gq.norm().item() for gq in gp)
    got_p = [t.grad for i, t in enumerate(pd) if i not in (7, 8, 12, 13)]
    for got, ref, nm in zip(got_p, gp, names):
        e = (got.cpu().double() - ref).norm().item() / max(ref.norm().item(), 1e-3 * gscale)
        errs.append(e)
        assert e < 2e-5, (nm, e)
    for i in (7, 8, 12, 13):
        assert (pd[i].detach().cpu() - p64[i].detach().float()).abs().max().item() < 1e-6, i
    print(f"C={c} {h}x{w} B={b} groups={groups} bn_train={bn_train}: {nr} rows / {nc} columns with tied maxima; dx1 {e_dx1:.1e} "
          f"(bound 5e-6), worst parameter gradient {max(errs[1:]):.1e} (bound 2e-5)")
    assert e_dx1 < 5e-6, ("dx1", e_dx1)


@pytest.mark.parametrize("c,h,w", [(32, 37, 130), (64, 130, 23), (128, 75, 130), (32, 200, 200)])
def test_plane_stats_argmax_and_apply_bwd_single_map(c, h, w):
    """The one-map entry points on tied planes: spei_plane_stats returns the maxima bit-exactly and their arg-max as torch.max(dim)
    does (lowest x of a row, lowest y of a column — also when the equal maxima lie in different 16-wide tiles), and
    spei_resblock_apply_bwd, given the float64 statement's gates and statistic gradients, returns its dx1."""
    import ctypes as C
    from speinet_amd import _lib
    x1, pos = _tie_planes(1, h, w, c, seed=7 * c + h)
    _assert_ties(x1, pos)
    dout = rnd(500 + c, 1, h, w, c)
    prm = _gate_params(c, c + 3 * h)
    x164 = x1.double().requires_grad_(True)
    p64 = [t.double() for t in prm]
    out64, stats, gates = _gated_sum_torch(torch.zeros_like(x164), x164, p64, 1, False)
    d_stats = torch.autograd.grad(out64, stats, dout.double(), retain_graph=True)
    dx1_64 = torch.autograd.grad(out64, x164, dout.double())[0]
    ctx = T._ctx(torch.device(DEV))
    lib = _lib.lib()
    P = lambda t: T._p(ctx, t)
    dv = lambda t: t.float().contiguous().to(DEV)
    a = dv(x1.reshape(-1, c))
    rowmax, rowmean, colmax, colmean, mean = (torch.empty(n, c, device=DEV) for n in (h, h, w, w, 1))
    rowarg, colarg = torch.full((h, c), -1, dtype=torch.int32, device=DEV), torch.full((w, c), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.spei_plane_ws_floats(h, w, c), device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(lib.spei_plane_stats(P(a), T._NULL, 0, h, w, c, P(rowmax), T._pi(ctx, rowarg), P(rowmean), P(colmax), T._pi(ctx, colarg),
                                        P(colmean), P(mean), P(ws), ctx._stream()), "spei_plane_stats")
        ref_rm, ref_ra = x1[0].max(dim=1)                       # [h, c] over x
        ref_cm, ref_ca = x1[0].max(dim=0)                       # [w, c] over y
        assert torch.equal(rowmax.cpu(), ref_rm) and torch.equal(colmax.cpu(), ref_cm), "maxima"
        bad_r, bad_c = int((rowarg.cpu() != ref_ra).sum()), int((colarg.cpu() != ref_ca).sum())
        assert bad_r == 0 and bad_c == 0, f"{bad_r} row / {bad_c} column arg-maxima differ from torch's first index"
        assert rel(rowmean, x1[0].double().mean(1)) < 1e-6 and rel(colmean, x1[0].double().mean(0)) < 1e-6
        s, g1, g2 = (dv(t.detach()[0]) for t in gates)
        dd = [dv(t[0]) for t in d_stats]
        dx1 = torch.empty_like(a)
        _lib.check(lib.spei_resblock_apply_bwd(P(dv(dout.reshape(-1, c))), P(s), P(g1), P(g2), T._pi(ctx, rowarg), T._pi(ctx, colarg),
                                               *[P(t) for t in dd], P(dx1), h, w, c, ctx._stream()), "spei_resblock_apply_bwd")
    e = rel(dx1, dx1_64.reshape(-1, c))
    print(f"C={c} {h}x{w}: arg-maxima exact; dx1 {e:.1e} (bound 5e-6)")
    assert e < 5e-6, e


def _flat_frame(kind, h, w):
    """One [1, 3, h, w] frame of flat content: 'letterbox' (black bars of h // 4 rows at the top and bottom) or 'highlight' (clipped
    at 1.0 in all channels: a blown-out band over the top h // 4 rows and a disc), over a synth_frames field."""
    f = synth_frames(1, h, w, seed=61)[0, 1].clone()
    if kind == "letterbox":
        f[:, :h // 4] = 0.0
        f[:, h - h // 4:] = 0.0
    else:
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        f[:, (yy - 0.6 * h) ** 2 + (xx - 0.55 * w) ** 2 < (0.25 * min(h, w)) ** 2] = 1.0
        f[:, :h // 4] = 1.0
    return f[None]


@pytest.mark.parametrize("kind,h,w", [("letterbox", 40, 60), ("highlight", 37, 53), ("letterbox", 64, 130)])
def test_resblock_backward_flat_content_vs_torch(synth_sd, kind, h, w):
    """The ResBlock of test_resblock_backward_vs_torch (inBlock.1, 32 channels, eval-mode gates) on conv_in features of flat content,
    where whole rows / columns of x1 are bit-identical.  The float64 statement takes the HIP forward's decisions, as
    test_conv_forward_backward does: its ReLU mask, and its ZPool arg-max — the FIRST exact maximum of HIP's fp32 x1 of each row /
    column, taken with gather — so only the arithmetic is compared, at the f32 bounds 1e-5 / 5e-5 / 1e-4."""
    net = SPEINet(args=default_args())
    net.load_state_dict(synth_sd, strict=True)
    rn = net.recons_net.to(DEV)
    blk = rn.inBlock[1]
    c = 32
    with torch.no_grad():
        x = T._ConvIn.apply(_flat_frame(kind, h, w).to(DEV), rn.inBlock[0][0].weight, rn.inBlock[0][0].bias)
        t_h = T._Conv2d.apply(x, blk.main[0].main[0].weight, blk.main[0].main[0].bias, None, 1, h, w, 5, 1, True)
        x1_h = T._Conv2d.apply(t_h, blk.main[1].main[0].weight, blk.main[1].main[0].bias, None, 1, h, w, 5, 1, False)
    x1_h = x1_h.cpu().view(1, h, w, c)
    mask = (t_h.cpu() > 0).view(1, h, w, c).permute(0, 3, 1, 2)
    ridx, cidx = x1_h.max(dim=2)[1], x1_h.max(dim=1)[1]                # first exact maxima: [1, h, c] over x, [1, w, c] over y
    ties_r = int(((x1_h == x1_h.amax(dim=2, keepdim=True)).sum(2) > 1).sum())
    ties_c = int(((x1_h == x1_h.amax(dim=1, keepdim=True)).sum(1) > 1).sum())
    assert ties_r + ties_c > 0, "no tied maxima in HIP's x1: the case does not test ties"
    # float64 statement with HIP's decisions
    sd = {k: v.detach().cpu().double().requires_grad_(v.requires_grad) for k, v in
          list(blk.named_parameters()) + [(k, b) for k, b in blk.named_buffers() if "running_" in k]}
    xd = x.cpu().double().view(1, h, w, c).permute(0, 3, 1, 2).requires_grad_(True)
    t = F.conv2d(xd, sd["main.0.main.0.weight"], sd["main.0.main.0.bias"], padding=2) * mask
    x1 = F.conv2d(t, sd["main.1.main.0.weight"], sd["main.1.main.0.bias"], padding=2).permute(0, 2, 3, 1)   # [1, h, w, c]
    stats = [x1.gather(2, ridx[:, :, None, :]).squeeze(2), x1.mean(dim=2), x1.gather(1, cidx[:, None]).squeeze(1), x1.mean(dim=1),
             x1.mean(dim=(1, 2))]
    names = ("se.fc.0.weight", "se.fc.0.bias", "se.fc.2.weight", "se.fc.2.bias", "te.cw.conv.conv.weight", "te.cw.conv.bn.weight",
             "te.cw.conv.bn.bias", "te.cw.conv.bn.running_mean", "te.cw.conv.bn.running_var", "te.hc.conv.conv.weight",
             "te.hc.conv.bn.weight", "te.hc.conv.bn.bias", "te.hc.conv.bn.running_mean", "te.hc.conv.bn.running_var")
    s, g1, g2 = gate_maps_torch(*stats, [sd[k].reshape(-1) if "running_" in k else sd[k] for k in names], False, False)
    out_ref = xd.permute(0, 2, 3, 1) + x1 * (s[:, None, None, :] + g1[:, :, None, :] + g2[:, None, :, :])
    g = rnd(70 + h, 1, h, w, c)
    out_ref.backward(g.double())
    # HIP
    xg = x.detach().clone().requires_grad_(True)
    out = T.resblock(xg, blk, 1, h, w, False)
    eo = rel(out, out_ref.detach().reshape(-1, c))
    out.backward(g.reshape(-1, c).to(DEV))
    ed = rel(xg.grad, xd.grad.permute(0, 2, 3, 1).reshape(-1, c))
    ep = {k: rel(p.grad, sd[k].grad) for k, p in blk.named_parameters()}
    worst = max(ep.items(), key=lambda kv: kv[1])
    print(f"{kind} {h}x{w}: x1 rows / columns with tied maxima {ties_r} / {ties_c}; output {eo:.1e} (1e-5), data gradient {ed:.1e} (5e-5), "
          f"worst parameter gradient {worst[1]:.1e} ({worst[0]}, 1e-4)")
    assert eo < 1e-5 and ed < 5e-5, (eo, ed)
    for k, e in ep.items():
        assert e < 1e-4, (k, e)


@pytest.mark.parametrize("content", ["natural", "flat"])
def test_encoder_groups_equal_separate_passes(synth_sd, content):
    """train.encoder(frames, groups=n) — n encoder passes of the reference in ONE set of launches, BatchNorm(1) statistics of the
    gates per group — against n separate train.encoder calls on a second copy of the model: the pyramid outputs, every parameter
    gradient and every BatchNorm running buffer within 1e-6 (train-mode gates, where the groups matter)."""
    from speinet_amd.synth import synth_frames_flat
    n, bs, h, w = 3, 2, 24, 36
    frames = (synth_frames(n * bs, h, w, seed=81) if content == "natural" else synth_frames_flat(n * bs, h, w, seed=82))[:, 1].contiguous().to(DEV)
    nets = []
    for _ in range(2):
        net = SPEINet(args=default_args())
        net.load_state_dict(synth_sd, strict=True)
        nets.append(net.to(DEV).train())
    g = torch.Generator().manual_seed(83)
    r = [torch.randn(n * bs * hh * ww, cc, generator=g).to(DEV) for cc, hh, ww in ((32, h, w), (64, h // 2, w // 2), (128, h // 4, w // 4))]

    def loss_of(levels):
        return sum((lv * rr).sum() * 0.5 ** i for i, (lv, rr) in enumerate(zip(levels, r)))

    lv_g = T.encoder(frames, nets[0].recons_net, True, pyramid=True, groups=n)
    loss_of(lv_g).backward()
    per = [T.encoder(frames[i * bs:(i + 1) * bs], nets[1].recons_net, True, pyramid=True) for i in range(n)]
    lv_s = [torch.cat([p[k].view(bs, -1, p[k].shape[1]) for p in per]).view(-1, per[0][k].shape[1]) for k in range(3)]
    loss_of(lv_s).backward()
    eo = max(rel(a, b.detach().cpu()) for a, b in zip(lv_g, lv_s))
    pa, pb = dict(nets[0].recons_net.named_parameters()), dict(nets[1].recons_net.named_parameters())
    errs = []
    for k, p in pa.items():
        if p.grad is None:
            assert pb[k].grad is None, k
            continue
        scale = pb[k].grad.norm().item()
        if ".bn." in k:                                   # a one-number, cancelling sum: against its gate's convolution weight
            scale = max(scale, pb[k.rsplit(".bn.", 1)[0] + ".conv.weight"].grad.norm().item())
        errs.append(((p.grad - pb[k].grad).norm().item() / max(scale, 1e-30), k))
    ba, bb = dict(nets[0].recons_net.named_buffers()), dict(nets[1].recons_net.named_buffers())
    eb = max((ba[k].double() - bb[k].double()).abs().max().item() / max(1.0, bb[k].double().abs().max().item()) for k in ba)
    worst = max(errs)
    print(f"{content}: encoder groups={n} vs {n} passes: outputs {eo:.1e}, {len(errs)} gradients worst {worst[0]:.1e} ({worst[1]}), "
          f"running buffers {eb:.1e}")
    assert len(errs) == 132 and eo < 1e-6 and worst[0] < 1e-6 and eb < 1e-6, (eo, worst, eb)
