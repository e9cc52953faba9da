"""The Swin and conv kernels on both sides of their 2^21-token kernel switches.

Three 16-bit kernels change code path with the map size; the rest of the suite stays below 60 000 tokens per map:

  MLP              stacked rows M <= 2^21   mlp_pipe_kernel     above: mlp_fused_kernel   (mlp_fused16.hip, mlp_launch)
  attention        tokens per map <= 2^21   attn_pipe_kernel    above: attn_win4_kernel   (attn_fused16.hip, attn4_launch)
  3x3 / 256 conv   pixels per map <= 2^21   conv3_pipe_kernel   above: the slab kernel    (ops.Ctx._conv3_pipe_ok)

These sizes are reachable: SPEINet.forward takes any H, W that are multiples of 20, and an 8K frame stacks M = 4 147 200 rows into each
MLP launch of its Swin body.  Every case asserts the side of the switch it runs on, next to the threshold it mirrors (the HIP thresholds
are read from the source, `test_dispatch_thresholds`), so that moving a threshold cannot quietly turn a case into a test of the other
kernel.  Tolerances are test_gpu_bf16.py's, relative to the magnitude of the branch; the float64 references run on sampled rows, windows
and tiles, never whole maps.  Peak device memory stays under ~20 GB per case (printed with the time of each case).

The two tests without the `gpu` mark prove the window-subset and cropped-tile references against the full-map oracle on the CPU.
"""
import os
import re
import time

import pytest
import torch
import torch.nn.functional as F

from oracle import speinet_oracle as O
from speinet_amd import engine, pack
from speinet_amd.ops import ACT_NONE, BMap, Ctx, FMap

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"bf16": 1.5e-2, "f16": 2e-3}                 # the per-kernel tolerances of test_gpu_bf16.py
LPD = {"bf16": torch.bfloat16, "f16": torch.float16}
MODES = ["f16", "bf16"]

# The dispatch thresholds mirrored here (test_dispatch_thresholds checks them against the HIP source):
MLP_PIPE_MAX_M = 1 << 21          # mlp_fused16.hip, mlp_launch:   pipe && M <= (1ll << 21)
ATTN_PIPE_MAX_HW = 1 << 21        # attn_fused16.hip, attn4_launch: pipe && (int64_t)H * W <= (1ll << 21)
T21 = 1 << 21                     # row / token 2^21: byte offset 2^31 of a [*, 256] fp32 buffer

MLP_P = "swin.layers.1.residual_group.blocks.2."
ATTN_P = "swin.layers.2.residual_group.blocks.1."


def _src_limit(name: str, pattern: str) -> int:
    with open(os.path.join(ROOT, "speinet_amd", "csrc", name)) as f:
        found = re.findall(pattern, f.read())
    assert len(found) == 1, (name, pattern, found)
    return 1 << int(found[0])


def test_dispatch_thresholds():
    """The thresholds this file's cases are placed around are the ones the launchers use."""
    assert _src_limit("mlp_fused16.hip", r"if \(pipe && M <= \(1ll << (\d+)\)\)") == MLP_PIPE_MAX_M
    assert _src_limit("attn_fused16.hip", r"if \(pipe && \(int64_t\)H \* W <= \(1ll << (\d+)\)\)") == ATTN_PIPE_MAX_HW


@pytest.fixture(autouse=True)
def _device_budget(request):
    """Each GPU case starts from an empty cache and reports its peak device memory and time."""
    if request.node.get_closest_marker("gpu") is None:
        yield
        return
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print(f"\n  [{request.node.name}] peak {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB, {time.time() - t0:.1f} s")
    torch.cuda.empty_cache()


def _randn(gen, rows, scale, shift):
    return torch.randn(rows, 256, device=DEV, generator=gen).mul_(scale).add_(shift)


def _rel(a, b, base, rows=1 << 20):
    """max |a - b| / max |base| on the device, over row chunks (the temporaries of a whole 4 GB map would double the peak)."""
    d = max((a[i:i + rows] - b[i:i + rows]).abs().max().item() for i in range(0, a.shape[0], rows))
    return d / max(max(base[i:i + rows].abs().max().item() for i in range(0, base.shape[0], rows)), 1e-30)


def _finite(t, rows=1 << 20):
    return all(torch.isfinite(t[i:i + rows]).all().item() for i in range(0, t.shape[0], rows))


# ---- 1. MLP -------------------------------------------------------------------------------------------------------------------------
def _sd64(sd, prefix, device):
    return {k: v.to(device, torch.float64) for k, v in sd.items() if k.startswith(prefix)}


def mlp_ref64(x, sd64, p):
    """x + fc2(GELU(fc1(LN(x)))) in float64 (reference model/swinir.py:279), the formula of test_mlp_fused_vs_oracle."""
    x = x.double()
    h = F.layer_norm(x, (256,), sd64[p + "norm2.weight"], sd64[p + "norm2.bias"], 1e-5)
    h = F.gelu(F.linear(h, sd64[p + "mlp.fc1.weight"], sd64[p + "mlp.fc1.bias"]))
    return x + F.linear(h, sd64[p + "mlp.fc2.weight"], sd64[p + "mlp.fc2.bias"])


MLP_CASES = [((1 << 21) - 1, "pipe"), (1 << 21, "pipe"), ((1 << 21) + 1, "fallback"), ((1 << 21) + 96 * 7 + 37, "fallback"),
             (2 * (7680 // 4) * (4320 // 4), "fallback")]        # last: an 8K frame's two Swin calls stacked (engine.swin_multi)


@pytest.mark.gpu
@pytest.mark.parametrize("M,kernel", MLP_CASES, ids=[f"{m}-{k}" for m, k in MLP_CASES])
@pytest.mark.parametrize("mode", MODES)
def test_mlp_both_sides_of_2p21(synth_sd, mode, M, kernel):
    """ops.mlp_fused on M rows (one launch) against (a) the same rows cut into views of at most 1.1M rows, each a pipe-kernel launch
    (every row compared; bit-identity reported, not required), (b) float64 on sampled rows: the first two tiles, the last 3 x 96 rows,
    the rows around row 2^21 (byte offset 2^31) and 4096 seeded random rows; in place (out is x, as engine.swin_multi calls it) and out
    of place must agree bit for bit."""
    assert (M <= MLP_PIPE_MAX_M) == (kernel == "pipe")
    ops = Ctx(mode, device=DEV)
    bk = pack._to_device(pack.swin_block(synth_sd, MLP_P, 8, 5), DEV)
    args = (bk["w1"], bk["b1"], bk["w2"], bk["b2"])
    gen = torch.Generator(device=DEV).manual_seed(M)
    x = _randn(gen, M, 1.5, 0.3)
    out = ops.mlp_fused(x, *args, out=torch.empty_like(x))
    ip = x.clone()
    ops.mlp_fused(ip, *args, out=ip)
    assert torch.equal(ip, out), "in place and out of place differ"
    del ip

    # (a) views of at most 1.1M rows, each below the switch
    CH = 1_100_000
    assert CH <= MLP_PIPE_MAX_M
    tmp = torch.empty(min(CH, M), 256, device=DEV)
    dmax, bmax, same = 0.0, 0.0, True
    for a in range(0, M, CH):
        b = min(M, a + CH)
        ref = ops.mlp_fused(x[a:b], *args, out=tmp[:b - a])
        dmax = max(dmax, (out[a:b] - ref).abs().max().item())
        bmax = max(bmax, (ref - x[a:b]).abs().max().item())
        same = same and torch.equal(out[a:b], ref)
    del tmp
    e_views = dmax / bmax
    assert _finite(out) and e_views < TOL[mode], f"M={M}: vs views rel err {e_views:.2e}"

    # (b) float64 on sampled rows
    sd64 = _sd64(synth_sd, MLP_P, DEV)
    g = torch.Generator().manual_seed(7 + M)
    groups = {"first two tiles": torch.arange(0, 256), "last 3x96 rows": torch.arange(M - 3 * 96, M),
              "rows around 2^21": torch.arange(max(0, T21 - 200), min(M, T21 + 200)),
              "4096 random": torch.randint(0, M, (4096,), generator=g)}
    errs = {}
    for name, rows in groups.items():
        rows = rows.to(DEV)
        xs = x[rows]
        ref = mlp_ref64(xs, sd64, MLP_P)
        errs[name] = _rel(out[rows].double(), ref, ref - xs.double())
    print(f"\n  MLP {mode} M={M} ({kernel}): vs views {e_views:.2e} (bit-identical: {same}); float64 "
          + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for name, e in errs.items():
        assert e < TOL[mode], f"M={M} {name}: rel err {e:.2e}"


# ---- 2. attention -------------------------------------------------------------------------------------------------------------------
def window_branch64(x, y, sd64, p, h, w, shift, wins):
    """The attention branch (reference model/swinir.py:238-278) of the shifted-frame windows `wins` ([n, 2] = (window row, window col))
    of ONE h x w map, from the oracle's pieces: x, y [h*w, 256] tokens (any device; gathered and computed in float64).  Returns the
    map pixels of the windows' tokens [n, 25] and the branch at them [n, 25, 256].  The roll is taken per token and the shift mask
    from the region ids of the requested rows / columns only (O.shift_mask's slices)."""
    dev = x.device
    assert wins.ndim == 2 and (wins >= 0).all() and (wins[:, 0] < h // 5).all() and (wins[:, 1] < w // 5).all(), "window out of the map"
    wins = wins.to(dev)
    t = torch.arange(25, device=dev)
    ysf = wins[:, :1] * 5 + t // 5                      # shifted-frame coordinates [n, 25]
    xsf = wins[:, 1:] * 5 + t % 5
    pix = ((ysf + shift) % h) * w + (xsf + shift) % w   # torch.roll(-shift): shifted[y] = x[(y + shift) % H]
    ln = lambda v: F.layer_norm(v[pix].double(), (256,), sd64[p + "norm1.weight"], sd64[p + "norm1.bias"], 1e-5)
    mask = None
    if shift:
        def region(n):
            r = torch.zeros(n, dtype=torch.long, device=dev)
            r[slice(-5, -shift)] = 1
            r[slice(-shift, None)] = 2
            return r
        reg = 3 * region(h)[ysf] + region(w)[xsf]
        mask = torch.zeros(reg.shape + (25,), dtype=torch.float64, device=dev).masked_fill_(reg.unsqueeze(2) != reg.unsqueeze(1), -100.0)
    return pix, O.window_attention(ln(x), ln(y), sd64, p + "attn.", 8, 5, mask)


def attn_oracle_full(x, y, sd, p, h, w, shift):
    """The full-map construction of test_attn_fused_vs_oracle: the branch [h*w, 256] in map order."""
    ln = lambda t: F.layer_norm(t, (256,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-5).view(1, h, w, 256)
    xn, yn = ln(x), ln(y)
    if shift:
        xn, yn = (torch.roll(t, shifts=(-shift, -shift), dims=(1, 2)) for t in (xn, yn))
    xw, yw = (O.window_partition(t, 5).view(-1, 25, 256) for t in (xn, yn))
    mask = O.shift_mask(h, w, 5, shift) if shift else None
    br = O.window_reverse(O.window_attention(xw, yw, sd, p + "attn.", 8, 5, mask).view(-1, 5, 5, 256), 5, h, w)
    if shift:
        br = torch.roll(br, shifts=(shift, shift), dims=(1, 2))
    return br.reshape(h * w, 256)


@pytest.mark.parametrize("h,w", [(20, 35), (45, 80)])
@pytest.mark.parametrize("shift", [0, 2])
def test_window_subset_reference_matches_full_oracle(synth_sd, h, w, shift):
    """window_branch64 on every window of a map = the full-map oracle (float64, CPU)."""
    sd64 = _sd64(synth_sd, ATTN_P, "cpu")
    g = torch.Generator().manual_seed(h * w + shift)
    x = torch.randn(h * w, 256, generator=g, dtype=torch.float64) * 1.3 + 0.2
    y = torch.randn(h * w, 256, generator=g, dtype=torch.float64) * 0.9 - 0.1
    full = attn_oracle_full(x, y, sd64, ATTN_P, h, w, shift)
    wy, wx = torch.meshgrid(torch.arange(h // 5), torch.arange(w // 5), indexing="ij")
    wins = torch.stack((wy.reshape(-1), wx.reshape(-1)), 1)[torch.randperm(h * w // 25, generator=g)]      # any order
    pix, br = window_branch64(x, y, sd64, ATTN_P, h, w, shift, wins)
    assert torch.equal(torch.sort(pix.reshape(-1)).values, torch.arange(h * w))
    torch.testing.assert_close(br.reshape(-1, 256), full[pix.reshape(-1)], rtol=1e-12, atol=1e-12)


def _window_of(pix, h, w, shift):
    y, x = divmod(pix, w)
    return [((y - shift) % h) // 5, ((x - shift) % w) // 5]


def _sample_windows(h, w, shift, b, m, seed):
    """The last window row and column of map b (wrapped and masked), the windows holding stacked tokens 2^21 - 1 and 2^21 where they lie
    in map b, and 256 seeded random windows."""
    nwy, nwx = h // 5, w // 5
    wins = [[nwy - 1, j] for j in range(nwx)] + [[i, nwx - 1] for i in range(nwy - 1)]
    wins += [_window_of(t - b * m, h, w, shift) for t in (T21 - 1, T21) if b * m <= t < (b + 1) * m]
    g = torch.Generator().manual_seed(seed)
    wins += torch.stack((torch.randint(0, nwy, (256,), generator=g), torch.randint(0, nwx, (256,), generator=g)), 1).tolist()
    return torch.tensor(wins)


ATTN_CASES = [(1445, 1450, "pipe"), (1450, 1450, "fallback")]     # 2 095 250 / 2 102 500 tokens per map


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("h,w,kernel", ATTN_CASES, ids=[f"{h}x{w}-{k}" for h, w, k in ATTN_CASES])
@pytest.mark.parametrize("mode", MODES)
def test_attn_both_sides_of_2p21(synth_sd, mode, h, w, kernel, shift):
    """ops.attn_fused (the four-window kernel family) on two stacked h x w maps (a >4 GB buffer): each map's rows bit-identical to that
    map launched alone; float64 window-subset reference (window_branch64) on the last window row and column, the windows of stacked
    tokens 2^21 - 1 / 2^21 and 256 random windows per map; with shift 0 (independent windows) also every token against row blocks of
    40 rows (contiguous views, 58 000 tokens: the 720p size class) run as maps of their own."""
    m = h * w
    assert (m <= ATTN_PIPE_MAX_HW) == (kernel == "pipe")
    ops = Ctx(mode, device=DEV)
    assert ops.attn_win4
    bk = pack._to_device(pack.swin_block(synth_sd, ATTN_P, 8, 5), DEV)
    gen = torch.Generator(device=DEV).manual_seed(m + shift)
    x = _randn(gen, 2 * m, 1.3, 0.2)
    y = _randn(gen, 2 * m, 0.9, -0.1)
    yhat = ops.layernorm(y, out_dtype=LPD[mode])
    sd64 = _sd64(synth_sd, ATTN_P, DEV)
    refs = []
    for b in range(2):                                  # float64 references first: y is not needed after them
        pix, br = window_branch64(x[b * m:(b + 1) * m], y[b * m:(b + 1) * m], sd64, ATTN_P, h, w, shift,
                                  _sample_windows(h, w, shift, b, m, 100 * b + shift))
        refs.append((b * m + pix.reshape(-1), br.reshape(-1, 256)))
    del y
    both = ops.attn_fused(x, yhat, bk, h, w, shift, out=torch.empty_like(x))
    assert _finite(both)
    alone = torch.empty(m, 256, device=DEV)
    for b in range(2):
        ops.attn_fused(x[b * m:(b + 1) * m], yhat[b * m:(b + 1) * m], bk, h, w, shift, out=alone)
        assert torch.equal(both[b * m:(b + 1) * m], alone), f"map {b} of the batch differs from the map alone"
    del alone
    errs = []
    for rows, br in refs:
        errs.append(_rel(both[rows].double() - x[rows].double(), br, br))
    msg = f"\n  attention {mode} {h}x{w} shift {shift} ({kernel}): float64 windows map 0 {errs[0]:.2e}, map 1 {errs[1]:.2e}"
    if shift == 0:
        RB = 40
        tmp = torch.empty(RB * w, 256, device=DEV)
        dmax, bmax, same = 0.0, 0.0, True
        for b in range(2):
            for r0 in range(0, h, RB):
                r1 = min(h, r0 + RB)
                s = slice(b * m + r0 * w, b * m + r1 * w)
                blk = ops.attn_fused(x[s], yhat[s], bk, r1 - r0, w, 0, out=tmp[:(r1 - r0) * w])
                dmax = max(dmax, (both[s] - blk).abs().max().item())
                bmax = max(bmax, (blk - x[s]).abs().max().item())
                same = same and torch.equal(both[s], blk)
        errs.append(dmax / bmax)
        msg += f"; vs 40-row blocks {errs[-1]:.2e} (bit-identical: {same})"
    print(msg)
    for e in errs:
        assert e < TOL[mode], msg


# ---- 3. 3x3 / 256-channel conv ------------------------------------------------------------------------------------------------------
def conv_tile_ref64(xm, rm, w64, b64, y0, x0, th, tw):
    """F.conv2d(x, w, b, padding=1) + r on the th x tw output tile at (y0, x0) of one map, in float64, from the tile's input crop with a
    one-pixel halo (zeros outside the map).  xm, rm: [H, W, 256]."""
    H, W = xm.shape[:2]
    crop = torch.zeros(th + 2, tw + 2, 256, dtype=torch.float64, device=xm.device)
    ya, yb, xa, xb = max(y0 - 1, 0), min(y0 + th + 1, H), max(x0 - 1, 0), min(x0 + tw + 1, W)
    crop[ya - (y0 - 1):yb - (y0 - 1), xa - (x0 - 1):xb - (x0 - 1)] = xm[ya:yb, xa:xb].double()
    cols = F.unfold(crop.permute(2, 0, 1).unsqueeze(0), 3)[0]                  # [256 * 9, th * tw], (channel, ky, kx) order
    out = (w64.reshape(256, -1) @ cols + b64[:, None]).reshape(256, th, tw).permute(1, 2, 0)
    return out + rm[y0:y0 + th, x0:x0 + tw].double()


def test_conv_tile_reference_matches_conv2d():
    """conv_tile_ref64 = F.conv2d on the whole map (float64, CPU) at corners, edges and the interior."""
    g = torch.Generator().manual_seed(5)
    H, W = 18, 40
    x = torch.randn(H, W, 256, generator=g)
    r = torch.randn(H, W, 256, generator=g)
    wt, b = torch.randn(256, 256, 3, 3, generator=g, dtype=torch.float64) * 0.03, torch.randn(256, generator=g, dtype=torch.float64)
    full = F.conv2d(x.double().permute(2, 0, 1).unsqueeze(0), wt, b, padding=1)[0].permute(1, 2, 0) + r.double()
    for (y0, x0) in ((0, 0), (0, W - 32), (H - 12, 0), (H - 12, W - 32), (3, 5)):
        torch.testing.assert_close(conv_tile_ref64(x, r, wt, b, y0, x0, 12, 32), full[y0:y0 + 12, x0:x0 + 32], rtol=1e-12, atol=1e-12)


def _conv_tiles(h, w, b, m, seed, th=12, tw=32):
    """Output tiles (y0, x0) of map b: the four corners, the tiles around stacked pixels 2^21 - 1 and 2^21 where they lie in map b,
    and six seeded random positions."""
    tiles = [(0, 0), (0, w - tw), (h - th, 0), (h - th, w - tw)]
    for t in (T21 - 1, T21):
        if b * m <= t < (b + 1) * m:
            y, x = divmod(t - b * m, w)
            tiles.append((min(max(y - th // 2, 0), h - th), min(max(x - tw // 2, 0), w - tw)))
    g = torch.Generator().manual_seed(seed)
    tiles += [(int(torch.randint(0, h - th + 1, (1,), generator=g)), int(torch.randint(0, w - tw + 1, (1,), generator=g))) for _ in range(6)]
    return tiles


CONV_CASES = [(1536, 1360, "pipe"), (1548, 1360, "slab")]       # 2 088 960 (the largest pipe map of this width) / 2 105 280 pixels


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,kernel", CONV_CASES, ids=[f"{h}x{w}-{k}" for h, w, k in CONV_CASES])
@pytest.mark.parametrize("mode", MODES)
def test_conv3_both_sides_of_2p21(mode, h, w, kernel):
    """The Swin body's 3x3 / 256-channel conv on two stacked h x w maps through igemm_batched with the residual aliasing the output (as
    engine.swin_multi calls it), and on map 0 alone through igemm (residual aliasing the output, as engine.swin calls it): float64 tiles
    with halo at the corners, around stacked pixel 2^21 - 1 and at random positions of both maps; on the pipe map also the whole result
    against the slab kernel (conv3_pipe=False)."""
    m = h * w
    ops = Ctx(mode, device=DEV)
    g = torch.Generator().manual_seed(31)
    wt, bias = torch.randn(256, 256, 3, 3, generator=g) * 0.03, torch.randn(256, generator=g) * 0.1
    pw = pack.PackedW(pack.conv_w(wt), DEV)
    bd = bias.to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(m)
    x = _randn(gen, 2 * m, 1.0, 0.0)
    r = _randn(gen, 2 * m, 1.0, 0.0)
    xb, rb = BMap(x, 2, h, w, 256), BMap(r.clone(), 2, h, w, 256)
    assert ops._conv3_pipe_ok(xb, pw, 256, 3, 1, ACT_NONE, rb, rb) == (kernel == "pipe")
    out = ops.igemm_batched(xb, pw, bd, 256, 3, residual=rb, out=rb)
    assert out.t.data_ptr() == rb.t.data_ptr() and _finite(out.t)
    # map 0 alone through igemm, in place on its residual
    one = FMap(r[:m].clone(), h, w, 256)
    assert ops._conv3_pipe_ok(FMap(x[:m], h, w, 256), pw, 256, 3, 1, ACT_NONE, one, one) == (kernel == "pipe")
    ops.igemm(FMap(x[:m], h, w, 256), pw, bd, 256, ksize=3, residual=one, out=one)
    e_one, same_one = _rel(one.t, out.t[:m], out.t[:m]), torch.equal(one.t, out.t[:m])
    del one
    w64, b64 = wt.to(DEV, torch.float64), bias.to(DEV, torch.float64)
    errs = []
    for b in range(2):
        xm, rm, om = (t[b * m:(b + 1) * m].view(h, w, 256) for t in (x, r, out.t))
        for (y0, x0) in _conv_tiles(h, w, b, m, 40 + b):
            ref = conv_tile_ref64(xm, rm, w64, b64, y0, x0, 12, 32)
            errs.append(((y0, x0, b), _rel(om[y0:y0 + 12, x0:x0 + 32].double(), ref, ref)))
    worst = max(errs, key=lambda t: t[1])
    msg = (f"\n  conv3 {mode} {h}x{w} ({kernel}): float64 tiles worst {worst[1]:.2e} at (y, x, map) {worst[0]}; "
           f"igemm map 0 vs batched {e_one:.2e} (bit-identical: {same_one})")
    if kernel == "pipe":
        slab = ops.replace(conv3_pipe=False)
        assert not slab._conv3_pipe_ok(xb, pw, 256, 3, 1, ACT_NONE, BMap(r, 2, h, w, 256), None)
        old = slab.igemm_batched(xb, pw, bd, 256, 3, residual=BMap(r, 2, h, w, 256))
        e_slab = _rel(out.t, old.t, old.t)
        msg += f"; vs slab kernel {e_slab:.2e} (bit-identical: {torch.equal(out.t, old.t)})"
        errs.append(("slab", e_slab))
    print(msg)
    for where, e in errs:
        assert e < TOL[mode], f"{msg} ({where}: {e:.2e})"
    assert e_one < TOL[mode], msg


# ---- 4. routing through engine.swin_multi -------------------------------------------------------------------------------------------
# swin_multi against swin per map, measured on two stacked 180 x 320 maps (both sides of every switch the same kernel): map 0 bit-identical,
# map 1 8.5e-4 (f16) / 5.4e-3 (bf16) -- the MLP and attention pipe kernels start each tile's K walk at a rotation taken from the tile
# index, which moves when a map is stacked behind another; the same calls differ from the f32 engine by 8.8e-4 / 8.1e-3.  The bound is
# test_gpu_bf16.py's per-kernel TOL, 2.3x / 2.8x the 720p figure.
ROUTE_TOL = {"f16": 2e-3, "bf16": 1.5e-2}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_swin_multi_past_2p21_matches_swin(synth_sd, mode):
    """engine.swin_multi on two stacked 1025 x 1025 maps (M = 2 101 250 rows: every MLP launch takes the fallback kernel, attention the
    pipe kernel per map, the conv the slab kernel) against engine.swin on each map alone (M = 1 050 625: the MLP pipe kernel).  Measured:
    6.6e-4 / 6.5e-4 (f16) and 5.3e-3 / 5.1e-3 (bf16) for maps 0 / 1 -- the 720p size of the difference (ROUTE_TOL)."""
    from speinet_amd.speinet import SPEINet, default_args
    h = w = 1025
    m = h * w
    assert 2 * m > MLP_PIPE_MAX_M and m <= MLP_PIPE_MAX_M and m <= ATTN_PIPE_MAX_HW
    net = SPEINet(args=default_args())
    net.load_state_dict(synth_sd, strict=True)
    sw = net._pack(torch.device(DEV))["swin"]
    ops = Ctx(mode, device=DEV)
    assert ops.swin_multi_available()
    gen = torch.Generator(device=DEV).manual_seed(1025)
    f_mid = FMap(torch.randn(m, 128, device=DEV, generator=gen).mul_(0.5), h, w, 128)
    feats = BMap(torch.randn(2 * m, 128, device=DEV, generator=gen).mul_(0.5), 2, h, w, 128)
    sx = engine.SwinX(ops, f_mid, sw)
    outs = [FMap.empty(h, w, 128, DEV) for _ in range(2)]
    engine.swin_multi(ops, sx, feats, sw, outs)
    one = FMap.empty(h, w, 128, DEV)
    errs = []
    for b in range(2):
        engine.swin(ops, sx, feats.map(b), sw, out=one)
        assert _finite(outs[b].t)
        errs.append((_rel(outs[b].t, one.t, one.t), torch.equal(outs[b].t, one.t)))
    print(f"\n  swin_multi {mode} 2 x {h}x{w} vs swin per map: " + ", ".join(f"map {b} {e:.2e} (bit-identical: {s})" for b, (e, s) in enumerate(errs)))
    for e, _ in errs:
        assert e < ROUTE_TOL[mode]
