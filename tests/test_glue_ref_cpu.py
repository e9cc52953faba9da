"""CPU suite for tests/glue_ref.py, the float64 statement that tests/test_gpu_glue_f64.py holds the fp32 glue kernels to (RL prior,
bicubic upsampling, LayerNorm, the f32 window-attention core).  It runs no kernel.  The attention reference reproduces the reference
implementation's golden vectors and the oracle; the written-out forms that the wrong variants are built from equal the references;
every mistake of `wrong_variants()` moves some small case of the GPU test's own tables by at least 100 times that operation's bound --
the evidence that the GPU test would fail on a kernel with that mistake; and what the GPU tests assume about their cases holds."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_ref as R
from oracle import speinet_oracle as O

F64 = torch.float64
BLOCKS = "swin.layers.0.residual_group.blocks."


def g(golden_dir, name):
    d = np.load(os.path.join(golden_dir, name + ".npz"))
    return {k: torch.from_numpy(d[k]) for k in d.files}


def attn_params64(sd, p):
    """(scaled q weights, kv weights, relbias [8,25,25], proj) of one block in float64, from the state_dict alone."""
    w = {k: sd[p + "attn." + k].to(F64) for k in ("qkv_y.weight", "qkv_y.bias", "qkv_x.weight", "qkv_x.bias", "proj.weight", "proj.bias",
                                                  "relative_position_bias_table")}
    relbias = w["relative_position_bias_table"][O.rel_pos_index(5).view(-1)].view(25, 25, -1).permute(2, 0, 1).contiguous()
    return w, relbias


def attention_through_linears64(sd, p, x, y, h, w, shift):
    """x (K, V side) and y (Q side): [H*W, 256] normalised tokens of the unshifted frame -> proj(core(q, kv))."""
    wt, relbias = attn_params64(sd, p)
    q = F.linear(y.to(F64), wt["qkv_y.weight"] * R.HD ** -0.5, wt["qkv_y.bias"] * R.HD ** -0.5)
    kv = F.linear(x.to(F64), wt["qkv_x.weight"], wt["qkv_x.bias"])
    return F.linear(R.window_attention64(q, kv, relbias, h, w, shift), wt["proj.weight"], wt["proj.bias"])


def token_order(win, h, w):
    """[nW, 25, C] window-major -> [h*w, C]."""
    return O.window_reverse(win.reshape(-1, 5, 5, win.shape[-1]), 5, h, w).reshape(h * w, -1)


def unshift(t, h, w, shift):
    return torch.roll(t.view(h, w, -1), (shift, shift), (0, 1)).reshape(h * w, -1) if shift else t


def test_window_attention64_reproduces_golden_g04(golden_dir, synth_sd):
    """Both blocks of g04 (no mask; shift 2 with the reference's own mask) through float64 linears.  The golden outputs are the
    reference's fp32: 256-term sums of products, so |difference| <= 1e-6 + 1e-5 max|golden| as everywhere in this suite's fp32 checks."""
    d = g(golden_dir, "g04_winattn")
    h, w = 10, 15
    for blk, key, shift in ((0, "out_nomask", 0), (1, "out_mask", 2)):
        xs, ys = (unshift(token_order(d[k], h, w), h, w, shift) for k in ("xw", "yw"))
        got = attention_through_linears64(synth_sd, f"{BLOCKS}{blk}.", xs, ys, h, w, shift)
        want = unshift(token_order(d[key], h, w), h, w, shift).to(F64)
        err = (got - want).abs().max().item()
        print(f"g04 block {blk}: max|float64 - golden| {err:.3e}, max|golden| {want.abs().max().item():.3e}")
        assert err <= 1e-6 + 1e-5 * want.abs().max().item()


@pytest.mark.parametrize("h,w", [(10, 15), (5, 5)])
@pytest.mark.parametrize("shift", [0, 2])
def test_window_attention64_reproduces_the_oracle(synth_sd, h, w, shift):
    """`O.window_attention` evaluated in float64 on rolled and partitioned tokens, with the oracle's mask; float64 round-off only."""
    p = f"{BLOCKS}{1 if shift else 0}."
    sd64 = {k: v.to(F64) for k, v in synth_sd.items() if k.startswith(p + "attn.") and v.dtype.is_floating_point}
    r = R.rng(50 + h + shift)
    x, y = (torch.from_numpy(r.randn(h * w, 256)) for _ in range(2))

    def windows(t):
        t = t.view(1, h, w, 256)
        t = torch.roll(t, (-shift, -shift), (1, 2)) if shift else t
        return O.window_partition(t, 5).view(-1, 25, 256)
    mask = O.shift_mask(h, w, 5, shift).to(F64) if shift else None
    want = O.window_reverse(O.window_attention(windows(x), windows(y), sd64, p + "attn.", 8, 5, mask).view(-1, 5, 5, 256), 5, h, w)
    want = (torch.roll(want, (shift, shift), (1, 2)) if shift else want).reshape(h * w, 256)
    got = attention_through_linears64(synth_sd, p, x, y, h, w, shift)
    assert R.nerr(got, want) <= 1e-12


def test_written_out_forms_equal_the_references():
    """The tap-matrix bicubic and the RL loop that the wrong variants switch pieces of are the references when nothing is switched."""
    for _, h, w, c, s, relu in R.bicubic_cases():
        x = R.bicubic_map(h, w, c)
        assert R.nerr(R.bicubic_taps64(x, h, w, s, relu), R.bicubic64(x, h, w, s, relu)) <= 1e-14, (h, w, c, s, relu)
    for h, w, c, it, lam, content in R.rl_cases():
        x = R.rl_image(h, w, c, content)
        assert R.nerr(R._rl_variant(x, it, lam), R.rl_prior64(x, it, lam)) <= 1e-13, (h, w, c, it, lam, content)


def test_region_mean_is_the_uniform_sets_attention():
    for h, w in R.ATTN_SIZES:
        for shift in R.ATTN_SHIFTS:
            q, kv, rb = R.attn_operands("uniform", h, w)
            assert R.nerr(R.region_mean64(kv, h, w, shift), R.window_attention64(q, kv, rb, h, w, shift)) <= 1e-14, (h, w, shift)


def test_mask_regions_of_the_attention_sizes():
    """A 5 x 5 map is one window cut into the four regions {1, 2} x {1, 2} (region 0, v < n - 5, is empty there), 10 x 15 has all
    nine, and the region ids written here give the oracle's mask."""
    for shift in (1, 2, 3, 4):
        assert R._window_regions(5, 5, shift).unique().tolist() == [4, 5, 7, 8]
        assert R._window_regions(10, 15, shift).unique().numel() == 9
        assert torch.equal(R._window_regions(10, 15, shift)[:, None, :] != R._window_regions(10, 15, shift)[:, :, None],
                           O.shift_mask(10, 15, 5, shift) != 0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_ulp16(dtype):
    p = R.LP_BITS[dtype][0]
    x = torch.tensor([1.0, 1.5, 1.9999, 2.0, 0.75, -3.0, 1000.0], dtype=F64)
    assert torch.equal(R.ulp16(x, dtype), torch.tensor([1.0, 1.0, 1.0, 2.0, 0.5, 2.0, 512.0], dtype=F64) * 2.0 ** (1 - p))
    if dtype == torch.float16:
        assert torch.equal(R.ulp16(torch.tensor([0.0, 1e-6, 2.0 ** -14], dtype=F64), dtype), torch.full((3,), 2.0 ** -24, dtype=F64))
    v = torch.from_numpy(R.rng(9).randn(100000).astype(np.float32) * 3)
    err = (v.to(dtype).to(F64) - v.to(F64)).abs()
    assert (err <= R.ulp16(v.to(F64), dtype) / 2).all() and (err > 0.49 * R.ulp16(v.to(F64), dtype)).any()


# ------------------------------------------------------------------------------------------------------------------------------
# sensitivity: the small cases of the GPU test's tables see every wrong variant at 100 times the bound
# ------------------------------------------------------------------------------------------------------------------------------
def variant_ratios(op, fn):
    """{case: max|variant - reference| / max|reference| / bound} on the smallest shapes of the operation's table."""
    out = {}
    if op == "window_attention":
        for name, h, w, shift in R.attn_cases():
            if (h, w) == R.ATTN_SIZES[0]:
                q, kv, rb = R.attn_operands(name, h, w)
                out[(name, h, w, shift)] = R.nerr(fn(q, kv, rb, h, w, shift), R.window_attention64(q, kv, rb, h, w, shift)) / R.bound(R.attn_op(name))
    elif op == "layernorm":
        for m in R.LN_ROWS[:4]:
            for affine in (True, False):
                x, gm, bt, want, _ = R.ln_case(m, affine)
                out[(m, affine)] = R.nerr(fn(x, gm, bt) if affine else fn(x), want) / R.bound(op)
    elif op == "bicubic":
        for case in R.bicubic_cases():
            _, h, w, c, s, relu = case
            if (h, w) in R.BICUBIC_SIZES[:4]:
                x = R.bicubic_map(h, w, c)
                out[case] = R.nerr(fn(x, h, w, s, relu), R.bicubic64(x, h, w, s, relu)) / R.bound(op)
    elif op == "rl_prior":
        for case in R.rl_cases():
            h, w, c, it, lam, content = case
            if (h, w) in R.RL_SIZES[:4]:
                x = R.rl_image(h, w, c, content)
                out[case] = R.nerr(fn(x, it, lam), R.rl_prior64(x, it, lam)) / R.bound(op)
    return out


@pytest.mark.parametrize("name", list(R.wrong_variants()))
def test_the_cases_see_each_wrong_variant(name):
    op, fn = R.wrong_variants()[name]
    ratios = variant_ratios(op, fn)
    case = max(ratios, key=ratios.get)
    print(f"{name}: {ratios[case]:.3g} x the bound at {case}")
    assert ratios[case] >= 100


# ------------------------------------------------------------------------------------------------------------------------------
# what the GPU tests assume about their cases
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", R.OPS)
def test_host_fp32_error_is_positive(op):
    errs = R.host_errors(op)
    lo, hi = min(errs, key=errs.get), max(errs, key=errs.get)
    print(f"{op}: e_host {errs[hi]:.3e} at {hi}; smallest {errs[lo]:.3e} at {lo}; {len(errs)} cases")
    assert 0 < errs[hi] < 1e-4 and R.e_host(op) == errs[hi] and R.bound(op) == 4 * errs[hi]


def test_references_are_finite_and_rl_zeros_stay_zero():
    for h, w, c, it, lam, content in R.rl_cases():
        x = R.rl_image(h, w, c, content)
        want = R.rl_prior64(x, it, lam)
        assert torch.isfinite(want).all(), (h, w, c, it, lam, content)
        if content == "zeros":
            assert (x == 0).sum().item() >= 3 * (9 * 11 + 6 * 7) and torch.equal(want == 0, x == 0), (h, w, it, lam)
        if content == "signed":
            assert (x < 0).any() and (want[x < 0] == 0).all()
    for _, h, w, c, s, relu in R.bicubic_cases():
        assert torch.isfinite(R.bicubic64(R.bicubic_map(h, w, c), h, w, s, relu)).all()
    for m in R.LN_HOST_ROWS:
        for affine in (True, False):
            x, gm, bt, want1, want2 = R.ln_case(m, affine)
            assert torch.isfinite(want1).all() and torch.isfinite(want2).all()
            for kind, exact in (("zero", True), ("const7", True), ("gauss", False)):
                rows = torch.arange(m) % len(R.LN_KINDS) == R.LN_KINDS.index(kind)
                assert (want1[rows] == (bt.to(F64) if affine else 0.0)).all().item() == (exact or not rows.any().item())
    for name, h, w, shift in R.attn_cases():
        q, kv, rb = R.attn_operands(name, h, w)
        assert torch.isfinite(R.window_attention64(q, kv, rb, h, w, shift)).all()


def test_the_offset_set_needs_the_max_subtraction():
    """Its scores lie near 104: exp overflows in fp32 (exp(88.7) = inf) although the float64 softmax is fine."""
    q, kv, _ = R.attn_operands("offset", 5, 5)
    scores = (q[:, :32] @ kv[:, :32].t())
    assert scores.mean().item() > 100 and torch.isinf(torch.exp(scores)).all()


def test_the_bias_only_bias_is_neither_symmetric_nor_shared():
    rb = R.attn_operands("bias_only", 5, 5)[2]
    assert (rb - rb.transpose(1, 2)).abs().max().item() > 1 and (rb[0::2] - rb[1::2]).abs().max().item() > 1
    assert math.isclose(rb.std().item(), 3.0, rel_tol=0.05)
