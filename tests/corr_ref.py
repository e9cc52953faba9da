"""Exact-integer operands and float64 references for the correlation arg-max kernels (helper of test_corr_ref_cpu.py and
test_gpu_corr_exact.py; no GPU).

A score is one 9 C-term dot product of two 3x3 patches times a normaliser per reference position (and one per query).  The features here
are integers |x| <= 8, exact in bf16 AND f16, with every product and partial sum far below 2^24: whatever a kernel's order of summation
(the diagonal kernel's three row terms included), its fp32 dot product D[j,i] is the exact integer.  The normalisers are powers of two
2^-e, e random in {0,1,2,3}, handed to `Ctx.corr_plan` in place of `patch_invnorm`'s: R[j,i] = D[j,i] * inv_ref[j] and R[j,i] * inv_lr[i]
are exact too, and with max |D| < 2^18 they leave the low six mantissa bits clear, where the candidate kernels keep their position tag.  So
every arg-max kernel, in every arithmetic mode, has to return the float64 result itself: the checks below compare with torch.equal, no
tolerance.  Random exponents (not constant ones) are what expose a normaliser read at a neighbouring index.  inv_ref is never 0: that is
the slab kernel's mark for a row outside the map.

Exact ties are implementation-defined in the candidate kernels (include/speinet_hip.h), so `check_candidates` is written per query to hold
under any tie rule and demands index equality exactly where the reference has no tie; the top-1 kernels' contract is the lowest maximising
index, ties included (`check_top1`).  `check_preconditions` reads operands and reference only, never a kernel's output."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

AMP = 8
FAMILIES = ("random", "copy", "negative")
TAG_BITS = 6                         # low mantissa bits of a candidate key that carry the position tag (5 in the 32x32 folds, 6 elsewhere)
MAX_D = 1 << 18
COPY_SHARE_SAME, COPY_SHARE_LARGER = 0.95, 0.9
# Maps of one size on which a copy's own score is too weak to win under the smallest normaliser 2^-3, whatever the seed: maps of two or
# three rows (shift (1,1): the cyclic seam crosses every patch, at most six of nine taps match: 9216 / 8 against independent scores of
# sigma 665) and 64-channel maps (576 terms: 13824 / 8 = 3.0 sigma of the independent scores, below the largest of several hundred).
# The copies with e <= 2, three quarters of them, still win (13824 / 4 = 6 sigma): that share is asked for there.
COPY_SHARE_WEAK = 0.75
CHUNK = 2048                         # query columns per float64 score block of the chunked walks

Case = namedtuple("Case", "lr ref inv_lr inv_ref")
Top = namedtuple("Top", "v1 i1 v2 i2 v3")


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def copy_shift(hl, wl):
    return (3, 5) if hl > 3 and wl > 5 else (1, 1)


def copied_area(hl, wl, hr, wr):
    return min(hl, hr), min(wl, wr)


def maps(seed, hl, wl, hr, wr, family, amp=AMP, c=128):
    """Integer-valued fp32 lr [1,c,hl,wl] and ref [1,c,hr,wr], |x| <= amp.  "random": independent maps.  "copy": ref[y,x] =
    lr[(y-dy) % hl, (x-dx) % wl] on the area the two maps share, (dy,dx) = `copy_shift`; the rest of a larger reference map is
    independent integers (no tiling: that would plant exact ties) — each query's winner is then its shifted self, so nearly every
    reference position's full nine-tap score is observed as some query's maximum, the partial and edge blocks and the zero-padded border
    included.  "negative": lr >= 0 and ref <= 0, every score <= 0."""
    g = torch.Generator().manual_seed(seed)
    if family == "negative":
        return _ints(g, 0, amp, 1, c, hl, wl), -_ints(g, 0, amp, 1, c, hr, wr)
    lr, ref = _ints(g, -amp, amp, 1, c, hl, wl), _ints(g, -amp, amp, 1, c, hr, wr)
    if family == "copy":
        dy, dx = copy_shift(hl, wl)
        ch, cw = copied_area(hl, wl, hr, wr)
        ys, xs = (torch.arange(ch) - dy) % hl, (torch.arange(cw) - dx) % wl
        ref[:, :, :ch, :cw] = lr[:, :, ys][:, :, :, xs]
    else:
        assert family == "random", family
    return lr, ref


def pow2(seed, n, emax=3):
    """n normalisers 2^-e, e random in {0, ..., emax} (fp32)."""
    g = torch.Generator().manual_seed(seed)
    return torch.ldexp(torch.ones(n), -torch.randint(0, emax + 1, (n,), generator=g)).float()


def seed_of(hl, wl, hr, wr, family, c=128):
    return (((hl * 131 + wl) * 131 + hr) * 131 + wr) * 7 + FAMILIES.index(family) + 1000003 * (c != 128)


@functools.lru_cache(maxsize=16)
def case(hl, wl, hr, wr, family, c=128):
    """The operands of one GPU case: maps and power-of-two normalisers.  Do not modify the result."""
    s = seed_of(hl, wl, hr, wr, family, c)
    lr, ref = maps(s, hl, wl, hr, wr, family, c=c)
    return Case(lr, ref, pow2(s + 1, hl * wl), pow2(s + 2, hr * wr))


def patches(x, wrap_right=False):
    """float64 [c*9, h*w]: F.unfold(x, 3, padding=1) of a [1,c,h,w] map.  wrap_right: FAULT, no zero fill at the right edge — the tap
    right of the map's last column reads the next row's first pixel (zero after the last row)."""
    _, c, h, w = x.shape
    x = x[0].double()
    if not wrap_right:
        return F.unfold(x[None], 3, padding=1)[0]
    flat = F.pad(x, (0, 0, 1, 2)).reshape(c, -1)                    # rows only: one above, one below and a spare one for the last wrap
    xp = F.pad(x, (1, 1, 1, 1))
    taps = []
    for ky in range(3):
        for kx in range(3):
            if kx == 2:
                idx = (torch.arange(h)[:, None] + ky) * w + torch.arange(w)[None, :] + 1
                taps.append(flat[:, idx.reshape(-1)])
            else:
                taps.append(xp[:, ky:ky + h, kx:kx + w].reshape(c, -1))
    return torch.stack(taps, 1).reshape(c * 9, h * w)


def dots(lr, ref, cols=None):
    """float64 D [Nr, Nl] (or the query columns `cols`, a slice): D[j,i] = <P_ref[j], P_lr[i]>, one matmul of the two unfolds."""
    pl = patches(lr)
    return patches(ref).t() @ (pl if cols is None else pl[:, cols])


def scores(lr, ref, inv_ref, cols=None):
    """float64 R [Nr, Nl]: R[j,i] = D[j,i] * inv_ref[j]."""
    return dots(lr, ref, cols) * inv_ref.double()[:, None]


def topk(R, k):
    """The k best of every column of R [Nr, n] as ([values], [indices]), ordered by value descending then index ascending; past the Nr
    rows that exist: value -inf, index -1."""
    nr, n = R.shape
    work, cols = R.clone(), torch.arange(n)
    vals, idxs = [], []
    for t in range(k):
        if t >= nr:
            vals.append(torch.full((n,), float("-inf"), dtype=R.dtype))
            idxs.append(torch.full((n,), -1, dtype=torch.int64))
            continue
        v, i = work.max(0)                                          # torch.max(dim): the first of equal maxima (checked against a loop)
        work[i, cols] = float("-inf")
        vals.append(v)
        idxs.append(i)
    return vals, idxs


def top2(R):
    """v1, i1, v2, i2 of every column: the best and the runner-up by (value descending, index ascending); i2 = -1 and v2 = -inf when
    Nr == 1."""
    v, i = topk(R, 2)
    return v[0], i[0], v[1], i[1]


def top3(R):
    v, i = topk(R, 3)
    return Top(v[0], i[0], v[1], i[1], v[2])


def f32_bits(x):
    return x.contiguous().view(torch.int32)


def clear_tag(s):
    """fp32 candidate keys with the position tag (the low six mantissa bits) cleared."""
    return (f32_bits(s) & ~((1 << TAG_BITS) - 1)).view(torch.float32)


def exact_f32(x64):
    """x64 as fp32, asserting that nothing is rounded."""
    f = x64.float()
    assert torch.equal(f.double(), x64), "the reference is not exact in fp32: the case is built wrongly"
    return f


def column_chunks(n, chunk=CHUNK):
    return [slice(a, min(a + chunk, n)) for a in range(0, n, chunk)]


def check_preconditions(c, family):
    """What makes torch.equal a fair demand of every arg-max kernel on the case `c`: integer features exact in both 16-bit formats,
    power-of-two normalisers, max |D| < 2^18, every R and every R * inv_lr equal to its own fp32 value with the low six mantissa bits
    clear, and no three-way tie at the top of any column (two tied maxima are both among the two candidates, so the re-scored winner is
    the lowest index; with three a candidate pass may legitimately miss it).  "copy": the share of reference positions that are some
    query's winner is at least 0.95 on maps of one size, else at least 0.9 times the copied share of the reference area (0.75 in place
    of either factor where COPY_SHARE_WEAK applies).  Returns
    (max |D|, share of reference positions that win)."""
    lr, ref, inv_lr, inv_ref = c
    for t in (lr, ref):
        assert torch.equal(t, t.round()) and t.dtype == torch.float32, "features must be integers"
        for dt in (torch.bfloat16, torch.float16):
            assert torch.equal(t.to(dt).float(), t), f"a feature is not exact in {dt}"
    for inv in (inv_lr, inv_ref):
        m, _ = torch.frexp(inv)
        assert inv.dtype == torch.float32 and (m == 0.5).all() and (inv > 0).all(), "normalisers must be powers of two (never 0)"
    (hl, wl), (hr, wr) = lr.shape[2:], ref.shape[2:]
    nl, nr = hl * wl, hr * wr
    assert inv_lr.numel() == nl and inv_ref.numel() == nr
    low = (1 << TAG_BITS) - 1
    dmax, hit = 0.0, torch.zeros(nr, dtype=torch.bool)
    for cols in column_chunks(nl):
        D = dots(lr, ref, cols)
        dmax = max(dmax, D.abs().max().item())
        R = D * inv_ref.double()[:, None]
        for x in (R, R * inv_lr.double()[cols][None, :]):
            assert (f32_bits(exact_f32(x)) & low).eq(0).all(), "a score has low mantissa bits set"
        t = top3(R)
        assert not ((t.v1 == t.v3) & (t.v3 > float("-inf"))).any(), "a three-way tie at the top"
        hit[t.i1] = True
    assert dmax < MAX_D, f"max |D| = {dmax}"
    share = hit.double().mean().item()
    if family == "copy":
        same_size = (hl, wl) == (hr, wr)
        ch, cw = copied_area(hl, wl, hr, wr)
        weak = lr.shape[1] < 128 or (same_size and copy_shift(hl, wl) == (1, 1))
        if same_size:
            need = COPY_SHARE_WEAK if weak else COPY_SHARE_SAME
        else:
            need = (COPY_SHARE_WEAK if weak else COPY_SHARE_LARGER) * ch * cw / nr
        assert share >= need, f"only {share:.3f} of the reference positions win a query ({need:.3f} needed)"
    return dmax, share


def _fail(what, bad, n=8):
    idx = bad.nonzero().reshape(-1)
    raise AssertionError(f"{what}: {idx.numel()} of {bad.numel()} queries, first {idx[:n].tolist()}")


def _need(ok, what):
    if not ok.all():
        _fail(what, ~ok)


def check_candidates(R, S, arg, S2, arg2, top=None):
    """A candidate pass (spei_corr_slab_top2_16, spei_corr_diag_top2_16) against the float64 scores R [Nr, n], per query, under any tie
    rule.  S, S2 fp32 keys (tag bits are cleared here), arg, arg2 int32, CPU tensors of n queries.  `top`: top3(R), if at hand."""
    nr, n = R.shape
    t = top3(R) if top is None else top
    S, S2, arg, arg2 = clear_tag(S.cpu()), clear_tag(S2.cpu()), arg.cpu().long(), arg2.cpu().long()
    assert S.shape == S2.shape == arg.shape == arg2.shape == (n,)
    _need((arg >= 0) & (arg < nr), "arg outside the reference map")
    ra = R.gather(0, arg.clamp(0, nr - 1)[None])[0]
    _need(ra == t.v1, "the winner's score is not the maximum")
    _need(S == exact_f32(t.v1), "S is not the winner's score")
    if nr == 1:
        _need(arg2 == -1, "arg2 must be -1 with a single reference position")
        _need(S2 == float("-inf"), "S2 must be -inf without a runner-up")
    else:
        _need((arg2 >= 0) & (arg2 < nr), "arg2 outside the reference map (or -1 although a runner-up exists)")
        _need(arg2 != arg, "the runner-up is the winner again")
        r2 = R.gather(0, arg2.clamp(0, nr - 1)[None])[0]
        _need(r2 == t.v2, "the runner-up's score is not the second best")
        _need(S2 == exact_f32(t.v2), "S2 is not the runner-up's score")
    clear1 = t.v1 > t.v2
    _need(~clear1 | (arg == t.i1), "arg differs from the only maximum")
    _need(~(clear1 & (t.v2 > t.v3)) | (arg2 == t.i2), "arg2 differs from the only second best")


def check_top1(R, inv_lr, S, arg, top=None):
    """A top-1 kernel, or the re-scored result of the top-2 form: S == fp32(R[arg] * inv_lr), R[arg] the maximum, and arg the LOWEST
    maximising index everywhere, ties included (the contract of spei_corr_argmax and of `better()`)."""
    nr, n = R.shape
    t = top3(R) if top is None else top
    S, arg = S.cpu(), arg.cpu().long()
    assert S.shape == arg.shape == (n,) and S.dtype == torch.float32
    _need((arg >= 0) & (arg < nr), "arg outside the reference map")
    ra = R.gather(0, arg.clamp(0, nr - 1)[None])[0]
    _need(ra == t.v1, "the winner's score is not the maximum")
    _need(f32_bits(S) == f32_bits(exact_f32(ra * inv_lr.double())), "S is not fp32(R[arg] * inv_lr)")
    _need(arg == t.i1, "arg is not the lowest maximising index")


def reference_pass(R):
    """What a correct candidate pass returns for R (fp32 S, int32 arg, S2, arg2) — the faulty passes of test_corr_ref_cpu.py start here."""
    v1, i1, v2, i2 = top2(R)
    return v1.float(), i1.int(), v2.float(), i2.int()


def tie_case(hl=12, wl=20, seed=77, c=128):
    """The planted-tie case of the top-1 kernels: the query map twice in the reference map, each copy framed by zero rows and columns (as
    the zero padding frames the query map), with the same normalisers — every reference position of the first copy has a twin of exactly
    equal score 13 rows below, in another reference block of every kernel (exponents 0 and 1 only: a copy's own score then wins on 64
    channels too, so the two maxima of every query are the twins).  Returns a Case with ref [1,c,2 hl + 3, wl + 2]."""
    g = torch.Generator().manual_seed(seed)
    lr = _ints(g, -AMP, AMP, 1, c, hl, wl)
    hr, wr = 2 * hl + 3, wl + 2
    ref = torch.zeros(1, c, hr, wr)
    ref[:, :, 1:1 + hl, 1:1 + wl] = lr
    ref[:, :, hl + 2:2 * hl + 2, 1:1 + wl] = lr
    inv_ref = pow2(seed + 2, hr * wr, 1).reshape(hr, wr)
    inv_ref[hl + 1:2 * hl + 3] = inv_ref[:hl + 2].clone()           # the second copy and its frame rows: the first one's normalisers
    return Case(lr, ref, pow2(seed + 1, hl * wl), inv_ref.reshape(-1).contiguous())


# ---- the case tables, shared by the CPU and the GPU file -------------------------------------------------------------------------------
# (hl, wl, hr, wr)
CAND_BOTH = [(20, 30, 20, 30), (37, 45, 37, 45), (3, 3, 3, 3), (1, 5, 9, 3), (2, 70, 2, 70), (5, 65, 5, 65), (29, 51, 37, 45),
             (20, 70, 70, 20)]
CAND_SLAB = [(37, 45, 29, 51), (4, 32, 40, 70), (9, 33, 1, 1)]
CAND_DIAG = [(12, 130, 13, 66), (7, 69, 7, 69)]           # 69: the last tile holds 5 reference columns, one lane quad and a single position
CAND_DIAG_LARGE = (48, 320, 48, 320)                               # f16 only: the walk is cut into segments
TOP1_SHAPES = [(20, 30, 20, 30), (37, 45, 29, 51), (15, 20, 15, 20), (4, 32, 40, 70)]
TOP1_FAMILIES = ("random", "copy")
RESCORE_SHAPE = (37, 45, 29, 51)


def candidate_cases():
    """(kernel, shape, formats) of every candidate-pass case."""
    for s in CAND_BOTH:
        yield "slab", s, ("bf16", "f16")
        yield "diag", s, ("bf16", "f16")
    for s in CAND_SLAB:
        yield "slab", s, ("bf16", "f16")
    for s in CAND_DIAG:
        yield "diag", s, ("bf16", "f16")
    yield "diag", CAND_DIAG_LARGE, ("f16",)


def gpu_cases():
    """(label, Case, family) of every exact-operand case of test_gpu_corr_exact.py, each once."""
    seen = set()
    for _, s, _ in candidate_cases():
        for fam in FAMILIES:
            if (s, fam) not in seen:
                seen.add((s, fam))
                yield f"candidates {s} {fam}", case(*s, fam), fam
    for s in TOP1_SHAPES:
        for fam in TOP1_FAMILIES:
            if (s, fam) not in seen:
                seen.add((s, fam))
                yield f"top1 {s} {fam}", case(*s, fam), fam
            yield f"top1 C=64 {s} {fam}", case(*s, fam, 64), fam
    yield "rescore", case(*RESCORE_SHAPE, "random"), "random"
