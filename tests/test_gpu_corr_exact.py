"""GPU suite: the correlation arg-max kernels bit for bit on exact integer operands (tests/corr_ref.py).

The features are small integers and the normalisers powers of two (handed to Ctx.corr_plan in place of patch_invnorm's), so every score
any kernel forms is exact in fp32 and every kernel — the f32 MFMA kernel, the slab and tile-restaging top-1 kernels in bf16, f16 and
bf16x3, the two candidate kernels in bf16 and f16 — must return the float64 scores and indices themselves.  The candidate kernels' own
outputs (S, arg, S2, arg2 before the re-score) are checked per query under any tie rule; the top-1 kernels and the re-scored result must
name the lowest maximising index.  Every comparison is torch.equal; the one tolerance of the file is patch_invnorm's, on real-valued
data.  test_corr_ref_cpu.py checks the conditions of every case of this file, and that the checks see a dropped tap, a wrong halo, a
normaliser of the neighbouring position, a missing or doubled runner-up, a lost split and a wrong low bit.  Each case asserts which C-ABI
entry point took the call and the 16-bit format it was given."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import corr_ref as R                              # noqa: E402
from speinet_amd import _lib, pack                # noqa: E402
from speinet_amd.ops import Ctx, FMap             # noqa: E402

DEV = "cuda:0"
FMT = {"bf16": pack.BF16, "f16": pack.F16}
LP = {"bf16": torch.bfloat16, "f16": torch.float16}


class Spy:
    """Counts the launches of one C-ABI entry point and keeps the arguments of the last one."""
    def __init__(self, monkeypatch, name):
        lib = _lib.lib()
        self.n, self.args, fn = 0, None, getattr(lib, name)

        def call(*a):
            self.n += 1
            self.args = a
            return fn(*a)
        monkeypatch.setattr(lib, name, call)


ENTRIES = ("spei_corr_argmax", "spei_corr_argmax_bf16", "spei_corr_slab16", "spei_corr_slab_top2_16", "spei_corr_diag_top2_16",
           "spei_corr_rescore")


def spies(monkeypatch):
    return {n: Spy(monkeypatch, n) for n in ENTRIES}


def took(sp, counts):
    """Exactly these launches were made since the spies were set."""
    assert {n: s.n for n, s in sp.items() if s.n} == counts, "another kernel took the call"


def null(p):
    return p.value is None


def fm(x):
    """[1,c,h,w] on the host -> the kernels' NHWC map on the device."""
    _, c, h, w = x.shape
    return FMap(x[0].permute(1, 2, 0).reshape(h * w, c).contiguous().to(DEV), h, w, c)


def run(entries, ops):
    for fn, name, args in entries:
        _lib.check(fn(*args, ops._stream()), name)


def plan_of(ops, c):
    return ops.corr_plan(fm(c.lr), fm(c.ref), c.inv_lr.to(DEV), c.inv_ref.to(DEV))


@functools.lru_cache(maxsize=6)
def _cached_blocks(c_key):
    return list(_blocks(R.case(*c_key)))


def _blocks(c):
    for cols in R.column_chunks(c.inv_lr.numel()):
        Rm = R.scores(c.lr, c.ref, c.inv_ref, cols)
        yield cols, Rm, R.top3(Rm)


def blocks(key):
    """(query columns, float64 scores, their top three) of the case `key` = the arguments of corr_ref.case, computed once and shared by
    the kernels and formats of a shape; the large case block by block, not kept."""
    hl, wl, hr, wr = key[:4]
    return _cached_blocks(key) if hl * wl * hr * wr <= 1 << 23 else _blocks(R.case(*key))


def labelled(label, check, *a, **kw):
    try:
        check(*a, **kw)
    except AssertionError as e:
        raise AssertionError(f"{label}: {e}") from None


# ---- candidate kernels ----------------------------------------------------------------------------------------------------------------------
CAND = {"slab": ("spei_corr_slab_top2_16", "corr_slab_kernel<top2, "), "diag": ("spei_corr_diag_top2_16", "corr_diag_kernel<top2, ")}


def candidate_case(kernel, shape, fmt, family, monkeypatch):
    entry, kname = CAND[kernel]
    key = (*shape, family)
    c = R.case(*key)
    sp = spies(monkeypatch)
    ops = Ctx(fmt, "top2", device=DEV, corr_bf16=False, corr_diag=kernel == "diag")
    plan = plan_of(ops, c)
    assert plan.kernel == f"{kname}{fmt}>", plan.kernel
    s2, arg2 = plan.keep[6], plan.keep[7]
    # the candidate pass alone: its own four outputs, before the re-score overwrites S and arg
    run(plan.main, ops)
    torch.cuda.synchronize()
    took(sp, {entry: 1})
    assert sp[entry].args[0] == FMT[fmt], "the candidate kernel was given another 16-bit format"
    cand = [t.cpu().clone() for t in (plan.s, plan.arg, s2, arg2)]
    run(plan.post, ops)
    torch.cuda.synchronize()
    took(sp, {entry: 1, "spei_corr_rescore": 1})
    s, arg = plan.s.cpu(), plan.arg.cpu()
    label = f"{entry} {fmt} {shape} {family}"
    for cols, Rm, top in blocks(key):
        labelled(label, R.check_candidates, Rm, *(t[cols] for t in cand), top=top)
        labelled(label + " re-scored", R.check_top1, Rm, c.inv_lr[cols], s[cols], arg[cols], top=top)


CAND_PARAMS = [(k, s, f) for k, s, fmts in R.candidate_cases() if s != R.CAND_DIAG_LARGE for f in fmts]


@pytest.mark.parametrize("kernel,shape,fmt", CAND_PARAMS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_candidate_kernels_exact(kernel, shape, fmt, monkeypatch):
    """S, arg, S2, arg2 of the slab and the diagonal candidate kernel in bf16 and in f16 (corr_bf16=False), then the re-scored result, on
    the three families: maps of one size, smaller than a tile, single rows, one pixel past a tile, a larger, a rotated and (slab) a
    lower reference map, one query tile against 15 reference blocks merged across splits, a single reference position; (diagonal) a
    last reference tile of one and of five columns."""
    for family in R.FAMILIES:
        candidate_case(kernel, shape, fmt, family, monkeypatch)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_diag_candidates_exact_segmented_walk(family, monkeypatch):
    """48 x 320 in f16: five tiles per row, the walk down the query rows cut into segments (the one large case of the file)."""
    candidate_case("diag", R.CAND_DIAG_LARGE, "f16", family, monkeypatch)


# ---- top-1 kernels --------------------------------------------------------------------------------------------------------------------------
# form -> (precision, corr_precision, entry point, channels, 16-bit format or None, split)
TOP1 = {"f32": ("f32", "bf16x3", "spei_corr_argmax", 128, None, False),
        "slab bf16": ("bf16", "single", "spei_corr_slab16", 128, "bf16", False),
        "slab f16": ("f16", "single", "spei_corr_slab16", 128, "f16", False),
        "slab bf16x3": ("bf16x3", "bf16x3", "spei_corr_slab16", 128, "bf16", True),
        "tile bf16": ("bf16", "single", "spei_corr_argmax_bf16", 64, "bf16", False),
        "tile bf16x3": ("bf16x3", "bf16x3", "spei_corr_argmax_bf16", 64, "bf16", True)}


def top1_case(form, c, blks, label, monkeypatch):
    precision, corr, entry, ch, fmt, split = TOP1[form]
    assert c.lr.shape[1] == ch
    sp = spies(monkeypatch)
    ops = Ctx(precision, corr, device=DEV)
    plan = plan_of(ops, c)
    assert not plan.post
    plan.launch()
    torch.cuda.synchronize()
    took(sp, {entry: 1})
    a = sp[entry].args
    if entry == "spei_corr_slab16":
        assert a[0] == FMT[fmt] and null(a[2]) == null(a[4]) == (not split)
    elif entry == "spei_corr_argmax_bf16":
        assert null(a[1]) == null(a[3]) == (not split) and a[10] == 64
    s, arg = plan.s.cpu(), plan.arg.cpu()
    for cols, Rm, top in blks:
        labelled(f"{entry} {form} {label}", R.check_top1, Rm, c.inv_lr[cols], s[cols], arg[cols], top=top)


@pytest.mark.parametrize("shape", R.TOP1_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", list(TOP1))
def test_top1_kernels_exact(form, shape, monkeypatch):
    """spei_corr_argmax (f32), spei_corr_slab16 (single bf16, single f16, bf16x3) and spei_corr_argmax_bf16 (64 channels; single, bf16x3):
    S == fp32(R[arg] * inv_lr) and arg the lowest maximising index, on independent maps and on the shifted copy."""
    for family in R.TOP1_FAMILIES:
        key = (*shape, family, TOP1[form][3])
        top1_case(form, R.case(*key), blocks(key), f"{shape} {family}", monkeypatch)


@functools.lru_cache(maxsize=2)
def tie_blocks(ch):
    c = R.tie_case(c=ch)
    return c, list(_blocks(c))


@pytest.mark.parametrize("form", list(TOP1))
def test_top1_planted_ties(form, monkeypatch):
    """Every query has two exactly equal maxima, 13 reference rows apart (other reference blocks, other splits): the lower index wins."""
    c, blks = tie_blocks(TOP1[form][3])
    for _, _, top in blks:
        assert (top.v1 == top.v2).all() and (top.v2 > top.v3).all()
    top1_case(form, c, blks, "planted ties", monkeypatch)


# ---- spei_corr_rescore alone ------------------------------------------------------------------------------------------------------------------
def draw_candidates(g, n, hr, wr):
    """n reference positions, a third of them on the map's border rows and columns."""
    pos = torch.arange(hr * wr)
    y, x = pos // wr, pos % wr
    border = pos[(y == 0) | (y == hr - 1) | (x == 0) | (x == wr - 1)]
    anywhere = torch.randint(0, hr * wr, (n,), generator=g)
    on_border = border[torch.randint(0, border.numel(), (n,), generator=g)]
    return torch.where(torch.arange(n) % 3 == 0, on_border, anywhere).int()


def rescore(c, arg, arg2):
    """spei_corr_rescore on the candidates (arg, arg2) -> (S, arg) on the host."""
    ops = Ctx("f16", "top2", device=DEV)
    lr, ref = fm(c.lr), fm(c.ref)
    n = lr.H * lr.W
    tp = ops._tp
    s = torch.full((n,), float("nan"), device=DEV)
    a, a2 = arg.to(DEV).contiguous(), arg2.to(DEV).contiguous()
    inv_lr, inv_ref = c.inv_lr.to(DEV), c.inv_ref.to(DEV)
    s2 = torch.zeros(n, device=DEV)
    _lib.check(_lib.lib().spei_corr_rescore(ops._fp(lr), lr.ld, ops._fp(ref), ref.ld, tp(inv_lr), tp(inv_ref), lr.H, lr.W, ref.H, ref.W,
                                            lr.C, tp(s), tp(a), tp(s2), tp(a2), ops._stream()), "spei_corr_rescore")
    torch.cuda.synchronize()
    return s.cpu(), a.cpu()


def rescore_expected(Rm, arg, arg2):
    """The winner of two candidates on float64 scores: the higher score, the lower index between equal ones; arg2 = -1: arg."""
    arg, arg2 = arg.long(), arg2.long()
    r0 = Rm.gather(0, arg[None])[0]
    r1 = torch.where(arg2 >= 0, Rm.gather(0, arg2.clamp(min=0)[None])[0], torch.full_like(r0, float("-inf")))
    second = (arg2 >= 0) & ((r1 > r0) | ((r1 == r0) & (arg2 < arg)))
    win = torch.where(second, arg2, arg)
    return Rm.gather(0, win[None])[0], win


def test_rescore_exact():
    """spei_corr_rescore on hand-made candidates, 37x45 queries against a 29x51 map: no second candidate, the true winner second and a
    poor one first, two equal-scoring candidates in either order (the lower index wins), the same candidate twice."""
    hl, wl, hr, wr = R.RESCORE_SHAPE
    c = R.case(hl, wl, hr, wr, "random")
    Rm = R.scores(c.lr, c.ref, c.inv_ref)
    n = hl * wl
    g = torch.Generator().manual_seed(11)
    rnd = draw_candidates(g, n, hr, wr)
    v1, i1, _, _ = R.top2(Rm)
    # two positions of exactly equal score per query: neighbours in the sorted column (scores are multiples of 1/8 in a narrow range)
    sv, si = torch.sort(Rm, dim=0, stable=True)
    eq = sv[1:] == sv[:-1]
    assert eq.any(0).float().mean().item() > 0.9
    k = eq.int().argmax(0)
    lo, hi = si.gather(0, k[None])[0].int(), si.gather(0, (k + 1)[None])[0].int()
    swap = torch.arange(n) % 2 == 0
    cases = {"no second candidate": (rnd, torch.full_like(rnd, -1)),
             "the true winner second": (rnd, i1.int()),
             "equal scores": (torch.where(swap, hi, lo), torch.where(swap, lo, hi)),
             "the same candidate twice": (rnd, rnd.clone())}
    for label, (arg, arg2) in cases.items():
        want_r, want_arg = rescore_expected(Rm, arg, arg2)
        if label == "the true winner second":
            assert torch.equal(want_arg, i1)
        if label == "equal scores":
            tied = eq.any(0)
            assert torch.equal(want_arg[tied], torch.minimum(lo, hi).long()[tied])
        s, a = rescore(c, arg, arg2)
        assert torch.equal(a.long(), want_arg), label
        assert torch.equal(s, R.exact_f32(want_r * c.inv_lr.double())), label


def test_rescore_gaussian_against_float64():
    """Real-valued maps and normalisers: S is the float64 score (dot * inv_ref[j]) * inv_lr[i] of the winner rounded once to fp32 — the
    kernel's order of the two normaliser products, mirrored here — and the winner is float64's."""
    hl, wl, hr, wr = R.RESCORE_SHAPE
    g = torch.Generator().manual_seed(12)
    lr, ref = torch.randn(1, 128, hl, wl, generator=g), torch.randn(1, 128, hr, wr, generator=g)
    pl, pr = R.patches(lr), R.patches(ref)
    c = R.Case(lr, ref, (1 / pl.norm(dim=0)).float(), (1 / pr.norm(dim=0)).float())
    n = hl * wl
    arg, arg2 = draw_candidates(g, n, hr, wr), draw_candidates(g, n, hr, wr)
    sc = [(pr[:, a.long()] * pl).sum(0) * c.inv_ref.double()[a.long()] for a in (arg, arg2)]
    assert (sc[0] != sc[1]).all() or (arg == arg2)[sc[0] == sc[1]].all()
    second = (sc[1] > sc[0]) | ((sc[1] == sc[0]) & (arg2 < arg))
    s, a = rescore(c, arg, arg2)
    assert torch.equal(a, torch.where(second, arg2, arg))
    assert torch.equal(s, (torch.where(second, sc[1], sc[0]) * c.inv_lr.double()).float())


# ---- spei_split16 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("m,ld", [(1, 128), (63, 128), (1000, 128), (63, 160)])
def test_split16_exact(m, ld, fmt):
    """hi = fmt(x) and lo = fmt(x - hi), each rounded once to nearest even; a row pitch above C; lo = NULL."""
    ops = Ctx("f32", device=DEV)
    dt = LP[fmt]
    buf = torch.randn(m, ld, generator=torch.Generator().manual_seed(m + ld)).to(DEV)
    x = buf[:, :128]
    want_hi = x.to(dt)
    want_lo = (x - want_hi.float()).to(dt)
    for with_lo in (True, False):
        hi = torch.full((m, 128), float("nan"), device=DEV, dtype=dt)
        lo = torch.full((m, 128), float("nan"), device=DEV, dtype=dt) if with_lo else None
        _lib.check(_lib.lib().spei_split16(FMT[fmt], ops._tp(buf), ld, ops._tp(hi), ops._tp(lo), m, 128, ops._stream()), "spei_split16")
        torch.cuda.synchronize()
        assert torch.equal(hi, want_hi)
        if with_lo:
            assert torch.equal(lo, want_lo)


# ---- spei_gather_fold -------------------------------------------------------------------------------------------------------------------------
def fold_args():
    """arg over the 5 x 11 reference map for 7 x 9 queries: the four corners and a position inside every border row and column first,
    the rest uniform; shuffled."""
    h3, w3, hr3, wr3 = 7, 9, 5, 11
    g = torch.Generator().manual_seed(13)
    forced = [0, wr3 - 1, (hr3 - 1) * wr3, hr3 * wr3 - 1, 4, (hr3 - 1) * wr3 + 6, 2 * wr3, 3 * wr3 - 1]
    arg = torch.cat((torch.tensor(forced), torch.randint(0, hr3 * wr3, (h3 * w3 - len(forced),), generator=g)))
    arg = arg[torch.randperm(h3 * w3, generator=g)]
    y, x = arg // wr3, arg % wr3
    assert all(((y == r).any() for r in (0, hr3 - 1))) and all(((x == q).any() for q in (0, wr3 - 1)))
    return h3, w3, hr3, wr3, arg


@pytest.mark.parametrize("s,ch", [(1, 128), (2, 64), (4, 32)])
def test_gather_fold_exact(s, ch):
    """unfold -> gather -> fold / 9 (model/SearchTransfer.py:36-46) in float64 on a map of multiples of 9 (the division is exact), with
    patches taken from the corners and borders of the reference map, where they reach into its zero padding."""
    h3, w3, hr3, wr3, arg = fold_args()
    g = torch.Generator().manual_seed(14 + s)
    ref = 9.0 * torch.randint(-7, 8, (1, ch, hr3 * s, wr3 * s), generator=g).float()
    unf = F.unfold(ref.double(), 3 * s, padding=s, stride=s)
    t = unf.gather(2, arg.view(1, 1, -1).expand(1, unf.shape[1], -1))
    want = F.fold(t, (h3 * s, w3 * s), 3 * s, padding=s, stride=s) / 9.0
    out = Ctx("f32", device=DEV).gather_fold(fm(ref), arg.int().to(DEV), h3, w3, hr3, wr3, s)
    assert (out.H, out.W, out.C) == (h3 * s, w3 * s, ch)
    assert torch.equal(out.nchw().cpu(), R.exact_f32(want))


# ---- spei_rot90, spei_patch_invnorm -----------------------------------------------------------------------------------------------------------
def test_rot90_exact():
    x = torch.randn(1, 128, 7, 33, generator=torch.Generator().manual_seed(15))
    out = Ctx("f32", device=DEV).rot90(fm(x))
    assert (out.H, out.W) == (33, 7)
    assert torch.equal(out.nchw().cpu(), x.transpose(2, 3).flip(2))


def test_patch_invnorm_of_a_zero_neighbourhood():
    """An all-zero 3x3 neighbourhood: exactly 1 / 1e-12 (F.normalize's eps), inside the map and in a corner."""
    x = torch.randn(1, 128, 9, 12, generator=torch.Generator().manual_seed(16))
    x[:, :, 3:6, 4:7] = 0
    x[:, :, :2, :2] = 0
    inv = Ctx("f32", device=DEV).patch_invnorm(fm(x)).cpu().reshape(9, 12)
    want = torch.tensor(1e12, dtype=torch.float32)
    assert inv[4, 5] == want and inv[0, 0] == want
    assert torch.isfinite(inv).all() and (inv[inv != want] < 1).all()


def test_patch_invnorm_against_float64():
    """Gaussian 17 x 35: the largest relative error against float64 1 / max(norm, 1e-12) is at most four times what the reference's own
    order of summation gives in fp32 on the host (a float32 norm of the unfolded patches against float64).  Measured on the MI355X:
    1.24e-7 for the kernel, 7.78e-7 for float32 on the host (bound 3.1e-6)."""
    x = torch.randn(1, 128, 17, 35, generator=torch.Generator().manual_seed(17))
    want = 1 / R.patches(x).norm(dim=0).clamp(min=1e-12)
    host = 1 / F.unfold(x, 3, padding=1)[0].norm(dim=0).clamp(min=1e-12)
    host_err = ((host.double() - want) / want).abs().max().item()
    inv = Ctx("f32", device=DEV).patch_invnorm(fm(x)).cpu()
    err = ((inv.double() - want) / want).abs().max().item()
    print(f"patch_invnorm: max relative error {err:.3e}; float32 on the host {host_err:.3e}")
    assert host_err > 0 and err <= 4 * host_err
