"""CPU suite for tests/gates_ref.py, the float64 statement the GPU tests of csrc/resblock.hip compare with (test_gpu_gates.py): it
agrees with the fp32 oracle, its derived bound holds for an fp32 evaluation in another summation order with room to spare, and the
case table it shares with the GPU test sees each defect model -- the evidence that the GPU test would fail on a subtly wrong kernel."""
import numpy as np
import pytest
import torch

import gates_ref as R
from oracle import speinet_oracle as O
from speinet_amd import pack

BLOCK = {32: "recons_net.inBlock.1.", 64: "recons_net.encoder_first.1.", 128: "recons_net.encoder_second.1."}
SMALL_ROWS = ("degenerate", "one_tile", "column_tiles", "row_tiles", "block_boundary")
OUTPUTS = ("s", "g1", "g2")


def params(synth_sd, c):
    return R.pk64(pack.resblock(synth_sd, BLOCK[c]))


def ratios(got, ref):
    return {n: float((np.abs(g - getattr(ref, n)) / getattr(ref, "tol_" + n)).max()) for g, n in zip(got, OUTPUTS)}


@pytest.mark.parametrize("c", R.CHANNELS)
def test_reference_vs_fp32_oracle(synth_sd, c):
    """`oracle.speinet_oracle.resblock_gates` (fp32 torch, pinned by the reference's golden vectors) on every small shape of the table,
    gauss and neg: its distance from the float64 statement stays within the bound of an fp32 evaluation."""
    pk, worst = params(synth_sd, c), dict.fromkeys(OUTPUTS, 0.0)
    for row in SMALL_ROWS:
        for i, (h, w) in enumerate(R.ROWS[row][1](c, "fp32")):
            for fam in ("gauss", "neg"):
                x1 = R.content(fam, h, w, c, "fp32", 7 * h + w + i)
                ref = R.gates_f64(x1, pk)
                s, g1, g2 = O.resblock_gates(torch.from_numpy(x1).float().permute(2, 0, 1)[None], synth_sd, BLOCK[c])
                got = (s.view(c), g1[0, :, :, 0].t(), g2[0, :, 0, :].t())                    # ours: [C], [H][C], [W][C]
                rt = ratios([t.double().numpy() for t in got], ref)
                assert max(rt.values()) <= 1.0, (row, h, w, fam, rt)
                worst = {n: max(worst[n], rt[n]) for n in OUTPUTS}
    print(f"C={c}: largest |oracle - float64| / tol " + " ".join(f"{n}={v:.3f}" for n, v in worst.items()))


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("c", R.CHANNELS)
def test_bound_holds_for_another_summation_order(synth_sd, c, fmt):
    """fp32 numpy with sequential line sums and unfused products -- not the kernel's order -- on every case of the table.  Measured:
    at most 0.27 of the bound at C = 32, 0.11 at C = 64 and 0.06 at C = 128; the largest figures come from the integer content of the SE
    row, whose bound has no length terms while the unfused chain rounds each tap twice."""
    pk, worst = params(synth_sd, c), 0.0
    for row in R.ROWS:
        for h, w, fam, exact, seed in R.cases(row, c, fmt):
            x1 = R.content(fam, h, w, c, fmt, seed)
            rt = ratios(R.gates_fp32_sequential(x1, pk), R.gates_f64(x1, pk, exact))
            assert max(rt.values()) <= 1.0, (row, h, w, fam, rt)
            worst = max(worst, *rt.values())
    print(f"C={c} {fmt}: largest |fp32 sequential - float64| / tol = {worst:.3f}")


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("c", R.CHANNELS)
def test_every_defect_exceeds_the_bound(synth_sd, c, fmt):
    """Each defect model, applied to the float64 statement, leaves the bound on at least one content family of every row of the table
    in which it can occur (a mask defect needs a ragged tile, swapped denominators H != W), and on the family it names wherever a row
    holds that family.  Measured over all C and formats, smallest of the per-row largest |defect - float64| / tol: zeros in the column
    maxima 17 005, in the row maxima 3 214, row mean without its last column 44, column mean without its last row 608, denominators
    swapped 37 487, SE mean without its last tile 8 (a ragged last tile is a single pixel; 50 and more on the SE row), halo line 30 824."""
    pk = params(synth_sd, c)
    least = {}
    for row, (fams, shapes) in R.ROWS.items():
        seen = {}
        for h, w, fam, exact, seed in R.cases(row, c, fmt):
            x1 = R.content(fam, h, w, c, fmt, seed)
            ref = R.gates_f64(x1, pk, exact)
            for name, (_, named, applies) in R.DEFECTS.items():
                if applies(h, w, c, fmt):
                    d = seen.setdefault(name, {})
                    d[fam] = max(d.get(fam, 0.0), R.exceeds(R.gates_with_defect(name, x1, pk, c, fmt), ref))
        for name, by_family in seen.items():
            named = R.DEFECTS[name][1]
            assert max(by_family.values()) > 1.0, (name, row, by_family)
            if named in fams:
                assert by_family[named] > 1.0, (name, row, by_family)
            least[name] = min(least.get(name, np.inf), max(by_family.values()))
    assert set(least) == set(R.DEFECTS)
    print(f"C={c} {fmt}: " + " ".join(f"{n}={v:.0f}" for n, v in least.items()))


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("c", R.CHANNELS)
def test_a_map_that_reads_map_zero_exceeds_the_bound(synth_sd, c, fmt):
    """The batched cases: map b > 0 given map 0's gates (a workspace slice or an output offset that ignores the map index)."""
    pk = params(synth_sd, c)
    for row, i in R.BATCHED:
        h, w = R.ROWS[row][1](c, fmt)[i]
        maps = [R.gates_f64(R.content(fam, h, w, c, fmt, 50 + j), pk) for j, fam in enumerate(R.BATCHED_FAMILIES)]
        for b in (1, 2):
            for n in OUTPUTS:
                over = float((np.abs(getattr(maps[0], n) - getattr(maps[b], n)) / getattr(maps[b], "tol_" + n)).max())
                assert over > 100.0, (row, b, n, over)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_contents_are_what_they_claim(fmt):
    c = 32
    tr, tc = R.tile_rows(fmt), R.tile_cols(c)
    h, w = 2 * tr + 1, tc + 3
    for fam in ("gauss", "neg", "ints", "planted", "flat"):
        x = R.content(fam, h, w, c, fmt, 3)
        assert x.shape == (h, w, c) and np.array_equal(R.round_to(x, fmt), x), fam
        assert np.array_equal(x, R.content(fam, h, w, c, fmt, 3)), fam
    neg = R.content("neg", h, w, c, fmt, 3)
    assert (neg <= -0.5).all()
    ints = R.content("ints", h, w, c, fmt, 3)
    assert np.array_equal(ints, np.round(ints)) and ints.min() == -8 and ints.max() == 8
    flat = R.content("flat", h, w, c, fmt, 3)
    assert (flat == flat[0, 0]).all() and np.array_equal(flat.max(axis=1), flat.mean(axis=1))
    p = R.content("planted", h, w, c, fmt, 3)
    assert (p < 0).all()
    rows_at, cols_at = set(), set()
    for ch in range(0, c, 2):                       # row lines: exactly one value above -1/2, at one of the three positions
        assert ((p[:, :, ch] > -0.5).sum(axis=1) == 1).all()
        rows_at |= set(p[:, :, ch].argmax(axis=1))
    for ch in range(1, c, 2):
        assert ((p[:, :, ch] > -0.5).sum(axis=0) == 1).all()
        cols_at |= set(p[:, :, ch].argmax(axis=0))
    assert rows_at == {w - 1, tc, 0} and cols_at == {h - 1, 2 * tr, 0}


def test_bf16_rounding_is_round_to_nearest_even():
    x = np.random.RandomState(0).randn(4096) * np.exp(np.random.RandomState(1).randn(4096) * 3)
    x = np.concatenate([x, [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.0, 0.0]])            # two ties: down to even, up to even
    want = torch.from_numpy(x).float().to(torch.bfloat16).double().numpy()
    assert np.array_equal(R.round_to(x, "bf16"), want)
    assert np.array_equal(R.round_to(x, "f16"), torch.from_numpy(x).float().to(torch.float16).double().numpy())


@pytest.mark.parametrize("extra", [False, True])
def test_apply_statements(extra):
    """The int64 and float64 statements of the gated sum agree on integer operands, an exchange of two indices changes the result, and
    an fp32 evaluation in another order (the sum of the gates first) stays within the bound on Gaussian operands."""
    b, h, w, c = 2, 5, 5, 32
    x, x1, s, g1, g2, e = R.apply_ints(b, h, w, c, 5, extra)
    for m in range(b):
        want = R.apply_i64(x[m], x1[m], s[m], g1[m], g2[m], None if e is None else e[m])
        out, _ = R.apply_f64(x[m], x1[m], s[m], g1[m], g2[m], None if e is None else e[m])
        assert np.array_equal(out, want.astype(np.float64))
        o = 1 - m
        wrong = (R.apply_i64(x[m], x1[m], s[m], g2[m], g1[m]), R.apply_i64(x[m], x1[m], s[m, ::-1], g1[m], g2[m]),
                 R.apply_i64(x[m], x1[m], s[m], g1[m].T.reshape(h, c), g2[m]), R.apply_i64(x[m], x1[m], s[o], g1[m], g2[m]),
                 R.apply_i64(x[m], x1[m], s[m], g1[o], g2[m]), R.apply_i64(x[m], x1[m], s[m], g1[m], g2[o]),
                 R.apply_i64(x[m], x1[o], s[m], g1[m], g2[m]), R.apply_i64(x1[m], x[m], s[m], g1[m], g2[m]))
        base = R.apply_i64(x[m], x1[m], s[m], g1[m], g2[m])
        assert all((v != base).mean() > 0.5 for v in wrong)
    for fmt in R.FORMATS:
        x, x1, s, g1, g2, e = (None if t is None else t[0] for t in R.apply_gauss(1, 17, 33, 64, fmt, 9, extra))
        out, tol = R.apply_f64(x, x1, s, g1, g2, e)
        f = np.float32
        got = x.astype(f) + x1.astype(f) * ((s.astype(f) + g1.astype(f)[:, None, :]) + g2.astype(f)[None, :, :])
        if e is not None:
            got = got + e.astype(f)
        assert got.dtype == f and (np.abs(got.astype(np.float64) - out) <= tol).all()
        assert (tol > 0).all() and (tol < 1e-5).all()
