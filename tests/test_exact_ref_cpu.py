"""CPU suite for tests/exact_ref.py, the exact-integer references of test_gpu_exact_gemm.py: the conditions under which a kernel must
return the float64 result bit for bit hold for every case of the GPU file, fp32 arithmetic in any order reproduces float64 on these
operands, and torch.equal sees each structural or rounding fault that the max-norm tolerances of the older GPU tests let through."""
import pytest
import torch
import torch.nn.functional as F

import exact_ref as E

BF16, F16 = torch.bfloat16, torch.float16


def test_preconditions_of_every_gpu_case():
    """Exactly representable operands, sums below 2^24, |y| <= 60000, and for 16-bit outputs at least 10 % inexact values and 1 % ties,
    for every reference of the GPU file (walk shapes as built for 256 CUs)."""
    n = 0
    for label, o, y, lp_out, epilogue, fan_in in E.gpu_cases(E.MI355X_CUS):
        try:
            E.check_exact_preconditions(o, y, lp_out, epilogue, fan_in)
        except AssertionError as e:
            raise AssertionError(f"{label}: {e}") from None
        n += 1
    assert n == 72


def test_preconditions_reject_wrongly_built_cases():
    a = (3, 1, 64, 32, 1, 21, 19)
    with pytest.raises(AssertionError, match="inexact"):                         # sums of 64 products of the wide set: mostly f16 integers
        E.check_exact_preconditions(E.operands(*a, "wide"), E.conv_ref(*a, "wide"), (F16,))
    with pytest.raises(AssertionError, match="not exact"):                       # 300 is no bf16 number
        E.check_exact_preconditions(E.operands(*a, 300), E.conv_ref(*a, 300))
    o = E.operands(*a, "wide")
    with pytest.raises(AssertionError):                                          # a real-valued weight
        E.check_exact_preconditions(o._replace(w=o.w + 0.1), E.conv_ref(*a, "wide"))
    with pytest.raises(AssertionError, match="can reach"):
        E.check_exact_preconditions(o, E.conv_ref(*a, "wide"), fan_in=1 << 17)


@pytest.mark.parametrize("cus", [64, 104, 256, 304])
def test_walk_shapes(cus):
    """The walk shapes meet the rule for any CU count: tiles > 2 CUs and no multiple of them, >= 3 maps (>= 2 of whole tiles for the 3x3
    kernel), fewer tiles per map than workgroups, ragged last tile row and column for the weight-stationary kernels."""
    for c, tile in E.WS_TILES.items():
        maps, h, w = E.ws_walk_shape(c, cus)
        n = E.tiles_of(maps, h, w, tile)
        assert n > 2 * cus and n % cus and maps >= 3 and n // maps < cus and h % tile[0] and w % tile[1] and n <= 2 * cus + 4 * maps
    maps, h, w = E.pipe_walk_shape(cus)
    n = E.tiles_of(maps, h, w, E.PIPE_TILE)
    assert n > 2 * cus and n % cus and maps >= 2 and n // maps < cus and h % 6 == 0 and w % 16 == 0


def test_fp32_conv_equals_float64():
    """F.conv2d, conv_transpose2d and F.linear in float32 give the float64 reference bit for bit on these operands."""
    for cin, cout, k, s, h, w in E.IGEMM_CASES + E.HEAD_CASES:
        a = E.igemm_args(cin, cout, k, s, h, w)
        o = E.operands(*a)
        assert torch.equal(F.conv2d(o.x, o.w, o.bias, stride=s, padding=k // 2).double(), E.conv_ref(*a)), a
    for c in E.WS_TILES:
        for maps, h, w in E.WS_SMALL:
            a = E.ws_args(c, maps, h, w)
            o = E.operands(*a)
            assert torch.equal(F.relu(F.conv2d(o.x, o.w, o.bias, padding=2)).double(), E.conv_ref(*a, relu=True)), a
    for cin, cout, h, w in E.CONVT_CASES:
        a = E.convt_args(cin, cout, h, w)
        o = E.operands(*a)
        assert torch.equal(F.conv_transpose2d(o.x, o.w, o.bias, stride=2, padding=1, output_padding=1).double(), E.conv_ref(*a)), a
    for m, kd, n in E.LINEAR_CASES:
        o = E.linear_operands(*E.linear_args(m, kd, n))
        y = F.linear(E.rows(o.x), o.w.reshape(n, kd), o.bias) + E.rows(o.residual)
        assert torch.equal(y.double(), E.linear_ref(*E.linear_args(m, kd, n), residual=True))
    c0, c1, cout, k, h, w = E.CONCAT_CASE
    a = E.concat_args()
    o = E.operands(*a)
    y = F.relu(F.conv2d(o.x, o.w, o.bias, padding=1)) * o.rowscale + o.residual
    assert torch.equal(y.double(), E.conv_ref(*a, relu=True, rowscale=True, residual=True, split=c0))


@pytest.mark.parametrize("maps,c,k,h,w,amp", [(1, 32, 5, 20, 24, "wide"), (3, 64, 5, 7, 33, "wide"), (1, 256, 3, 9, 11, "wide"),
                                              (2, 256, 3, 6, 16, "narrow")])
def test_summation_order_cannot_matter(maps, c, k, h, w, amp):
    """A tap-by-tap accumulation in float32, forwards and with taps and channels reversed, equals the float64 conv."""
    a = (7, maps, c, c, k, h, w, amp)
    o, y = E.operands(*a), E.conv_ref(*a)
    assert torch.equal(E.conv_taps(o.x, o.w, o.bias).double(), y)
    assert torch.equal(E.conv_taps(o.x, o.w, o.bias, reverse=True, chunk=8).double(), y)


FAULT_CASE = (9, 3, 32, 32, 5, 18, 33, "wide")


def test_fault_dropped_product():
    """(a) one (tap, input channel) product missing from one output channel at every pixel: torch.equal fails, on that channel only, in
    float64 and after either 16-bit rounding."""
    o, y = E.operands(*FAULT_CASE), E.conv_ref(*FAULT_CASE)
    bad = E.conv_taps(o.x, o.w, o.bias, dtype=torch.float64, drop=(5, 17, 1, 3))
    assert torch.equal(E.conv_taps(o.x, o.w, o.bias, dtype=torch.float64), y)
    assert not torch.equal(bad, y)
    ch = (bad != y).any(0).any(-1).any(-1).nonzero().reshape(-1).tolist()
    assert ch == [5]
    for dt in (BF16, F16):
        assert not torch.equal(E.rounded(bad, dt), E.rounded(y, dt))


def test_fault_right_edge_wrap():
    """(b) no zero fill at the right edge: the taps right of the map read the next row's first pixels."""
    o, y = E.operands(*FAULT_CASE), E.conv_ref(*FAULT_CASE)
    bad = E.conv_taps(o.x, o.w, o.bias, dtype=torch.float64, wrap_right=True)
    assert not torch.equal(bad, y)
    cols = (bad != y).any(0).any(0).any(0).nonzero().reshape(-1).tolist()
    assert cols == [31, 32]                                                       # the two columns whose taps reach past the edge


def test_fault_halo_leak_between_maps():
    """(c) in a stack of maps, the top halo of map b reads the last rows of map b - 1."""
    o, y = E.operands(*FAULT_CASE), E.conv_ref(*FAULT_CASE)
    bad = E.conv_stack_halo_leak(o.x, o.w, o.bias)
    assert torch.equal(bad[0], y[0]) and torch.equal(bad[:, :, 2:], y[:, :, 2:])
    assert not torch.equal(bad[1, :, :2], y[1, :, :2]) and not torch.equal(bad[2, :, :2], y[2, :, :2])


def test_fault_stale_tile():
    """(d) one 6-row tile computed from the previous tile's input rows."""
    o, y = E.operands(*FAULT_CASE), E.conv_ref(*FAULT_CASE)
    bad = E.conv_stale_tile(o.x, o.w, o.bias, tile_rows=6, tile=2)
    assert not torch.equal(bad, y)
    assert (bad != y).any(0).any(0).any(-1).nonzero().reshape(-1).tolist() == list(range(12, 18))


@pytest.mark.parametrize("dt", [BF16, F16])
def test_fault_truncated_output(dt):
    """(e) a 16-bit output truncated instead of rounded to nearest even: differs where the exact value is inexact and nearer to the
    neighbour above in magnitude, and on the ties that nearest-even rounds up."""
    y = E.conv_ref(*FAULT_CASE)
    good, bad = E.rounded(y, dt), E.truncated(y, dt)
    assert (bad.double().abs() <= y.abs()).all()
    inexact, _ = E.rounding_shares(y, dt)
    assert not torch.equal(bad, good) and (bad != good).double().mean() > 0.3 * inexact
    assert torch.equal(E.truncated(good.double(), dt), good)                      # representable values stay


@pytest.mark.parametrize("dt", [BF16, F16])
def test_fault_ties_away_from_zero(dt):
    """(f) ties rounded away from zero: differs from nearest-even only on the ties whose even neighbour is the smaller one, about half of
    the ties — the reason the preconditions ask for ties."""
    y = E.conv_ref(*FAULT_CASE)
    good, bad = E.rounded(y, dt), E.ties_away(y, dt)
    _, ties = E.rounding_shares(y, dt)
    share = (bad != good).double().mean().item()
    assert not torch.equal(bad, good) and 0.3 * ties < share < 0.7 * ties
    assert torch.equal((bad.double() - y).abs(), (good.double() - y).abs())       # the same distance, the other neighbour
