"""CPU suite for the feathered tile seams (speinet_amd/tiles.py `feather`, `seam_ramps`; the definition in include/speinet_hip.h): the
ramps' half-widths from the tables, the weights, the refusals, and the numpy restatement (tests/tiles_feather_ref.py) on constant
tiles and against float32 evaluations of the blend."""
import dataclasses

import numpy as np
import pytest

import tiles_feather_ref as FR
import tiles_ref as R
from speinet_amd import tiles as T

HAND = T.TilePlan(47, 61, 2, 3, 40, 40, (0, 7), (0, 11, 21), (0, 23, 47), (0, 20, 41, 61))      # the GPU suite's hand-made table


def test_ramps_of_plans():
    """Within the margin every seam of a `tile_plan` plan gets the whole feather."""
    for hw, grid in (((33, 90), (1, 2)), ((130, 47), (3, 1)), ((80, 120), (2, 2)), ((1080, 1920), "auto"), ((2160, 3840), "auto"),
                     ((2160, 3840), (2, 5))):
        for feather in (0, 1, 8, 20):
            p = T.tile_plan(*hw, grid, feather=feather)
            assert p.feather == feather and p == dataclasses.replace(T.tile_plan(*hw, grid), feather=feather)
            assert T.seam_ramps(p) == ((feather,) * (p.rows - 1), (feather,) * (p.cols - 1)), (hw, grid, feather)
            assert FR.ramps(p) == T.seam_ramps(p)
            FR.corners(p)                                  # asserts that no ramp leaves the real pixels or meets another
    assert T.tile_plan(80, 120, (2, 2)).feather == 0 and T.seam_ramps(T.tile_plan(80, 120, (2, 2))) == ((0,), (0,))
    assert T.seam_ramps(T.tile_plan(40, 60, (1, 1), feather=20)) == ((), ())
    p = T.tile_plan(192, 200, (2, 1), shave=48, feather=48)
    assert T.seam_ramps(p) == ((48,), ())


def test_ramps_of_hand_made_tables():
    """The clip: the row seam at 23 has 16 rows of tile 1 above it (17 of tile 0 below); the column seam at 20 has 9 columns of tile
    1 left of it, the one at 41 has 10 columns of tile 1 right of it, and the band between them, 21 wide, gives each seam 10."""
    assert T.seam_ramps(dataclasses.replace(HAND, feather=20)) == ((16,), (9, 10))
    assert T.seam_ramps(dataclasses.replace(HAND, feather=9)) == ((9,), (9, 9))
    assert T.seam_ramps(HAND) == ((0,), (0, 0))
    FR.corners(dataclasses.replace(HAND, feather=20))
    # a band with a seam on both sides gives each half of itself; an edge band may be crossed further
    assert T.axis_ramps((0, 0, 0), (0, 50, 61, 120), 120, 20) == (5, 5)
    assert T.axis_ramps((0, 30), (0, 40, 100), 70, 20) == (10,)            # the high tile starts 10 before the seam
    assert T.axis_ramps((0, 20), (0, 40, 100), 45, 20) == (5,)             # the low tile ends 5 after it
    assert T.axis_ramps((0, 20), (0, 40, 100), 38, 20) == (0,)             # ... or before it: a hard seam
    assert T.axis_ramps((30, 0), (0, 40, 100), 100, 20) == (10,)           # origins that do not increase: still inside both tiles
    # a band at the frame's edge gives all of itself and no more: no ramp leaves the frame, whatever the tiles would allow
    assert T.axis_ramps((0, 30, 60), (0, 40, 90, 100), 90, 20) == (10, 10) # 10 before seam 40 in tile 1; 10 of frame after seam 90
    assert T.axis_ramps((0, 20, 60), (0, 40, 90, 100), 90, 20) == (20, 10)
    assert T.axis_ramps((0, 0), (0, 8, 100), 100, 20) == (8,)
    edge = T.TilePlan(100, 40, 3, 1, 90, 40, (0, 20, 60), (0,), (0, 40, 90, 100), (0, 40), feather=20)
    assert T.seam_ramps(edge) == ((20, 10), ())
    assert FR.corners(edge)[3].sum() == (40 + 20) * 40                     # the ramps [20, 60) and [80, 100)


@pytest.mark.parametrize("f", [1, 2, 3, 9, 16, 20, 200])
def test_weights(f):
    w = FR.weights(f)
    assert w.dtype == np.float32 and w.shape == (2 * f,)
    assert (np.diff(w) > 0).all() and w[0] > 0 and w[-1] < 1
    exact = (2 * np.arange(2 * f) + 1) / (4.0 * f)
    assert np.abs(w.astype(np.float64) - exact).max() <= 2.0 ** -23
    ulp = np.spacing(np.float32(1.0))
    assert np.abs((w.astype(np.float64) + w[::-1].astype(np.float64)) - 1.0).max() <= ulp      # w[p] + w[mirror p] == 1 within one ulp
    lo, hi, ww, inside = FR.axis(100, (0, 50, 100), (min(f, 50),))
    g = min(f, 50)
    assert inside.sum() == 2 * g and (lo[inside] == 0).all() and (hi[inside] == 1).all() and (ww[~inside] == 0).all()
    assert (lo[:50 - g] == 0).all() and (hi[:50 - g] == 0).all() and (lo[50 + g:] == 1).all() and (hi[50 + g:] == 1).all()
    assert np.array_equal(ww[inside], FR.weights(g))


class _NoModel:
    """A model that must not be asked for anything."""

    def parameters(self):
        raise AssertionError("the model was touched")

    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name})")


def test_refusals():
    for feather in (21, -1, True, 2.0, 8.5, "8", None):
        with pytest.raises(ValueError, match="feather"):
            T.tile_plan(720, 1280, (2, 2), feather=feather)
    with pytest.raises(ValueError, match="feather"):
        T.tile_plan(720, 1280, (2, 2), shave=8, feather=9)
    assert T.tile_plan(720, 1280, (2, 2), shave=8, feather=8).feather == 8
    from speinet_amd import video
    frames = np.zeros((4, 80, 120, 3), np.uint8)
    for feather in (8, -1, 2.5, True):
        with pytest.raises(ValueError, match="feather"):
            video.deblur_clip(_NoModel(), frames, [1, 0, 0, 1], feather=feather)
    for feather in (21, -1, 2.5):                          # with tiles: the plan's refusal, still before the model is looked at
        with pytest.raises(ValueError, match="feather"):
            video.deblur_clip(_NoModel(), frames, [1, 0, 0, 1], tiles=(2, 2), feather=feather)
    with pytest.raises(SystemExit, match="--feather 30"):
        video.main(["--input", "nowhere", "--output", "nowhere", "--model_path", "synthetic", "--tiles", "2x2", "--feather", "30", "--shave", "20"])
    with pytest.raises(SystemExit, match="needs --tiles"):
        video.main(["--input", "nowhere", "--output", "nowhere", "--model_path", "synthetic", "--feather", "8"])


@pytest.mark.parametrize("depth", [8, 12])
@pytest.mark.parametrize("plan, feather", [(T.tile_plan(33, 90, (1, 2)), 20), (T.tile_plan(130, 47, (3, 1)), 8), (T.tile_plan(80, 120, (2, 2)), 20),
                                           (HAND, 20), (T.tile_plan(80, 120, (2, 2)), 1)],
                         ids=lambda v: f"{v.H}x{v.W}-{v.rows}x{v.cols}" if hasattr(v, "rows") else str(v))
def test_constant_tiles(plan, feather, depth):
    """Tiles of one value each: the hard stitch steps by |c_i - c_j| at a seam, the feathered frame by at most the step spread over the
    ramp, |c_i - c_j| / (2 f), plus one level of rounding."""
    D = R.scale_of(depth)
    thp, twp = plan.padded
    c = np.linspace(0.1, 0.9, plan.n)[np.random.default_rng(5).permutation(plan.n)].astype(np.float32)
    tiles = np.broadcast_to(c[:, None, None, None], (plan.n, 3, thp, twp)).copy()
    hard = R.egress(tiles, plan, depth)[0].astype(np.int64)
    zero = FR.blend(tiles, dataclasses.replace(plan, feather=0), depth)        # float64 against float32: equal but for a tie (0.9 * 255)
    assert not zero["ramp"].any() and (zero["lo"] <= hard).all() and (hard <= zero["hi"]).all() and (zero["hi"] - zero["lo"] <= 1).all()
    fplan = dataclasses.replace(plan, feather=feather)
    soft = FR.blend(tiles, fplan, depth)
    assert not soft["bad"].any() and (soft["lo"] <= soft["mid"]).all() and (soft["mid"] <= soft["hi"]).all()
    out = ~soft["ramp"]
    assert np.array_equal(soft["lo"][out], zero["lo"][out]) and np.array_equal(soft["hi"][out], zero["hi"][out])
    fy, fx = T.seam_ramps(fplan)
    q = R.quantise(c, depth).astype(np.int64)
    for axis_, bounds, fs, cols_step in ((0, plan.yb, fy, plan.cols), (1, plan.xb, fx, 1)):
        for s in range(1, len(bounds) - 1):
            f, b = fs[s - 1], bounds[s]
            pairs = [(k - cols_step, k) for k in range(plan.n) if (k // plan.cols if axis_ == 0 else k % plan.cols) == s]
            step_hard = np.abs(np.diff(hard.take([b - 1, b], axis=axis_), axis=axis_))
            assert step_hard.max() == max(abs(q[j] - q[i]) for i, j in pairs)
            # the tiles of THIS seam: where the other axis' ramp crosses, the step is a convex mix of the pairs' differences
            step = max(abs(float(c[j]) - float(c[i])) for i, j in pairs)
            across = np.abs(np.diff(soft["mid"].take(range(b - f - 1, b + f + 1), axis=axis_), axis=axis_))
            assert across.max() <= step / (2 * f) * D + 1, (axis_, s, int(across.max()), step / (2 * f) * D + 1)
            assert across.max() < step_hard.max() or step_hard.max() <= 2


def test_float32_forms_stay_in_the_band():
    """Three float32 evaluations of the blend (fma(w, hi - lo, lo) emulated through float64, lo + w * (hi - lo) and (1 - w) * lo + w * hi
    with every step rounded) stay inside [lo, hi], and the band is open (lo != hi) for less than 1 % of the ramp samples."""
    plan = dataclasses.replace(HAND, feather=20)
    thp, twp = plan.padded
    rng = np.random.default_rng(11)
    x = rng.uniform(-0.5, 1.5, (plan.n, 3, thp, twp)).astype(np.float32)
    places, wy, wx, ramp = FR.corners(plan)
    a, b, c, d = (x[k, :, ry, cx] for k, ry, cx in places)
    wy, wx = wy[..., None], wx[..., None]
    f32 = np.float32

    def fma(w, lo, hi):
        return (w.astype(np.float64) * (hi - lo).astype(np.float64) + lo.astype(np.float64)).astype(f32)

    def plain(w, lo, hi):
        return lo + w * (hi - lo)

    def convex(w, lo, hi):
        return (f32(1) - w) * lo + w * hi

    for depth in (8, 10, 12):
        ref = FR.blend(x, plan, depth)
        assert (ref["lo"] != ref["hi"])[ramp].mean() <= 0.01
        for lerp in (fma, plain, convex):
            v = lerp(wy, lerp(wx, a, b), lerp(wx, c, d))
            assert v.dtype == f32
            got = R.quantise(v, depth).astype(np.int64)
            assert ((ref["lo"] <= got) & (got <= ref["hi"])).all(), (depth, lerp.__name__)
            assert np.array_equal(got[~ramp], R.egress(x, plan, depth)[0][~ramp])
