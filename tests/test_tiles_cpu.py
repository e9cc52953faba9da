"""CPU suite for the tile plan of the clip API's large-frame mode (speinet_amd/tiles.py): the per-axis rule by brute force, the
reference's forward_chop slices as numbers (inference_SPEINet.py:545-607), the "auto" grids, the refusals, the command-line parser,
and the numpy restatement of ingest and stitch (tests/tiles_ref.py) that the GPU suite compares the kernels with."""
import numpy as np
import pytest

import tiles_ref as R
from speinet_amd import tiles as T


@pytest.mark.parametrize("shave", [0, 20, 48])
def test_axis_rule_brute_force(shave):
    """Every admissible axis: every tile inside the frame, the tile length a multiple of 20 or the whole axis, every band inside its
    tile, and at least `shave` pixels of margin on every side of a band that is not a frame edge."""
    admissible = 0
    for n in range(20, 1301):
        for r in range(1, 9):
            try:
                t, o, b = T.axis_plan(n, r, shave)
            except ValueError:
                small = min((i + 1) * n // r - i * n // r for i in range(r))
                assert r > 1 and small < max(40, 2 * shave), (n, r)
                continue
            admissible += 1
            assert b == [i * n // r for i in range(r + 1)] and b[0] == 0 and b[-1] == n
            assert len(o) == r and (t % 20 == 0 or t == n) and 0 < t <= n, (n, r, t)
            if t == n:
                assert o == [0] * r
            for i in range(r):
                assert 0 <= o[i] and o[i] + t <= n, (n, r, i)
                assert o[i] <= b[i] and b[i + 1] <= o[i] + t, (n, r, i)
                assert o[i] == 0 or b[i] - o[i] >= shave, (n, r, i)
                assert o[i] + t == n or o[i] + t - b[i + 1] >= shave, (n, r, i)
    assert admissible > 1281                               # every r = 1 axis, and many more


def test_reference_slices_2x2():
    """forward_chop's four quadrants: h_size = h // 2 + shave, seams at h // 2 and w // 2."""
    p = T.tile_plan(80, 120, (2, 2))
    assert (p.th, p.tw, p.y0, p.x0) == (60, 80, (0, 20), (0, 40))
    assert (p.yb, p.xb, p.n, p.padded, p.shave) == ((0, 40, 80), (0, 60, 120), 4, (60, 80), 20)
    p = T.tile_plan(720, 1280, (2, 2))
    assert (p.th, p.tw, p.y0, p.x0) == (380, 660, (0, 340), (0, 620))
    assert (p.yb, p.xb) == ((0, 360, 720), (0, 640, 1280))
    for n, t in ((720, 380), (1280, 660), (1080, 560), (1920, 980), (2160, 1100), (3840, 1940)):
        assert T.axis_plan(n, 2, 20)[:2] == (t, [0, n // 2 - 20]), n
    # the bands partition the frame
    for hw, grid in (((80, 120), (2, 2)), ((720, 1280), (2, 2)), ((130, 47), (3, 1)), ((1080, 1920), (3, 5))):
        p = T.tile_plan(*hw, grid)
        cover = np.zeros(hw, int)
        for i in range(p.rows):
            for j in range(p.cols):
                cover[p.yb[i]:p.yb[i + 1], p.xb[j]:p.xb[j + 1]] += 1
        assert (cover == 1).all()


def test_spanning_axis_and_sliding_tiles():
    p = T.tile_plan(33, 90, (1, 2))                        # 33 rows span the axis (the ingest reflects them to 40); 90 columns do not
    assert (p.th, p.tw, p.y0, p.x0, p.padded) == (33, 80, (0,), (0, 10), (40, 80))
    p = T.tile_plan(130, 47, (3, 1))                       # the last tile slides inward: 66 -> 30
    assert (p.th, p.tw, p.y0, p.x0, p.yb, p.padded) == (100, 47, (0, 23, 30), (0,), (0, 43, 86, 130), (100, 60))
    p = T.tile_plan(100, 100, (2, 2), shave=0)             # no margin: 50 rounds up to 60, the second tile slides from 50 to 40
    assert (p.th, p.tw, p.y0, p.x0, p.yb) == (60, 60, (0, 40), (0, 40), (0, 50, 100))


def test_auto():
    for hw in ((20, 20), (720, 1280), (80, 120), (800, 1200)):
        p = T.tile_plan(*hw, "auto")
        assert (p.rows, p.cols, p.th, p.tw, p.n) == (1, 1, *hw, 1)
    p = T.tile_plan(1080, 1920, "auto")
    assert (p.rows, p.cols, p.th, p.tw) == (1, 3, 1080, 680)
    p = T.tile_plan(2160, 3840, "auto")
    assert (p.rows, p.cols, p.th, p.tw) == (2, 5, 1100, 820)
    p = T.tile_plan(4320, 7680, "auto")
    assert (p.rows, p.cols) == (5, 8) and p.th * p.tw <= T.MAX_TILE_PIXELS
    # the fewest tiles: no grid with fewer fits
    for hw in ((1080, 1920), (2160, 3840)):
        p = T.tile_plan(*hw, "auto")
        for r in range(1, 9):
            for c in range(1, 9):
                if r * c < p.n:
                    q = T.tile_plan(*hw, (r, c))
                    assert q.th * q.tw > T.MAX_TILE_PIXELS, (hw, r, c)


def test_refusals():
    with pytest.raises(ValueError, match="band of 39"):
        T.tile_plan(78, 200, (2, 1))
    with pytest.raises(ValueError, match="needs at least 96"):
        T.tile_plan(180, 200, (2, 1), shave=48)
    T.tile_plan(192, 200, (2, 1), shave=48)
    for grid in ((0, 1), (1, 9), (2,), (2, 2, 2), (1.5, 2), (True, 2), "2x2", None, 3):
        with pytest.raises(ValueError, match="tiles must be|rows and columns"):
            T.tile_plan(720, 1280, grid)
    for shave in (-1, 201, 2.5, True):
        with pytest.raises(ValueError, match="shave"):
            T.tile_plan(720, 1280, (2, 2), shave=shave)
    with pytest.raises(ValueError, match="no grid"):
        T.tile_plan(8 * 1300, 8 * 1300, "auto")
    with pytest.raises(ValueError, match="no grid"):
        T.tile_plan(4320, 7680, "auto", shave=200)


def test_parse_tiles():
    assert T.parse_tiles("none") is None and T.parse_tiles("None") is None
    assert T.parse_tiles("auto") == "auto"
    assert T.parse_tiles("2x2") == (2, 2) and T.parse_tiles("3X1") == (3, 1) and T.parse_tiles(" 1x8 ") == (1, 8)
    for bad in ("", "2", "2x", "x2", "2x2x2", "axb", "-1x2", "2 x 2"):
        with pytest.raises(ValueError, match="none, auto or RxC"):
            T.parse_tiles(bad)
    with pytest.raises(ValueError, match="rows and columns"):
        T.tile_plan(720, 1280, T.parse_tiles("9x9"))


HAND = T.TilePlan(47, 61, 2, 3, 40, 40, (0, 7), (0, 11, 21), (0, 23, 47), (0, 20, 41, 61))      # the GPU suite's hand-made table


@pytest.mark.parametrize("plan", [HAND, T.tile_plan(33, 90, (1, 2)), T.tile_plan(130, 47, (3, 1)), T.tile_plan(80, 120, (2, 2)),
                                  T.tile_plan(37, 53, (1, 1))], ids=lambda p: f"{p.H}x{p.W}-{p.rows}x{p.cols}")
@pytest.mark.parametrize("depth", [None, 10, 12])
def test_numpy_restatement(plan, depth):
    """tests/tiles_ref.py against torch on the crops, and the round trip: a frame cut into tiles and stitched again is the frame."""
    import torch
    import torch.nn.functional as F
    D = R.scale_of(depth)
    rng = np.random.default_rng(plan.H * 1000 + plan.W)
    frame = rng.integers(0, D + 1, (plan.H, plan.W, 3)).astype(np.uint8 if depth is None else np.uint16)
    tiles = R.ingest(frame, plan, depth)
    thp, twp = plan.padded
    assert tiles.shape == (plan.n, 3, thp, twp) and tiles.dtype == np.float32
    for i in range(plan.rows):
        for j in range(plan.cols):
            crop = frame[plan.y0[i]:plan.y0[i] + plan.th, plan.x0[j]:plan.x0[j] + plan.tw].astype(np.float32)
            t = torch.from_numpy(crop).permute(2, 0, 1).mul_(1.0 / D)                # numpy2tensor: one float32 multiply
            ref = F.pad(t[None], (0, twp - plan.tw, 0, thp - plan.th), mode="reflect")[0]
            assert torch.equal(torch.from_numpy(tiles[i * plan.cols + j]), ref), (i, j)
    out_depth = 8 if depth is None else depth
    back, bad = R.egress(tiles, plan, out_depth)
    assert not bad and back.dtype == frame.dtype and np.array_equal(back, frame)
    # torch's rounding (tensor2numpy: mul, clamp, round half to even), ties included
    x = rng.uniform(-0.5, 1.5, (3, 40, 40)).astype(np.float32)
    x[0, 0, :8] = np.float32([0.5 / D, 1.5 / D, 2.5 / D, 1.0, 0.0, -3.0, 7.0, (D - 0.5) / D])
    ref = torch.from_numpy(x).mul(float(D)).clamp(0, D).round().numpy()
    assert np.array_equal(R.quantise(x, out_depth), ref.astype(back.dtype))
    # the flag: owned pixels only
    own = R.owned(plan)
    assert own.sum() == plan.H * plan.W
    if (~own).any():
        k, y, x_ = np.argwhere(~own)[len(np.argwhere(~own)) // 2]
        t2 = tiles.copy()
        t2[k, 1, y, x_] = np.nan
        assert not R.egress(t2, plan, out_depth)[1]
        assert np.array_equal(R.egress(t2, plan, out_depth)[0], frame)
    k, y, x_ = np.argwhere(own)[len(np.argwhere(own)) // 2]
    t2 = tiles.copy()
    t2[k, 2, y, x_] = np.inf
    got, bad = R.egress(t2, plan, out_depth)
    assert bad
    yy, xx = y + plan.y0[k // plan.cols], x_ + plan.x0[k % plan.cols]
    assert got[yy, xx, 2] == 0
    got[yy, xx, 2] = frame[yy, xx, 2]
    assert np.array_equal(got, frame)
