"""GPU suite for the feathered tile seams (spei_tiles_u8_blend / spei_tiles_u16_blend, csrc/tile_io.hip; `ops.tiles_out` on a plan with
`feather`; `video.deblur_clip(..., tiles=, feather=)`): outside the ramps the hard stitch bit for bit, inside them the float64 blend
of tests/tiles_feather_ref.py within the band its definition allows, the margins really read, the non-finite flag for contributing
values only, the refusals of bad arguments, and feathered clips against the hard-seam clip and every tile's own clip."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tiles_feather_ref as FR                                                 # noqa: E402
import tiles_ref as R                                                          # noqa: E402
from speinet_amd import _lib, ops, video                                       # noqa: E402
from speinet_amd import tiles as T                                             # noqa: E402
from speinet_amd.synth import synth_frames                                     # noqa: E402

DEV = "cuda:0"

# the plans of tests/test_gpu_tiles.py: odd origins, seams off multiples of 4, W no multiple of 4; reflect-padded rows; a tile that
# slides inward; the reference's quadrants
HAND = T.TilePlan(47, 61, 2, 3, 40, 40, (0, 7), (0, 11, 21), (0, 23, 47), (0, 20, 41, 61))
PLANS = [HAND, T.tile_plan(33, 90, (1, 2)), T.tile_plan(130, 47, (3, 1)), T.tile_plan(80, 120, (2, 2))]
IDS = [f"{p.H}x{p.W}-{p.rows}x{p.cols}" for p in PLANS]


def _ties(D: int) -> np.ndarray:
    """float32 values v with fl(v * D) == k + 0.5 exactly: round-half-even decides them (tests/test_gpu_tiles.py's)."""
    out = []
    for k in range(0, D, max(1, D // 255)):
        v = np.float32((k + 0.5) / D)
        for c in (v, np.nextafter(v, np.float32(1)), np.nextafter(v, np.float32(0))):
            if np.float32(c) * np.float32(D) == np.float32(k + 0.5):
                out.append(c)
                break
    return np.asarray(out, np.float32)


def _out(x: np.ndarray, plan, depth, **kw) -> np.ndarray:
    return ops.tiles_out(torch.from_numpy(x).to(DEV), plan, depth, **kw).cpu().numpy()


def _seam_place(plan):
    """A pixel (y, x) on the high side of an inner seam and outside the other axis' ramps, with the seam's low tile k and the place
    (row, column) of the pixel in it: inside the ramp, outside k's band."""
    if plan.cols > 1:
        y, x = 0, plan.xb[1]
        k = 0
    else:
        y, x = plan.yb[1], 0
        k = 0
    return y, x, k, y - plan.y0[k // plan.cols], x - plan.x0[k % plan.cols]


@pytest.mark.parametrize("depth", [8, 10, 12])
@pytest.mark.parametrize("feather", [1, 3, 20])
@pytest.mark.parametrize("plan", PLANS, ids=IDS)
def test_tiles_blend(plan, feather, depth):
    D = R.scale_of(depth)
    thp, twp = plan.padded
    fplan = dataclasses.replace(plan, feather=feather)
    fy, fx = T.seam_ramps(fplan)
    assert max(fy + fx) >= 1
    rng = np.random.default_rng(plan.H * 77 + plan.W + depth + 1000 * feather)
    x = rng.uniform(-0.5, 1.5, (plan.n, 3, thp, twp)).astype(np.float32)
    used = np.broadcast_to(FR.contributing(fplan)[:, None], x.shape)
    assert used.sum() > R.owned(plan).sum() * 3 and (used | ~np.broadcast_to(R.owned(plan)[:, None], x.shape)).all()
    # the ties, exact 0 and 1 and values far outside [0, 1] at random CONTRIBUTING places
    special = np.concatenate([_ties(D), np.float32([0.0, 1.0, -0.0, -3.0, 7.0, 255.0])])
    x.reshape(-1)[rng.choice(np.flatnonzero(used), size=len(special), replace=False)] = special
    ref = FR.blend(x, fplan, depth)
    ramp = ref["ramp"]
    assert ramp.any() and not ramp.all() and not ref["bad"].any()
    tiles = torch.from_numpy(x).to(DEV)
    hard = ops.tiles_out(tiles, plan, depth).cpu().numpy()
    assert np.array_equal(hard, R.egress(x, plan, depth)[0])
    flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)                     # cleared by the call
    got_t = ops.tiles_out(tiles, fplan, depth, nonfinite=flag)
    assert got_t.shape == (plan.H, plan.W, 3) and got_t.dtype == (torch.uint8 if depth == 8 else torch.uint16)
    got = got_t.cpu().numpy()
    assert int(flag.item()) == 0
    # outside every ramp: the hard stitch, bit for bit
    assert np.array_equal(got[~ramp], hard[~ramp])
    # inside: the band of the float64 blend, which is closed (lo == hi) for all but a few samples, so it cannot hide a wrong blend
    g = got.astype(np.int64)
    open_share = float((ref["lo"] != ref["hi"])[ramp].mean())
    off = (g < ref["lo"]) | (g > ref["hi"])
    print(f"{plan.H}x{plan.W} feather {feather} depth {depth}: {int(ramp.sum()) * 3} ramp samples, open band {100 * open_share:.3f} %, "
          f"outside the band {int(off.sum())}, differing from the hard stitch {int((got != hard)[ramp].sum())}")
    assert open_share <= 0.01
    assert not off.any(), np.argwhere(off)[:5]
    assert (got != hard)[ramp].mean() > 0.5                                       # the ramps are blended, not copied
    # the tiles as separate allocations, into a given destination, without a flag
    out = torch.zeros_like(got_t)
    assert ops.tiles_out([tiles[k].clone() for k in range(plan.n)], fplan, depth, out=out).data_ptr() == out.data_ptr()
    assert np.array_equal(out.cpu().numpy(), got)
    # NaNs and infinities wherever NO pixel reads (the rest of the margins, the reflect pad): the same frame, the flag stays 0
    xm = np.where(used, x, np.float32(np.nan))
    xm[:, 1][~used[:, 1]] = np.inf
    assert used.all() == (plan.rows == plan.cols == 2 and feather == plan.shave)  # the quadrants with feather = shave are read whole
    flag.fill_(7)
    assert np.array_equal(_out(xm, fplan, depth, nonfinite=flag), got)
    assert int(flag.item()) == 0
    # the margin is really used: one value of the low tile, inside the ramp and outside that tile's band
    y, x_, k, ry, cx = _seam_place(fplan)
    assert ramp[y, x_] and used[k, 0, ry, cx] and not R.owned(plan)[k, ry, cx]
    cross = bool(fy and fx and fy[0] > 0 and fx[0] > 0)                           # a row and a column ramp cross at (yb[1], xb[1])
    xa = xm.copy()
    for py, px, ch, v in [(y, x_, 2, 0.25)] + ([(plan.yb[1], plan.xb[1], 1, 0.5)] if cross else []):
        for p in FR.corners(fplan)[0]:                                            # every value that the pixel is made from
            xa[int(p[0][py, px]), ch, int(p[1][py, px]), int(p[2][py, px])] = v
    base = _out(xa, fplan, depth)
    xb = xa.copy()
    xb[k, 2, ry, cx] = 0.75
    moved = _out(xb, fplan, depth)
    want = FR.blend(xb, fplan, depth)
    assert want["lo"][y, x_, 2] > FR.blend(xa, fplan, depth)["hi"][y, x_, 2] + D // 16
    assert want["lo"][y, x_, 2] <= int(moved[y, x_, 2]) <= want["hi"][y, x_, 2]
    moved[y, x_, 2] = base[y, x_, 2]
    assert np.array_equal(moved, base)
    # one non-finite value there: 0 at that sample, the flag set, every other sample as before
    for v in (np.nan, np.inf, -np.inf):
        xn = xa.copy()
        xn[k, 2, ry, cx] = v
        flag.fill_(0)
        bad = _out(xn, fplan, depth, nonfinite=flag)
        assert int(flag.item()) != 0
        assert bad[y, x_, 2] == 0 and base[y, x_, 2] != 0
        bad[y, x_, 2] = base[y, x_, 2]
        assert np.array_equal(bad, base), v
    # where a row and a column ramp cross, four tiles contribute: a non-finite value in the one diagonally opposite the owner
    if cross:
        y, x_ = plan.yb[1], plan.xb[1]                                            # owned by tile (1, 1); tile (0, 0) is the low-low one
        ry, cx = y - plan.y0[0], x_ - plan.x0[0]
        assert used[0, 1, ry, cx] and not R.owned(plan)[0, ry, cx]
        xn = xa.copy()
        xn[0, 1, ry, cx] = np.inf
        flag.fill_(0)
        bad = _out(xn, fplan, depth, nonfinite=flag)
        assert int(flag.item()) != 0 and bad[y, x_, 1] == 0 and base[y, x_, 1] != 0
        bad[y, x_, 1] = base[y, x_, 1]
        assert np.array_equal(bad, base)


def test_edge_band_clips_the_ramp():
    """A hand-made table whose last tile reaches past the frame: the band at the frame's edge, 10 rows, clips the last seam's ramp to
    10 where the tiles alone would allow 20, so the ramp ends with the frame; the first seam keeps 20."""
    plan = T.TilePlan(100, 40, 3, 1, 90, 40, (0, 20, 60), (0,), (0, 40, 90, 100), (0, 40), feather=20)
    assert T.seam_ramps(plan) == ((20, 10), ())
    thp, twp = plan.padded
    x = np.random.default_rng(9).uniform(-0.5, 1.5, (plan.n, 3, thp, twp)).astype(np.float32)
    ref = FR.blend(x, plan, 8)
    ramp = ref["ramp"]
    assert ramp[20:60].all() and ramp[80:].all() and ramp.sum() == 60 * 40
    got = _out(x, plan, 8)
    assert np.array_equal(got[~ramp], R.egress(x, plan, 8)[0][~ramp])
    g = got.astype(np.int64)
    assert (ref["lo"] != ref["hi"])[ramp].mean() <= 0.01
    assert ((ref["lo"] <= g) & (g <= ref["hi"])).all()


@pytest.mark.parametrize("depth", [8, 10, 12])
def test_egress_paths_agree(depth):
    """The four ways out of the model's planes share one rounding, one non-finite rule and one store (csrc/pixel_group.h): on a 37x53
    frame in planes of 40x60 the hard stitch of a 1x1 plan, the feathered stitch of the same plan (no seam, so no ramp) and the ROI
    paste of the whole frame give the frame egress's frame and flag, with non-finite values inside the crop and, unseen, in the pad."""
    h, w, hp, wp = 37, 53, 40, 60
    hard = T.tile_plan(h, w, (1, 1))
    assert (hard.th, hard.tw, hard.padded, hard.y0, hard.x0, hard.yb, hard.xb) == (h, w, (hp, wp), (0,), (0,), (0, h), (0, w))
    soft = dataclasses.replace(hard, feather=20)
    dtype = torch.uint8 if depth == 8 else torch.uint16
    x = np.random.default_rng(3753 + depth).uniform(-0.1, 1.1, (3, hp, wp)).astype(np.float32)
    x[1, 38, 10] = np.nan                                                         # the pad: a row below the crop,
    x[0, 5, 53] = np.nan                                                          # and a column of the crop's last group of four
    frame = torch.full((h, w, 3), 77, dtype=torch.uint8, device=DEV)              # the paste's input frame: every pixel replaced
    for bad in (True, False):
        xs = x.copy()
        if bad:
            xs[0, 5, 7], xs[2, 36, 52] = np.nan, np.inf                           # inside the crop, the second in its last row and column
        planes = torch.from_numpy(xs).to(DEV)
        flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)
        want = (ops.frame_u8_out(planes, h, w, nonfinite=flag) if depth == 8 else ops.frame_u16_out(planes, h, w, depth, nonfinite=flag))
        want, want_flag = want.cpu().numpy(), int(flag.item())
        assert want.dtype == (np.uint8 if depth == 8 else np.uint16) and (want_flag != 0) == bad
        assert len(np.unique(want)) > 200 and (not bad or (want[5, 7, 0] == 0 and want[36, 52, 2] == 0))
        for name, call in (("tiles_out, hard", lambda f: ops.tiles_out([planes], hard, depth, nonfinite=f)),
                           ("tiles_out, feather 20", lambda f: ops.tiles_out([planes], soft, depth, nonfinite=f)),
                           ("roi_paste", lambda f: ops.roi_paste(planes, frame, (0, 0, h, w), depth, nonfinite=f))):
            flag.fill_(7)
            got = call(flag)
            assert got.dtype == dtype and np.array_equal(got.cpu().numpy(), want), (name, bad)
            assert (int(flag.item()) != 0) == (want_flag != 0), (name, bad)


def test_bad_arguments():
    """Refused through the C-ABI before anything is launched: the flag is not cleared, the frame not written."""
    plan = HAND
    thp, twp = plan.padded
    lib, vp = _lib.lib(), ctypes.c_void_p
    st = vp(torch.cuda.current_stream(DEV).cuda_stream)
    tiles = torch.zeros(plan.n, 3, thp, twp, device=DEV)
    ptrs = (vp * plan.n)(*[tiles[k].data_ptr() for k in range(plan.n)])
    tabs = [(ctypes.c_int * len(t))(*t) for t in (plan.y0, plan.x0, plan.yb, plan.xb)]
    for depth in (8, 12):
        out = torch.full((plan.H, plan.W, 3), 9, dtype=torch.uint8 if depth == 8 else torch.uint16, device=DEV)
        flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)

        def call(thp_, twp_, th, tw, feather, tabs_=tabs, rows=plan.rows, depth_=depth):
            head = (ptrs, vp(out.data_ptr()), vp(flag.data_ptr()), plan.H, plan.W, *tabs_, rows, plan.cols, thp_, twp_, th, tw, feather)
            return lib.spei_tiles_u8_blend(*head, st) if depth == 8 else lib.spei_tiles_u16_blend(*head, depth_, st)

        for args, text in (((thp, twp, plan.th, plan.tw, -1), "feather -1"),
                           ((thp, twp, plan.th, plan.tw, 201), "feather 201"),
                           ((60, twp, plan.th, plan.tw, 8), "rounded up"),                         # thp is not th rounded up
                           ((thp, 44, plan.th, plan.tw, 8), "rounded up"),
                           ((60, twp, 60, plan.tw, 8), "does not fit"),                            # th = 60 > H = 47
                           ((thp, 80, plan.th, 80, 8), "does not fit"),
                           ((thp, twp, 0, plan.tw, 8), "does not fit")):
            assert call(*args) != 0, args
            assert text in lib.spei_last_error().decode(), (args, lib.spei_last_error().decode())
        # the table checks of the hard stitch hold here as well
        bad_yb = [tabs[0], tabs[1], (ctypes.c_int * 3)(0, 41, 47), tabs[3]]
        assert call(thp, twp, plan.th, plan.tw, 8, tabs_=bad_yb) != 0 and "outside its tile" in lib.spei_last_error().decode()
        assert call(thp, twp, plan.th, plan.tw, 8, rows=9) != 0 and "1..8 rows and columns" in lib.spei_last_error().decode()
        if depth != 8:
            assert call(thp, twp, plan.th, plan.tw, 8, depth_=11) != 0 and "unknown depth 11" in lib.spei_last_error().decode()
        torch.cuda.synchronize()
        assert int(flag.item()) == 7 and (out == 9).all()                         # neither cleared nor written: nothing ran
        # and the wrapper: a plan whose feather the C-ABI refuses, and one that is no whole number
        with pytest.raises(RuntimeError, match="feather 201"):
            ops.tiles_out(tiles, dataclasses.replace(plan, feather=201), depth, out=out, nonfinite=flag)
        with pytest.raises(ValueError, match="feather"):
            ops.tiles_out(tiles, dataclasses.replace(plan, feather=2.5), depth, out=out, nonfinite=flag)
        assert int(flag.item()) == 7 and (out == 9).all()
        assert call(thp, twp, plan.th, plan.tw, 0) == 0                            # feather 0 through the blend entry: the hard stitch
        assert int(flag.item()) == 0 and (out == 0).all()


# ---- the clip loop -----------------------------------------------------------------------------------------------------------------------
LABELS = [1, 0, 0, 1]


def _clip(n, h, w, seed=3):
    """uint8 [n,h,w,3]: the synthetic frames, shifted a little per frame (tests/test_gpu_tiles.py's)."""
    x = synth_frames(1, h, w, seed=seed)[0]
    return np.stack([(torch.roll(x[i % 5], shifts=(i, -2 * i), dims=(1, 2)).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
                     for i in range(n)])


@pytest.fixture(scope="module")
def net16():
    return video.load_model("synthetic", DEV, "f16", graph=True)


def _frames(run) -> np.ndarray:
    got = {i: t.cpu().numpy() for i, t in run}
    assert sorted(got) == list(range(len(got)))
    return np.stack([got[i] for i in range(len(got))])


@pytest.mark.parametrize("h, w, grid, feather, out_depth", [(80, 120, (2, 2), 8, None), (130, 47, (3, 1), 20, 10)])
def test_feathered_clip(net16, h, w, grid, feather, out_depth):
    """A feathered clip is the hard-seam clip outside the ramps, bit for bit; inside them every sample lies within one level of the
    [min, max] of what the contributing tiles' own clips (the untiled clip API on each tile's crop) hold at that pixel."""
    frames = _clip(4, h, w)
    plan = T.tile_plan(h, w, grid, feather=feather)
    run = video.deblur_clip(net16, frames, LABELS, tiles=grid, feather=feather, out_depth=out_depth)
    assert run.tiles == plan and run.tiles.feather == feather
    soft = _frames(run)
    assert soft.shape == (4, h, w, 3) and soft.dtype == (np.uint8 if out_depth is None else np.uint16) and run.recomputed == []
    hard_run = video.deblur_clip(net16, frames, LABELS, tiles=grid, out_depth=out_depth)
    assert hard_run.tiles.feather == 0
    hard = _frames(hard_run)
    places, _, _, ramp = FR.corners(plan)
    assert ramp.any() and np.array_equal(soft[:, ~ramp], hard[:, ~ramp])
    per_tile = []
    for i in range(plan.rows):
        for j in range(plan.cols):
            crop = np.ascontiguousarray(frames[:, plan.y0[i]:plan.y0[i] + plan.th, plan.x0[j]:plan.x0[j] + plan.tw])
            per_tile.append(_frames(video.deblur_clip(net16, crop, LABELS, out_depth=out_depth)))
    per_tile = np.stack(per_tile).astype(np.int64)                                # [n, 4, th, tw, 3]
    for f in range(4):
        vals = np.stack([per_tile[k, f, ry, cx] for k, ry, cx in places])         # [4, H, W, 3]: the contributing tiles' own results
        assert np.array_equal(hard[f], R.stitch([per_tile[k, f] for k in range(plan.n)], plan)), f
        lo, hi = vals.min(0) - 1, vals.max(0) + 1
        s = soft[f].astype(np.int64)
        assert ((lo <= s) & (s <= hi))[ramp].all(), f
    print(f"{h}x{w} feather {feather}: {int((soft[:, ramp] != hard[:, ramp]).sum())} of {soft[:, ramp].size} ramp samples differ from the "
          "hard-seam clip")


def test_feathered_non_finite_windows_recomputed():
    """One weight beyond +-65504 makes every f16 frame non-finite (tests/test_gpu_tiles.py's case): the blend's flag sends every window
    to the bf16x3 recompute, whose frames are blended in turn and equal the hard-seam clip's outside the ramps."""
    import warnings
    net = video.load_model("synthetic", DEV, "f16", graph=True)
    with torch.no_grad():
        net.recons_net.outBlock[3].weight[0, 0, 0, 0] = 1.0e5
    net.invalidate_packed()
    frames = _clip(4, 80, 120)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        run = video.deblur_clip(net, frames, LABELS, tiles=(2, 2), feather=8)
        soft = _frames(run)
        assert run.recomputed == [0, 1, 2, 3]
        assert sum("recomputed in bf16x3" in str(c.message) for c in caught) == 4
        hard_run = video.deblur_clip(net, frames, LABELS, tiles=(2, 2))
        hard = _frames(hard_run)
        assert hard_run.recomputed == [0, 1, 2, 3]
    ramp = FR.corners(run.tiles)[3]
    assert ramp.any() and np.array_equal(soft[:, ~ramp], hard[:, ~ramp])


def test_feather_needs_tiles(net16):
    frames = _clip(4, 80, 120)
    with pytest.raises(ValueError, match="needs tiles"):
        video.deblur_clip(net16, frames, LABELS, feather=8)
    with pytest.raises(ValueError, match="feather"):
        video.deblur_clip(net16, frames, LABELS, tiles=(2, 2), feather=21)
    run = video.deblur_clip(net16, frames, LABELS, tiles="auto", feather=8)       # one tile: the untiled path, nothing to blend
    assert run.tiles is None


def test_cli_feather(net16, tmp_path, capsys):
    """`python -m speinet_amd.video --tiles 2x2 --feather 8` (its `main`, in this process) writes the frames the library yields."""
    from PIL import Image
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    frames = _clip(4, 80, 120, seed=13)
    for i in range(4):
        Image.fromarray(frames[i]).save(src / f"frame_{i:03d}.png")
    labels = np.asarray([0, 1, 0, 0])
    np.save(tmp_path / "labels.npy", labels)
    base = ["--input", str(src), "--output", str(dst), "--model_path", "synthetic", "--labels", str(tmp_path / "labels.npy"), "--device", DEV]
    video.main(base + ["--tiles", "2x2", "--feather", "8"])
    text = capsys.readouterr().out
    assert "# 2x2 tiles of 80x60, shave 20, feather 8" in text and text.count("> frame_") == 4
    assert sorted(os.listdir(dst)) == [f"frame_{i:03d}.png" for i in range(4)]
    ref = _frames(video.deblur_clip(net16, frames, labels, tiles=(2, 2), feather=8))
    for i in range(4):
        assert np.array_equal(np.asarray(Image.open(dst / f"frame_{i:03d}.png").convert("RGB")), ref[i]), i
    with pytest.raises(SystemExit, match="--feather 30"):
        video.main(base + ["--tiles", "2x2", "--feather", "30", "--shave", "20"])
    with pytest.raises(SystemExit, match="needs --tiles"):
        video.main(base + ["--feather", "8"])
