"""GPU suite for the clip API's large-frame mode (speinet_amd/tiles.py, csrc/tile_io.hip, video.deblur_clip(..., tiles=)): the tile
ingest bit for bit against the frame ingest on every tile's crop, the tile egress against the frame egress stitched in numpy by the
plan's bands (and against tests/tiles_ref.py), its non-finite flag for owned pixels only, the refusals of bad tables, and a tiled
clip against the untiled clip API on every tile's cropped clip.  No tolerances anywhere."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tiles_ref as R                                                          # noqa: E402
from speinet_amd import _lib, ops, video                                       # noqa: E402
from speinet_amd import tiles as T                                             # noqa: E402
from speinet_amd.synth import synth_frames                                     # noqa: E402

DEV = "cuda:0"

# odd origins and rows that start on odd bytes; seams off multiples of 4; W no multiple of 4
HAND = T.TilePlan(47, 61, 2, 3, 40, 40, (0, 7), (0, 11, 21), (0, 23, 47), (0, 20, 41, 61))
PLANS = [HAND,
         T.tile_plan(33, 90, (1, 2)),                      # th = 33 pads to 40 by reflection
         T.tile_plan(130, 47, (3, 1)),                     # tw = 47 pads to 60; the last tile slides inward
         T.tile_plan(80, 120, (2, 2))]                     # the reference's quadrants: every row aligned
IDS = [f"{p.H}x{p.W}-{p.rows}x{p.cols}" for p in PLANS]


def _crops(frame: torch.Tensor, plan):
    for i in range(plan.rows):
        for j in range(plan.cols):
            yield i * plan.cols + j, frame[plan.y0[i]:plan.y0[i] + plan.th, plan.x0[j]:plan.x0[j] + plan.tw].contiguous()


# ---- 1. ingest -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [None, 10, 12])
@pytest.mark.parametrize("plan", PLANS, ids=IDS)
def test_tiles_in(plan, depth):
    D = R.scale_of(depth)
    rng = np.random.default_rng(plan.H * 131 + plan.W + (depth or 0))
    if depth is None:
        host = rng.integers(0, 256, (plan.H, plan.W, 3), dtype=np.uint8)
    else:
        host = rng.integers(0, D + 1, (plan.H, plan.W, 3)).astype(np.uint16)
        host[::5, ::7] = rng.integers(D + 1, 65536, host[::5, ::7].shape).astype(np.uint16)      # words above D read as D
    frame = torch.from_numpy(host).to(DEV)
    thp, twp = plan.padded
    # the tiles as frame 1 of every tile's window input: a tile stride of five frames; the other frames stay as they are
    x = torch.full((plan.n, 5, 3, thp, twp), float("nan"), device=DEV)
    got = ops.tiles_in(frame, plan, x[:, 1], depth)
    assert got.data_ptr() == x[:, 1].data_ptr()
    for k, crop in _crops(frame, plan):
        ref = ops.frames_u8_in(crop)[0] if depth is None else ops.frames_u16_in(crop, depth)[0]
        assert ref.shape == (1, 3, thp, twp)
        assert torch.equal(x[k, 1], ref[0]), k
    for j in (0, 2, 3, 4):
        assert torch.isnan(x[:, j]).all(), j
    assert np.array_equal(x[:, 1].cpu().numpy(), R.ingest(host, plan, depth))
    # a packed destination, and a frame that starts on an odd sample
    packed = torch.empty(plan.n, 3, thp, twp, device=DEV)
    ops.tiles_in(frame, plan, packed, depth)
    assert torch.equal(packed, x[:, 1])
    buf = torch.zeros(frame.numel() + 1, dtype=frame.dtype, device=DEV)
    buf[1:] = frame.reshape(-1)
    packed.fill_(float("nan"))
    ops.tiles_in(buf[1:].view(plan.H, plan.W, 3), plan, packed, depth)
    assert torch.equal(packed, x[:, 1])


# ---- 2. egress -----------------------------------------------------------------------------------------------------------------------
def _ties(D: int) -> np.ndarray:
    """float32 values v with fl(v * D) == k + 0.5 exactly: round-half-even decides them (tests/test_gpu_video.py's, for any D)."""
    out = []
    for k in range(0, D, max(1, D // 255)):
        v = np.float32((k + 0.5) / D)
        for c in (v, np.nextafter(v, np.float32(1)), np.nextafter(v, np.float32(0))):
            if np.float32(c) * np.float32(D) == np.float32(k + 0.5):
                out.append(c)
                break
    return np.asarray(out, np.float32)


def _frame_out(t: torch.Tensor, depth: int) -> np.ndarray:
    """The whole tile through the frame egress kernel."""
    _, h, w = t.shape
    return (ops.frame_u8_out(t, h, w) if depth == 8 else ops.frame_u16_out(t, h, w, depth)).cpu().numpy()


@pytest.mark.parametrize("depth", [8, 10, 12])
@pytest.mark.parametrize("plan", PLANS, ids=IDS)
def test_tiles_out(plan, depth):
    D = R.scale_of(depth)
    thp, twp = plan.padded
    rng = np.random.default_rng(plan.H * 77 + plan.W + depth)
    x = rng.uniform(-0.5, 1.5, (plan.n, 3, thp, twp)).astype(np.float32)
    own = np.broadcast_to(R.owned(plan)[:, None], x.shape)
    ties = _ties(D)
    assert len(ties) > 200
    # the ties, exact 0 and 1 and values far outside [0, 1] at random OWNED places
    special = np.concatenate([ties, np.float32([0.0, 1.0, -0.0, -3.0, 7.0, 255.0])])
    sel = rng.choice(np.flatnonzero(own), size=len(special), replace=False)
    x.reshape(-1)[sel] = special
    tiles = torch.from_numpy(x).to(DEV)
    ref = R.stitch([_frame_out(tiles[k], depth) for k in range(plan.n)], plan)
    flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)                     # cleared by the call
    got = ops.tiles_out(tiles, plan, depth, nonfinite=flag)
    assert got.shape == (plan.H, plan.W, 3) and got.dtype == (torch.uint8 if depth == 8 else torch.uint16)
    assert np.array_equal(got.cpu().numpy(), ref)
    assert np.array_equal(ref, R.egress(x, plan, depth)[0])
    assert int(flag.item()) == 0
    # the tiles as separate allocations, into a given destination, without a flag
    out = torch.zeros_like(got)
    assert ops.tiles_out([tiles[k].clone() for k in range(plan.n)], plan, depth, out=out).data_ptr() == out.data_ptr()
    assert np.array_equal(out.cpu().numpy(), ref)
    # NaNs and infinities everywhere OUTSIDE the bands (margins, reflect pad): the same frame, the flag stays 0
    xm = np.where(own, x, np.float32(np.nan))
    xm[:, 1][~own[:, 1]] = np.inf
    flag.fill_(7)
    got = ops.tiles_out(torch.from_numpy(xm).to(DEV), plan, depth, nonfinite=flag)
    assert np.array_equal(got.cpu().numpy(), ref)
    assert int(flag.item()) == 0
    # one non-finite OWNED value, at the first and the last pixel of a band and at a seam: 0 there, the flag set
    i, j = plan.rows - 1, plan.cols - 1
    k = i * plan.cols + j
    for (kk, c, y, x_), v in ((((k, 0, plan.yb[i] - plan.y0[i], plan.xb[j] - plan.x0[j])), np.nan),
                              ((k, 2, plan.H - 1 - plan.y0[i], plan.W - 1 - plan.x0[j]), np.inf),
                              ((0, 1, plan.yb[1] - 1 - plan.y0[0], plan.xb[1] - 1 - plan.x0[0]), -np.inf)):
        assert own[kk, c, y, x_]
        xn = xm.copy()
        xn[kk, c, y, x_] = v
        flag.fill_(0)
        got = ops.tiles_out(torch.from_numpy(xn).to(DEV), plan, depth, nonfinite=flag).cpu().numpy()
        assert int(flag.item()) != 0
        want = ref.copy()
        want[y + plan.y0[kk // plan.cols], x_ + plan.x0[kk % plan.cols], c] = 0
        assert np.array_equal(got, want), (kk, c, y, x_)


# ---- 3. bad tables: refused before anything is launched ---------------------------------------------------------------------------------
def _bad(plan, **changes):
    return dataclasses.replace(plan, **changes)


def test_bad_tables():
    plan = HAND
    thp, twp = plan.padded
    frame = torch.zeros(plan.H, plan.W, 3, dtype=torch.uint8, device=DEV)
    deep = torch.zeros(plan.H, plan.W, 3, dtype=torch.uint16, device=DEV)
    x = torch.full((plan.n, 3, thp, twp), 5.0, device=DEV)
    for bad, text in ((_bad(plan, y0=(0, 8)), "outside the 47x61 frame"),                          # 8 + 40 > 47
                      (_bad(plan, x0=(0, 11, 22)), "outside the 47x61 frame"),
                      (_bad(plan, x0=(-1, 11, 21)), "outside the 47x61 frame"),
                      (_bad(plan, rows=9, y0=(0,) * 9), "1..8 rows and columns")):
        o = torch.full((bad.rows * bad.cols, 3, thp, twp), 5.0, device=DEV)
        for fr, depth in ((frame, None), (deep, 10)):
            with pytest.raises(RuntimeError, match=text):
                ops.tiles_in(fr, bad, o, depth)
            assert text in _lib.lib().spei_last_error().decode()
        assert (o == 5.0).all()                                                   # nothing was written: nothing ran
    # an empty grid, through the C-ABI itself
    lib, vp = _lib.lib(), ctypes.c_void_p
    st = vp(torch.cuda.current_stream(DEV).cuda_stream)
    zeros = (ctypes.c_int * 9)()
    assert lib.spei_tiles_u8_in(vp(frame.data_ptr()), plan.H, plan.W, vp(x.data_ptr()), 3 * thp * twp, zeros, zeros, 2, 0, 40, 40, st) != 0
    assert "1..8 rows and columns" in lib.spei_last_error().decode()
    assert lib.spei_tiles_u16_in(vp(deep.data_ptr()), plan.H, plan.W, vp(x.data_ptr()), 3 * thp * twp, zeros, zeros, 0, 3, 40, 40, 10, st) != 0
    assert "1..8 rows and columns" in lib.spei_last_error().decode()
    assert lib.spei_tiles_u16_in(vp(deep.data_ptr()), plan.H, plan.W, vp(x.data_ptr()), 3 * thp * twp, zeros, zeros, 1, 1, 40, 40, 11, st) != 0
    assert "unknown depth 11" in lib.spei_last_error().decode()
    assert (x == 5.0).all()
    tiles = torch.zeros(plan.n, 3, thp, twp, device=DEV)
    for bad, text in ((_bad(plan, yb=(0, 41, 47)), "outside its tile"),                            # band 0 ends past row 40 of its tile
                      (_bad(plan, xb=(0, 10, 41, 61)), "outside its tile"),                        # band 1 starts left of its tile
                      (_bad(plan, y0=(0, 24)), "outside its tile"),
                      (_bad(plan, y0=(0, 47)), "outside the 47x61 frame"),
                      (_bad(plan, yb=(0, 23, 46)), "must span"),
                      (_bad(plan, xb=(0, 20, 20, 61)), "empty or reversed"),
                      (_bad(plan, cols=9, x0=(0,) * 9, xb=tuple(range(0, 60, 6))), "1..8 rows and columns")):
        n = bad.rows * bad.cols
        for depth in (8, 12):
            out = torch.full((plan.H, plan.W, 3), 9, dtype=torch.uint8 if depth == 8 else torch.uint16, device=DEV)
            flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)
            with pytest.raises(RuntimeError, match=text):
                ops.tiles_out([tiles[0]] * n, bad, depth, out=out, nonfinite=flag)
            assert text in _lib.lib().spei_last_error().decode()
            assert int(flag.item()) == 7 and (out == 9).all()                     # neither cleared nor written: nothing ran
    # the wrappers' own refusals
    with pytest.raises(ValueError, match="tile plan is for"):
        ops.tiles_in(frame[:40].contiguous(), plan, x)
    with pytest.raises(ValueError, match="has 6 tiles"):
        ops.tiles_out([tiles[0]] * 5, plan, 8)
    with pytest.raises(ValueError, match="depth"):
        ops.tiles_in(deep, plan, x)


# ---- 4. the clip loop --------------------------------------------------------------------------------------------------------------------
LABELS = [1, 0, 0, 1, 0, 0]
NUMBERS = [0, 1, 2, 13, 14, 15]          # frame numbers with a gap: frames 2 and 3 are more than 7 from their reference, so both routings run


def _clip(n, h, w, seed=3):
    """uint8 [n,h,w,3]: the synthetic frames, shifted a little per frame (tests/test_gpu_video.py's)."""
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


@pytest.mark.parametrize("h, w, grid, out_depth", [(80, 120, (2, 2), None), (130, 47, (3, 1), 10)])
def test_tiled_clip_equals_tile_clips(net16, h, w, grid, out_depth):
    """A tiled clip is, bit for bit, the untiled clip API on every tile's cropped clip, stitched by the plan's bands."""
    frames = _clip(6, h, w)
    plan = T.tile_plan(h, w, grid)
    assert {p["zero_pre"] for p in video.window_plan(LABELS, numbers=NUMBERS)} == {True, False}
    run = video.deblur_clip(net16, frames, LABELS, numbers=NUMBERS, tiles=grid, out_depth=out_depth)
    assert run.tiles == plan and run.tiles.n == plan.rows * plan.cols > 1
    got = _frames(run)
    assert got.shape == (6, h, w, 3) and got.dtype == (np.uint8 if out_depth is None else np.uint16)
    assert run.recomputed == []
    assert np.array_equal(run.labels, LABELS) and run.cuts == []
    per_tile = []
    for i in range(plan.rows):
        for j in range(plan.cols):
            crop = np.ascontiguousarray(frames[:, plan.y0[i]:plan.y0[i] + plan.th, plan.x0[j]:plan.x0[j] + plan.tw])
            one = video.deblur_clip(net16, crop, LABELS, numbers=NUMBERS, out_depth=out_depth)
            assert one.tiles is None
            per_tile.append(_frames(one))
            assert one.recomputed == []
    for f in range(6):
        assert np.array_equal(got[f], R.stitch([t[f] for t in per_tile], plan)), f


def test_tiled_non_finite_windows_recomputed():
    """One weight beyond +-65504 makes every f16 frame non-finite (tests/test_gpu_video.py::test_non_finite_windows_recomputed): a tiled
    clip recomputes every tile of every window in bf16x3, as the untiled clip API does on every tile's cropped clip."""
    import warnings
    net = video.load_model("synthetic", DEV, "f16", graph=True)
    with torch.no_grad():
        net.recons_net.outBlock[3].weight[0, 0, 0, 0] = 1.0e5
    net.invalidate_packed()
    frames, labels = _clip(4, 80, 120), [1, 0, 0, 1]
    plan = T.tile_plan(80, 120, (2, 2))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        run = video.deblur_clip(net, frames, labels, tiles=(2, 2))
        got = _frames(run)
        assert run.recomputed == [0, 1, 2, 3]
        assert sum("recomputed in bf16x3" in str(c.message) for c in caught) == 4
        assert (net.precision, net.corr_precision, net.use_graph) == ("f16", "top2", True)     # restored
        per_tile = []
        for i in range(plan.rows):
            for j in range(plan.cols):
                crop = np.ascontiguousarray(frames[:, plan.y0[i]:plan.y0[i] + plan.th, plan.x0[j]:plan.x0[j] + plan.tw])
                one = video.deblur_clip(net, crop, labels)
                per_tile.append(_frames(one))
                assert one.recomputed == [0, 1, 2, 3]
    for f in range(4):
        assert np.array_equal(got[f], R.stitch([t[f] for t in per_tile], plan)), f


def test_auto_on_a_small_frame_is_the_untiled_path(net16):
    frames = _clip(6, 80, 120)
    ref = _frames(video.deblur_clip(net16, frames, LABELS, numbers=NUMBERS))
    for tiles in ("auto", (1, 1)):
        run = video.deblur_clip(net16, frames, LABELS, numbers=NUMBERS, tiles=tiles)
        assert run.tiles is None
        assert np.array_equal(_frames(run), ref)
    with pytest.raises(ValueError, match="band of 30"):
        video.deblur_clip(net16, frames, LABELS, tiles=(2, 4))
    with pytest.raises(ValueError, match="shave"):
        video.deblur_clip(net16, frames, LABELS, tiles=(2, 2), shave=300)


def test_cli_tiles(net16, tmp_path, capsys):
    """`python -m speinet_amd.video --tiles 2x2` (its `main`, in this process) writes the frames the library yields."""
    from PIL import Image
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    frames = _clip(5, 80, 120, seed=13)
    for i in range(5):
        Image.fromarray(frames[i]).save(src / f"frame_{i:03d}.png")
    labels = np.asarray([0, 1, 0, 0, 0])
    np.save(tmp_path / "labels.npy", labels)
    video.main(["--input", str(src), "--output", str(dst), "--model_path", "synthetic", "--labels", str(tmp_path / "labels.npy"),
                "--device", DEV, "--tiles", "2x2", "--shave", "20"])
    text = capsys.readouterr().out
    assert "# 2x2 tiles of 80x60, shave 20" in text and text.count("> frame_") == 5
    assert sorted(os.listdir(dst)) == [f"frame_{i:03d}.png" for i in range(5)]
    ref = _frames(video.deblur_clip(net16, frames, labels, tiles=(2, 2)))
    for i in range(5):
        assert np.array_equal(np.asarray(Image.open(dst / f"frame_{i:03d}.png").convert("RGB")), ref[i]), i
    with pytest.raises(SystemExit, match="--tiles"):
        video.main(["--input", str(src), "--output", str(dst), "--model_path", "synthetic", "--device", DEV, "--tiles", "2by2"])
