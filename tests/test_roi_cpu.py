"""CPU suite for the region of interest in the clip API: `requant` against float64 over every code, the bar rule `video.find_bars`,
the refusals of `deblur_clip(..., roi=, roi_feather=, bar_params=)` that precede all device work, and the numpy restatement of the
paste (tests/roi_ref.py) against itself: it sees the mistakes a kernel could make, and on the inputs of the GPU suite its float32
evaluation stays inside the float64 band with fewer than 1 % of the ramp samples on an open band.  No device."""
import numpy as np
import pytest

import roi_ref as RR
import tiles_ref as R
from speinet_amd import video

DEPTHS = (8, 10, 12)

# (frame H, W), rectangle (y0, x0, h, w): the shapes of the GPU suite
ODD = ((23, 29), (2, 5, 20, 21))                 # W % 4 != 0, an odd origin: the element paths
ALIGNED = ((40, 64), (4, 8, 32, 48))             # everything a multiple of 4: the 16-byte paths
CORNERS = [((40, 64), r) for r in ((0, 0, 24, 28), (0, 36, 24, 28), (16, 0, 24, 28), (16, 36, 24, 28))]
WHOLE = ((40, 64), (0, 0, 40, 64))
PADDED = ((50, 70), (3, 6, 33, 47))              # hp = 40 > h, wp = 60 > w
SHAPES = [ODD, ALIGNED] + CORNERS + [WHOLE, PADDED]


def make_case(shape, roi, in_depth=8, seed=0):
    """(src float32 [3, hp, wp], frame [H, W, 3]) for a paste: the model's values uniform in [-0.5, 1.5], the frame's uniform over
    the codes of its depth.  The same inputs on the CPU and on the GPU."""
    H, W = shape
    y0, x0, h, w = roi
    rng = np.random.default_rng(1000 * H + 10 * W + 7 * y0 + x0 + in_depth + seed)
    src = rng.uniform(-0.5, 1.5, (3, R.up20(h), R.up20(w))).astype(np.float32)
    frame = rng.integers(0, R.scale_of(in_depth) + 1, (H, W, 3)).astype(np.uint8 if in_depth == 8 else np.uint16)
    return src, frame


def feathers(roi):
    return [1, 3, min(roi[2], roi[3]) // 2]


# ---- requant ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_depth", DEPTHS)
@pytest.mark.parametrize("in_depth", DEPTHS)
def test_requant_every_code(in_depth, out_depth):
    din, dout = R.scale_of(in_depth), R.scale_of(out_depth)
    v = np.arange(65536 if in_depth > 8 else 256)
    want = np.floor(np.minimum(v, din).astype(np.float64) * dout / din + 0.5).astype(np.int64)        # round half up
    got = RR.requant(v, in_depth, out_depth)
    assert np.array_equal(got, want)
    assert got.min() == 0 and got.max() == dout
    if in_depth == out_depth:
        assert np.array_equal(got, np.minimum(v, din))


def test_requant_rounding_down_is_seen():
    v = np.arange(256)
    assert (v * 1023 // 255 != RR.requant(v, 8, 10)).any()
    src, frame = make_case(*ODD)
    floor = RR.paste(src, frame, ODD[1], 8, 10)["out"].copy()
    y0, x0, h, w = ODD[1]
    outside = np.ones(frame.shape[:2], bool)
    outside[y0:y0 + h, x0:x0 + w] = False
    assert (frame.astype(np.int64) * 1023 // 255 != floor)[outside].any()


# ---- find_bars -------------------------------------------------------------------------------------------------------------------------
def _maxima(H, W, top=0, bottom=0, left=0, right=0, black=16, picture=180, depth=8):
    s = 1 << (depth - 8)
    rows, cols = np.full(H, picture * s), np.full(W, picture * s)
    rows[:top] = black * s
    rows[H - bottom:] = black * s
    cols[:left] = black * s
    cols[W - right:] = black * s
    return rows, cols


def test_find_bars_shapes():
    assert video.find_bars(*_maxima(120, 160, top=12, bottom=12)) == (12, 0, 96, 160)                  # letterbox
    assert video.find_bars(*_maxima(120, 160, left=20, right=24)) == (0, 20, 120, 116)                 # pillarbox
    assert video.find_bars(*_maxima(120, 160, 10, 14, 8, 6)) == (10, 8, 96, 146)                       # windowbox
    assert video.find_bars(*_maxima(120, 160, top=12)) == (12, 0, 108, 160)                            # one bar
    assert video.find_bars(*_maxima(120, 160)) is None                                                 # no bars
    assert video.find_bars(np.full(120, 16), np.full(160, 16)) is None                                 # a black clip
    assert video.find_bars(np.zeros(120, int), np.zeros(160, int)) is None
    assert video.find_bars(*_maxima(120, 160, top=55, bottom=55)) is None                              # 10 rows left: below 20x20
    assert video.find_bars(*_maxima(120, 160, top=50, bottom=50)) == (50, 0, 20, 160)


def test_find_bars_min_bar():
    assert video.find_bars(*_maxima(120, 160, top=3, bottom=3)) is None                                # a dark edge line is not a bar
    assert video.find_bars(*_maxima(120, 160, top=3, bottom=12)) == (0, 0, 108, 160)
    assert video.find_bars(*_maxima(120, 160, top=4)) == (4, 0, 116, 160)
    assert video.find_bars(*_maxima(120, 160, top=3), min_bar=3) == (3, 0, 117, 160)
    assert video.find_bars(*_maxima(120, 160, top=3), min_bar=0) == (3, 0, 117, 160)


def test_find_bars_level():
    assert video.find_bars(*_maxima(120, 160, top=12, black=24)) == (12, 0, 108, 160)                  # exactly `level`: black
    assert video.find_bars(*_maxima(120, 160, top=12, black=25)) is None                               # level + 1: picture
    assert video.find_bars(*_maxima(120, 160, top=12, black=25), level=25) == (12, 0, 108, 160)
    assert video.find_bars(*_maxima(120, 160, top=12, black=1), level=0) is None
    assert video.find_bars(*_maxima(120, 160, top=12, black=0), level=0) == (12, 0, 108, 160)


@pytest.mark.parametrize("depth", [10, 12])
def test_find_bars_deep(depth):
    s = 1 << (depth - 8)
    assert video.find_bars(*_maxima(120, 160, top=12, bottom=12, depth=depth), depth) == (12, 0, 96, 160)
    rows, cols = _maxima(120, 160, top=12, black=24, depth=depth)
    assert video.find_bars(rows, cols, depth) == (12, 0, 108, 160)                                     # 24 << (depth - 8): black
    rows[:12] = 24 * s + 1
    assert video.find_bars(rows, cols, depth) is None
    assert video.find_bars(rows, cols, 8) is None                                                      # read as 8-bit: all picture
    with pytest.raises(ValueError, match="depth"):
        video.find_bars(rows, cols, 9)
    with pytest.raises(ValueError, match="min_bar"):
        video.find_bars(rows, cols, depth, min_bar=-1)


def test_sample_indices():
    assert video.sample_indices(10, None) == list(range(10))
    assert video.sample_indices(10, 64) == list(range(10))
    assert video.sample_indices(100, 4) == [12, 37, 62, 87]
    for T, n in ((7, 3), (1000, 64), (65, 64)):
        idx = video.sample_indices(T, n)
        assert len(idx) == n and idx == sorted(set(idx)) and 0 <= idx[0] and idx[-1] < T


# ---- the refusals of deblur_clip, all in front of any device work (no model is needed to reach them) ---------------------------------------
def test_deblur_clip_refusals():
    frames = np.zeros((4, 60, 80, 3), np.uint8)

    def refused(match, **kw):
        with pytest.raises(ValueError, match=match):
            video.deblur_clip(None, frames, [0, 1, 0, 0], **kw)

    for roi in ((1, 2, 3), (1, 2, 30, 40, 5), (True, 0, 30, 40), (0.0, 0, 30, 40), "whole", ("1", 2, 30, 40), 7):
        refused("four whole numbers", roi=roi)
    refused("lies outside", roi=(-1, 0, 30, 40))
    refused("lies outside", roi=(0, -1, 30, 40))
    refused("lies outside", roi=(31, 0, 30, 40))           # y0 + h = 61 > 60
    refused("lies outside", roi=(0, 41, 30, 40))
    refused("at least 20x20", roi=(0, 0, 19, 40))
    refused("at least 20x20", roi=(0, 0, 30, 19))
    refused("tiles", roi=(5, 5, 30, 40), tiles=(1, 2))
    refused("tiles", roi="auto", tiles="auto")
    refused("crop", roi=(5, 5, 30, 40), crop=True)
    refused("needs roi=", roi_feather=2)
    refused("roi_feather", roi=(5, 5, 30, 40), roi_feather=-1)
    refused("roi_feather", roi=(5, 5, 30, 40), roi_feather=True)
    refused("roi_feather", roi=(5, 5, 30, 40), roi_feather=1.5)
    refused("roi_feather=16", roi=(5, 5, 30, 40), roi_feather=16)                  # h // 2 = 15
    refused("roi_feather=21", roi=(5, 5, 50, 40), roi_feather=21)                  # w // 2 = 20
    refused("roi_feather=31", roi="auto", roi_feather=31)                          # no rectangle of a 60x80 frame fits it
    refused("bar_params holds \\['window'\\]", roi="auto", bar_params={"window": 2})
    big = np.zeros((2, 500, 500, 3), np.uint8)
    with pytest.raises(ValueError, match="roi_feather=201"):
        video.deblur_clip(None, big, [0, 1], roi=(0, 0, 450, 450), roi_feather=201)
    # what is accepted gets as far as the model (None has no parameters)
    for kw in (dict(roi=(5, 5, 30, 40), roi_feather=15), dict(roi=[5, 5, 30, 40]), dict(roi="auto", bar_params={"level": 30, "frames": None}),
               dict(roi=(np.int64(0), 0, 60, 80))):
        with pytest.raises(AttributeError):
            video.deblur_clip(None, frames, [0, 1, 0, 0], **kw)


def test_roi_of_and_parse_roi():
    assert video.roi_of(None, 60, 80) is None and video.roi_of("auto", 60, 80) == "auto"
    assert video.roi_of((7, 13, 40, 60), 60, 80) == (7, 13, 40, 60)
    assert video.roi_of((0, 0, 60, 80), 60, 80) is None                            # the whole frame: the path without a region
    assert video.parse_roi("none") is None and video.parse_roi("auto") == "auto"
    assert video.parse_roi("7,13,40,60") == (7, 13, 40, 60)
    for text in ("7,13,40", "a,b,c,d", "7,13,40,-60", "7;13;40;60", ""):
        with pytest.raises(ValueError):
            video.parse_roi(text)


def test_frames_view_and_sample():
    clip = np.arange(5 * 30 * 40 * 3, dtype=np.uint8).reshape(5, 30, 40, 3)
    fr = video.frames_of(clip)
    v = fr.view((3, 5, 20, 21))
    assert (v.H, v.W, v.T) == (20, 21, 5) and (fr.H, fr.W) == (30, 40)
    assert np.array_equal(v.host(2), clip[2, 3:23, 5:26])
    s = v.sample([4, 0])
    assert s.T == 2 and np.array_equal(s.host(0), clip[4, 3:23, 5:26]) and np.array_equal(s.host(1), clip[0, 3:23, 5:26])
    assert np.array_equal(fr.host(1), clip[1])


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,roi", SHAPES)
def test_hard_paste_is_crop_and_requant(shape, roi):
    y0, x0, h, w = roi
    for in_depth in DEPTHS:
        src, frame = make_case(shape, roi, in_depth)
        for out_depth in DEPTHS:
            ref = RR.paste(src, frame, roi, in_depth, out_depth)
            want = RR.requant(frame, in_depth, out_depth)
            want[y0:y0 + h, x0:x0 + w] = R.quantise(src[:, :h, :w], out_depth).transpose(1, 2, 0)
            assert np.array_equal(ref["out"], want) and not ref["bad"] and not ref["ramp"].any()
            assert np.array_equal(ref["lo"], want) and np.array_equal(ref["hi"], want)
            if in_depth == out_depth:
                keep = np.ones(shape, bool)
                keep[y0:y0 + h, x0:x0 + w] = False
                assert np.array_equal(ref["out"][keep], np.minimum(frame, R.scale_of(in_depth))[keep])


def test_origin_off_by_one_is_seen():
    for shape, roi in (ODD, ALIGNED, PADDED):
        src, frame = make_case(shape, roi)
        ref = RR.paste(src, frame, roi)["out"]
        y0, x0, h, w = roi
        for moved in ((y0 + 1, x0, h, w), (y0 - 1, x0, h, w), (y0, x0 + 1, h, w), (y0, x0 - 1, h, w)):
            assert (RR.paste(src, frame, moved)["out"] != ref).any(), moved


def test_ramp_on_a_border_side_is_seen(monkeypatch):
    """A rectangle in a corner of the frame has ramps on its two inner sides only; ramps on all four change samples."""
    for shape, roi in CORNERS:
        src, frame = make_case(shape, roi)
        right = RR.paste(src, frame, roi, feather=3)
        y0, x0, h, w = roi
        H, W = shape
        assert int(right["ramp"].sum()) == h * w - (h - 3) * (w - 3)
        edge_rows = right["ramp"][0 if y0 == 0 else H - 1, x0 + 3 * (x0 > 0):x0 + w - 3 * (x0 + w < W)]
        assert not edge_rows.any()                                                 # the side on the frame's border: no ramp
        with monkeypatch.context() as mp:
            mp.setattr(RR, "weights", lambda H_, W_, roi_, f: (RR.axis_weights(roi_[2], f, f, f)[:, None], RR.axis_weights(roi_[3], f, f, f)[None, :]))
            wrong = RR.paste(src, frame, roi, feather=3)
        assert int(wrong["ramp"].sum()) == h * w - (h - 6) * (w - 6)
        assert (wrong["out"] != right["out"]).any()


def test_flag_follows_the_model_not_the_blend():
    """+inf on a ramp: the blend is +inf too and would clamp to D; the sample is 0 and the flag set, because the model's value decides."""
    shape, roi = ALIGNED
    y0, x0, h, w = roi
    src, frame = make_case(shape, roi)
    clean = RR.paste(src, frame, roi, feather=3)
    for v, at in ((np.inf, (1, 1, 20)), (-np.inf, (0, 10, 1)), (np.nan, (2, 15, 15))):
        s = src.copy()
        s[at] = v
        ref = RR.paste(s, frame, roi, feather=3)
        c, ry, rx = at
        assert ref["bad"] and ref["out"][y0 + ry, x0 + rx, c] == 0 and clean["out"][y0 + ry, x0 + rx, c] != 0
        assert ref["lo"][y0 + ry, x0 + rx, c] == 0 == ref["hi"][y0 + ry, x0 + rx, c]
        diff = ref["out"] != clean["out"]
        assert diff.sum() == 1
    # the mistake: the flag and the 0 read from the clamped blend, which is finite
    s = src.copy()
    s[1, 1, 20] = np.inf
    blend = np.clip(np.float64(1.0) * np.inf, 0, 255)
    assert np.isfinite(blend) and int(blend) == 255 != RR.paste(s, frame, roi, feather=3)["out"][y0 + 1, x0 + 20, 1]
    # NaN in the pad of a padded rectangle: never read
    shape, roi = PADDED
    src, frame = make_case(shape, roi)
    s = src.copy()
    s[:, roi[2]:, :] = np.nan
    s[:, :, roi[3]:] = np.inf
    for f in (0, 4):
        a, b = RR.paste(s, frame, roi, feather=f), RR.paste(src, frame, roi, feather=f)
        assert not a["bad"] and np.array_equal(a["out"], b["out"])


@pytest.mark.parametrize("shape,roi", [ODD, ALIGNED, PADDED] + CORNERS)
def test_float32_restatement_inside_the_float64_band(shape, roi):
    """The inputs of the GPU suite's feathered cases: the float32 evaluation lies in the band, and the band is open (lo != hi) for fewer
    than 1 % of the ramp samples, so it cannot hide a wrong blend."""
    for in_depth, out_depth in ((8, 8), (8, 10), (10, 10), (12, 8), (12, 12)):
        src, frame = make_case(shape, roi, in_depth)
        hard = RR.paste(src, frame, roi, in_depth, out_depth)["out"]
        for f in feathers(roi):
            ref = RR.paste(src, frame, roi, in_depth, out_depth, f)
            ramp = ref["ramp"]
            assert ramp.any() and not ref["bad"]
            out = ref["out"].astype(np.int64)
            assert ((ref["lo"] <= out) & (out <= ref["hi"])).all()
            assert np.array_equal(ref["out"][~ramp], hard[~ramp]) and np.array_equal(ref["lo"][~ramp], ref["hi"][~ramp])
            share = float((ref["lo"] != ref["hi"])[ramp].mean())
            assert share < 0.01, (in_depth, out_depth, f, share)
            assert (ref["out"] != hard)[ramp].mean() > 0.5                         # blended, not copied


def test_extent_restatement():
    f = np.zeros((2, 6, 8, 3), np.uint8)
    f[1, 2, 5] = (255, 255, 255)
    f[0, 4, 1] = (0, 0, 255)
    rows, cols = RR.extent(f)
    assert rows.tolist() == [0, 0, 255, 0, 29, 0] and cols.tolist() == [0, 29, 0, 0, 0, 255, 0, 0]
    deep = np.full((1, 2, 2, 3), 65535, np.uint16)
    assert RR.extent(deep, 10)[0].tolist() == [1023, 1023] and RR.extent(deep, 12)[1].tolist() == [4095, 4095]
