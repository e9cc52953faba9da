"""CPU suite for scene cuts in the clip API (speinet_amd/plan.py, under its own name): the cut rule `find_cuts` on hand-made statistics
and on translated edge scenes (against a numpy restatement of the pair-statistics kernel), the per-scene window plan
`window_plan(..., cuts=)`, and that the plan module loads neither the HIP library nor the clip loop."""
import os
import subprocess
import sys

import numpy as np
import pytest

from speinet_amd import plan as V, video
from speinet_amd.synth import synth_scene_u8

PIXELS = 6400


def luma(frames: np.ndarray) -> np.ndarray:
    f = frames.astype(np.int64)
    return (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8


def numpy_stats(frames: np.ndarray):
    """spei_frame_pair_stats restated: (sad [T-1], hist [T,64]) of uint8 frames [T,H,W,3]."""
    y = luma(frames)
    hist = np.stack([np.bincount((f >> 2).ravel(), minlength=64) for f in y])
    return np.abs(np.diff(y, axis=0)).sum(axis=(1, 2)), hist


def _hist(*bins) -> np.ndarray:
    """A 64-bin histogram of PIXELS pixels spread evenly over `bins`."""
    h = np.zeros(64, np.int64)
    h[list(bins)] = PIXELS // len(bins)
    return h


def _sad(d) -> np.ndarray:
    return (np.asarray(d, np.float64) * PIXELS).astype(np.int64)


def test_find_cuts_clean_cut():
    a, b = _hist(10, 11), _hist(40, 41)
    hist = np.stack([a, a, a, b, b, b])
    assert V.find_cuts(_sad([2, 2, 100, 2, 2]), hist, PIXELS) == [3]
    # half of the pixels move to other bins: g = 0.5
    half = (a + b) // 2
    assert V.find_cuts(_sad([2, 2, 50, 2, 2]), np.stack([a, a, a, half, half, half]), PIXELS) == [3]
    # every term can veto on its own: the histogram threshold, the SAD threshold, the ratio
    assert V.find_cuts(_sad([2, 2, 50, 2, 2]), np.stack([a, a, a, half, half, half]), PIXELS, hist_min=0.6) == []
    assert V.find_cuts(_sad([2, 2, 50, 2, 2]), np.stack([a, a, a, half, half, half]), PIXELS, min_delta=51.0) == []
    assert V.find_cuts(_sad([2, 2, 50, 2, 2]), np.stack([a, a, a, half, half, half]), PIXELS, min_delta=50.0) == [3]
    # two cuts three frames apart are outside each other's window of 2; with a window of 3 they veto each other
    hist = np.stack([a, a, b, b, b, a, a])
    assert V.find_cuts(_sad([2, 90, 2, 2, 90, 2]), hist, PIXELS) == [2, 5]
    assert V.find_cuts(_sad([2, 90, 2, 2, 90, 2]), hist, PIXELS, window=3) == []


def test_find_cuts_flash_is_no_cut():
    a, flash = _hist(10, 11), _hist(62, 63)
    hist = np.stack([a, a, a, flash, a, a, a])
    assert V.find_cuts(_sad([2, 2, 200, 200, 2, 2]), hist, PIXELS) == []
    assert V.find_cuts(_sad([2, 2, 200, 200, 2, 2]), hist, PIXELS, window=0) == [3, 4]      # the neighbourhood term is what vetoes


def test_find_cuts_brightness_step_is_no_cut():
    """Every pixel moves one bin up (g = 1) by a luma step of 4: d = 4 < min_delta."""
    a, b = _hist(10, 20, 30), _hist(11, 21, 31)
    hist = np.stack([a, a, a, b, b, b])
    assert V.find_cuts(_sad([1, 1, 4, 1, 1]), hist, PIXELS) == []
    assert V.find_cuts(_sad([1, 1, 4, 1, 1]), hist, PIXELS, min_delta=4.0) == [3]


def test_find_cuts_misses_equal_histograms():
    """The documented blind spot: two shots of one tonal distribution (here a frame and its mirror image) have g = 0."""
    r = np.random.RandomState(0)
    f = r.randint(0, 256, (40, 60, 3)).astype(np.uint8)
    clip = np.stack([f, f, f, f[:, ::-1], f[:, ::-1], f[:, ::-1]])
    sad, hist = numpy_stats(clip)
    assert sad[2] / (40 * 60) > 50 and np.array_equal(hist[2], hist[3])
    assert V.find_cuts(sad, hist, 40 * 60) == []


def test_find_cuts_two_frame_clip():
    a, b = _hist(10, 11), _hist(40, 41)
    assert V.find_cuts(_sad([100]), np.stack([a, b]), PIXELS) == [1]          # no neighbours: the third term holds vacuously
    assert V.find_cuts(_sad([2]), np.stack([a, a]), PIXELS) == []
    assert V.find_cuts(_sad([4]), np.stack([a, b]), PIXELS) == []


def test_find_cuts_validation():
    a = _hist(1)
    for sad, hist in (([1, 2], np.stack([a, a])), ([], np.stack([a])), ([1], a)):
        with pytest.raises(ValueError, match="find_cuts needs"):
            V.find_cuts(sad, hist, PIXELS)
    with pytest.raises(ValueError, match="pixels must be positive"):
        V.find_cuts([1], np.stack([a, a]), 0)


@pytest.mark.parametrize("seeds", [(1700, 5, 77), (3, 4, 5), (100, 200, 300)])
@pytest.mark.parametrize("h, w", [(40, 60), (37, 53), (90, 130)])
def test_find_cuts_on_edge_scenes(seeds, h, w):
    """Three translated edge scenes of 6, 5 and 7 frames (steps 1, 2, 1): the rule with its defaults finds exactly the two joins."""
    clip = np.concatenate([synth_scene_u8(t, h, w, s, step) for t, s, step in zip((6, 5, 7), seeds, (1, 2, 1))])
    assert clip.shape == (18, h, w, 3) and clip.dtype == np.uint8
    sad, hist = numpy_stats(clip)
    assert (hist.sum(axis=1) == h * w).all()
    assert V.find_cuts(sad, hist, h * w) == [6, 11]


# ---- the per-scene window plan -------------------------------------------------------------------------------------------------------
def _shifted(plan, at):
    """A scene's plan with its local frame indices mapped through `at` (local index -> index in the whole clip)."""
    out = []
    for p in plan:
        out.append({"index": at[p["index"]], "window": [at[i] for i in p["window"]], "pre": at[p["pre"]], "sub": at[p["sub"]],
                    "zero_pre": p["zero_pre"], "zero_sub": p["zero_sub"], "keys": [k if k is V.ZERO else at[k] for k in p["keys"]]})
    return out


def _by_scene(labels, numbers, cuts):
    """The definition: every scene planned as a clip of its own; a one-frame scene {i} as the first entry of the clip [i, i]."""
    T = len(labels)
    out = []
    for a, b in zip([0] + list(cuts), list(cuts) + [T]):
        if b - a == 1:
            out += _shifted(V.window_plan([labels[a]] * 2, numbers=[numbers[a]] * 2)[:1], [a, a])
        else:
            out += _shifted(V.window_plan(labels[a:b], numbers=numbers[a:b]), list(range(a, b)))
    return out


@pytest.mark.parametrize("labels, cuts", [
    ([0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 1, 0], [6, 11]),      # 0, 1 and several sharp frames per scene
    ([0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0], [6, 13]),      # a sharp frame on each side of a cut
    ([1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 1, 0], [6, 7]),                          # a one-frame scene, sharp
    ([1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 1, 0], [5, 6]),                          # a one-frame scene, blurry
    ([1, 0, 1, 1], [1, 2, 3]),                                               # one-frame scenes only
    ([0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1], [2]),             # a long scene whose far references are zeroed
])
def test_window_plan_with_cuts_is_the_plan_of_each_scene(labels, cuts):
    T = len(labels)
    for numbers in (list(range(T)), [100 + 2 * i + (i // 5) * 3 for i in range(T)]):
        plan = V.window_plan(labels, numbers=numbers, cuts=cuts)
        assert plan == _by_scene(labels, numbers, cuts)
        assert [p["index"] for p in plan] == list(range(T))
        bounds = [0] + cuts + [T]
        for p in plan:
            a, b = next((a, b) for a, b in zip(bounds, bounds[1:]) if a <= p["index"] < b)
            assert all(a <= k < b for k in p["keys"] if k is not V.ZERO), p          # nothing crosses a cut
            assert p["window"][1] == p["index"]
    assert V.window_plan(labels, cuts=cuts) == V.window_plan(labels, numbers=list(range(T)), cuts=cuts)
    assert V.window_plan(np.asarray(labels), cuts=np.asarray(cuts)) == V.window_plan(labels, cuts=cuts)


def test_sharp_frame_across_a_cut_is_not_chosen():
    labels = [1, 0, 0, 0, 1, 0, 1, 0, 0, 1, 0, 0]
    whole, cut = V.window_plan(labels), V.window_plan(labels, cuts=[6])
    # one scene: frames 4 and 5 take the sharp frame 6 as their later reference, frame 6 the sharp frame 4 as its earlier one
    assert (whole[4]["sub"], whole[5]["sub"], whole[6]["pre"]) == (6, 6, 4)
    assert whole[5]["window"] == [4, 5, 6] and whole[6]["window"] == [5, 6, 7]
    # two scenes: each side keeps to its own sharp frames, and the windows reflect at the cut
    assert (cut[4]["sub"], cut[5]["sub"], cut[6]["pre"]) == (4, 4, 6)
    assert cut[5]["window"] == [4, 5, 4] and cut[6]["window"] == [7, 6, 7]
    assert all(k < 6 for p in cut[:6] for k in p["keys"] if k is not V.ZERO)
    assert all(k >= 6 for p in cut[6:] for k in p["keys"] if k is not V.ZERO)


def test_one_frame_scene():
    plan = V.window_plan([1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 1, 0], cuts=[6, 7])
    assert plan[6]["window"] == [6, 6, 6] and plan[6]["index"] == 6
    assert all(k is V.ZERO or k == 6 for k in plan[6]["keys"])


def test_no_cuts_is_todays_plan():
    labels = [0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0]
    numbers = [3 * i for i in range(len(labels))]
    for kw in ({}, {"numbers": numbers}):
        assert V.window_plan(labels, cuts=None, **kw) == V.window_plan(labels, **kw) == V.window_plan(labels, cuts=[], **kw)
    assert V.window_plan(labels) != V.window_plan(labels, cuts=[5])


@pytest.mark.parametrize("cuts, message", [
    ([0], "outside 1..9"),
    ([10], "outside 1..9"),
    ([-1], "outside 1..9"),
    ([3, 3], "strictly increasing"),
    ([5, 2], "strictly increasing"),
    ([2.5], "whole frame indices"),
    ([[1, 2]], "flat sequence"),
    (["a"], "whole frame indices"),
    ("auto", "sequence of frame indices"),
    (4, "sequence of frame indices"),
])
def test_cut_validation(cuts, message):
    with pytest.raises(ValueError, match=message):
        V.window_plan([0] * 10, cuts=cuts)
    if cuts != "auto":
        with pytest.raises(ValueError, match=message):
            video.deblur_clip(None, np.zeros((10, 30, 30, 3), np.uint8), [0] * 10, cuts=cuts)


def test_deblur_clip_cut_arguments():
    frames = np.zeros((10, 30, 30, 3), np.uint8)
    with pytest.raises(ValueError, match='"auto"'):
        video.deblur_clip(None, frames, [0] * 10, cuts="yes")
    with pytest.raises(ValueError, match="find_cuts takes"):
        video.deblur_clip(None, frames, [0] * 10, cuts="auto", cut_params={"threshold": 1})


def test_read_cuts(tmp_path):
    np.save(tmp_path / "cuts.npy", np.asarray([6, 11]))
    (tmp_path / "cuts.txt").write_text("6\n11\n")
    (tmp_path / "none.txt").write_text("")
    assert video.read_cuts(str(tmp_path / "cuts.npy")) == [6, 11] == video.read_cuts(str(tmp_path / "cuts.txt"))
    assert video.read_cuts(str(tmp_path / "none.txt")) == []
    with pytest.raises(ValueError):
        (tmp_path / "bad.txt").write_text("6 x")
        video.read_cuts(str(tmp_path / "bad.txt"))


def test_plan_module_stands_alone():
    """In a fresh interpreter (this one imported the clip loop long ago), importing the plan loads neither the HIP library's wrapper
    nor the clip loop, and the clip loop hands out the plan's names as its own."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; import speinet_amd.plan as P; "
            "bad = [m for m in ('ops', 'video', 'clip', 'detector', '_lib') if 'speinet_amd.' + m in sys.modules]; "
            "assert not bad, bad; assert P.find_cuts and P.StreamPlan and P.CUT_PARAMS == ('hist_min', 'ratio', 'min_delta', 'window')")
    done = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
    for name in ("ZERO", "CUT_PARAMS", "ASSUMED_TAIL", "MIN_HORIZON", "labels_of", "cuts_of", "find_cuts", "StreamCuts", "window_plan", "StreamPlan"):
        assert getattr(video, name) is getattr(V, name)


def test_header_declares_pair_stats():
    from speinet_amd import _lib
    import ctypes
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert _lib.SIGNATURES["spei_frame_pair_stats"] == (I, [P, L, P, I, I, I, P, P, P])
