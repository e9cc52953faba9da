"""`deblur_clip`'s argument checks as one table: every call violates one rule (a few violate two, to pin the order of the checks) and
names the exception and its text.  What the whole-clip mode and the stream mode share runs in both: on an array, and on an iterator
of the same frames with `stream=True`.  The model is None: every refusal comes before the model is looked at."""
import numpy as np
import pytest
import torch

from speinet_amd import video

T, H, W = 8, 20, 24
FRAMES = np.zeros((T, H, W, 3), np.uint8)

# (id, keyword arguments, text) of a ValueError in both modes
SHARED = [
    ("roi_outside", dict(roi=(0, 0, 30, 30)), r"roi \(0, 0, 30, 30\): the rectangle lies outside the 24x20 frame"),
    ("roi_small", dict(roi=(0, 0, 10, 20)), r"roi \(0, 0, 10, 20\): the rectangle must be at least 20x20"),
    ("roi_feather_over", dict(roi=(0, 2, 20, 20), roi_feather=11), r"roi_feather=11 is outside 0\.\.10: at most 200 and half of the 20x20 rectangle"),
    ("roi_feather_alone", dict(roi_feather=2), r"roi_feather=2 needs roi="),
    ("roi_feather_type", dict(roi=(0, 2, 20, 20), roi_feather=1.5), r"roi_feather must be a whole number >= 0, got 1\.5"),
    ("roi_string", dict(roi="bars"), r"roi must be None, \"auto\" or four whole numbers"),
    ("roi_tiles", dict(roi=(0, 2, 20, 20), tiles=(1, 1)), r"roi= with tiles= is not built"),
    ("roi_crop", dict(roi=(0, 2, 20, 20), crop=True), r"roi= with crop=True"),
    ("out_depth", dict(out_depth=9), r"out_depth must be None, 8, 10 or 12, got 9"),
    ("cuts_string", dict(cuts="scenes"), r"cuts must be None, \"auto\" or a sequence of frame indices, got 'scenes'"),
    ("cut_params", dict(cut_params={"ratio": 2.0, "sigma": 1}), r"cut_params holds \['sigma'\]: find_cuts takes hist_min, ratio, min_delta and window"),
    ("bar_params", dict(bar_params={"level": 20, "rows": 1}), r"bar_params holds \['rows'\]: find_bars takes level and min_bar"),
    ("feather_alone", dict(feather=4), r"feather=4 needs tiles="),
    ("tiles_grid", dict(tiles=(9, 1)), r"a tile grid has 1\.\.8 rows and columns, got \(9, 1\)"),
    ("tiles_feather", dict(tiles=(1, 2), shave=4, feather=5), r"feather must be a whole number 0\.\.shave \(4\)"),
    ("ensemble", dict(ensemble=3), r"ensemble must be 1, 2, 4 or 8"),
    ("stream_value", dict(stream=1.5), r"stream must be False, True or \"force\", got 1\.5"),
    # two violations: the check that comes first speaks
    ("roi_before_out_depth", dict(roi=(0, 0, 30, 30), out_depth=9), r"the rectangle lies outside"),
    ("out_depth_before_cut_params", dict(out_depth=9, cut_params={"sigma": 1}), r"out_depth must be"),
    ("cuts_before_tiles", dict(cuts="scenes", tiles=(9, 1)), r"cuts must be None"),
    ("ensemble_before_feather", dict(ensemble=3, feather=4), r"ensemble must be"),
    ("cut_params_before_tiles", dict(cut_params={"sigma": 1}, tiles=(9, 1)), r"cut_params holds"),
]

WHOLE = [
    ("labels_length", dict(labels=[1, 0]), ValueError, r"labels has 2 entries for a clip of 8 frames"),
    ("labels_values", dict(labels=[2] * T), ValueError, r"labels must be 0 \(blurry\) or 1 \(sharp\) per frame"),
    ("numbers_length", dict(numbers=[0, 1]), ValueError, r"numbers has 2 entries for a clip of 8 frames"),
    ("out_dtype", dict(out=torch.zeros((T, H, W, 3), dtype=torch.float32)), ValueError, r"out must be a contiguous uint8 \[8,20,24,3\] tensor \(out_depth 8\)"),
    ("out_shape", dict(out=torch.zeros((T - 1, H, W, 3), dtype=torch.uint8)), ValueError, r"out must be a contiguous uint8 \[8,20,24,3\] tensor"),
    ("cuts_zero", dict(cuts=[0]), ValueError, r"cut 0 is outside 1\.\.7"),
    ("cuts_repeated", dict(cuts=[5, 5]), ValueError, r"cuts must be strictly increasing, got \[5, 5\]"),
    ("cuts_scalar", dict(cuts=3), ValueError, r"cuts must be a sequence of frame indices, got 3"),
    ("stream_on_array", dict(stream=True), ValueError, r"stream=True on a clip whose length is known"),
    ("out_depth_before_labels", dict(out_depth=9, labels=[1, 0]), ValueError, r"out_depth must be"),
    ("labels_before_cuts", dict(labels=[1, 0], cuts="scenes"), ValueError, r"labels has 2 entries"),
    ("numbers_before_out", dict(numbers=[0, 1], out=torch.zeros(1)), ValueError, r"numbers has 2 entries"),
]

STREAM = [
    ("iterator_without_stream", dict(stream=False), ValueError, r"its length is not known, pass stream=True"),
    ("out", dict(out=torch.zeros((T, H, W, 3), dtype=torch.uint8)), ValueError, r"out= with stream=True"),
    ("numbers", dict(numbers=list(range(T))), ValueError, r"numbers= with stream=True"),
    ("roi_auto", dict(roi="auto"), ValueError, r"roi=\"auto\" with stream=True"),
    ("out_before_roi", dict(out=torch.zeros(1), roi=(0, 0, 30, 30)), ValueError, r"out= with stream=True"),
    # bad label values: refused by the argument checks, or (the model being None) not before `ClipRun` has looked at the model
    ("labels_values", dict(labels=[2] * T), (ValueError, AttributeError), r"labels must be 0 \(blurry\) or 1 \(sharp\) per frame|parameters"),
]


def _call(frames, kw):
    kw = dict(kw)
    return video.deblur_clip(None, frames, kw.pop("labels", None), **kw)


@pytest.mark.parametrize("mode", ["whole", "stream"])
@pytest.mark.parametrize("name,kw,text", SHARED, ids=[c[0] for c in SHARED])
def test_shared_refusals(name, kw, text, mode):
    with pytest.raises(ValueError, match=text):
        _call(FRAMES, kw) if mode == "whole" else _call(iter(list(FRAMES)), dict({"stream": True}, **kw))


@pytest.mark.parametrize("name,kw,exc,text", WHOLE, ids=[c[0] for c in WHOLE])
def test_whole_clip_refusals(name, kw, exc, text):
    with pytest.raises(exc, match=text):
        _call(FRAMES, kw)


@pytest.mark.parametrize("name,kw,exc,text", STREAM, ids=[c[0] for c in STREAM])
def test_stream_refusals(name, kw, exc, text):
    with pytest.raises(exc, match=text):
        _call(iter(list(FRAMES)), dict({"stream": True}, **kw))


def test_stream_force_refusal():
    with pytest.raises(ValueError, match="takes an array or a list of host frames"):
        video.deblur_clip(None, "clip.png", stream="force")
