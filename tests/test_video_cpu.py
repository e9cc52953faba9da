"""CPU suite for the clip API (speinet_amd/video.py): the reflect-pad indices of the ingest kernel, input validation, the window plan
against the harness's for the G11 selection cases, and the two frame I/O entry points in the C-ABI header."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from speinet_amd import _lib, selection
from speinet_amd import video as V


def test_reflect_index_matches_f_pad():
    for n in range(20, 81):
        npad = V.padded_size(n)
        assert npad % 20 == 0 and 0 <= npad - n < 20
        x = torch.arange(n, dtype=torch.float32).view(1, 1, n, 1)
        ref = F.pad(x, (0, 0, 0, npad - n), mode="reflect").view(-1).long().numpy()
        assert np.array_equal(V.reflect_index(n), ref), n
        xw = torch.arange(n, dtype=torch.float32).view(1, 1, 1, n)
        assert np.array_equal(V.reflect_index(n), F.pad(xw, (0, npad - n, 0, 0), mode="reflect").view(-1).long().numpy()), n
    with pytest.raises(ValueError, match="pad smaller"):
        V.reflect_index(5, 20)


def _u8(*shape):
    return np.zeros(shape, np.uint8)


@pytest.mark.parametrize("frames, labels, message", [
    (_u8(1, 30, 30, 3), None, "at least 2 frames"),
    ([_u8(30, 30, 3)], None, "at least 2 frames"),
    (np.zeros((3, 30, 30, 3), np.float32), None, "must be uint8"),
    (torch.zeros(3, 30, 30, 3), None, "must be uint8"),
    ([_u8(30, 30, 3), np.zeros((30, 30, 3), np.int16)], None, "must be uint8"),
    (_u8(3, 30, 30, 4), None, "3-channel"),
    ([_u8(30, 30), _u8(30, 30)], None, "3-channel"),
    (_u8(3, 30, 30), None, r"\[T,H,W,3\]"),
    (_u8(3, 19, 30, 3), None, "at least 20x20"),
    ([_u8(30, 19, 3), _u8(30, 19, 3)], None, "at least 20x20"),
    ([_u8(30, 30, 3), _u8(30, 40, 3)], None, "mixed frame sizes"),
    ([_u8(30, 30, 3), "a.png"], None, "mixes image paths and arrays"),
    ([_u8(30, 30, 3), 7], None, "not an array"),
    (7, None, "indexable sequence"),
    (_u8(3, 30, 30, 3), [0, 1], "2 entries for a clip of 3"),
    (_u8(3, 30, 30, 3), [0, 1, 2], "0 \\(blurry\\) or 1 \\(sharp\\)"),
])
def test_validation_errors(frames, labels, message):
    with pytest.raises(ValueError, match=message):
        V.deblur_clip(None, frames, labels)


def test_validation_of_image_files(tmp_path):
    from PIL import Image
    for name, (h, w) in {"a.png": (30, 40), "b.png": (30, 40), "c.png": (31, 40), "d.png": (19, 40)}.items():
        Image.fromarray(np.zeros((h, w, 3), np.uint8)).save(tmp_path / name)
    fr = V.frames_of([str(tmp_path / "a.png"), tmp_path / "b.png"])
    assert (fr.T, fr.H, fr.W, fr.paths) == (2, 30, 40, True)
    with pytest.raises(ValueError, match="mixed frame sizes"):
        V.deblur_clip(None, [str(tmp_path / "a.png"), str(tmp_path / "c.png")])
    with pytest.raises(ValueError, match="at least 20x20"):
        V.deblur_clip(None, [str(tmp_path / "a.png"), str(tmp_path / "d.png")])
    with pytest.raises(ValueError, match="out must be"):
        V.deblur_clip(None, _u8(3, 30, 30, 3), out=torch.empty(3, 30, 30, 3))


def _harness_plan(labels, numbers=None):
    """The harness's selection run directly (selection.assemble_windows on frame files whose names carry `numbers`, default the
    indices): routing, zeroed references and the frames of each window, as frame numbers."""
    numbers = list(range(len(labels))) if numbers is None else numbers
    frames = [f"clip/{n:06d}.png" for n in numbers]
    out = []
    for w in selection.assemble_windows(frames, np.asarray(labels)):
        keys = list(w["window"]) + [("zero", 0, 0) if w["zero_pre"] else w["pre"], ("zero", 0, 0) if w["zero_sub"] else w["sub"]]
        out.append((int(w["name"]), bool(w["zero_pre"]), bool(w["zero_sub"]),
                    [None if isinstance(k, tuple) else selection.frame_number(k) for k in keys]))
    return out


def test_window_plan_equals_harness_plan(golden_dir):
    g11 = json.load(open(os.path.join(golden_dir, "g11_selection.json")))
    assert len(g11) >= 5
    routed, renumbered = set(), 0
    for name, d in g11.items():
        plan = V.window_plan(d["labels"])
        mine = [(p["index"], p["zero_pre"], p["zero_sub"], [None if k is V.ZERO else k for k in p["keys"]]) for p in plan]
        assert mine == _harness_plan(d["labels"]), name
        assert [p["index"] for p in plan] == list(range(len(d["labels"])))
        for p in plan:
            assert p["keys"][:3] == p["window"] and p["window"][1] == p["index"]
            assert (p["keys"][3] is V.ZERO) == p["zero_pre"] and (p["keys"][4] is V.ZERO) == p["zero_sub"]
            routed.add(p["zero_pre"])
        # frame numbers that are not the indices (gaps, an offset): the references are zeroed by the numbers, the keys stay indices
        numbers = [100 + 2 * i + (i // 5) * 3 for i in range(len(d["labels"]))]
        plan_n = V.window_plan(d["labels"], numbers=numbers)
        mine_n = [(numbers[p["index"]], p["zero_pre"], p["zero_sub"], [None if k is V.ZERO else numbers[k] for k in p["keys"]]) for p in plan_n]
        assert mine_n == _harness_plan(d["labels"], numbers), name
        renumbered += [(p["zero_pre"], p["zero_sub"]) for p in plan_n] != [(p["zero_pre"], p["zero_sub"]) for p in plan]
    assert routed == {True, False}
    assert renumbered > 0          # the numbering changed which references are zeroed in some case


def test_header_declares_frame_io():
    syms = _lib.header_symbols()
    for s in ("spei_frames_u8_in", "spei_frame_u8_out"):
        assert s in syms and s in _lib.SIGNATURES
    text = open(_lib.HEADER_PATH).read()
    assert "int spei_frames_u8_in(const unsigned char* src, int64_t frame_stride, float* dst, float* gray, int N, int H, int W, " in text
    assert "int spei_frame_u8_out(const float* src, unsigned char* dst, int* nonfinite, int H, int W, int Hp, int Wp, spei_stream_t stream);" in text
    from speinet_amd.build import sources
    assert "frame_io.hip" in sources()
