"""The clip loop: deblur a clip of uint8 (or 10- / 12-bit uint16) frames of any size (at least 20x20), with or without sharpness labels.  The library API is
`deblur_clip`; the command line, for the user's own footage (no ground truth), is

    python -m speinet_amd.video --input <dir | glob | clip.y4m | -> --output <dir | out.y4m | -> --model_path <checkpoint | synthetic>
                                [--labels <file.npy>] [--detector <detector.json>] [--cuts none|auto|<file>]
                                [--matrix bt601|bt709] [--range full|limited] [--fps num:den]
                                [--chroma 420jpeg|420mpeg2|422|444|mono] [--out_chroma 420jpeg|420mpeg2|422|444|mono]
                                [--out_depth 8|10|12] [--tiles none|auto|RxC] [--shave N] [--feather N] [--ensemble 1|2|4|8]
                                [--roi none|auto|matte|Y,X,H,W] [--roi_feather N] [--stream [--horizon N]] [--sharp deblur|keep]
                                [--fields auto|progressive|split] [--matte <image | dir | glob | matte.y4m> [--matte_invert]]
                                [--matte auto [--matte_params thr=192,flat=2,grow=1,hold=1]] [--matte_out <matte.y4m>]

(`-`: a YUV4MPEG2 stream on stdin / stdout, as `ffmpeg -f yuv4mpegpipe` writes and reads it; by default stdin is spooled to a temporary
file on disk before the first frame is deblurred, with `--stream` it is deblurred as it arrives, see `main`)

and the dataset harness (speinet_amd.inference) runs every clip through `deblur_clip` as well, adding its ground truth and metrics.
  * labels — given (0/1 per frame, 1 = sharp), or computed by the LD detector (speinet_amd.detector) in a first streaming pass over the
    clip in batches of 16 frames: gray planes from the ingest kernel, focus measures, logistic regression;
  * the window plan — speinet_amd.plan (host-only; its public names are this module's too): `window_plan` runs
    `selection.assemble_windows` on the frame numbers, every scene between two cuts (`cuts`: given, or found by `find_cuts` from the
    pair statistics of the labelling pass) as a clip of its own, so no window and no reference frame crosses a cut;
  * the windows — `forward_window` with a per-clip `EncoderCache`, `prefetch_window` one window ahead, windows alternating over two
    launch streams that the model keeps, in whatever `precision` / `corr_precision` / `use_graph` / `streams` the caller set on it;
  * the frames come from speinet_amd.clip (`frames_of`, `FrameCache`); a window whose 16-bit pass left a non-finite value is recomputed in bf16x3;
  * a y4m clip (speinet_amd.y4m) crosses PCIe as its planar bytes, 1.5 per pixel for 4:2:0, and becomes packed RGB on the device
    (csrc/yuv_io.hip, integer arithmetic); a y4m output is made there from the deblurred frame the same way;
  * 4:2:2 and mono streams (`C422`, `C422p10`, `C422p12`, `Cmono`, `Cmono10`, `Cmono12`: what `ffmpeg -pix_fmt yuv422p10le` or `gray10le`
    `-f yuv4mpegpipe` writes) take the same road at 2 and 1 samples per pixel: `deblur_clip` and the command line open their readers
    with `layouts=y4m.LAYOUTS`, and everything behind `Frames.rgb` sees packed RGB.  `--out_chroma` writes the y4m output in another
    layout than the input's (4:2:2 in and 4:2:0 out for delivery, 4:2:0 in and 4:4:4 out to avoid a second subsampling);
  * a deep clip (10 or 12 bits per sample: a `C420p10` ... `C444p12` y4m stream, or uint16 frames with `depth=`) never passes through
    8 bits: its bytes cross PCIe through the same page-locked rings, the labelling pass, the scene statistics and the window loop
    read uint16 frames (`ops.frames_u16_in`, `ops.frame_pair_stats_u16`), and the deblurred frame is quantised once, to `out_depth`
    (`ops.frame_u16_out`).  Image files stay 8-bit.
  * a large frame can be deblurred as a grid of overlapping tiles (`tiles=`, `--tiles`; speinet_amd.tiles, csrc/tile_io.hip): what the
    reference's `forward_chop` does with four quadrants.  The frames are still uploaded, labelled and planned whole; every window
    then runs once per tile, all tiles of one shape (one set of captured graphs, one encoder cache with keys per tile), and one
    launch stitches the tiles' bands into the frame: with hard seams and no blending by default, as the reference does, or
    (`feather=`, `--feather`) blending the margins that both tiles of a seam computed over a ramp of 2 * feather pixels around it
    (`tiles.seam_ramps`, `ops.tiles_out`).  Off by default.
  * geometric self-ensemble (`ensemble=`, `--ensemble`; speinet_amd.ensemble, csrc/ensemble_io.hip): every window also runs on the
    mirrored, upside-down and (for 8) transposed copies of its padded input, made on the device by one launch per member
    (`ops.planes_d4`), and one launch transforms the members' outputs back and averages them in float32 in a fixed order
    (`ops.d4_mean`) in front of the unchanged egress: what the reference's `forward_x8` does on the host, and never calls.  K members
    cost K forward passes.  Off by default.
  * a region of interest (`roi=`, `--roi`; csrc/roi_io.hip): only a rectangle of every frame is deblurred, given, or found as the
    active picture area of letterboxed or pillarboxed footage ("auto": `active_area`, one `ops.frame_extent` launch per batch of
    sampled frames, and the bar rule `find_bars`).  The frames are still uploaded and cached whole; the labelling pass, the scene
    statistics and the window plan see the cropped frames; the rectangle is ingested by the tile ingest with a table of one tile
    (`ops.roi_in`) and one launch pastes the model's output into the otherwise untouched frame (`ops.roi_paste`), with a hard edge
    or (`roi_feather=`, `--roi_feather`) blended with the input over a ramp inside the rectangle.  Off by default.
  * a stream (`stream=True`, `--stream`): a clip whose length is not known (a `y4m.Y4MStream` on a pipe, an iterator of frames) is read
    by one thread into a bounded ring of page-locked frames (`clip.StreamFrames`); the labelling pass and the scene statistics run in the
    same batches as frames arrive (`detector.clip_analysis`) and feed `plan.StreamPlan`, which hands out the entries of `window_plan`
    after a look-ahead of at most `horizon` frames (`ClipRun.assumed` lists the frames it planned under its assumption).  The loop
    asks its plan source whether frame k is planned yet (`_WholePlan`: always; `_ArrivingPlan`: after analysing as far as needed) and
    is otherwise the whole clip's, launch for launch: every frame outside `assumed` is bit-identical.  Host memory is bounded by
    the look-ahead.  Off by default.
  * sharp frames kept (`sharp="keep"`, `--sharp keep`; csrc/frame_io.hip `spei_frame_requant`): no window runs for a frame labelled
    sharp; it is handed out as the input frame at the output depth by one `ops.frame_requant` launch on the home stream and takes no
    lane, launch slot or flag slot.  The other frames keep their plan entries and their bits: a sharp frame is still a neighbour and a
    reference.  The window after a kept frame has no encoder prefetch and computes what it misses in `forward_window` (the same
    values); the frame cache is asked for a kept frame itself.  The command line writes a kept y4m frame as the record it read, byte
    for byte, when the output has the input's chroma layout, depth and range.  An extension beyond the reference, which deblurs every
    frame; no trained checkpoint exists here, so nothing is claimed about quality, nor about a visible step between a kept frame and
    its deblurred neighbours.  Off by default.
  * interlaced clips (`fields="split"`, `--fields`; csrc/field_io.hip, the field entries of csrc/yuv_io.hip): a frame of even height
    is two fields, field p its rows p::2, two different instants.  Each parity is deblurred as a clip of its own: frame k of the
    result has, in its rows p::2, frame k of `deblur_clip` on the clip of the fields of parity p, bit for bit, both under ONE plan,
    the top-field clip's labels and cuts (or the caller's).  A window runs as two parts of one shape (H / 2 x W, each field with its
    own reflect pad), one launch splits a frame into both fields' planes (`ops.fields_in`) and one weaves the two outputs into the
    frame (`ops.fields_out`); the analysis pass sees the top-field clip (`Frames.field(0)`), and a 4:2:0 y4m clip is converted field
    by field (`ops.yuv_to_rgb_u8(..., fields=True)`), so no chroma of one instant reaches the other.  Same-parity windows have
    frame-rate spacing and no half-line bob between neighbours (one clip of 2T alternating fields would bob: rejected); field order
    therefore does not enter the result, `It` and `Ib` differ in the tag that is passed through; `Im` stays refused.  An extension
    beyond the reference; no trained checkpoint exists here, so nothing is claimed about quality.  Off by default.
  * mattes (`matte=`, `--matte`; csrc/matte_io.hip `spei_frame_matte_u8` / `_u16`): an 8-bit mask, one for the clip or one per frame
    (`clip.mattes_of`), says how much of the deblurred frame every pixel gets: with a the input sample at the output depth, b the
    sample the run without a matte hands out and m the matte byte, every sample is (a * (255 - m) + b * m + 127) // 255, exact
    integers.  One more launch on the packed frame, in place, behind whichever egress ran (`ops.frame_matte`), also behind a bf16x3
    recompute's; the window's centre input frame is kept for it as for the ROI paste, and the mattes are uploaded through a
    `FrameCache` of their own.  A frame whose matte is empty takes the kept-frame path (`ClipRun.unmatted`), and `roi="matte"` is the
    mattes' bounding box, grown by 20 pixels.  An extension beyond the reference; no trained checkpoint exists here, so nothing is
    claimed about quality.  Off by default.
  * automatic blur mattes (`matte="auto"`, `--matte auto`; csrc/blur_map.hip, speinet_amd/blurmap.py): the mattes are measured, one per
    frame, on the device.  Per cell of 16x16 pixels and per direction the re-blur measure says how much of the adjacent-pixel variation
    a 9-tap box removes (`ops.blur_cells`, one launch per analysis batch, in the labelling pass where that sees the full frames); frame
    k's cell map is the maximum over the frames of plan entry k's window, dilated, and its matte the bilinear interpolation between cell
    centres (`ops.blur_matte`, one launch per matted frame).  `blurmap.AutoMattes` stands where a `clip.Mattes` does, so everything
    behind the matte is the given matte's.  Four untuned design parameters (`matte_params=`).  An extension beyond the reference; no
    trained checkpoint exists here, so nothing is claimed about quality.  Off by default.
A frame whose size is not a multiple of 20 is padded at the bottom and right by reflection (torch F.pad mode "reflect", the padding
SwinIR's `check_image_size` uses for window multiples) and the result is cropped back: csrc/frame_io.hip does both, the padding on
the way in (with `numpy2tensor`'s values) and the crop on the way out (with `tensor2numpy`'s rounding).  The reference cannot run
such sizes at all; its harness crops the frames to multiples of 20 instead, which `crop=True` does (on the host, as each frame is
loaded).  Device memory is bounded by one window, the encoder cache and the windows in flight: it does not grow with the clip's length.
"""
from __future__ import annotations

import argparse
import collections
import glob
import os
import sys
import time
import warnings
from concurrent.futures import ThreadPoolExecutor
from typing import Optional

import numpy as np
import torch

from . import blurmap, detector, engine, ensemble as ens, ops, tiles as tiling, y4m
from .blurmap import MATTE_PARAMS, BlurParams  # noqa: F401
from .clip import (IMAGE_EXTS, MIN_SIZE, FrameCache, Frames, HostRing, Mattes, RecordQueue, frames_of, imread, imwrite, mattes_of,  # noqa: F401
                   padded_size, reflect_index)
from .plan import (ASSUMED_TAIL, CUT_PARAMS, MIN_HORIZON, ZERO, StreamCuts, StreamPlan, cuts_of, find_cuts, labels_of,  # noqa: F401
                   window_plan)
from .speinet import EncoderCache

_imread, _imwrite = imread, imwrite

CORR_PRECISION = {"f32": "bf16x3", "bf16x3": "bf16x3", "bf16": "top2", "f16": "top2"}    # correlation arithmetic per precision
DETECT_BATCH = 16                # frames per launch of the labelling pass (the harness's batch)
PREFETCH = 4                     # windows decoded ahead of the GPU
LANES = 2                        # launch streams the windows alternate over (3 and 4 measured 8-25 % slower than 2 on 720p)
LAG = 2                          # windows enqueued after a frame before it is handed out
FLAG_RING = 8                    # non-finite flags in flight (> LAG + 1)
READY_MAX = LAG + 2              # finished or queued frames held back at most (kept frames among them; < FLAG_RING, and a stream's look-back)


def scene_stats(frames, device):
    """The pair statistics of a clip (anything `frames_of` accepts) in one streaming pass of DETECT_BATCH frames at a time on `device`
    (`detector.clip_pass`: the labelling pass's uploader; `ops.frame_pair_stats` per batch, the last frame of a batch carried over as
    `prev` of the next): (sad int64 [T-1], hist int64 [T,64]) as numpy arrays, the input of `find_cuts`.  A deep clip (a `Frames`
    of `frames_of(..., depth=)`, or a deep y4m reader) goes through `ops.frame_pair_stats_u16`, and its sad comes back divided by
    2^(depth-8), as float64, so that `find_cuts`' `min_delta` keeps its 8-bit unit."""
    fr = frames if isinstance(frames, Frames) else frames_of(frames)
    return _host_stats(detector.clip_pass(fr, device, batch=DETECT_BATCH, features=False, pair_stats=True)[1], fr.depth)


def _host_stats(stats, depth: int):
    """Pair statistics (sad, hist) on the device as the host arrays `find_cuts` takes: the SAD of a clip of `depth` bits in the 8-bit
    unit of `min_delta` (an exact division by a power of 2)."""
    sad, hist = stats[0].cpu().numpy(), stats[1].cpu().numpy()
    return (sad if depth == 8 else sad / float(1 << (depth - 8))), hist


BAR_PARAMS = ("level", "min_bar", "frames")       # `bar_params`: find_bars' keywords, and the number of frames `active_area` scans
ROI_FEATHER_MAX = ops.ROI_FEATHER_MAX


def find_bars(rowmax, colmax, depth: int = 8, *, level: int = 24, min_bar: int = 4):
    """The active picture area of a clip from its extent maxima (`active_area`): rowmax [H], colmax [W], the maximum over every row
    and every column of the clip's integer luma at `depth` bits.  A line is black iff its maximum is at most level << (depth - 8);
    top, bottom, left and right are the numbers of leading / trailing black rows and columns; a bar of fewer than `min_bar` lines
    counts as none (a dark edge line is not a bar).  Returns the rectangle (y0, x0, h, w) that is left, or None when no bar is left
    (the whole frame is picture) or when the rest is smaller than 20x20 (a black clip).

    `level` and `min_bar` are design parameters, not measurements: limited-range black is 16 and compression leaves a few levels of
    noise above it, hence 24; nobody has tuned either on real footage, which is why they are keywords (`bar_params=`).  Blind spots: a
    logo or a subtitle inside a bar ends the bar there; a scene darker than `level` along a whole edge reads as a bar (scan more frames)."""
    if isinstance(depth, bool) or depth not in y4m.DEPTHS:
        raise ValueError(f"find_bars: depth must be 8, 10 or 12, got {depth!r}")
    for name, v in (("level", level), ("min_bar", min_bar)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError(f"find_bars: {name} must be a whole number >= 0, got {v!r}")
    rows, cols = np.asarray(rowmax).reshape(-1), np.asarray(colmax).reshape(-1)
    thr = int(level) << (depth - 8)

    def lead(a) -> int:
        lit = np.flatnonzero(a > thr)
        return int(lit[0]) if lit.size else int(a.size)

    bars = [lead(rows), lead(rows[::-1]), lead(cols), lead(cols[::-1])]
    top, bottom, left, right = (b if b >= min_bar else 0 for b in bars)
    if not (top or bottom or left or right):
        return None
    h, w = rows.size - top - bottom, cols.size - left - right
    if h < MIN_SIZE or w < MIN_SIZE:
        return None
    return top, left, h, w


def sample_indices(T: int, n: Optional[int]) -> list:
    """min(n, T) frame indices spread evenly over a clip of T frames, the middle of each of as many equal parts (None: every frame)."""
    n = T if n is None else min(int(n), T)
    return [((2 * k + 1) * T) // (2 * n) for k in range(n)]


def active_area(frames, device, frames_max: Optional[int] = 64):
    """The extent maxima of a clip (anything `frames_of` accepts, or its result): (rowmax int64 [H], colmax int64 [W]) as numpy arrays,
    the input of `find_bars`, from one streaming pass on `device` over at most `frames_max` frames spread evenly over the clip (None:
    every frame).  The pass is `detector.clip_batches` on that subset, DETECT_BATCH frames at a time, so a y4m or deep clip goes
    through its usual conversion, with one `ops.frame_extent` launch per batch joining the maxima: the sampled frames are uploaded once
    more than a run that does not ask for the area."""
    fr = frames if isinstance(frames, Frames) else frames_of(frames)
    if frames_max is not None and (isinstance(frames_max, bool) or not isinstance(frames_max, (int, np.integer)) or frames_max < 1):
        raise ValueError(f"active_area: frames_max must be None or a whole number >= 1, got {frames_max!r}")
    sub = fr.sample(sample_indices(fr.T, frames_max))
    dev, ext = torch.device(device), None
    with torch.no_grad(), torch.cuda.device(dev):
        for _, batch in detector.clip_batches(sub, dev, DETECT_BATCH):
            ext = ops.frame_extent(batch, None if fr.depth == 8 else fr.depth, out=ext)
    return ext[0].cpu().numpy().astype(np.int64), ext[1].cpu().numpy().astype(np.int64)


def roi_of(roi, H: int, W: int):
    """Validate a region of interest for H x W frames: None, "auto", "matte", or (y0, x0, h, w), four whole numbers (no bools) with
    0 <= y0, y0 + h <= H, the same for x, and h, w >= 20.  Returns None, "auto", "matte", the tuple of ints, or None for the rectangle that is
    the whole frame (the path without a region).  Raises ValueError with the reason."""
    if roi is None or (isinstance(roi, str) and roi in ("auto", "matte")):
        return roi
    vals = tuple(roi) if isinstance(roi, (tuple, list)) else ()
    if len(vals) != 4 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in vals):
        raise ValueError(f"roi must be None, \"auto\" or four whole numbers (y0, x0, h, w), or \"matte\" beside matte=, got {roi!r}")
    y0, x0, h, w = (int(v) for v in vals)
    if h < MIN_SIZE or w < MIN_SIZE:
        raise ValueError(f"roi {(y0, x0, h, w)}: the rectangle must be at least {MIN_SIZE}x{MIN_SIZE}, the smallest frame the clip API takes")
    if y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
        raise ValueError(f"roi {(y0, x0, h, w)}: the rectangle lies outside the {W}x{H} frame (0 <= y0, y0 + h <= {H}, 0 <= x0, x0 + w <= {W})")
    return None if (y0, x0, h, w) == (0, 0, H, W) else (y0, x0, h, w)


def check_roi_feather(roi_feather: int, h: int, w: int, tail) -> None:
    """Refuse a `roi_feather` above the bound for an h x w rectangle; `tail(bound)` is what the ValueError says after "roi_feather=N "."""
    bound = min(ROI_FEATHER_MAX, h // 2, w // 2)
    if roi_feather > bound:
        raise ValueError(f"roi_feather={roi_feather} " + tail(bound))


SHARP = ("deblur", "keep")       # what becomes of a frame labelled sharp: a window of its own like any other, or the input frame


def check_fields(fields):
    """How a frame is read: None, progressive; "split", as two woven fields that are deblurred as clips of their own."""
    if fields is not None and not (isinstance(fields, str) and fields == "split"):
        raise ValueError(f"fields must be None or \"split\", got {fields!r}")
    return fields


def check_sharp(sharp) -> str:
    if not isinstance(sharp, str) or sharp not in SHARP:
        raise ValueError(f"sharp must be \"deblur\" or \"keep\", got {sharp!r}")
    return sharp


def _lanes(model, device, n: int) -> list:
    """The launch streams of the windows, one set per model and device: `forward_window` captures one graph per launch stream, so
    fresh streams per clip would capture fresh graphs per clip."""
    return engine.model_streams(model, ("video_lanes", device.index, n), device, n)


class _WholePlan:
    """The plan source of a clip whose length is known: `labels`, `cuts` and `plan` of the whole clip, `has(k)`: it has a frame k."""

    def __init__(self, run: "ClipRun", labels, cuts):
        self.run, self._labels, self._cuts, self._plan, self.assumed = run, labels, cuts, None, []

    def _known(self, name: str):
        if getattr(self, name) is None:
            self._analyse()
        return getattr(self, name)

    labels = property(lambda self: self._known("_labels"))
    cuts = property(lambda self: self._known("_cuts"))

    @property
    def plan(self) -> list:
        if self._plan is None:
            self._plan = window_plan(self.labels, numbers=self.run.numbers, cuts=self.cuts)
        return self._plan

    def _analyse(self) -> None:
        """Whatever is missing of the LD detector's labels and the scene cuts, in ONE pass over the clip, DETECT_BATCH frames at a time:
        upload, then gray planes (spei_frames_u8_in / spei_frames_u16_in) and focus measures, pair statistics (spei_frame_pair_stats /
        spei_frame_pair_stats_u16), or both.  A deep clip stays deep throughout.  With a region of interest the pass is handed the
        clip's view through it, so the detector and the pair statistics see the cropped frames.  Under matte="auto" the pass also
        measures the blur cells (one more launch per batch), when it sees the full frames and nobody has measured them yet."""
        run, p, fr = self.run, self.run.detector, self.run._view()
        am = run.matte if isinstance(run.matte, blurmap.AutoMattes) and fr is run.frames and not run.matte.fed else None
        feats, stats = detector.clip_pass(fr, run.device, p.kernel_size, DETECT_BATCH, features=self._labels is None,
                                          pair_stats=self._cuts is None, **({} if am is None else dict(blur=am.params, cells=am.feed)))
        if feats is not None:
            self._labels = detector.predict(feats, p)
        if stats is not None:
            self._cuts = find_cuts(*_host_stats(stats, fr.depth), fr.H * fr.W, **run.cut_params)

    def has(self, k: int, home) -> bool:
        return k < len(self.plan)

    def label(self, k: int) -> int:
        return int(self.labels[k])


class _ArrivingPlan:
    """The plan source of a stream (`run.frames` is a `clip.StreamFrames`): a `StreamPlan` fed by the analysis of the frames as they
    arrive; `labels`, `cuts` and `plan` hold what is known so far, `assumed` the frames planned under `StreamPlan`'s assumption."""

    def __init__(self, run: "ClipRun", labels, cuts, horizon: int):
        self.run, self.view = run, run._view()
        self.sp = sp = StreamPlan(horizon, cuts="auto" if cuts is None else (cuts or None), labels=labels,
                                  pixels=self.view.H * self.view.W, cut_params=run.cut_params)
        # what is held at once: the look-ahead of the plan, the analysis batch in front of it and the windows behind (`ClipRun._run`)
        run.frames.reserve(sp.horizon + 2 * DETECT_BATCH + PREFETCH + 4 + (run.cut_params.get("window", 2) - 2 if cuts is None else 0))
        # matte="auto": the blur cells are measured on the full frames, in the analysis pass when that sees them (also when labels
        # and cuts were given: the pass then measures the cells alone), in a pass of its own beside it otherwise (a fixed roi), which
        # reads the same frames of the ring in the same batches
        am = self.am = run.matte if isinstance(run.matte, blurmap.AutoMattes) else None
        shared = am is not None and self.view is run.frames
        self.analysis = None if labels is not None and cuts is not None and not shared else detector.clip_analysis(
            self.view, run.device, run.detector.kernel_size, DETECT_BATCH, features=labels is None, pair_stats=cuts is None,
            **(dict(blur=am.params) if shared else {}))
        self.cells = None if am is None or shared else detector.clip_analysis(
            run.frames, run.device, run.detector.kernel_size, DETECT_BATCH, features=False, pair_stats=False, blur=am.params)

    labels = property(lambda self: np.asarray(self.sp.labels, dtype=np.int64))
    cuts = property(lambda self: self.sp.cuts)
    plan = property(lambda self: self.sp.plan)
    assumed = property(lambda self: self.sp.assumed)

    def label(self, k: int) -> int:
        """The label of a frame whose entry is planned (its batch has been fed)."""
        return self.sp.labels[k]

    def _pump(self) -> None:
        """One DETECT_BATCH of the stream into the plan, as soon as its frames have arrived: the batch `_WholePlan._analyse` would run."""
        sp, analysis = self.sp, self.analysis
        own = None if self.cells is None else next(self.cells, None)
        if own is not None:
            self.am.feed(own[0], own[3])
        if analysis is not None:
            item = next(analysis, None)
            if item is not None and len(item) > 3:         # the batch's blur cells: they exist before its entries are planned
                self.am.feed(item[0], item[3])
            n = 0 if item is None else len(item[3] if len(item) > 3 else item[1] if item[1] is not None else item[2][1])
        elif self.cells is not None:
            n = 0 if own is None else len(own[3])
        else:
            n = self.view.upto(sp.fed + DETECT_BATCH) - sp.fed
        if n <= 0:
            if sp.fed < 2:
                raise ValueError(f"a clip needs at least 2 frames (its 3-frame windows reflect at the ends); got {sp.fed}")
            sp.finish()
        elif analysis is None:
            sp.feed(count=n)
        else:
            feats, stats = item[1], item[2]
            sad, hist = (None, None) if stats is None else _host_stats(stats, self.view.depth)
            sp.feed(None if feats is None else detector.predict(feats, self.run.detector), sad, hist, count=n)

    def has(self, k: int, home) -> bool:
        """Whether the clip has a frame k: analyses the stream (on the stream `home`) until entry k is planned (or the stream has
        ended), and on until the plan is PREFETCH entries ahead while that takes no waiting.  Frames that neither a later window (its
        references lie at most 7 behind its last frame) nor the analysis will ask for are given up."""
        sp, plan, fr = self.sp, self.sp.plan, self.run.frames
        fr.release(max(0, min(sp.fed, k - 8)))
        while not sp.ended and (len(plan) <= k or (len(plan) <= k + PREFETCH and fr.ready(sp.fed + DETECT_BATCH) == sp.fed + DETECT_BATCH)):
            with torch.no_grad(), torch.cuda.device(self.run.device), torch.cuda.stream(home):
                self._pump()
        return k < len(plan)


class ClipRun:
    """Iterator of (index, [H,W,3] device tensor) in frame order, uint8 for `out_depth` 8 and uint16 for 10 and 12; see `deblur_clip`.
    `depth` is the clip's sample depth (8, 10 or 12), `out_depth` that of the frames handed out.  `labels` (0/1 per frame; computed on first
    access when the caller gave none), `cuts` (the scene cuts in use; found on first access when the caller asked for "auto", in the
    labelling pass when that runs too) and `plan` (`window_plan(labels, numbers=numbers, cuts=cuts)`) describe what runs; `recomputed` lists the
    frames that were recomputed in bf16x3 because their 16-bit pass left a non-finite value; `seconds[k]` is window k's host time
    [assembling its input, enqueueing it] (the wait for a free launch slot excluded).  `tiles` is the `tiles.TilePlan` of a clip that is
    deblurred tile by tile, None for one that is deblurred whole (a plan of one tile included).  `ensemble` is the number of members of
    the geometric self-ensemble every window runs as (1: none).  `roi` is the region of interest in use, (y0, x0, h, w), or None for a
    clip that is deblurred whole (found on first access, by `active_area` + `find_bars`, when the caller asked for "auto"); labels,
    cuts and the plan are then those of the clip of cropped frames.  In stream mode (`horizon` set: the clip is a `clip.StreamFrames`)
    `labels`, `cuts` and `plan` hold what is known so far and are complete after the last frame, and `assumed` lists the frames whose
    plan entry `StreamPlan` handed out under its assumption (empty in whole-clip mode).  `sharp` is "deblur" or "keep"; with "keep"
    no window runs for a frame whose label is 1: it is handed out as the input frame at `out_depth` (`ops.frame_requant`), `kept` is
    the increasing list of those handed out so far, none of them is ever in `recomputed`, and `assumed` leaves them out (a kept frame's
    plan entry is not used; `plan` itself is the same list either way).  `fields` is None or "split"; with "split" every frame is
    deblurred as its two fields (rows p::2), each parity a clip of its own, and `labels`, `cuts` and `plan` are the top-field clip's:
    one plan for both parities.  `matte` is the clip's `clip.Mattes` or None; with one, every frame handed out is the blend of the
    input frame with the deblurred one that its matte says (`ops.frame_matte`), a frame whose matte is empty runs no window and is
    handed out as the input frame at `out_depth`, `unmatted` is the increasing list of those handed out so far, none of them is ever
    in `recomputed`, and `assumed` leaves them out.  `roi` may also be the mattes' bounding box (`roi="matte"`).  Under `matte="auto"`
    `matte` is a `blurmap.AutoMattes`, which measures the mattes on the device and whose `cells` holds the verdict maps on the host.
    `handed_matte` is the device matte [H,W] (as given, before `matte_invert`) that the frame handed out last was blended with, or None
    where it left as its input."""

    def __init__(self, model, frames: Frames, labels, out, numbers=None, detector_params=None, cuts=None, cut_params=None,
                 out_depth: Optional[int] = None, tiles: Optional[tiling.TilePlan] = None, ensemble: int = 1, roi=None,
                 roi_feather: int = 0, bar_params: Optional[dict] = None, horizon: Optional[int] = None, sharp: str = "deblur",
                 fields: Optional[str] = None, matte: Optional[Mattes] = None):
        self.fields = check_fields(fields)
        if self.fields is not None:
            if tiles is not None or roi is not None:
                raise ValueError("fields= with tiles= or roi=: a window's table of parts is taken")
            frames = frames.woven()          # a y4m clip's frames become RGB field by field
        self.model, self.frames = model, frames
        self.sharp = check_sharp(sharp)
        self.kept = []                   # sharp="keep": the frames handed out as their input, in order
        self.matte = matte               # the clip's mattes (`clip.Mattes`, or `blurmap.AutoMattes` under matte="auto"), or None
        if isinstance(matte, blurmap.AutoMattes):
            matte.bind(self)             # it measures this run's frames, and its plan entries name the windows it holds over
        self.handed_matte = None         # the matte (device uint8 [H,W], as given: before `matte_invert`) that the frame handed out last was blended with; None: none was
        self.unmatted = []               # matte=: the frames whose matte is empty, handed out as their input, in order
        self._roi = roi                  # None, a rectangle, or "auto" while the scan has not run
        self.roi_feather = roi_feather
        self.bar_params = dict(bar_params or {})
        self.ensemble = ens.check_size(ensemble)
        self.tiles = tiles               # the tile plan of a clip that is deblurred tile by tile (more than one tile), or None
        self.depth = frames.depth
        self.out_depth = frames.depth if out_depth is None else out_depth
        self.detector = detector.DEFAULT if detector_params is None else detector_params
        params = list(model.parameters())
        self.device = params[0].device if params else torch.device("cpu")
        if self.device.type != "cuda":
            raise RuntimeError("speinet_amd runs on MI355X only (HIP kernels): move the model to a ROCm device first")
        self.cut_params = dict(cut_params or {})
        if out is not None and out.device != self.device:
            raise ValueError(f"out is on {out.device}, the model on {self.device}")
        self.out = out
        self.recomputed = []         # frames whose 16-bit pass left a non-finite value and that were recomputed in bf16x3
        self.seconds = []
        self.numbers = numbers
        self._it = None
        self.horizon = horizon       # None: the whole clip is known; a number: stream mode, with that look-ahead
        # labels, cuts (a list, or None for "auto") and the plan: known whole, or as the stream goes
        self._source = _WholePlan(self, labels, cuts) if horizon is None else _ArrivingPlan(self, labels, cuts, horizon)

    @property
    def roi(self):
        if isinstance(self._roi, str) and self._roi == "matte":     # the mattes' bounding box, grown and clamped; all empty: the path without
            found = self.matte.bbox()
            self._roi = None if found is None else roi_of(found, self.frames.H, self.frames.W)
            if self._roi is not None:
                check_roi_feather(self.roi_feather, *self._roi[2:], lambda _: f"does not fit the rectangle {self._roi} that "
                                  f"roi=\"matte\" found: at most min({ROI_FEATHER_MAX}, h // 2, w // 2)")
        if isinstance(self._roi, str):   # "auto": the bar rule on the extent maxima of the sampled frames; no bars: the path without
            fr, bp = self.frames, self.bar_params
            ext = active_area(fr, self.device, bp.get("frames", 64))
            found = find_bars(*ext, fr.depth, **{k: v for k, v in bp.items() if k != "frames"})
            self._roi = None if found is None else roi_of(found, fr.H, fr.W)
            if self._roi is not None:
                check_roi_feather(self.roi_feather, *self._roi[2:], lambda _: f"does not fit the rectangle {self._roi} that "
                                  f"roi=\"auto\" found: at most min({ROI_FEATHER_MAX}, h // 2, w // 2)")
        return self._roi

    def _view(self) -> Frames:
        """The clip the analysis pass sees: the frames cropped to the region of interest; of an interlaced clip, the top-field clip."""
        if self.fields is not None:
            return self.frames.field(0)
        return self.frames if self.roi is None else self.frames.view(self.roi)

    labels = property(lambda self: self._source.labels)
    cuts = property(lambda self: self._source.cuts)
    plan = property(lambda self: self._source.plan)

    @property
    def assumed(self) -> list:
        a = self._source.assumed
        if self.sharp == "keep":
            a = [i for i in a if self._source.label(i) != 1]
        return a if self.matte is None else [i for i in a if not self.matte.empty(i)]

    def __iter__(self):
        return self

    def __next__(self):
        if self._it is None:
            self._it = self._run()
        return next(self._it)

    def _run(self):
        m, dev, fr = self.model, self.device, self.frames
        H, W = fr.H, fr.W
        tp = self.tiles
        split = self.fields is not None                # the two fields of a frame: two parts of one shape, as two tiles are
        nt = 2 if split else 1 if tp is None else tp.n     # parts per frame: each is a window of its own, all of one shape
        Hp, Wp = (padded_size(H // 2 if split else H), padded_size(W)) if tp is None else tp.padded
        # a region of interest: the model sees the rectangle only, the cache keeps whole frames (the paste needs them)
        roi, roi_feather = self.roi, self.roi_feather
        if roi is not None:
            Hp, Wp = padded_size(roi[2]), padded_size(roi[3])
        centres = {}                     # per window in flight: its centre input frame, whole, for the paste (and a recompute's)
        src = self._source
        plan = src.plan                  # the whole clip's; a stream's grows as `src.has` analyses it
        n = m.n_sequence
        pool = ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 4), thread_name_prefix="speinet-video")
        # frames (uint8, or uint16 for a deep clip), decoded and uploaded once each; a y4m clip's as planar bytes, made RGB on the device
        cache = FrameCache(pool, fr.host, dev, convert=None if fr.yuv is None else (lambda planar: fr.rgb(planar)[0]))
        # mattes, one byte per pixel, through a cache of their own (a static matte is uploaded once: its one key stays)
        mt = self.matte
        mcache = None if mt is None else FrameCache(pool, mt.host, dev)
        mats = {}                        # per window in flight: its frame's matte on the device, for the blend (and a recompute's)
        K = self.ensemble
        members = ens.MEMBERS[K]         # every window runs once per member (and tile): K - 1 transformed copies of its input
        enc = EncoderCache(EncoderCache().capacity * nt * K)
        inflight, ready = collections.deque(), collections.deque()
        # the stream current at the first `next` assembles the inputs; the windows run on the lanes; a frame handed out is ordered
        # before later work on whatever stream is current at that `next`
        home = torch.cuda.current_stream(dev)
        lanes = _lanes(m, dev, LANES)
        # per window: the egress kernel's non-finite flag, copied to page-locked memory behind the window (read once the window is done)
        flags = torch.zeros(FLAG_RING, dtype=torch.int32, device=dev)
        flags_host = torch.zeros(FLAG_RING, dtype=torch.int32, pin_memory=True)
        # ingest and egress by depth: a deep clip is read as uint16, and the frame is quantised once, to out_depth
        depth, out_depth = self.depth, self.out_depth
        out_dtype = torch.uint8 if out_depth == 8 else torch.uint16

        def ingest(f, x, j):
            """Frame f as frame j of the window's input: of its one sample, or of every tile's or both fields' in one launch."""
            if split:
                return ops.fields_in(f, x[:, j], None if depth == 8 else depth)
            if tp is not None:
                return ops.tiles_in(f, tp, x[:, j], None if depth == 8 else depth)
            if roi is not None:          # the tile ingest with a table of one tile: bit-identical to the frame ingest on the crop
                return ops.roi_in(f, roi, x[0, j], None if depth == 8 else depth)
            return ops.frames_u8_in(f, out=x[0, j]) if depth == 8 else ops.frames_u16_in(f, depth, out=x[0, j])

        def egress(y, dst, flag, k):
            """The model's output, a list of nt planes [3, Hp, Wp], as frame k: the crop, the tiles' bands stitched, the two fields
            woven, or the rectangle pasted into the input frame."""
            if split:
                return ops.fields_out(y, H, W, out_depth, out=dst, nonfinite=flag)
            if tp is not None:
                return ops.tiles_out(y, tp, out_depth, out=dst, nonfinite=flag)
            if roi is not None:
                return ops.roi_paste(y[0], centres[k], roi, out_depth, roi_feather, None if depth == 8 else depth, out=dst,
                                     nonfinite=flag)
            if out_depth == 8:
                return ops.frame_u8_out(y[0], H, W, out=dst, nonfinite=flag)
            return ops.frame_u16_out(y[0], H, W, out_depth, out=dst, nonfinite=flag)

        def parts(run):
            """The nt planes of a window.  It runs as nt * K parts, one after the other: `run(t, g)` is the output plane of member g of
            tile (or field) t on the input xs[g][t:t + 1]; one launch turns the K planes of a tile back and averages them (K = 1: none)."""
            mean = (lambda outs: outs[0]) if K == 1 else (lambda outs: ops.d4_mean(outs, members))
            return [mean([run(t, g) for g in members]) for t in range(nt)]

        def frame(i):
            return fr.device(i).to(dev).contiguous() if fr.on_device(i) else cache.get_dev(i)

        keep = self.sharp == "keep"

        def unmatted(k):
            """Is the matte of frame k empty?  A stream that has a frame k and no matte for it ends here."""
            if mt is None:
                return False
            if not mt.static and k >= mt.T:
                raise ValueError(f"frame {k} has no matte: the stream outruns its matte of {mt.T} frames")
            return mt.empty(k)

        def kept(k):
            """Is frame k (planned already, so labelled) handed out as its input, with no window of its own: labelled sharp under
            sharp="keep", or with an empty matte?"""
            return (keep and src.label(k) == 1) or unmatted(k)

        def matte(k):
            return mt.device(k) if mt.on_device(k) else mcache.get_dev(mt.key(k))

        def blend(k, dst):
            """The deblurred frame where the matte says, the input elsewhere: one launch on the packed frame, in place, behind
            whichever egress wrote it."""
            ops.frame_matte(centres[k], dst, mats[k], out_depth, None if depth == 8 else depth, mt.invert, out=dst)

        def request(k):
            """The frames that steps k .. k + PREFETCH will ask the cache for: a window's keys; a kept frame itself, which no running
            window need hold (the middle of a run of sharp frames)."""
            ahead = range(k, min(k + 1 + PREFETCH, len(plan)))
            if mt is not None and not mt.static:           # decoded on the worker threads, in front of the `empty` that `kept` asks for
                mt.prefetch(pool, [j for j in ahead if j < mt.T])
            for j in ahead:
                keys = [j] if kept(j) else plan[j]["keys"]
                cache.request([i for i in keys if i is not ZERO and not fr.on_device(i)])
                if mt is not None and not kept(j) and not mt.on_device(j):
                    mcache.request([mt.key(j)])

        def stage(k):
            """What step k needs one step ahead: window k's input, or None (and the frame's `seconds` entry) for a kept frame."""
            if not kept(k):
                return prepare(k)
            self.seconds.append([0.0, 0.0])
            return None

        def keep_frame(k):
            """Frame k as its input at the output depth: one launch on the home stream, queued for the hand-out behind the windows
            before it.  It takes no lane, no launch slot and no flag slot."""
            t0 = time.time()
            request(k)
            f = frame(k)
            t1 = time.time()
            dst = self.out[k] if self.out is not None else torch.empty(H, W, 3, dtype=out_dtype, device=dev)
            ops.frame_requant(f, out_depth, None if depth == 8 else depth, out=dst)
            ev = torch.cuda.Event()
            ev.record()
            ready.append((k, dst, ev, None))
            self.seconds[k] = [t1 - t0, time.time() - t1]

        def prepare(k):
            """Window k's input [nt, n + 2, 3, Hp, Wp] on the home stream (nt = 1 without tiles): one per ensemble member."""
            t0 = time.time()
            request(k)
            x = torch.empty(nt, n + 2, 3, Hp, Wp, device=dev)
            for j, key in enumerate(plan[k]["keys"]):
                if key is ZERO:
                    x[:, j].zero_()
                else:
                    ingest(frame(key), x, j)
            if roi is not None or mt is not None:
                centres[k] = frame(plan[k]["window"][n // 2])     # uploaded just now: the frame that window k deblurs
            if mt is not None:
                mats[k] = matte(k)
            xs = [x] + [ops.planes_d4(x, g) for g in members[1:]]     # T_g of all its planes, one launch each (a zeroed frame stays zero)
            self.seconds.append([time.time() - t0, 0.0])
            return xs

        def enqueue(k, xs, nxts):
            """Window k on its lane (and window k + 1's encoder passes on the model's prefetch stream; `nxts` is None where frame k + 1
            is kept: the next window that runs then computes the encoder passes it misses itself, the same values)."""
            if len(inflight) >= max(2, len(lanes)):
                inflight.popleft().synchronize()           # the host stays at most two windows ahead of the GPU
            t0 = time.time()
            w = plan[k]
            dst = self.out[k] if self.out is not None else torch.empty(H, W, 3, dtype=out_dtype, device=dev)
            lane = lanes[k % len(lanes)]
            lane.wait_stream(home)                         # the window's input was assembled on the home stream
            slot = k % FLAG_RING

            def part(t, g):
                """Part (t, g) of window k behind the encoder passes of that part of window k + 1.  The keys: equal pixels per (member, tile,
                frame).  `forward_window` hands out a copy of its graph's static output, so the plane outlives the next part's replay."""
                if nxts is not None:
                    m.prefetch_window(nxts[g][t:t + 1], [(g, t, key) for key in plan[k + 1]["keys"]], enc, zero_ref=plan[k + 1]["zero_pre"])
                return m.forward_window(xs[g][t:t + 1], [(g, t, key) for key in w["keys"]], enc, zero_ref=w["zero_pre"])[0]

            with torch.cuda.stream(lane):
                for v in xs + (nxts or []):
                    v.record_stream(lane)
                dst.record_stream(lane)
                y = parts(part)
                if k in centres:
                    centres[k].record_stream(lane)
                egress(y, dst, flags[slot:slot + 1], k)
                if mt is not None:
                    mats[k].record_stream(lane)
                    blend(k, dst)
                flags_host[slot:slot + 1].copy_(flags[slot:slot + 1], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
            inflight.append(ev)
            ready.append((k, dst, ev, xs))
            self.seconds[k][1] = time.time() - t0

        def redo(k, xs, dst):
            """Window k again in split-bf16 arithmetic (fp32 exponent range), eagerly, on the home stream: a 16-bit pass left a NaN or an
            infinity in the frame (half operands do not saturate; one in any ensemble member reaches the mean, and so the flag).  Every
            member of every tile runs again."""
            keep = (m.precision, m.corr_precision, m.use_graph)
            m.precision, m.corr_precision, m.use_graph = "bf16x3", "bf16x3", False
            try:
                y = parts(lambda t, g: m(xs[g][t:t + 1], routing=[plan[k]["zero_pre"]])[0])
            finally:
                m.precision, m.corr_precision, m.use_graph = keep
            slot = k % FLAG_RING
            egress(y, dst, flags[slot:slot + 1], k)          # a region of interest: the same paste
            if mt is not None:
                blend(k, dst)                                # and the same blend behind it
            if int(flags[slot].item()):
                raise FloatingPointError(f"non-finite values in deblurred frame {k} in bf16x3 arithmetic as well: the input or the "
                                         "checkpoint is at fault")
            self.recomputed.append(k)
            warnings.warn(f"speinet_amd.video: frame {k} had a non-finite value in {keep[0]} arithmetic and was recomputed in bf16x3",
                          RuntimeWarning, stacklevel=3)

        def due():
            """Is the frame at the head of `ready` handed out now?"""
            return bool(ready) and (ready[0][3] is None or sum(r[3] is not None for r in ready) > LAG or len(ready) > READY_MAX)

        def hand_out():
            k, t, e, x = ready.popleft()
            cur = torch.cuda.current_stream(dev)
            if mt is not None:
                self.handed_matte = None if x is None else mats.get(k)
            if x is None:                                  # a kept frame: no window ran, so there is no flag to read
                cur.wait_event(e)
                if keep and src.label(k) == 1:
                    self.kept.append(k)
                if unmatted(k):
                    self.unmatted.append(k)
                if cur != home:
                    t.record_stream(cur)
                return k, t
            e.synchronize()                                # done already: the limiter in `enqueue` waited for it (not so while draining,
                                                           # nor for a window that READY_MAX sends out with kept frames behind it)
            if int(flags_host[k % FLAG_RING]):
                with torch.cuda.stream(home):
                    home.wait_event(e)
                    redo(k, x, t)
                cur.wait_stream(home)
            else:
                cur.wait_event(e)
            centres.pop(k, None)
            mats.pop(k, None)
            if cur != home:
                t.record_stream(cur)
            return k, t

        # grad mode and the current device are set around each step, not across a `yield`: they are the caller's while it holds a frame
        try:
            more = src.has(0, home)
            with torch.no_grad(), torch.cuda.device(dev), torch.cuda.stream(home):
                nxt = stage(0)
            k = -1
            while more:
                k += 1
                more = src.has(k + 1, home)
                with torch.no_grad(), torch.cuda.device(dev):
                    with torch.cuda.stream(home):
                        x = nxt
                        nxt = stage(k + 1) if more else None
                        if x is None:
                            keep_frame(k)
                        else:
                            enqueue(k, x, nxt)
                    # a window is handed out LAG windows behind: by then the limiter has waited for it, so its non-finite flag is on
                    # the host without a stall, and the windows after it keep running.  Kept frames do not pass the limiter, so they
                    # do not count towards LAG; a kept frame at the head has nothing to wait for and leaves at once, one behind a
                    # window waits its turn, so the order is the frames'.  READY_MAX bounds the queue: a window with fewer than LAG
                    # windows but that many frames behind it is handed out all the same, and `hand_out` then does wait for it
                    got = hand_out() if due() else None
                while got is not None:
                    yield got
                    with torch.no_grad(), torch.cuda.device(dev):
                        got = hand_out() if due() else None
            while ready:
                with torch.no_grad(), torch.cuda.device(dev):
                    got = hand_out()
                yield got
            if mt is not None and not mt.static and mt.T != len(plan):       # a stream: its length is known now
                raise ValueError(f"the matte holds {mt.T} mattes for a stream of {len(plan)} frames: a per-frame matte has one per frame")
        finally:
            pool.shutdown(wait=False, cancel_futures=True)
            if self.horizon is not None:
                fr.close()               # a stream: its reader thread ends


def deblur_clip(model, frames, labels=None, *, out: Optional[torch.Tensor] = None, crop: bool = False, numbers=None,
                detector=None, cuts=None, cut_params: Optional[dict] = None, yuv: Optional[dict] = None,
                depth: Optional[int] = None, out_depth: Optional[int] = None, tiles=None, shave: int = 20, feather: int = 0,
                ensemble: int = 1, roi=None, roi_feather: int = 0, bar_params: Optional[dict] = None, stream=False,
                horizon: int = 48, sharp: str = "deblur", fields: Optional[str] = None, matte=None,
                matte_invert: bool = False, matte_params: Optional[dict] = None) -> ClipRun:
    """Deblur a clip: an iterator of (index, [H,W,3] frame on the model's device), in frame order, one per input frame: uint8 frames,
    or uint16 frames when `out_depth` is 10 or 12.

    model  — an eval() `SPEINet` on a ROCm device; its `precision`, `corr_precision`, `use_graph` and `streams` are used as set.
    frames — T >= 2 frames of one size, at least 20x20: a uint8 [T,H,W,3] numpy array or torch tensor (host or device), a list of
             uint8 [H,W,3] arrays / tensors, a list of image paths (decoded to RGB on worker threads, a few windows ahead), or a
             y4m clip: a `y4m.Y4MReader`, or the path of a `.y4m` file (opened here).  A y4m frame is uploaded
             as its planar bytes (1.5 bytes per pixel for 4:2:0) and becomes packed RGB on the device (`ops.yuv_to_rgb_u8`).
             Deep clips: a 10- or 12-bit y4m stream (`C420p10` ... `C444p12`; a path, or a reader opened with
             `depths=(8, 10, 12)`; deep 4:2:0 has no siting tag, the reader's `layout` says LEFT unless the caller sets it), or uint16
             frames ([T,H,W,3], or a list of [H,W,3]) with `depth`.  A deep clip never passes through 8 bits.
             4:2:2 and mono clips (`C422*`, `Cmono*`): a path, or a reader opened with `layouts=y4m.LAYOUTS`; 2 and 1 samples per
             pixel cross PCIe.
    labels — optional 0/1 per frame (1 = sharp); None: the LD detector labels the clip in a first streaming pass.
    out    — optional contiguous [T,H,W,3] tensor on the model's device, uint8 for `out_depth` 8 and uint16 for 10 and 12: frame i is
             written to out[i] and that view is yielded.
    crop   — crop every frame at the bottom and right to multiples of 20 as it is loaded, as the reference's harness does, instead of
             padding it (H and W are then the cropped size).
    numbers — optional frame number per frame, in which the distance to a reference frame is measured (default: the indices).
    detector — optional `detector.DetectorParams` (a model fitted by `python -m speinet_amd.detector fit`) that labels the clip when
             `labels` is None; None: the reference's GoPro model (`detector.DEFAULT`).
    cuts   — scene cuts: None (the default) plans the clip as one continuous scene; a strictly increasing sequence of
             first-frame-of-scene indices in 1..T-1 is used as given; "auto" finds hard cuts with `scene_stats` and `find_cuts` (in
             the labelling pass when `labels` is None: the clip is uploaded once).  Every scene is planned as a clip of its own
             (`window_plan`), so no window and no reference frame crosses a cut.  `ClipRun.cuts` holds the list in use.
    cut_params — optional keyword arguments of `find_cuts` for "auto" (hist_min, ratio, min_delta, window: untuned defaults).
    yuv    — for a y4m clip, optional `dict(matrix="bt601" | "bt709", range="full" | "limited")` (either or both) in place of what
             the reader derived: y4m carries no matrix tag and often no range tag.

    depth  — 10 or 12: the bits per sample of uint16 frames (a word above 2^depth - 1 reads as that).  Required for uint16 input, an
             error for anything else.
    out_depth — 8, 10 or 12: the depth of the frames handed out, round_half_even(clamp(x * (2^out_depth - 1))) of the model's float
             output; None: the input's depth.  An 8-bit clip with `out_depth=10` is allowed and useful: the model's output carries
             more than 8 bits.

    tiles  — None (the default): every frame is deblurred whole.  (rows, cols), 1..8 each, or "auto": the frame is cut into a grid
             of overlapping tiles of one shape (`tiles.tile_plan`), every tile is deblurred as a clip of its own and the tiles' bands
             are stitched with hard seams, as the reference's `forward_chop` does for 2x2 (no blending unless `feather` is set).
             "auto" leaves a frame of at most 960000 pixels whole and otherwise takes the fewest tiles of at most that many.  A
             tile's result differs from the whole frame's there: its correlation and attention see the tile only.  Labels, scene
             cuts and the window plan are still those of the whole frames.  `ClipRun.tiles` holds the plan in use (None for one
             tile).
    shave  — 0..200: the margin in pixels a tile keeps around the band it owns (the reference's 20).
    feather — 0..shave, with `tiles` only: 0 (the default) stitches with hard seams.  N > 0 blends the two tiles of every inner seam
             linearly over the 2 N pixels around it (four tiles where a row and a column ramp cross), from the margins the tiles
             computed anyway; every pixel further than N from the seams is the hard stitch's, bit for bit.  A non-finite value
             anywhere a pixel is blended from sends the window to the bf16x3 recompute, as one in a band does.
    ensemble — 1 (the default), 2, 4 or 8: geometric self-ensemble over the members 0..K-1 of `speinet_amd.ensemble` (2: the frame and
             its mirror; 4: the four flips, one frame shape; 8: also the four transposed members, a second frame shape with its own
             captured graphs).  Every window runs once per member on the transformed padded input; the outputs are transformed back and
             averaged in float32 in member order (`ops.d4_mean`) in front of the egress, so it composes with `tiles`, `feather`,
             `out_depth` and y4m.  K forward passes per frame; labels, scene cuts and the window plan are those of the upright frames.
             A non-finite value in any member sends the window to the bf16x3 recompute, which runs all K members again.  1 is the
             path without it, launch for launch.  `ClipRun.ensemble` holds it.
    roi    — region of interest: None (the default) deblurs whole frames, launch for launch the path without it.  (y0, x0, h, w), four
             whole numbers with the rectangle inside the frame and h, w >= 20: only that rectangle is deblurred.  Inside it, frame i of
             the result is frame i of `deblur_clip` on the clip of cropped frames f[y0:y0+h, x0:x0+w] with every other argument the
             same, bit for bit (`roi_feather` 0): its reflect pad at the rectangle's bottom and right, the detector's labels of the
             cropped frames when `labels` is None, `cuts="auto"` on their pair statistics, their window plan.  Outside it, it is the
             input frame's sample at the output depth, (min(v, D_in) * 2 * D_out + D_in) // (2 * D_in) with D = 2^depth - 1 (exact,
             rounds half up, the identity at equal depths); for a y4m clip the input frame is the RGB frame made from it.  One launch
             per frame pastes the rectangle into the frame (`ops.roi_paste`); the rectangle is ingested by the tile ingest with a table
             of one tile (`ops.roi_in`).  A rectangle equal to the whole frame is the path without it.  "auto": the active picture area
             of letterboxed or pillarboxed footage, found by `active_area` (one more streaming pass over at most 64 sampled frames) and
             `find_bars`; no bars: the path without it.  Not with `tiles` (the tile egress writes whole frames only) and not with
             `crop`.  `ClipRun.roi` holds the rectangle in use, or None.
    roi_feather — 0..min(200, h // 2, w // 2), with `roi` only: 0 (the default) pastes with a hard edge.  N > 0 blends the deblurred
             rectangle with the input linearly over the N pixels inside every side of the rectangle that is not a side of the frame;
             every pixel off those ramps is the hard paste's, bit for bit.
    bar_params — optional keyword arguments of `find_bars` for "auto" (level, min_bar: untuned defaults), and `frames`: the number of
             frames `active_area` scans (default 64, None: every frame).

    stream — False (the default): the clip's length is known and it is planned whole.  True: `frames` is a `y4m.Y4MStream` (or the path
             of a `.y4m` file, then read in order) or an iterator of host frames, uint8 [H,W,3] or uint16 with `depth`; its length is
             not known, at least 2 frames must come.  Frames are handed out while the stream is still being read, after a bounded
             look-ahead; `labels` (for the whole stream; a stream longer or shorter is a ValueError when that is known), `cuts`
             (a list, "auto" or None), a fixed `roi`, `tiles`, `feather`, `ensemble`, `out_depth`, `yuv` and `depth` work as above.
             Not with `out`, `numbers` or `roi="auto"`, and not on an indexable clip (its whole-clip plan is exact) unless
             `stream="force"`.  `ClipRun.assumed` lists the frames that are not the whole-clip run's, see `StreamPlan`.
    horizon — with `stream`: the look-ahead in frames, at least 24, after which a plan entry is committed (`StreamPlan`).

    sharp  — "deblur" (the default): every frame runs its window, as the reference does; launch for launch the path without this
             argument.  "keep": a frame whose label is 1 (from `labels` or the detector; with `roi`, the cropped clip's label) is
             KEPT: no window runs for it, and it is handed out as the input frame at the output depth, every sample
             (min(v, D_in) * 2 * D_out + D_in) // (2 * D_in) with D = 2^depth - 1 (`ops.frame_requant`, one launch; the identity at
             equal depths; for a y4m clip the input frame is the RGB frame made from it).  That is the whole frame under `tiles`,
             `ensemble` and `roi` too: what the paste writes outside the rectangle, so a kept frame has no seam there.  Every frame
             that is not kept has the same plan entry and is bit-identical to the "deblur" run's: sharp frames still enter the
             neighbouring windows and serve as references, as inputs.  `ClipRun.kept` lists the kept frames handed out so far; none
             is ever flagged non-finite or in `recomputed`; in a stream none is in `assumed`.  With every frame kept the model is never
             called.  An extension beyond the reference.  No trained checkpoint exists here, so nothing is claimed about quality: in
             particular not that the step from a kept frame to its deblurred neighbours is invisible.

    fields — None (the default): the frames are progressive; launch for launch the path without this argument.  "split": the frames
             are INTERLACED.  A frame f of even height H is two fields, field p (0 = top, 1 = bottom) = f[p::2]: H / 2 rows, the same
             W and depth, two different instants.  Frame k of the result has, in its rows p::2, frame k of
             `deblur_clip(model, [f[p::2] for f in frames], labels=L, cuts=C, ...)` with every other argument the same, bit for bit,
             for p = 0 and 1.  L and C are the caller's `labels` / `cuts` when given; otherwise the labels and, with `cuts="auto"`,
             the cuts that the detector and `find_cuts` give the TOP-FIELD clip: one plan for both parities, and `ClipRun.labels`,
             `.cuts` and `.plan` are the top-field clip's.  The reflect pad to multiples of 20 is each field's own (field row
             H / 2 + j is field row H / 2 - 2 - j).  H must be even and H / 2 >= 20.  Design choices: each parity is its own clip, so a
             window has frame-rate spacing and no half-line bob between its frames (one clip of 2T alternating fields bobs: rejected);
             field order (top or bottom first) therefore does not enter the result, a y4m `It` and `Ib` clip differ in the tag only;
             mixed-mode `Im` streams stay refused.  A y4m clip is made RGB field by field (4:2:0: chroma-plane row j belongs to field
             j & 1, and H must be a multiple of 4; the other layouts convert row by row).  Composes with `cuts`, `ensemble`,
             `sharp="keep"` (a kept frame is the whole input frame), deep clips, `out_depth`, every y4m layout, `out` and `stream`
             (one plan stands behind both parts).  Not with `tiles` or `roi`: a window's table of parts is taken.  A y4m reader or
             stream whose `interlace` is "t" or "b" needs `fields="split"` said: there is no silent default.  An extension beyond the
             reference; no trained checkpoint exists here, so nothing is claimed about quality.

    matte  — None (the default): launch for launch the path without this argument.  Otherwise an 8-bit mask that says how much of the
             deblurred result every pixel gets.  Write a for the input frame's sample at the output depth (what `sharp="keep"` and
             the outside of `roi` hand out; for a y4m clip the input frame is the RGB frame made from it), b for the sample that the
             same call without `matte=` hands out there, and m for the pixel's matte byte (255 - m under `matte_invert`).  Every
             sample of the frame handed out is
                 (a * (255 - m) + b * m + 127) // 255
             in exact integers (at most 4095 * 255 + 127): m = 0 gives a, m = 255 gives b, a == b gives a for every m, and swapping
             a with b under the inverted matte gives the same value.  So a matte of 255 everywhere is the run without a matte, bit
             for bit, and a matte of 0 everywhere is the input.  The matte has the size of the frames as given and is cropped as
             they are under `crop`.  Static (one for the clip): a uint8 or bool [H,W] numpy array or torch tensor (host or device; a
             bool matte is 0 / 255), or the path of an image file, decoded to one 8-bit channel (PIL `convert("L")`).  Per frame
             (T of them: any other length is a ValueError): a [T,H,W] array or tensor; a list of [H,W] arrays or of image paths
             (decoded on the worker threads, prefetched as the frames are); a directory of images, in file-name order; an 8-bit
             `Cmono` y4m file or `y4m.Y4MReader`, whose luma bytes are the matte AS STORED: m = 255 needs full-range grey (a
             limited-range white is 235).  Mattes cross PCIe as 1 byte per pixel through a frame cache of their own.
             A frame whose matte (in effect: after `matte_invert`) is 0 everywhere runs NO window: it takes the kept-frame path
             (one `ops.frame_requant`, no lane, no flag slot), is never in `recomputed`, is left out of `assumed`, and is listed,
             in order, in `ClipRun.unmatted` (`ClipRun.kept` stays what it is).  Every other frame keeps its plan entry; unmatted
             frames still serve as neighbours and references, as inputs.  Emptiness is decided on the host for host mattes, and
             with one reduction and one sync at the start for a device-resident [T,H,W] tensor.
             The blend is one more launch on the packed frame (`ops.frame_matte`, in place) behind whichever egress ran, so it
             composes: with `sharp="keep"` a kept frame is the input and the blend is skipped; with `roi` / `roi_feather` the paste
             runs first, then the blend over the whole frame (outside the rectangle a == b); with `tiles` / `feather` it runs
             behind the stitch; with `fields="split"` on the woven frame; `ensemble`, `out_depth`, deep input, `cuts`, `out`,
             `crop` and every y4m layout are unchanged behind it.  A non-finite value anywhere in the egress's frame still sends the
             window to the bf16x3 recompute, wherever the matte is 0 (conservative, simple), and the blend runs again behind the
             recompute's egress.  With `stream=True` a static matte or an indexable per-frame matte is accepted (a stream that
             outruns its matte is a ValueError naming the frame; an iterator of mattes is not built).
             `roi="matte"`: the region of interest is the union bounding box of the non-zero matte samples of all frames, grown
             by 20 pixels on every side (the `shave` default, so the rectangle's reflect pad does not sit on the subject's edge),
             then symmetrically to at least 20x20, and clamped to the frame; `ClipRun.roi` holds it and everything `roi` says about
             labels, cuts and the plan applies.  It needs every matte up front (one pass over them before the first window), so it is
             refused with `stream=True` unless the matte is static.  An all-empty clip never calls the model.
             An extension beyond the reference; no trained checkpoint exists here, so nothing is claimed about quality.
             matte="auto" (the string; a file of that name is "./auto"): the mattes are MEASURED, one per frame, on the device: where
             is the picture blurred?  The frames as given (after `crop`) are cut into cells of 16x16 pixels; per cell and direction
             the re-blur measure says how much of the adjacent-pixel variation a 9-tap box removes (`ops.blur_cells`, one launch per
             analysis batch of 16 frames, in the labelling / cut pass when that sees the full frames; in one more pass over the clip,
             one more upload of a host clip, when that pass sees a region of interest or does not run because `labels` and `cuts`
             were given); a cell is lit where either direction has texture and a box removes little of it.  Frame k's cell map is the
             maximum of the verdict maps of the frames of plan entry k's window (`hold`: it never crosses a cut and needs no frame
             that a stream has not delivered by the time the window runs), dilated by `grow` cells, and its matte the bilinear
             interpolation between cell centres, exact integers (`ops.blur_matte`, one launch per matted frame): a ramp of 16 pixels
             between a lit and an unlit cell.  Everything behind the matte is what it is for a given one, and the result is that of
             `matte=M` with M the [T,H,W] mattes so made, bit for bit: the blend, `ClipRun.unmatted` for a frame whose cell map is
             empty (decided from the cell bytes on the host; no window runs), `sharp="keep"`, tiles, ensemble, deep clips, `out`,
             `crop`, cuts, every y4m layout, the bf16x3 recompute, `roi` as a rectangle, "auto" or "matte" (the rectangle around
             every lit cell of every frame's cell map, moved out by the 8 pixels the ramp reaches, then grown as above), and
             `stream=True` (an all-sharp stream never calls the model).  `ClipRun.matte` is then a `blurmap.AutoMattes`, whose
             `cells` holds the verdict maps [T,ch,cw] on the host.  Refused: with `fields=` (the rows of a frame are two instants,
             so the vertical measure is meaningless: not built), with `matte_invert=True`, and `roi="matte"` with `stream=True`.
             The definition in full, its four parameters (design parameters, not measurements: nobody has tuned them) and its
             blind spots (grain on top of a blurred region reads as sharp; a defocused background is "blurred"; a cell below
             `flat` is never lit): speinet_amd/blurmap.py.
    matte_invert — with `matte` only: the matte in effect is 255 - m.
    matte_params — with matte="auto" only: a dict over `MATTE_PARAMS`: thr (0..257, default 192), flat (0..255, default 2), grow
             (0..4, default 1), hold (0 or 1, default 1); an unknown key or a value out of range is a ValueError.

    The frames are validated here (ValueError with the reason); the GPU work starts with the first `next`.  A yielded frame is
    complete in the order of the stream that is current at that `next`: use it there, or synchronise first.  A window whose frame
    holds a NaN or an infinity (half operands do not saturate) is recomputed in bf16x3 arithmetic, as the harness does: its index goes
    to `ClipRun.recomputed` with a RuntimeWarning, and FloatingPointError is raised if the frame is still not finite."""
    ensemble = ens.check_size(ensemble)                    # in front of everything else: no frame is looked at
    sharp = check_sharp(sharp)
    fields = check_fields(fields)
    if matte is None and matte_invert:
        raise ValueError("matte_invert=True needs matte=: there is no matte to invert")
    auto = isinstance(matte, str) and matte == "auto"
    if matte_params is not None and not auto:
        raise ValueError("matte_params= needs matte=\"auto\": they are the parameters of the measured matte, a given one has none")
    if auto:
        if fields is not None:
            raise ValueError(f"matte=\"auto\" with fields={fields!r} is not built: the rows of an interlaced frame are two instants, so the "
                             "vertical blur measure is meaningless")
        if matte_invert:
            raise ValueError("matte=\"auto\" with matte_invert=True: the measured matte is lit where the picture is blurred, and deblurring "
                             "where it is sharp instead serves nothing")
        if stream and isinstance(roi, str) and roi == "matte":
            raise ValueError("roi=\"matte\" with stream=True and matte=\"auto\": the bounding box is found from the mattes of every frame "
                             "before the first window, and a stream's length is not known; give the rectangle (y0, x0, h, w)")
        blur_params = BlurParams.of(matte_params)
    if matte is None and isinstance(roi, str) and roi == "matte":
        raise ValueError("roi=\"matte\" needs matte=: the rectangle is the bounding box of the mattes")
    if fields is not None and (tiles is not None or roi is not None):
        raise ValueError(f"fields={fields!r} with {'tiles=' if tiles is not None else 'roi='} is not built: the fields of a frame run as the "
                         "two parts of its window, and the table of parts is taken by the tiles or the rectangle")
    if tiles is None and not (isinstance(feather, int) and not isinstance(feather, bool) and feather == 0):
        raise ValueError(f"feather={feather!r} needs tiles=: it blends the seams between tiles, and an untiled frame has none")
    if isinstance(roi_feather, bool) or not isinstance(roi_feather, (int, np.integer)) or roi_feather < 0:
        raise ValueError(f"roi_feather must be a whole number >= 0, got {roi_feather!r}")
    if roi is None and roi_feather != 0:
        raise ValueError(f"roi_feather={roi_feather!r} needs roi=: it blends the edge of the region of interest, and a whole frame has none")
    if roi is not None and tiles is not None:
        raise ValueError("roi= with tiles= is not built: the tile egress writes whole packed frames only, not a rectangle of one")
    if roi is not None and crop:
        raise ValueError("roi= with crop=True: the rectangle is given in the frames as they are, crop them first or leave crop off")
    if bar_params is not None and set(bar_params) - set(BAR_PARAMS):
        raise ValueError(f"bar_params holds {sorted(set(bar_params) - set(BAR_PARAMS))}: find_bars takes level and min_bar, and frames is "
                         "the number of frames that active_area scans")
    if stream not in (False, True, "force"):
        raise ValueError(f"stream must be False, True or \"force\", got {stream!r}")
    if isinstance(frames, (str, os.PathLike)) and os.fspath(frames).lower().endswith(".y4m"):
        frames = (y4m.Y4MStream if stream else y4m.Y4MReader)(frames, depths=y4m.DEPTHS, layouts=y4m.LAYOUTS, interlace=y4m.INTERLACE)
    if fields is None and getattr(frames, "interlace", "p") in ("t", "b") and isinstance(frames, (y4m.Y4MReader, y4m.Y4MStream)):
        raise ValueError(f"the y4m clip is interlaced (I{frames.interlace}): pass fields=\"split\" to deblur its two fields as clips of "
                         "their own, or open it as progressive on purpose; there is no silent default")
    unbounded = isinstance(frames, y4m.Y4MStream) or hasattr(frames, "__next__")
    if unbounded and not stream:
        raise ValueError("frames is a stream (a Y4MStream, or an iterator of frames): its length is not known, pass stream=True")
    if stream and not unbounded:
        if stream != "force":
            raise ValueError("stream=True on a clip whose length is known: the whole-clip plan is exact and costs no look-ahead; pass a "
                             "y4m.Y4MStream or an iterator of frames (stream=\"force\" streams an array or a list of host frames)")
        if isinstance(frames, y4m.Y4MReader) or isinstance(frames, (str, bytes)) or not hasattr(frames, "__iter__"):
            raise ValueError("stream=\"force\" takes an array or a list of host frames; open a y4m clip as a y4m.Y4MStream")
        frames = iter(frames)
    if stream:                                             # what needs the whole clip, or its length
        if out is not None:
            raise ValueError("out= with stream=True: the tensor holds every frame, and a stream's length is not known")
        if numbers is not None:
            raise ValueError("numbers= with stream=True: the incremental plan measures the reference gap in frame indices")
        if isinstance(roi, str) and roi == "auto":
            raise ValueError("roi=\"auto\" with stream=True: the active area is found from frames sampled over the whole clip; give "
                             "the rectangle (y0, x0, h, w)")
    # a stream's `fr.T` is None: what is measured against the clip's length is then checked by `StreamPlan` as the stream goes
    fr = frames_of(frames, crop, yuv, depth)
    mt = None if matte is None else blurmap.AutoMattes(blur_params, fr.H, fr.W) if auto else mattes_of(matte, fr.T, *fr.src, crop, matte_invert)
    if stream and mt is not None and not mt.static and isinstance(roi, str) and roi == "matte":
        raise ValueError("roi=\"matte\" with stream=True and a per-frame matte: the bounding box is found in one pass over every matte "
                         "before the first window, and a stream's length is not known; give the rectangle (y0, x0, h, w) or a static matte")
    if fields is not None:
        if fr.H % 2 or fr.H // 2 < MIN_SIZE:
            raise ValueError(f"fields={fields!r}: a {fr.W}x{fr.H} frame does not split into two fields of at least {MIN_SIZE} rows "
                             f"(H must be even and H / 2 >= {MIN_SIZE})")
        if fr.yuv is not None and fr.yuv[0] in (y4m.CENTER, y4m.LEFT) and fr.src[0] % 4:
            raise ValueError(f"fields={fields!r}: the fields of a 4:2:0 clip of H = {fr.src[0]} rows have no whole chroma rows (H must "
                             "be a multiple of 4)")
    if roi is not None and not isinstance(roi, str):
        roi = roi_of(tuple(roi) if isinstance(roi, list) else roi, fr.H, fr.W)
        h, w = (fr.H, fr.W) if roi is None else roi[2:]
        check_roi_feather(roi_feather, h, w, lambda bound: f"is outside 0..{bound}: at most {ROI_FEATHER_MAX} and half of the {w}x{h} rectangle")
    elif roi is not None:
        roi = roi_of(roi, fr.H, fr.W)    # "auto" or "matte", or a ValueError for any other string
        check_roi_feather(roi_feather, fr.H, fr.W, lambda bound: f"is outside 0..{bound}: at most {ROI_FEATHER_MAX} and half of the "
                          f"rectangle, which lies inside the {fr.W}x{fr.H} frame")
    if out_depth is not None and (isinstance(out_depth, bool) or out_depth not in y4m.DEPTHS):
        raise ValueError(f"out_depth must be None, 8, 10 or 12, got {out_depth!r}")
    out_depth = fr.depth if out_depth is None else int(out_depth)
    out_dtype = torch.uint8 if out_depth == 8 else torch.uint16
    lab = None if labels is None else labels_of(labels, fr.T)
    if numbers is not None and len(numbers) != fr.T:
        raise ValueError(f"numbers has {len(numbers)} entries for a clip of {fr.T} frames")
    shape = (fr.T, fr.H, fr.W, 3)
    if out is not None and not (torch.is_tensor(out) and out.dtype == out_dtype and tuple(out.shape) == shape and out.is_contiguous()):
        raise ValueError(f"out must be a contiguous {str(out_dtype).split('.')[-1]} [{fr.T},{fr.H},{fr.W},3] tensor "
                         f"(out_depth {out_depth})")
    if isinstance(cuts, str):
        if cuts != "auto":
            raise ValueError(f"cuts must be None, \"auto\" or a sequence of frame indices, got {cuts!r}")
        cuts = None
    elif cuts is None or fr.T is not None:
        cuts = cuts_of(cuts, fr.T)       # a stream's list: `StreamPlan` checks it, its upper bound at the stream's end
    if cut_params is not None and set(cut_params) - set(CUT_PARAMS):
        raise ValueError(f"cut_params holds {sorted(set(cut_params) - set(CUT_PARAMS))}: find_cuts takes hist_min, ratio, min_delta and window")
    tp = None if tiles is None else tiling.tile_plan(fr.H, fr.W, tuple(tiles) if isinstance(tiles, list) else tiles, shave, feather)
    if tp is not None and tp.n == 1:
        tp = None                        # one tile that spans the frame: the untiled path
    return ClipRun(model, fr, lab, out, numbers, detector, cuts, cut_params, out_depth, tp, ensemble, roi, int(roi_feather), bar_params,
                   horizon if stream else None, sharp, fields, mt)


def _inputs(spec: str) -> list:
    files = [os.path.join(spec, f) for f in os.listdir(spec)] if os.path.isdir(spec) else glob.glob(spec)
    return sorted(f for f in files if f.lower().endswith(IMAGE_EXTS) and os.path.isfile(f))


def parse_roi(text: str):
    """`--roi`: 'none' -> None, 'auto' -> "auto", 'matte' -> "matte", 'Y,X,H,W' -> (y0, x0, h, w).  Raises ValueError with the reason."""
    if text in ("none", "auto", "matte"):
        return None if text == "none" else text
    parts = text.split(",")
    if len(parts) != 4 or not all(p.strip().lstrip("+").isdigit() for p in parts):
        raise ValueError(f"{text!r} is not none, auto, matte or Y,X,H,W (four whole numbers: top, left, height, width)")
    return tuple(int(p) for p in parts)


def read_cuts(path: str) -> list:
    """Scene cuts from a file: a .npy array, or a text file of whitespace-separated first-frame-of-scene indices."""
    if path.lower().endswith(".npy"):
        return np.asarray(np.load(path)).reshape(-1).tolist()
    with open(path) as f:
        return [int(tok) for tok in f.read().split()]


def load_model(model_path: str, device, precision: str = "f16", graph: bool = True):
    """A SPEINet in eval() on `device` with the harness's arithmetic pairing for `precision` (`synthetic`: the seed-0 test weights)."""
    from . import checkpoint
    from .speinet import SPEINet, default_args
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    net = SPEINet(in_channels=3, n_sequence=3, out_channels=3, n_resblock=3, n_feat=32, device=str(device), args=default_args())
    if model_path == "synthetic":
        from .synth import state_dict_template, synth_state_dict
        net.load_state_dict(synth_state_dict(state_dict_template(), seed=0))
    else:
        checkpoint.load_into(net, model_path, strict=True)
    net = net.to(device).eval()
    net.precision, net.corr_precision = precision, CORR_PRECISION[precision]
    net.use_graph = graph
    net.streams = 1
    return net


def _fps(text: str):
    num, _, den = text.replace("/", ":").partition(":")
    return int(num), int(den or 1)


class _Numbered:
    """The frame names of a clip whose length is not known: 000000, 000001, ..."""

    def __init__(self, ext: str):
        self.ext = ext

    def __getitem__(self, i: int) -> str:
        return f"{i:06d}{self.ext}"


def _spool(stream, spool_dir: Optional[str]):
    """Copy a pipe to an unnamed temporary file (in `spool_dir`, default: the system's) and return that file."""
    import shutil
    import tempfile
    f = tempfile.TemporaryFile(dir=spool_dir)
    shutil.copyfileobj(stream, f, 1 << 22)
    f.flush()
    return f


def main(argv=None) -> None:
    """The command line.  `--input` is a directory or glob of image files, a `.y4m` file, or `-` for a y4m stream on stdin; `--output`
    a directory (one PNG per frame), a `.y4m` file, or `-` for a y4m stream on stdout (every log line then goes to stderr), so the
    tool sits between two ffmpeg processes:

        ffmpeg -i in.mp4 -pix_fmt yuv420p -f yuv4mpegpipe - | python -m speinet_amd.video --input - --output - --model_path ... \
            | ffmpeg -f yuv4mpegpipe -i - out.mp4

    By default a pipe on stdin is SPOOLED TO DISK first, to an unnamed temporary file (`--spool_dir`), all of it before the first
    frame is deblurred: the whole-clip window plan needs the clip's length and its labels before the first window.  With `--stream
    [--horizon N]` stdin (or a `.y4m` file) is read through `y4m.Y4MStream` as it arrives, with no spool: the first frames leave
    while the input is still coming, every output frame is flushed, cuts are reported as they are found, and the last log line
    says how many frames were planned under `StreamPlan`'s assumption.  The y4m output is written by one thread, in frame order."""
    p = argparse.ArgumentParser(description="Deblur a clip of any size (at least 20x20) on an MI355X: image files or a YUV4MPEG2 stream in, "
                                "one PNG per frame or a YUV4MPEG2 stream out")
    p.add_argument("--input", required=True, help="a directory of frames, or a glob (PNG / JPG / BMP); frames in file-name order; or a "
                   ".y4m file; or '-': a y4m stream on stdin (spooled to a temporary file first)")
    p.add_argument("--output", required=True, help="directory for the deblurred PNGs (input file name, .png; 000000.png ... for y4m "
                   "input); or a .y4m file; or '-': a y4m stream on stdout")
    p.add_argument("--labels", default=None, help="0/1 per frame (1 = sharp) as a .npy file; default: the LD detector labels the clip")
    p.add_argument("--detector", default=None, help="a detector JSON file of `python -m speinet_amd.detector fit` (default: the reference's "
                   "GoPro model)")
    p.add_argument("--cuts", default="none", help="scene cuts: 'none' (one continuous scene, the default), 'auto' (hard cuts found from "
                   "luma histograms and frame differences), or a .npy / text file of first-frame-of-scene indices")
    p.add_argument("--model_path", required=True, help="checkpoint in the reference layout, or 'synthetic' (seed-0 test weights)")
    p.add_argument("--precision", choices=sorted(CORR_PRECISION), default="f16",
                   help="arithmetic of the GEMM-shaped kernels (default f16 with the top2 correlation: the throughput configuration)")
    p.add_argument("--device", default="cuda")
    p.add_argument("--no_graph", dest="graph", action="store_false", default=True, help="launch kernels eagerly (no hipGraph replay)")
    p.add_argument("--matrix", choices=sorted(y4m.MATRIX_NAMES), default=None, help="YUV matrix of y4m input and output (default: bt709 "
                   "for 720 rows and more, bt601 below: y4m has no matrix tag)")
    p.add_argument("--range", choices=sorted(y4m.RANGE_NAMES), default=None, help="YUV range of y4m input and output (default: the "
                   "input's XCOLORRANGE tag, limited without one; full for image input)")
    p.add_argument("--fps", type=_fps, default=None, help="frame rate of y4m output as num:den (default: the y4m input's; 25:1 for image input)")
    p.add_argument("--chroma", choices=sorted(y4m.TAG_OF_LAYOUT.values()), default=None, help="chroma layout of y4m output from image "
                   "input (default 420jpeg; y4m input keeps its own, see --out_chroma); 420jpeg | 420mpeg2 also select the chroma "
                   "siting of a 10- or 12-bit 4:2:0 y4m input, whose tag carries none (default 420mpeg2: co-sited with the even column)")
    p.add_argument("--out_chroma", choices=sorted(y4m.TAG_OF_LAYOUT.values()), default=None, help="chroma layout of the y4m output whatever "
                   "the input was: 4:2:2 in and 420mpeg2 out for delivery, 4:2:0 in and 444 out to avoid a second subsampling (default: "
                   "the y4m input's layout, or --chroma for image input)")
    p.add_argument("--out_depth", type=int, choices=y4m.DEPTHS, default=None, help="bits per sample of the output (default: the "
                   "input's for y4m output; a PNG directory always gets 8-bit files)")
    p.add_argument("--tiles", default="none", help="deblur every frame as a grid of overlapping tiles, stitched with hard seams (or "
                   "blended ones: --feather): 'none' "
                   "(the default: whole frames), 'auto' (whole up to 960000 pixels, else the fewest tiles of at most that many) or RxC "
                   "(rows x columns, 1..8 each, such as 2x2: the reference's forward_chop)")
    p.add_argument("--shave", type=int, default=20, help="pixels of margin a tile keeps around the band it owns (default 20, 0..200)")
    p.add_argument("--feather", type=int, default=0, help="with --tiles: blend the two tiles of every seam over the 2 N pixels around it, "
                   "from the margins they keep (0..shave; default 0: hard seams)")
    p.add_argument("--ensemble", type=int, choices=ens.SIZES, default=1, help="geometric self-ensemble: run every window on 2 (the frame "
                   "and its mirror), 4 (the flips) or 8 (flips and transpositions) transformed copies and average the results; K times "
                   "the work (default 1: off)")
    p.add_argument("--roi", default="none", help="region of interest: 'none' (the default: whole frames), 'auto' (the active picture area "
                   "of letterboxed or pillarboxed footage, found from the clip), 'matte' (with --matte: the bounding box of the mattes, "
                   "grown by 20 pixels) or Y,X,H,W (top, left, height, width; at least 20x20): "
                   "only that rectangle is deblurred, the rest of every frame is the input's")
    p.add_argument("--roi_feather", type=int, default=0, help="with --roi: blend the deblurred rectangle with the input over the N pixels "
                   "inside every side of it that is not a side of the frame (0..min(200, H/2, W/2); default 0: a hard edge)")
    p.add_argument("--matte", default=None, help="an 8-bit matte that says how much of the deblurred frame every pixel gets (255: all of "
                   "it, 0: the input frame): an image file (one matte for the clip), or one matte per frame as a directory of images, a "
                   "glob (both in file-name order) or an 8-bit Cmono .y4m file, whose luma bytes are used as stored (255 needs full-range "
                   "grey).  Images are read as one 8-bit channel.  A frame whose matte is empty runs no window and is written as the "
                   "input frame (y4m in and out with the input's chroma layout, depth and range: the input's record, byte for byte)")
    p.add_argument("--matte_invert", action="store_true", help="with --matte: use 255 - m, deblur where the matte is black")
    p.add_argument("--matte_params", default=None, help="with --matte auto ('auto' measures the mattes: deblur where the picture is blurred; "
                   "a file of that name is ./auto): NAME=N,... over thr (0..257, default 192: a cell is blurred where a 9-tap box removes "
                   "less than thr/256 of its adjacent-pixel variation), flat (0..255, default 2: 8-bit levels of RMS difference below "
                   "which a cell is not judged), grow (0..4, default 1: cells of dilation) and hold (0 | 1, default 1: join the cells of "
                   "the frames of a window).  Untuned design parameters")
    p.add_argument("--matte_out", default=None, help="with --matte: write the matte in effect of every frame to this file as an 8-bit Cmono "
                   "y4m record, full range as stored, zeros for a frame that was written as its input; inspect it, repair it in a paint "
                   "tool and feed it back through --matte FILE.y4m")
    p.add_argument("--sharp", choices=SHARP, default="deblur", help="what becomes of a frame labelled sharp (by --labels or the detector): "
                   "'deblur' (the default) runs its window like any other; 'keep' runs none and writes the input frame (y4m in and out "
                   "with the input's chroma layout, depth and range: the input's record, byte for byte).  The blurry frames are the "
                   "same either way; sharp frames still serve them as neighbours and references")
    p.add_argument("--fields", choices=("auto", "progressive", "split"), default="auto", help="interlaced footage: 'split' deblurs the two "
                   "fields of every frame (its even and its odd rows, two instants) as clips of their own under one plan, the top-field "
                   "clip's, and weaves the results; 'progressive' treats the frames as they are, whatever the input's tag says; 'auto' "
                   "(the default) splits iff the y4m input is tagged It or Ib.  The y4m output carries the input's I tag.  Needs an even "
                   "height of at least 40 (a multiple of 4 for 4:2:0 y4m); not with --tiles or --roi")
    p.add_argument("--stream", action="store_true", help="y4m input only: deblur the stream as it arrives, with a bounded look-ahead and "
                   "no spool ('--input -' reads stdin as a pipe; a .y4m file is read in order); the first frames leave before the "
                   "input has ended.  The window plan is exact except where it depends on the rest of a scene, however long: there it "
                   "is committed --horizon frames ahead under an assumption (see StreamPlan) and the frame is counted as assumed")
    p.add_argument("--horizon", type=int, default=48, help=f"with --stream: frames of look-ahead after which a plan entry is committed "
                   f"(default 48, at least {MIN_HORIZON})")
    p.add_argument("--spool_dir", default=None, help="directory of the temporary file that '--input -' is copied to (default: the system's)")
    a = p.parse_args(argv)
    try:
        tiles = tiling.parse_tiles(a.tiles)
    except ValueError as e:
        raise SystemExit(f"--tiles: {e}")
    if a.feather != 0:                                     # refused here, before the model is loaded
        if tiles is None:
            raise SystemExit(f"--feather {a.feather}: needs --tiles: it blends the seams between tiles")
        if not 0 <= a.shave <= tiling.MAX_SHAVE or not 0 <= a.feather <= a.shave:
            raise SystemExit(f"--feather {a.feather}: must be 0..shave (--shave {a.shave}, itself 0..{tiling.MAX_SHAVE}): the ramp is "
                             "blended from the margin the tiles keep")
    try:
        roi = parse_roi(a.roi)
    except ValueError as e:
        raise SystemExit(f"--roi: {e}")
    if roi is not None and tiles is not None:              # refused here, before the model is loaded
        raise SystemExit("--roi with --tiles is not built: the tile egress writes whole frames only")
    if a.fields == "split" and (tiles is not None or roi is not None):
        raise SystemExit(f"--fields split with {'--tiles' if tiles is not None else '--roi'} is not built: the two fields run as the parts "
                         "of a window, and the table of parts is taken")
    if a.roi_feather != 0 and roi is None:
        raise SystemExit(f"--roi_feather {a.roi_feather}: needs --roi: it blends the edge of the region of interest")
    if a.matte is None and a.matte_invert:
        raise SystemExit("--matte_invert: needs --matte: there is no matte to invert")
    if a.matte is None and a.roi == "matte":
        raise SystemExit("--roi matte: needs --matte: the rectangle is the bounding box of the mattes")
    matte, matte_params = None, None
    if a.matte_params is not None:
        if a.matte != "auto":
            raise SystemExit("--matte_params: needs --matte auto: they are the parameters of the measured matte")
        try:
            matte_params = blurmap.parse_params(a.matte_params)
            BlurParams.of(matte_params)
        except ValueError as e:
            raise SystemExit(f"--matte_params: {e}")
    if a.matte_out is not None and a.matte is None:
        raise SystemExit("--matte_out: needs --matte: there is no matte to write")
    if a.matte_out is not None and not a.matte_out.lower().endswith(".y4m"):
        raise SystemExit(f"--matte_out {a.matte_out}: the mattes are written as one Cmono .y4m file")
    if a.matte == "auto":                                  # measured, not read: a file of that name is ./auto
        if a.matte_invert:
            raise SystemExit("--matte auto with --matte_invert: the measured matte is lit where the picture is blurred")
        if a.fields == "split":
            raise SystemExit("--matte auto with --fields split is not built: the rows of an interlaced frame are two instants")
        if a.stream and a.roi == "matte":
            raise SystemExit("--roi matte with --stream: the bounding box is found from every matte before the first window; give Y,X,H,W")
        matte = "auto"
    elif a.matte is not None:                              # a file (an image or a .y4m clip), a directory, or a glob of images
        matte = a.matte if os.path.isfile(a.matte) or os.path.isdir(a.matte) else _inputs(a.matte)
        if not matte or (os.path.isdir(a.matte) and not _inputs(a.matte)):
            raise SystemExit(f"--matte {a.matte}: no image file, directory of images, glob or .y4m file of that name")
        if a.stream and a.roi == "matte" and not (isinstance(matte, str) and os.path.isfile(matte) and not matte.lower().endswith(".y4m")):
            raise SystemExit("--roi matte with --stream: the bounding box is found from every matte before the first window; give "
                             "Y,X,H,W, or one image as the matte of the whole clip")
    to_stdout = a.output == "-"
    to_y4m = to_stdout or a.output.lower().endswith(".y4m")
    log = sys.stderr if to_stdout else sys.stdout
    if not to_y4m and a.out_depth not in (None, 8):
        raise SystemExit(f"--out_depth {a.out_depth}: a PNG directory gets 8-bit files; write a .y4m file or '-' for a deep output")

    if not to_y4m and a.out_chroma is not None:
        raise SystemExit(f"--out_chroma {a.out_chroma}: a PNG directory holds RGB files; write a .y4m file or '-' for a chroma layout")

    def say(text: str) -> None:
        print(text, file=log, flush=True)

    reader = None
    if a.stream:
        if a.horizon < MIN_HORIZON:
            raise SystemExit(f"--horizon {a.horizon}: at least {MIN_HORIZON}")
        if a.roi == "auto":
            raise SystemExit("--roi auto with --stream: the active area is found from the whole clip; give Y,X,H,W")
        if a.input != "-" and not (a.input.lower().endswith(".y4m") and os.path.isfile(a.input)):
            raise SystemExit(f"--stream: --input {a.input} is not '-' or a .y4m file (image files have a known length: nothing to stream)")
        reader = y4m.Y4MStream(sys.stdin.buffer if a.input == "-" else a.input, depths=y4m.DEPTHS, layouts=y4m.LAYOUTS,
                               interlace=y4m.INTERLACE)
    elif a.input == "-":
        reader = y4m.Y4MReader(_spool(sys.stdin.buffer, a.spool_dir), depths=y4m.DEPTHS, layouts=y4m.LAYOUTS, interlace=y4m.INTERLACE)
    elif a.input.lower().endswith(".y4m") and os.path.isfile(a.input):
        reader = y4m.Y4MReader(a.input, depths=y4m.DEPTHS, layouts=y4m.LAYOUTS, interlace=y4m.INTERLACE)
    tag = "p" if reader is None else reader.interlace      # the input's I tag: the y4m output carries it, whatever --fields says
    fields = "split" if a.fields == "split" or (a.fields == "auto" and tag != "p") else None
    if fields is not None and (tiles is not None or roi is not None):
        raise SystemExit(f"--input {a.input} is interlaced (I{tag}) and --fields auto splits it, which is not built with "
                         f"{'--tiles' if tiles is not None else '--roi'}: say --fields progressive to treat the frames as they are")
    if reader is not None:
        if fields is None:
            reader.interlace = "p"       # --fields progressive on an It / Ib input: the user's call, the frames as they are
        if reader.depth > 8 and reader.layout in (y4m.CENTER, y4m.LEFT) and a.chroma in ("420jpeg", "420mpeg2"):
            reader.layout = y4m.layout_of(a.chroma)
        if not a.stream and len(reader) < 2:
            raise SystemExit(f"--input {a.input}: {len(reader)} frame(s) found, a clip needs at least 2")
        files, stems = reader, None if a.stream else [f"{i:06d}" for i in range(len(reader))]
    else:
        files = _inputs(a.input)
        if len(files) < 2:
            raise SystemExit(f"--input {a.input}: {len(files)} image file(s) found, a clip needs at least 2")
        stems = [os.path.splitext(os.path.basename(f))[0] for f in files]
        if len(set(stems)) != len(stems):
            raise SystemExit(f"--input {a.input}: two frames share a file name stem (the outputs are <stem>.png)")
    names = _Numbered("" if to_y4m else ".png") if stems is None else [s if to_y4m else s + ".png" for s in stems]
    labels = np.load(a.labels) if a.labels else None
    net = load_model(a.model_path, a.device, a.precision, a.graph)
    cuts = {"none": None, "auto": "auto"}[a.cuts] if a.cuts in ("none", "auto") else read_cuts(a.cuts)
    yuv = {k: v for k, v in (("matrix", a.matrix), ("range", a.range)) if v is not None} if reader is not None else None
    out_depth = a.out_depth
    if not to_y4m:
        if reader is not None and reader.depth > 8:
            say(f"# {reader.depth}-bit input, PNG output: the frames are written with 8 bits per sample (out_depth 8)")
        out_depth = 8
    run = deblur_clip(net, files, labels, detector=detector.DetectorParams.load(a.detector) if a.detector else None, cuts=cuts,
                      yuv=yuv or None, out_depth=out_depth, tiles=tiles, shave=a.shave, feather=a.feather, ensemble=a.ensemble,
                      roi=roi, roi_feather=a.roi_feather, stream=a.stream, horizon=a.horizon, sharp=a.sharp, fields=fields,
                      **({} if matte is None else dict(matte=matte, matte_invert=a.matte_invert)),
                      **({} if matte_params is None else dict(matte_params=matte_params)))
    out_depth = run.out_depth
    H, W = run.frames.H, run.frames.W
    writer = None
    if to_y4m:
        if reader is not None:
            layout, matrix, rng = run.frames.yuv
            fps, aspect = a.fps or reader.fps, reader.aspect
        else:
            layout, rng = y4m.layout_of(a.chroma or "420jpeg"), y4m.range_of(a.range or "full")
            matrix = y4m.matrix_of(a.matrix) if a.matrix else (y4m.BT709 if H >= 720 else y4m.BT601)
            fps, aspect = a.fps or (25, 1), None
        if a.out_chroma is not None:
            layout = y4m.layout_of(a.out_chroma)
        if fields is not None and layout in (y4m.CENTER, y4m.LEFT) and H % 4:
            raise SystemExit(f"--fields split: a 4:2:0 y4m output of H = {H} rows has no whole chroma rows per field (H must be a multiple "
                             "of 4); write --out_chroma 422 or 444")
        writer = y4m.Y4MWriter(sys.stdout.buffer if to_stdout else a.output, W, H, fps, layout, rng, aspect, depth=out_depth, interlace=tag)
    else:
        os.makedirs(a.output, exist_ok=True)
    if reader is not None:
        say(f"# y4m input C{reader.chroma}" + (f", output C{writer.chroma}" if writer is not None and writer.chroma != reader.chroma else ""))
    if fields is not None or tag != "p":
        say(f"# fields: {'split' if fields is not None else 'progressive'} (I{tag})")
    if run.matte is not None:
        say(f"# matte {a.matte}: {run.matte.describe()}")
    matte_writer = None
    if a.matte_out is not None:
        matte_writer = y4m.Y4MWriter(a.matte_out, W, H, a.fps or (reader.fps if reader is not None else (25, 1)), y4m.MONO, y4m.FULL)
    if run.roi is not None:
        say("# roi " + ",".join(str(v) for v in run.roi))
    said = 0                                               # a stream's cuts are reported as they are found
    if not a.stream:
        for c in run.cuts:
            say(f"# cut before {names[c]}")
    if run.tiles is not None:
        say(f"# {run.tiles.rows}x{run.tiles.cols} tiles of {run.tiles.tw}x{run.tiles.th}, shave {run.tiles.shave}"
            + (f", feather {run.tiles.feather}" if run.tiles.feather else ""))
    if run.ensemble > 1:
        say(f"# ensemble {run.ensemble}: members 0..{run.ensemble - 1}, {run.ensemble} forward passes per frame")
    # a kept frame of a y4m clip (labelled sharp under --sharp keep, or with an empty matte) leaves as the record it came in, when the output's layout, depth and range are the input's (the matrix
    # is one for both sides): no colour conversion, no chroma resampling.  `run.frames.host(i)` is that record
    as_read = ((a.sharp == "keep" or run.matte is not None) and writer is not None and reader is not None
               and (writer.layout, writer.depth, writer.range, writer.frame_bytes) == (run.frames.yuv[0], reader.depth, reader.range,
                                                                                     reader.frame_bytes))
    if a.sharp == "keep":
        say("# sharp keep: no window runs for a frame labelled sharp, it is written as "
            + ("its input record, byte for byte" if as_read else "the input frame at the output depth"))
    t0 = t_prev = time.time()
    done = 0

    def write(buf) -> None:
        writer.write(buf.numpy() if torch.is_tensor(buf) else buf)
        if a.stream and to_stdout:                         # a live pipe: the frame leaves now, not when the buffer is full
            sys.stdout.buffer.flush()
    # PNGs are encoded on four threads; a y4m stream is written by ONE, so its frames land in the order they were queued
    # the mattes of --matte_out (only then): a ring and one writer of their own, so that they land in frame order
    matte_writers = None if matte_writer is None else ThreadPoolExecutor(max_workers=1, thread_name_prefix="speinet-matte")
    matte_ring, blank = None if matte_writer is None else HostRing(matte_writers), None
    with ThreadPoolExecutor(max_workers=1 if to_y4m else 4, thread_name_prefix="speinet-y4m" if to_y4m else "speinet-png") as writers:
        ring = HostRing(writers)
        records = RecordQueue(writers, ring.n)             # input records on their way out: as many in flight as the ring has slots
        for i, frame in run:
            done = i + 1
            if a.stream:
                for c in run.cuts[said:]:
                    say(f"# cut before {names[c]}")
                said = len(run.cuts)
            is_kept = bool(run.kept) and run.kept[-1] == i
            is_unmatted = bool(run.unmatted) and run.unmatted[-1] == i
            if matte_writer is not None:                   # the matte in effect: 255 - m under --matte_invert, zeros where none was used
                m = run.handed_matte
                if m is None:
                    m = blank = torch.zeros(H, W, dtype=torch.uint8, device=frame.device) if blank is None else blank
                elif run.matte.invert:
                    m = 255 - m
                matte_ring.land(lambda buf: matte_writer.write(buf.numpy()), m)
            if (is_kept or is_unmatted) and as_read:                        # a copy: a stream gives the record up a few frames on; the one writer keeps order
                records.put(write, run.frames.host(i))
            elif to_y4m:
                woven = fields is not None and layout in (y4m.CENTER, y4m.LEFT)     # the other layouts convert row by row
                planar = (ops.rgb_u8_to_yuv(frame, layout, matrix, rng, fields=woven) if out_depth == 8 else
                          ops.rgb_u16_to_yuv(frame, layout, matrix, rng, out_depth, fields=woven))
                ring.land(write, planar)
            else:
                ring.land(lambda buf, path=os.path.join(a.output, names[i]): imwrite(path, buf.numpy()), frame)
            now = time.time()
            branch = "kept" if is_kept else "unmatted" if is_unmatted else "no-reference" if run.plan[i]["zero_pre"] else "reference"
            say(f"> {names[i]} {branch} {now - t_prev:.3f}s")
            if run.recomputed and run.recomputed[-1] == i:
                say(f"# {names[i]}: non-finite value in the {a.precision} frame, recomputed in bf16x3 ({len(run.recomputed)} so far)")
            t_prev = now
        ring.drain()
        records.drain()
    if writer is not None:
        writer.close()
    if matte_writer is not None:
        matte_ring.drain()
        matte_writers.shutdown()
        matte_writer.close()
    dt = time.time() - t0
    if a.sharp == "keep":
        say(f"# kept {len(run.kept)} of {done} frames")
    if run.matte is not None:
        say(f"# unmatted {len(run.unmatted)} of {done} frames")
    say(f"# {done} frames {W}x{H} in {dt:.2f}s: {done / dt:.2f} frames/s ({a.precision}"
        + (f", ensemble {run.ensemble}" if run.ensemble > 1 else "")
        + (f", streamed with horizon {a.horizon}: {len(run.assumed)} frames assumed" if a.stream else "") + ")")


if __name__ == "__main__":
    main()
