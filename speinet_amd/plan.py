"""The window plan of a clip: which frames every output frame's window reads.  Host-only numpy code on `speinet_amd.selection`; the
clip loop that runs the plan on the GPU is speinet_amd.video, which hands out every public name of this module as its own.
  * labels and cuts — `labels_of` (0/1 per frame, 1 = sharp) and `cuts_of` (first-frame-of-scene indices) validate what a caller gave;
  * the cut rule — `find_cuts` on the pair statistics of a whole clip (`video.scene_stats`), `StreamCuts` on the same statistics as
    they arrive; both ask `_is_cut` about every pair and `_check_cut_rule` about their parameters (`CUT_PARAMS`: the keywords);
  * the plan — `window_plan`: `selection.assemble_windows` on every scene as a clip of its own (`_scene_plan`), its frame indices
    mapped back into the clip (`_reindex`), a one-frame scene planned as `_one_frame_scene` says.  An entry's `keys` name the
    n_seq + 2 frames `forward_window` reads, `ZERO` for a zeroed reference;
  * the plan of a stream — `StreamPlan`: the entries of `window_plan` as soon as no continuation of the stream can change them, or
    `horizon` frames ahead under `ASSUMED_TAIL` in the two situations where the reference's selection depends on the whole rest of a
    scene.  Its docstring holds the contract and the argument; tests/stream_ref.py states the two situations independently."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import selection

ZERO = ("zero",)                 # window key of a zeroed reference frame
CUT_PARAMS = ("hist_min", "ratio", "min_delta", "window")     # `cut_params`: find_cuts' keywords


def labels_of(labels, T: Optional[int] = None) -> np.ndarray:
    """Validate sharpness labels: 0 (blurry) or 1 (sharp) per frame, `T` of them when the clip's length is known."""
    lab = np.asarray(labels).reshape(-1)
    if T is not None and lab.size != T:
        raise ValueError(f"labels has {lab.size} entries for a clip of {T} frames")
    if not np.isin(lab, (0, 1)).all():
        raise ValueError("labels must be 0 (blurry) or 1 (sharp) per frame")
    return lab.astype(np.int64)


def cuts_of(cuts, T: int) -> list:
    """Validate scene cuts for a clip of T frames: a strictly increasing sequence of first-frame-of-scene indices in 1..T-1 (None: no
    cuts).  Raises ValueError with the reason."""
    if cuts is None:
        return []
    if isinstance(cuts, (str, bytes)) or not hasattr(cuts, "__iter__"):
        raise ValueError(f"cuts must be a sequence of frame indices, got {cuts!r}")
    arr = np.asarray(list(cuts))
    whole = arr.size == 0 or arr.dtype.kind in "iu" or (arr.dtype.kind == "f" and (arr == np.floor(arr)).all())
    if arr.ndim != 1 or not whole:
        raise ValueError(f"cuts must be a flat sequence of whole frame indices, got {cuts!r}")
    out = [int(c) for c in arr]
    for c in out:
        if not 1 <= c <= T - 1:
            raise ValueError(f"cut {c} is outside 1..{T - 1}: a cut is the index of a scene's first frame in a clip of {T} frames")
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError(f"cuts must be strictly increasing, got {out}")
    return out


def _check_cut_rule(pixels: int, window: int) -> None:
    if pixels <= 0 or window < 0:
        raise ValueError(f"find_cuts: pixels must be positive and window >= 0; got {pixels} and {window}")


def _is_cut(g, d, i: int, hist_min: float, ratio: float, min_delta: float, window: int) -> bool:
    """`find_cuts`' rule for pair i of the float64 sequences g and d (arrays or lists: the maximum of the same doubles either way)."""
    others = [*g[max(0, i - window):i], *g[i + 1:i + 1 + window]]
    return bool(g[i] >= hist_min and d[i] >= min_delta and (not others or g[i] >= ratio * max(others)))


def find_cuts(sad, hist, pixels: int, *, hist_min: float = 0.25, ratio: float = 3.0, min_delta: float = 8.0, window: int = 2) -> list:
    """Hard scene cuts from the pair statistics of a clip (`scene_stats`): sad [T-1], hist [T,64], `pixels` = H * W.  With
    g[i] = sum_b |hist[i+1][b] - hist[i][b]| / (2 pixels) (the share of pixels that changed luma bin, 0..1) and d[i] = sad[i] / pixels
    (mean absolute luma difference), there is a cut before frame i + 1 iff
      g[i] >= hist_min,  d[i] >= min_delta,  and  g[i] >= ratio * max(g[j]) over the other pairs j with |j - i| <= window
    (vacuously true when there are none).  The histogram term is blind to motion; the SAD term vetoes small global brightness steps;
    the neighbourhood term makes a one-frame flash no cut, because its two pairs veto each other.  Returns the sorted list of
    first-frame-of-scene indices.

    Blind spots: a cut between two shots of the same tonal distribution has g near 0 and is missed; dissolves and fades are not hard
    cuts and are not looked for; two cuts within `window` frames of each other veto each other.  The four defaults are design
    parameters, not measurements: ratio 3 over a window of 2 is borrowed from common adaptive cut detectors, and nobody has tuned any
    of them on real footage.  An extension beyond the reference, whose data sets hold one shot per folder."""
    hist = np.asarray(hist, dtype=np.int64)
    sad = np.asarray(sad, dtype=np.float64).reshape(-1)
    if hist.ndim != 2 or hist.shape[0] < 2 or sad.size != hist.shape[0] - 1:
        raise ValueError(f"find_cuts needs hist [T,bins] of T >= 2 frames and sad [T-1]; got {hist.shape} and {sad.shape}")
    _check_cut_rule(pixels, window)
    g = np.abs(np.diff(hist, axis=0)).sum(axis=1) / (2.0 * pixels)
    d = sad / pixels
    return [i + 1 for i in range(g.size) if _is_cut(g, d, i, hist_min, ratio, min_delta, window)]


class StreamCuts:
    """`find_cuts` as the pair statistics arrive: `feed(sad, hist)` takes the next frames' batch (`hist` [n,64]; `sad` [n], or [n-1]
    for the first batch, which has no frame before it: what `detector.clip_analysis` yields) and returns the cuts that became
    certain, `finish()` those that the end of the stream decides.  Pair i is decided once pair i + `window` is known (or the stream
    has ended): the neighbourhood rule looks no further.  `cuts` holds every cut found so far; after `finish` it equals `find_cuts`
    on the whole arrays, with the same arithmetic per pair.  `safe` is the number of leading frames whose scene is certain: no cut
    that is still undecided lies in front of any of them."""

    def __init__(self, pixels: int, *, hist_min: float = 0.25, ratio: float = 3.0, min_delta: float = 8.0, window: int = 2):
        _check_cut_rule(pixels, window)
        self.pixels, self.hist_min, self.ratio, self.min_delta, self.window = pixels, hist_min, ratio, min_delta, int(window)
        self.g, self.d, self.cuts = [], [], []
        self.frames = self.decided = 0
        self._last = None

    def feed(self, sad, hist) -> list:
        hist = np.asarray(hist, dtype=np.int64)
        sad = np.asarray(sad, dtype=np.float64).reshape(-1)
        rows = hist if self._last is None or hist.ndim != 2 else np.concatenate([self._last[None], hist])
        if hist.ndim != 2 or hist.shape[0] < 1 or sad.size != rows.shape[0] - 1:
            raise ValueError(f"StreamCuts.feed needs hist [n,bins] of n >= 1 frames and sad of one entry per new pair; got {hist.shape} "
                             f"and {sad.shape} after {self.frames} frames")
        self.g += (np.abs(np.diff(rows, axis=0)).sum(axis=1) / (2.0 * self.pixels)).tolist()
        self.d += (sad / self.pixels).tolist()
        self._last, self.frames = hist[-1].copy(), self.frames + hist.shape[0]
        return self._decide(False)

    def finish(self) -> list:
        return self._decide(True)

    def _decide(self, ended: bool) -> list:
        new = []
        while self.decided < len(self.g) and (ended or self.decided + self.window < len(self.g)):
            if _is_cut(self.g, self.d, self.decided, self.hist_min, self.ratio, self.min_delta, self.window):
                new.append(self.decided + 1)
            self.decided += 1
        self.cuts += new
        return new

    @property
    def safe(self) -> int:
        return min(self.frames, self.decided + 1)


def _scene_plan(labels, n_seq: int, numbers) -> list:
    """The plan of one continuous scene: `selection.assemble_windows` on its frames."""
    T = len(labels)
    number = int if numbers is None else (lambda i: int(numbers[int(i)]))
    wins = selection.assemble_windows([str(i) for i in range(T)], labels, n_seq, True, number=number)
    plan = []
    for k, w in enumerate(wins):
        win, pre, sub = [int(f) for f in w["window"]], int(w["pre"]), int(w["sub"])
        plan.append({"index": k, "window": win, "pre": pre, "sub": sub, "zero_pre": bool(w["zero_pre"]), "zero_sub": bool(w["zero_sub"]),
                     "keys": win + [ZERO if w["zero_pre"] else pre, ZERO if w["zero_sub"] else sub]})
    return plan


def _reindex(p: dict, index: int, at) -> dict:
    """Entry p of a `_scene_plan` as entry `index` of the clip: every frame index f of the scene becomes the clip's at(f); a `ZERO`
    key stays."""
    q = dict(p, index=index, window=[at(f) for f in p["window"]], pre=at(p["pre"]), sub=at(p["sub"]))
    q["keys"] = [k if k is ZERO else at(k) for k in p["keys"]]
    return q


def _one_frame_scene(i: int, label, n_seq: int, number=None) -> dict:
    """The entry of a one-frame scene {i}: the first entry of the two-frame clip [i, i] with labels [l_i, l_i] and numbers
    [n_i, n_i] (None: the two-frame clip's own indices)."""
    p = _scene_plan([label] * 2, n_seq, None if number is None else [number] * 2)[0]
    return _reindex(p, i, lambda f: i)


def window_plan(labels, n_seq: int = 3, numbers=None, cuts=None) -> list:
    """The window plan for a clip labelled `labels`: one entry per output frame with the n_seq window frames, the two reference frames
    (frame indices), whether each reference is zeroed (more than 7 frame numbers from the last window frame; `zero_pre` is the
    routing: True = no-reference branch) and the n_seq + 2 `forward_window` keys (frame indices, `ZERO` for a zeroed reference).
    `numbers`: the frame numbers the reference gap is measured in (the harness's come from its file names); default: the indices.
    `cuts` (`cuts_of`): the first frame of every scene after the first.  Each scene [a, b) is planned as a clip of its own, on
    labels[a:b] and numbers[a:b], with every frame index shifted by a (`index` stays the output frame's index in the whole clip): the
    windows reflect at the scene's ends and the references come from the scene.  A one-frame scene {i} is planned as the first entry of
    the two-frame clip [i, i] with labels [l_i, l_i] and numbers [n_i, n_i]."""
    T = len(labels)
    cuts = cuts_of(cuts, T)
    if not cuts:
        return _scene_plan(labels, n_seq, numbers)
    plan = []
    for a, b in zip([0] + cuts, cuts + [T]):
        if b - a == 1:
            plan.append(_one_frame_scene(a, labels[a], n_seq, a if numbers is None else numbers[a]))
            continue
        at = list(range(a, b))                                     # the scene's frames
        scene = _scene_plan([labels[i] for i in at], n_seq, [i if numbers is None else numbers[i] for i in at])
        plan += [_reindex(p, a + p["index"], at.__getitem__) for p in scene]
    return plan


ASSUMED_TAIL = [0] * 16 + [1, 1]     # what `StreamPlan` assumes of a scene at its horizon: it goes on, with sharp frames out of reach
MIN_HORIZON = 24


class StreamPlan:
    """`window_plan` as the labels arrive: the plan of a clip whose length, later labels and later cuts are not known yet.

    `feed(labels=None, sad=None, hist=None, count=None)` takes the next frames' batch and returns the plan entries that can be handed
    out now, in frame order, each the dict that `window_plan` makes; `finish()` ends the stream and returns the rest.  `labels`: the
    batch's 0/1 per frame, or None when the constructor was given `labels` for the whole stream (then `count`, or `hist`, says how
    many frames the batch holds; a stream longer or shorter than the labels is a ValueError from the `feed` or the `finish` that
    finds it out).  `cuts`: None (one scene), a strictly increasing list of first-frame-of-scene indices, or "auto": `sad` / `hist`
    of every batch go to a `StreamCuts` (`pixels`, `cut_params`).  `labels`, `cuts` and `plan` hold what is known so far, `assumed`
    the frames whose entry was handed out under the assumption below, `at[j]` the number of frames that had been taken in when entry
    j was handed out.

    The contract, with `horizon` (at least 24; default 48, about 2 s of video: a design parameter, larger than every bounded
    dependence of the plan):
      * an entry is handed out as soon as it is FINAL: its `keys`, `zero_pre` and `zero_sub` are the same for every continuation of
        the stream, whatever labels follow, however long the scene gets, and wherever a cut that `StreamCuts` has not excluded yet
        falls.  At the end of a scene (a cut that is certain, or the end of the stream) everything left is final: it is planned on
        the scene's true labels;
      * if frame j + horizon is known to lie in entry j's scene and entry j is still not final, it is handed out as entry j of
        `window_plan` on the scene's known labels followed by `ASSUMED_TAIL` (the scene goes on and holds later sharp frames, none
        within reach), and j is appended to `assumed`.
    A batch is taken in 8 frames at a time, so an entry is handed out no later than the feed position j + horizon + window + 9
    (`window`: `find_cuts`' neighbourhood, 2 by default, 0 without "auto"), which is below j + horizon + DETECT_BATCH.

    Why this is enough.  With m frames of the scene known, m >= 24 and m >= j + 11 (j counted from the scene's start), every
    continuation gives the scene at least m frames, so both far indices of `blurry_indices` (the padded clip's ends) are more than 7
    frames from entry j's last window frame and are zeroed, and every later sharp frame, the reflected one at the padded clip's end
    included, is at least 10 frames past that frame: out of reach of the 7-frame rule.  What is left of the future in entry j is one
    bit: whether ANY sharp frame follows the known ones.  So the entry is computed for the continuation without one (the known
    labels and two blurry frames) and for `ASSUMED_TAIL`, and is final iff the two agree.  They disagree in two situations only,
    the two global quirks of the reference's selection:
      1. after the last sharp frame so far: entry j's last window frame is fewer than 7 frames past a sharp frame s and no known
         sharp frame follows it.  If s is the scene's last sharp frame the later reference is s; if any sharp frame follows, however
         far, it is the zeroed far index;
      2. exactly one sharp frame in the scene's padded labels so far: the scene is planned by the neighbour rule, and a second sharp
         frame anywhere later switches all of it to the nearest-sharp rule.
    `numbers=` is not supported: the gap rule is in frame indices.  `pre` and `sub` of a zeroed reference (`keys` holds `ZERO` there)
    name the far frame of the continuation the entry was computed on, which need not be the whole clip's, nor a frame of it.

    A long scene is planned on its last frames only (`keep`, at least horizon + 32, kept behind the next entry), with the sharp
    frames before them stood in for by none, one or two sharp frames out of reach: entry j depends on what lies more than 7 frames
    behind it only through their count (none, one, more)."""

    STEP = 8

    def __init__(self, horizon: int = 48, cuts=None, labels=None, pixels: Optional[int] = None, cut_params: Optional[dict] = None,
                 n_seq: int = 3, keep: Optional[int] = None):
        if isinstance(horizon, bool) or not isinstance(horizon, (int, np.integer)) or horizon < MIN_HORIZON:
            raise ValueError(f"horizon must be a whole number >= {MIN_HORIZON}, got {horizon!r}")
        if n_seq != 3:
            raise ValueError("StreamPlan plans 3-frame windows")
        self.horizon, self.n_seq = int(horizon), n_seq
        self.keep = max(self.horizon + 32, 64) if keep is None else int(keep)
        if self.keep < self.horizon + 32:
            raise ValueError(f"keep must be at least horizon + 32 = {self.horizon + 32}, got {keep!r}")
        self._given = None if labels is None else labels_of(labels)
        self._auto = None
        self._cut_list = None
        if isinstance(cuts, str):
            if cuts != "auto":
                raise ValueError(f"cuts must be None, \"auto\" or a sequence of frame indices, got {cuts!r}")
            if pixels is None:
                raise ValueError("cuts=\"auto\" needs pixels= (H * W)")
            self._auto = StreamCuts(pixels, **(cut_params or {}))
        elif cuts is not None:
            try:                         # the clip's length is not known: every bound but the upper one is checked here
                top = max((int(c) for c in cuts), default=0)
            except (TypeError, ValueError):
                top = 0
            self._cut_list = cuts_of(cuts, top + 1)
        self.labels, self.cuts, self.plan, self.assumed, self.at = [], [], [], [], []
        self.fed = 0                     # frames taken in
        self.start = 0                   # first frame of the scene being planned
        self._c0, self._before = 0, 0    # the scene is planned from frame _c0 on; sharp frames (padded) of the scene before it
        self.ended = False

    # ---- feeding ----
    def feed(self, labels=None, sad=None, hist=None, count: Optional[int] = None) -> list:
        if self.ended:
            raise ValueError("the stream has ended")
        if self._given is not None:
            n = int(count) if count is not None else (len(hist) if hist is not None else len(labels))
            if self.fed + n > self._given.size:
                raise ValueError(f"labels has {self._given.size} entries and the stream is longer: frame {self._given.size} has arrived")
            lab = self._given[self.fed:self.fed + n]
        else:
            lab = labels_of(labels)
        n = len(lab)
        if self._auto is not None:
            if hist is None or sad is None or len(hist) != n:
                raise ValueError(f"cuts=\"auto\" needs the pair statistics of the batch's {n} frames")
            sad, hist = np.asarray(sad).reshape(-1), np.asarray(hist)
        out, lead = [], 1 if self.fed == 0 else 0        # the stream's first batch has no pair for its first frame
        for a in range(0, n, self.STEP):
            b = min(n, a + self.STEP)
            self.labels += [int(v) for v in lab[a:b]]
            self.fed += b - a
            if self._auto is not None:
                self._auto.feed(sad[max(a - lead, 0):b - lead], hist[a:b])
                self.cuts = list(self._auto.cuts)
            out += self._advance()
        return out

    def finish(self) -> list:
        if self.ended:
            return []
        if self._given is not None and self.fed != self._given.size:
            raise ValueError(f"labels has {self._given.size} entries and the stream is shorter: it ended after {self.fed} frames")
        if self._cut_list and self._cut_list[-1] > self.fed - 1:
            cuts_of(self._cut_list, self.fed)
        self.ended = True
        if self._auto is not None:
            self._auto.finish()
            self.cuts = list(self._auto.cuts)
        return self._advance()

    # ---- planning ----
    def _safe(self) -> int:
        return self.fed if self._auto is None or self.ended else self._auto.safe

    def _scene_end(self) -> Optional[int]:
        """The end of the scene being planned, once it is certain; None while it is not."""
        if self._cut_list is not None:
            nxt = next((c for c in self._cut_list if c > self.start), None)
            if nxt is not None and nxt <= self.fed:
                if nxt not in self.cuts:
                    self.cuts.append(nxt)
                return nxt
        elif self._auto is not None:
            nxt = next((c for c in self.cuts if c > self.start), None)
            if nxt is not None:
                return nxt
        return self.fed if self.ended else None

    def _planned(self, stop: int, tail: list):
        """`_scene_plan` of the scene's frames [_c0, stop) and `tail`, behind the stand-in of what was dropped; (plan, offset): entry
        j of the clip is plan[j - offset], its frame indices shifted by offset."""
        head = [] if self._c0 == self.start else [0, 0, 0] + [1] * min(self._before, 2) + [0] * 16
        return _scene_plan(head + self.labels[self._c0:stop] + tail, self.n_seq, None), self._c0 - len(head)

    def _hand(self, q: dict, assumed: bool = False) -> dict:
        if assumed:
            self.assumed.append(q["index"])
        self.plan.append(q)
        self.at.append(self.fed)
        return q

    def _advance(self) -> list:
        out = []
        while True:
            nxt, end = len(self.plan), self._scene_end()
            if end is not None:          # a whole scene (what is left of it): its true labels
                if end - self.start == 1:
                    out.append(self._hand(_one_frame_scene(self.start, self.labels[self.start], self.n_seq)))
                elif nxt < end:
                    plan, off = self._planned(end, [])
                    out += [self._hand(_reindex(plan[j - off], j, lambda f: f + off)) for j in range(nxt, end)]
                if end >= self.fed and self.ended:
                    return out
                self.start = self._c0 = end
                self._before = 0
                continue
            m = self._safe() - self.start                                  # frames known to lie in the scene
            if self._cut_list is not None:
                m = min(m, next((c for c in self._cut_list if c > self.start), self.fed) - self.start)
            if m < MIN_HORIZON or nxt - self.start + 11 > m:
                return out
            if nxt - self._c0 > 2 * self.keep:                             # plan on the scene's last frames only
                c0 = nxt - self.keep
                if self._c0 == self.start:
                    self._before += self.labels[self.start + 1]            # the padded clip's first frame is frame 1 again
                self._before += sum(self.labels[self._c0:c0])
                self._c0 = c0
            stop = self.start + m
            (blurry, off), (sharp, _) = self._planned(stop, [0, 0]), self._planned(stop, ASSUMED_TAIL)
            for j in range(nxt, stop - 10):
                a, b = blurry[j - off], sharp[j - off]
                final = (a["keys"], a["zero_pre"], a["zero_sub"]) == (b["keys"], b["zero_pre"], b["zero_sub"])
                if not final and not j + self.horizon < stop:
                    break
                out.append(self._hand(_reindex(b, j, lambda f: f + off), assumed=not final))
            return out
