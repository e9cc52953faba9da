"""CPU suite of the streaming clip API: the sequential y4m reader (`y4m.Y4MStream`) against `Y4MReader` on the same bytes through a
pipe, the bounded frame source (`clip.FrameRing`, `clip.StreamFrames`), the incremental cuts (`video.StreamCuts`) against
`find_cuts`, the incremental plan (`video.StreamPlan`) against `window_plan` (randomised, and exhaustively for short scenes) with
the two situations of tests/stream_ref.py as the only ones in which it may assume, and `deblur_clip`'s argument checks."""
import itertools
import os
import threading

import numpy as np
import pytest

import stream_ref as R
from speinet_amd import clip, video, y4m

H, W = 21, 23


def _piped(data: bytes, chunk: int = 997):
    """A non-seekable binary file object that a writer thread feeds `data` in chunks of `chunk` bytes."""
    rd, wr = os.pipe()

    def work():
        try:
            with os.fdopen(wr, "wb", buffering=0) as f:
                for i in range(0, len(data), chunk):
                    f.write(data[i:i + chunk])
        except BrokenPipeError:                      # the reader gave up on purpose
            pass
    t = threading.Thread(target=work, daemon=True)
    t.start()
    return os.fdopen(rd, "rb", buffering=0), t


ATTRS = ("width", "height", "fps", "aspect", "layout", "depth", "chroma", "range", "matrix", "frame_bytes")


# ---- the reader -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(R.TAGS))
def test_stream_reader_equals_file_reader(tmp_path, tag):
    data, frames = R.y4m_bytes(tag, H, W, 5, seed=len(tag))
    path = tmp_path / "clip.y4m"
    path.write_bytes(data)
    f, t = _piped(data, 997)
    with y4m.Y4MReader(str(path), depths=y4m.DEPTHS, layouts=y4m.LAYOUTS) as ref, y4m.Y4MStream(f, depths=y4m.DEPTHS, layouts=y4m.LAYOUTS) as s:
        assert not hasattr(s, "__len__")
        assert [getattr(s, a) for a in ATTRS] == [getattr(ref, a) for a in ATTRS]
        buf = np.empty(s.frame_bytes, np.uint8)
        for i in range(len(ref)):
            assert s.read_into(buf) is True and s.frames == i + 1
            assert buf.tobytes() == frames[i] == ref.raw(i).tobytes()
        assert s.read_into(buf) is False and s.read_into(buf) is False
    t.join(10)
    f.close()


def test_stream_reader_frame_parameters_and_defaults():
    data, frames = R.y4m_bytes("420jpeg", H, W, 3, frame_line=b"FRAME Ip\n", extra="")
    f, t = _piped(data, 13)
    s = y4m.Y4MStream(f)
    assert (s.fps, s.aspect, s.range, s.matrix, s.layout, s.depth) == ((25, 1), None, y4m.LIMITED, y4m.BT601, y4m.CENTER, 8)
    buf = bytearray(s.frame_bytes)
    assert [s.read_into(buf) and bytes(buf) == fr for fr in frames] == [True] * 3 and not s.read_into(buf)
    with pytest.raises(ValueError, match="the buffer holds 7"):
        s.read_into(bytearray(7))
    f.close()


def test_stream_reader_errors(tmp_path):
    data, frames = R.y4m_bytes("420jpeg", H, W, 3)
    buf = np.empty(len(frames[0]), np.uint8)
    for cut in (5, 3 + len(frames[0]) // 2):                                # inside the last FRAME line's record; inside its payload
        f, _ = _piped(data[:len(data) - len(frames[0]) - 6 + cut])
        s = y4m.Y4MStream(f)
        assert s.read_into(buf) and s.read_into(buf)
        with pytest.raises(ValueError, match="frame 2 is cut short"):
            s.read_into(buf)
        f.close()
    bad = data.replace(b"FRAME\n" + frames[1], b"FRAMe\n" + frames[1])     # a wrong FRAME line, of the first one's length
    f, _ = _piped(bad)
    s = y4m.Y4MStream(f)
    assert s.read_into(buf)
    with pytest.raises(ValueError, match="frame 1 does not start with a FRAME line of 6 bytes like the first frame's"):
        s.read_into(buf)
    f.close()
    # the header's errors are the file reader's, word for word
    for head in (b"YUV4MPEG2 W23 H21 It C420jpeg\n", b"YUV4MPEG2 W23 H21 C422\n", b"YUV4MPEG2 W23 H21 C420p10\n", b"YUV4MPEG2 H21\n", b"RIFF....\n"):
        path = tmp_path / "bad.y4m"
        path.write_bytes(head + b"FRAME\n" + frames[0])
        with pytest.raises(ValueError) as want:
            y4m.Y4MReader(str(path))
        f, _ = _piped(head + b"FRAME\n" + frames[0])
        with pytest.raises(ValueError) as got:
            y4m.Y4MStream(f)
        assert str(got.value).split(": ", 1)[1] == str(want.value).split(": ", 1)[1]               # behind the stream's name
        f.close()
    f, _ = _piped(b"YUV4MPEG2 W23 H21 It C420jpeg\n")
    with pytest.raises(ValueError, match="interlaced streams are not supported"):
        y4m.Y4MStream(f)
    f.close()
    f, _ = _piped(b"YUV4MPEG2 W23 H21 C420jpeg\n")                          # a header and nothing else: a clean end at once
    assert y4m.Y4MStream(f).read_into(buf) is False
    f.close()


# ---- the ring ---------------------------------------------------------------------------------------------------------------------------
def test_ring_is_bounded_and_released_frames_raise():
    made = []

    def source():
        for i in range(40):
            made.append(i)
            yield np.full((20, 24, 3), i, np.uint8)

    fr = clip.frames_of(source())
    assert isinstance(fr, clip.StreamFrames) and fr.T is None and (fr.H, fr.W, fr.depth, fr.yuv) == (20, 24, 8, None)
    fr.reserve(6)
    assert fr.upto(4) == 4
    fr.ring.cv.acquire()
    fr.ring.cv.wait_for(lambda: fr.ring.read == 6, timeout=10)               # the reader thread fills the ring and stops there
    fr.ring.cv.release()
    assert fr.ring.read == 6 and len(made) <= 7                             # at most the ring (and the frame it holds in its hand)
    assert [int(fr.host(i)[0, 0, 0]) for i in range(6)] == list(range(6))
    with pytest.raises(IndexError, match="has not been read yet"):
        fr.host(6)
    with pytest.raises(IndexError, match="cannot be waited for"):
        fr.upto(8)
    fr.release(3)
    assert fr.upto(9) == 9 and int(fr.host(8)[1, 2, 0]) == 8
    with pytest.raises(IndexError, match="released already"):
        fr.host(2)
    view = fr.view((2, 4, 10, 12))
    assert view.host(5).shape == (10, 12, 3) and view.T is None
    with pytest.raises(ValueError, match="cannot be sampled"):
        fr.sample([0])
    n = 9
    while fr.T is None:                                                      # drain it: the length is known at the end only
        fr.release(n - 2)
        n = fr.upto(n + 4)
    assert fr.T == 40 == view.T and fr.upto(100) == 40


def test_stream_source_errors_reach_the_consumer():
    def source():
        yield np.zeros((20, 24, 3), np.uint8)
        yield np.zeros((20, 25, 3), np.uint8)

    fr = clip.frames_of(source())
    with pytest.raises(ValueError, match="mixed frames"):
        fr.upto(2)
    with pytest.raises(ValueError, match="uint16 frames need depth"):
        clip.frames_of(iter([np.zeros((20, 24, 3), np.uint16)]))
    deep = clip.frames_of(iter([np.zeros((20, 24, 3), np.uint16)] * 3), depth=10)
    assert deep.depth == 10 and deep.upto(5) == 3 and deep.T == 3 and deep.host(2).dtype == np.uint16
    data, frames = R.y4m_bytes("422p10", H, W, 3)
    f, _ = _piped(data[:-5])
    fr = clip.frames_of(y4m.Y4MStream(f, depths=y4m.DEPTHS, layouts=y4m.LAYOUTS), yuv=dict(matrix="bt709"))
    assert fr.yuv == (y4m.P422, y4m.BT709, y4m.FULL) and fr.depth == 10 and fr.upto(2) == 2 and fr.host(1).tobytes() == frames[1]
    with pytest.raises(ValueError, match="frame 2 is cut short"):
        fr.upto(3)
    f.close()


# ---- the cuts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(40))
def test_stream_cuts_equal_find_cuts(seed):
    rng = np.random.default_rng(seed)
    T, pixels, window = int(rng.integers(2, 120)), 4096, int(rng.integers(0, 4))
    hist = np.empty((T, 64), np.int64)
    for t in range(T):                                                       # a new tonal distribution now and then, else the last one, jittered
        hist[t] = rng.multinomial(pixels, rng.dirichlet(np.ones(64) * 0.3)) if t == 0 or rng.random() < 0.25 else hist[t - 1]
    sad = rng.choice([0.0, 5.0, 9.0, 40.0], T - 1) * pixels
    ref = video.find_cuts(sad, hist, pixels, window=window)
    sc, i, found = video.StreamCuts(pixels, window=window), 0, []
    while i < T:
        n = int(rng.integers(1, 24))
        found += sc.feed(sad[max(i - 1, 0):i + n - 1], hist[i:i + n])
        assert sc.safe <= sc.frames == min(T, i + n) and all(c <= sc.safe for c in sc.cuts)
        assert sc.cuts == [c for c in ref if c <= sc.decided]                 # what is decided is decided for good
        i += n
    found += sc.finish()
    assert found == sc.cuts == ref and sc.safe == T


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
FIELDS = ("keys", "zero_pre", "zero_sub", "index", "window")
N_CASES = 2400


def _stream_plan(labels, cuts, horizon, batches, **kw):
    sp, out, i = video.StreamPlan(horizon, cuts=cuts or None, **kw), [], 0
    for n in batches:
        out += sp.feed(labels[i:i + n])
        i += n
    return sp, out + sp.finish()


def test_stream_plan_randomised():
    """Every randomised case must stay inside the first assertion (what is not assumed is `window_plan`'s): none is left out."""
    seen = {1: 0, 2: 0}
    for seed in range(N_CASES):
        labels, cuts, horizon, batches = R.plan_case(seed)
        T = len(labels)
        sp, got = _stream_plan(labels, cuts, horizon, batches, keep=None if seed % 2 else horizon + 32)
        ref = video.window_plan(labels, cuts=cuts)
        assert [p["index"] for p in got] == list(range(T)) and got == sp.plan and sp.labels == labels and sp.cuts == cuts
        for p, q in zip(got, ref):
            if p["index"] not in sp.assumed:
                assert all(p[k] == q[k] for k in FIELDS), (seed, p, q)
        if all(b - a <= horizon for a, b in R.scenes(T, cuts)):
            assert sp.assumed == [], seed
        allowed = R.may_assume(labels, cuts, horizon)
        for j in sp.assumed:
            assert j in allowed, (seed, j)
            (a, b), = [s for s in R.scenes(T, cuts) if s[0] <= j < s[1]]
            seen[R.quirk(labels[a:b], j - a, horizon)] += 1
        assert all(sp.at[j] <= j + horizon + video.DETECT_BATCH for j in range(T)), seed
    assert min(seen.values()) > 50, seen                                     # both situations were met


def test_stream_plan_long_scene_is_planned_on_its_last_frames():
    rng = np.random.default_rng(5)
    labels = (rng.random(1500) < 0.04).astype(int).tolist()
    labels[3:400] = [0] * 397                                                # a long stretch behind one sharp frame: situation 2, then 1
    for cuts in (None, [700, 701, 1200]):
        sp, got = _stream_plan(labels, cuts, 24, [16] * 93 + [12])
        ref = video.window_plan(labels, cuts=cuts)
        assert sp._c0 > sp.start                                             # the scene's head was dropped
        assert all(p[k] == q[k] for p, q in zip(got, ref) for k in FIELDS if p["index"] not in sp.assumed)
        assert set(sp.assumed) <= set(R.may_assume(labels, cuts or [], 24)) and sp.assumed


def test_stream_plan_exhaustive_short_scenes():
    for n in range(2, 13):
        for labels in itertools.product((0, 1), repeat=n):
            for batches in ([n], [1] * n):
                sp, got = _stream_plan(list(labels), None, 24, batches)
                assert not sp.assumed and all(p[k] == q[k] for p, q in zip(got, video.window_plan(list(labels))) for k in FIELDS), labels


def test_stream_plan_given_labels_and_cuts():
    labels = [0, 1] * 30
    sp = video.StreamPlan(24, labels=np.asarray(labels), cuts=[10, 11])
    got = sp.feed(count=40) + sp.feed(count=20) + sp.finish()
    assert all(p[k] == q[k] for p, q in zip(got, video.window_plan(labels, cuts=[10, 11])) for k in FIELDS) and len(got) == 60
    sp = video.StreamPlan(24, labels=labels)
    sp.feed(count=50)
    with pytest.raises(ValueError, match="labels has 60 entries and the stream is longer"):
        sp.feed(count=11)
    sp = video.StreamPlan(24, labels=labels)
    sp.feed(count=59)
    with pytest.raises(ValueError, match="labels has 60 entries and the stream is shorter: it ended after 59"):
        sp.finish()
    sp = video.StreamPlan(24, cuts=[30, 70])
    sp.feed([0] * 70)
    with pytest.raises(ValueError, match="cut 70 is outside 1..69"):
        sp.finish()
    for bad in (dict(horizon=23), dict(horizon=True), dict(cuts="scenes"), dict(cuts=[5, 5]), dict(cuts=[0]), dict(cuts="auto"),
                dict(labels=[0, 2]), dict(keep=40)):
        with pytest.raises(ValueError):
            video.StreamPlan(**bad)


def test_stream_plan_with_auto_cuts():
    rng = np.random.default_rng(11)
    T, pixels = 150, 2400
    hist = np.stack([rng.multinomial(pixels, np.ones(64) / 64)] * T)
    for c in (40, 41, 100):
        hist[c:] = rng.multinomial(pixels, rng.dirichlet(np.ones(64) * 0.2))
    sad = np.full(T - 1, 30.0 * pixels)
    cuts = video.find_cuts(sad, hist, pixels, window=0)
    assert cuts == [40, 41, 100]
    labels = (rng.random(T) < 0.1).astype(int).tolist()
    for window in (0, 2):
        ref_cuts = video.find_cuts(sad, hist, pixels, window=window)
        sp, got, i = video.StreamPlan(24, cuts="auto", pixels=pixels, cut_params=dict(window=window)), [], 0
        while i < T:
            n = int(rng.integers(1, 30))
            got += sp.feed(labels[i:i + n], sad[max(i - 1, 0):i + n - 1], hist[i:i + n])
            i += n
        got += sp.finish()
        assert sp.cuts == ref_cuts
        ref = video.window_plan(labels, cuts=ref_cuts)
        assert len(got) == T and all(p[k] == q[k] for p, q in zip(got, ref) for k in FIELDS if p["index"] not in sp.assumed)
        assert set(sp.assumed) <= set(R.may_assume(labels, ref_cuts, 24))
        assert all(sp.at[j] <= j + 24 + video.DETECT_BATCH for j in range(T))


# ---- deblur_clip's argument checks ---------------------------------------------------------------------------------------------------------
def test_deblur_clip_stream_argument_errors():
    frames = np.zeros((4, 20, 24, 3), np.uint8)

    def it():
        return iter(list(frames))

    with pytest.raises(ValueError, match="stream=True on a clip whose length is known"):
        video.deblur_clip(None, frames, [1, 0, 0, 1], stream=True)
    with pytest.raises(ValueError, match="its length is not known, pass stream=True"):
        video.deblur_clip(None, it(), [1, 0, 0, 1])
    with pytest.raises(ValueError, match="out= with stream=True"):
        video.deblur_clip(None, it(), out=frames, stream=True)
    with pytest.raises(ValueError, match="numbers= with stream=True"):
        video.deblur_clip(None, it(), numbers=[0, 1, 2, 3], stream=True)
    with pytest.raises(ValueError, match='roi="auto" with stream=True'):
        video.deblur_clip(None, it(), roi="auto", stream=True)
    with pytest.raises(ValueError, match="stream must be False, True or"):
        video.deblur_clip(None, it(), stream=1.5)
    with pytest.raises(ValueError, match="roi .* lies outside"):
        video.deblur_clip(None, it(), roi=(0, 0, 30, 30), stream=True)
    with pytest.raises(ValueError, match="takes an array or a list of host frames"):
        video.deblur_clip(None, "clip.png", stream="force")
