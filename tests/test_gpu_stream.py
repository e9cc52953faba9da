"""GPU suite of the streaming clip API (`deblur_clip(..., stream=True)`): a stream's frames against the whole clip's, bit for bit,
with labels given and computed, through every clip feature that composes behind the plan (scene cuts, a y4m pipe, a deep 4:2:2
stream, tiles with an ensemble, a region of interest); the frames that were planned under the assumption (tests/stream_ref.py) and
what they equal; how far the source is read ahead; and the command line between two pipes, whose first frame must leave before the
input has ended.  Synthetic weights, no graphs, frames of 40x60."""
import io
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import stream_ref as R                                             # noqa: E402
from speinet_amd import detector, ops, video, y4m                  # noqa: E402
from speinet_amd.clip import frames_of                             # noqa: E402
from speinet_amd.synth import synth_frames                         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
HORIZON = 24
LABELS = [1 if i in (4, 18, 35) else 0 for i in range(40)]         # three sharp frames, the last one 4 frames from the end
CUTS = [12, 13, 26]                                                # with a one-frame scene


def _clip(T, h, w, depth=8, seed=3):
    """[T,h,w,3] of `depth` bits: the synthetic frames, shifted a little per frame."""
    D = (1 << depth) - 1
    x = synth_frames(1, h, w, seed=seed)[0]
    return np.stack([(torch.roll(x[i % 5], shifts=(i, -2 * i), dims=(1, 2)).permute(1, 2, 0).numpy().astype(np.float64) * D).round()
                     .clip(0, D).astype(np.uint8 if depth == 8 else np.uint16) for i in range(T)])


def _y4m(clip, layout, depth=8, matrix=y4m.BT601, rng=y4m.LIMITED) -> bytes:
    """The clip as a y4m stream's bytes (the project's own RGB -> YUV kernels make the planes)."""
    f = io.BytesIO()
    wr = y4m.Y4MWriter(f, clip.shape[2], clip.shape[1], (25, 1), layout, rng, depth=depth)
    for frame in clip:
        t = torch.from_numpy(np.ascontiguousarray(frame)).to(DEV)
        planar = ops.rgb_u8_to_yuv(t, layout, matrix, rng) if depth == 8 else ops.rgb_u16_to_yuv(t, layout, matrix, rng, depth)
        wr.write(planar.cpu().numpy())
    return f.getvalue()


def _piped(data: bytes, chunk: int = 4099):
    rd, wr = os.pipe()

    def work():
        try:
            with os.fdopen(wr, "wb", buffering=0) as f:
                for i in range(0, len(data), chunk):
                    f.write(data[i:i + chunk])
        except BrokenPipeError:
            pass
    threading.Thread(target=work, daemon=True).start()
    return os.fdopen(rd, "rb", buffering=0)


def _frames(run, upto=None):
    out = []
    for i, t in run:
        assert i == len(out)
        out.append(t.cpu().numpy())
        if upto is not None and i == upto:
            break
    return out


@pytest.fixture(scope="module", params=["f32", "f16"])
def net(request):
    return video.load_model("synthetic", DEV, request.param, False)


@pytest.fixture(scope="module")
def net32():
    return video.load_model("synthetic", DEV, "f32", False)


def _same(a, b, skip=()):
    assert len(a) == len(b)
    bad = [i for i, (x, y) in enumerate(zip(a, b)) if i not in skip and not (x.dtype == y.dtype and np.array_equal(x, y))]
    assert not bad, bad
    assert len({x.tobytes() for x in a}) > len(a) // 2                           # something was computed


def _plans_equal(a, b, skip=()):
    """In what the windows are made from (`pre` and `sub` of a zeroed reference name a far frame of whatever clip was planned)."""
    fields = ("index", "window", "keys", "zero_pre", "zero_sub")
    return len(a) == len(b) and all(p[k] == q[k] for p, q in zip(a, b) for k in fields if p["index"] not in skip)


# ---- labels given: every frame, bit for bit ---------------------------------------------------------------------------------------------
VARIANTS = {
    "plain": dict(),
    "cuts": dict(cuts=CUTS),
    "tiles_ensemble": dict(tiles=(1, 2), ensemble=2, size=(40, 100)),
    "roi": dict(roi=(4, 10, 30, 40), roi_feather=3),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_stream_equals_whole_clip_with_labels(net, variant):
    kw = dict(VARIANTS[variant])
    clip = _clip(40, *kw.pop("size", (40, 60)))
    whole = video.deblur_clip(net, clip, LABELS, **kw)
    run = video.deblur_clip(net, iter(clip), LABELS, stream=True, horizon=HORIZON, **kw)
    assert run.assumed == [] and run.frames.T is None
    ref = _frames(whole)
    _same(_frames(run), ref)
    assert run.assumed == [] and run.frames.T == 40
    assert _plans_equal(run.plan, whole.plan) and run.cuts == whole.cuts and list(run.labels) == LABELS and not run.recomputed
    if variant == "plain":                                                       # an indexable clip, forced to stream
        _same(_frames(video.deblur_clip(net, list(clip), LABELS, stream="force", horizon=HORIZON)), ref)


@pytest.mark.parametrize("layout, depth, out_depth", [(y4m.CENTER, 8, None), (y4m.P422, 10, 8)])
def test_stream_equals_whole_clip_from_a_y4m_pipe(net, tmp_path, layout, depth, out_depth):
    data = _y4m(_clip(40, 40, 60, depth), layout, depth)
    path = tmp_path / "clip.y4m"
    path.write_bytes(data)
    whole = video.deblur_clip(net, str(path), LABELS, out_depth=out_depth)
    pipe = _piped(data)
    run = video.deblur_clip(net, y4m.Y4MStream(pipe, depths=y4m.DEPTHS, layouts=y4m.LAYOUTS), LABELS, out_depth=out_depth, stream=True,
                            horizon=HORIZON)
    assert (run.depth, run.out_depth, run.frames.yuv) == (depth, out_depth or depth, whole.frames.yuv)
    got = _frames(run)
    pipe.close()
    _same(got, _frames(whole))
    assert got[0].dtype == (np.uint8 if (out_depth or depth) == 8 else np.uint16) and run.assumed == []
    again = _frames(video.deblur_clip(net, str(path), LABELS, out_depth=out_depth, stream=True, horizon=HORIZON))   # a path: read in order
    _same(again, got)


def test_stream_errors_on_the_device(net32):
    with pytest.raises(ValueError, match="at least 2 frames .* got 1"):
        next(video.deblur_clip(net32, iter(_clip(1, 40, 60)), stream=True))
    with pytest.raises(ValueError, match="labels has 40 entries and the stream is shorter"):
        _frames(video.deblur_clip(net32, iter(_clip(30, 40, 60)), LABELS, stream=True, horizon=HORIZON))
    with pytest.raises(ValueError, match="horizon must be a whole number >= 24"):
        video.deblur_clip(net32, iter(_clip(3, 40, 60)), stream=True, horizon=8)


# ---- labels and cuts computed as the frames arrive; how far the source is read --------------------------------------------------------------
def _footage(T=64, cut=32, h=40, w=60):
    """Sharp frames (fine texture over the synthetic fields) and box-blurred ones, with another scene from frame `cut` on."""
    rng = np.random.default_rng(7)
    base = _clip(T, h, w).astype(np.float64)
    texture = rng.integers(0, 2, (h // 2, w // 2, 1)).repeat(2, 0).repeat(2, 1)
    out = []
    for i in range(T):
        f = base[i] * 0.6 + texture * 24.0
        if i >= cut:
            f = 255.0 - f * 0.5                                                   # another tonal distribution: a hard cut
        if i % 9 not in (0, 1):                                                   # blurred: a horizontal box of 9
            pad = np.pad(f, ((0, 0), (4, 4), (0, 0)), mode="edge")
            f = np.mean([pad[:, k:k + w] for k in range(9)], axis=0)
        out.append(f.round().clip(0, 255).astype(np.uint8))
    return np.stack(out)


def test_stream_computes_labels_and_cuts_and_reads_ahead_boundedly(net32):
    clip = _footage()
    T = len(clip)
    # a detector that splits this footage: the measure that spreads most, thresholded at its median (the GoPro model calls frames
    # of this size all blurry)
    feats = detector.clip_features(frames_of(clip), DEV).double().cpu().numpy()
    k = int(np.argmax(feats.std(axis=0) / (np.abs(feats).mean(axis=0) + 1e-30)))
    params = detector.DetectorParams(tuple(float(i == k) for i in range(6)), -float(np.median(feats[:, k])))
    whole = video.deblur_clip(net32, clip, cuts="auto", detector=params)
    ref = _frames(whole)
    print("labels", [int(v) for v in whole.labels], "cuts", whole.cuts)
    assert whole.cuts == [32] and T // 4 <= sum(whole.labels) <= T // 2          # the footage has both kinds of frames and its cut
    taken = []

    def source():
        for f in clip:
            taken.append(1)
            yield f

    run = video.deblur_clip(net32, source(), cuts="auto", detector=params, stream=True, horizon=HORIZON)
    bound = HORIZON + 2 * video.DETECT_BATCH + video.PREFETCH + video.LAG + 2
    got = []
    for k, frame in run:
        assert len(taken) <= k + bound, (k, len(taken))
        assert len(run.plan) > k and len(run.labels) >= len(run.plan)
        got.append(frame.cpu().numpy())
    assert list(run.labels) == list(whole.labels) and run.cuts == whole.cuts and run.frames.T == T == len(taken)
    assert set(run.assumed) <= set(R.may_assume(list(whole.labels), whole.cuts, HORIZON))
    _same(got, ref, skip=run.assumed)
    assert _plans_equal(run.plan, whole.plan, skip=run.assumed)


# ---- the frames that were assumed -----------------------------------------------------------------------------------------------------
def test_assumed_frames_are_the_predicted_ones_and_equal_the_assumed_continuation(net32):
    T = 70
    clip, labels = _clip(T, 40, 60), [1 if i == 10 else 0 for i in range(T)]
    want = R.may_assume(labels, [], HORIZON)
    assert want == [j for j in range(3, 17) if j != 12]                           # one sharp frame: situation 2 around it
    run = video.deblur_clip(net32, iter(clip), labels, stream=True, horizon=HORIZON)
    got = _frames(run)
    assert run.assumed == want
    whole = _frames(video.deblur_clip(net32, clip, labels))
    _same(got, whole, skip=want)
    tail = video.ASSUMED_TAIL
    longer = video.deblur_clip(net32, np.concatenate([clip, clip[:len(tail)]]), labels + tail)
    cont = _frames(longer, upto=want[-1])                                          # only the frames in question
    assert all(np.array_equal(got[j], cont[j]) for j in want)
    assert any(not np.array_equal(got[j], whole[j]) for j in want)                 # the assumption mattered
    assert all(run.plan[j]["keys"] == longer.plan[j]["keys"] for j in want)


# ---- the command line between two pipes ---------------------------------------------------------------------------------------------------
def test_cli_streams_between_two_pipes(tmp_path):
    """The child must hand out its first frame while the last 10 input frames are still held back; one timeout over all of it."""
    T, h, w, hold = 80, 40, 40, 10
    data = _y4m(_clip(T, h, w), y4m.CENTER)
    record = len(b"FRAME\n") + y4m.frame_bytes(h, w, y4m.CENTER)
    head = len(data) - T * record
    path = tmp_path / "clip.y4m"
    path.write_bytes(data)
    net16 = video.load_model("synthetic", DEV, "f16", False)
    ref_run = video.deblur_clip(net16, str(path), stream=True)
    ref = [ops.rgb_u8_to_yuv(f, *ref_run.frames.yuv).cpu().numpy().tobytes() for _, f in ref_run]
    assert len(ref) == T
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "speinet_amd.video", "--input", "-", "--output", "-", "--stream", "--no_graph", "--model_path", "synthetic",
           "--device", DEV]
    child = subprocess.Popen(cmd, cwd=ROOT, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    first_out = threading.Event()
    errors = []

    def feed():
        try:
            child.stdin.write(data[:head + (T - hold) * record])
            child.stdin.flush()
            first_out.wait()                                                       # set below, or by the watchdog
            if child.poll() is None:
                child.stdin.write(data[head + (T - hold) * record:])
            child.stdin.close()
        except (BrokenPipeError, ValueError) as e:
            errors.append(e)

    log = []
    logger = threading.Thread(target=lambda: log.append(child.stderr.read()), daemon=True)
    logger.start()
    watchdog = threading.Timer(300, lambda: (child.kill(), first_out.set()))
    watchdog.start()
    try:
        threading.Thread(target=feed, daemon=True).start()

        def read(n):
            buf = b""
            while len(buf) < n:
                more = child.stdout.read(n - len(buf))
                if not more:
                    break
                buf += more
            return buf

        header = child.stdout.readline()
        assert header.startswith(b"YUV4MPEG2 W40 H40 F25:1 Ip C420jpeg"), (header, log)
        out = [read(record)]
        assert len(out[0]) == record, log                                          # the first frame, with 10 input frames still held back
        first_out.set()
        out += [read(record) for _ in range(T - 1)]
        assert child.stdout.read() == b"" and child.wait() == 0
    finally:
        watchdog.cancel()
        if child.poll() is None:
            child.kill()
        child.wait()
    logger.join(10)
    assert not errors and [o[6:] for o in out] == ref and all(o[:6] == b"FRAME\n" for o in out)
    text = log[0].decode() if log else ""
    assert f"# {T} frames 40x40" in text and "streamed with horizon 48" in text and "frames assumed" in text
