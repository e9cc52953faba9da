"""GPU suite for `deblur_clip(..., sharp="keep")`: the requant launch (csrc/frame_io.hip `spei_frame_requant`, `ops.frame_requant`)
against the numpy statement `roi_ref.requant`, exactly, and against what `ops.roi_paste` writes outside its rectangle; the clip loop
with kept frames against the `sharp="deblur"` run, frame by frame and bit for bit, alone and composed with every other clip feature;
the launches it issues, counted by entry point; a stream; and the command line, whose kept y4m records are the input's bytes, also
in a stream longer than its ring, with a bounded number of records waiting for a slow sink.
Synthetic weights, frames of 40x60 (80x120 under tiles), clips of 8 frames (40 in the stream that plans under its assumption)."""
import collections
import ctypes
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import roi_ref as RR                                               # noqa: E402
from speinet_amd import _lib, ops, video, y4m                      # noqa: E402
from speinet_amd.clip import frames_of                             # noqa: E402
from speinet_amd.synth import synth_frames                         # noqa: E402

DEV = "cuda:0"
VP = ctypes.c_void_p
DEPTHS = (8, 10, 12)
LABELS = [1, 0, 0, 1, 1, 0, 1, 0]
T = len(LABELS)
SHARP = [i for i, v in enumerate(LABELS) if v]


def _np_dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def _t_dtype(depth):
    return torch.uint8 if depth == 8 else torch.uint16


def _requant(frame, in_depth, out_depth):
    return RR.requant(frame, in_depth, out_depth).astype(_np_dtype(out_depth))


def _dev_requant(frame: np.ndarray, in_depth, out_depth, **kw):
    return ops.frame_requant(torch.from_numpy(frame).to(DEV), out_depth, None if in_depth == 8 else in_depth, **kw).cpu().numpy()


# ---- 1. the launch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_depth", DEPTHS)
@pytest.mark.parametrize("in_depth", DEPTHS)
def test_requant_kernel(in_depth, out_depth):
    """Shapes whose 3 * H * W is a multiple of 16 and not (one sample-triple, fewer than 16 samples, a tail behind whole runs), every
    frame from an aligned base and from a view one sample into a buffer (the element path), words above D_in among the deep ones."""
    Din = (1 << in_depth) - 1
    for h, w in ((1, 1), (3, 5), (21, 37), (40, 64)):
        rng = np.random.default_rng(1000 * h + w + in_depth)
        frame = rng.integers(0, Din + 1, (h, w, 3)).astype(_np_dtype(in_depth))
        if in_depth > 8:
            at = rng.random(frame.shape) < 0.1
            frame[at] = rng.integers(Din + 1, 65536, int(at.sum())).astype(np.uint16)
        ref = _requant(frame, in_depth, out_depth)
        got = _dev_requant(frame, in_depth, out_depth)
        assert got.dtype == ref.dtype and got.shape == (h, w, 3)
        assert np.array_equal(got, ref), (h, w, np.argwhere(got != ref)[:5])
        # source one sample into a buffer; then the destination as well
        buf = torch.from_numpy(np.concatenate([np.zeros(1, frame.dtype), frame.reshape(-1)])).to(DEV)
        view = buf[1:].view(h, w, 3)
        assert view.data_ptr() % 16 != 0
        deep = None if in_depth == 8 else in_depth
        assert np.array_equal(ops.frame_requant(view, out_depth, deep).cpu().numpy(), ref), (h, w)
        obuf = torch.zeros(frame.size + 2, dtype=_t_dtype(out_depth), device=DEV)
        oview = obuf[1:-1].view(h, w, 3)
        assert ops.frame_requant(torch.from_numpy(frame).to(DEV), out_depth, deep, out=oview).data_ptr() == oview.data_ptr()
        flat = obuf.cpu().numpy()
        assert np.array_equal(flat[1:-1].reshape(h, w, 3), ref) and flat[0] == 0 and flat[-1] == 0    # nothing past either end


@pytest.mark.parametrize("out_depth", DEPTHS)
@pytest.mark.parametrize("in_depth", DEPTHS)
def test_requant_every_code(in_depth, out_depth):
    Din = (1 << in_depth) - 1
    codes = list(range(Din + 1)) + ([Din + 1, 4095, 4096, 32768, 65535] if in_depth > 8 else [])
    codes += [0] * (-len(codes) % 3)
    frame = np.asarray(codes).astype(_np_dtype(in_depth)).reshape(1, -1, 3)
    got = _dev_requant(frame, in_depth, out_depth)
    assert np.array_equal(got, _requant(frame, in_depth, out_depth))
    if in_depth == out_depth:
        assert np.array_equal(got, np.minimum(frame, Din))                                          # a copy, with the word clamp
    assert got.max() == (1 << out_depth) - 1 and got.min() == 0


@pytest.mark.parametrize("in_depth,out_depth", [(8, 8), (8, 10), (12, 8), (10, 12)])
def test_requant_is_the_outside_of_the_roi_paste(in_depth, out_depth):
    """One definition: outside a 20x20 rectangle `ops.roi_paste` writes `ops.frame_requant`'s samples."""
    H, W, roi = 40, 64, (10, 20, 20, 20)
    rng = np.random.default_rng(in_depth * 16 + out_depth)
    frame = rng.integers(0, 1 << (in_depth if in_depth == 8 else 16), (H, W, 3)).astype(_np_dtype(in_depth))
    f = torch.from_numpy(frame).to(DEV)
    deep = None if in_depth == 8 else in_depth
    pasted = ops.roi_paste(torch.rand(3, 20, 20, device=DEV), f, roi, out_depth, 0, deep).cpu().numpy()
    whole = ops.frame_requant(f, out_depth, deep).cpu().numpy()
    outside = np.ones((H, W), bool)
    outside[10:30, 20:40] = False
    assert np.array_equal(pasted[outside], whole[outside])
    assert not np.array_equal(pasted[~outside], whole[~outside])


def test_requant_refusals():
    """Refused through the C-ABI before anything is launched: the destination is not written."""
    H, W = 20, 24
    lib = _lib.lib()
    st = VP(torch.cuda.current_stream(DEV).cuda_stream)
    src = torch.full((H, W, 3), 5, dtype=torch.uint16, device=DEV)
    dst = torch.full((H, W, 3), 9, dtype=torch.uint16, device=DEV)
    good = dict(src=src.data_ptr(), in_depth=10, dst=dst.data_ptr(), out_depth=12, H=H, W=W)

    def call(**kw):
        a = dict(good, **kw)
        return lib.spei_frame_requant(VP(a["src"]), a["in_depth"], VP(a["dst"]), a["out_depth"], a["H"], a["W"], st)

    n = 2 * H * W * 3
    cases = [(dict(src=None), "null pointer"), (dict(dst=None), "null pointer"),
             (dict(in_depth=9), "unknown in_depth 9"), (dict(in_depth=16), "unknown in_depth 16"), (dict(in_depth=0), "unknown in_depth 0"),
             (dict(out_depth=11), "unknown out_depth 11"), (dict(out_depth=-8), "unknown out_depth -8"),
             (dict(H=0), "bad frame shape"), (dict(W=0), "bad frame shape"), (dict(H=-1), "bad frame shape"),
             (dict(H=32768, W=32768), "bad frame shape"), (dict(H=1 << 15, W=21846), "bad frame shape"),       # 3 H W >= 2^31
             (dict(src=src.data_ptr() + 1), "misaligned"), (dict(dst=dst.data_ptr() + 1), "misaligned"),
             (dict(dst=src.data_ptr()), "dst overlaps src"), (dict(dst=src.data_ptr() + n - 2), "dst overlaps src"),
             (dict(src=dst.data_ptr() + n - 2), "dst overlaps src"),
             (dict(dst=src.data_ptr() + n - 1, out_depth=8), "dst overlaps src")]
    for kw, text in cases:
        assert call(**kw) != 0, kw
        assert text in lib.spei_last_error().decode() and "spei_frame_requant" in lib.spei_last_error().decode(), (kw, lib.spei_last_error())
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 9).all() and (src.cpu().numpy() == 5).all()                        # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 20).all()                                                           # (5 * 8190 + 1023) // 2046
    # and the wrapper
    f8 = torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="out_depth"):
        ops.frame_requant(f8, 9)
    with pytest.raises(ValueError, match="uint16 frames only"):
        ops.frame_requant(f8, 8, in_depth=10)
    with pytest.raises(ValueError, match="depth must be 10 or 12"):
        ops.frame_requant(src, 8)
    with pytest.raises(RuntimeError, match="dst overlaps src"):
        ops.frame_requant(f8, 8, out=f8)


# ---- 2. the clip --------------------------------------------------------------------------------------------------------------------------
def _clip(n, h, w, depth=8, seed=3):
    """[n,h,w,3] of `depth` bits: the synthetic frames, shifted a little per frame."""
    D = (1 << depth) - 1
    x = synth_frames(1, h, w, seed=seed)[0]
    return np.stack([(torch.roll(x[i % 5], shifts=(i, -2 * i), dims=(1, 2)).permute(1, 2, 0).numpy().astype(np.float64) * D).round()
                     .clip(0, D).astype(_np_dtype(depth)) for i in range(n)])


@pytest.fixture(scope="module", params=["f16-graph", "f32-eager"])
def net(request):
    precision, how = request.param.split("-")
    return video.load_model("synthetic", DEV, precision, how == "graph")


@pytest.fixture(scope="module")
def net32():
    return video.load_model("synthetic", DEV, "f32", False)


def _frames(run):
    out = []
    for i, t in run:
        assert i == len(out)
        out.append(t.cpu().numpy())
    return out


def _inputs(clip, **kw):
    """The input frames as the loop sees them, [H,W,3] numpy each: the array's (cropped for `crop`), or a y4m clip's RGB frames."""
    fr = frames_of(clip, kw.get("crop", False), kw.get("yuv"), kw.get("depth"))
    if fr.yuv is None:
        return fr, [np.asarray(fr.host(i)) for i in range(fr.T)]
    return fr, [fr.rgb(torch.from_numpy(fr.host(i)).to(DEV)[None])[0].cpu().numpy() for i in range(fr.T)]


def _keep_against_deblur(net, clip, labels, **kw):
    """Both runs of one clip; every kept frame is requant(input), every other one the `deblur` run's, bit for bit."""
    base_run = video.deblur_clip(net, clip, labels, **kw)
    base = _frames(base_run)
    if kw.get("out") is not None:
        kw = dict(kw, out=torch.zeros_like(kw["out"]))
    run = video.deblur_clip(net, clip, labels, sharp="keep", **kw)
    assert run.kept == []
    sharp = [i for i, v in enumerate(labels) if v]
    got = []
    for i, t in run:                                           # `kept`: the kept frames handed out so far, this one included
        assert i == len(got) and run.kept == [j for j in sharp if j <= i], (i, run.kept)
        got.append(t.cpu().numpy())
    fr, inputs = _inputs(clip, **kw)
    assert run.kept == sharp and run.recomputed == [] and base_run.kept == [] and run.assumed == []
    assert run.plan == base_run.plan and list(run.labels) == list(base_run.labels) == list(labels)
    assert len(run.seconds) == len(got) == len(base) == len(labels)
    for i in range(len(labels)):
        assert got[i].dtype == base[i].dtype == _np_dtype(run.out_depth) and got[i].shape == base[i].shape == (fr.H, fr.W, 3)
        if i in sharp:
            assert np.array_equal(got[i], _requant(inputs[i], run.depth, run.out_depth)), i
            assert not np.array_equal(got[i], base[i]), i                                           # the window would have changed it
        else:
            assert np.array_equal(got[i], base[i]), i
    if kw.get("out") is not None:
        assert np.array_equal(kw["out"].cpu().numpy(), np.stack(got))
    return run, got


def test_kept_frames_are_the_input_and_the_rest_is_the_deblur_run(net):
    _keep_against_deblur(net, _clip(T, 40, 60), LABELS)


def test_runs_of_sharp_frames_and_sharp_ends(net32):
    """A run of sharp frames whose middle no running window asks for (frames 2..6 around 4, with a gap of 12 in the frame numbers), a
    clip that ends sharp, one that starts with two."""
    clip = _clip(T, 40, 60)
    _keep_against_deblur(net32, clip, [0, 0, 1, 1, 1, 1, 1, 0], numbers=[0, 1, 2, 3, 20, 37, 38, 39])
    _keep_against_deblur(net32, clip, [1, 1, 0, 0, 0, 0, 1, 1])
    _keep_against_deblur(net32, clip[:6], [0, 1, 0, 1, 0, 1])


def test_every_frame_kept_never_calls_the_model(net, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the model was called")
    for name in ("forward_window", "forward", "prefetch_window"):
        monkeypatch.setattr(type(net), name, boom)
    clip = _clip(T, 40, 60)
    run = video.deblur_clip(net, clip, [1] * T, sharp="keep")
    got = _frames(run)
    assert np.array_equal(np.stack(got), clip) and run.kept == list(range(T)) and len(run.seconds) == T
    deep = _clip(6, 40, 60, 12)
    got = _frames(video.deblur_clip(net, deep, [1] * 6, sharp="keep", depth=12, out_depth=8))
    assert np.array_equal(np.stack(got), _requant(deep, 12, 8))


def _counted(monkeypatch):
    seen = []
    orig = _lib.check

    def check(rc, what):
        seen.append(what)
        return orig(rc, what)
    monkeypatch.setattr(_lib, "check", check)
    return seen


def test_launches(net, monkeypatch):
    """By entry point (`_lib.check` sees every call of the library, as in tests/test_gpu_video.py): no blurry label, and `keep` is the
    default run launch for launch; mixed labels, one requant per kept frame and one egress per frame that is not kept."""
    clip = _clip(T, 40, 60)
    for labels in ([0] * T, LABELS):                         # every graph of both plans is captured before anything is counted
        _frames(video.deblur_clip(net, clip, labels))
    seen = _counted(monkeypatch)

    def counts(labels, **kw):
        seen.clear()
        run = video.deblur_clip(net, clip, labels, **kw)
        out = _frames(run)
        torch.cuda.synchronize()
        return collections.Counter(seen), out, run

    blurry_default, a, _ = counts([0] * T)
    blurry_keep, b, run = counts([0] * T, sharp="keep")
    assert blurry_keep == blurry_default and run.kept == [] and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert blurry_default["spei_frame_requant"] == 0 and blurry_default["spei_frame_u8_out"] == T
    mixed_default, _, _ = counts(LABELS)
    assert mixed_default["spei_frame_requant"] == 0 and mixed_default["spei_frame_u8_out"] == T
    mixed_keep, _, run = counts(LABELS, sharp="keep")
    assert run.kept == SHARP
    assert mixed_keep["spei_frame_requant"] == len(SHARP) and mixed_keep["spei_frame_u8_out"] == T - len(SHARP)
    assert mixed_keep["spei_frame_u16_out"] == 0 and mixed_keep["spei_roi_paste_u8"] == 0
    # the ingests of the windows that run, and no other: a kept frame ingests no window input of its own
    n_in = sum(key is not video.ZERO for p in run.plan if p["index"] not in SHARP for key in p["keys"])
    assert mixed_keep["spei_frames_u8_in"] == n_in < mixed_default["spei_frames_u8_in"]


# ---- 3. compositions --------------------------------------------------------------------------------------------------------------------
def _y4m_bytes(clip, layout, depth=8, matrix=y4m.BT601, rng=y4m.LIMITED) -> bytes:
    """The clip as a y4m stream's bytes (the project's own RGB -> YUV kernels make the planes)."""
    f = io.BytesIO()
    wr = y4m.Y4MWriter(f, clip.shape[2], clip.shape[1], (25, 1), layout, rng, depth=depth)
    for frame in clip:
        t = torch.from_numpy(np.ascontiguousarray(frame)).to(DEV)
        planar = ops.rgb_u8_to_yuv(t, layout, matrix, rng) if depth == 8 else ops.rgb_u16_to_yuv(t, layout, matrix, rng, depth)
        wr.write(planar.cpu().numpy())
    return f.getvalue()


COMPOSITIONS = {
    "tiles": (dict(size=(80, 120)), dict(tiles=(2, 2), feather=8)),
    "roi": (dict(), dict(roi=(7, 13, 40, 60), roi_feather=4)),
    "ensemble": (dict(), dict(ensemble=2)),
    "deeper_out": (dict(), dict(out_depth=10)),
    "deep_in": (dict(depth=10), dict(depth=10, out_depth=8)),
    "cuts": (dict(), dict(cuts=[3])),
    "out": (dict(), dict(out=True)),
    "crop": (dict(size=(47, 61)), dict(crop=True)),
    "y4m": (dict(y4m=True), dict()),
}


@pytest.mark.parametrize("name", sorted(COMPOSITIONS))
def test_compositions(net32, name, tmp_path):
    how, kw = (dict(v) for v in COMPOSITIONS[name])
    h, w = how.get("size", (60, 90) if name == "roi" else (40, 60))
    clip = _clip(T, h, w, how.get("depth", 8))
    if how.get("y4m"):
        path = tmp_path / "clip.y4m"
        path.write_bytes(_y4m_bytes(clip, y4m.CENTER))
        clip = y4m.Y4MReader(str(path))
    if kw.get("out"):
        kw["out"] = torch.zeros((T, h, w, 3), dtype=torch.uint8, device=DEV)
    run, got = _keep_against_deblur(net32, clip, LABELS, **kw)
    if name == "crop":
        assert got[0].shape == (40, 60, 3)
    if name == "roi":
        assert run.roi == (7, 13, 40, 60)
    if name == "tiles":
        assert run.tiles is not None and run.tiles.n == 4


# ---- 4. a stream ------------------------------------------------------------------------------------------------------------------------
def test_stream(net32):
    """40 frames with one run of three sharp frames and none after it: `StreamPlan` hands out the entries 11..15 under its assumption
    (situation 1: behind the last sharp frame so far), the last sharp frame's among them; kept, it is not in `assumed`, and every
    frame outside `assumed` is the whole-clip `keep` run's."""
    n = 40
    clip, labels = _clip(n, 40, 60), [1 if i in (9, 10, 11) else 0 for i in range(n)]
    whole = video.deblur_clip(net32, clip, labels, sharp="keep")
    ref = _frames(whole)
    run = video.deblur_clip(net32, iter(clip), labels, stream=True, horizon=24, sharp="keep")
    got = _frames(run)
    assert run.kept == whole.kept == [9, 10, 11] and run.recomputed == []
    raw = run._source.assumed                                  # what the plan assumed, kept frames included
    print("assumed", raw, "of which not kept", run.assumed)
    assert set(raw) & set(run.kept) and run.assumed                               # the case is not empty on either side
    assert run.assumed == [i for i in raw if i not in run.kept] and not set(run.kept) & set(run.assumed)
    for i in range(n):
        if i not in run.assumed:
            assert np.array_equal(got[i], ref[i]), i
    for i in run.kept:
        assert np.array_equal(got[i], clip[i])
    # the same stream under "deblur": its plan, and every frame that is not kept, the assumed ones included
    base_run = video.deblur_clip(net32, iter(clip), labels, stream=True, horizon=24)
    base = _frames(base_run)
    assert base_run.assumed == raw and base_run.plan == run.plan
    assert all(np.array_equal(got[i], base[i]) for i in range(n) if i not in run.kept)
    # the short stream of the other tests: it ends before anything is assumed
    short = video.deblur_clip(net32, iter(_clip(T, 40, 60)), LABELS, stream=True, horizon=24, sharp="keep")
    a, b = _frames(short), _frames(video.deblur_clip(net32, _clip(T, 40, 60), LABELS, sharp="keep"))
    assert short.kept == SHARP and short.assumed == [] and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 5. the command line ------------------------------------------------------------------------------------------------------------------
def _main(capsys, *argv):
    video.main(["--model_path", "synthetic", "--precision", "f32", "--no_graph", "--device", DEV, *argv])
    return capsys.readouterr().out.splitlines()


def _check_log(lines, n_kept, n):
    assert sum(" kept " in ln and ln.startswith("> ") for ln in lines) == n_kept
    assert sum(ln.startswith("> ") for ln in lines) == n
    assert f"# kept {n_kept} of {n} frames" in lines and lines[-1].startswith(f"# {n} frames ")
    assert sum(ln.startswith("# sharp keep") for ln in lines) == 1


def test_cli_png(tmp_path, capsys):
    from PIL import Image
    clip = _clip(T, 40, 60)
    src, dst, lab = tmp_path / "in", tmp_path / "out", tmp_path / "labels.npy"
    src.mkdir()
    for i, f in enumerate(clip):
        Image.fromarray(f).save(src / f"f{i:02d}.png")
    np.save(lab, np.asarray(LABELS))
    lines = _main(capsys, "--input", str(src), "--output", str(dst), "--labels", str(lab), "--sharp", "keep")
    _check_log(lines, len(SHARP), T)
    for i in range(T):
        img = np.asarray(Image.open(dst / f"f{i:02d}.png").convert("RGB"))
        assert np.array_equal(img, clip[i]) == (i in SHARP), i
        assert (f"> f{i:02d}.png kept " in "\n".join(lines)) == (i in SHARP)


def _records(path):
    rd = y4m.Y4MReader(str(path), depths=y4m.DEPTHS, layouts=y4m.LAYOUTS)
    return rd, [rd.raw(i).tobytes() for i in range(len(rd))]


@pytest.mark.parametrize("layout,depth", [(y4m.CENTER, 8), (y4m.P422, 10)], ids=["420p8", "422p10"])
def test_cli_y4m(tmp_path, capsys, layout, depth):
    src, lab = tmp_path / "in.y4m", tmp_path / "labels.npy"
    src.write_bytes(_y4m_bytes(_clip(T, 40, 60, depth), layout, depth))
    np.save(lab, np.asarray(LABELS))
    rd_in, records = _records(src)
    common = ("--input", str(src), "--labels", str(lab))
    lines = _main(capsys, *common, "--output", str(tmp_path / "deblur.y4m"))
    assert not any("kept" in ln for ln in lines)
    rd_ref, ref = _records(tmp_path / "deblur.y4m")
    assert (rd_ref.chroma, rd_ref.depth, rd_ref.range, len(ref)) == (rd_in.chroma, depth, rd_in.range, T)
    variants = [("keep.y4m", ())] + ([("stream.y4m", ("--stream",))] if depth == 8 else [])
    for out, extra in variants:
        lines = _main(capsys, *common, "--output", str(tmp_path / out), "--sharp", "keep", *extra)
        _check_log(lines, len(SHARP), T)
        assert any("byte for byte" in ln for ln in lines if ln.startswith("# sharp keep"))
        rd, got = _records(tmp_path / out)
        assert (rd.chroma, rd.depth, rd.range, len(got)) == (rd_in.chroma, depth, rd_in.range, T)
        for i in range(T):
            assert got[i] == (records[i] if i in SHARP else ref[i]), (out, i)
            assert got[i] != ref[i] or i not in SHARP, (out, i)                   # the round trip through RGB is not the identity
    if depth == 8:                                             # another chroma layout: the kept frame is converted from the input RGB frame
        lines = _main(capsys, *common, "--output", str(tmp_path / "k444.y4m"), "--sharp", "keep", "--out_chroma", "444")
        _check_log(lines, len(SHARP), T)
        assert not any("byte for byte" in ln for ln in lines)
        rd, got = _records(tmp_path / "k444.y4m")
        assert rd.chroma == "444"
        fr, inputs = _inputs(y4m.Y4MReader(str(src)))
        for i in SHARP:
            want = ops.rgb_u8_to_yuv(torch.from_numpy(inputs[i]).to(DEV), y4m.P444, fr.yuv[1], fr.yuv[2]).cpu().numpy().tobytes()
            assert got[i] == want, i


def test_cli_long_stream_of_mostly_kept_frames_holds_few_records(tmp_path, capsys, monkeypatch, net32):
    """96 frames, seven of eight sharp, through `--stream`: more frames than the stream's ring holds (64 slots at horizon 24), so the
    ring has moved on long before the end and every kept record must be taken while its frame is still there; and a sink slower than
    the loop (the write of kept record j does not end before the loop has come to queue record j + 8), so a run of kept frames runs up
    against the bound of the writes in flight: never more than 8 records handed over and not yet written, and 8 reached."""
    import threading
    n, bound = 96, 8
    labels = [0 if i % 8 == 3 else 1 for i in range(n)]
    kept = [i for i, v in enumerate(labels) if v]
    src, lab = tmp_path / "in.y4m", tmp_path / "labels.npy"
    src.write_bytes(_y4m_bytes(_clip(n, 40, 40), y4m.CENTER))
    np.save(lab, np.asarray(labels))
    _, records = _records(src)
    cond = threading.Condition()
    state = dict(reached=0, handed=0, written=0, most=0, peaks=[])

    class Spy(video.RecordQueue):
        def put(self, fn, record):
            with cond:
                j = state["reached"]
                state["reached"] += 1
                cond.notify_all()

            def slow(rec):
                with cond:
                    assert cond.wait_for(lambda: state["reached"] > min(j + self.n, len(kept) - 1), 60)
                    state["most"] = max(state["most"], state["handed"] - state["written"])
                fn(rec)
                with cond:
                    state["written"] += 1
            super().put(slow, record)
            with cond:
                state["handed"] += 1
            state["peaks"].append(self.in_flight)

    monkeypatch.setattr(video, "RecordQueue", Spy)
    lines = _main(capsys, "--input", str(src), "--labels", str(lab), "--output", str(tmp_path / "out.y4m"), "--sharp", "keep", "--stream",
                  "--horizon", "24")
    _check_log(lines, len(kept), n)
    assert state["reached"] == state["written"] == len(kept) and max(state["peaks"]) == bound
    assert state["most"] == bound, state["most"]
    _, got = _records(tmp_path / "out.y4m")
    assert len(got) == n and all(got[i] == records[i] for i in kept)
    run = video.deblur_clip(net32, str(src), labels, stream=True, horizon=24, sharp="keep")      # the other frames: the library's
    for i, f in run:
        if i not in kept:
            assert got[i] == ops.rgb_u8_to_yuv(f, *run.frames.yuv).cpu().numpy().tobytes(), i
    assert run.kept == kept
