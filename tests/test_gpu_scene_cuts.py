"""GPU suite for scene cuts in the clip API: the pair-statistics kernel (csrc/frame_io.hip spei_frame_pair_stats) against numpy, exactly;
`scene_stats` across batch boundaries; `deblur_clip(cuts=...)` bit for bit against `deblur_clip` on every scene alone; `cuts="auto"`;
and the command line's `--cuts`."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from speinet_amd import _lib, detector, inference, ops, video      # noqa: E402
from speinet_amd.synth import synth_frames, synth_scene_u8         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def numpy_stats(frames: np.ndarray):
    """The kernel's contract restated: (sad [T-1], hist [T,64]) of uint8 frames [T,H,W,3] on Y = (77 R + 150 G + 29 B + 128) >> 8."""
    f = frames.astype(np.int64)
    y = (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8
    hist = np.stack([np.bincount((p >> 2).ravel(), minlength=64) for p in y])
    return np.abs(np.diff(y, axis=0)).sum(axis=(1, 2)), hist


def _stats(u8, prev=None):
    sad, hist = ops.frame_pair_stats(u8, prev)
    assert sad.dtype == torch.int64 and hist.dtype == torch.int64 and hist.shape == (u8.shape[0], 64)
    return sad.cpu().numpy(), hist.cpu().numpy()


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h, w", [(20, 20), (37, 53), (99, 141)])
def test_pair_stats_kernel(h, w):
    rng = np.random.default_rng(h * 10007 + w)
    fr = rng.integers(0, 256, (6, h, w, 3), dtype=np.uint8)          # frame 0 serves as `prev`
    ref_sad, ref_hist = numpy_stats(fr)
    assert (ref_hist.sum(axis=1) == h * w).all()
    dev = torch.from_numpy(fr).to(DEV)
    for n in (1, 2, 5):                                              # N = 1 with prev, 2 and 5 without and with
        sad, hist = _stats(dev[1:1 + n], dev[0])
        assert np.array_equal(sad, ref_sad[:n]) and np.array_equal(hist, ref_hist[1:1 + n]), n
        if n > 1:
            sad, hist = _stats(dev[1:1 + n])
            assert np.array_equal(sad, ref_sad[1:n]) and np.array_equal(hist, ref_hist[1:1 + n]), n
    # splitting invariance: 5 frames in one call, or 2 + 3 with the last frame of the first call as `prev` of the second
    s2, h2 = _stats(dev[1:3])
    s3, h3 = _stats(dev[3:6], dev[2])
    assert np.array_equal(np.concatenate([s2, s3]), ref_sad[1:]) and np.array_equal(np.concatenate([h2, h3]), ref_hist[1:])
    # a frame stride larger than the frame: every other frame of a wider buffer
    big = torch.zeros(12, h, w, 3, dtype=torch.uint8, device=DEV)
    big[::2] = dev
    sad, hist = _stats(big[::2][1:], big[0])
    assert np.array_equal(sad, ref_sad) and np.array_equal(hist, ref_hist[1:])
    # a base that is not 4-byte aligned (the byte path), for the frames, for `prev`, and for both
    buf = torch.zeros(fr.size + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = dev.reshape(-1)
    odd = buf[1:].view(6, h, w, 3)
    for frames, prev in ((odd[1:], dev[0]), (dev[1:], odd[0]), (odd[1:], odd[0])):
        sad, hist = _stats(frames, prev)
        assert np.array_equal(sad, ref_sad) and np.array_equal(hist, ref_hist[1:])
    # a frame stride that is no multiple of 4: the frames of one call alternate between the dword path and the byte path
    fs = h * w * 3 + 1
    buf = torch.zeros(6 * fs, dtype=torch.uint8, device=DEV)
    skew = torch.as_strided(buf, (6, h, w, 3), (fs, w * 3, 3, 1))
    skew.copy_(dev)
    sad, hist = _stats(skew)
    assert np.array_equal(sad, ref_sad) and np.array_equal(hist, ref_hist)


def test_pair_stats_kernel_large_extremes():
    """723x1283: more groups of 4 pixels than the launch has threads, so the grid-stride loop runs more than once per thread; an all-0
    frame beside an all-255 frame gives every SAD partial its largest possible value and puts every pixel of a frame into one bin."""
    h, w = 723, 1283
    fr = np.zeros((3, h, w, 3), np.uint8)
    fr[1] = 255
    fr[2] = np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8)
    ref_sad, ref_hist = numpy_stats(fr)
    assert ref_sad[0] == 255 * h * w and ref_hist[0, 0] == h * w and ref_hist[1, 63] == h * w
    dev = torch.from_numpy(fr).to(DEV)
    sad, hist = _stats(dev)
    assert np.array_equal(sad, ref_sad) and np.array_equal(hist, ref_hist)
    sad, hist = _stats(dev[1:2], dev[0])
    assert np.array_equal(sad, ref_sad[:1]) and np.array_equal(hist, ref_hist[1:2])


def test_pair_stats_bad_arguments():
    lib = _lib.lib()
    h, w = 20, 24
    fr = torch.zeros(2, h, w, 3, dtype=torch.uint8, device=DEV)
    hist = torch.zeros(2, 64, dtype=torch.int32, device=DEV)
    sad = torch.zeros(2, dtype=torch.int64, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    src, hp, sp, fs = fr.data_ptr(), hist.data_ptr(), sad.data_ptr(), h * w * 3

    def call(src=src, stride=fs, prev=None, n=2, h=h, w=w, hist=hp, sad=sp):
        return lib.spei_frame_pair_stats(C.c_void_p(src), stride, C.c_void_p(prev), n, h, w, C.c_void_p(hist), C.c_void_p(sad), st)

    assert call() == 0 and call(n=1, prev=src) == 0
    for kw, text in (({"src": None}, "null pointer"), ({"hist": None}, "null pointer"), ({"sad": None}, "null pointer"),
                     ({"n": 0}, "0 frames"), ({"n": -3}, "-3 frames"), ({"n": 1}, "no prev"), ({"stride": fs - 1}, "frame stride"),
                     ({"h": 0}, "bad frame shape"), ({"w": -1}, "bad frame shape"), ({"h": 30000, "w": 30000}, "bad frame shape")):
        assert call(**kw) != 0, kw
        assert text in lib.spei_last_error().decode(), (kw, lib.spei_last_error().decode())
    with pytest.raises(RuntimeError, match="spei_frame_pair_stats failed"):
        ops.frame_pair_stats(fr[:1])


# ---- 2. the streaming pass ------------------------------------------------------------------------------------------------------------------
def test_scene_stats_across_batches(tmp_path):
    """T = 37 crosses two boundaries of the 16-frame batches: the pairs (15, 16) and (31, 32) come from the carried-over frame."""
    from PIL import Image
    T, h, w = 37, 37, 53
    assert T > 2 * video.DETECT_BATCH
    fr = np.random.default_rng(9).integers(0, 256, (T, h, w, 3), dtype=np.uint8)
    ref_sad, ref_hist = numpy_stats(fr)
    for i in range(T):
        Image.fromarray(fr[i]).save(tmp_path / f"{i:04d}.png")
    paths = sorted(str(p) for p in tmp_path.glob("*.png"))
    for src in (paths, fr, torch.from_numpy(fr).to(DEV), list(torch.from_numpy(fr).to(DEV))):
        sad, hist = video.scene_stats(src, DEV)
        assert isinstance(sad, np.ndarray) and sad.dtype == np.int64 and hist.dtype == np.int64
        assert np.array_equal(sad, ref_sad) and np.array_equal(hist, ref_hist)
    # the labelling pass alone, and both in one pass: the same measures, the same statistics
    frs = video.frames_of(fr)
    feats = detector.clip_features(frs, DEV)
    both, (sad, hist) = detector.clip_pass(frs, DEV, features=True, pair_stats=True)
    assert torch.equal(both, feats) and feats.shape == (T, 6)
    assert np.array_equal(sad.cpu().numpy(), ref_sad) and np.array_equal(hist.cpu().numpy(), ref_hist)


# ---- 3. the clip loop: bit identity with every scene run alone ----------------------------------------------------------------------------
def _clip(T, h, w, seed=3):
    """uint8 [T,h,w,3]: the synthetic frames, shifted a little per frame (tests/test_gpu_video.py::_clip)."""
    x = synth_frames(1, h, w, seed=seed)[0]
    return np.stack([(torch.roll(x[i % 5], shifts=(i, -2 * i), dims=(1, 2)).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
                     for i in range(T)])


def _frames(run):
    out = {i: t.cpu().numpy() for i, t in run}
    assert sorted(out) == list(range(len(out)))
    return [out[i] for i in range(len(out))]


@pytest.mark.parametrize("precision, graph", [("f32", False), ("f16", True)])
def test_cuts_equal_every_scene_alone(precision, graph):
    net = video.load_model("synthetic", DEV, precision, graph)
    A, B, Cc = _clip(6, 40, 60, seed=3), _clip(1, 40, 60, seed=11), _clip(5, 40, 60, seed=13)
    la, lb, lc = [1, 0, 0, 0, 0, 1], [1], [1, 0, 0, 0, 1]            # a sharp frame at each side of each join
    joined, labels = np.concatenate([A, B, Cc]), la + lb + lc
    out = torch.empty(12, 40, 60, 3, dtype=torch.uint8, device=DEV)
    run = video.deblur_clip(net, joined, labels, cuts=[6, 7], out=out)
    assert run.cuts == [6, 7] and run.plan == video.window_plan(labels, cuts=[6, 7])
    order = [(i, t.data_ptr()) for i, t in run]
    assert order == [(i, out[i].data_ptr()) for i in range(12)]          # `out=` and the yield order are as without cuts
    got = list(out.cpu().numpy())
    alone_a, alone_c = _frames(video.deblur_clip(net, A, la)), _frames(video.deblur_clip(net, Cc, lc))
    alone_b = _frames(video.deblur_clip(net, np.concatenate([B, B]), lb * 2))[0]
    for k in range(6):
        assert np.array_equal(got[k], alone_a[k]), k
    assert np.array_equal(got[6], alone_b)
    for k in range(5):
        assert np.array_equal(got[7 + k], alone_c[k]), 7 + k
    assert not run.recomputed
    # the argument does something: as one scene, the frames next to the joins take neighbours and references from the other shots
    whole = video.deblur_clip(net, joined, labels)
    assert whole.cuts == []
    one = _frames(whole)
    for k in (5, 6, 7):
        assert not np.array_equal(one[k], got[k]), k


# ---- 4. cuts="auto" ------------------------------------------------------------------------------------------------------------------------
def _edge_clip(h, w, seeds=(1700, 5, 77)):
    return np.concatenate([synth_scene_u8(t, h, w, s, step) for t, s, step in zip((6, 5, 7), seeds, (1, 2, 1))])


@pytest.fixture(scope="module")
def net32():
    return video.load_model("synthetic", DEV, "f32")


@pytest.mark.parametrize("h, w", [(37, 53), (90, 130)])
def test_auto_cuts(net32, h, w, monkeypatch):
    clip = _edge_clip(h, w)
    passes = []
    batches = detector.clip_batches
    monkeypatch.setattr(detector, "clip_batches", lambda *a, **k: passes.append(1) or batches(*a, **k))
    auto = video.deblur_clip(net32, clip, cuts="auto")
    assert not passes                                                # lazily: nothing runs before the first access
    assert auto.cuts == [6, 11]
    labels = auto.labels
    assert len(passes) == 1                                          # labels and cuts from ONE pass over the clip
    assert np.array_equal(labels, video.deblur_clip(net32, clip).labels)
    assert auto.plan == video.window_plan(labels, cuts=[6, 11])
    got = _frames(auto)
    explicit = _frames(video.deblur_clip(net32, clip, labels, cuts=[6, 11]))
    assert all(np.array_equal(a, b) for a, b in zip(got, explicit))
    # given labels: the statistics pass alone; `cut_params` reach the rule
    given = video.deblur_clip(net32, torch.from_numpy(clip).to(DEV), labels, cuts="auto")
    assert given.cuts == [6, 11]
    assert video.deblur_clip(net32, clip, labels, cuts="auto", cut_params={"hist_min": 0.9}).cuts == []
    assert video.find_cuts(*video.scene_stats(clip, DEV), h * w) == [6, 11]


# ---- 5. command line --------------------------------------------------------------------------------------------------------------------------
def test_cli_cuts(net32, tmp_path):
    from PIL import Image
    h, w = 37, 53
    clip = _edge_clip(h, w)
    src = tmp_path / "in"
    src.mkdir()
    for i in range(len(clip)):
        Image.fromarray(clip[i]).save(src / f"frame_{i:03d}.png")
    (tmp_path / "cuts.txt").write_text("6\n11\n")
    labels = np.asarray([1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 1])
    np.save(tmp_path / "labels.npy", labels)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    with_cuts = _frames(video.deblur_clip(net32, clip, labels, cuts=[6, 11]))
    without = _frames(video.deblur_clip(net32, clip, labels))
    assert any(not np.array_equal(a, b) for a, b in zip(with_cuts, without))
    for name, flag, ref in (("none", [], without), ("auto", ["--cuts", "auto"], with_cuts),
                            ("file", ["--cuts", str(tmp_path / "cuts.txt")], with_cuts)):
        dst = tmp_path / name
        r = subprocess.run([sys.executable, "-m", "speinet_amd.video", "--input", str(src), "--output", str(dst), "--model_path", "synthetic",
                            "--labels", str(tmp_path / "labels.npy"), "--precision", "f32", "--device", DEV] + flag,
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        assert [ln for ln in lines if ln.startswith("# cut before ")] == ([] if name == "none" else
                                                                          ["# cut before frame_006.png", "# cut before frame_011.png"])
        assert sum(ln.startswith("> frame_") for ln in lines) == len(clip)
        for i in range(len(clip)):
            assert np.array_equal(inference._imread(str(dst / f"frame_{i:03d}.png")), ref[i]), (name, i)
