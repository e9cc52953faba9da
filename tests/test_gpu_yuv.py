"""GPU suite for y4m clips: the two planar-YUV kernels (csrc/yuv_io.hip) bit for bit against the numpy restatement of their definition
(tests/yuv_ref.py); `deblur_clip` on a y4m clip against `deblur_clip` on the RGB frames the kernel makes of it; the command line's
y4m input and output; and the C-ABI's argument checks."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import yuv_ref as R                                                # noqa: E402
from speinet_amd import _lib, detector, ops, video, y4m            # noqa: E402
from speinet_amd.synth import synth_frames                         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LAYOUTS = (R.CENTER, R.LEFT, R.P444)
MODES = [(lay, m, r) for lay in LAYOUTS for m in (R.BT601, R.BT709) for r in (R.FULL, R.LIMITED)]
# 1x1 and 3x5: every neighbour clamped; 20x20: aligned rows, 4:2:0 chroma rows of 10 bytes; 21x23: odd on both axes (partial last
# chroma row and column, unaligned rows); 37x53: the same over more than one block
SIZES = [(1, 1), (3, 5), (20, 20), (21, 23), (37, 53)]


def _to_rgb(planar, h, w, mode):
    return ops.yuv_to_rgb_u8(planar, h, w, *mode).cpu().numpy()


# ---- 1. the kernels -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h, w", SIZES)
def test_yuv_to_rgb_kernel(h, w):
    rng = np.random.default_rng(h * 10007 + w)
    for mode in MODES:
        nb = R.frame_bytes(h, w, mode[0])
        assert ops.yuv_frame_bytes(h, w, mode[0]) == nb
        fr = np.stack([rng.integers(0, 256, nb, dtype=np.uint8), np.zeros(nb, np.uint8), np.full(nb, 255, np.uint8)])
        ref = np.stack([R.yuv_to_rgb(f, h, w, *mode) for f in fr])
        dev = torch.from_numpy(fr).to(DEV)
        got = ops.yuv_to_rgb_u8(dev, h, w, *mode)                          # N = 3, packed
        assert got.dtype == torch.uint8 and got.shape == (3, h, w, 3)
        assert np.array_equal(got.cpu().numpy(), ref), mode
        assert np.array_equal(_to_rgb(dev[0], h, w, mode), ref[:1]), mode   # one frame, [frame_bytes]
        out = torch.zeros(3, h, w, 3, dtype=torch.uint8, device=DEV)
        assert ops.yuv_to_rgb_u8(dev, h, w, *mode, out=out) is out and np.array_equal(out.cpu().numpy(), ref), mode
        for stride in (nb + 8, nb + 5):                                    # a frame stride larger than a frame: a multiple of 4, and not
            big = torch.full((3 * stride,), 99, dtype=torch.uint8, device=DEV)
            wide = torch.as_strided(big, (3, nb), (stride, 1))
            wide.copy_(dev)
            assert np.array_equal(_to_rgb(wide, h, w, mode), ref), (mode, stride)
        buf = torch.zeros(3 * nb + 1, dtype=torch.uint8, device=DEV)       # src offset by one byte: the unaligned path
        buf[1:] = dev.reshape(-1)
        assert np.array_equal(_to_rgb(buf[1:].view(3, nb), h, w, mode), ref), mode


@pytest.mark.parametrize("h, w", SIZES)
def test_rgb_to_yuv_kernel(h, w):
    rng = np.random.default_rng(h * 20011 + w)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8), np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)]
    for mode in MODES:
        nb = R.frame_bytes(h, w, mode[0])
        for k, f in enumerate(frames):
            ref = R.rgb_to_yuv(f, *mode)
            dev = torch.from_numpy(f).to(DEV)
            got = ops.rgb_u8_to_yuv(dev, *mode)
            assert got.dtype == torch.uint8 and got.shape == (nb,)
            assert np.array_equal(got.cpu().numpy(), ref), (mode, k)
        # `out=`, and a source and a destination that are not 4-byte aligned: the byte paths
        f = frames[0]
        ref = R.rgb_to_yuv(f, *mode)
        src = torch.zeros(f.size + 1, dtype=torch.uint8, device=DEV)
        src[1:] = torch.from_numpy(f).to(DEV).reshape(-1)
        dst = torch.full((nb + 2,), 99, dtype=torch.uint8, device=DEV)
        assert ops.rgb_u8_to_yuv(src[1:].view(h, w, 3), *mode, out=dst[1:nb + 1]).data_ptr() == dst.data_ptr() + 1
        host = dst.cpu().numpy()
        assert np.array_equal(host[1:nb + 1], ref) and host[0] == 99 and host[-1] == 99, mode      # and nothing beyond the frame


def test_kernels_large():
    """723x1283: more groups of 4 pixels than the launch has threads, so the grid-stride loop runs more than once per thread; odd on
    both axes.  One case per kernel."""
    h, w = 723, 1283
    assert h * ((w + 3) // 4) > 512 * 256                             # BLOCKS_MAX blocks of 256 threads (csrc/yuv_io.hip)
    rng = np.random.default_rng(11)
    mode = (R.CENTER, R.BT709, R.LIMITED)
    planar = rng.integers(0, 256, R.frame_bytes(h, w, mode[0]), dtype=np.uint8)
    assert np.array_equal(_to_rgb(torch.from_numpy(planar).to(DEV), h, w, mode)[0], R.yuv_to_rgb(planar, h, w, *mode))
    mode = (R.LEFT, R.BT601, R.FULL)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    assert np.array_equal(ops.rgb_u8_to_yuv(torch.from_numpy(rgb).to(DEV), *mode).cpu().numpy(), R.rgb_to_yuv(rgb, *mode))


def test_bad_arguments():
    lib = _lib.lib()
    h, w = 20, 24
    nb = R.frame_bytes(h, w, R.CENTER)
    planar = torch.zeros(2, nb, dtype=torch.uint8, device=DEV)
    rgb = torch.zeros(2, h, w, 3, dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    pp, rp = planar.data_ptr(), rgb.data_ptr()

    def to_rgb(src=pp, stride=nb, dst=rp, n=2, h=h, w=w, layout=R.CENTER, matrix=R.BT601, rng=R.FULL):
        return lib.spei_yuv_to_rgb_u8(C.c_void_p(src), stride, C.c_void_p(dst), n, h, w, layout, matrix, rng, st)

    def to_yuv(src=rp, dst=pp, h=h, w=w, layout=R.CENTER, matrix=R.BT601, rng=R.FULL):
        return lib.spei_rgb_u8_to_yuv(C.c_void_p(src), C.c_void_p(dst), h, w, layout, matrix, rng, st)

    assert to_rgb() == 0 and to_yuv() == 0 and to_rgb(n=1, stride=0) == 0
    for fn, name in ((to_rgb, "spei_yuv_to_rgb_u8"), (to_yuv, "spei_rgb_u8_to_yuv")):
        for kw, text in (({"src": None}, "null pointer"), ({"dst": None}, "null pointer"), ({"h": 0}, "bad frame shape"),
                         ({"w": -1}, "bad frame shape"), ({"h": 30000, "w": 30000}, "bad frame shape"), ({"layout": 3}, "unknown layout"),
                         ({"layout": -1}, "unknown layout"), ({"matrix": 2}, "unknown layout"), ({"rng": 2}, "unknown layout")):
            assert fn(**kw) != 0, (name, kw)
            msg = lib.spei_last_error().decode()
            assert text in msg and name in msg, (name, kw, msg)
    for kw, text in (({"stride": nb - 1}, "frame stride"), ({"stride": nb, "layout": R.P444}, "frame stride"), ({"n": 0}, "bad frame shape")):
        assert to_rgb(**kw) != 0, kw
        assert text in lib.spei_last_error().decode(), (kw, lib.spei_last_error().decode())
    with pytest.raises(RuntimeError, match="spei_yuv_to_rgb_u8 failed"):
        ops.yuv_to_rgb_u8(planar, h, w, R.CENTER, 5, R.FULL)


# ---- 2. the clip loop ---------------------------------------------------------------------------------------------------------------------
def _clip(T, h, w, seed=3):
    """uint8 [T,h,w,3]: the synthetic frames, shifted a little per frame (tests/test_gpu_video.py::_clip)."""
    x = synth_frames(1, h, w, seed=seed)[0]
    return np.stack([(torch.roll(x[i % 5], shifts=(i, -2 * i), dims=(1, 2)).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
                     for i in range(T)])


def _write_y4m(path, clip, layout, rng, matrix, fps=(30000, 1001), aspect=(1, 1)):
    with y4m.Y4MWriter(path, clip.shape[2], clip.shape[1], fps, layout, rng, aspect) as wr:
        for f in clip:
            wr.write(R.rgb_to_yuv(f, layout, matrix, rng))
    return str(path)


def _frames(run):
    out = {i: t.cpu().numpy() for i, t in run}
    assert sorted(out) == list(range(len(out)))
    return [out[i] for i in range(len(out))]


@pytest.fixture(scope="module")
def net16():
    return video.load_model("synthetic", DEV, "f16")


@pytest.mark.parametrize("h, w, layout, rng", [(40, 60, R.CENTER, R.LIMITED), (37, 53, R.LEFT, R.FULL)])
def test_clip_from_y4m_equals_clip_from_its_rgb(net16, tmp_path, h, w, layout, rng, monkeypatch):
    T = 5
    path = _write_y4m(tmp_path / "clip.y4m", _clip(T, h, w), layout, rng, R.BT601)
    reader = y4m.Y4MReader(path)
    assert (len(reader), reader.matrix, reader.range, reader.layout) == (T, R.BT601, rng, layout)
    planar = torch.from_numpy(np.stack([reader.raw(i) for i in range(T)])).to(DEV)
    rgb = ops.yuv_to_rgb_u8(planar, h, w, layout, R.BT601, rng).cpu().numpy()
    assert np.array_equal(rgb[2], R.yuv_to_rgb(reader.raw(2), h, w, layout, R.BT601, rng))
    # no labels, cuts="auto": the analysis pass runs on the y4m clip
    passes = []
    batches = detector.clip_batches
    monkeypatch.setattr(detector, "clip_batches", lambda *a, **k: passes.append(1) or batches(*a, **k))
    a, b = video.deblur_clip(net16, reader, cuts="auto"), video.deblur_clip(net16, rgb, cuts="auto")
    assert np.array_equal(a.labels, b.labels) and a.cuts == b.cuts and len(passes) == 2
    assert (a.frames.H, a.frames.W) == (h, w)
    fa, fb = _frames(a), _frames(b)
    assert len(fa) == T and all(x.shape == (h, w, 3) and np.array_equal(x, y) for x, y in zip(fa, fb))
    sad, hist = video.scene_stats(reader, DEV)
    ref_sad, ref_hist = video.scene_stats(rgb, DEV)
    assert np.array_equal(sad, ref_sad) and np.array_equal(hist, ref_hist)
    # given labels, crop=True: cropped on the device after the conversion; the path of a .y4m file opens it
    labels = [1, 0, 0, 0, 1]
    a, b = video.deblur_clip(net16, path, labels, crop=True), video.deblur_clip(net16, rgb, labels, crop=True)
    hc, wc = h - h % 20, w - w % 20
    assert (a.frames.H, a.frames.W) == (hc, wc)
    fa, fb = _frames(a), _frames(b)
    assert all(x.shape == (hc, wc, 3) and np.array_equal(x, y) for x, y in zip(fa, fb))
    assert not a.recomputed and not b.recomputed


def test_yuv_overrides(net16, tmp_path):
    h, w = 20, 24
    path = _write_y4m(tmp_path / "clip.y4m", _clip(3, h, w), R.CENTER, R.LIMITED, R.BT601)
    fr = video.frames_of(y4m.Y4MReader(path))
    assert fr.yuv == (R.CENTER, R.BT601, R.LIMITED) and fr.host(1).shape == (R.frame_bytes(h, w, R.CENTER),)
    run = video.deblur_clip(net16, path, [1, 0, 1], yuv=dict(matrix="bt709", range="full"))
    assert run.frames.yuv == (R.CENTER, R.BT709, R.FULL)
    planar = torch.from_numpy(run.frames.host(1)).to(DEV)[None]
    assert np.array_equal(run.frames.rgb(planar).cpu().numpy()[0], R.yuv_to_rgb(run.frames.host(1), h, w, R.CENTER, R.BT709, R.FULL))
    for bad in (dict(matrix="bt2020"), dict(layout=2)):
        with pytest.raises(ValueError):
            video.deblur_clip(net16, path, [1, 0, 1], yuv=bad)
    with pytest.raises(ValueError, match="y4m clips only"):
        video.deblur_clip(net16, _clip(3, h, w), [1, 0, 1], yuv=dict(matrix="bt709"))


# ---- 3. command line ----------------------------------------------------------------------------------------------------------------------
def _records(data: bytes, nb: int):
    """(header line, [payload bytes]) of a y4m stream whose FRAME lines are bare."""
    end = data.index(b"\n") + 1
    body = data[end:]
    assert len(body) % (6 + nb) == 0
    recs = [body[i:i + 6 + nb] for i in range(0, len(body), 6 + nb)]
    assert all(r[:6] == b"FRAME\n" for r in recs)
    return data[:end], [np.frombuffer(r[6:], dtype=np.uint8) for r in recs]


def test_cli_y4m(tmp_path):
    T, h, w = 5, 37, 53
    layout, rng, matrix = R.LEFT, R.FULL, R.BT601
    path = _write_y4m(tmp_path / "clip.y4m", _clip(T, h, w), layout, rng, matrix)
    labels = np.asarray([1, 0, 0, 0, 1])
    np.save(tmp_path / "labels.npy", labels)
    net32 = video.load_model("synthetic", DEV, "f32")
    ref = _frames(video.deblur_clip(net32, path, labels))
    nb = R.frame_bytes(h, w, layout)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "speinet_amd.video", "--model_path", "synthetic", "--labels", str(tmp_path / "labels.npy"),
            "--precision", "f32", "--device", DEV]

    # y4m in -> y4m out: the input's header fields, T frames, each the conversion of the frame deblur_clip yields
    out = tmp_path / "out.y4m"
    r = subprocess.run(base + ["--input", path, "--output", str(out)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sum(ln.startswith("> 00000") for ln in r.stdout.splitlines()) == T
    with y4m.Y4MReader(out) as got:
        assert (got.width, got.height, got.fps, got.aspect, got.layout, got.range, len(got)) == (w, h, (30000, 1001), (1, 1), layout, rng, T)
        for i in range(T):
            assert np.array_equal(got.raw(i), R.rgb_to_yuv(ref[i], layout, matrix, rng)), i
    file_bytes = out.read_bytes()

    # y4m in -> directory: the same frames as PNGs, 000000.png ...
    dst = tmp_path / "png"
    r = subprocess.run(base + ["--input", path, "--output", str(dst)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(dst)) == [f"{i:06d}.png" for i in range(T)]
    for i in range(T):
        assert np.array_equal(video._imread(str(dst / f"{i:06d}.png")), ref[i]), i

    # stdin -> stdout: the same bytes as from the path; every log line on stderr
    spool = tmp_path / "spool"
    spool.mkdir()
    with open(path, "rb") as f:
        r = subprocess.run(base + ["--input", "-", "--output", "-", "--spool_dir", str(spool)], cwd=ROOT, env=env, stdin=f,
                           capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == file_bytes
    assert sum(ln.startswith("> 00000") for ln in r.stderr.decode().splitlines()) == T and os.listdir(spool) == []
    head, payloads = _records(r.stdout, nb)
    assert head == b"YUV4MPEG2 W53 H37 F30000:1001 Ip A1:1 C420mpeg2 XCOLORRANGE=FULL\n" and len(payloads) == T


def test_cli_images_to_y4m(tmp_path):
    """Image input, y4m output: 25:1, C420jpeg and full range unless told otherwise; --matrix / --range reach the conversion."""
    from PIL import Image
    T, h, w = 3, 20, 24
    clip = _clip(T, h, w)
    src = tmp_path / "in"
    src.mkdir()
    for i in range(T):
        Image.fromarray(clip[i]).save(src / f"f{i}.png")
    np.save(tmp_path / "labels.npy", np.asarray([1, 0, 1]))
    net32 = video.load_model("synthetic", DEV, "f32")
    ref = _frames(video.deblur_clip(net32, clip, [1, 0, 1]))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = tmp_path / "out.y4m"
    r = subprocess.run([sys.executable, "-m", "speinet_amd.video", "--model_path", "synthetic", "--labels", str(tmp_path / "labels.npy"),
                        "--precision", "f32", "--device", DEV, "--input", str(src), "--output", str(out), "--matrix", "bt709",
                        "--fps", "24:1"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    with y4m.Y4MReader(out) as got:
        assert (got.width, got.height, got.fps, got.layout, got.range, len(got)) == (w, h, (24, 1), R.CENTER, R.FULL, T)
        for i in range(T):
            assert np.array_equal(got.raw(i), R.rgb_to_yuv(ref[i], R.CENTER, R.BT709, R.FULL)), i
