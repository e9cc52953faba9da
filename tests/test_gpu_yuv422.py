"""GPU suite for 4:2:2 and mono clips: the four planar entry points (csrc/yuv_io.hip: the LAYOUT values SPEI_YUV_422 and SPEI_YUV_MONO
of the YUV kernel templates) bit for bit against the numpy restatement of their definition (tests/yuv422_ref.py) at 8, 10 and 12
bits; against the existing entry points on the frames where the definitions coincide; their argument checks; `deblur_clip` on
`C422`, `C422p10` and `Cmono` files against `deblur_clip` on the RGB frames the reference makes of them; and the command line's
4:2:2 input and output, `--out_chroma` and `--chroma mono`.

uint16 tensors are built on the host and compared there: the device side only views, slices and copies them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import yuv422_ref as R                                             # noqa: E402
from speinet_amd import _lib, ops, video, y4m                      # noqa: E402
from speinet_amd.synth import synth_frames                         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LAYOUTS = (R.P422, R.MONO)
MODES = [(lay, m, r) for lay in LAYOUTS for m in (R.BT601, R.BT709) for r in (R.FULL, R.LIMITED)]
# (h, w).  1x1 and 3x5: every neighbour clamped; 20x24: aligned rows, chroma rows of 12 samples; 21x23: odd on both axes, a partial
# last chroma column, unaligned rows; 37x53: the same over more than one block; 64x40: W % 8 == 0, the widest access paths (chroma
# stores of 4 samples)
SIZES = [(1, 1), (3, 5), (20, 24), (21, 23), (37, 53), (64, 40)]
CASES = [(d, h, w) for d in R.DEPTHS for h, w in SIZES]


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy()


def _to_rgb(planar, h, w, layout, matrix, rng, depth, out=None):
    if depth == 8:
        return ops.yuv_to_rgb_u8(planar, h, w, layout, matrix, rng, out=out)
    return ops.yuv_to_rgb_u16(planar, h, w, layout, matrix, rng, depth, out=out)


def _to_yuv(rgb, layout, matrix, rng, depth, out=None):
    if depth == 8:
        return ops.rgb_u8_to_yuv(rgb, layout, matrix, rng, out=out)
    return ops.rgb_u16_to_yuv(rgb, layout, matrix, rng, depth, out=out)


def _kinds(rng, shape, depth):
    """Frames of one shape: random samples, all 0, all D, and random full words (deep frames: above D, read as D)."""
    D, dt = (1 << depth) - 1, R.dtype_of(depth)
    return np.stack([rng.integers(0, D + 1, shape).astype(dt), np.zeros(shape, dt), np.full(shape, D, dt),
                     rng.integers(0, 256 if depth == 8 else 65536, shape).astype(dt)])


def _strided(frames: np.ndarray, stride: int, fill=99):
    """[N, ns] frames `stride` samples apart in one device buffer (the gaps hold `fill`): the strided device view."""
    n, ns = frames.shape
    big = np.full(n * stride, fill, frames.dtype)
    for i in range(n):
        big[i * stride:i * stride + ns] = frames[i]
    return torch.as_strided(_dev(big), (n, ns), (stride, 1))


# ---- 1. the kernels against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth, h, w", CASES)
def test_planar_to_rgb_kernel(depth, h, w):
    rng = np.random.default_rng(depth * 100003 + h * 10007 + w)
    dt, tdt = R.dtype_of(depth), torch.uint8 if depth == 8 else torch.uint16
    for mode in MODES:
        ns = R.frame_samples(h, w, mode[0])
        assert ops.yuv_frame_bytes(h, w, mode[0]) == ns
        fr = _kinds(rng, ns, depth)
        ref = np.stack([R.yuv_to_rgb(f, h, w, *mode, depth) for f in fr])
        dev = _dev(fr)
        got = _to_rgb(dev, h, w, *mode, depth)                              # N = 4, packed
        assert got.dtype == tdt and got.shape == (4, h, w, 3)
        assert np.array_equal(_host(got), ref), mode
        assert np.array_equal(_host(_to_rgb(dev[0], h, w, *mode, depth)), ref[:1]), mode                 # one frame, [frame samples]
        # out=: nothing written beyond the frames
        buf = _dev(np.full(4 * h * w * 3 + 2, 99, dt))
        out = buf[1:-1].view(4, h, w, 3)
        assert _to_rgb(dev, h, w, *mode, depth, out=out) is out
        host = _host(buf)
        assert np.array_equal(host[1:-1].reshape(4, h, w, 3), ref) and host[0] == 99 and host[-1] == 99, mode
        # N = 3 with a frame stride larger than a frame: a multiple of 4 bytes (8 for u16), and not
        even = ns + 4 + (-ns % 4)
        for stride in (even, even + 1):
            assert np.array_equal(_host(_to_rgb(_strided(fr[:3], stride), h, w, *mode, depth)), ref[:3]), (mode, stride)
        assert np.array_equal(_host(_to_rgb(_dev(fr[:3]), h, w, *mode, depth)), ref[:3]), mode           # N = 3 packed
        # a source offset by one element: the unaligned path
        off = _dev(np.concatenate([np.zeros(1, dt), fr.reshape(-1)]))
        assert np.array_equal(_host(_to_rgb(off[1:].view(4, ns), h, w, *mode, depth)), ref), mode


@pytest.mark.parametrize("depth, h, w", CASES)
def test_rgb_to_planar_kernel(depth, h, w):
    rng = np.random.default_rng(depth * 200003 + h * 20011 + w)
    dt, tdt = R.dtype_of(depth), torch.uint8 if depth == 8 else torch.uint16
    frames = _kinds(rng, (h, w, 3), depth)
    for mode in MODES:
        ns = R.frame_samples(h, w, mode[0])
        refs = [R.rgb_to_yuv(f, *mode, depth) for f in frames]
        for k, f in enumerate(frames):
            got = _to_yuv(_dev(f), *mode, depth)
            assert got.dtype == tdt and got.shape == (ns,)
            assert np.array_equal(_host(got), refs[k]), (mode, k)
        # `out=`, and a source and a destination offset by one element: the element paths; nothing written beyond the frame
        for k in (0, 3):
            src = _dev(np.concatenate([np.zeros(1, dt), frames[k].reshape(-1)]))
            dst = _dev(np.full(ns + 2, 99, dt))
            got = _to_yuv(src[1:].view(h, w, 3), *mode, depth, out=dst[1:ns + 1])
            assert got.data_ptr() == dst.data_ptr() + dst.element_size()
            host = _host(dst)
            assert np.array_equal(host[1:ns + 1], refs[k]) and host[0] == 99 and host[-1] == 99, mode
        # an aligned `out=` with guards on both sides
        dst = _dev(np.full(ns + 16, 99, dt))
        _to_yuv(_dev(frames[0]), *mode, depth, out=dst[8:ns + 8])
        host = _host(dst)
        assert np.array_equal(host[8:ns + 8], refs[0]) and (host[:8] == 99).all() and (host[ns + 8:] == 99).all(), mode


def test_kernels_large_422():
    """723x1283: more groups of 4 pixels than the launch has threads, so the grid-stride loop runs more than once per thread; odd on
    both axes.  One case per direction: 8 bits in, 12-bit limited range (the 64-bit sums) out of the planar frame."""
    h, w = 723, 1283
    assert h * ((w + 3) // 4) > 512 * 256                             # BLOCKS_MAX blocks of 256 threads (csrc/yuv_io.hip)
    rng = np.random.default_rng(12)
    mode = (R.P422, R.BT709, R.LIMITED)
    planar = rng.integers(0, 4096, R.frame_samples(h, w, R.P422)).astype(np.uint16)
    assert np.array_equal(_host(ops.yuv_to_rgb_u16(_dev(planar), h, w, *mode, 12))[0], R.yuv_to_rgb(planar, h, w, *mode, 12))
    mode = (R.P422, R.BT601, R.LIMITED)
    rgb = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    assert np.array_equal(_host(ops.rgb_u8_to_yuv(_dev(rgb), *mode)), R.rgb_to_yuv(rgb, *mode))


# ---- 2. new entry against existing entry ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", R.DEPTHS)
def test_identities_on_the_device(depth):
    D, s, dt = (1 << depth) - 1, depth - 8, R.dtype_of(depth)
    rng = np.random.default_rng(depth)
    for h, w in ((3, 5), (21, 23), (64, 40)):
        cw = (w + 1) // 2
        for m, r in [(m, r) for m in (R.BT601, R.BT709) for r in (R.FULL, R.LIMITED)]:
            # 1. every row one colour: the chroma planes are the even columns of the 4:4:4 planes, the RGB made back is 4:4:4's
            rows = _dev(np.repeat(rng.integers(0, D + 1, (h, 1, 3)).astype(dt), w, axis=1))
            p422, p444 = _to_yuv(rows, R.P422, m, r, depth), _to_yuv(rows, R.P444, m, r, depth)
            a, b = _host(p422), _host(p444)
            assert np.array_equal(a[:h * w], b[:h * w])
            assert np.array_equal(a[h * w:].reshape(2, h, cw), b[h * w:].reshape(2, h, w)[:, :, ::2])
            assert np.array_equal(_host(_to_rgb(p422, h, w, R.P422, m, r, depth)), _host(_to_rgb(p444, h, w, R.P444, m, r, depth)))
            # 2. all rows equal: the even chroma rows are LEFT's planes, the RGB made back is LEFT's
            cols = _dev(np.repeat(rng.integers(0, D + 1, (1, w, 3)).astype(dt), h, axis=0))
            p422, pleft = _to_yuv(cols, R.P422, m, r, depth), _to_yuv(cols, R.LEFT, m, r, depth)
            a, b = _host(p422), _host(pleft)
            assert np.array_equal(a[:h * w], b[:h * w])
            assert np.array_equal(a[h * w:].reshape(2, h, cw)[:, ::2], b[h * w:].reshape(2, (h + 1) // 2, cw))
            assert np.array_equal(_host(_to_rgb(p422, h, w, R.P422, m, r, depth)), _host(_to_rgb(pleft, h, w, R.LEFT, m, r, depth)))
            # 5. mono in is 4:4:4 in with the chroma planes at the chroma zero; mono out is the Y plane of 4:4:4 out
            yp = rng.integers(0, D + 1, h * w).astype(dt)
            as444 = _dev(np.concatenate([yp, np.full(2 * h * w, 128 << s, dt)]))
            assert np.array_equal(_host(_to_rgb(_dev(yp), h, w, R.MONO, m, r, depth)), _host(_to_rgb(as444, h, w, R.P444, m, r, depth)))
            rgb = _dev(rng.integers(0, D + 1, (h, w, 3)).astype(dt))
            assert np.array_equal(_host(_to_yuv(rgb, R.MONO, m, r, depth)), _host(_to_yuv(rgb, R.P444, m, r, depth))[:h * w])


# ---- 3. argument checks -------------------------------------------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments():
    lib = _lib.lib()
    h, w = 20, 24
    ns = R.frame_samples(h, w, R.P422)
    planar = torch.zeros(2 * 2 * ns + 8, dtype=torch.uint8, device=DEV)
    rgb = torch.zeros(2 * 2 * h * w * 3 + 8, dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    pp, rp = planar.data_ptr(), rgb.data_ptr()

    def to_rgb8(src=pp, stride=ns, dst=rp, n=2, h=h, w=w, layout=R.P422, matrix=R.BT601, rng=R.FULL):
        return lib.spei_planar_to_rgb_u8(C.c_void_p(src), stride, C.c_void_p(dst), n, h, w, layout, matrix, rng, st)

    def to_yuv8(src=rp, dst=pp, h=h, w=w, layout=R.P422, matrix=R.BT601, rng=R.FULL):
        return lib.spei_rgb_u8_to_planar(C.c_void_p(src), C.c_void_p(dst), h, w, layout, matrix, rng, st)

    def to_rgb16(src=pp, stride=2 * ns, dst=rp, n=2, h=h, w=w, layout=R.P422, matrix=R.BT601, rng=R.FULL, depth=10):
        return lib.spei_planar_to_rgb_u16(C.c_void_p(src), stride, C.c_void_p(dst), n, h, w, layout, matrix, rng, depth, st)

    def to_yuv16(src=rp, dst=pp, h=h, w=w, layout=R.P422, matrix=R.BT601, rng=R.FULL, depth=10):
        return lib.spei_rgb_u16_to_planar(C.c_void_p(src), C.c_void_p(dst), h, w, layout, matrix, rng, depth, st)

    assert to_rgb8() == 0 and to_yuv8() == 0 and to_rgb16() == 0 and to_yuv16() == 0
    assert to_rgb8(layout=R.MONO, stride=h * w) == 0 and to_yuv8(layout=R.MONO) == 0 and to_rgb16(layout=R.MONO, stride=2 * h * w) == 0
    assert to_yuv16(layout=R.MONO, depth=12) == 0 and to_rgb8(n=1, stride=0) == 0 and to_rgb16(n=1, stride=1, depth=12) == 0
    common = [({"src": None}, "null pointer"), ({"dst": None}, "null pointer"), ({"h": 0}, "bad frame shape"), ({"w": -1}, "bad frame shape"),
              ({"h": 30000, "w": 30000}, "bad frame shape")]
    common += [({"layout": lay}, "unknown layout") for lay in (R.CENTER, R.LEFT, R.P444, 5, -1)]
    common += [({"matrix": 2}, "unknown layout"), ({"rng": 2}, "unknown layout"), ({"matrix": -1}, "unknown layout")]
    depths = [({"depth": 8}, "unknown depth"), ({"depth": 16}, "unknown depth"), ({"depth": 0}, "unknown depth")]
    cases = {
        "spei_planar_to_rgb_u8": (to_rgb8, common + [({"n": 0}, "bad frame shape"), ({"stride": ns - 1}, "frame stride"),
                                                     ({"stride": h * w, "layout": R.P422}, "frame stride"),
                                                     ({"stride": h * w - 1, "layout": R.MONO}, "frame stride")]),
        "spei_rgb_u8_to_planar": (to_yuv8, common),
        "spei_planar_to_rgb_u16": (to_rgb16, common + depths + [({"n": 0}, "bad frame shape"), ({"stride": 2 * ns - 2}, "frame stride"),
                                                                ({"stride": ns}, "frame stride"), ({"stride": 2 * ns + 1}, "odd frame stride"),
                                                                ({"stride": 2 * h * w - 2, "layout": R.MONO}, "frame stride"),
                                                                ({"src": pp + 1}, "2-byte aligned"), ({"dst": rp + 1}, "2-byte aligned")]),
        "spei_rgb_u16_to_planar": (to_yuv16, common + depths + [({"src": rp + 1}, "2-byte aligned"), ({"dst": pp + 1}, "2-byte aligned")]),
    }
    for name, (fn, bad) in cases.items():
        for kw, text in bad:
            assert fn(**kw) != 0, (name, kw)
            msg = lib.spei_last_error().decode()
            assert text in msg and name in msg, (name, kw, msg)
    # ops hands each layout to its entry, and reports that entry's failure
    with pytest.raises(RuntimeError, match="spei_planar_to_rgb_u8 failed"):
        ops.yuv_to_rgb_u8(planar[:2 * ns].view(2, ns), h, w, R.P422, 5, R.FULL)
    with pytest.raises(RuntimeError, match="spei_rgb_u16_to_planar failed"):
        ops.rgb_u16_to_yuv(rgb[:2 * h * w * 3].view(torch.uint16).view(h, w, 3), R.MONO, R.BT601, 7, 10)
    # the existing entries keep refusing the two layouts
    for lay in LAYOUTS:
        assert lib.spei_yuv_to_rgb_u8(C.c_void_p(pp), 2 * ns, C.c_void_p(rp), 2, h, w, lay, R.BT601, R.FULL, st) != 0
        assert "unknown layout" in lib.spei_last_error().decode() and "spei_yuv_to_rgb_u8" in lib.spei_last_error().decode()
        assert lib.spei_rgb_u16_to_yuv(C.c_void_p(rp), C.c_void_p(pp), h, w, lay, R.BT601, R.FULL, 10, st) != 0
        assert "unknown layout" in lib.spei_last_error().decode()


# ---- 4. the clip loop ---------------------------------------------------------------------------------------------------------------------
def _clip(T, h, w, depth, seed=3):
    """[T,h,w,3] of `depth` bits: the synthetic frames, shifted a little per frame (tests/test_gpu_yuv16.py::_clip)."""
    D = (1 << depth) - 1
    x = synth_frames(1, h, w, seed=seed)[0]
    return np.stack([(torch.roll(x[i % 5], shifts=(i, -2 * i), dims=(1, 2)).permute(1, 2, 0).numpy().astype(np.float64) * D).round()
                     .clip(0, D).astype(R.dtype_of(depth)) for i in range(T)])


def _write_y4m(path, clip, layout, rng, matrix, depth, fps=(30000, 1001), aspect=(1, 1)):
    with y4m.Y4MWriter(path, clip.shape[2], clip.shape[1], fps, layout, rng, aspect, depth=depth) as wr:
        for f in clip:
            wr.write(R.rgb_to_yuv(f, layout, matrix, rng, depth).astype("u1" if depth == 8 else "<u2"))
    return str(path)


def _frames(run):
    out = {i: t.cpu().numpy() for i, t in run}
    assert sorted(out) == list(range(len(out)))
    return [out[i] for i in range(len(out))]


@pytest.fixture(scope="module")
def net32():
    return video.load_model("synthetic", DEV, "f32", False)


def _reference_rgb(path, h, w, layout, matrix, rng, depth):
    """The RGB frames the reference makes of the file's frames."""
    with y4m.Y4MReader(path, depths=y4m.DEPTHS, layouts=y4m.LAYOUTS) as reader:
        assert (reader.layout, reader.depth, reader.matrix, reader.range, reader.chroma) == (layout, depth, matrix, rng, y4m.chroma_tag(layout, depth))
        raws = [reader.raw(i) for i in range(len(reader))]
    return np.stack([R.yuv_to_rgb(p if depth == 8 else p.view("<u2"), h, w, layout, matrix, rng, depth) for p in raws])


CLIPS = [(4, 40, 60, R.P422, 8, R.LIMITED), (4, 40, 60, R.P422, 10, R.LIMITED), (4, 40, 60, R.MONO, 8, R.FULL), (3, 41, 63, R.P422, 8, R.FULL)]


@pytest.mark.parametrize("T, h, w, layout, depth, rng", CLIPS)
def test_clip_from_file_equals_clip_from_its_rgb(net32, tmp_path, T, h, w, layout, depth, rng):
    path = _write_y4m(tmp_path / "clip.y4m", _clip(T, h, w, depth), layout, rng, R.BT601, depth)
    rgb = _reference_rgb(path, h, w, layout, R.BT601, rng, depth)
    assert rgb.shape == (T, h, w, 3) and rgb.dtype == R.dtype_of(depth)
    if layout == R.MONO:
        assert np.array_equal(rgb[..., 0], rgb[..., 1]) and np.array_equal(rgb[..., 0], rgb[..., 2])
    labels = [1, 0, 0, 1][:T - 1] + [1]
    a = video.deblur_clip(net32, path, labels)                                      # the path opens the file
    b = video.deblur_clip(net32, rgb, labels, depth=None if depth == 8 else depth)
    assert (a.depth, a.out_depth, a.frames.yuv, a.frames.H, a.frames.W) == (depth, depth, (layout, R.BT601, rng), h, w)
    fa, fb = _frames(a), _frames(b)
    assert len(fa) == T and all(x.shape == (h, w, 3) and x.dtype == R.dtype_of(depth) and np.array_equal(x, y) for x, y in zip(fa, fb))
    assert a.plan == b.plan and not a.recomputed and not b.recomputed
    assert len({v.tobytes() for v in fa}) == T                                       # the frames differ: something was computed
    # a reader the caller opened with the layouts is accepted; one frame's conversion through `Frames.rgb`
    with y4m.Y4MReader(path, depths=y4m.DEPTHS, layouts=y4m.LAYOUTS) as reader:
        c = video.deblur_clip(net32, reader, labels)
        assert np.array_equal(_host(c.frames.rgb(_dev(np.stack([reader.raw(1)]))))[0], rgb[1])
        assert all(np.array_equal(x, y) for x, y in zip(fa, _frames(c)))


def test_clip_422p10_in_f16_with_graphs(tmp_path):
    T, h, w, depth, layout, rng = 4, 40, 60, 10, R.P422, R.LIMITED
    net16 = video.load_model("synthetic", DEV, "f16")
    assert net16.use_graph and net16.precision == "f16"
    path = _write_y4m(tmp_path / "clip.y4m", _clip(T, h, w, depth), layout, rng, R.BT601, depth)
    rgb = _reference_rgb(path, h, w, layout, R.BT601, rng, depth)
    labels = [1, 0, 0, 1]
    fa, fb = _frames(video.deblur_clip(net16, path, labels)), _frames(video.deblur_clip(net16, rgb, labels, depth=depth))
    assert len(fa) == T and all(x.dtype == np.uint16 and np.array_equal(x, y) for x, y in zip(fa, fb))
    assert max(int(x.max()) for x in fa) <= 1023 and len({int(v) & 3 for v in fa[1].reshape(-1)}) == 4      # 10 bits, all in use


# ---- 5. command line ----------------------------------------------------------------------------------------------------------------------
def _cli(tmp_path, T, *args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "speinet_amd.video", "--model_path", "synthetic", "--labels", str(tmp_path / "labels.npy"),
           "--precision", "f32", "--device", DEV] + list(args)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sum(ln.startswith("> ") for ln in r.stdout.splitlines()) == T
    return r.stdout


def test_cli_422p10_in_and_out(tmp_path):
    T, h, w, depth, layout, rng, matrix = 3, 21, 24, 10, R.P422, R.LIMITED, R.BT601
    path = _write_y4m(tmp_path / "clip.y4m", _clip(T, h, w, depth), layout, rng, matrix, depth)
    np.save(tmp_path / "labels.npy", np.asarray([1, 0, 1]))
    ref = _frames(video.deblur_clip(video.load_model("synthetic", DEV, "f32"), path, [1, 0, 1]))
    out = tmp_path / "out.y4m"
    # --chroma selects the siting of a deep 4:2:0 input only: a 4:2:2 input keeps its layout
    text = _cli(tmp_path, T, "--input", path, "--output", str(out), "--chroma", "420jpeg")
    assert "# y4m input C422p10" in text.splitlines() and "output C" not in text
    assert out.read_bytes().split(b"\n", 1)[0] == b"YUV4MPEG2 W24 H21 F30000:1001 Ip A1:1 C422p10 XYSCSS=422P10 XCOLORRANGE=LIMITED"
    with y4m.Y4MReader(out, depths=y4m.DEPTHS, layouts=y4m.LAYOUTS) as got:
        assert (got.width, got.height, got.fps, got.layout, got.depth, got.range, len(got)) == (w, h, (30000, 1001), layout, depth, rng, T)
        assert got.frame_bytes == 2 * R.frame_samples(h, w, layout)
        for i in range(T):
            assert ref[i].dtype == np.uint16
            assert np.array_equal(got.raw(i).view("<u2"), R.rgb_to_yuv(ref[i], layout, matrix, rng, depth)), i


def test_cli_out_chroma_444_from_420jpeg(tmp_path):
    T, h, w, rng, matrix = 3, 21, 24, R.FULL, R.BT601
    clip = _clip(T, h, w, 8)
    path = tmp_path / "clip.y4m"
    with y4m.Y4MWriter(path, w, h, (25, 1), y4m.CENTER, rng) as wr:
        for f in clip:
            wr.write(R.old_rgb_to_yuv(f, R.CENTER, matrix, rng))
    np.save(tmp_path / "labels.npy", np.asarray([1, 0, 1]))
    ref = _frames(video.deblur_clip(video.load_model("synthetic", DEV, "f32"), str(path), [1, 0, 1]))
    out = tmp_path / "out.y4m"
    text = _cli(tmp_path, T, "--input", str(path), "--output", str(out), "--out_chroma", "444")
    assert "# y4m input C420jpeg, output C444" in text.splitlines()
    with y4m.Y4MReader(out) as got:
        assert (got.chroma, got.layout, got.depth, got.range, len(got), got.frame_bytes) == ("444", y4m.P444, 8, rng, T, 3 * h * w)
        for i in range(T):
            assert np.array_equal(got.raw(i), R.old_rgb_to_yuv(ref[i], R.P444, matrix, rng)), i


def test_cli_chroma_mono_from_pngs(tmp_path):
    from PIL import Image
    T, h, w = 3, 20, 24
    clip = _clip(T, h, w, 8)
    src = tmp_path / "in"
    src.mkdir()
    for i in range(T):
        Image.fromarray(clip[i]).save(src / f"f{i}.png")
    np.save(tmp_path / "labels.npy", np.asarray([1, 0, 1]))
    ref = _frames(video.deblur_clip(video.load_model("synthetic", DEV, "f32"), clip, [1, 0, 1]))
    out = tmp_path / "out.y4m"
    text = _cli(tmp_path, T, "--input", str(src), "--output", str(out), "--chroma", "mono")
    assert "# y4m input" not in text
    assert out.read_bytes().split(b"\n", 1)[0] == b"YUV4MPEG2 W24 H20 F25:1 Ip Cmono XCOLORRANGE=FULL"
    with y4m.Y4MReader(out, layouts=y4m.LAYOUTS) as got:
        assert (got.layout, got.depth, len(got), got.frame_bytes) == (y4m.MONO, 8, T, h * w)
        for i in range(T):
            assert np.array_equal(got.raw(i), R.rgb_to_yuv(ref[i], R.MONO, R.BT601, R.FULL)), i
