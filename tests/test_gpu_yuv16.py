"""GPU suite for deep (10- and 12-bit) clips: the two 16-bit planar-YUV kernels (csrc/yuv_io.hip) bit for bit against the numpy
restatement of their definition (tests/yuv16_ref.py); the 16-bit ingest, egress and pair-statistics kernels (csrc/frame_io.hip)
against torch and numpy; the C-ABI's argument checks; `deblur_clip` on deep y4m clips against `deblur_clip` on the uint16 RGB
frames the kernel makes of them; and the command line's deep input and output.

uint16 tensors are built on the host and compared there: the device side only views, slices and copies them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import yuv16_ref as R                                              # noqa: E402
import yuv_ref as R8                                               # noqa: E402
from speinet_amd import _lib, detector, ops, video, y4m            # noqa: E402
from speinet_amd.synth import synth_frames, synth_scene_u8         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LAYOUTS = (R.CENTER, R.LEFT, R.P444)
MODES = [(lay, m, r) for lay in LAYOUTS for m in (R.BT601, R.BT709) for r in (R.FULL, R.LIMITED)]
# the smallest shapes of tests/test_gpu_yuv.py: 1x1 and 3x5: every neighbour clamped; 20x20: aligned rows; 21x23: odd on both axes
# (partial last chroma row and column, unaligned rows); 37x53: the same over more than one block
SIZES = [(1, 1), (3, 5), (20, 20), (21, 23), (37, 53)]
CASES = [(d, h, w) for d in R.DEPTHS for h, w in SIZES]


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy()


def _kinds(rng, shape, depth):
    """Frames of one shape: random samples, all 0, all D, and random full 16-bit words (above D: read as D)."""
    D = (1 << depth) - 1
    return np.stack([rng.integers(0, D + 1, shape).astype(np.uint16), np.zeros(shape, np.uint16), np.full(shape, D, np.uint16),
                     rng.integers(0, 65536, shape).astype(np.uint16)])


def _strided(frames: np.ndarray, stride: int, fill=99):
    """[N, ns] frames `stride` samples apart in one device buffer (the gaps hold `fill`): the strided device view."""
    n, ns = frames.shape
    big = np.full(n * stride, fill, np.uint16)
    for i in range(n):
        big[i * stride:i * stride + ns] = frames[i]
    return torch.as_strided(_dev(big), (n, ns), (stride, 1))


# ---- 1. the YUV kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth, h, w", CASES)
def test_yuv_to_rgb_u16_kernel(depth, h, w):
    rng = np.random.default_rng(depth * 100003 + h * 10007 + w)
    for mode in MODES:
        ns = R.frame_samples(h, w, mode[0])
        fr = _kinds(rng, ns, depth)
        ref = np.stack([R.yuv_to_rgb(f, h, w, *mode, depth) for f in fr])
        dev = _dev(fr)
        got = ops.yuv_to_rgb_u16(dev, h, w, *mode, depth)                   # N = 4, packed
        assert got.dtype == torch.uint16 and got.shape == (4, h, w, 3)
        assert np.array_equal(_host(got), ref), mode
        assert np.array_equal(_host(ops.yuv_to_rgb_u16(dev[0], h, w, *mode, depth)), ref[:1]), mode      # one frame, [frame samples]
        # out=: nothing written beyond the frames
        buf = _dev(np.full(4 * h * w * 3 + 2, 99, np.uint16))
        out = buf[1:-1].view(4, h, w, 3)
        assert ops.yuv_to_rgb_u16(dev, h, w, *mode, depth, out=out) is out
        host = _host(buf)
        assert np.array_equal(host[1:-1].reshape(4, h, w, 3), ref) and host[0] == 99 and host[-1] == 99, mode
        # N = 3 with a frame stride larger than a frame: a multiple of 8 bytes, and not
        even = ns + 4 + (-ns % 4)
        for stride in (even, even + 1):
            assert (2 * stride % 8 == 0) == (stride == even)
            assert np.array_equal(_host(ops.yuv_to_rgb_u16(_strided(fr[:3], stride), h, w, *mode, depth)), ref[:3]), (mode, stride)
        # a source offset by one sample: the unaligned path
        off = _dev(np.concatenate([np.zeros(1, np.uint16), fr.reshape(-1)]))
        assert np.array_equal(_host(ops.yuv_to_rgb_u16(off[1:].view(4, ns), h, w, *mode, depth)), ref), mode


@pytest.mark.parametrize("depth, h, w", CASES)
def test_rgb_u16_to_yuv_kernel(depth, h, w):
    rng = np.random.default_rng(depth * 200003 + h * 20011 + w)
    frames = _kinds(rng, (h, w, 3), depth)
    for mode in MODES:
        ns = R.frame_samples(h, w, mode[0])
        for k, f in enumerate(frames):
            ref = R.rgb_to_yuv(f, *mode, depth)
            got = ops.rgb_u16_to_yuv(_dev(f), *mode, depth)
            assert got.dtype == torch.uint16 and got.shape == (ns,)
            assert np.array_equal(_host(got), ref), (mode, k)
        # `out=`, and a source and a destination that are not 8-byte aligned: the element paths; nothing written beyond the frame
        for f in (frames[0], frames[3]):
            ref = R.rgb_to_yuv(f, *mode, depth)
            src = _dev(np.concatenate([np.zeros(1, np.uint16), f.reshape(-1)]))
            dst = _dev(np.full(ns + 2, 99, np.uint16))
            assert ops.rgb_u16_to_yuv(src[1:].view(h, w, 3), *mode, depth, out=dst[1:ns + 1]).data_ptr() == dst.data_ptr() + 2
            host = _host(dst)
            assert np.array_equal(host[1:ns + 1], ref) and host[0] == 99 and host[-1] == 99, mode


def test_kernels_large_u16():
    """723x1283: more groups of 4 pixels than the launch has threads, so the grid-stride loop runs more than once per thread; odd on
    both axes.  One case per kernel, 12-bit limited range (the 64-bit sums)."""
    h, w = 723, 1283
    assert h * ((w + 3) // 4) > 512 * 256                             # BLOCKS_MAX blocks of 256 threads (csrc/yuv_io.hip)
    rng = np.random.default_rng(11)
    mode = (R.CENTER, R.BT709, R.LIMITED)
    planar = rng.integers(0, 4096, R.frame_samples(h, w, mode[0])).astype(np.uint16)
    assert np.array_equal(_host(ops.yuv_to_rgb_u16(_dev(planar), h, w, *mode, 12))[0], R.yuv_to_rgb(planar, h, w, *mode, 12))
    mode = (R.LEFT, R.BT601, R.LIMITED)
    rgb = rng.integers(0, 4096, (h, w, 3)).astype(np.uint16)
    assert np.array_equal(_host(ops.rgb_u16_to_yuv(_dev(rgb), *mode, 12)), R.rgb_to_yuv(rgb, *mode, 12))


# ---- 2. the frame kernels -----------------------------------------------------------------------------------------------------------------
def _det_gray(rgb255: np.ndarray) -> np.ndarray:
    """spei_det_gray on fp32 frames [N,H,W,3] (0..255 scale)."""
    rgb = torch.from_numpy(rgb255).permute(0, 3, 1, 2).contiguous().to(DEV)
    n, _, h, w = rgb.shape
    g = torch.empty(n, h, w, device=DEV)
    _lib.check(_lib.lib().spei_det_gray(C.c_void_p(rgb.data_ptr()), C.c_void_p(g.data_ptr()), n, h, w,
                                        C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)), "spei_det_gray")
    return _host(g)


@pytest.mark.parametrize("depth", R.DEPTHS)
@pytest.mark.parametrize("h, w", [(20, 20), (21, 23), (37, 53)])
def test_frames_u16_in(depth, h, w):
    """Bit-identical to torch F.pad(reflect) of v.float() * float32(1 / D); the gray plane bit-identical to spei_det_gray on
    v.float() * float32(255 / D); v = min(word, D)."""
    D = (1 << depth) - 1
    rng = np.random.default_rng(depth * 31 + h * 7 + w)
    fr = _kinds(rng, (h, w, 3), depth)
    v = np.minimum(fr, D).astype(np.float32)
    hp, wp = ops.padded_size(h), ops.padded_size(w)
    planes = torch.from_numpy(v).permute(0, 3, 1, 2) * torch.tensor(np.float32(1.0 / D))
    ref = F.pad(planes, (0, wp - w, 0, hp - h), mode="reflect").numpy() if (hp, wp) != (h, w) else planes.numpy()
    gray = _det_gray(v * np.float32(255.0 / D))
    variants = [_dev(fr), _dev(np.concatenate([np.zeros(1, np.uint16), fr.reshape(-1)]))[1:].view(4, h, w, 3)]
    for stride in (h * w * 3 + 4 + (-(h * w * 3) % 4), h * w * 3 + 5 + (-(h * w * 3) % 4)):
        variants.append(_strided(fr.reshape(4, -1), stride).as_strided((4, h, w, 3), (stride, w * 3, 3, 1)))
    for dev in variants:
        p, g = ops.frames_u16_in(dev, depth, gray=True)
        assert p.shape == (4, 3, hp, wp) and p.dtype == torch.float32 and np.array_equal(_host(p), ref)
        assert g.shape == (4, h, w) and np.array_equal(_host(g), gray)
    p, g = ops.frames_u16_in(variants[0][1], depth)                             # one frame, planes only
    assert g is None and np.array_equal(_host(p), ref[1:2])
    p, g = ops.frames_u16_in(variants[0], depth, gray=True, planes=False)       # gray only
    assert p is None and np.array_equal(_host(g), gray)
    out = torch.zeros(4, 3, hp, wp, device=DEV)
    assert ops.frames_u16_in(variants[0], depth, out=out)[0] is out and np.array_equal(_host(out), ref)


@pytest.mark.parametrize("depth", R.DEPTHS)
@pytest.mark.parametrize("h, w, hp, wp", [(37, 53, 40, 60), (40, 60, 40, 60), (37, 53, 37, 53)])
def test_frame_u16_out(depth, h, w, hp, wp):
    """Equal to x.mul(D).clamp(0, D).round() (torch rounds half to even) on the crop; NaN and +-inf -> 0 with the flag set; the pad
    columns ignored."""
    D = (1 << depth) - 1
    rng = np.random.default_rng(depth * hp * wp)
    x = rng.uniform(-0.5, 1.5, (3, hp, wp)).astype(np.float32)
    n = min(D, x.size // 2)
    x.reshape(-1)[:2 * n:2] = ((np.arange(n) + 0.5) / D).astype(np.float32)        # candidates for ties
    x[0, 0, :4] = (0.0, 1.0, -0.0, 2.0)

    def ref_of(a):
        return torch.from_numpy(a)[:, :h, :w].mul(D).clamp(0, D).round().permute(1, 2, 0).numpy().astype(np.uint16)

    got = ops.frame_u16_out(_dev(x), h, w, depth)
    assert got.dtype == torch.uint16 and got.shape == (h, w, 3) and np.array_equal(_host(got), ref_of(x))
    buf = _dev(np.full(h * w * 3 + 2, 99, np.uint16))                              # out=, not 8-byte aligned: the element stores
    flag = _dev(np.full(1, 7, np.int32))                                           # cleared by the call
    out = buf[1:-1].view(h, w, 3)
    assert ops.frame_u16_out(_dev(x), h, w, depth, out=out, nonfinite=flag) is out
    host = _host(buf)
    assert np.array_equal(host[1:-1].reshape(h, w, 3), ref_of(x)) and host[0] == 99 and host[-1] == 99 and int(flag.item()) == 0
    if wp > w:                                                                     # a NaN in the pad columns is not part of the crop
        xp = x.copy()
        xp[1, h - 1, w] = np.nan
        assert np.array_equal(_host(ops.frame_u16_out(_dev(xp), h, w, depth, nonfinite=flag)), ref_of(x)) and int(flag.item()) == 0
    for nf in ([(0, 1, 2, np.nan)], [(2, h - 1, w - 1, np.inf)], [(0, 1, 2, np.nan), (1, 3, 4, np.inf), (2, 5, 6, -np.inf)]):
        xn = x.copy()
        for c_, y_, x_, val in nf:
            xn[c_, y_, x_] = val
        got = ops.frame_u16_out(_dev(xn), h, w, depth, nonfinite=flag)
        assert np.array_equal(_host(got), ref_of(np.where(np.isfinite(xn), xn, np.float32(0)))) and int(flag.item()) != 0
        for c_, y_, x_, val in nf:
            assert int(_host(got)[y_, x_, c_]) == 0
    # an unaligned fp32 source: the element loads
    xs = _dev(np.concatenate([np.zeros(1, np.float32), x.reshape(-1)]))[1:].view(3, hp, wp)
    assert np.array_equal(_host(ops.frame_u16_out(xs, h, w, depth)), ref_of(x))


def _pair_ref(fr, depth, prev=None):
    y = R.luma(fr, depth)
    hist = np.stack([np.bincount((f >> (depth - 6)).reshape(-1), minlength=64) for f in y])
    seq = y if prev is None else np.concatenate([R.luma(prev, depth)[None], y])
    return np.abs(np.diff(seq, axis=0)).sum(axis=(1, 2)), hist


@pytest.mark.parametrize("depth", R.DEPTHS)
@pytest.mark.parametrize("h, w", [(20, 20), (21, 23), (37, 53)])
def test_frame_pair_stats_u16(depth, h, w):
    rng = np.random.default_rng(depth + h * w)
    fr = np.concatenate([_kinds(rng, (h, w, 3), depth), _kinds(rng, (h, w, 3), depth)[:1]])        # 5 frames
    dev = _dev(fr)
    sad, hist = ops.frame_pair_stats_u16(dev, depth)
    ref_sad, ref_hist = _pair_ref(fr, depth)
    assert sad.dtype == torch.int64 and sad.shape == (4,) and hist.shape == (5, 64)
    assert np.array_equal(_host(sad), ref_sad) and np.array_equal(_host(hist), ref_hist) and (ref_hist.sum(axis=1) == h * w).all()
    # the `prev` carry: frames 2.. with frame 1 before them, and a single frame with prev
    sad, hist = ops.frame_pair_stats_u16(dev[2:], depth, prev=dev[1])
    assert np.array_equal(_host(sad), ref_sad[1:]) and np.array_equal(_host(hist), ref_hist[2:])
    sad, hist = ops.frame_pair_stats_u16(dev[4:5], depth, prev=dev[0])
    one_sad, one_hist = _pair_ref(fr[4:5], depth, prev=fr[0])
    assert np.array_equal(_host(sad), one_sad) and np.array_equal(_host(hist), one_hist)
    # a frame stride larger than a frame, not a multiple of 8 bytes, and frames offset by one sample: the element loads
    stride = h * w * 3 + 5 + (-(h * w * 3) % 4)
    wide = _strided(fr.reshape(5, -1), stride).as_strided((5, h, w, 3), (stride, w * 3, 3, 1))
    sad, hist = ops.frame_pair_stats_u16(wide, depth)
    assert np.array_equal(_host(sad), ref_sad) and np.array_equal(_host(hist), ref_hist)


def test_frame_pair_stats_u16_matches_u8_on_shifted_gray():
    """At d = 10, on 8-bit values shifted left by 2, the histogram equals the u8 kernel's and sad / 4 its sad.  The inputs are gray
    (R = G = B): the rounding term of Yd = (77 R + 150 G + 29 B + 128) >> 8 does not scale with the samples, so Yd(4 c) = 4 Y8(c)
    holds exactly where 77 R + 150 G + 29 B is a multiple of 256, which gray pixels are (77 + 150 + 29 = 256), and not for every
    colour."""
    h, w = 37, 53
    rng = np.random.default_rng(5)
    gray8 = np.repeat(rng.integers(0, 256, (4, h, w, 1), dtype=np.uint8), 3, axis=3)
    sad8, hist8 = ops.frame_pair_stats(_dev(gray8))
    sad10, hist10 = ops.frame_pair_stats_u16(_dev(gray8.astype(np.uint16) << 2), 10)
    assert np.array_equal(_host(hist10), _host(hist8))
    assert (_host(sad10) % 4 == 0).all() and np.array_equal(_host(sad10) // 4, _host(sad8)) and int(_host(sad8).min()) > 0


def test_bad_arguments_u16():
    lib = _lib.lib()
    h, w = 20, 24
    ns = R.frame_samples(h, w, R.CENTER)
    planar = torch.zeros(2, ns * 2, dtype=torch.uint8, device=DEV)
    rgb = torch.zeros(2, h, w, 3 * 2, dtype=torch.uint8, device=DEV)
    f32 = torch.zeros(2, 3, h, 40, device=DEV)
    gray = torch.zeros(2, h, w, device=DEV)
    hist = torch.zeros(2, 64, dtype=torch.int32, device=DEV)
    sad = torch.zeros(2, dtype=torch.int64, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    pp, rp, fp, gp, hp_, sp = (t.data_ptr() for t in (planar, rgb, f32, gray, hist, sad))
    nb, fb = 2 * ns, h * w * 6

    def to_rgb(src=pp, stride=nb, dst=rp, n=2, h=h, w=w, layout=R.CENTER, matrix=R.BT601, rng=R.FULL, depth=10):
        return lib.spei_yuv_to_rgb_u16(C.c_void_p(src), stride, C.c_void_p(dst), n, h, w, layout, matrix, rng, depth, st)

    def to_yuv(src=rp, dst=pp, h=h, w=w, layout=R.CENTER, matrix=R.BT601, rng=R.FULL, depth=10):
        return lib.spei_rgb_u16_to_yuv(C.c_void_p(src), C.c_void_p(dst), h, w, layout, matrix, rng, depth, st)

    def f_in(src=rp, stride=fb, dst=fp, gray=gp, n=2, h=h, w=w, depth=10):
        return lib.spei_frames_u16_in(C.c_void_p(src), stride, C.c_void_p(dst), C.c_void_p(gray), n, h, w, depth, st)

    def f_out(src=fp, dst=rp, flag=None, h=h, w=w, hp=h, wp=40, depth=10):
        return lib.spei_frame_u16_out(C.c_void_p(src), C.c_void_p(dst), C.c_void_p(flag), h, w, hp, wp, depth, st)

    def stats(src=rp, stride=fb, prev=None, n=2, h=h, w=w, depth=10, hist=hp_, sad=sp):
        return lib.spei_frame_pair_stats_u16(C.c_void_p(src), stride, C.c_void_p(prev), n, h, w, depth, C.c_void_p(hist), C.c_void_p(sad), st)

    assert to_rgb() == 0 and to_yuv() == 0 and f_in() == 0 and f_out() == 0 and stats() == 0
    assert to_rgb(n=1, stride=0) == 0 and f_in(n=1, stride=1) == 0 and stats(n=1, stride=3, prev=rp) == 0 and to_rgb(depth=12) == 0
    unknown = [({"layout": 3}, "unknown layout"), ({"layout": -1}, "unknown layout"), ({"matrix": 2}, "unknown layout"),
               ({"rng": 2}, "unknown layout")]
    depths = [({"depth": 8}, "unknown depth"), ({"depth": 16}, "unknown depth"), ({"depth": 0}, "unknown depth")]
    shape = [({"h": 0}, "bad"), ({"w": -1}, "bad"), ({"h": 30000, "w": 30000}, "bad")]
    cases = {
        "spei_yuv_to_rgb_u16": (to_rgb, [({"src": None}, "null pointer"), ({"dst": None}, "null pointer"), ({"n": 0}, "bad frame shape"),
                                         ({"stride": nb - 2}, "frame stride"), ({"stride": nb, "layout": R.P444}, "frame stride"),
                                         ({"stride": nb + 1}, "odd frame stride")] + shape + unknown + depths),
        "spei_rgb_u16_to_yuv": (to_yuv, [({"src": None}, "null pointer"), ({"dst": None}, "null pointer")] + shape + unknown + depths),
        "spei_frames_u16_in": (f_in, [({"src": None}, "null pointer"), ({"dst": None, "gray": None}, "null pointer"),
                                      ({"n": 0}, "bad frame shape"), ({"stride": fb - 2}, "frame stride"),
                                      ({"stride": fb + 1}, "odd frame stride"), ({"h": 10, "w": 10}, "reflect-pad")] + shape + depths),
        "spei_frame_u16_out": (f_out, [({"src": None}, "null pointer"), ({"dst": None}, "null pointer"), ({"hp": h - 1}, "bad sizes"),
                                       ({"wp": w - 1}, "bad sizes"), ({"h": 0}, "bad sizes")] + depths),
        "spei_frame_pair_stats_u16": (stats, [({"src": None}, "null pointer"), ({"hist": None}, "null pointer"),
                                              ({"sad": None}, "null pointer"), ({"n": 0}, "frames"), ({"n": 1}, "no prev"),
                                              ({"stride": fb - 2}, "frame stride"), ({"stride": fb + 1}, "odd frame stride")]
                                      + shape + depths),
    }
    for name, (fn, bad) in cases.items():
        for kw, text in bad:
            assert fn(**kw) != 0, (name, kw)
            msg = lib.spei_last_error().decode()
            assert text in msg and name in msg, (name, kw, msg)
    with pytest.raises(ValueError, match="depth must be 10 or 12"):
        ops.yuv_to_rgb_u16(planar.view(torch.uint16), h, w, R.CENTER, R.BT601, R.FULL, 8)
    with pytest.raises(RuntimeError, match="spei_yuv_to_rgb_u16 failed"):
        ops.yuv_to_rgb_u16(planar.view(torch.uint16), h, w, R.CENTER, 5, R.FULL, 10)
    # the u8 entry points keep layout 3 unknown
    assert lib.spei_yuv_to_rgb_u8(C.c_void_p(pp), ns, C.c_void_p(rp), 2, h, w, 3, R.BT601, R.FULL, st) != 0
    assert "unknown layout" in lib.spei_last_error().decode()


# ---- 3. the clip loop ---------------------------------------------------------------------------------------------------------------------
def _clip(T, h, w, depth, seed=3):
    """uint16 [T,h,w,3] of `depth` bits: the synthetic frames, shifted a little per frame (tests/test_gpu_yuv.py::_clip), quantised
    to the depth (so the low bits are in use)."""
    D = (1 << depth) - 1
    x = synth_frames(1, h, w, seed=seed)[0]
    return np.stack([(torch.roll(x[i % 5], shifts=(i, -2 * i), dims=(1, 2)).permute(1, 2, 0).numpy().astype(np.float64) * D).round()
                     .clip(0, D).astype(np.uint16) for i in range(T)])


def _write_y4m(path, clip, layout, rng, matrix, depth, fps=(30000, 1001), aspect=(1, 1)):
    with y4m.Y4MWriter(path, clip.shape[2], clip.shape[1], fps, layout, rng, aspect, depth=depth) as wr:
        for f in clip:
            wr.write(R.rgb_to_yuv(f, layout, matrix, rng, depth).astype("<u2"))
    return str(path)


def _frames(run):
    out = {i: t.cpu().numpy() for i, t in run}
    assert sorted(out) == list(range(len(out)))
    return [out[i] for i in range(len(out))]


@pytest.fixture(scope="module")
def net16():
    return video.load_model("synthetic", DEV, "f16")


def _planar_rgb(reader, h, w, layout, matrix, rng, depth):
    planar = np.stack([reader.raw(i).view("<u2") for i in range(len(reader))])
    rgb = _host(ops.yuv_to_rgb_u16(_dev(planar), h, w, layout, matrix, rng, depth))
    assert np.array_equal(rgb[2], R.yuv_to_rgb(planar[2], h, w, layout, matrix, rng, depth))
    return rgb


def test_clip_from_444p10_equals_clip_from_its_rgb(net16, tmp_path):
    T, h, w, depth, layout, rng = 5, 40, 60, 10, R.P444, R.LIMITED
    path = _write_y4m(tmp_path / "clip.y4m", _clip(T, h, w, depth), layout, rng, R.BT601, depth)
    reader = y4m.Y4MReader(path, depths=(8, 10, 12))
    assert (len(reader), reader.matrix, reader.range, reader.layout, reader.depth) == (T, R.BT601, rng, layout, depth)
    rgb = _planar_rgb(reader, h, w, layout, R.BT601, rng, depth)
    labels = [1, 0, 0, 0, 1]
    a, b = video.deblur_clip(net16, path, labels), video.deblur_clip(net16, rgb, labels, depth=depth)       # the path opens the file
    assert (a.depth, a.out_depth, b.depth, b.out_depth) == (10, 10, 10, 10) and a.frames.yuv == (layout, R.BT601, rng)
    fa, fb = _frames(a), _frames(b)
    assert len(fa) == T and all(x.shape == (h, w, 3) and x.dtype == np.uint16 and np.array_equal(x, y) for x, y in zip(fa, fb))
    assert max(int(x.max()) for x in fa) <= 1023 and len({int(v) & 3 for v in fa[1].reshape(-1)}) == 4      # 10 bits, all in use
    assert a.plan == b.plan and not a.recomputed and not b.recomputed
    # out=, a list of device tensors, out_depth=8 of the deep clip
    out = torch.zeros(T, h, w, 3, dtype=torch.uint16, device=DEV)
    fc = _frames(video.deblur_clip(net16, [t for t in _dev(rgb)], labels, depth=depth, out=out))
    assert all(np.array_equal(x, y) for x, y in zip(fa, fc)) and np.array_equal(_host(out), np.stack(fa))
    f8 = _frames(video.deblur_clip(net16, reader, labels, out_depth=8))
    assert all(x.dtype == np.uint8 and x.shape == (h, w, 3) for x in f8)
    assert max(float(np.abs(x / 1023.0 - y / 255.0).max()) for x, y in zip(fa, f8)) <= 0.5 / 255 + 0.5 / 1023


def test_padded_420p12_clip_with_auto_cuts_and_detector_labels(net16, tmp_path, monkeypatch):
    T, h, w, depth, layout, rng = 5, 37, 53, 12, R.LEFT, R.FULL
    path = _write_y4m(tmp_path / "clip.y4m", _clip(T, h, w, depth), layout, rng, R.BT601, depth)
    reader = y4m.Y4MReader(path, depths=(8, 10, 12))
    assert (reader.layout, reader.depth, reader.chroma) == (R.LEFT, 12, "420p12")          # no siting tag: LEFT
    rgb = _planar_rgb(reader, h, w, layout, R.BT601, rng, depth)
    passes, u8_calls = [], []
    batches = detector.clip_batches
    monkeypatch.setattr(detector, "clip_batches", lambda *a, **k: passes.append(1) or batches(*a, **k))
    for name in ("frames_u8_in", "frame_u8_out", "frame_pair_stats", "yuv_to_rgb_u8"):     # a deep clip never passes through 8 bits
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: u8_calls.append(_n))
    a, b = video.deblur_clip(net16, reader, cuts="auto"), video.deblur_clip(net16, rgb, cuts="auto", depth=depth)
    assert np.array_equal(a.labels, b.labels) and a.cuts == b.cuts and a.plan == b.plan and len(passes) == 2
    assert (a.frames.H, a.frames.W, a.depth, a.out_depth) == (h, w, 12, 12)
    fa, fb = _frames(a), _frames(b)
    assert len(fa) == T and all(x.shape == (h, w, 3) and x.dtype == np.uint16 and np.array_equal(x, y) for x, y in zip(fa, fb))
    assert max(int(x.max()) for x in fa) <= 4095 and not u8_calls
    # the labels are the detector's on the gray planes of the ingest kernel, the cuts find_cuts' on the statistics in 8-bit units
    gray = ops.frames_u16_in(_dev(rgb), depth, gray=True, planes=False)[1]
    assert np.array_equal(a.labels, detector.predict(detector.gray_focus_measures(gray, detector.DEFAULT.kernel_size), detector.DEFAULT))
    sad, hist = video.scene_stats(reader, DEV)
    ref_sad, ref_hist = _pair_ref(rgb, depth)
    assert np.array_equal(sad, ref_sad / 16.0) and np.array_equal(hist, ref_hist)
    assert a.cuts == video.find_cuts(ref_sad / 16.0, ref_hist, h * w)
    # the siting is the reader's plain attribute
    reader.layout = y4m.CENTER
    c = video.deblur_clip(net16, reader, a.labels)
    assert c.frames.yuv[0] == R.CENTER
    planar = _dev(np.stack([reader.raw(1)]))
    assert np.array_equal(_host(c.frames.rgb(planar))[0], R.yuv_to_rgb(reader.raw(1).view("<u2"), h, w, R.CENTER, R.BT601, rng, depth))


def test_scene_cut_in_a_deep_clip(net16):
    """Two shots of different tone (tests/test_gpu_scene_cuts.py::_edge_clip's first two) in one 10-bit clip: "auto" finds the cut
    with the default min_delta, because the SAD is brought to the 8-bit unit first, as it does on the same clip at 8 bits."""
    h, w = 37, 53
    clip8 = np.concatenate([synth_scene_u8(6, h, w, 1700, 1), synth_scene_u8(5, h, w, 5, 2)])
    clip10 = clip8.astype(np.uint16) << 2 | np.random.default_rng(0).integers(0, 4, clip8.shape).astype(np.uint16)
    r8, r10 = video.deblur_clip(net16, clip8, cuts="auto"), video.deblur_clip(net16, clip10, cuts="auto", depth=10)
    assert r8.cuts == [6] and r10.cuts == [6]
    ref_sad, ref_hist = _pair_ref(clip10, 10)
    assert video.find_cuts(ref_sad / 4.0, ref_hist, h * w) == [6] and video.find_cuts(ref_sad, ref_hist, h * w, min_delta=32.0) == [6]
    sad, _ = video.scene_stats(video.frames_of(clip10, depth=10), DEV)
    assert sad.dtype == np.float64 and np.array_equal(sad * 4, _pair_ref(clip10, 10)[0])


def test_8_bit_clip_with_out_depth_10(net16):
    T, h, w = 5, 40, 60
    clip = (_clip(T, h, w, 8)).astype(np.uint8)
    labels = [1, 0, 0, 0, 1]
    a, b = video.deblur_clip(net16, clip, labels), video.deblur_clip(net16, clip, labels, out_depth=10)
    assert (a.depth, a.out_depth, b.depth, b.out_depth) == (8, 8, 8, 10)
    f8, f10 = _frames(a), _frames(b)
    assert all(x.dtype == np.uint8 for x in f8) and all(x.dtype == np.uint16 and x.shape == (h, w, 3) for x in f10)
    worst = max(float(np.abs(x.astype(np.float64) / 1023 - y.astype(np.float64) / 255).max()) for x, y in zip(f10, f8))
    print(f"max |o10 / 1023 - o8 / 255| = {worst:.6f} (bound {0.5 / 255 + 0.5 / 1023:.6f})")
    assert worst <= 0.5 / 255 + 0.5 / 1023                           # the two roundings of one float value, not a tolerance
    assert len({int(v) & 3 for v in f10[1].reshape(-1)}) == 4        # the extra bits carry something


def test_non_finite_deep_windows_recomputed():
    """One weight beyond +-65504 makes every f16 frame non-finite (tests/test_gpu_video.py::test_non_finite_windows_recomputed): the
    flag of spei_frame_u16_out sends each window to the bf16x3 recompute, which yields the uint16 frame of the bf16x3 forward."""
    import warnings
    T, h, w, depth, labels = 4, 40, 60, 10, np.asarray([1, 0, 0, 1])
    net = video.load_model("synthetic", DEV, "f16")
    with torch.no_grad():
        net.recons_net.outBlock[3].weight[0, 0, 0, 0] = 1.0e5
    net.invalidate_packed()
    clip = _clip(T, h, w, depth)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        run = video.deblur_clip(net, clip, labels, depth=depth)
        got = _frames(run)
    assert run.recomputed == list(range(T)) and sum("recomputed in bf16x3" in str(c.message) for c in caught) == T
    assert (net.precision, net.corr_precision, net.use_graph) == ("f16", "top2", True)     # restored
    assert all(x.dtype == np.uint16 and x.shape == (h, w, 3) for x in got)
    net.precision, net.corr_precision, net.use_graph = "bf16x3", "bf16x3", False
    dev = _dev(clip)
    zero = torch.zeros(1, 3, h, w, device=DEV)
    for p in video.window_plan(labels):
        parts = [ops.frames_u16_in(dev[i], depth)[0] for i in p["window"]]
        parts += [zero if p["zero_pre"] else ops.frames_u16_in(dev[p["pre"]], depth)[0],
                  zero if p["zero_sub"] else ops.frames_u16_in(dev[p["sub"]], depth)[0]]
        with torch.no_grad():
            y = net(torch.cat(parts)[None], routing=[p["zero_pre"]])
        assert torch.isfinite(y).all()
        assert np.array_equal(got[p["index"]], _host(ops.frame_u16_out(y[0], h, w, depth))), p["index"]


# ---- 4. command line ----------------------------------------------------------------------------------------------------------------------
def test_cli_deep_y4m(tmp_path):
    T, h, w, depth = 3, 21, 24, 10
    layout, rng, matrix = R.LEFT, R.LIMITED, R.BT601
    path = _write_y4m(tmp_path / "clip.y4m", _clip(T, h, w, depth), layout, rng, matrix, depth)
    labels = np.asarray([1, 0, 1])
    np.save(tmp_path / "labels.npy", labels)
    net32 = video.load_model("synthetic", DEV, "f32")
    ref = _frames(video.deblur_clip(net32, path, labels))
    ref8 = _frames(video.deblur_clip(net32, path, labels, out_depth=8))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "speinet_amd.video", "--model_path", "synthetic", "--labels", str(tmp_path / "labels.npy"),
            "--precision", "f32", "--device", DEV, "--input", path]

    def run(*more):
        r = subprocess.run(base + list(more), cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert sum(ln.startswith("> 00000") for ln in r.stdout.splitlines()) == T
        return r.stdout

    # deep y4m in -> y4m out at the same depth: the tag, T frames, each the conversion of the frame deblur_clip yields
    out = tmp_path / "out.y4m"
    run("--output", str(out))
    assert out.read_bytes().split(b"\n", 1)[0] == b"YUV4MPEG2 W24 H21 F30000:1001 Ip A1:1 C420p10 XYSCSS=420P10 XCOLORRANGE=LIMITED"
    with y4m.Y4MReader(out, depths=(8, 10, 12)) as got:
        assert (got.width, got.height, got.fps, got.layout, got.depth, got.range, len(got)) == (w, h, (30000, 1001), layout, depth, rng, T)
        assert got.frame_bytes == 2 * R.frame_samples(h, w, layout)
        for i in range(T):
            assert np.array_equal(got.raw(i).view("<u2"), R.rgb_to_yuv(ref[i], layout, matrix, rng, depth)), i

    # --out_depth 8 -> an 8-bit stream in the input's layout; --chroma selects the siting the deep 4:2:0 input is read with
    out8 = tmp_path / "out8.y4m"
    run("--output", str(out8), "--out_depth", "8")
    with y4m.Y4MReader(out8) as got:
        assert (got.chroma, got.depth, got.layout, len(got), got.frame_bytes) == ("420mpeg2", 8, layout, T, R.frame_samples(h, w, layout))
        for i in range(T):
            assert np.array_equal(got.raw(i), R8.rgb_to_yuv(ref8[i], layout, matrix, rng)), i

    # deep input -> PNG directory: 8-bit PNGs and the one log line
    dst = tmp_path / "png"
    text = run("--output", str(dst))
    assert sum("10-bit input, PNG output" in ln for ln in text.splitlines()) == 1
    assert sorted(os.listdir(dst)) == [f"{i:06d}.png" for i in range(T)]
    for i in range(T):
        img = video._imread(str(dst / f"{i:06d}.png"))
        assert img.dtype == np.uint8 and np.array_equal(img, ref8[i]), i


def test_cli_chroma_selects_deep_siting_and_png_refuses_deep_output(tmp_path):
    T, h, w, depth = 3, 20, 24, 12
    matrix, rng = R.BT601, R.FULL
    path = _write_y4m(tmp_path / "clip.y4m", _clip(T, h, w, depth), R.CENTER, rng, matrix, depth)
    np.save(tmp_path / "labels.npy", np.asarray([1, 0, 1]))
    reader = y4m.Y4MReader(path, depths=(8, 10, 12))
    reader.layout = y4m.CENTER
    ref = _frames(video.deblur_clip(video.load_model("synthetic", DEV, "f32"), reader, [1, 0, 1]))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "speinet_amd.video", "--model_path", "synthetic", "--labels", str(tmp_path / "labels.npy"),
            "--precision", "f32", "--device", DEV, "--input", path]
    out = tmp_path / "out.y4m"
    r = subprocess.run(base + ["--output", str(out), "--chroma", "420jpeg"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    with y4m.Y4MReader(out, depths=(8, 10, 12)) as got:
        assert (got.chroma, got.depth, len(got)) == ("420p12", 12, T)
        for i in range(T):
            assert np.array_equal(got.raw(i).view("<u2"), R.rgb_to_yuv(ref[i], R.CENTER, matrix, rng, depth)), i
    r = subprocess.run(base + ["--output", str(tmp_path / "png"), "--out_depth", "10"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode != 0 and "PNG directory gets 8-bit files" in r.stderr
