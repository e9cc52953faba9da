"""GPU suite for the region of interest in the clip API (csrc/roi_io.hip; `ops.roi_paste`, `ops.roi_in`, `ops.frame_extent`;
`video.deblur_clip(..., roi=, roi_feather=)`): the paste bit for bit against tests/roi_ref.py (hard) and inside the float64 band of the
feathered tile seams' rule (feathered), the extent maxima exactly, the refusals of bad arguments, and the defining property of a clip
with a region of interest: inside the rectangle the clip of cropped frames, outside it the input at the output depth, bit for bit."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import roi_ref as RR                                                           # noqa: E402
import tiles_ref as R                                                          # noqa: E402
import yuv_ref as Y                                                            # noqa: E402
from test_roi_cpu import ALIGNED, CORNERS, DEPTHS, ODD, PADDED, SHAPES, feathers, make_case            # noqa: E402
from speinet_amd import _lib, ops, video, y4m                                  # noqa: E402
from speinet_amd.synth import synth_frames                                     # noqa: E402

DEV = "cuda:0"
VP = ctypes.c_void_p


def _paste(src, frame, roi, in_depth=8, out_depth=8, feather=0, **kw):
    return ops.roi_paste(torch.from_numpy(src).to(DEV), torch.from_numpy(frame).to(DEV), roi, out_depth, feather,
                         None if in_depth == 8 else in_depth, **kw).cpu().numpy()


def _ties(D: int) -> np.ndarray:
    """float32 values v with fl(v * D) == k + 0.5 exactly: round-half-even decides them (tests/test_gpu_tiles.py's)."""
    out = []
    for k in range(0, D, max(1, D // 255)):
        v = np.float32((k + 0.5) / D)
        for c in (v, np.nextafter(v, np.float32(1)), np.nextafter(v, np.float32(0))):
            if np.float32(c) * np.float32(D) == np.float32(k + 0.5):
                out.append(c)
                break
    return np.asarray(out, np.float32)


# ---- 1. the hard paste -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,roi", SHAPES)
def test_paste_hard(shape, roi):
    y0, x0, h, w = roi
    for in_depth, out_depth in ((8, 8), (10, 10), (12, 12), (8, 12), (12, 8)):
        D = R.scale_of(out_depth)
        src, frame = make_case(shape, roi, in_depth)
        # the .5 quantisation boundaries, exact 0 and 1 and values far outside [0, 1], inside the crop
        special = np.concatenate([_ties(D), np.float32([0.0, 1.0, -0.0, -3.0, 7.0, 255.0])])
        crop = src[:, :h, :w].copy()
        rng = np.random.default_rng(h * w + out_depth)
        crop.reshape(-1)[rng.choice(crop.size, size=len(special), replace=False)] = special
        src[:, :h, :w] = crop
        ref = RR.paste(src, frame, roi, in_depth, out_depth)
        flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)                  # cleared by the call
        got = _paste(src, frame, roi, in_depth, out_depth, nonfinite=flag)
        assert got.dtype == ref["out"].dtype and got.shape == shape + (3,)
        assert np.array_equal(got, ref["out"]), (in_depth, out_depth, np.argwhere(got != ref["out"])[:5])
        assert int(flag.item()) == 0
        # into a given destination, without a flag; planes that are not 16-byte aligned: the element loads
        out = torch.zeros(shape + (3,), dtype=torch.uint8 if out_depth == 8 else torch.uint16, device=DEV)
        buf = torch.zeros(src.size + 1, device=DEV)
        buf[1:] = torch.from_numpy(src).to(DEV).reshape(-1)
        deep = None if in_depth == 8 else in_depth
        assert ops.roi_paste(buf[1:].view(src.shape), torch.from_numpy(frame).to(DEV), roi, out_depth, 0, deep, out=out).data_ptr() == out.data_ptr()
        assert np.array_equal(out.cpu().numpy(), got)


@pytest.mark.parametrize("shape,roi", [((48, 64), (4, 8, 20, 24)), ((47, 57), (6, 9, 21, 23))])
@pytest.mark.parametrize("out_depth", DEPTHS)
@pytest.mark.parametrize("in_depth", DEPTHS)
def test_paste_every_code(shape, roi, in_depth, out_depth):
    """All nine depth pairs on a frame that holds, outside the rectangle, every code of its depth and, for a deep frame, words above
    D_in (read as D_in)."""
    Din = R.scale_of(in_depth)
    src, frame = make_case(shape, roi, in_depth)
    y0, x0, h, w = roi
    outside = np.ones(shape, bool)
    outside[y0:y0 + h, x0:x0 + w] = False
    codes = list(range(Din + 1)) + ([int(v) for v in np.linspace(Din + 1, 65535, 64)] if in_depth > 8 else [])
    at = np.argwhere(np.broadcast_to(outside[..., None], frame.shape))
    assert len(at) >= len(codes)
    at = at[np.random.default_rng(5).choice(len(at), size=len(codes), replace=False)]
    frame[at[:, 0], at[:, 1], at[:, 2]] = codes
    assert len(np.unique(np.minimum(frame, Din)[outside])) == Din + 1 and (in_depth == 8 or (frame[outside] > Din).any())
    ref = RR.paste(src, frame, roi, in_depth, out_depth)
    got = _paste(src, frame, roi, in_depth, out_depth)
    assert np.array_equal(got, ref["out"])
    assert np.array_equal(got[outside], RR.requant(frame, in_depth, out_depth)[outside])


@pytest.mark.parametrize("depth", DEPTHS)
def test_whole_frame_rectangle_is_the_frame_egress(depth):
    for H, W in ((40, 64), (23, 29)):
        roi = (0, 0, H, W)
        src, frame = make_case((H, W), roi, depth)
        src[0, 3, 5], src[2, H - 1, W - 1] = np.nan, np.inf
        x = torch.from_numpy(src).to(DEV)
        flag_a, flag_b = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        want = ops.frame_u8_out(x, H, W, nonfinite=flag_a) if depth == 8 else ops.frame_u16_out(x, H, W, depth, nonfinite=flag_a)
        for feather in (0, 5):                                                     # every side lies on the frame's border: no ramp
            got = ops.roi_paste(x, torch.from_numpy(frame).to(DEV), roi, depth, feather, None if depth == 8 else depth, nonfinite=flag_b)
            assert torch.equal(got, want) and int(flag_a.item()) != 0 and int(flag_b.item()) != 0


def test_non_finite_values():
    for shape, roi in (ODD, PADDED):
        y0, x0, h, w = roi
        src, frame = make_case(shape, roi)
        base = _paste(src, frame, roi)
        # NaN and infinities in the pad (and nowhere else): the same frame, no flag
        if R.up20(h) > h or R.up20(w) > w:
            padded = src.copy()
            padded[:, h:, :] = np.nan
            padded[:, :, w:] = -np.inf
            flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)
            assert np.array_equal(_paste(padded, frame, roi, nonfinite=flag), base) and int(flag.item()) == 0
        for v, (c, ry, rx) in ((np.nan, (0, 0, 0)), (np.inf, (1, h - 1, w - 1)), (-np.inf, (2, h // 2, 1))):
            s = src.copy()
            s[c, ry, rx] = v
            flag = torch.zeros(1, dtype=torch.int32, device=DEV)
            got = _paste(s, frame, roi, nonfinite=flag)
            ref = RR.paste(s, frame, roi)
            assert ref["bad"] and int(flag.item()) != 0 and got[y0 + ry, x0 + rx, c] == 0
            assert np.array_equal(got, ref["out"])
            got[y0 + ry, x0 + rx, c] = base[y0 + ry, x0 + rx, c]
            assert np.array_equal(got, base)                                       # the rest of the frame intact


def test_paste_refusals():
    """Refused through the C-ABI before anything is launched: the flag is not cleared, the frame not written."""
    (H, W), (y0, x0, h, w) = ALIGNED
    hp, wp = R.up20(h), R.up20(w)
    lib = _lib.lib()
    st = VP(torch.cuda.current_stream(DEV).cuda_stream)
    src = torch.zeros(3, hp, wp, device=DEV)
    for depth in (8, 12):
        dtype = torch.uint8 if depth == 8 else torch.uint16
        frame = torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV)
        out = torch.full((H, W, 3), 9, dtype=dtype, device=DEV)
        flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)
        good = dict(src=src.data_ptr(), frame=frame.data_ptr(), in_depth=8, dst=out.data_ptr(), H=H, W=W, y0=y0, x0=x0, h=h, w=w, hp=hp,
                    wp=wp, feather=0, depth=depth)

        def call(**kw):
            a = dict(good, **kw)
            head = (VP(a["src"]), VP(a["frame"]), a["in_depth"], VP(a["dst"]), VP(flag.data_ptr()), a["H"], a["W"], a["y0"], a["x0"],
                    a["h"], a["w"], a["hp"], a["wp"], a["feather"])
            return lib.spei_roi_paste_u8(*head, st) if depth == 8 else lib.spei_roi_paste_u16(*head, a["depth"], st)

        cases = [(dict(src=None), "null pointer"), (dict(frame=None), "null pointer"), (dict(dst=None), "null pointer"),
                 (dict(in_depth=9), "unknown in_depth 9"), (dict(in_depth=16), "unknown in_depth 16"),
                 (dict(y0=-1), "lies outside"), (dict(x0=W - w + 1), "lies outside"), (dict(y0=H - h + 1), "lies outside"),
                 (dict(h=0, hp=0), "lies outside"), (dict(w=0, wp=0), "lies outside"), (dict(h=H + 1, hp=R.up20(H + 1), y0=0), "lies outside"),
                 (dict(hp=hp + 20), "rounded up"), (dict(wp=w), "rounded up"),
                 (dict(feather=-1), "feather -1"), (dict(feather=h // 2 + 1), f"feather {h // 2 + 1}"), (dict(feather=201), "feather 201"),
                 (dict(dst=frame.data_ptr()), "dst overlaps frame"), (dict(dst=src.data_ptr()), "dst overlaps src"),
                 # the last two bytes of src: the allocator may have placed `frame` right behind it, and that is named first
                 (dict(dst=src.data_ptr() + 4 * 3 * hp * wp - 2), "dst overlaps")]
        if depth != 8:
            cases += [(dict(depth=8), "unknown depth 8"), (dict(depth=11), "unknown depth 11")]
        for kw, text in cases:
            assert call(**kw) != 0, kw
            assert text in lib.spei_last_error().decode(), (kw, lib.spei_last_error().decode())
        torch.cuda.synchronize()
        assert int(flag.item()) == 7 and (out == 9).all() and (frame == 0).all()    # neither cleared nor written: nothing ran
        assert call() == 0
        torch.cuda.synchronize()
        assert int(flag.item()) == 0 and not (out == 9).all()
    # and the wrapper
    x, f8 = torch.zeros(3, hp, wp, device=DEV), torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV)
    for kw, text in ((dict(roi=(y0, x0, h, w + 40)), "outside"), (dict(roi=(y0, x0, h, True)), "four whole numbers"),
                     (dict(roi=(y0, x0, h - 20, w)), "rounds up"), (dict(feather=h // 2 + 1), "feather"), (dict(feather=1.0), "feather"),
                     (dict(out_depth=9), "out_depth"), (dict(in_depth=10), "uint16 frames only")):
        a = dict(dict(roi=(y0, x0, h, w), out_depth=8, feather=0, in_depth=None), **kw)
        with pytest.raises(ValueError, match=text):
            ops.roi_paste(x, f8, a["roi"], a["out_depth"], a["feather"], a["in_depth"])
    with pytest.raises(RuntimeError, match="dst overlaps frame"):
        ops.roi_paste(x, f8, (y0, x0, h, w), out=f8)


# ---- 2. the feathered paste ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,roi", [ODD, ALIGNED, PADDED] + CORNERS)
def test_paste_feathered(shape, roi):
    y0, x0, h, w = roi
    H, W = shape
    for in_depth, out_depth in ((8, 8), (8, 10), (10, 10), (12, 8), (12, 12)):
        src, frame = make_case(shape, roi, in_depth)
        hard = _paste(src, frame, roi, in_depth, out_depth)
        for f in feathers(roi):
            ref = RR.paste(src, frame, roi, in_depth, out_depth, f)
            ramp = ref["ramp"]
            flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)
            got = _paste(src, frame, roi, in_depth, out_depth, f, nonfinite=flag)
            assert int(flag.item()) == 0
            # every sample with wt == 1: the hard paste, bit for bit
            assert np.array_equal(got[~ramp], hard[~ramp])
            g = got.astype(np.int64)
            open_share = float((ref["lo"] != ref["hi"])[ramp].mean())
            off = (g < ref["lo"]) | (g > ref["hi"])
            print(f"{H}x{W} {roi} feather {f} depths {in_depth}->{out_depth}: {int(ramp.sum()) * 3} ramp samples, open band "
                  f"{100 * open_share:.3f} %, outside the band {int(off.sum())}, differing from the float32 restatement "
                  f"{int((got != ref['out']).sum())}")
            assert open_share < 0.01
            assert not off.any(), np.argwhere(off)[:5]
            assert (got != hard)[ramp].mean() > 0.5                                # blended, not copied
            # a side on the frame's border has no ramp: its edge line is the hard paste's off the other axis' ramps
            inner_x = slice(x0 + f * (x0 > 0), x0 + w - f * (x0 + w < W))
            if y0 == 0:
                assert not ramp[0, inner_x].any() and np.array_equal(got[0, inner_x], hard[0, inner_x])
            if y0 + h == H:
                assert not ramp[H - 1, inner_x].any() and np.array_equal(got[H - 1, inner_x], hard[H - 1, inner_x])
    # a non-finite value on a ramp: the flag and the 0 follow the model's value
    src, frame = make_case(shape, roi)
    f = feathers(roi)[1]
    ry, rx = (1 if y0 > 0 else h - 2), w // 2
    base = _paste(src, frame, roi, feather=f)
    assert RR.paste(src, frame, roi, feather=f)["ramp"][y0 + ry, x0 + rx]
    for v in (np.nan, np.inf, -np.inf):
        s = src.copy()
        s[1, ry, rx] = v
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        got = _paste(s, frame, roi, feather=f, nonfinite=flag)
        assert int(flag.item()) != 0 and got[y0 + ry, x0 + rx, 1] == 0
        got[y0 + ry, x0 + rx, 1] = base[y0 + ry, x0 + rx, 1]
        assert np.array_equal(got, base), v


# ---- 3. the extent ---------------------------------------------------------------------------------------------------------------------------
def _extent(frames, depth=8, out=None):
    rows, cols = ops.frame_extent(torch.from_numpy(frames).to(DEV), None if depth == 8 else depth, out=out)
    return rows.cpu().numpy(), cols.cpu().numpy()


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H,W", [(21, 37), (40, 64), (19, 301)])
def test_extent(H, W, n, depth):
    D = R.scale_of(depth)
    dtype = np.uint8 if depth == 8 else np.uint16
    rng = np.random.default_rng(H * W + n + depth)
    # one bright pixel at each corner and on each edge of an otherwise black frame
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 3), (H // 2, 0), (H // 3, W - 1)):
        f = np.zeros((n, H, W, 3), dtype)
        f[n - 1, y, x] = (D, D // 2, 3)
        rows, cols = _extent(f, depth)
        want = RR.extent(f, depth)
        assert np.array_equal(rows, want[0]) and np.array_equal(cols, want[1])
        assert np.flatnonzero(rows).tolist() == [y] and np.flatnonzero(cols).tolist() == [x] and rows[y] == cols[x] > 0
    # random frames, dim rows and columns among them; deep words above D clamp
    f = rng.integers(0, D + 1, (n, H, W, 3)).astype(dtype)
    f[:, :3] //= 16
    f[:, :, W - 5:] //= 8
    if depth > 8:
        f[0, H // 2, W // 2] = (65535, D + 1, 40000)
        assert RR.extent(f, depth)[0][H // 2] == D
    want = RR.extent(f, depth)
    rows, cols = _extent(f, depth)
    assert rows.dtype == np.int32 and np.array_equal(rows, want[0]) and np.array_equal(cols, want[1])
    # frames that are not 4-byte (8-byte) aligned, at a frame stride that is none either: the element loads
    pad = 3
    buf = torch.zeros(n * (H * W * 3 + pad) + 1, dtype=torch.from_numpy(f).dtype, device=DEV)
    view = buf[1:].as_strided((n, H, W, 3), (H * W * 3 + pad, W * 3, 3, 1))
    view.copy_(torch.from_numpy(f).to(DEV))
    rows, cols = ops.frame_extent(view, None if depth == 8 else depth)
    assert np.array_equal(rows.cpu().numpy(), want[0]) and np.array_equal(cols.cpu().numpy(), want[1])
    # two accumulating calls equal one call, and a call without `out` clears
    if n > 1:
        dev = torch.from_numpy(f).to(DEV)
        deep = None if depth == 8 else depth
        ext = ops.frame_extent(dev[:1], deep)
        assert not np.array_equal(ext[0].cpu().numpy(), want[0])
        ext2 = ops.frame_extent(dev[1:], deep, out=ext)
        assert ext2[0].data_ptr() == ext[0].data_ptr()
        assert np.array_equal(ext[0].cpu().numpy(), want[0]) and np.array_equal(ext[1].cpu().numpy(), want[1])
        lib, st = _lib.lib(), VP(torch.cuda.current_stream(DEV).cuda_stream)
        ext[0].fill_(70000)
        ext[1].fill_(70000)
        black = torch.zeros_like(dev[:1])
        args = (VP(black.data_ptr()), black.stride(0) * black.element_size(), 1, H, W) + (() if depth == 8 else (depth,))
        fn = lib.spei_frame_extent if depth == 8 else lib.spei_frame_extent_u16
        assert fn(*args, VP(ext[0].data_ptr()), VP(ext[1].data_ptr()), 1, st) == 0
        assert (ext[0] == 70000).all() and (ext[1] == 70000).all()                 # accumulate: what is there stays
        assert fn(*args, VP(ext[0].data_ptr()), VP(ext[1].data_ptr()), 0, st) == 0
        assert (ext[0] == 0).all() and (ext[1] == 0).all()                         # accumulate == 0 clears


def test_extent_refusals():
    lib, st = _lib.lib(), VP(torch.cuda.current_stream(DEV).cuda_stream)
    f = torch.zeros(2, 20, 24, 3, dtype=torch.uint8, device=DEV)
    rows, cols = torch.full((20,), 5, dtype=torch.int32, device=DEV), torch.full((24,), 5, dtype=torch.int32, device=DEV)
    p, r, c = VP(f.data_ptr()), VP(rows.data_ptr()), VP(cols.data_ptr())
    for args, text in (((None, 1440, 2, 20, 24, r, c, 0, st), "null pointer"), ((p, 1440, 2, 20, 24, None, c, 0, st), "null pointer"),
                       ((p, 1440, 0, 20, 24, r, c, 0, st), "0 frames"), ((p, 1440, 2, 0, 24, r, c, 0, st), "bad frame shape"),
                       ((p, 1439, 2, 20, 24, r, c, 0, st), "frame stride")):
        assert lib.spei_frame_extent(*args) != 0 and text in lib.spei_last_error().decode(), lib.spei_last_error().decode()
    assert lib.spei_frame_extent_u16(p, 2880, 1, 20, 24, 9, r, c, 0, st) != 0 and "unknown depth 9" in lib.spei_last_error().decode()
    assert lib.spei_frame_extent_u16(p, 2881, 2, 20, 12, 10, r, c, 0, st) != 0 and "odd frame stride" in lib.spei_last_error().decode()
    torch.cuda.synchronize()
    assert (rows == 5).all() and (cols == 5).all()


def test_roi_in_is_the_frame_ingest_of_the_crop():
    for (H, W), roi in (ODD, ALIGNED, PADDED):
        y0, x0, h, w = roi
        for depth in DEPTHS:
            _, frame = make_case((H, W), roi, depth)
            dev = torch.from_numpy(frame).to(DEV)
            crop = dev[y0:y0 + h, x0:x0 + w].contiguous()
            want = ops.frames_u8_in(crop)[0] if depth == 8 else ops.frames_u16_in(crop, depth)[0]
            out = torch.full((3, R.up20(h), R.up20(w)), -1.0, device=DEV)
            assert ops.roi_in(dev, roi, out, None if depth == 8 else depth) is out
            assert torch.equal(out, want[0])


# ---- 4. the clip ---------------------------------------------------------------------------------------------------------------------------
LABELS, CUTS = [0, 1, 0, 0, 0, 0], [3]     # a sharp frame in the first scene, none in the second
NUMBERS = [0, 1, 2, 13, 23, 33]            # gaps in the second scene, so that window 4 routes to the no-reference branch
MODES = {"f16-graph": ("f16", True), "f32-eager": ("f32", False)}
H, W = 60, 80
RECTS = [(7, 13, 40, 60), (3, 5, 43, 61), (20, 19, 40, 61)]       # multiples of 20 at an odd origin; padded; the bottom-right corner


def _clip(n, h, w, seed=3):
    """uint8 [n,h,w,3]: the synthetic frames, shifted a little per frame (tests/test_gpu_video.py's)."""
    x = synth_frames(1, h, w, seed=seed)[0]
    return np.ascontiguousarray(np.stack([(torch.roll(x[i % 5], shifts=(i, -2 * i), dims=(1, 2)).permute(1, 2, 0).numpy() * 255)
                                          .round().astype(np.uint8) for i in range(n)]))


def _frames(run) -> np.ndarray:
    got = {i: t.cpu().numpy() for i, t in run}
    assert sorted(got) == list(range(len(got)))
    return np.stack([got[i] for i in range(len(got))])


def _crop(frames, roi):
    y0, x0, h, w = roi
    return np.ascontiguousarray(frames[:, y0:y0 + h, x0:x0 + w])


def _expected(frames, inner, roi, in_depth=8, out_depth=8):
    """The defining property: the input at the output depth with the cropped clip's result in the rectangle."""
    y0, x0, h, w = roi
    want = RR.requant(frames, in_depth, out_depth).astype(inner.dtype)
    want[:, y0:y0 + h, x0:x0 + w] = inner
    return want


@pytest.fixture(scope="module")
def nets():
    return {mode: video.load_model("synthetic", DEV, precision, graph=graph) for mode, (precision, graph) in MODES.items()}


@pytest.fixture(scope="module")
def clip():
    return _clip(6, H, W)


@pytest.mark.parametrize("roi", RECTS, ids=[",".join(map(str, r)) for r in RECTS])
@pytest.mark.parametrize("mode", list(MODES))
def test_roi_clip_is_the_cropped_clip_in_the_frame(nets, clip, mode, roi):
    net = nets[mode]
    kw = dict(numbers=NUMBERS, cuts=CUTS)
    inner_run = video.deblur_clip(net, _crop(clip, roi), LABELS, **kw)
    inner = _frames(inner_run)
    out = torch.zeros(6, H, W, 3, dtype=torch.uint8, device=DEV)
    run = video.deblur_clip(net, clip, LABELS, roi=roi, out=out, **kw)
    assert run.roi == roi and run.tiles is None
    assert [(p["keys"], p["zero_pre"]) for p in run.plan] == [(p["keys"], p["zero_pre"]) for p in inner_run.plan]
    assert any(p["zero_pre"] for p in run.plan) and any(not p["zero_pre"] for p in run.plan)
    got = _frames(run)
    assert run.recomputed == []
    want = _expected(clip, inner, roi)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(out.cpu().numpy(), want)
    assert (inner != _crop(clip, roi)).mean() > 0.1                                # the rectangle is deblurred, not copied


def test_roi_whole_frame_and_none_are_the_path_without(nets, clip):
    net = nets["f32-eager"]
    ref = _frames(video.deblur_clip(net, clip, LABELS, numbers=NUMBERS, cuts=CUTS))
    for roi in (None, (0, 0, H, W)):
        run = video.deblur_clip(net, clip, LABELS, numbers=NUMBERS, cuts=CUTS, roi=roi)
        assert run.roi is None
        assert np.array_equal(_frames(run), ref)


def test_roi_with_ensemble(nets, clip):
    roi, net = RECTS[1], nets["f16-graph"]
    inner = _frames(video.deblur_clip(net, _crop(clip, roi), LABELS, numbers=NUMBERS, cuts=CUTS, ensemble=2))
    got = _frames(video.deblur_clip(net, clip, LABELS, numbers=NUMBERS, cuts=CUTS, ensemble=2, roi=roi))
    assert np.array_equal(got, _expected(clip, inner, roi))


def test_roi_out_depth_10(nets, clip):
    roi, net = RECTS[0], nets["f32-eager"]
    inner = _frames(video.deblur_clip(net, _crop(clip, roi), LABELS, numbers=NUMBERS, cuts=CUTS, out_depth=10))
    run = video.deblur_clip(net, clip, LABELS, numbers=NUMBERS, cuts=CUTS, out_depth=10, roi=roi)
    got = _frames(run)
    assert got.dtype == np.uint16 and run.out_depth == 10 and run.depth == 8
    want = _expected(clip, inner, roi, 8, 10)
    assert np.array_equal(got, want)
    assert want.max() > 255 and (want[:, 0, 0] == (clip[:, 0, 0].astype(np.int64) * 2046 + 255) // 510).all()


def test_roi_deep_clip(nets):
    """A 12-bit clip, 12 bits out, with words above 4095 outside the rectangle: they come out as 4095."""
    roi, net = RECTS[1], nets["f16-graph"]
    deep = (_clip(6, H, W).astype(np.uint16) << 4) | 9
    deep[:, 0, :4] = 60000
    inner = _frames(video.deblur_clip(net, _crop(deep, roi), LABELS, numbers=NUMBERS, cuts=CUTS, depth=12))
    got = _frames(video.deblur_clip(net, deep, LABELS, numbers=NUMBERS, cuts=CUTS, depth=12, roi=roi))
    assert np.array_equal(got, _expected(deep, inner, roi, 12, 12)) and (got[:, 0, :4] == 4095).all()


def test_roi_from_y4m(nets, clip, tmp_path):
    """The input frame of a y4m clip is the RGB frame the conversion kernel made from it, inside and outside the rectangle."""
    roi, net = RECTS[0], nets["f16-graph"]
    mode = (Y.CENTER, Y.BT601, Y.LIMITED)
    path = tmp_path / "clip.y4m"
    with y4m.Y4MWriter(path, W, H, (25, 1), mode[0], mode[2], (1, 1)) as wr:
        for f in clip:
            wr.write(Y.rgb_to_yuv(f, *mode))
    reader = y4m.Y4MReader(str(path))
    planar = torch.from_numpy(np.stack([reader.raw(i) for i in range(6)])).to(DEV)
    rgb = ops.yuv_to_rgb_u8(planar, H, W, mode[0], Y.BT601, mode[2]).cpu().numpy()
    inner = _frames(video.deblur_clip(net, _crop(rgb, roi), LABELS, numbers=NUMBERS, cuts=CUTS))
    run = video.deblur_clip(net, str(path), LABELS, numbers=NUMBERS, cuts=CUTS, roi=roi, yuv=dict(matrix="bt601"))
    assert np.array_equal(_frames(run), _expected(rgb, inner, roi))


def test_roi_labels_and_cuts_are_the_cropped_clips(nets):
    """labels=None and cuts="auto": the detector and the pair statistics see the rectangle only.  A clip whose frame OUTSIDE the
    rectangle changes abruptly at frame 3 and whose inside does not: no cut with the rectangle, a cut without it."""
    net = nets["f32-eager"]
    roi = (10, 10, 40, 60)
    base = _clip(1, H, W, seed=11)[0]
    frames = np.stack([np.roll(base, i, axis=1) for i in range(6)])                # one shot, panning a pixel per frame
    outside = np.ones((H, W), bool)
    outside[10:50, 10:70] = False
    frames[:3, outside] //= 4
    frames[3:, outside] = 255 - frames[3:, outside] // 4
    inner_run = video.deblur_clip(net, _crop(frames, roi), cuts="auto")
    run = video.deblur_clip(net, frames, cuts="auto", roi=roi)
    whole = video.deblur_clip(net, frames, cuts="auto")
    assert np.array_equal(run.labels, inner_run.labels) and run.cuts == inner_run.cuts == [] and whole.cuts == [3]
    assert np.array_equal(_frames(run), _expected(frames, _frames(inner_run), roi))


# ---- 5. roi="auto" -------------------------------------------------------------------------------------------------------------------------
def _letterboxed(n=6, bar=12):
    frames = np.maximum(_clip(n, H, W, seed=7), 40)                                # no picture line at or below the bar level
    boxed = frames.copy()
    boxed[:, :bar] = 16
    boxed[:, H - bar:] = 17
    return frames, boxed


def test_roi_auto(nets):
    net = nets["f16-graph"]
    frames, boxed = _letterboxed()
    rows, cols = video.active_area(boxed, DEV)
    want = RR.extent(boxed)
    assert np.array_equal(rows, want[0]) and np.array_equal(cols, want[1])
    rows2, _ = video.active_area(boxed, DEV, frames_max=2)
    assert np.array_equal(rows2, RR.extent(boxed[[1, 4]])[0])
    roi = (12, 0, 36, 80)
    assert video.find_bars(rows, cols) == roi
    run = video.deblur_clip(net, boxed, LABELS, numbers=NUMBERS, cuts=CUTS, roi="auto")
    assert run.roi == roi
    explicit = _frames(video.deblur_clip(net, boxed, LABELS, numbers=NUMBERS, cuts=CUTS, roi=roi))
    got = _frames(run)
    assert np.array_equal(got, explicit)
    assert np.array_equal(got[:, :12], boxed[:, :12]) and np.array_equal(got[:, 48:], boxed[:, 48:])
    # bars that the caller's level does not see as black, and the clip without bars: the path without a region
    run = video.deblur_clip(net, boxed, LABELS, numbers=NUMBERS, cuts=CUTS, roi="auto", bar_params=dict(level=15))
    assert run.roi is None
    run = video.deblur_clip(net, frames, LABELS, numbers=NUMBERS, cuts=CUTS, roi="auto")
    assert run.roi is None
    assert np.array_equal(_frames(run), _frames(video.deblur_clip(net, frames, LABELS, numbers=NUMBERS, cuts=CUTS)))
    # a feathered edge: outside the ramps the hard run, bit for bit; on them something else
    soft = _frames(video.deblur_clip(net, boxed, LABELS, numbers=NUMBERS, cuts=CUTS, roi="auto", roi_feather=4))
    ramp = np.zeros((H, W), bool)
    ramp[12:16] = ramp[44:48] = True                                               # the left and right sides lie on the frame's border
    assert np.array_equal(soft[:, ~ramp], explicit[:, ~ramp])
    assert (soft[:, ramp] != explicit[:, ramp]).mean() > 0.05


def test_roi_auto_from_device_frames_and_deep(nets):
    frames, boxed = _letterboxed(4)
    deep = boxed.astype(np.uint16) << 2
    assert video.find_bars(*video.active_area(video.frames_of(torch.from_numpy(deep).to(DEV), depth=10), DEV), 10) == (12, 0, 36, 80)
    pillar = np.ascontiguousarray(boxed.transpose(0, 2, 1, 3))
    assert video.find_bars(*video.active_area(torch.from_numpy(pillar).to(DEV), DEV)) == (0, 12, 80, 36)


# ---- 6. a 16-bit pass that leaves the half range ---------------------------------------------------------------------------------------------
def test_roi_non_finite_windows_recomputed():
    """One weight beyond +-65504 makes every f16 frame non-finite (tests/test_gpu_ensemble.py's): every window is recomputed in bf16x3
    and ends in the same paste, so the frame still is the cropped clip's in the input frame."""
    net = video.load_model("synthetic", DEV, "f16", graph=True)
    with torch.no_grad():
        net.recons_net.outBlock[3].weight[0, 0, 0, 0] = 1.0e5
    net.invalidate_packed()
    frames, labels, roi = _clip(4, 50, 70), [1, 0, 0, 1], (6, 9, 37, 53)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        run = video.deblur_clip(net, frames, labels, roi=roi)
        got = _frames(run)
        inner_run = video.deblur_clip(net, _crop(frames, roi), labels)
        inner = _frames(inner_run)
    assert run.recomputed == [0, 1, 2, 3] == inner_run.recomputed
    assert sum("recomputed in bf16x3" in str(c.message) for c in caught) == 8
    assert (net.precision, net.corr_precision, net.use_graph) == ("f16", "top2", True)     # restored
    assert np.array_equal(got, _expected(frames, inner, roi))


# ---- 7. the command line -------------------------------------------------------------------------------------------------------------------
def test_cli_roi(nets, tmp_path, capsys):
    from PIL import Image
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    _, boxed = _letterboxed(4)
    for i in range(4):
        Image.fromarray(boxed[i]).save(src / f"frame_{i:03d}.png")
    labels = np.asarray([0, 1, 0, 0])
    np.save(tmp_path / "labels.npy", labels)
    base = ["--input", str(src), "--output", str(dst), "--model_path", "synthetic", "--labels", str(tmp_path / "labels.npy"), "--device", DEV]
    video.main(base + ["--roi", "auto"])
    text = capsys.readouterr().out
    assert "# roi 12,0,36,80\n" in text and text.count("> frame_") == 4
    ref = _frames(video.deblur_clip(nets["f16-graph"], boxed, labels, roi=(12, 0, 36, 80)))
    for i in range(4):
        assert np.array_equal(np.asarray(Image.open(dst / f"frame_{i:03d}.png").convert("RGB")), ref[i]), i
    video.main(base + ["--roi", "8,4,40,60", "--roi_feather", "3"])
    assert "# roi 8,4,40,60\n" in capsys.readouterr().out
    ref = _frames(video.deblur_clip(nets["f16-graph"], boxed, labels, roi=(8, 4, 40, 60), roi_feather=3))
    assert np.array_equal(np.asarray(Image.open(dst / "frame_002.png").convert("RGB")), ref[2])
    for bad in (["--roi", "1,2,3"], ["--roi", "auto", "--tiles", "2x2"], ["--roi_feather", "3"]):
        with pytest.raises(SystemExit):
            video.main(base + bad)
