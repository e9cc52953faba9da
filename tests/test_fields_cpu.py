"""Host side of the interlaced mode (`deblur_clip(..., fields="split")`), no GPU: the y4m `interlace=` opt-in of the reader, the stream
and the writer; the numpy statement `fields_ref` (split / weave, the per-field YUV conversions), with the one fact that makes the GPU
tests of the 4:2:0 field conversion meaningful: per field it DIFFERS from the progressive conversion; the `Frames` field view; the
C-ABI declarations; the command line's `--fields`."""
import io

import numpy as np
import pytest

import fields_ref as FR
from speinet_amd import _lib, video, y4m
from speinet_amd.clip import frames_of

OPT_IN = ("p", "t", "b")


def _head(tag):
    return b"YUV4MPEG2 W8 H8 F25:1 " + (b"I" + tag + b" " if tag else b"") + b"C420jpeg\n"


def _stream(data):
    return io.BufferedReader(io.BytesIO(data))


# ---- y4m ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,want", [(b"t", "t"), (b"b", "b"), (b"p", "p"), (b"?", "p"), (b"", "p")])
def test_reader_and_stream_opt_in(tag, want):
    payload = _head(tag) + b"FRAME\n" + bytes(96)
    r = y4m.Y4MReader(io.BytesIO(payload), interlace=OPT_IN)
    assert r.interlace == want and len(r) == 1 and r.frame_bytes == 96
    s = y4m.Y4MStream(_stream(payload), interlace=OPT_IN)
    assert s.interlace == want and s.frame_bytes == 96
    buf = np.empty(96, np.uint8)
    assert s.read_into(buf) and not s.read_into(buf)
    if want != "p":                                               # the default keeps its refusal, word for word
        for cls, f in ((y4m.Y4MReader, io.BytesIO(payload)), (y4m.Y4MStream, _stream(payload))):
            with pytest.raises(ValueError, match=r"tag I%s: interlaced streams are not supported \(progressive Ip only\)" % want):
                cls(f)
    else:
        assert y4m.Y4MReader(io.BytesIO(payload)).interlace == "p"


def test_one_parity_opt_in_and_bad_values():
    assert y4m.Y4MReader(io.BytesIO(_head(b"t")), interlace=("p", "t")).interlace == "t"
    with pytest.raises(ValueError, match="tag Ib: interlaced streams are not supported"):
        y4m.Y4MReader(io.BytesIO(_head(b"b")), interlace=("p", "t"))
    with pytest.raises(ValueError, match="interlace must hold"):
        y4m.Y4MReader(io.BytesIO(_head(b"t")), interlace=("p", "m"))
    with pytest.raises(ValueError, match="interlace must be"):
        y4m.Y4MWriter(io.BytesIO(), 8, 8, interlace="m")


@pytest.mark.parametrize("kw", [{}, {"interlace": OPT_IN}])
def test_mixed_mode_is_refused_either_way(kw):
    for cls, f in ((y4m.Y4MReader, io.BytesIO(_head(b"m"))), (y4m.Y4MStream, _stream(_head(b"m")))):
        with pytest.raises(ValueError, match="tag Im: mixed-mode streams"):
            cls(f, **kw)


@pytest.mark.parametrize("tag", ["p", "t", "b"])
def test_writer_round_trip(tag):
    rng = np.random.default_rng(7)
    f = io.BytesIO()
    w = y4m.Y4MWriter(f, 8, 8, (30000, 1001), y4m.LEFT, y4m.FULL, interlace=tag)
    frames = [rng.integers(0, 256, w.frame_bytes).astype(np.uint8) for _ in range(3)]
    for fr in frames:
        w.write(fr)
    w.close()
    assert (b" I" + tag.encode() + b" ") in f.getvalue().split(b"\n")[0]
    f.seek(0)
    r = y4m.Y4MReader(f, interlace=OPT_IN)
    assert (r.interlace, r.layout, r.range, r.fps, len(r)) == (tag, y4m.LEFT, y4m.FULL, (30000, 1001), 3)
    assert r.frame_bytes == w.frame_bytes == y4m.frame_bytes(8, 8, y4m.LEFT)      # a record is a woven frame: unchanged
    for i, fr in enumerate(frames):
        assert np.array_equal(r.raw(i), fr)


# ---- the numpy statement ------------------------------------------------------------------------------------------------------------------
def test_weave_of_split_is_the_frame():
    rng = np.random.default_rng(1)
    x = rng.integers(0, 256, (10, 7, 3)).astype(np.uint8)
    assert np.array_equal(FR.weave(FR.split(x, 0), FR.split(x, 1)), x)
    assert FR.split(x, 0).shape == (5, 7, 3) and np.array_equal(FR.split(x, 1)[2], x[5])
    a, b = rng.integers(0, 9, (4, 3)), rng.integers(0, 9, (4, 3))
    w = FR.weave(a, b)
    assert np.array_equal(w[0::2], a) and np.array_equal(w[1::2], b)


def _planar(rng, h, w, layout, depth):
    n = y4m.frame_bytes(h, w, layout)
    return rng.integers(0, 1 << depth, n).astype(np.uint8 if depth == 8 else np.uint16)


@pytest.mark.parametrize("depth", (8, 10, 12))
@pytest.mark.parametrize("layout", (FR.P444, FR.P422, FR.MONO))
def test_row_wise_layouts_convert_per_field_as_progressive(layout, depth):
    rng = np.random.default_rng(100 * layout + depth)
    for h, w in ((6, 5), (8, 8)):
        planar = _planar(rng, h, w, layout, depth)
        assert np.array_equal(FR.yuv_fields_to_rgb(planar, h, w, layout, FR.BT709, FR.LIMITED, depth),
                              FR.yuv_to_rgb(planar, h, w, layout, FR.BT709, FR.LIMITED, depth))
        rgb = rng.integers(0, 1 << depth, (h, w, 3)).astype(planar.dtype)
        assert np.array_equal(FR.rgb_to_yuv_fields(rgb, layout, FR.BT601, FR.FULL, depth), FR.rgb_to_yuv(rgb, layout, FR.BT601, FR.FULL, depth))


@pytest.mark.parametrize("depth", (8, 10))
@pytest.mark.parametrize("layout", (FR.CENTER, FR.LEFT))
def test_420_per_field_differs_from_progressive(layout, depth):
    """A frame whose two fields differ in chroma: the progressive 3 : 1 row rule mixes the chroma rows of both fields, the per-field
    rule never does; the same the other way round."""
    h, w, D = 8, 8, (1 << depth) - 1
    yp, up, vp = (np.full(s, D // 2) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))
    up[0::2], up[1::2], vp[0::2], vp[1::2] = D // 4, 3 * (D // 4), 3 * (D // 4), D // 4
    planar = np.concatenate([a.reshape(-1) for a in (yp, up, vp)]).astype(np.uint8 if depth == 8 else np.uint16)
    per_field = FR.yuv_fields_to_rgb(planar, h, w, layout, FR.BT601, FR.FULL, depth)
    progressive = FR.yuv_to_rgb(planar, h, w, layout, FR.BT601, FR.FULL, depth)
    assert not np.array_equal(per_field, progressive)
    for p in (0, 1):                                              # each field is flat: one chroma per field, nothing of the other
        assert (per_field[p::2] == per_field[p, 0]).all()
    assert not np.array_equal(per_field[0], per_field[1])
    rgb = np.zeros((h, w, 3), planar.dtype)
    rgb[0::2, :, 0], rgb[1::2, :, 2] = D, D                       # a red top field, a blue bottom field
    a, b = FR.rgb_to_yuv_fields(rgb, layout, FR.BT601, FR.FULL, depth), FR.rgb_to_yuv(rgb, layout, FR.BT601, FR.FULL, depth)
    assert not np.array_equal(a, b) and np.array_equal(a[:h * w], b[:h * w])      # luma is per pixel; chroma is not
    u = a[h * w:h * w + (h // 2) * (w // 2)].reshape(h // 2, w // 2)
    assert (u[0::2] == u[0, 0]).all() and (u[1::2] == u[1, 0]).all() and u[0, 0] != u[1, 0]


def test_field_pictures_round_trip():
    rng = np.random.default_rng(5)
    for layout in FR.LAYOUTS:
        planar = _planar(rng, 8, 6, layout, 8)
        tb = [FR.field_planar(planar, 8, 6, layout, p) for p in (0, 1)]
        assert tb[0].size == tb[1].size == y4m.frame_bytes(4, 6, layout)
        assert np.array_equal(FR.weave_planar(*tb, 8, 6, layout), planar)


# ---- the Frames view ------------------------------------------------------------------------------------------------------------------------
def test_frames_field_view_copies_nothing():
    clip = np.random.default_rng(2).integers(0, 256, (3, 44, 23, 3)).astype(np.uint8)
    fr = frames_of(clip)
    for p in (0, 1):
        v = fr.field(p)
        assert (v.H, v.W, v.T, v.interlaced, fr.interlaced) == (22, 23, 3, True, False)
        got = v.host(1)
        assert np.array_equal(got, clip[1, p::2]) and np.shares_memory(got, clip)
    assert fr.woven().interlaced and fr.woven().H == 44


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_field_entries():
    C = _lib.C
    want = {"spei_fields_u8_in": 6, "spei_fields_u16_in": 7, "spei_fields_u8_out": 9, "spei_fields_u16_out": 10,
            "spei_yuv_fields_to_rgb_u8": 10, "spei_rgb_u8_to_yuv_fields": 8, "spei_yuv_fields_to_rgb_u16": 11, "spei_rgb_u16_to_yuv_fields": 9}
    for name, nargs in want.items():
        assert name in _lib.header_symbols(), name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, name
    assert _lib.SIGNATURES["spei_fields_u8_in"][1] == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    # the progressive conversions keep their signatures
    assert len(_lib.SIGNATURES["spei_yuv_to_rgb_u8"][1]) == 10 and len(_lib.SIGNATURES["spei_rgb_u8_to_yuv"][1]) == 8


# ---- the argument checks that need no device ------------------------------------------------------------------------------------------------
def test_fields_value_is_checked_before_the_frames():
    with pytest.raises(ValueError, match='fields must be None or "split"'):
        video.deblur_clip(None, None, fields="bob")
    with pytest.raises(ValueError, match=r"fields='split' with tiles="):
        video.deblur_clip(None, None, fields="split", tiles=(2, 2))
    with pytest.raises(ValueError, match=r"fields='split' with roi="):
        video.deblur_clip(None, None, fields="split", roi=(0, 0, 20, 20))
    assert video.check_fields(None) is None and video.check_fields("split") == "split"


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
def test_cli_fields_argument(tmp_path, capsys, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the model was loaded")
    monkeypatch.setattr(video, "load_model", boom)
    base = ["--input", str(tmp_path), "--output", str(tmp_path / "out"), "--model_path", "synthetic"]
    with pytest.raises(SystemExit) as e:
        video.main(base + ["--fields", "bob"])
    assert e.value.code not in (0, None)
    err = capsys.readouterr().err
    assert "--fields" in err and "auto" in err and "progressive" in err and "split" in err
    for other in (["--tiles", "2x2"], ["--roi", "0,0,20,20"]):
        with pytest.raises(SystemExit, match=r"--fields split with %s" % other[0]):
            video.main(base + ["--fields", "split"] + other)
    # auto on an It input with --tiles: refused once the header is read, before the model is loaded
    path = tmp_path / "in.y4m"
    with y4m.Y4MWriter(str(path), 24, 48, interlace="t") as w:
        for _ in range(2):
            w.write(np.zeros(w.frame_bytes, np.uint8))
    with pytest.raises(SystemExit, match=r"interlaced \(It\).*--tiles"):
        video.main(["--input", str(path), "--output", str(tmp_path / "o.y4m"), "--model_path", "synthetic", "--tiles", "2x2"])
    # with neither, the three values parse: the run gets as far as the model
    for value in ("auto", "progressive", "split"):
        with pytest.raises(AssertionError, match="the model was loaded"):
            video.main(["--input", str(path), "--output", str(tmp_path / "o.y4m"), "--model_path", "synthetic", "--fields", value])
