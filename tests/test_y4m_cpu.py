"""CPU suite for y4m clips: the numpy restatement of the planar-YUV conversions (tests/yuv_ref.py, the reference of the kernel tests)
against Pillow and against itself, and the YUV4MPEG2 reader and writer (speinet_amd/y4m.py)."""
import io
import os

import numpy as np
import pytest

import yuv_ref as R
from speinet_amd import y4m

TABLES = [(m, r) for m in (R.BT601, R.BT709) for r in (R.FULL, R.LIMITED)]


def _triples():
    """All 2^24 RGB triples, 2^20 at a time: uint8 [2^20, 3]."""
    gb = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), axis=-1).reshape(-1, 2)
    for r0 in range(0, 256, 16):
        r = np.repeat(np.arange(r0, r0 + 16), 65536)
        yield np.concatenate([r[:, None], np.tile(gb, (16, 1))], axis=1).astype(np.uint8)


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------------------
def test_constants_match_the_modules():
    assert (R.CENTER, R.LEFT, R.P444, R.BT601, R.BT709, R.FULL, R.LIMITED) == \
           (y4m.CENTER, y4m.LEFT, y4m.P444, y4m.BT601, y4m.BT709, y4m.FULL, y4m.LIMITED)
    for (m, r), row in R.TABLE.items():
        k = R.coef(m, r)
        assert k["ur"] + k["ug"] + k["ub"] == 0 and k["vr"] + k["vg"] + k["vb"] == 0
        assert k["yr"] + k["yg"] + k["yb"] == (16384 if r == R.FULL else round(16384 * 219 / 255))
        assert k["yo"] == (0 if r == R.FULL else 16)


def test_restatement_against_pillow_all_triples():
    """Pillow's RGB <-> YCbCr is JFIF: BT.601, full range, 4:4:4.  Every channel within 1 (Pillow truncates where this rounds)."""
    from PIL import Image
    worst = [0, 0]
    for t in _triples():
        img = t.reshape(1024, 1024, 3)
        pil = np.asarray(Image.fromarray(img, "RGB").convert("YCbCr")).astype(np.int64)
        y, u, v = R.rgb_to_yuv_values(img, R.BT601, R.FULL)
        worst[0] = max(worst[0], int(np.abs(np.stack([y, u, v], axis=-1) - pil).max()))
        back = np.asarray(Image.fromarray(img, "YCbCr").convert("RGB")).astype(np.int64)       # the triple read as (Y, Cb, Cr)
        i = img.astype(np.int64)
        mine = R.yuv_to_rgb_values(i[..., 0], 16 * i[..., 1], 16 * i[..., 2], R.BT601, R.FULL).astype(np.int64)
        worst[1] = max(worst[1], int(np.abs(mine - back).max()))
    print(f"max |restatement - Pillow|: RGB->YCbCr {worst[0]}, YCbCr->RGB {worst[1]}")
    assert worst[0] <= 1 and worst[1] <= 1


@pytest.mark.parametrize("matrix, rng", TABLES)
def test_444_round_trip_all_triples(matrix, rng):
    """RGB -> YUV -> RGB at 4:4:4 over all 2^24 triples: at most 1 in full range, at most 2 in limited range."""
    worst = 0
    for t in _triples():
        y, u, v = R.rgb_to_yuv_values(t, matrix, rng)
        back = R.yuv_to_rgb_values(y, 16 * u, 16 * v, matrix, rng).astype(np.int64)
        worst = max(worst, int(np.abs(back - t.astype(np.int64)).max()))
    print(f"matrix {matrix} range {rng}: max round-trip error {worst}")
    assert worst <= (1 if rng == R.FULL else 2)


@pytest.mark.parametrize("matrix, rng", TABLES)
def test_gray_has_neutral_chroma(matrix, rng):
    g = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    _, u, v = R.rgb_to_yuv_values(g, matrix, rng)
    assert (u == 128).all() and (v == 128).all()
    img = np.broadcast_to(g[:, None, :], (256, 7, 3))               # 256 x 7: one gray per row, odd width
    for layout in (R.CENTER, R.LEFT, R.P444):
        p = R.rgb_to_yuv(img, layout, matrix, rng)
        assert (p[256 * 7:] == 128).all(), layout
    flat = np.full((5, 9, 3), 93, np.uint8)                         # a flat gray frame survives every layout exactly or within the 4:4:4 bound
    for layout in (R.CENTER, R.LEFT, R.P444):
        back = R.yuv_to_rgb(R.rgb_to_yuv(flat, layout, matrix, rng), 5, 9, layout, matrix, rng).astype(np.int64)
        assert np.abs(back - 93).max() <= (1 if rng == R.FULL else 2)
        assert (back == back[0, 0, 0]).all()


@pytest.mark.parametrize("layout", [R.CENTER, R.LEFT])
@pytest.mark.parametrize("h, w", [(1, 1), (3, 5), (8, 8), (21, 23)])
def test_constant_chroma_upsamples_to_constant(layout, h, w):
    ch, cw = R.chroma_shape(h, w, layout)
    for c in (0, 1, 77, 128, 255):
        assert (R.upsample16(np.full((ch, cw), c), h, w, layout) == 16 * c).all()
    # and the weights are the stated ones: a lone sample spreads 3 : 1 (9 3 3 1 over 16), LEFT columns 4 : 0 / 2 : 2
    if (h, w) == (8, 8):
        c = np.zeros((4, 4), np.int64)
        c[1, 1] = 16
        up = R.upsample16(c, 8, 8, layout)
        assert up.sum() == 16 * 16 * 4                                    # each sample feeds 4 pixels' worth of weight
        assert up[2, 2] == (9 * 16 if layout == R.CENTER else 12 * 16) and up[1, 2] == (3 * 16 if layout == R.CENTER else 4 * 16)
        assert up[2, 3] == (9 * 16 if layout == R.CENTER else 6 * 16) and up[2, 1] == (3 * 16 if layout == R.CENTER else 6 * 16)


def test_downsampling_rules_by_hand():
    """4:2:0 chroma of a 2x4 frame by hand: CENTER is the 2x2 box, LEFT the [1 2 1] filter centred on the even column, edges clamped."""
    rgb = np.zeros((2, 4, 3), np.uint8)
    rgb[:, 1] = (255, 0, 0)                                           # one red column at x = 1
    k = R.coef(R.BT601, R.FULL)
    for layout, sums, shift in ((R.CENTER, (2 * 255, 0), 16), (R.LEFT, (2 * 255, 2 * 255), 17)):
        p = R.rgb_to_yuv(rgb, layout, R.BT601, R.FULL)
        assert p.size == 8 + 2 * 2
        for i, s in enumerate(sums):
            assert p[8 + i] == ((k["ur"] * s + (1 << (shift - 1))) >> shift) + 128
            assert p[10 + i] == min(((k["vr"] * s + (1 << (shift - 1))) >> shift) + 128, 255)


# ---- 2. the reader and the writer ------------------------------------------------------------------------------------------------------
def _stream(header: bytes, frames, line=b"FRAME\n") -> bytes:
    lines = line if isinstance(line, (list, tuple)) else [line] * len(frames)
    return header + b"".join(ln + bytes(f) for ln, f in zip(lines, frames))


def _payloads(n, nbytes, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, nbytes, dtype=np.uint8) for _ in range(n)]


def test_reader_tags_in_any_order_and_frame_parameters():
    fr = _payloads(3, 6 * 4 + 2 * 3 * 2)
    data = _stream(b"YUV4MPEG2 C420mpeg2 XYSCSS=420MPEG2 A4:3 Ip F30000:1001 H4 XCOLORRANGE=FULL W6\n", fr, b"FRAME Ip Xfoo=1\n")
    r = y4m.Y4MReader(io.BytesIO(data))
    assert (r.width, r.height, r.fps, r.aspect, r.layout, r.range, r.matrix) == (6, 4, (30000, 1001), (4, 3), y4m.LEFT, y4m.FULL, y4m.BT601)
    assert len(r) == 3 and r.frame_bytes == 36
    for i in (2, 0, 1):
        got = r.raw(i)
        assert got.dtype == np.uint8 and got.shape == (36,) and np.array_equal(got, fr[i])
    assert np.array_equal(r[-1], fr[2])
    with pytest.raises(IndexError):
        r.raw(3)


@pytest.mark.parametrize("w, h, tag, nbytes", [(5, 3, "420jpeg", 15 + 2 * 6), (5, 3, "444", 45), (1, 1, "420", 3), (7, 8, "420mpeg2", 56 + 32),
                                               (6, 5, "420jpeg", 30 + 18)])
def test_frame_bytes_of_odd_sizes(w, h, tag, nbytes):
    assert y4m.frame_bytes(h, w, y4m.LAYOUT_OF_TAG[tag]) == nbytes == R.frame_bytes(h, w, y4m.LAYOUT_OF_TAG[tag])
    fr = _payloads(2, nbytes)
    r = y4m.Y4MReader(io.BytesIO(_stream(f"YUV4MPEG2 W{w} H{h} F25:1 C{tag}\n".encode(), fr)))
    assert len(r) == 2 and r.frame_bytes == nbytes and np.array_equal(r.raw(1), fr[1])


def test_reader_defaults():
    r = y4m.Y4MReader(io.BytesIO(_stream(b"YUV4MPEG2 W4 H4\n", _payloads(1, 24))))
    assert (r.layout, r.range, r.matrix, r.fps, r.aspect, r.chroma) == (y4m.CENTER, y4m.LIMITED, y4m.BT601, (25, 1), None, "420jpeg")
    assert y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H719 F1:1 I? C420\n")).matrix == y4m.BT601
    hd = y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H720 F1:1 Ip C444 XCOLORRANGE=LIMITED\n"))
    assert (hd.matrix, hd.range, hd.layout, len(hd)) == (y4m.BT709, y4m.LIMITED, y4m.P444, 0)
    assert "ffmpeg" in y4m.Y4MReader.__doc__ and "no matrix tag" in y4m.Y4MReader.__doc__


@pytest.mark.parametrize("header, tag", [
    (b"YUV4MPEG2 W4 H4 F25:1 It C420jpeg\n", "It"), (b"YUV4MPEG2 W4 H4 F25:1 Ib\n", "Ib"), (b"YUV4MPEG2 W4 H4 Im\n", "Im"),
    (b"YUV4MPEG2 W4 H4 C420p10\n", "C420p10"), (b"YUV4MPEG2 W4 H4 C444p12\n", "C444p12"), (b"YUV4MPEG2 W4 H4 C422p16\n", "C422p16"),
    (b"YUV4MPEG2 W4 H4 Cmono16\n", "Cmono16"), (b"YUV4MPEG2 W4 H4 C420paldv\n", "C420paldv"), (b"YUV4MPEG2 W4 H4 C422\n", "C422"),
    (b"YUV4MPEG2 W4 H4 C411\n", "C411"), (b"YUV4MPEG2 W4 H4 Cmono\n", "Cmono"), (b"YUV4MPEG2 H4 F25:1 C420jpeg\n", "W tag"),
    (b"YUV4MPEG2 W4 F25:1 C420jpeg\n", "H tag")])
def test_reader_rejections_name_the_tag(header, tag):
    with pytest.raises(ValueError) as e:
        y4m.Y4MReader(io.BytesIO(_stream(header, _payloads(2, 24))))
    assert tag in str(e.value) and "ffmpeg" in str(e.value) and "-pix_fmt yuv420p -f yuv4mpegpipe" in str(e.value)


def test_reader_rejects_what_is_no_stream():
    for data in (b"", b"RIFF....", b"YUV4MPEG2 W4 H4 with no newline"):
        with pytest.raises(ValueError, match="not a YUV4MPEG2 stream"):
            y4m.Y4MReader(io.BytesIO(data))
    with pytest.raises(ValueError, match="no FRAME line"):
        y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4\n" + bytes(30)))


def test_truncated_file():
    fr = _payloads(3, 24)
    data = _stream(b"YUV4MPEG2 W4 H4 F25:1 C420jpeg\n", fr)
    for cut in (1, 24, 25, 29):                                       # inside the last payload, its whole payload, into its FRAME line
        with pytest.raises(ValueError, match="truncated"):
            y4m.Y4MReader(io.BytesIO(data[:-cut]))
    assert len(y4m.Y4MReader(io.BytesIO(data[:-30]))) == 2             # cut at a frame boundary: a shorter clip


def test_differing_frame_line_raises_when_that_frame_is_read():
    """Lines of 9, 6 and 12 bytes make three records' worth of bytes: the length gives nothing away, the second FRAME line does."""
    fr = _payloads(3, 24)
    r = y4m.Y4MReader(io.BytesIO(_stream(b"YUV4MPEG2 W4 H4 F25:1 C420jpeg\n", fr, [b"FRAME I1\n", b"FRAME\n", b"FRAME I1 X2\n"])))
    assert len(r) == 3 and np.array_equal(r.raw(0), fr[0])
    with pytest.raises(ValueError, match="FRAME line"):
        r.raw(1)


@pytest.mark.parametrize("layout, rng, aspect", [(y4m.CENTER, y4m.FULL, None), (y4m.LEFT, y4m.LIMITED, (16, 15)), (y4m.P444, y4m.FULL, (1, 1))])
def test_writer_reader_round_trip(tmp_path, layout, rng, aspect):
    w, h = 23, 21
    fr = _payloads(4, y4m.frame_bytes(h, w, layout), seed=layout)
    path = tmp_path / "clip.y4m"
    with y4m.Y4MWriter(path, w, h, (24000, 1001), layout, rng, aspect) as wr:
        assert wr.frame_bytes == len(fr[0])
        wr.write(fr[0])                                               # a numpy array,
        wr.write(bytes(fr[1]))                                        # bytes,
        wr.write(memoryview(fr[2]))                                   # a memoryview,
        wr.write(bytearray(fr[3]))                                    # a bytearray
        with pytest.raises(ValueError, match="bytes"):
            wr.write(fr[0][:-1])
    with y4m.Y4MReader(path) as r:
        assert (r.width, r.height, r.fps, r.aspect, r.layout, r.range, len(r)) == (w, h, (24000, 1001), aspect, layout, rng, 4)
        assert all(np.array_equal(r.raw(i), fr[i]) for i in range(4))
    buf = io.BytesIO()                                                # a file object stays open
    wr = y4m.Y4MWriter(buf, w, h, (25, 1), layout, rng)
    wr.write(fr[0])
    wr.close()
    assert not buf.closed and buf.getvalue().startswith(b"YUV4MPEG2 W23 H21 F25:1 Ip C") and os.path.getsize(path) > 4 * len(fr[0])
    assert np.array_equal(y4m.Y4MReader(buf).raw(0), fr[0])


def test_names_of_matrix_and_range():
    assert y4m.matrix_of("BT709") == y4m.BT709 == y4m.matrix_of(y4m.BT709) and y4m.range_of("full") == y4m.FULL
    for bad in ("bt2020", 7, None, True):
        with pytest.raises(ValueError):
            y4m.matrix_of(bad)


def test_module_needs_no_torch():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; import speinet_amd.y4m; assert 'torch' not in sys.modules, 'y4m imported torch'"
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_entry_points_declared():
    from speinet_amd import _lib
    from speinet_amd.build import sources
    I, L, P = _lib.C.c_int, _lib.C.c_int64, _lib.C.c_void_p
    assert _lib.SIGNATURES["spei_yuv_to_rgb_u8"] == (I, [P, L, P, I, I, I, I, I, I, P])
    assert _lib.SIGNATURES["spei_rgb_u8_to_yuv"] == (I, [P, P, I, I, I, I, I, P])
    assert "yuv_io.hip" in sources()
    text = open(_lib.HEADER_PATH).read()
    for name, value in (("SPEI_YUV_420_CENTER", y4m.CENTER), ("SPEI_YUV_420_LEFT", y4m.LEFT), ("SPEI_YUV_444", y4m.P444),
                        ("SPEI_YUV_BT601", y4m.BT601), ("SPEI_YUV_BT709", y4m.BT709), ("SPEI_YUV_FULL", y4m.FULL),
                        ("SPEI_YUV_LIMITED", y4m.LIMITED)):
        assert f"#define {name} {value}" in text, name
