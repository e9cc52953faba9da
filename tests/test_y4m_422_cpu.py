"""CPU suite for 4:2:2 and mono y4m clips: `y4m.frame_bytes`, the reader's `layouts=` opt-in and the writer (speinet_amd/y4m.py); the
numpy restatement of the two layouts (tests/yuv422_ref.py, the reference of the kernel tests) against the 4:2:0 / 4:4:4 restatements
it must agree with on special frames, against float64 and against itself, at 8, 10 and 12 bits; and the command line's refusals."""
import io

import numpy as np
import pytest

import yuv16_ref as R16
import yuv422_ref as R
from speinet_amd import video, y4m

SIZES = [(1, 1), (3, 2), (5, 7), (6, 8), (20, 24), (37, 53)]
MODES = [(m, r) for m in (R.BT601, R.BT709) for r in (R.FULL, R.LIMITED)]
TAGS = [("422", y4m.P422, 8), ("422p10", y4m.P422, 10), ("422p12", y4m.P422, 12), ("mono", y4m.MONO, 8), ("mono10", y4m.MONO, 10),
        ("mono12", y4m.MONO, 12)]


def _rng(*key):
    return np.random.default_rng([int.from_bytes(str(k).encode(), "little") % (1 << 32) for k in key])


def _rgb(g, h, w, depth):
    return g.integers(0, 1 << depth, (h, w, 3)).astype(R.dtype_of(depth))


# ---- 1. y4m.py ---------------------------------------------------------------------------------------------------------------------------
def test_constants_and_frame_bytes():
    assert (y4m.P422, y4m.MONO, R.P422, R.MONO) == (3, 4, 3, 4) and y4m.LAYOUTS == (y4m.CENTER, y4m.LEFT, y4m.P444, y4m.P422, y4m.MONO)
    assert y4m.frame_bytes(3, 5, y4m.P422) == 33 and y4m.frame_bytes(3, 5, y4m.MONO) == 15 and y4m.frame_bytes(8, 7, y4m.P422) == 120
    for d in (10, 12):
        assert y4m.frame_bytes(3, 5, y4m.P422, d) == 66 and y4m.frame_bytes(3, 5, y4m.MONO, d) == 30 and y4m.frame_bytes(8, 7, y4m.P422, d) == 240
    for h, w in SIZES:
        for lay in (y4m.P422, y4m.MONO):
            assert y4m.frame_bytes(h, w, lay) == R.frame_samples(h, w, lay)
    for tag, lay, d in TAGS:
        assert y4m.chroma_tag(lay, d) == tag
    assert y4m.layout_of("422") == y4m.P422 and y4m.layout_of("mono") == y4m.MONO and y4m.layout_of(4) == y4m.MONO
    with pytest.raises(ValueError):
        y4m.layout_of("411")
    with pytest.raises(ValueError):
        y4m.frame_bytes(4, 4, 5)


@pytest.mark.parametrize("tag, layout, depth", TAGS)
def test_round_trip_of_the_six_tags(tag, layout, depth):
    h, w, T = 5, 7, 3
    g = _rng("rt", tag)
    ns = R.frame_samples(h, w, layout)
    frames = [g.integers(0, 1 << depth, ns).astype("u1" if depth == 8 else "<u2") for _ in range(T)]
    f = io.BytesIO()
    with y4m.Y4MWriter(f, w, h, (30000, 1001), layout, y4m.FULL, (1, 1), depth=depth) as wr:
        assert (wr.chroma, wr.frame_bytes) == (tag, ns * (1 if depth == 8 else 2))
        for fr in frames:
            wr.write(fr)
        with pytest.raises(ValueError, match="bytes"):
            wr.write(np.zeros(wr.frame_bytes + 1, np.uint8))
    scss = f" XYSCSS={tag.upper()}" if depth > 8 and layout == y4m.P422 else ""
    assert f.getvalue().split(b"\n", 1)[0] == f"YUV4MPEG2 W7 H5 F30000:1001 Ip A1:1 C{tag}{scss} XCOLORRANGE=FULL".encode()
    r = y4m.Y4MReader(f, depths=y4m.DEPTHS, layouts=y4m.LAYOUTS)
    nb = y4m.frame_bytes(h, w, layout, depth)
    assert (r.width, r.height, r.fps, r.aspect, r.layout, r.depth, r.chroma, r.range, r.frame_bytes, len(r)) == \
           (w, h, (30000, 1001), (1, 1), layout, depth, tag, y4m.FULL, nb, T)
    for i, fr in enumerate(frames):
        raw = r.raw(i)
        assert raw.dtype == np.uint8 and raw.shape == (nb,) and np.array_equal(raw.view(fr.dtype), fr)
    # a reader that takes this layout and depth only
    only = y4m.Y4MReader(f, depths=(depth,), layouts=(layout,))
    assert (only.layout, only.depth, len(only)) == (layout, depth, T)
    # the default readers still refuse the stream, with the tag named and today's hint
    for kw in ({}, {"depths": y4m.DEPTHS}, {"depths": (depth,)}):
        with pytest.raises(ValueError) as e:
            y4m.Y4MReader(f, **kw)
        assert f"C{tag}" in str(e.value) and "-pix_fmt yuv420p -f yuv4mpegpipe" in str(e.value)
    # the layouts are an opt-in of their own: without the depth the deep tags stay refused
    if depth > 8:
        with pytest.raises(ValueError, match=f"C{tag}: {depth} bits per sample"):
            y4m.Y4MReader(f, layouts=y4m.LAYOUTS)
    # the wider reader reads the old tags as before
    g8 = io.BytesIO()
    with y4m.Y4MWriter(g8, w, h, layout=y4m.LEFT) as w8:
        w8.write(np.zeros(y4m.frame_bytes(h, w, y4m.LEFT), np.uint8))
    r8 = y4m.Y4MReader(g8, depths=y4m.DEPTHS, layouts=y4m.LAYOUTS)
    assert (r8.layout, r8.depth, r8.chroma, len(r8)) == (y4m.LEFT, 8, "420mpeg2", 1)


@pytest.mark.parametrize("tag", ["411", "420paldv", "440", "420p9", "422p9", "422p14", "422p16", "444p16", "mono9", "mono14", "mono16"])
def test_still_refused_by_every_reader(tag):
    f = io.BytesIO(f"YUV4MPEG2 W4 H4 C{tag}\nFRAME\n".encode() + bytes(64))
    for kw in ({}, {"depths": y4m.DEPTHS}, {"layouts": y4m.LAYOUTS}, {"depths": y4m.DEPTHS, "layouts": y4m.LAYOUTS}):
        with pytest.raises(ValueError) as e:
            y4m.Y4MReader(f, **kw)
        assert f"C{tag}" in str(e.value), kw


def test_interlaced_and_bad_layout_arguments():
    for kw in ({}, {"depths": y4m.DEPTHS, "layouts": y4m.LAYOUTS}):
        with pytest.raises(ValueError, match="It"):
            y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4 It C422\n"), **kw)
    with pytest.raises(ValueError, match="chroma layout"):
        y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4\n"), layouts=(0, 7))
    # a reader without the 4:2:0 layouts refuses them
    with pytest.raises(ValueError, match="C420jpeg"):
        y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4 C420jpeg\n"), layouts=(y4m.P422,))
    r = video.frames_of(y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W24 H20 C422p10\n" + 2 * (b"FRAME\n" + bytes(2 * 960))), depths=y4m.DEPTHS,
                                      layouts=y4m.LAYOUTS))
    assert (r.yuv, r.depth, r.T, r.H, r.W) == ((y4m.P422, y4m.BT601, y4m.LIMITED), 10, 2, 20, 24)


# ---- 2. the restatement ------------------------------------------------------------------------------------------------------------------
def test_tables_are_the_rule():
    for d in R.DEPTHS:
        for m, r in MODES:
            assert tuple(R.coef(d, m, r).values()) == R16.rule(d, m, r), (d, m, r)


def _planes(planar, h, w, layout, depth):
    """Y, U, V of a frame in any of the five layouts."""
    if layout in (R.P422, R.MONO):
        return R.split(planar, h, w, layout, depth)
    ch, cw = R16.chroma_shape(h, w, layout)
    p = np.asarray(planar).reshape(-1).astype(np.int64)
    return p[:h * w].reshape(h, w), p[h * w:h * w + ch * cw].reshape(ch, cw), p[h * w + ch * cw:].reshape(ch, cw)


@pytest.mark.parametrize("depth", R.DEPTHS)
@pytest.mark.parametrize("h, w", SIZES)
def test_identities_1_2_3_5(depth, h, w):
    g = _rng("id", depth, h, w)
    D, s = (1 << depth) - 1, depth - 8
    for m, r in MODES:
        # 1. every row one colour: the 4:2:2 chroma planes are the even columns of the 4:4:4 planes, and the RGB made back is the
        #    4:4:4 round trip
        rows = np.repeat(_rgb(g, h, 1, depth), w, axis=1)
        p422, p444 = R.rgb_to_yuv(rows, R.P422, m, r, depth), R.old_rgb_to_yuv(rows, R.P444, m, r, depth)
        y2, u2, v2 = _planes(p422, h, w, R.P422, depth)
        y4, u4, v4 = _planes(p444, h, w, R.P444, depth)
        assert np.array_equal(y2, y4) and np.array_equal(u2, u4[:, ::2]) and np.array_equal(v2, v4[:, ::2])
        back = R.yuv_to_rgb(p422, h, w, R.P422, m, r, depth)
        assert np.array_equal(back, R.old_yuv_to_rgb(p444, h, w, R.P444, m, r, depth))
        # ... and that round trip is within the 4:4:4 bound
        assert int(np.abs(back.astype(np.int64) - rows).max()) <= (1 if r == R.FULL else 2)
        # 2. all rows equal: the even chroma rows of 4:2:2 are LEFT's planes, and the RGB made back is LEFT's
        cols = np.repeat(_rgb(g, 1, w, depth), h, axis=0)
        p422, pleft = R.rgb_to_yuv(cols, R.P422, m, r, depth), R.old_rgb_to_yuv(cols, R.LEFT, m, r, depth)
        y2, u2, v2 = _planes(p422, h, w, R.P422, depth)
        yl, ul, vl = _planes(pleft, h, w, R.LEFT, depth)
        assert np.array_equal(y2, yl) and np.array_equal(u2[::2], ul) and np.array_equal(v2[::2], vl)
        assert np.array_equal(R.yuv_to_rgb(p422, h, w, R.P422, m, r, depth), R.old_yuv_to_rgb(pleft, h, w, R.LEFT, m, r, depth))
        # 3. gray stays gray
        gray = np.repeat(g.integers(0, D + 1, (h, w, 1)), 3, axis=2).astype(R.dtype_of(depth))
        _, u, v = _planes(R.rgb_to_yuv(gray, R.P422, m, r, depth), h, w, R.P422, depth)
        assert (u == 128 << s).all() and (v == 128 << s).all()
        # 5. mono in is 4:4:4 in with both chroma planes at the chroma zero; mono out is the Y plane of 4:4:4 out
        yp = g.integers(0, D + 1, h * w).astype(R.dtype_of(depth))
        as444 = np.concatenate([yp, np.full(2 * h * w, 128 << s, yp.dtype)])
        got = R.yuv_to_rgb(yp, h, w, R.MONO, m, r, depth)
        assert np.array_equal(got, R.old_yuv_to_rgb(as444, h, w, R.P444, m, r, depth))
        assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
        assert np.array_equal(got, R.yuv_to_rgb(yp, h, w, R.MONO, 1 - m, r, depth))                       # the matrix has no effect
        rgb = _rgb(g, h, w, depth)
        assert np.array_equal(R.rgb_to_yuv(rgb, R.MONO, m, r, depth), R.old_rgb_to_yuv(rgb, R.P444, m, r, depth)[:h * w])


def _float_rgb(y, u, v, depth, matrix, rng):
    """The conversion in float64, unrounded, clipped to [0, D] (tests/test_y4m_deep_cpu.py, any depth)."""
    s, D = depth - 8, (1 << depth) - 1
    kr, kb = (float(x) for x in R16.KR_KB[matrix])
    kg = 1 - kr - kb
    ly, lc, yo = (1.0, 1.0, 0.0) if rng == R.FULL else ((219 << s) / D, (224 << s) / D, float(16 << s))
    yy, cu, cv = (y - yo) / ly, (u - (128 << s)) / lc, (v - (128 << s)) / lc
    rgb = np.stack([yy + 2 * (1 - kr) * cv, yy - (2 * kb * (1 - kb) * cu + 2 * kr * (1 - kr) * cv) / kg, yy + 2 * (1 - kb) * cu], axis=-1)
    return np.clip(rgb, 0, D)


@pytest.mark.parametrize("depth", R.DEPTHS)
def test_identity_4_against_float64(depth):
    """4:2:2 YUV -> RGB against float64 with the same linear interpolation: within 1 code (0.504 measured at 8 bits on 37x53)."""
    worst = 0.0
    for h, w in SIZES:
        g = _rng("f64", depth, h, w)
        for m, r in MODES:
            planar = g.integers(0, 1 << depth, R.frame_samples(h, w, R.P422)).astype(R.dtype_of(depth))
            y, u, v = (a.astype(np.float64) for a in R.split(planar, h, w, R.P422, depth))
            x = np.arange(w)
            i, i1 = x >> 1, np.minimum((x >> 1) + 1, u.shape[1] - 1)
            uf = np.where(x % 2 == 0, u[:, i], (u[:, i] + u[:, i1]) / 2)
            vf = np.where(x % 2 == 0, v[:, i], (v[:, i] + v[:, i1]) / 2)
            err = float(np.abs(R.yuv_to_rgb(planar, h, w, R.P422, m, r, depth).astype(np.float64) - _float_rgb(y, uf, vf, depth, m, r)).max())
            worst = max(worst, err)
            assert err <= 1.0, (h, w, m, r, err)
    print(f"depth {depth}: max |int - float64| {worst:.3f}")


def test_words_above_the_depth_read_as_the_maximum():
    h, w = 5, 7
    for d in (10, 12):
        D = (1 << d) - 1
        g = _rng("words", d)
        for lay in (R.P422, R.MONO):
            planar = g.integers(D + 1, 65536, R.frame_samples(h, w, lay)).astype(np.uint16)
            assert np.array_equal(R.yuv_to_rgb(planar, h, w, lay, R.BT601, R.LIMITED, d),
                                  R.yuv_to_rgb(np.full_like(planar, D), h, w, lay, R.BT601, R.LIMITED, d))
            rgb = g.integers(0, 65536, (h, w, 3)).astype(np.uint16)
            assert np.array_equal(R.rgb_to_yuv(rgb, lay, R.BT709, R.FULL, d), R.rgb_to_yuv(np.minimum(rgb, D), lay, R.BT709, R.FULL, d))


# ---- 3. command line ----------------------------------------------------------------------------------------------------------------------
def test_cli_refusals(tmp_path, capsys):
    base = ["--input", str(tmp_path / "in.y4m"), "--model_path", "synthetic"]
    with pytest.raises(SystemExit) as e:                              # before the input is opened and the model is loaded
        video.main(base + ["--output", str(tmp_path / "png"), "--out_chroma", "422"])
    assert "--out_chroma 422" in str(e.value) and "PNG directory" in str(e.value)
    for flag in ("--out_chroma", "--chroma"):
        for tag in ("411", "440", "422p10", "yuv422p"):
            with pytest.raises(SystemExit) as e:
                video.main(base + ["--output", str(tmp_path / "out.y4m"), flag, tag])
            assert e.value.code == 2
            err = capsys.readouterr().err
            assert "invalid choice" in err and tag in err and "'422'" in err and "'mono'" in err
