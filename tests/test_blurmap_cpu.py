"""Automatic blur mattes without a GPU: the numpy statement `blurmap_ref` against hand-computed cases (edges and ramps, flat frames,
the expansion, the lone cell's ramp, the box rule), `blurmap`'s parameters and its host rules for an empty matte and for the box
against the reference, the three entry points in the C-ABI header, the refusals of `deblur_clip` with the model None (each comes
before any frame is looked at) and of the command line before the model loads, and `--matte_params` parsing."""
import itertools

import numpy as np
import pytest

import blurmap_ref as BR
import matte_ref as MR
from speinet_amd import _lib, blurmap, build, video
from speinet_amd.blurmap import BlurParams
from speinet_amd.clip import grow_box

T, H, W = 8, 40, 60
FRAMES = np.zeros((T, H, W, 3), np.uint8)
LINEAR = (1, 2, 3, 4, 5, 6, 8, 10, 12)     # the widths that divide the edge's 120 levels: the integer ramp is linear


def _edge(width: int, axis: int, lo: int = 60, amp: int = 120, n: int = 64):
    """A gray [16,n,3] (axis 1) or [n,16,3] (axis 0) frame: `lo` up to `lo + amp` over `width` pixels from position 24 on."""
    line = lo + amp * np.clip(np.arange(n) - 24, 0, width) // width
    plane = np.broadcast_to(line[None, :], (16, n)) if axis == 1 else np.broadcast_to(line[:, None], (n, 16))
    return np.repeat(plane[..., None], 3, axis=2).astype(np.uint8)


def _ratio(width: int):
    """sum V / sum D of an isolated linear edge of `width` steps of s, by hand: step j has d = 9 s, and the box of 9 taps around it
    spans c_j = min(w - 1, j + 4) - max(0, j - 4) + 1 of the steps, so b = c_j s, and V = (81 - c_j^2) s^2 (never negative: c_j <= 9)."""
    c = [min(width - 1, j + 4) - max(0, j - 4) + 1 for j in range(width)]
    return sum(81 - v * v for v in c), 81 * width


# ---- the reference against hand-computed cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [1, 0])
def test_edges_and_ramps(axis):
    """A step edge and linear ramps of widths 1..12 in both directions.  Where integer division leaves the ramp linear the sums are
    the hand-computed ones; for w <= 5, where every box spans the whole edge, that is 1 - w^2 / 81; the verdict flips between the
    widths 4 and 5 at the default thr; the other direction sees nothing."""
    a, b = (0, 2) if axis == 1 else (2, 0)                 # the sums of the edge's direction, and the other's
    lit = {}
    for w in range(1, 13):
        f = _edge(w, axis)
        S = BR.cell_sums(f).sum((0, 1))
        assert S[b] == 0 and S[b + 1] == 0
        if w in LINEAR:
            s = 120 // w
            num, den = _ratio(w)
            assert S[a] == 16 * den * s * s and S[a + 1] == 16 * num * s * s, w       # 16 rows (columns) of the edge
            if w <= 5:
                assert S[a + 1] * 81 == S[a] * (81 - w * w), w                 # sum V / sum D = 1 - w^2 / 81
            else:
                assert S[a + 1] * 81 > S[a] * max(0, 81 - w * w), w            # a wider edge falls more slowly
        cells = BR.verdict(BR.cell_sums(f), *f.shape[:2])
        lit[w] = bool(cells.any())
        ch, cw = cells.shape
        assert not cells.reshape(-1)[[0, ch * cw - 1]].any()                    # the flat cells at either end
    assert [w for w in lit if lit[w]] == list(range(5, 13))
    # 1 - w^2 / 81 against thr / 256: w = 4 gives 0.802 and w = 5 gives 0.691 around 0.75
    assert 256 * (81 - 16) >= 192 * 81 and 256 * (81 - 25) < 192 * 81


def test_luma_and_clamp():
    f = np.array([[[255, 255, 255], [10, 20, 30], [4095, 5000, 65535]]], np.uint16)
    assert BR.luma(f.astype(np.uint8)[..., :2, :], 8).tolist() == [[255, (770 + 3000 + 870 + 128) >> 8]]
    assert BR.luma(f, 12)[0, 2] == 4095                    # a word above D reads as D
    Y = np.arange(12, dtype=np.int64).reshape(3, 4)
    Dh, Vh, Dv, Vv = BR.pixel_terms(Y)
    assert Dh[:, 0].tolist() == [0, 0, 0] and Dh[:, 1:].tolist() == [[81] * 3] * 3      # Y(y,-1) is Y(y,0)
    assert Dv[0].tolist() == [0] * 4 and (Dv[1:] == 81 * 16).all()
    assert (Vh == np.maximum(0, Dh - 9)).all()             # b = Y(y,3) - Y(y,0) = 3 wherever the window leaves the row on both sides


def test_flat_and_faint_frames_light_nothing():
    flat = np.full((40, 64, 3), 77, np.uint8)
    assert not BR.cells_of(flat[None])[0].any() and not BR.cells_of(flat[None], thr=257, flat=0)[0].any()      # sum D = 0 is never lit
    faint = flat.copy()
    faint[:, ::2] += 1                                     # adjacent differences of 1 level: below flat = 2, blurred or not
    cells, S = BR.cells_of(faint[None])
    assert (S[..., 0] > 0).all() and not cells.any()
    assert BR.cells_of(BR.box9(faint, 1)[None])[0].any() is np.False_
    # and lit once flat lets it through; not the first column of cells: Y(y,-1) is Y(y,0), so 240 of its 256 pixels differ
    assert BR.cells_of(faint[None], thr=257, flat=1)[0][:, :, 1:].all() and not BR.cells_of(faint[None], thr=257, flat=1)[0][:, :, 0].any()
    # partial cells: n < 256 pixels enter the floor
    px = BR.cell_pixels(40, 70)
    assert px.shape == (3, 5) and px[0, 0] == 256 and px[2, 4] == 8 * 6 and px.sum() == 40 * 70


def test_thr_extremes():
    rng = np.random.default_rng(5)
    f = rng.integers(0, 256, (3, 33, 47, 3)).astype(np.uint8)
    assert not BR.cells_of(f, thr=0, flat=0)[0].any()
    cells, S = BR.cells_of(f, thr=257, flat=0)
    assert (S[..., 0] > 0).all() and cells.all()
    gray = np.repeat(f[..., :1], 3, axis=3)                # the luma of a gray pixel is its level, at every depth
    c8, s8 = BR.cells_of(gray, 8, 128, 8)
    c12, s12 = BR.cells_of(gray.astype(np.uint16) << 4, 12, 128, 8)
    assert np.array_equal(s12, s8 * 256) and np.array_equal(c12, c8)           # the floor scales with the depth


def test_expansion():
    for h, w in ((1, 1), (20, 20), (33, 47), (48, 80)):
        ch, cw = BR.cell_shape(h, w)
        assert (BR.expand(np.full((ch, cw), 255), h, w) == 255).all() and (BR.expand(np.zeros((ch, cw)), h, w) == 0).all()
    rng = np.random.default_rng(9)
    for _ in range(20):                                    # monotone: a cell map that is nowhere smaller gives a matte that is nowhere smaller
        a = np.where(rng.random((3, 5)) < 0.4, 255, 0)
        b = np.maximum(a, np.where(rng.random((3, 5)) < 0.3, 255, 0))
        assert (BR.expand(b, 48, 80) >= BR.expand(a, 48, 80)).all()


def test_lone_cell_ramp():
    c = np.zeros((5, 5), np.uint8)
    c[2, 2] = 255
    m = BR.expand(c, 80, 80)
    # by hand: the cell spans 32..47, its centre lies at 39.5, and the weight of the cell at pixel x is a(x) = 32 - |2 x - 79| thirty-
    # seconds where that is positive: 1 at x = 24, 31 at x = 39 and x = 40, 1 at x = 55, nothing at 23 and 56
    a = np.maximum(0, 32 - np.abs(2 * np.arange(80) - 79))
    assert a[23] == 0 and a[24] == 1 and a[39] == a[40] == 31 and a[55] == 1 and a[56] == 0
    assert np.array_equal(m, (a[:, None] * a[None, :] * 255 + 512) // 1024)
    row = m[40].astype(int)
    assert (np.diff(row[24:40]) > 0).all() and (np.diff(row[40:56]) < 0).all()  # the ramp to an unlit cell's centre: 16 pixels wide
    assert row[24] == 8 and row[39] == row[40] == (31 * 31 * 255 + 512) // 1024 > 0 and row[23] == row[56] == 0
    lit = np.argwhere(m)
    assert lit.min() == 32 - 8 and lit.max() == 48 + 8 - 1                      # exactly 0 beyond 8 pixels past the cell
    d = BR.dilate(c, 1)
    assert d[1:4, 1:4].all() and d.sum() == 9 * 255 and BR.dilate(c, 0).sum() == 255 and BR.dilate(c, 4).all()
    assert np.array_equal(BR.cell_map(np.stack([c, np.roll(c, 1, 1)]), 0), np.maximum(c, np.roll(c, 1, 1)))


def test_box_rule_covers_every_lit_pixel():
    """Every one- and two-cell map of a 3x5 grid, expanded: no matte pixel outside the box is lit, and the box is tight."""
    h, w = 40, 72                                          # partial cells at the bottom and the right
    cellsat = list(itertools.product(range(3), range(5)))
    for picks in itertools.chain(itertools.combinations(cellsat, 1), itertools.combinations(cellsat, 2)):
        c = np.zeros((3, 5), np.uint8)
        for p in picks:
            c[p] = 255
        m = BR.expand(c, h, w)
        ya, yb, xa, xb = BR.cell_box(c, h, w)
        out = m.copy()
        out[ya:yb, xa:xb] = 0
        assert not out.any(), picks
        assert m[ya].any() and m[yb - 1].any() and m[:, xa].any() and m[:, xb - 1].any(), picks
        assert BR.empty(c) is False
    assert BR.cell_box(np.zeros((3, 5)), h, w) is None and BR.empty(np.zeros((3, 5)))


# ---- blurmap: parameters and host rules ---------------------------------------------------------------------------------------------------
def test_blur_params():
    p = BlurParams()
    assert (p.thr, p.flat, p.grow, p.hold) == (192, 2, 1, 1) and blurmap.MATTE_PARAMS == ("thr", "flat", "grow", "hold")
    assert BlurParams.of(None) == p and BlurParams.of(dict(thr=0, flat=255, grow=4, hold=0)) == BlurParams(0, 255, 4, 0)
    assert BlurParams.of(dict(thr=np.int64(257))).thr == 257
    for kw, text in ((dict(thr=-1), "thr must be a whole number in 0..257"), (dict(thr=258), "thr must be"), (dict(flat=256), "flat must be a whole number in 0..255"),
                     (dict(grow=5), "grow must be a whole number in 0..4"), (dict(hold=2), "hold must be a whole number in 0..1"),
                     (dict(hold=True), "hold must be"), (dict(thr=1.5), "thr must be"), (dict(flat="2"), "flat must be")):
        with pytest.raises(ValueError, match=text):
            BlurParams.of(kw)
    with pytest.raises(ValueError, match=r"matte_params holds \['gain'\]: it takes thr, flat, grow and hold"):
        BlurParams.of(dict(gain=2))
    with pytest.raises(ValueError, match="must be a dict"):
        BlurParams.of([192])
    assert blurmap.cell_shape(48, 80) == (3, 5) == BR.cell_shape(48, 80) and blurmap.cell_shape(1, 17) == (1, 2)


def test_parse_params():
    assert blurmap.parse_params("thr=192,flat=2,grow=1,hold=1") == dict(thr=192, flat=2, grow=1, hold=1)
    assert blurmap.parse_params(" grow = 0 ") == dict(grow=0)
    for text, why in (("thr", "is not NAME=N"), ("gain=3", "is not NAME=N"), ("thr=x", "is not NAME=N"), ("thr=1,thr=2", "thr is given twice"),
                      ("thr=1,,flat=2", "is not NAME=N")):
        with pytest.raises(ValueError, match=why):
            blurmap.parse_params(text)


def test_host_empty_and_box_against_the_reference():
    """`blurmap.empty` and `blurmap.cell_box` decide from the VERDICT maps what the reference decides from the held and dilated cell
    maps: random clips, every grow, with and without the hold."""
    rng = np.random.default_rng(11)
    h, w = 40, 72
    for trial in range(40):
        t = 6
        cells = np.where(rng.random((t, 3, 5)) < (0.08 if trial % 2 else 0.0 if trial == 0 else 0.02), 255, 0).astype(np.uint8)
        plan = video.window_plan(np.zeros(t, np.int64))
        for grow, hold in itertools.product((0, 1, 2, 4), (0, 1)):
            cmaps = BR.clip_cell_maps(cells, plan, grow, hold)
            for k in range(t):
                assert blurmap.empty(cells, plan[k]["window"], hold, k) == BR.empty(cmaps[k]) == (not BR.expand(cmaps[k], h, w).any())
            box = blurmap.cell_box(cells, h, w, grow)
            assert box == BR.cell_box(cmaps, h, w)
            mask = np.zeros((h, w), np.uint8)
            if box is not None:
                mask[box[0]:box[1], box[2]:box[3]] = 1
            assert grow_box(box, h, w) == MR.bbox(mask, h, w)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries():
    C = _lib.C
    for name, n in (("spei_blur_cells_u8", 10), ("spei_blur_cells_u16", 11), ("spei_blur_matte", 8)):
        assert name in _lib.header_symbols()
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n and args[-1] is C.c_void_p
    assert _lib.SIGNATURES["spei_blur_cells_u8"][1][:5] == [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int]
    assert "blur_map.hip" in build.sources()


# ---- deblur_clip's checks ---------------------------------------------------------------------------------------------------------------
class _NoFrames:
    """A clip that fails the test when anything looks at it."""

    def __len__(self):
        raise AssertionError("the frames were looked at")

    __getitem__ = __iter__ = __len__


def test_deblur_clip_refusals_come_before_the_frames():
    for kw, text in ((dict(matte="auto", fields="split"), r"matte=\"auto\" with fields='split' is not built"),
                     (dict(matte="auto", matte_invert=True), r"matte=\"auto\" with matte_invert=True"),
                     (dict(matte_params=dict(thr=1)), r"matte_params= needs matte=\"auto\""),
                     (dict(matte=np.zeros((H, W), np.uint8), matte_params={}), r"matte_params= needs matte=\"auto\""),
                     (dict(matte="auto", roi="matte", stream=True), r"roi=\"matte\" with stream=True and matte=\"auto\""),
                     (dict(matte="auto", matte_params=dict(gain=1)), r"matte_params holds \['gain'\]"),
                     (dict(matte="auto", matte_params=dict(grow=9)), "grow must be a whole number in 0..4")):
        with pytest.raises(ValueError, match=text):
            video.deblur_clip(None, _NoFrames(), **kw)
    # what passes the checks fails where `ClipRun` looks at the model
    for frames, kw in ((FRAMES, dict(matte="auto")), (FRAMES, dict(matte="auto", matte_params=dict(hold=0), roi="matte")),
                       (iter(list(FRAMES)), dict(matte="auto", stream=True))):
        with pytest.raises(AttributeError, match="parameters"):
            video.deblur_clip(None, frames, **kw)


def test_cli_refusals_before_the_model_loads(monkeypatch, tmp_path):
    def boom(*a, **k):
        raise AssertionError("the model was loaded")
    monkeypatch.setattr(video, "load_model", boom)
    from PIL import Image
    src = tmp_path / "in"
    src.mkdir()
    for i in range(2):
        Image.fromarray(FRAMES[i]).save(src / f"f{i}.png")
    head = ["--input", str(src), "--output", str(tmp_path / "out"), "--model_path", "synthetic"]
    for extra, text in ((["--matte_params", "thr=1"], "--matte_params: needs --matte auto"),
                        (["--matte", "auto", "--matte_params", "thr=300"], "--matte_params: matte_params: thr must be"),
                        (["--matte", "auto", "--matte_params", "gain=1"], "--matte_params: 'gain=1' is not NAME=N"),
                        (["--matte", "auto", "--matte_invert"], "--matte auto with --matte_invert"),
                        (["--matte", "auto", "--fields", "split"], "--matte auto with --fields split"),
                        (["--matte_out", str(tmp_path / "m.y4m")], "--matte_out: needs --matte"),
                        (["--matte", "auto", "--matte_out", str(tmp_path / "m.png")], "--matte_out .*m.png: the mattes are written as one Cmono"),
                        (["--matte", "auto", "--roi", "matte", "--stream"], "--roi matte with --stream")):
        with pytest.raises(SystemExit, match=text):
            video.main(head + extra)
    assert not (tmp_path / "out").exists() and not (tmp_path / "m.y4m").exists()
