"""Mattes of the clip API without a GPU: the blend's four properties in numpy (`matte_ref.blend`), the matte source `clip.mattes_of`
(what it takes and refuses, `empty`, `bbox` against `matte_ref.bbox`), the two entry points in the C-ABI header, the `deblur_clip`
argument checks with the model None (every refusal comes before the model is looked at), and the command line's refusals before
the model loads."""
import io

import numpy as np
import pytest
import torch

import matte_ref as MR
from speinet_amd import _lib, build, video, y4m
from speinet_amd.clip import grow_box, mattes_of

T, H, W = 8, 40, 60
FRAMES = np.zeros((T, H, W, 3), np.uint8)


# ---- the blend ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [255, 1023, 4095])
def test_blend_properties(D):
    """Over every m and a grid of a, b that holds the extremes: m = 0 is a, m = 255 is b, a == b is a for every m, and swapping a with b
    under the inverted matte changes nothing.  The value lies between a and b and never beyond D."""
    grid = np.unique(np.concatenate([np.arange(0, D + 1, max(1, D // 64)), [0, 1, 2, D // 2, D - 2, D - 1, D]]))
    a, b, m = np.meshgrid(grid, grid, np.arange(256), indexing="ij")

    def f(a, b, m, invert=False):
        return MR.blend(a[..., None, None], b[..., None, None], m[..., None], invert)[..., 0, 0]

    out = f(a, b, m)
    assert np.array_equal(out[..., 0], a[..., 0]) and np.array_equal(out[..., 255], b[..., 255])
    same = a == b
    assert np.array_equal(out[same], a[same])
    assert np.array_equal(out, f(b, a, 255 - m)) and np.array_equal(out, f(b, a, m, invert=True))
    assert np.array_equal(f(a, b, m, invert=True), f(a, b, 255 - m))
    assert (out >= np.minimum(a, b)).all() and (out <= np.maximum(a, b)).all() and out.max() == D and out.min() == 0
    assert int((a * (255 - m) + b * m + 127).max()) <= 4095 * 255 + 127
    # nearest to the exact value: the error of the integer statement is at most half a code
    exact = (a * (255 - m) + b * m) / 255.0
    assert np.abs(out - exact).max() <= 0.5


# ---- the matte source -----------------------------------------------------------------------------------------------------------------
def _png(path, a):
    from PIL import Image
    Image.fromarray(a).save(path)
    return str(path)


def test_mattes_of_takes_every_form(tmp_path):
    rng = np.random.default_rng(0)
    per = rng.integers(0, 256, (T, H, W)).astype(np.uint8)
    per[[0, 3, 4]] = 0
    one = per[1]
    forms = {"array": per, "tensor": torch.from_numpy(per), "list": list(per), "tensors": [torch.from_numpy(m) for m in per],
             "paths": [_png(tmp_path / f"m{i:02d}.png", m) for i, m in enumerate(per)], "dir": str(tmp_path)}
    f = io.BytesIO()
    wr = y4m.Y4MWriter(f, W, H, (25, 1), y4m.MONO, y4m.FULL)
    for m in per:
        wr.write(m.reshape(-1))
    (tmp_path / "m.y4m").write_bytes(f.getvalue())
    forms["y4m"] = str(tmp_path / "m.y4m")
    forms["reader"] = y4m.Y4MReader(str(tmp_path / "m.y4m"), layouts=y4m.LAYOUTS)
    for name, form in forms.items():
        mt = mattes_of(form, T, H, W)
        assert not mt.static and mt.T == T and (mt.H, mt.W) == (H, W), name
        assert [mt.empty(i) for i in range(T)] == [i in (0, 3, 4) for i in range(T)], name
        for i in range(T):
            got = mt.host(i)
            assert got.dtype == np.uint8 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, per[i]), (name, i)
        assert mt.bbox() == MR.bbox(per, H, W), name
    for name, form in {"array": one, "tensor": torch.from_numpy(one), "path": _png(tmp_path / "one.PNG", one)}.items():
        mt = mattes_of(form, T, H, W)
        assert mt.static and mt.T is None and not mt.empty(0) and not mt.empty(T - 1), name
        assert np.array_equal(mt.host(0), one) and np.array_equal(mt.host(T - 1), one) and mt.key(5) == 0, name
        assert mt.bbox() == MR.bbox(one, H, W), name
    # a stream's length is not known: nothing is measured against it
    assert mattes_of(per, None, H, W).T == T
    # an RGB image is read as one 8-bit channel
    from PIL import Image
    rgb = np.repeat(one[:, :, None], 3, axis=2)
    assert np.array_equal(mattes_of(_png(tmp_path / "rgb.png", rgb), T, H, W).host(0), np.asarray(Image.fromarray(rgb).convert("L")))


def test_bool_invert_and_crop():
    b = np.zeros((H, W), bool)
    b[5:9, 7:30] = True
    mt = mattes_of(b, T, H, W)
    assert np.array_equal(mt.host(0), b.astype(np.uint8) * 255) and not mt.empty(0)
    inv = mattes_of(np.full((H, W), 255, np.uint8), T, H, W, invert=True)
    assert inv.invert and inv.empty(0) and inv.bbox() is None and (inv.host(0) == 255).all()       # the bytes are handed out as given
    assert not mattes_of(np.zeros((H, W), np.uint8), T, H, W, invert=True).empty(0)
    # cropped as the frames are: 47x61 -> 40x60, a matte that is lit in the cropped margin only is empty
    m = np.zeros((T, 47, 61), np.uint8)
    m[0, 45, 3] = m[1, 2, 60] = 9
    m[2, 39, 59] = 1
    mt = mattes_of(m, T, 47, 61, crop=True)
    assert (mt.H, mt.W) == (40, 60) and mt.host(2).shape == (40, 60) and mt.host(2).flags["C_CONTIGUOUS"]
    assert [mt.empty(i) for i in range(3)] == [True, True, False]
    assert mt.bbox() == MR.bbox(m[:, :40, :60], 40, 60) == (19, 39, 21, 21)


def test_mattes_of_refusals(tmp_path):
    ok = np.zeros((T, H, W), np.uint8)
    cases = [(np.zeros((H, W + 1), np.uint8), r"shape \(40, 61\)"), (np.zeros((T, H - 1, W), np.uint8), r"shape \(39, 60\)"),
             (ok[:-1], "holds 7 mattes for a clip of 8 frames"), (list(ok) + [ok[0]], "holds 9 mattes for a clip of 8 frames"),
             (ok.astype(np.uint16), "uint8 or bool.*uint16"), (torch.zeros(H, W), "uint8 or bool.*float32"),
             (np.zeros((1, T, H, W), np.uint8), r"\[H,W\] \(static\) or \[T,H,W\]"),
             (list(ok[:-1]) + [np.zeros((H, W), np.int32)], "matte 7 is int32"), (list(ok[:-1]) + [None], "matte 7 is a NoneType"),
             (list(ok[:-1]) + ["x.png"], "mixes image paths and arrays"), (iter(ok), "an iterator of mattes is not built"),
             (7, "got int")]
    for matte, text in cases:
        with pytest.raises(ValueError, match=text):
            mattes_of(matte, T, H, W)
    with pytest.raises(ValueError, match="m.png.* is 61x40, the frames are 60x40"):
        mattes_of(_png(tmp_path / "m.png", np.zeros((40, 61), np.uint8)), T, H, W)
    with pytest.raises(ValueError, match="matte 1 .*b.png.* is 30x20"):
        mattes_of([_png(tmp_path / "a.png", ok[0]), _png(tmp_path / "b.png", np.zeros((20, 30), np.uint8))], 2, H, W)
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="holds no image file"):
        mattes_of(str(tmp_path / "empty"), T, H, W)
    for layout, depth, tag in ((y4m.MONO, 10, "Cmono10"), (y4m.CENTER, 8, "C420jpeg")):
        f = io.BytesIO()
        wr = y4m.Y4MWriter(f, W, H, (25, 1), layout, y4m.FULL, depth=depth)
        for _ in range(T):
            wr.write(np.zeros(y4m.frame_bytes(H, W, layout, depth), np.uint8))
        (tmp_path / f"{tag}.y4m").write_bytes(f.getvalue())
        with pytest.raises(ValueError, match=f"8-bit Cmono clip.*{tag}"):
            mattes_of(str(tmp_path / f"{tag}.y4m"), T, H, W)


def test_bbox_cases():
    def box(lit, **kw):
        m = np.zeros((3, H, W), np.uint8)
        for t, (ys, xs) in enumerate(lit):
            m[t, ys, xs] = 1 + t
        got = mattes_of(m, 3, H, W).bbox(**kw)
        assert got == MR.bbox(m, H, W, **kw)
        return got

    assert box([]) is None                                                                          # an empty matte
    assert box([(0, 0)]) == (0, 0, 21, 21) and box([(H - 1, W - 1)]) == (H - 21, W - 21, 21, 21)      # a single pixel in a corner
    assert box([(slice(0, 30), slice(45, W))]) == (0, 25, H, W - 25)                                # a box that touches two sides
    assert box([(10, 30), (12, 33)]) == (0, 10, 33, 44)                                             # the union over the frames
    # a box smaller than 20, grown to 20 at the frame's edge (no other growth): symmetrically, then back into the frame
    assert box([(slice(36, 40), slice(50, 58))], grow=0) == (20, 40, 20, 20)
    assert box([(slice(0, 3), slice(25, 30))], grow=0) == (0, 18, 20, 20)
    assert box([(slice(20, 23), slice(25, 30))], grow=0) == (12, 18, 20, 20)
    assert grow_box(None, H, W) is None and grow_box((0, H, 0, W), H, W) == (0, 0, H, W)
    # every rectangle is one the clip API takes
    rng = np.random.default_rng(1)
    for _ in range(200):
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        y1, x1 = int(rng.integers(y0 + 1, H + 1)), int(rng.integers(x0 + 1, W + 1))
        for grow in (0, 20):
            r = grow_box((y0, y1, x0, x1), H, W, grow)
            assert video.roi_of(r, H, W) in (None, r), r
            assert r[0] <= max(0, y0 - grow) and r[0] + r[2] >= min(H, y1 + grow) and r[1] <= max(0, x0 - grow)
            assert r[1] + r[3] >= min(W, x1 + grow)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_both_entries():
    C = _lib.C
    for name, n in (("spei_frame_matte_u8", 9), ("spei_frame_matte_u16", 10)):
        assert name in _lib.header_symbols()
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n
        assert args[:8] == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
        assert args[-1] is C.c_void_p and (n == 9 or args[8] is C.c_int)
    assert "matte_io.hip" in build.sources()


# ---- deblur_clip's checks ---------------------------------------------------------------------------------------------------------------
def test_deblur_clip_checks_need_no_device():
    ok = np.full((H, W), 255, np.uint8)
    with pytest.raises(ValueError, match="matte_invert=True needs matte="):
        video.deblur_clip(None, FRAMES, matte_invert=True)
    with pytest.raises(ValueError, match=r"roi=\"matte\" needs matte="):
        video.deblur_clip(None, FRAMES, roi="matte")
    with pytest.raises(ValueError, match=r"shape \(40, 61\), the frames are 60x40"):
        video.deblur_clip(None, FRAMES, matte=np.zeros((H, W + 1), np.uint8))
    with pytest.raises(ValueError, match=r"shape \(40, 60\), the frames are 61x47"):             # the matte is cropped WITH the frames
        video.deblur_clip(None, np.zeros((T, 47, 61, 3), np.uint8), matte=ok, crop=True)
    with pytest.raises(ValueError, match="holds 7 mattes for a clip of 8 frames"):
        video.deblur_clip(None, FRAMES, matte=np.zeros((T - 1, H, W), np.uint8))
    with pytest.raises(ValueError, match="uint8 or bool"):
        video.deblur_clip(None, FRAMES, matte=np.zeros((H, W), np.float32))
    with pytest.raises(ValueError, match=r"roi=\"matte\" with stream=True and a per-frame matte"):
        video.deblur_clip(None, iter(list(FRAMES)), matte=np.zeros((T, H, W), np.uint8), roi="matte", stream=True)
    with pytest.raises(ValueError, match="roi= with crop=True"):
        video.deblur_clip(None, FRAMES, matte=ok, roi="matte", crop=True)
    with pytest.raises(ValueError, match="roi= with tiles="):
        video.deblur_clip(None, FRAMES, matte=ok, roi="matte", tiles=(2, 2))
    # what passes the checks fails where `ClipRun` looks at the model: whole clip and stream, static and per frame
    for frames, kw in ((FRAMES, dict(matte=ok)), (FRAMES, dict(matte=np.zeros((T, H, W), bool), matte_invert=True, roi="matte")),
                       (iter(list(FRAMES)), dict(matte=ok, roi="matte", stream=True)),
                       (iter(list(FRAMES)), dict(matte=np.zeros((T - 1, H, W), np.uint8), stream=True))):
        with pytest.raises(AttributeError, match="parameters"):
            video.deblur_clip(None, frames, **kw)


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def test_cli_refusals_before_the_model_loads(monkeypatch, tmp_path):
    def boom(*a, **k):
        raise AssertionError("the model was loaded")
    monkeypatch.setattr(video, "load_model", boom)
    src = tmp_path / "in"
    src.mkdir()
    for i in range(2):
        _png(src / f"f{i}.png", FRAMES[i])
    (tmp_path / "mattes").mkdir()
    for i in range(2):
        _png(tmp_path / "mattes" / f"m{i}.png", np.zeros((H, W), np.uint8))
    (tmp_path / "none").mkdir()
    f = io.BytesIO()
    with y4m.Y4MWriter(f, W, H, (25, 1), y4m.CENTER, y4m.FULL) as wr:
        for _ in range(2):
            wr.write(np.zeros(y4m.frame_bytes(H, W, y4m.CENTER), np.uint8))
    (tmp_path / "in.y4m").write_bytes(f.getvalue())
    head = ["--input", str(src), "--output", str(tmp_path / "out"), "--model_path", "synthetic"]
    cases = [(["--matte_invert"], "--matte_invert: needs --matte"), (["--roi", "matte"], "--roi matte: needs --matte"),
             (["--matte", str(tmp_path / "nothing*.png")], "--matte .*nothing.*: no image file"),
             (["--matte", str(tmp_path / "none")], "--matte .*none: no image file"),
             (["--matte", str(tmp_path / "mattes"), "--roi", "matte", "--stream", "--input", str(tmp_path / "in.y4m")],
              "--roi matte with --stream"),
             (["--matte", str(tmp_path / "mattes"), "--roi", "matte", "--tiles", "2x2"], "--roi with --tiles"),
             (["--roi", "mat"], "--roi: 'mat' is not none, auto, matte or Y,X,H,W")]
    for extra, text in cases:
        with pytest.raises(SystemExit, match=text):
            video.main(head + extra)
    assert not (tmp_path / "out").exists()
