"""Codec artefacts of blur synthesis on the host: speinet_amd.codec's parser, tables and quality draw, the numpy restatement
tests/codec_ref.py against float64 and against PIL's JPEG, the plans, the C-ABI's declaration and the command lines.  No GPU."""
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import codec_ref  # noqa: E402
from speinet_amd import codec  # noqa: E402

QUALITIES = (10, 30, 50, 75, 90, 100)
# measured on `pictures()` x QUALITIES by `measure()` below (python tests/test_codec_cpu.py prints them)
COEF_GAP = 0.2500                  # max |F / 8 - float64 orthonormal DCT| before quantisation
PSNR_GAP = 0.6584                  # max |PSNR to source, integer pipeline - the same pipeline in float64|, dB
PIL_BAND = (-0.53, 0.37)           # min and max of (PSNR to source, this pipeline) - (PSNR to source, PIL's JPEG, subsampling=2), dB


def pictures():
    """Five fixed contents: a smooth pattern, that pattern with noise, saturated checker edges, uniform noise, an odd 37 x 51 frame."""
    rs = np.random.RandomState(11)
    y, x = np.mgrid[0:64, 0:80].astype(np.float64)
    lum = 120 + 90 * np.sin(x / 9.0) * np.cos(y / 7.0)                      # luminance carries the detail, colour drifts slowly
    smooth = np.stack([lum + 0.4 * x, 0.95 * lum + 10, 0.9 * lum + 30 - 0.3 * y], axis=-1)
    noisy = smooth + rs.normal(0.0, 12.0, smooth.shape)
    checker = np.where((((y // 5) + (x // 7)) % 2)[..., None] > 0, np.array([255.0, 0.0, 255.0]), np.array([0.0, 255.0, 30.0]))
    uniform = rs.randint(0, 256, (64, 80, 3)).astype(np.float64)
    odd = (smooth + rs.normal(0.0, 6.0, smooth.shape))[5:42, 9:60]
    return {k: np.clip(np.rint(v), 0, 255).astype(np.uint8) for k, v in
            (("smooth", smooth), ("noisy", noisy), ("checker", checker), ("uniform", uniform), ("odd", odd))}


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 100.0 if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


def dct_matrix():
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    return np.where(u == 0, np.sqrt(1.0 / 8.0), 0.5) * np.cos((2 * x + 1) * u * np.pi / 16.0)


def float_plane(p, Q):
    """codec_ref.code_plane with the transform, the quantiser (halves away from zero) and the final rounding in float64."""
    C = dct_matrix()
    s = codec_ref._blocks(p.astype(np.float64)) - 128.0
    F = np.einsum("vy,...yx,ux->...vu", C, s, C)
    Q = np.asarray(Q, np.float64).reshape(8, 8)
    G = np.sign(F) * np.floor(np.abs(F) / Q + 0.5) * Q
    r = np.einsum("vy,...vu,ux->...yx", C, G, C)
    return codec_ref._plane(np.clip(np.floor(r + 128.5), 0, 255).astype(np.int64))


def float_round_trip(rgb, qtabs, oy=0, ox=0):
    """codec_ref.round_trip with `float_plane` for the blocks: the colour conversions stay the contract's."""
    H, W = rgb.shape[:2]
    Y, Cb, Cr = codec_ref.to_ycc(codec_ref.pad(rgb, oy, ox))
    out = codec_ref.to_rgb(float_plane(Y, qtabs[0]), float_plane(Cb, qtabs[1]), float_plane(Cr, qtabs[1]))
    return out[oy:oy + H, ox:ox + W].astype(np.uint8)


def coefficient_gap(rgb):
    C = dct_matrix()
    gap = 0.0
    for p in codec_ref.to_ycc(codec_ref.pad(rgb)):
        s = codec_ref._blocks(p) - 128
        gap = max(gap, float(np.abs(codec_ref.forward(s) / 8.0 - np.einsum("vy,...yx,ux->...vu", C, s.astype(np.float64), C)).max()))
    return gap


def pil_jpeg(rgb, q):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=q, subsampling=2)
    return np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))


def has_pil_jpeg():
    try:
        from PIL import features
        return bool(features.check("jpg"))
    except Exception:
        return False


def measure(pil=True):
    """(coefficient gap, PSNR gap, PIL band or None) on `pictures()` x QUALITIES."""
    pics = pictures()
    gap = max(coefficient_gap(p) for p in pics.values())
    dpsnr, band = 0.0, []
    for p in pics.values():
        for q in QUALITIES:
            t = codec.quant_tables(q)
            mine = psnr(codec_ref.round_trip(p, t), p)
            dpsnr = max(dpsnr, abs(mine - psnr(float_round_trip(p, t), p)))
            if pil:
                band.append(mine - psnr(pil_jpeg(p, q), p))
    return gap, dpsnr, ((min(band), max(band)) if pil else None)


def test_parse_and_name():
    assert codec.parse(None) is None and codec.name(None) is None
    assert codec.parse("75") == (75, 75) and codec.parse(" 30..90 ") == (30, 90) and codec.parse(40) == (40, 40)
    assert codec.parse("1..100") == (1, 100) and codec.name("030..90") == "30..90" and codec.name("7..7") == "7" and codec.name(55) == "55"
    for bad in ("", "0", "101", "90..30", "0..50", "50..101", "4.5", "30..", "..30", "a", "30..90..95", 2.5, True, "1e2"):
        with pytest.raises(ValueError, match="codec"):
            codec.parse(bad)
    codec.check("30..90")
    codec.check(None)
    with pytest.raises(ValueError):
        codec.check("x")


def test_quant_tables():
    t = codec.quant_tables(50)
    assert t.dtype == np.uint16 and t.shape == (2, 64) and np.array_equal(t, codec.BASE)
    # ITU-T T.81 Annex K, tables K.1 and K.2: the corners and the sums
    assert t[0].reshape(8, 8)[0].tolist() == [16, 11, 10, 16, 24, 40, 51, 61] and t[0].reshape(8, 8)[7].tolist() == [72, 92, 95, 98, 112, 100, 103, 99]
    assert t[1].reshape(8, 8)[0].tolist() == [17, 18, 24, 47, 99, 99, 99, 99] and int(t[0].sum()) == 3688 and int(t[1].sum()) == 5505
    assert (codec.quant_tables(100) == 1).all()
    for q in (1, 10, 49, 50, 75):
        scale = 5000 // q if q < 50 else 200 - 2 * q
        want = [[min(max((int(b) * scale + 50) // 100, 1), 255) for b in tab] for tab in codec.BASE]
        assert codec.quant_tables(q).tolist() == want, q
    assert (codec.quant_tables(1)[0] == 255).all() and codec.quant_tables(10)[0][0] == 80 and codec.quant_tables(75)[0][0] == 8
    for bad in (0, 101, 50.0, "50", True):
        with pytest.raises(ValueError):
            codec.quant_tables(bad)
    allt = codec.all_tables()
    assert allt.shape == (100, 2, 64) and np.array_equal(allt[49], codec.BASE) and allt.min() >= 1 and allt.max() <= 255


def test_quality_draw():
    from speinet_amd import light
    seen = set()
    for seed in (0, 1, (7 << 32) | 11):
        for clip in range(40):
            q = codec.quality("30..90", seed, clip)
            assert q == codec.quality("30..90", seed, clip) and 30 <= q <= 90
            w0 = light.philox((0xffffffff, 0xfffffffd, 0, clip), light.key_of(seed))[0]
            assert q == 30 + (61 * w0) // 2 ** 32
            seen.add(q)
            assert codec.quality("55", seed, clip) == 55
    assert len(seen) > 30 and {codec.quality("1..2", 5, c) for c in range(40)} == {1, 2}
    assert codec.ROW not in (0xffffffff, 0xfffffffe) and codec.ROW >= 2 ** 24


def test_transform_table():
    want = np.rint(8192.0 * dct_matrix())
    assert codec.D.dtype == np.int32 and np.array_equal(codec.D, want)
    assert int(np.abs(codec.D).sum(axis=1).max()) == 23168 and int(np.abs(codec.D).sum(axis=0).max()) == 21641
    # the bounds of the docstring, from those two sums
    r, c = 23168, 21641
    T = (128 * r + 512) >> 10
    F = (r * T + 4096) >> 13
    G = (F + 4 * 255) // 8
    U = (c * G + 512) >> 10
    assert (128 * r, r * T, c * G, c * U) == codec_ref.BOUNDS and c * U + 2 ** 15 < 2 ** 31 and (T, F, G, U) == (2896, 8190, 1151, 24325)
    # the extreme blocks reach the first bound and stay inside every one
    for s in (np.full((8, 8), -128), np.full((8, 8), 127), np.where(codec.D[1][None, :] > 0, 127, -128) * np.ones((8, 1), np.int64)):
        codec_ref.inverse(codec_ref.quantise(codec_ref.forward(s.astype(np.int64)), np.ones((8, 8), np.int64)))


def test_against_float64():
    gap, dpsnr, _ = measure(pil=False)
    print(f"coefficient gap {gap:.4f}, PSNR gap {dpsnr:.4f} dB")
    assert abs(gap - COEF_GAP) < 1e-3 and abs(dpsnr - PSNR_GAP) < 1e-3             # the figures quoted above and in codec.py are these
    assert gap <= np.ceil(COEF_GAP * 8) / 8 + 1e-9                                  # 1e-9: the float64 DCT's own rounding
    assert dpsnr <= 3 * PSNR_GAP


@pytest.mark.skipif(not has_pil_jpeg(), reason="PIL has no JPEG codec")
def test_against_pil_jpeg():
    from PIL import Image
    band = []
    for name, p in pictures().items():
        for q in QUALITIES:
            if name == "odd":                                                       # libjpeg's own tables at this quality: the same values
                buf = io.BytesIO()
                Image.fromarray(p).save(buf, format="JPEG", quality=q, subsampling=2)
                theirs = Image.open(io.BytesIO(buf.getvalue())).quantization
                assert [sorted(theirs[k]) for k in (0, 1)] == [sorted(t) for t in codec.quant_tables(q).tolist()], q
            d = psnr(codec_ref.round_trip(p, codec.quant_tables(q)), p) - psnr(pil_jpeg(p, q), p)
            print(f"{name} q{q}: {d:+.2f} dB against PIL")
            band.append(d)
    assert PIL_BAND[0] - 0.5 <= min(band) and max(band) <= PIL_BAND[1] + 0.5, (min(band), max(band))


def test_psnr_rises_with_quality_and_flat_stays_flat():
    for name, p in pictures().items():
        got = [psnr(codec_ref.round_trip(p, codec.quant_tables(q)), p) for q in QUALITIES]
        assert all(b >= a for a, b in zip(got, got[1:])), (name, got)
    for value in ((0, 0, 0), (255, 255, 255), (128, 128, 128), (200, 30, 90), (1, 254, 7)):
        flat = np.empty((21, 35, 3), np.uint8)
        flat[...] = value
        for q in (10, 50, 100):
            for oy, ox in ((0, 0), (7, 15)):
                out = codec_ref.round_trip(flat, codec.quant_tables(q), oy, ox)
                assert (out == out[0, 0]).all(), (value, q)
                # all tables 1: Y, Cb and Cr each come back within one level, so a channel within 1 + 1.772 + rounding
                assert q != 100 or np.abs(out[0, 0].astype(int) - value).max() <= 3, (value, out[0, 0])


def test_grid_offsets_and_in_place():
    """An MCU is self-contained: a frame coded on the grid at (-oy, -ox) equals, inside every whole MCU, the crop of the frame padded to
    that grid; and the offsets matter (another grid gives other bytes)."""
    p = pictures()["noisy"]
    t = codec.quant_tables(30)
    whole = codec_ref.round_trip(p, t)
    crop = p[7:7 + 40, 13:13 + 40]
    coded = codec_ref.round_trip(crop, t, 7, 13)
    assert np.array_equal(coded[9:25, 3:35], whole[16:32, 16:48])                   # the MCUs wholly inside the crop
    assert not np.array_equal(codec_ref.round_trip(crop, t, 0, 0)[9:25, 3:35], whole[16:32, 16:48])
    for flags in range(8):
        a = codec_ref.augment(crop, flags)
        assert np.array_equal(codec_ref.unaugment(a, flags), crop)
    assert np.array_equal(codec_ref.augment(crop, 4), np.rot90(crop)) and np.array_equal(codec_ref.augment(crop, 3), crop[::-1, ::-1])


def write_sharp(root, clips):
    from speinet_amd.video import _imwrite
    for name, frames in clips.items():
        os.makedirs(os.path.join(root, name), exist_ok=True)
        for i, f in enumerate(frames):
            _imwrite(os.path.join(root, name, f"{i:06d}.png"), f)
    return root


def test_plans_are_untouched_and_records(tmp_path):
    from speinet_amd import blurset, data
    a = blurset.plan_dataset([30, 41, 17], [0.1, 0.5], 3)
    for c in range(3):
        codec.quality("30..90", 3, c)
    b = blurset.plan_dataset([30, 41, 17], [0.1, 0.5], 3)
    assert all(ra == rb and all(np.array_equal(x, y) for x, y in zip(pa, pb)) for (ra, pa), (rb, pb) in zip(a, b))
    rs = np.random.RandomState(0)
    src = write_sharp(str(tmp_path / "sharp"), {f"clip{c}": rs.randint(0, 256, (30, 40, 48, 3)).astype(np.uint8) for c in range(2)})
    plain = data.SharpClipSet(src, references=True, seed=3)
    coded = data.SharpClipSet(src, references=True, seed=3, codec="30..90")
    assert plain.codec is None and coded.codec == "30..90" and "codec" not in plain.summary() and "codec 30..90" in coded.summary()
    for epoch in (0, 1):
        plain.plan(epoch)
        coded.plan(epoch)
        for k, (p, q) in enumerate(zip(plain.clips, coded.clips)):
            assert p["starts"].tolist() == q["starts"].tolist() and p["labels"] == q["labels"] and "quality" not in p
            assert q["quality"] == codec.quality("30..90", 3 + epoch, k)
    with pytest.raises(ValueError, match="codec"):
        data.SharpClipSet(src, references=True, codec="0..5")
    sampler = data.Sampler(coded, 2, 20, seed=1)
    items = sampler.epoch()[0]
    run = np.zeros(2 * 5 + 2, dtype=data.RUN_RECORD)
    run["y0"][:10], run["x0"][:10], run["flags"][:10] = np.repeat([7, 16], 5), np.repeat([29, 3], 5), np.repeat([5, 2], 5)
    run["flags"][3] |= 8
    rec = data.run_codec_records(coded, items, run)
    assert rec.dtype == codec.CODEC_RECORD and rec.shape == (10,)
    assert rec["oy"].tolist() == [7] * 5 + [0] * 5 and rec["ox"].tolist() == [13] * 5 + [3] * 5
    assert rec["flags"].tolist() == [5, 5, 5, 13, 5, 2, 2, 2, 2, 2]
    assert rec["qtab"].tolist() == [coded.clips[s.clip]["quality"] - 1 for _i, s, _d in items for _ in range(5)]
    r = codec.records(3, qtab=[0, 1, 0], oy=7, ox=[0, 15, 3], flags=[0, codec.SKIP, 0])
    assert r["qtab"].tolist() == [0, 1, 0] and r["oy"].tolist() == [7, 7, 7] and r["flags"].tolist() == [0, 16, 0] and r.nbytes == 48


def test_c_abi_declares_the_entries():
    from speinet_amd import _lib, build
    text = open(_lib.HEADER_PATH).read()
    assert "uint32_t qtab;" in text and "} spei_codec_record;" in text and "#define SPEI_CODEC_SKIP 16" in text
    for name, n_args in (("spei_codec_u8", 12), ("spei_train_batch_codec_f32", 10)):
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.SIGNATURES["spei_window_mean_u8"][0] and len(args) == n_args
    assert "codec.hip" in build.sources()


def test_command_lines(capsys):
    from speinet_amd import blurset, fit
    base = ["--dir_data_test", "v", "--save", "s"]
    io_ = ["--input", "a", "--output", "b"]
    assert blurset.parser().parse_args(io_).codec is None
    assert blurset.parser().parse_args(io_ + ["--codec", "30..90"]).codec == "30..90"
    assert fit.parser().parse_args(base + ["--dir_sharp", "a"]).blur_codec is None
    assert fit.parser().parse_args(base + ["--dir_sharp", "a", "--blur_codec", "75"]).blur_codec == "75"
    for main, argv, text in ((blurset.main, io_ + ["--codec", "0"], "--codec"),
                             (blurset.main, io_ + ["--codec", "90..30"], "--codec"),
                             (blurset.main, io_ + ["--light", "srgb", "--codec", "4.5"], "--codec"),
                             (fit.main, base + ["--dir_sharp", "a", "--blur_codec", "101"], "--blur_codec"),
                             (fit.main, base + ["--dir_data", "a", "--blur_codec", "30..90"], "--dir_sharp")):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert e.value.code == 2 and text in capsys.readouterr().err, argv


if __name__ == "__main__":
    print("coefficient gap %.4f, PSNR gap %.4f dB, PIL band %s" % measure(has_pil_jpeg()))
