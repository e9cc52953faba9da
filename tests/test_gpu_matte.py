"""GPU suite for `deblur_clip(..., matte=)`: the blend launch (csrc/matte_io.hip `spei_frame_matte_u8` / `_u16`, `ops.frame_matte`)
against the numpy statement `matte_ref.blend`, exactly; the clip loop with a matte against the run without one, frame by frame and
bit for bit, alone and composed with every other clip feature; the launches it issues, counted by entry point; `roi="matte"`; the
bf16x3 recompute; a stream; and the command line.
Synthetic weights, frames of 40x60 (80x120 under tiles), clips of 8 frames."""
import collections
import ctypes
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import matte_ref as MR                                             # noqa: E402
import roi_ref as RR                                               # noqa: E402
from speinet_amd import _lib, ops, video, y4m                      # noqa: E402
from speinet_amd.clip import frames_of                             # noqa: E402
from speinet_amd.synth import synth_frames                         # noqa: E402

DEV = "cuda:0"
VP = ctypes.c_void_p
DEPTHS = (8, 10, 12)
LABELS = [1, 0, 0, 1, 1, 0, 1, 0]
T = len(LABELS)
EMPTY = [0, 3, 4]                                                  # the frames of the per-frame matte that are empty


def _np_dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def _t_dtype(depth):
    return torch.uint8 if depth == 8 else torch.uint16


def _requant(frame, in_depth, out_depth):
    return RR.requant(frame, in_depth, out_depth).astype(_np_dtype(out_depth))


def _blend(frame, deb, matte, in_depth, out_depth, invert=False):
    """The definition: a = requant(input), b = min(deblurred, D_out)."""
    b = np.minimum(np.asarray(deb).astype(np.int64), (1 << out_depth) - 1)
    return MR.blend(RR.requant(frame, in_depth, out_depth), b, matte, invert).astype(_np_dtype(out_depth))


def _samples(rng, shape, depth, above=True):
    """Random samples of `depth` bits; a tenth of the deep ones are words above D."""
    D = (1 << depth) - 1
    a = rng.integers(0, D + 1, shape).astype(_np_dtype(depth))
    if depth > 8 and above:
        at = rng.random(shape) < 0.1
        a[at] = rng.integers(D + 1, 65536, int(at.sum())).astype(np.uint16)
    return a


def _matte_bytes(rng, h, w):
    m = rng.integers(0, 256, (h, w)).astype(np.uint8)
    pick = rng.random((h, w))
    m[pick < 0.2] = 0
    m[pick > 0.8] = 255
    return m


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _shifted(a, guard=0):
    """The array on the device as a view one element into a buffer (its base is not on a word boundary), and that buffer, which holds
    one guard element on either side of it."""
    buf = _dev(np.concatenate([np.full(1, guard, a.dtype), a.reshape(-1), np.full(1, guard, a.dtype)]))
    view = buf[1:-1].view(a.shape)
    assert view.data_ptr() % 4 != 0
    return view, buf


# ---- 1. the launch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_depth", DEPTHS)
@pytest.mark.parametrize("in_depth", DEPTHS)
def test_matte_kernel(in_depth, out_depth):
    """A lone pixel, a tail group, W % 4 != 0 and whole groups (two widths); out of place, in place and inverted; every operand in turn
    from a view one element into a buffer (the element paths), the destination between two guard words; words above D in the frame
    and in deb."""
    deep = None if in_depth == 8 else in_depth
    for h, w in ((1, 1), (3, 5), (21, 37), (6, 20), (40, 64)):
        rng = np.random.default_rng(1000 * h + w + 16 * in_depth + out_depth)
        frame, deb, matte = _samples(rng, (h, w, 3), in_depth), _samples(rng, (h, w, 3), out_depth), _matte_bytes(rng, h, w)
        ref = _blend(frame, deb, matte, in_depth, out_depth)
        f, d, m = _dev(frame), _dev(deb), _dev(matte)
        got = ops.frame_matte(f, d, m, out_depth, deep)
        assert got.dtype == _t_dtype(out_depth) and tuple(got.shape) == (h, w, 3) and got.data_ptr() != d.data_ptr()
        assert np.array_equal(got.cpu().numpy(), ref), (h, w, np.argwhere(got.cpu().numpy() != ref)[:5])
        assert np.array_equal(d.cpu().numpy(), deb)                                                 # out of place: deb is read only
        inv = ops.frame_matte(f, d, m, out_depth, deep, invert=True).cpu().numpy()
        assert np.array_equal(inv, _blend(frame, deb, matte, in_depth, out_depth, True))
        assert np.array_equal(inv, _blend(frame, deb, 255 - matte, in_depth, out_depth))
        place = d.clone()
        assert ops.frame_matte(f, place, m, out_depth, deep, out=place).data_ptr() == place.data_ptr()
        assert np.array_equal(place.cpu().numpy(), ref), (h, w)                                     # in place equals out of place
        for name in ("frame", "deb", "matte"):
            args = dict(frame=f, deb=d, matte=m)
            args[name] = _shifted(dict(frame=frame, deb=deb, matte=matte)[name])[0]
            assert np.array_equal(ops.frame_matte(args["frame"], args["deb"], args["matte"], out_depth, deep).cpu().numpy(), ref), (h, w, name)
        oview, obuf = _shifted(np.full((h, w, 3), 7, _np_dtype(out_depth)), guard=7)
        ops.frame_matte(f, d, m, out_depth, deep, out=oview)
        flat = obuf.cpu().numpy()
        assert np.array_equal(flat[1:-1].reshape(h, w, 3), ref) and flat[0] == 7 and flat[-1] == 7  # nothing past either end
        # in place in a shifted buffer: deb and dst on the element path at once
        pview, pbuf = _shifted(deb)
        ops.frame_matte(f, pview, m, out_depth, deep, out=pview)
        flat = pbuf.cpu().numpy()
        assert np.array_equal(flat[1:-1].reshape(h, w, 3), ref) and flat[0] == 0 and flat[-1] == 0


@pytest.mark.parametrize("out_depth", DEPTHS)
@pytest.mark.parametrize("in_depth", DEPTHS)
def test_every_matte_code(in_depth, out_depth):
    """Every m in 0..255 against the input samples {0, 1, D_in - 1, D_in} and the deblurred samples {0, 1, D_out - 1, D_out}: row
    4 * i + j of the frame holds input i and deblurred j, column m the matte code m."""
    Din, Dout = (1 << in_depth) - 1, (1 << out_depth) - 1
    va, vb = [0, 1, Din - 1, Din], [0, 1, Dout - 1, Dout]
    frame = np.repeat(np.asarray(va), 4)[:, None, None] * np.ones((1, 256, 3), np.int64)
    deb = np.tile(np.asarray(vb), 4)[:, None, None] * np.ones((1, 256, 3), np.int64)
    matte = np.tile(np.arange(256, dtype=np.uint8), (16, 1))
    frame, deb = frame.astype(_np_dtype(in_depth)), deb.astype(_np_dtype(out_depth))
    got = ops.frame_matte(_dev(frame), _dev(deb), _dev(matte), out_depth, None if in_depth == 8 else in_depth).cpu().numpy()
    assert np.array_equal(got, _blend(frame, deb, matte, in_depth, out_depth))
    assert np.array_equal(got[:, 0], _requant(frame[:, 0], in_depth, out_depth)) and np.array_equal(got[:, 255], deb[:, 255])
    assert got.min() == 0 and got.max() == Dout


def test_matte_refusals():
    """Refused through the C-ABI before anything is launched, each with its reason in `spei_last_error`: nothing is written."""
    H, W = 20, 24
    lib = _lib.lib()
    st = VP(torch.cuda.current_stream(DEV).cuda_stream)
    n = H * W * 3
    slots = torch.zeros(8 * 8192, dtype=torch.uint8, device=DEV)      # one buffer, a slot of 8192 bytes per operand: a pointer moved by
                                                                      # less than a frame meets no other operand by accident
    def slot(k, shape, dtype, value):
        t = slots[k * 8192:k * 8192 + int(np.prod(shape)) * (2 if dtype == torch.uint16 else 1)].view(dtype).view(shape)
        return t.fill_(value)

    frame, deb, dst = (slot(k, (H, W, 3), torch.uint16, v) for k, v in ((0, 5), (1, 9), (2, 3)))
    matte = slot(3, (H, W), torch.uint8, 255)
    good = dict(frame=frame.data_ptr(), in_depth=10, deb=deb.data_ptr(), matte=matte.data_ptr(), invert=0, dst=dst.data_ptr(), H=H, W=W, depth=12)

    def call16(**kw):
        a = dict(good, **kw)
        return lib.spei_frame_matte_u16(VP(a["frame"]), a["in_depth"], VP(a["deb"]), VP(a["matte"]), a["invert"], VP(a["dst"]), a["H"], a["W"],
                                        a["depth"], st)

    cases = [(dict(frame=None), "null pointer"), (dict(deb=None), "null pointer"), (dict(matte=None), "null pointer"),
             (dict(dst=None), "null pointer"),
             (dict(in_depth=9), "unknown in_depth 9"), (dict(in_depth=16), "unknown in_depth 16"), (dict(in_depth=0), "unknown in_depth 0"),
             (dict(depth=8), "unknown depth 8"), (dict(depth=11), "unknown depth 11"), (dict(depth=-10), "unknown depth -10"),
             (dict(H=0), "bad frame shape"), (dict(W=0), "bad frame shape"), (dict(H=-1), "bad frame shape"),
             (dict(H=32768, W=32768), "bad frame shape"), (dict(H=1 << 15, W=21846), "bad frame shape"),       # 3 H W >= 2^31
             (dict(frame=frame.data_ptr() + 1), "misaligned"), (dict(deb=deb.data_ptr() + 1), "misaligned"),
             (dict(dst=dst.data_ptr() + 1), "misaligned"),
             (dict(dst=deb.data_ptr() + 2), "dst overlaps deb"), (dict(dst=deb.data_ptr() + 2 * n - 2), "dst overlaps deb"),
             (dict(deb=dst.data_ptr() + 2 * n - 2), "dst overlaps deb"),
             (dict(dst=frame.data_ptr()), "dst overlaps frame"), (dict(dst=frame.data_ptr() + 2 * n - 2), "dst overlaps frame"),
             (dict(frame=dst.data_ptr() + 2 * n - 2), "dst overlaps frame"),
             (dict(matte=dst.data_ptr()), "dst overlaps matte"), (dict(matte=dst.data_ptr() + 2 * n - 1), "dst overlaps matte")]
    for kw, text in cases:
        assert call16(**kw) != 0, kw
        err = lib.spei_last_error().decode()
        assert text in err and "spei_frame_matte_u16" in err, (kw, err)
    # the 8-bit entry: its own name, and the same checks
    f8, d8, o8 = (slot(k, (H, W, 3), torch.uint8, v) for k, v in ((4, 5), (5, 9), (6, 3)))

    def call8(**kw):
        a = dict(dict(frame=f8.data_ptr(), in_depth=8, deb=d8.data_ptr(), matte=matte.data_ptr(), invert=0, dst=o8.data_ptr(), H=H, W=W), **kw)
        return lib.spei_frame_matte_u8(VP(a["frame"]), a["in_depth"], VP(a["deb"]), VP(a["matte"]), a["invert"], VP(a["dst"]), a["H"], a["W"], st)

    for kw, text in [(dict(matte=None), "null pointer"), (dict(in_depth=7), "unknown in_depth 7"), (dict(H=0), "bad frame shape"),
                     (dict(frame=frame.data_ptr() + 1, in_depth=12), "misaligned"), (dict(dst=d8.data_ptr() + 1), "dst overlaps deb"),
                     (dict(dst=f8.data_ptr() + n - 1), "dst overlaps frame"), (dict(dst=matte.data_ptr()), "dst overlaps matte")]:
        assert call8(**kw) != 0, kw
        err = lib.spei_last_error().decode()
        assert text in err and "spei_frame_matte_u8" in err, (kw, err)
    torch.cuda.synchronize()
    for t, v in ((dst, 3), (deb, 9), (frame, 5), (o8, 3), (d8, 9), (f8, 5), (matte, 255)):
        assert (t.cpu().numpy() == v).all()                                                         # nothing ran
    assert call16() == 0 and call8() == 0 and call8(dst=d8.data_ptr(), invert=1) == 0                # in place is allowed
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 9).all() and (o8.cpu().numpy() == 9).all() and (d8.cpu().numpy() == 5).all()
    # and the wrapper
    with pytest.raises(ValueError, match="out_depth"):
        ops.frame_matte(f8, d8, matte, 9)
    with pytest.raises(ValueError, match="uint16 frames only"):
        ops.frame_matte(f8, d8, matte, 8, in_depth=10)
    with pytest.raises(ValueError, match="depth must be 10 or 12"):
        ops.frame_matte(frame, d8, matte, 8)
    with pytest.raises(ValueError, match="deb must be"):
        ops.frame_matte(f8, deb, matte, 8)
    with pytest.raises(ValueError, match="matte must be"):
        ops.frame_matte(f8, d8, matte[:, :-1], 8)
    with pytest.raises(RuntimeError, match="dst overlaps frame"):
        ops.frame_matte(f8, d8, matte, 8, out=f8)


# ---- 2. the clip --------------------------------------------------------------------------------------------------------------------------
def _clip(n, h, w, depth=8, seed=3):
    """[n,h,w,3] of `depth` bits: the synthetic frames, shifted a little per frame."""
    D = (1 << depth) - 1
    x = synth_frames(1, h, w, seed=seed)[0]
    return np.stack([(torch.roll(x[i % 5], shifts=(i, -2 * i), dims=(1, 2)).permute(1, 2, 0).numpy().astype(np.float64) * D).round()
                     .clip(0, D).astype(_np_dtype(depth)) for i in range(n)])


def _static(h, w):
    """A matte with a region of 0, a region of 255 and every level between, on no word boundary."""
    return np.clip(9 * np.arange(w)[None, :] + 3 * np.arange(h)[:, None] - 70, 0, 255).astype(np.uint8)


def _per_frame(n, h, w):
    """A subject that moves through the shot; the frames EMPTY have none."""
    m = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        if i not in EMPTY:
            m[i, 4 + i:20 + i, 7 + 3 * i:31 + 3 * i] = np.clip(40 * np.arange(24)[None, :] + 17 * i, 0, 255)
    return m


@pytest.fixture(scope="module", params=["f16-graph", "f32-eager"])
def net(request):
    precision, how = request.param.split("-")
    return video.load_model("synthetic", DEV, precision, how == "graph")


@pytest.fixture(scope="module")
def net32():
    return video.load_model("synthetic", DEV, "f32", False)


def _frames(run):
    out = []
    for i, t in run:
        assert i == len(out)
        out.append(t.cpu().numpy())
    return out


def _inputs(clip, **kw):
    """The input frames as the loop sees them, [H,W,3] numpy each: the array's (cropped for `crop`), or a y4m clip's RGB frames."""
    fr = frames_of(clip, kw.get("crop", False), kw.get("yuv"), kw.get("depth"))
    if fr.yuv is None:
        return fr, [np.asarray(fr.host(i)) for i in range(fr.T)]
    if kw.get("fields"):
        fr = fr.woven()
    return fr, [fr.rgb(torch.from_numpy(fr.host(i)).to(DEV)[None])[0].cpu().numpy() for i in range(fr.T)]


def _matte_against_base(net, clip, labels, matte, invert=False, **kw):
    """Both runs of one clip, with the same arguments but for the matte: every frame is blend(requant(input), base, m), a frame that
    `sharp="keep"` keeps is requant(input) whatever its matte, and a frame whose matte is empty is listed as unmatted."""
    base_run = video.deblur_clip(net, clip, labels, **kw)
    base = _frames(base_run)
    if kw.get("out") is not None:
        kw = dict(kw, out=torch.zeros_like(kw["out"]))
    run = video.deblur_clip(net, clip, labels, matte=matte, matte_invert=invert, **kw)
    assert run.unmatted == [] and run.matte is not None and base_run.matte is None
    got = _frames(run)
    fr, inputs = _inputs(clip, **kw)
    m = np.asarray(matte.cpu() if torch.is_tensor(matte) else matte)
    m = m.astype(np.uint8) * 255 if m.dtype == np.bool_ else m
    m = np.broadcast_to(m, (len(labels),) + m.shape[-2:])[:, :fr.H, :fr.W]
    m = 255 - m if invert else m
    kept = [i for i, v in enumerate(labels) if v] if kw.get("sharp") == "keep" else []
    assert run.unmatted == [i for i in range(len(labels)) if not m[i].any()] and run.kept == kept and run.recomputed == []
    assert run.plan == base_run.plan and list(run.labels) == list(base_run.labels) and run.cuts == base_run.cuts
    assert len(run.seconds) == len(got) == len(base) == len(labels)
    for i in range(len(labels)):
        assert got[i].dtype == base[i].dtype == _np_dtype(run.out_depth) and got[i].shape == base[i].shape == (fr.H, fr.W, 3)
        want = _requant(inputs[i], run.depth, run.out_depth) if i in kept else _blend(inputs[i], base[i], m[i], run.depth, run.out_depth)
        assert np.array_equal(got[i], want), (i, np.argwhere(got[i] != want)[:5])
    if kw.get("out") is not None:
        assert np.array_equal(kw["out"].cpu().numpy(), np.stack(got))
    return run, got, base, inputs


def test_static_matte(net):
    clip = _clip(T, 40, 60)
    run, got, base, inputs = _matte_against_base(net, clip, LABELS, _static(40, 60))
    for i in range(T):                                         # the case is not empty: neither run, somewhere
        assert not np.array_equal(got[i], base[i]) and not np.array_equal(got[i], inputs[i]), i
    assert run.unmatted == [] and run.kept == []


def test_matte_of_255_is_the_run_without_and_a_device_matte(net):
    clip = _clip(T, 40, 60)
    _, got, base, _ = _matte_against_base(net, clip, LABELS, np.full((40, 60), 255, np.uint8))
    assert all(np.array_equal(a, b) for a, b in zip(got, base))
    _, got, base, _ = _matte_against_base(net, clip, LABELS, torch.ones(40, 60, dtype=torch.bool, device=DEV))
    assert all(np.array_equal(a, b) for a, b in zip(got, base))


def test_matte_of_0_is_the_input_and_never_calls_the_model(net, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the model was called")
    for name in ("forward_window", "forward", "prefetch_window"):
        monkeypatch.setattr(type(net), name, boom)
    clip = _clip(T, 40, 60)
    for matte, kw in ((np.zeros((40, 60), np.uint8), {}), (np.full((T, 40, 60), 255, np.uint8), dict(matte_invert=True)),
                      (torch.zeros(T, 40, 60, dtype=torch.uint8, device=DEV), {})):
        run = video.deblur_clip(net, clip, LABELS, matte=matte, **kw)
        got = _frames(run)
        assert np.array_equal(np.stack(got), clip) and run.unmatted == list(range(T)) and run.kept == [] and len(run.seconds) == T
    deep = _clip(6, 40, 60, 12)
    run = video.deblur_clip(net, deep, [0] * 6, matte=np.zeros((40, 60), bool), depth=12, out_depth=8)
    assert np.array_equal(np.stack(_frames(run)), _requant(deep, 12, 8)) and run.unmatted == list(range(6))


@pytest.mark.parametrize("form", ["array", "device", "list"])
def test_per_frame_matte(net, form):
    """Frames 0, 3 and 4 have an empty matte: no window runs for them, `unmatted` grows as they are handed out, and the plan and the
    labels are the base run's."""
    clip, per = _clip(T, 40, 60), _per_frame(T, 40, 60)
    matte = {"array": per, "device": _dev(per), "list": [m for m in per]}[form]
    base_run = video.deblur_clip(net, clip, LABELS)
    base = _frames(base_run)
    run = video.deblur_clip(net, clip, LABELS, matte=matte)
    got = []
    for i, t in run:
        assert i == len(got) and run.unmatted == [j for j in EMPTY if j <= i], (i, run.unmatted)
        got.append(t.cpu().numpy())
    assert run.unmatted == EMPTY and run.kept == [] and run.recomputed == [] and run.assumed == []
    assert run.plan == base_run.plan and list(run.labels) == list(base_run.labels) == LABELS
    for i in range(T):
        want = clip[i] if i in EMPTY else _blend(clip[i], base[i], per[i], 8, 8)
        assert np.array_equal(got[i], want), i
        assert (i in EMPTY) or not np.array_equal(got[i], clip[i]), i


# ---- 3. the launches --------------------------------------------------------------------------------------------------------------------
def _counted(monkeypatch):
    seen = []
    orig = _lib.check

    def check(rc, what):
        seen.append(what)
        return orig(rc, what)
    monkeypatch.setattr(_lib, "check", check)
    return seen


def test_launches(net, monkeypatch):
    """By entry point (`_lib.check` sees every call of the library): `matte=None` is the default run launch for launch; with a
    per-frame matte one blend per frame that is neither unmatted nor kept, one requant per frame that is, and no ingest for a window
    that does not run."""
    clip, per = _clip(T, 40, 60), _per_frame(T, 40, 60)
    _frames(video.deblur_clip(net, clip, LABELS))              # every graph of the plan is captured before anything is counted
    seen = _counted(monkeypatch)

    def counts(**kw):
        seen.clear()
        run = video.deblur_clip(net, clip, LABELS, **kw)
        out = _frames(run)
        torch.cuda.synchronize()
        return collections.Counter(seen), out, run

    default, a, _ = counts()
    none, b, run = counts(matte=None, matte_invert=False)
    assert none == default and run.unmatted == [] and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert default["spei_frame_matte_u8"] == 0 and default["spei_frame_requant"] == 0 and default["spei_frame_u8_out"] == T
    full, c, _ = counts(matte=np.full((40, 60), 255, np.uint8))
    extra = full - default
    assert extra == collections.Counter({"spei_frame_matte_u8": T}) and default - full == collections.Counter()
    assert all(np.array_equal(x, y) for x, y in zip(a, c))
    mixed, _, run = counts(matte=per)
    assert run.unmatted == EMPTY
    assert mixed["spei_frame_matte_u8"] == T - len(EMPTY) == mixed["spei_frame_u8_out"] and mixed["spei_frame_requant"] == len(EMPTY)
    assert mixed["spei_frame_matte_u16"] == 0 and mixed["spei_roi_paste_u8"] == 0
    n_in = sum(key is not video.ZERO for p in run.plan if p["index"] not in EMPTY for key in p["keys"])
    assert mixed["spei_frames_u8_in"] == n_in < default["spei_frames_u8_in"]
    both, _, run = counts(matte=per, sharp="keep")
    out = sorted(set(EMPTY) | {i for i, v in enumerate(LABELS) if v})
    assert run.unmatted == EMPTY and run.kept == [i for i, v in enumerate(LABELS) if v]
    assert both["spei_frame_matte_u8"] == T - len(out) == both["spei_frame_u8_out"] and both["spei_frame_requant"] == len(out)


# ---- 4. compositions --------------------------------------------------------------------------------------------------------------------
def _y4m_bytes(clip, layout, depth=8, matrix=y4m.BT601, rng=y4m.LIMITED) -> bytes:
    """The clip as a y4m stream's bytes (the project's own RGB -> YUV kernels make the planes)."""
    f = io.BytesIO()
    wr = y4m.Y4MWriter(f, clip.shape[2], clip.shape[1], (25, 1), layout, rng, depth=depth)
    for frame in clip:
        t = torch.from_numpy(np.ascontiguousarray(frame)).to(DEV)
        planar = ops.rgb_u8_to_yuv(t, layout, matrix, rng) if depth == 8 else ops.rgb_u16_to_yuv(t, layout, matrix, rng, depth)
        wr.write(planar.cpu().numpy())
    return f.getvalue()


COMPOSITIONS = {
    "tiles": (dict(size=(80, 120)), dict(tiles=(2, 2), feather=8)),
    "roi": (dict(size=(60, 90)), dict(roi=(7, 13, 40, 60), roi_feather=4)),
    "ensemble": (dict(), dict(ensemble=2)),
    "deeper_out": (dict(), dict(out_depth=10)),
    "deep_in": (dict(depth=10), dict(depth=10, out_depth=8)),
    "cuts": (dict(), dict(cuts=[3])),
    "out": (dict(), dict(out=True)),
    "crop": (dict(size=(47, 61)), dict(crop=True)),
    "y4m": (dict(y4m=True), dict()),
    "fields": (dict(), dict(fields="split")),
    "keep": (dict(matte="full"), dict(sharp="keep")),
    "invert": (dict(), dict(invert=True)),
}


@pytest.mark.parametrize("name", sorted(COMPOSITIONS))
def test_compositions(net32, name, tmp_path):
    how, kw = (dict(v) for v in COMPOSITIONS[name])
    h, w = how.get("size", (40, 60))
    clip = _clip(T, h, w, how.get("depth", 8))
    matte = np.full((h, w), 255, np.uint8) if how.get("matte") == "full" else _static(h, w) if name in ("tiles", "y4m") else _per_frame(T, h, w)
    if how.get("y4m"):
        path = tmp_path / "clip.y4m"
        path.write_bytes(_y4m_bytes(clip, y4m.CENTER))
        clip = y4m.Y4MReader(str(path))
    if kw.get("out"):
        kw["out"] = torch.zeros((T, h, w, 3), dtype=torch.uint8, device=DEV)
    run, got, base, inputs = _matte_against_base(net32, clip, LABELS, matte, **kw)
    if name == "crop":
        assert got[0].shape == (40, 60, 3) and run.matte.host(1).shape == (40, 60)
    if name == "roi":
        assert run.roi == (7, 13, 40, 60)
    if name == "tiles":
        assert run.tiles is not None and run.tiles.n == 4
    if name == "keep":                                         # a kept frame is the input even under m = 255; the others are the base run's
        assert run.kept == [i for i, v in enumerate(LABELS) if v] and run.unmatted == []
        assert all(np.array_equal(got[i], inputs[i]) for i in run.kept)
        assert all(np.array_equal(got[i], base[i]) and not np.array_equal(got[i], inputs[i]) for i in range(T) if i not in run.kept)
    if name == "invert":                                       # equals the run with 255 - m
        other = _frames(video.deblur_clip(net32, clip, LABELS, matte=255 - matte))
        assert all(np.array_equal(a, b) for a, b in zip(got, other))
        assert run.unmatted == []                              # 255 - 0 is not empty


# ---- 5. roi="matte" ---------------------------------------------------------------------------------------------------------------------
def test_roi_matte(net32, monkeypatch):
    h, w = 80, 100
    clip, per = _clip(T, h, w), np.zeros((T, h, w), np.uint8)
    per[:, 30:42, 50:60] = _per_frame(T, 40, 60)[:, 8:20, 20:30]
    rect = MR.bbox(per, h, w)
    assert rect is not None and rect != (0, 0, h, w) and rect[2] < h and rect[3] < w
    run = video.deblur_clip(net32, clip, LABELS, matte=per, roi="matte", roi_feather=3)
    got = _frames(run)
    assert run.roi == rect
    given = video.deblur_clip(net32, clip, LABELS, matte=per, roi=rect, roi_feather=3)
    want = _frames(given)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert run.plan == given.plan and run.unmatted == given.unmatted == [i for i in range(T) if not per[i].any()]
    assert any(not np.array_equal(got[i], clip[i]) for i in range(T))
    # a static matte in a stream
    run = video.deblur_clip(net32, iter(clip), LABELS, matte=per[1], roi="matte", stream=True, horizon=24)
    got = _frames(run)
    assert run.roi == MR.bbox(per[1], h, w)
    want = _frames(video.deblur_clip(net32, clip, LABELS, matte=per[1], roi=run.roi))
    assert run.assumed == [] and all(np.array_equal(a, b) for a, b in zip(got, want))

    def boom(*a, **k):
        raise AssertionError("the model was called")
    for name in ("forward_window", "forward", "prefetch_window"):
        monkeypatch.setattr(type(net32), name, boom)
    run = video.deblur_clip(net32, clip, LABELS, matte=np.zeros((T, h, w), np.uint8), roi="matte")
    assert np.array_equal(np.stack(_frames(run)), clip) and run.roi is None and run.unmatted == list(range(T))


# ---- 6. the recompute -------------------------------------------------------------------------------------------------------------------
def test_non_finite_windows_recomputed():
    """One weight beyond +-65504 makes every f16 frame non-finite (tests/test_gpu_video.py::test_non_finite_windows_recomputed):
    every window that runs is recomputed in bf16x3, the matted frames only, and the blend runs again behind the recompute's egress."""
    import warnings
    model = video.load_model("synthetic", DEV, "f16", True)
    with torch.no_grad():
        model.recons_net.outBlock[3].weight[0, 0, 0, 0] = 1.0e5
    model.invalidate_packed()
    clip, per = _clip(T, 40, 60), _per_frame(T, 40, 60)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        base_run = video.deblur_clip(model, clip, LABELS)
        base = _frames(base_run)                               # the bf16x3 result of every frame
        assert base_run.recomputed == list(range(T))
        n = len(caught)
        run = video.deblur_clip(model, clip, LABELS, matte=per)
        got = _frames(run)
    matted = [i for i in range(T) if i not in EMPTY]
    assert run.recomputed == matted and run.unmatted == EMPTY
    assert sum("recomputed in bf16x3" in str(c.message) for c in caught[n:]) == len(matted)
    assert (model.precision, model.corr_precision, model.use_graph) == ("f16", "top2", True)         # restored
    for i in range(T):
        want = clip[i] if i in EMPTY else _blend(clip[i], base[i], per[i], 8, 8)
        assert np.array_equal(got[i], want), i


# ---- 7. a stream ------------------------------------------------------------------------------------------------------------------------
def test_stream(net32):
    clip, per = _clip(T, 40, 60), _per_frame(T, 40, 60)
    for matte in (_static(40, 60), per, list(per)):
        whole = video.deblur_clip(net32, clip, LABELS, matte=matte)
        ref = _frames(whole)
        run = video.deblur_clip(net32, iter(clip), LABELS, matte=matte, stream=True, horizon=24)
        got = _frames(run)
        assert run.unmatted == whole.unmatted and run.plan == whole.plan
        assert len(got) == T and all(np.array_equal(got[i], ref[i]) for i in range(T) if i not in run.assumed)
        assert not set(run.assumed) & set(run.unmatted)
    assert whole.unmatted == EMPTY
    with pytest.raises(ValueError, match=f"frame {T - 1} has no matte: the stream outruns its matte of {T - 1} frames"):
        _frames(video.deblur_clip(net32, iter(clip), LABELS, matte=per[:-1], stream=True, horizon=24))
    with pytest.raises(ValueError, match=f"the matte holds {T + 1} mattes for a stream of {T} frames"):
        _frames(video.deblur_clip(net32, iter(clip), LABELS, matte=np.concatenate([per, per[:1]]), stream=True, horizon=24))


# ---- 8. the command line ------------------------------------------------------------------------------------------------------------------
def _main(capsys, *argv):
    video.main(["--model_path", "synthetic", "--precision", "f32", "--no_graph", "--device", DEV, *argv])
    return capsys.readouterr().out.splitlines()


def _check_log(lines, n_unmatted, n):
    assert sum(" unmatted " in ln and ln.startswith("> ") for ln in lines) == n_unmatted
    assert sum(ln.startswith("> ") for ln in lines) == n
    assert f"# unmatted {n_unmatted} of {n} frames" in lines and lines[-1].startswith(f"# {n} frames ")
    assert sum(ln.startswith("# matte ") for ln in lines) == 1


def test_cli_png(tmp_path, capsys, net32):
    from PIL import Image
    clip, per, one = _clip(T, 40, 60), _per_frame(T, 40, 60), _static(40, 60)
    src, mdir, lab = tmp_path / "in", tmp_path / "mattes", tmp_path / "labels.npy"
    src.mkdir()
    mdir.mkdir()
    for i in range(T):
        Image.fromarray(clip[i]).save(src / f"f{i:02d}.png")
        Image.fromarray(per[i]).save(mdir / f"m{i:02d}.png")
    Image.fromarray(one).save(tmp_path / "one.png")
    np.save(lab, np.asarray(LABELS))
    common = ("--input", str(src), "--labels", str(lab))

    def written(out):
        return [np.asarray(Image.open(tmp_path / out / f"f{i:02d}.png").convert("RGB")) for i in range(T)]

    lines = _main(capsys, *common, "--output", str(tmp_path / "static"), "--matte", str(tmp_path / "one.png"))
    _check_log(lines, 0, T)
    assert any(ln.startswith("# matte ") and "static" in ln for ln in lines)
    want = _frames(video.deblur_clip(net32, clip, LABELS, matte=one))
    assert all(np.array_equal(a, b) for a, b in zip(written("static"), want))
    for spec, out in ((str(mdir), "dir"), (str(mdir / "m*.png"), "glob")):
        lines = _main(capsys, *common, "--output", str(tmp_path / out), "--matte", spec)
        _check_log(lines, len(EMPTY), T)
        assert any(ln.startswith("# matte ") and f"per frame, {T} frames" in ln for ln in lines)
        want = _frames(video.deblur_clip(net32, clip, LABELS, matte=per))
        for i, img in enumerate(written(out)):
            assert np.array_equal(img, want[i]) and np.array_equal(img, clip[i]) == (i in EMPTY), i
            assert (f"> f{i:02d}.png unmatted " in "\n".join(lines)) == (i in EMPTY)
    lines = _main(capsys, *common, "--output", str(tmp_path / "inv"), "--matte", str(tmp_path / "one.png"), "--matte_invert")
    _check_log(lines, 0, T)
    assert any(ln.startswith("# matte ") and "inverted" in ln for ln in lines)
    want = _frames(video.deblur_clip(net32, clip, LABELS, matte=255 - one))
    assert all(np.array_equal(a, b) for a, b in zip(written("inv"), want))


def _records(path):
    rd = y4m.Y4MReader(str(path), depths=y4m.DEPTHS, layouts=y4m.LAYOUTS)
    return rd, [rd.raw(i).tobytes() for i in range(len(rd))]


def test_cli_y4m_and_roi_matte(tmp_path, capsys, net32):
    """y4m in and out in one layout, depth and range: an unmatted frame leaves as its input record, byte for byte, every other frame
    as the library's frame converted; the matte itself a Cmono y4m file; `--roi matte` logs the rectangle the library finds."""
    clip, per = _clip(T, 40, 60), _per_frame(T, 40, 60)
    src, lab, mpath = tmp_path / "in.y4m", tmp_path / "labels.npy", tmp_path / "matte.y4m"
    src.write_bytes(_y4m_bytes(clip, y4m.CENTER))
    np.save(lab, np.asarray(LABELS))
    with y4m.Y4MWriter(str(mpath), 60, 40, (25, 1), y4m.MONO, y4m.FULL) as wr:
        for m in per:
            wr.write(m.reshape(-1))
    _, records = _records(src)
    common = ("--input", str(src), "--labels", str(lab), "--matte", str(mpath))
    lines = _main(capsys, *common, "--output", str(tmp_path / "out.y4m"))
    _check_log(lines, len(EMPTY), T)
    rd, got = _records(tmp_path / "out.y4m")
    assert (rd.chroma, rd.depth, len(got)) == ("420jpeg", 8, T)
    run = video.deblur_clip(net32, str(src), LABELS, matte=str(mpath))
    for i, f in run:
        want = records[i] if i in EMPTY else ops.rgb_u8_to_yuv(f, *run.frames.yuv).cpu().numpy().tobytes()
        assert got[i] == want, i
        assert (got[i] == records[i]) == (i in EMPTY), i
    assert run.unmatted == EMPTY
    # another layout out: the unmatted frame is converted from the input's RGB frame
    lines = _main(capsys, *common, "--output", str(tmp_path / "k444.y4m"), "--out_chroma", "444")
    _check_log(lines, len(EMPTY), T)
    rd, got = _records(tmp_path / "k444.y4m")
    fr, inputs = _inputs(y4m.Y4MReader(str(src)))
    for i in EMPTY:
        assert got[i] == ops.rgb_u8_to_yuv(torch.from_numpy(inputs[i]).to(DEV), y4m.P444, fr.yuv[1], fr.yuv[2]).cpu().numpy().tobytes(), i
    # --roi matte, on a frame large enough for the rectangle to be smaller than it
    big, bper = _clip(T, 80, 100), np.zeros((T, 80, 100), np.uint8)
    bper[:, 30:42, 50:60] = per[:, 8:20, 20:30]
    (tmp_path / "big.y4m").write_bytes(_y4m_bytes(big, y4m.P444))
    with y4m.Y4MWriter(str(tmp_path / "bigm.y4m"), 100, 80, (25, 1), y4m.MONO, y4m.FULL) as wr:
        for m in bper:
            wr.write(m.reshape(-1))
    lines = _main(capsys, "--input", str(tmp_path / "big.y4m"), "--labels", str(lab), "--matte", str(tmp_path / "bigm.y4m"), "--roi", "matte",
                  "--output", str(tmp_path / "roi.y4m"))
    rect = MR.bbox(bper, 80, 100)
    assert "# roi " + ",".join(str(v) for v in rect) in lines
    _check_log(lines, sum(not m.any() for m in bper), T)
    _, got = _records(tmp_path / "roi.y4m")
    run = video.deblur_clip(net32, str(tmp_path / "big.y4m"), LABELS, matte=bper, roi=rect)
    _, records = _records(tmp_path / "big.y4m")
    for i, f in run:
        want = records[i] if not bper[i].any() else ops.rgb_u8_to_yuv(f, *run.frames.yuv).cpu().numpy().tobytes()
        assert got[i] == want, i
