"""GPU suite for `deblur_clip(..., matte="auto")`: the cell kernels (csrc/blur_map.hip `spei_blur_cells_u8` / `_u16`, `ops.blur_cells`)
and the matte kernel (`spei_blur_matte`, `ops.blur_matte`) against the numpy statement `blurmap_ref`, bit for bit; their refusals
through the C-ABI; the clip loop under `matte="auto"` against the run that is GIVEN the mattes the reference makes from the run's
own plan, frame by frame and bit for bit, alone and composed with the other clip features; the launches it issues, counted by
entry point; and the command line.
Synthetic weights, frames of 48x80 (80x120 under tiles), clips of 8 frames (36 where more than one analysis batch is the point)."""
import collections
import ctypes
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import blurmap_ref as BR                                           # noqa: E402
import matte_ref as MR                                             # noqa: E402
import roi_ref as RR                                               # noqa: E402
from speinet_amd import _lib, blurmap, ops, video, y4m             # noqa: E402
from speinet_amd.clip import frames_of                             # noqa: E402
from speinet_amd.synth import synth_scene_u8                       # noqa: E402

DEV = "cuda:0"
VP = ctypes.c_void_p
DEPTHS = (8, 10, 12)
SHAPES = ((1, 1), (3, 5), (16, 16), (17, 33), (21, 37), (40, 64), (48, 80))
PARAMS = ((192, 2), (0, 0), (257, 0), (128, 8))                    # (thr, flat)


def _np_dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _shifted(a, guard=0):
    """The array on the device as a view one element into a buffer (its base is not on a word boundary), and that buffer, which holds
    one guard element on either side of it."""
    buf = _dev(np.concatenate([np.full(1, guard, a.dtype), a.reshape(-1), np.full(1, guard, a.dtype)]))
    view = buf[1:-1].view(a.shape)
    assert view.data_ptr() % (4 * a.dtype.itemsize) != 0
    return view, buf


def _ramp(h, w, width, D, axis):
    """A gray frame with one linear edge of `width` pixels from D / 4 to 3 D / 4 across the middle of `axis`."""
    n = (h, w)[axis]
    lo, hi = D // 4, D - D // 4
    t = np.clip(np.arange(n) - (n // 2 - width // 2), 0, width)
    line = lo + (hi - lo) * t // width
    plane = np.broadcast_to(line[:, None] if axis == 0 else line[None, :], (h, w))
    return np.repeat(plane[..., None], 3, axis=2)


def _contents(rng, h, w, depth):
    """The frames of one case [N,H,W,3]: uniform noise (deep: a tenth of the words above D), a horizontal and a vertical ramp, noise
    whose left half went through a 9-tap horizontal box, a flat frame, and at 12 bits a 0 / D checkerboard, whose cell sums pass 2^32."""
    D, dt = (1 << depth) - 1, _np_dtype(depth)
    noise = rng.integers(0, D + 1, (h, w, 3)).astype(dt)
    if depth > 8:
        at = rng.random((h, w, 3)) < 0.1
        noise[at] = rng.integers(D + 1, 65536, int(at.sum())).astype(np.uint16)
    half = rng.integers(0, D + 1, (h, w, 3)).astype(dt)
    half[:, :max(1, w // 2)] = BR.box9(half, 1)[:, :max(1, w // 2)]
    frames = [noise, _ramp(h, w, 3, D, 1).astype(dt), _ramp(h, w, 7, D, 0).astype(dt), half, np.full((h, w, 3), D // 3, dt)]
    if depth == 12:
        yy, xx = np.mgrid[:h, :w]
        frames.append(np.repeat((((yy + xx) & 1) * D)[..., None], 3, axis=2).astype(dt))
    return np.stack(frames)


# ---- 1. the cell kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
def test_blur_cells_kernel(depth):
    """Sums and verdicts bit for bit: a lone pixel, partial cells, one whole cell, more than one strip and more than one row of cells,
    W % 4 != 0; every content; N = 3 through a strided view; the frames from a view one element into a buffer (the element path); the
    four parameter pairs.  Over the table both verdicts occur and a partial cell is lit (asserted from the reference)."""
    deep = None if depth == 8 else depth
    seen, partial_lit, past32 = set(), False, False
    for h, w in SHAPES:
        rng = np.random.default_rng(100 * h + w + depth)
        frames = _contents(rng, h, w, depth)
        n = len(frames)
        S = np.stack([BR.cell_sums(f, depth) for f in frames])
        past32 |= bool((S >= 1 << 32).any())
        whole = _dev(frames)
        strided = _dev(np.concatenate([frames.reshape(n, -1), np.zeros((n, 8 * depth), frames.dtype)], 1))[:, :h * w * 3].view(n, h, w, 3)[::2][:3]
        shifted, _ = _shifted(frames)
        for thr, flat in PARAMS:
            ref = np.stack([BR.verdict(s, h, w, depth, thr, flat) for s in S])
            seen |= set(np.unique(ref).tolist())
            px = BR.cell_pixels(h, w)
            partial_lit |= bool(((ref == 255) & (px < 256)[None]).any())
            for name, t, pick in (("whole", whole, slice(None)), ("strided", strided, slice(0, 2 * len(strided), 2)), ("shifted", shifted, slice(None))):
                cells, sums = ops.blur_cells(t, deep, thr, flat, sums=True)
                assert np.array_equal(sums.cpu().numpy(), S[pick]), (name, h, w, thr, flat)
                assert np.array_equal(cells.cpu().numpy(), ref[pick]), (name, h, w, thr, flat)
            assert np.array_equal(ops.blur_cells(whole, deep, thr, flat).cpu().numpy(), ref), ("no sums", h, w, thr, flat)
    assert seen == {0, 255} and partial_lit
    assert past32 == (depth == 12)                         # the checkerboard: a cell sum that 32 bits cannot hold


@pytest.mark.parametrize("depth", DEPTHS)
def test_blur_cells_outputs_from_offset_bases(depth):
    """The outputs in turn from a view one element into a buffer, through the C-ABI (`ops.blur_cells` allocates its own): `cells` one
    byte in, then `sums` one int64 in (the smallest offset its 8-byte alignment allows), each between guard elements that stay as
    they are, the result the reference's."""
    lib = _lib.lib()
    st = VP(torch.cuda.current_stream(DEV).cuda_stream)
    for h, w in ((21, 37), (48, 80)):
        frames = _contents(np.random.default_rng(7 * h + w + depth), h, w, depth)
        n, (ch, cw) = len(frames), BR.cell_shape(h, w)
        ref, S = BR.cells_of(frames, depth)
        src = _dev(frames)
        for shift_cells, shift_sums in ((1, 0), (0, 1), (1, 1)):
            cbuf = torch.full((n * ch * cw + 2,), 0xAB, dtype=torch.uint8, device=DEV)
            sbuf = torch.full((n * ch * cw * 4 + 2,), -77, dtype=torch.int64, device=DEV)
            cells = cbuf[shift_cells:shift_cells + n * ch * cw]
            sums = sbuf[shift_sums:shift_sums + n * ch * cw * 4]
            assert cells.data_ptr() % 4 == shift_cells and sums.data_ptr() % 16 == 8 * shift_sums
            head = (VP(src.data_ptr()), src.element_size() * src.stride(0), n, h, w)
            tail = (192, 2, VP(cells.data_ptr()), VP(sums.data_ptr()), st)
            rc = lib.spei_blur_cells_u8(*head, *tail) if depth == 8 else lib.spei_blur_cells_u16(*head, depth, *tail)
            assert rc == 0, lib.spei_last_error().decode()
            chost, shost = cbuf.cpu().numpy(), sbuf.cpu().numpy()
            inside = slice(shift_cells, shift_cells + n * ch * cw)
            assert np.array_equal(chost[inside].reshape(n, ch, cw), ref), (h, w, shift_cells, shift_sums)
            assert (np.delete(chost, np.r_[inside]) == 0xAB).all()
            inside = slice(shift_sums, shift_sums + n * ch * cw * 4)
            assert np.array_equal(shost[inside].reshape(n, ch, cw, 4), S), (h, w, shift_cells, shift_sums)
            assert (np.delete(shost, np.r_[inside]) == -77).all()


# ---- 2. the matte kernel ------------------------------------------------------------------------------------------------------------
def _maps(rng, n, ch, cw, kind):
    if kind == "zero":
        return np.zeros((n, ch, cw), np.uint8)
    if kind == "full":
        m = np.zeros((n, ch, cw), np.uint8)
        m[n - 1] = 255
        return m
    if kind == "lone":
        m = np.zeros((n, ch, cw), np.uint8)
        m[rng.integers(n), rng.integers(ch), rng.integers(cw)] = 255
        return m
    return np.where(rng.random((n, ch, cw)) < 0.3, 255, 0).astype(np.uint8)


@pytest.mark.parametrize("n", (1, 2, 3))
def test_blur_matte_kernel(n):
    """Hold, dilation and expansion in one launch against the reference: cell grids 1x1, 2x2, 2x3, 3x3, 3x4 (W % 4 != 0) and 3x5
    (two workgroups per row); every `grow`; all-0, all-255, lone-cell and random maps; the matte between guard bytes from an unaligned
    base and from an aligned one; `cell_out` given and not."""
    for h, w in ((1, 1), (20, 20), (17, 33), (33, 47), (48, 80), (40, 62)):
        ch, cw = BR.cell_shape(h, w)
        rng = np.random.default_rng(1000 * h + w + n)
        for kind in ("zero", "full", "lone", "random"):
            maps = _maps(rng, n, ch, cw, kind)
            cells = _dev(maps)
            for grow in (0, 1, 2, 4):
                cmap = BR.cell_map(maps, grow)
                ref = BR.expand(cmap, h, w)
                if kind in ("zero", "full"):
                    assert (ref == (0 if kind == "zero" else 255)).all()
                got = ops.blur_matte(cells, h, w, grow)
                assert np.array_equal(got.cpu().numpy(), ref), (h, w, kind, grow)
                buf = torch.full((h * w + 2,), 0xAB, dtype=torch.uint8, device=DEV)
                out, cout = buf[1:-1].view(h, w), torch.full((ch, cw), 7, dtype=torch.uint8, device=DEV)
                assert out.data_ptr() % 4 != 0
                ops.blur_matte(cells, h, w, grow, out=out, cell_out=cout)
                host = buf.cpu().numpy()
                assert host[0] == 0xAB and host[-1] == 0xAB and np.array_equal(host[1:-1].reshape(h, w), ref), (h, w, kind, grow)
                assert np.array_equal(cout.cpu().numpy(), cmap), (h, w, kind, grow)
                assert np.array_equal(cells.cpu().numpy(), maps)


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------------
def test_blur_refusals():
    """Refused through the C-ABI before anything is launched, each with its reason in `spei_last_error`: nothing is written."""
    H, W, N = 20, 24, 2
    ch, cw = BR.cell_shape(H, W)
    lib = _lib.lib()
    st = VP(torch.cuda.current_stream(DEV).cuda_stream)
    slots = torch.zeros(6 * 8192, dtype=torch.uint8, device=DEV)      # one buffer, a slot of 8192 bytes per operand

    def slot(k, nbytes, value):
        return slots[k * 8192:k * 8192 + nbytes].fill_(value)

    nb = H * W * 3 * 2
    src, cells, sums = slot(0, N * nb, 5), slot(2, N * ch * cw, 9), slot(3, N * ch * cw * 32, 3)
    good = dict(src=src.data_ptr(), stride=nb, N=N, H=H, W=W, depth=10, thr=192, flat=2, cells=cells.data_ptr(), sums=sums.data_ptr())

    def call16(**kw):
        a = dict(good, **kw)
        return lib.spei_blur_cells_u16(VP(a["src"]), a["stride"], a["N"], a["H"], a["W"], a["depth"], a["thr"], a["flat"], VP(a["cells"]),
                                       VP(a["sums"]), st)

    def call8(**kw):
        a = dict(dict(good, stride=nb // 2), **kw)
        return lib.spei_blur_cells_u8(VP(a["src"]), a["stride"], a["N"], a["H"], a["W"], a["thr"], a["flat"], VP(a["cells"]), VP(a["sums"]), st)

    cases = [(dict(src=None), "null pointer"), (dict(cells=None), "null pointer"),
             (dict(depth=8), "unknown depth 8"), (dict(depth=11), "unknown depth 11"), (dict(depth=0), "unknown depth 0"),
             (dict(N=0), "0 frames"), (dict(N=65536), "65536 frames"),
             (dict(H=0), "bad frame shape"), (dict(W=-1), "bad frame shape"), (dict(H=32768, W=32768), "bad frame shape"),
             (dict(stride=nb - 2), "frame stride"), (dict(src=src.data_ptr() + 1), "misaligned"), (dict(stride=nb + 1), "misaligned"),
             (dict(thr=-1), "thr -1"), (dict(thr=258), "thr 258"), (dict(flat=-1), "flat -1"), (dict(flat=256), "flat 256"),
             (dict(sums=sums.data_ptr() + 4), "sums must be 8-byte aligned"),
             (dict(cells=src.data_ptr() + N * nb - 1), "cells overlaps src"), (dict(src=cells.data_ptr() - N * nb + 2), "cells overlaps src"),
             (dict(sums=src.data_ptr() + 8), "sums overlaps src"), (dict(sums=cells.data_ptr() - N * ch * cw * 32 + 8), "sums overlaps cells")]
    for kw, text in cases:
        assert call16(**kw) != 0, kw
        err = lib.spei_last_error().decode()
        assert text in err and "spei_blur_cells_u16" in err, (kw, err)
    for kw, text in [(dict(src=None), "null pointer"), (dict(H=0), "bad frame shape"), (dict(thr=300), "thr 300"), (dict(flat=999), "flat 999"),
                     (dict(stride=nb // 2 - 1), "frame stride"), (dict(cells=src.data_ptr()), "cells overlaps src")]:
        assert call8(**kw) != 0, kw
        err = lib.spei_last_error().decode()
        assert text in err and "spei_blur_cells_u8" in err, (kw, err)
    maps, matte, cout = slot(4, 3 * ch * cw, 255), slot(5, H * W, 9), slot(1, ch * cw, 3)
    goodm = dict(cells=maps.data_ptr(), n=3, grow=1, H=H, W=W, matte=matte.data_ptr(), cell_out=cout.data_ptr())

    def callm(**kw):
        a = dict(goodm, **kw)
        return lib.spei_blur_matte(VP(a["cells"]), a["n"], a["grow"], a["H"], a["W"], VP(a["matte"]), VP(a["cell_out"]), st)

    for kw, text in [(dict(cells=None), "null pointer"), (dict(matte=None), "null pointer"), (dict(n=0), "0 verdict maps"),
                     (dict(n=9), "9 verdict maps"), (dict(grow=-1), "grow -1"), (dict(grow=5), "grow 5"),
                     (dict(H=0), "bad frame shape"), (dict(W=0), "bad frame shape"), (dict(H=65536, W=32768), "bad frame shape"),
                     (dict(matte=maps.data_ptr() + 3 * ch * cw - 1), "matte overlaps cells"), (dict(cells=matte.data_ptr() + H * W - 1), "matte overlaps cells"),
                     (dict(cell_out=maps.data_ptr()), "cell_out overlaps cells"), (dict(cell_out=matte.data_ptr() + H * W - 1), "cell_out overlaps matte")]:
        assert callm(**kw) != 0, kw
        err = lib.spei_last_error().decode()
        assert text in err and "spei_blur_matte" in err, (kw, err)
    torch.cuda.synchronize()
    host = slots.cpu().numpy()
    for k, nbytes, value in ((2, N * ch * cw, 9), (3, N * ch * cw * 32, 3), (5, H * W, 9), (1, ch * cw, 3)):
        assert (host[k * 8192:k * 8192 + nbytes] == value).all(), k       # nothing was written by a refused call
    assert call16() == 0 and call8() == 0 and call16(sums=None) == 0      # the good calls do run
    assert callm() == 0 and callm(cell_out=None) == 0
    torch.cuda.synchronize()
    assert (slots[5 * 8192:5 * 8192 + H * W] == 255).all()


# ---- 4. the clip --------------------------------------------------------------------------------------------------------------------
LABELS = [1, 0, 0, 1, 1, 0, 1, 0]
T = len(LABELS)


def _scene(h=48, w=80, depth=8, whole=(1, 2), half=(5,), t=T, seed=1700):
    """One synthetic shot; the frames `whole` went through a 9-tap horizontal box, the frames `half` with their left half only."""
    c = synth_scene_u8(t, h, w, seed)
    if depth > 8:
        c = (c.astype(np.uint16) << (depth - 8)) | (np.arange(w, dtype=np.uint16) % (1 << (depth - 8)))[None, None, :, None]
    for i in whole:
        c[i] = BR.box9(c[i], 1)
    for i in half:
        c[i][:, :w // 2] = BR.box9(c[i], 1)[:, :w // 2]
    return c


@pytest.fixture(scope="module")
def scene():
    """The clip of the issue and its reference cells, computed once."""
    clip = _scene()
    cells, sums = BR.cells_of(clip)
    return clip, cells, sums


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


def _auto_against_given(model, clip, labels, params=None, frames=None, given_clip=None, **kw):
    """`matte="auto"` against `matte=M`, M the mattes the reference makes of the frames as the loop sees them (`frames`; default:
    the clip's) with the run's own plan entries: bit for bit, frame by frame, and the same `unmatted`."""
    p = blurmap.BlurParams.of(params)
    extra = {} if params is None else dict(matte_params=params)
    run = video.deblur_clip(model, clip, labels, matte="auto", **extra, **kw)
    got = _frames(run)
    seen = np.asarray(clip if frames is None else frames)
    H, W = seen.shape[1:3]
    cells, _ = BR.cells_of(seen, kw.get("depth") or 8, p.thr, p.flat)
    assert np.array_equal(run.matte.cells, cells)
    M = BR.clip_mattes(cells, run.plan, H, W, p.grow, p.hold)
    given = video.deblur_clip(model, clip if given_clip is None else given_clip, labels, matte=M, **kw)
    want = _frames(given)
    assert len(got) == len(want) == len(seen)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and np.array_equal(a, b), (i, np.argwhere(a != b)[:5])
    assert run.unmatted == given.unmatted == [i for i in range(len(seen)) if not M[i].any()]
    assert run.plan == given.plan and run.kept == given.kept and run.recomputed == given.recomputed == []
    return run, got, M


def test_scene_has_every_case(scene):
    """What the clip tests lean on, from the reference: an untouched frame lights nothing, a blurred one nearly everything, the
    half-blurred one its left columns; under the default parameters some frame is unmatted, some matte holds 0, 255 and values
    between, and the hold changes a frame's matte."""
    clip, cells, sums = scene
    lit = [int((c != 0).sum()) for c in cells]
    assert all(lit[i] == 0 for i in (0, 3, 4, 6, 7)) and lit[1] >= 12 and lit[2] >= 12
    assert cells[5][:, :2].all() and not cells[5][:, 3:].any()
    assert (sums[..., 0] > 0).all()                        # every cell has texture: thr = 257 lights them all
    plan = video.window_plan(np.asarray(LABELS))
    held, own = BR.clip_mattes(cells, plan, 48, 80, 1, 1), BR.clip_mattes(cells, plan, 48, 80, 1, 0)
    assert any(not m.any() for m in held)
    assert any((m == 0).any() and (m == 255).any() and ((m > 0) & (m < 255)).any() for m in held)
    assert any(not np.array_equal(a, b) for a, b in zip(held, own))


@pytest.mark.parametrize("params", [None, dict(hold=0), dict(grow=0), dict(thr=128, flat=8, grow=2)], ids=["default", "hold0", "grow0", "other"])
def test_auto_is_the_given_matte(net, scene, params):
    clip = scene[0]
    run, got, M = _auto_against_given(net, clip, LABELS, params)
    assert isinstance(run.matte, blurmap.AutoMattes) and run.matte.on_device(0) and not run.matte.static
    if params is None:
        assert run.unmatted and len(run.unmatted) < T
        assert all(np.array_equal(got[i], clip[i]) for i in run.unmatted)
        assert any(not np.array_equal(got[i], clip[i]) for i in range(T))


def test_detector_labels_share_the_pass(net32, scene, monkeypatch):
    """Without labels the cells are measured in the labelling pass: one `spei_blur_cells_u8` launch for the clip's one batch."""
    clip = scene[0]
    seen = _counted(monkeypatch)
    run = video.deblur_clip(net32, clip, matte="auto", cuts="auto")
    got = _frames(run)
    n = collections.Counter(seen)
    assert n["spei_blur_cells_u8"] == 1 and n["spei_frame_pair_stats"] == 1
    M = BR.clip_mattes(scene[1], run.plan, 48, 80)
    want = _frames(video.deblur_clip(net32, clip, list(run.labels), matte=M, cuts=run.cuts))
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_every_cell_lit_is_the_run_without_a_matte(net, scene):
    clip = scene[0]
    run = video.deblur_clip(net, clip, LABELS, matte="auto", matte_params=dict(thr=257, flat=0))
    got = _frames(run)
    base = _frames(video.deblur_clip(net, clip, LABELS))
    assert run.unmatted == [] and (run.matte.cells == 255).all()
    assert all(np.array_equal(a, b) for a, b in zip(got, base))


def test_thr_0_is_the_input_and_never_calls_the_model(net32, scene, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the model was called")
    for name in ("forward_window", "forward", "prefetch_window"):
        monkeypatch.setattr(type(net32), name, boom)
    clip = scene[0]
    run = video.deblur_clip(net32, clip, LABELS, matte="auto", matte_params=dict(thr=0), out_depth=10)
    got = _frames(run)
    assert np.array_equal(np.stack(got), RR.requant(clip, 8, 10).astype(np.uint16)) and run.unmatted == list(range(T)) and run.kept == []
    run = video.deblur_clip(net32, iter(clip), LABELS, matte="auto", matte_params=dict(thr=0), stream=True, horizon=24)
    assert np.array_equal(np.stack(_frames(run)), clip) and run.unmatted == list(range(T))      # an all-sharp stream


def _counted(monkeypatch):
    seen = []
    orig = _lib.check

    def check(rc, what):
        seen.append(what)
        return orig(rc, what)
    monkeypatch.setattr(_lib, "check", check)
    return seen


NEW = ("spei_blur_cells_u8", "spei_blur_cells_u16", "spei_blur_matte")


def test_launches(net, scene, monkeypatch):
    """By entry point: no new entry is called without `matte="auto"` (a given matte included); with it one `spei_blur_cells_u8` per
    analysis batch, and one `spei_blur_matte` and one blend per matted frame; everything else is the given matte's run."""
    clip = scene[0]
    _frames(video.deblur_clip(net, clip, LABELS))              # every graph of the plan is captured before anything is counted
    seen = _counted(monkeypatch)

    def counts(**kw):
        seen.clear()
        run = video.deblur_clip(net, clip, LABELS, **kw)
        out = _frames(run)
        torch.cuda.synchronize()
        return collections.Counter(seen), out, run

    default, _, _ = counts()
    assert all(default[k] == 0 for k in NEW)
    auto, _, run = counts(matte="auto")
    matted = T - len(run.unmatted)
    assert 0 < matted < T
    assert auto["spei_blur_cells_u8"] == 1 and auto["spei_blur_cells_u16"] == 0        # 8 frames: one batch of the pass of its own
    assert auto["spei_blur_matte"] == matted == auto["spei_frame_matte_u8"] == auto["spei_frame_u8_out"]
    assert auto["spei_frame_requant"] == len(run.unmatted)
    M = BR.clip_mattes(scene[1], run.plan, 48, 80)
    given, _, _ = counts(matte=M)
    assert all(given[k] == 0 for k in NEW)
    assert auto - given == collections.Counter({"spei_blur_cells_u8": 1, "spei_blur_matte": matted}) and given - auto == collections.Counter()


# ---- 5. compositions ----------------------------------------------------------------------------------------------------------------
def _y4m_bytes(clip, layout, matrix=y4m.BT601, rng=y4m.LIMITED) -> bytes:
    f = io.BytesIO()
    wr = y4m.Y4MWriter(f, clip.shape[2], clip.shape[1], (25, 1), layout, rng)
    for frame in clip:
        wr.write(ops.rgb_u8_to_yuv(_dev(frame), layout, matrix, rng).cpu().numpy())
    return f.getvalue()


def test_tiles_with_feather(net32):
    run, _, _ = _auto_against_given(net32, _scene(80, 120), LABELS, tiles=(2, 2), feather=8)
    assert run.tiles is not None and run.tiles.n == 4 and 0 < len(run.unmatted) < T


def test_ensemble(net32, scene):
    _auto_against_given(net32, scene[0], LABELS, ensemble=2)


def test_deep_in_deeper_out(net32):
    clip = _scene(depth=10)
    run, got, _ = _auto_against_given(net32, clip, LABELS, depth=10, out_depth=12)
    assert got[0].dtype == np.uint16 and 0 < len(run.unmatted) < T


def test_y4m_420(net32, scene, tmp_path):
    path = tmp_path / "clip.y4m"
    path.write_bytes(_y4m_bytes(scene[0], y4m.CENTER))
    fr = frames_of(y4m.Y4MReader(str(path)))
    rgb = np.stack([fr.rgb(torch.from_numpy(fr.host(i)).to(DEV)[None])[0].cpu().numpy() for i in range(fr.T)])
    run, _, _ = _auto_against_given(net32, y4m.Y4MReader(str(path)), LABELS, frames=rgb, given_clip=y4m.Y4MReader(str(path)))
    assert 0 < len(run.unmatted) < T


def test_sharp_keep(net32, scene):
    run, got, _ = _auto_against_given(net32, scene[0], LABELS, sharp="keep")
    assert run.kept == [i for i, v in enumerate(LABELS) if v] and all(np.array_equal(got[i], scene[0][i]) for i in run.kept)


def test_cuts_hold_does_not_cross(net32):
    """Two scenes: the last frame of scene one is blurred, the first frame of scene two is sharp, and its matte is empty."""
    clip = np.concatenate([_scene(whole=(3,), half=(), t=4), _scene(whole=(), half=(), t=4, seed=1701)])
    run, _, M = _auto_against_given(net32, clip, LABELS, cuts=[4])
    assert 4 in run.unmatted and 3 not in run.unmatted and M[3].any()
    uncut = video.deblur_clip(net32, clip, LABELS, matte="auto")
    _frames(uncut)
    assert 4 not in uncut.unmatted                             # without the cut the hold reaches frame 3


def test_roi_matte_and_a_rectangle(net32):
    h, w = 64, 160
    clip = _scene(h, w, whole=(), half=())
    assert not BR.cells_of(clip)[0].any()                      # the untouched shot lights nothing
    for i in (2, 5):
        clip[i][:, :40] = BR.box9(clip[i], 1)[:, :40]
    cells, _ = BR.cells_of(clip)
    run = video.deblur_clip(net32, clip, LABELS, matte="auto", roi="matte", roi_feather=3)
    got = _frames(run)
    cmaps = BR.clip_cell_maps(cells, run.plan)
    ya, yb, xa, xb = BR.cell_box(cmaps, h, w)
    mask = np.zeros((h, w), np.uint8)
    mask[ya:yb, xa:xb] = 1
    rect = MR.bbox(mask, h, w)                                 # the box, grown as a given matte's is
    assert run.roi == rect and rect[3] < w
    M = BR.clip_mattes(cells, run.plan, h, w)
    assert all(not m[:, xb:].any() and not m[:ya].any() and not m[yb:].any() for m in M) and any(m[:, xb - 1].any() for m in M)
    given = video.deblur_clip(net32, clip, LABELS, matte=M, roi=rect, roi_feather=3)
    want = _frames(given)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and run.unmatted == given.unmatted and 0 < len(run.unmatted) < T
    # a given rectangle: the cells are still those of the full frames
    _auto_against_given(net32, clip, LABELS, roi=(10, 8, 44, 100))
    # and with the detector's labels of the cropped frames: the labelling pass sees the rectangle, the cells a pass of their own
    run = video.deblur_clip(net32, clip, matte="auto", roi=(10, 8, 44, 100))
    got = _frames(run)
    assert np.array_equal(run.matte.cells, cells)
    want = _frames(video.deblur_clip(net32, clip, list(run.labels), matte=BR.clip_mattes(cells, run.plan, h, w), roi=(10, 8, 44, 100)))
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_stream(net32, scene):
    clip = scene[0]
    whole = video.deblur_clip(net32, clip, LABELS, matte="auto")
    ref = _frames(whole)
    for kw in (dict(labels=LABELS), dict(labels=None), dict(labels=LABELS, roi=(4, 10, 40, 60))):
        labels = kw.pop("labels")
        run = video.deblur_clip(net32, clip, labels, matte="auto", stream="force", horizon=24, **kw)
        got = _frames(run)
        if labels is None or kw:
            whole = video.deblur_clip(net32, clip, list(run.labels), matte="auto", **kw)
            ref = _frames(whole)
        assert run.unmatted == whole.unmatted and run.plan == whole.plan and np.array_equal(run.matte.cells, scene[1])
        assert len(got) == T and all(np.array_equal(got[i], ref[i]) for i in range(T) if i not in run.assumed)


def test_more_than_one_analysis_batch(net32, monkeypatch):
    """36 frames, three analysis batches of 16, 16 and 4: windows whose frames lie in two batches (the gather), a second and a third
    `feed`, one `spei_blur_cells_u8` launch per batch; as a whole clip with given labels (the pass of its own) and with the
    detector's (the shared pass), and as a real stream (its length unknown, the old batches given up), each against `matte=M`."""
    t = 36
    clip = _scene(whole=(1, 2, 15, 16, 30), half=(5, 17, 33), t=t)
    labels = ([1, 0, 0, 1, 1, 0, 1, 0] * 5)[:t]
    cells, _ = BR.cells_of(clip)
    seen = _counted(monkeypatch)
    run, got, M = _auto_against_given(net32, clip, labels)
    assert collections.Counter(seen)["spei_blur_cells_u8"] == 3
    assert 0 < len(run.unmatted) < t and any(M[k].any() and not cells[k].any() for k in (14, 17, 31))     # lit by a neighbour's cells
    assert any(len({f // 16 for f in p["window"]}) > 1 for p in run.plan)                              # a window over two batches
    seen.clear()
    shared = video.deblur_clip(net32, clip, matte="auto")
    out = _frames(shared)
    assert collections.Counter(seen)["spei_blur_cells_u8"] == 3 and np.array_equal(shared.matte.cells, cells)
    want = _frames(video.deblur_clip(net32, clip, list(shared.labels), matte=BR.clip_mattes(cells, shared.plan, 48, 80)))
    assert all(np.array_equal(a, b) for a, b in zip(out, want))
    for kw in ({}, dict(roi=(4, 10, 40, 60))):                 # the cells in the stream's analysis pass, and in a pass of their own beside it
        seen.clear()
        stream = video.deblur_clip(net32, iter(clip), labels, matte="auto", stream=True, horizon=24, **kw)
        assert stream.frames.T is None
        out = _frames(stream)
        assert collections.Counter(seen)["spei_blur_cells_u8"] == 3 and np.array_equal(stream.matte.cells, cells)
        assert len(stream.matte._dev) < 3                      # a stream gives up the batches behind its windows
        whole = video.deblur_clip(net32, clip, labels, matte=BR.clip_mattes(cells, stream.plan, 48, 80), **kw)
        want = _frames(whole)
        assert stream.unmatted == whole.unmatted and len(out) == t
        assert all(np.array_equal(out[i], want[i]) for i in range(t) if i not in stream.assumed) and len(stream.assumed) < t


# ---- 6. the command line ------------------------------------------------------------------------------------------------------------
def _main(capsys, *argv):
    video.main(["--model_path", "synthetic", "--precision", "f32", "--no_graph", "--device", DEV, *argv])
    return capsys.readouterr().out.splitlines()


def test_cli(tmp_path, capsys, net32, scene):
    from PIL import Image
    clip, cells, _ = scene
    src, lab = tmp_path / "in", tmp_path / "labels.npy"
    src.mkdir()
    for i in range(T):
        Image.fromarray(clip[i]).save(src / f"f{i:02d}.png")
    np.save(lab, np.asarray(LABELS))
    common = ("--input", str(src), "--labels", str(lab))
    lines = _main(capsys, *common, "--output", str(tmp_path / "a.y4m"), "--matte", "auto", "--matte_out", str(tmp_path / "m.y4m"),
                  "--matte_params", "grow=2,hold=1")
    M = BR.clip_mattes(cells, video.window_plan(np.asarray(LABELS)), 48, 80, 2, 1)
    n_un = sum(not m.any() for m in M)
    assert 0 < n_un < T and f"# unmatted {n_un} of {T} frames" in lines
    assert [ln for ln in lines if ln.startswith("# matte auto: ")] == ["# matte auto: thr=192,flat=2,grow=2,hold=1, cells of 16x16: a grid of 5x3 for 80x48"]
    rd = y4m.Y4MReader(str(tmp_path / "m.y4m"), layouts=y4m.LAYOUTS)
    assert (rd.layout, rd.depth, rd.range, len(rd)) == (y4m.MONO, 8, y4m.FULL, T)
    assert all(np.array_equal(rd.raw(i).reshape(48, 80), M[i]) for i in range(T))
    lines = _main(capsys, *common, "--output", str(tmp_path / "b.y4m"), "--matte", str(tmp_path / "m.y4m"))
    assert f"# unmatted {n_un} of {T} frames" in lines
    assert (tmp_path / "a.y4m").read_bytes() == (tmp_path / "b.y4m").read_bytes()
    want = _frames(video.deblur_clip(net32, clip, LABELS, matte=M))
    out = y4m.Y4MReader(str(tmp_path / "a.y4m"))
    how = (out.layout, y4m.BT601, out.range)
    assert all(out.raw(i).tobytes() == ops.rgb_u8_to_yuv(_dev(want[i]), *how).cpu().numpy().tobytes() for i in range(T))
