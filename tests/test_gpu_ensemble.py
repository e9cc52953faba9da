"""GPU suite for the clip API's geometric self-ensemble (speinet_amd/ensemble.py, csrc/ensemble_io.hip, video.deblur_clip(...,
ensemble=)): the plane transform and the member mean bit for bit against the numpy restatement in tests/ensemble_ref.py, their
refusals, and an ensemble clip against the composition of its parts (ingest, numpy transform, `forward_window` per member, numpy
mean, egress).  No tolerances anywhere."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ensemble_ref as R                                                       # noqa: E402
from speinet_amd import _lib, ops, video                                       # noqa: E402
from speinet_amd import ensemble as E                                          # noqa: E402
from speinet_amd import tiles as T                                             # noqa: E402
from speinet_amd.speinet import EncoderCache                                   # noqa: E402
from speinet_amd.synth import synth_frames                                     # noqa: E402

DEV = "cuda:0"
VP = ctypes.c_void_p


def _bits(t) -> np.ndarray:
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int32)


def _stream():
    return VP(torch.cuda.current_stream(DEV).cuda_stream)


# ---- 1. spei_planes_d4 ---------------------------------------------------------------------------------------------------------------
# 20x20, 40x60, 60x100 and 128x128: multiples of 4, the 16-byte path (60x100 crosses the 32-wide tiles in both axes); 7x13, 33x64 and
# 64x33: element by element, with odd edges against the LDS tile
SIZES = [(20, 20), (40, 60), (60, 100), (7, 13), (33, 64), (64, 33), (128, 128)]
SPECIAL = np.array([0x7fc00123, 0xffc0beef, 0x7f800001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001], dtype=np.uint32)   # NaNs with
# payloads (quiet, negative, signalling), +-inf, -0.0, a denormal


def _planes(n, h, w, seed):
    """n planes of uniform values with the special words at random places, as int32 words [n, h, w]."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.5, 1.5, (n, h, w)).astype(np.float32).view(np.uint32)
    where = rng.choice(a.size, size=3 * len(SPECIAL), replace=False)
    a.reshape(-1)[where] = np.tile(SPECIAL, 3)
    a[0, 0, 0], a[-1, -1, -1] = SPECIAL[0], SPECIAL[1]                             # the corners
    return a.view(np.int32)


def _strided(words: np.ndarray, pad: int, lead: int = 0):
    """The planes on the device at a plane stride of h * w + pad floats, `lead` floats into their allocation: an fp32 view [n, h, w]."""
    n, h, w = words.shape
    buf = torch.zeros(lead + n * (h * w + pad), dtype=torch.int32, device=DEV)
    view = buf[lead:].view(n, h * w + pad)[:, :h * w].view(n, h, w)
    view.copy_(torch.from_numpy(words).to(DEV))
    return view.view(torch.float32)


@pytest.mark.parametrize("h, w", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_planes_d4(h, w):
    for n in (1, 3, 15):
        words = _planes(n, h, w, seed=h * 1000 + w + n)
        x = _strided(words, pad=4 if n > 1 else 0)                                 # a stride above h * w that keeps the 16-byte path
        assert n == 1 or x.stride(0) == h * w + 4
        x_odd = _strided(words, pad=3, lead=1)                                     # one float into the allocation: unaligned
        assert x_odd.data_ptr() % 16 == 4
        for g in range(8):
            want = R.t_op(words, g)                                                # the words themselves: no float ever touches them
            got = ops.planes_d4(x, g)
            assert got.is_contiguous() and tuple(got.shape) == (n,) + E.shape_of(h, w, g)
            assert np.array_equal(_bits(got), want), (n, g)
            # into a strided destination; the slack between its planes stays as it was
            hh, ww = E.shape_of(h, w, g)
            dst = torch.full((n, h * w + 8), -7.0, device=DEV)
            out = dst[:, :h * w].view(n, hh, ww)
            assert ops.planes_d4(x, g, out=out).data_ptr() == dst.data_ptr()
            assert np.array_equal(_bits(out), want) and (dst[:, h * w:] == -7.0).all()
            # the unaligned call equals the aligned one
            got_odd = ops.planes_d4(x_odd, g)
            assert np.array_equal(_bits(got_odd), want), (n, g, "unaligned")
            # the inverse member restores x
            back = ops.planes_d4(got, E.inverse_member(g))
            assert np.array_equal(_bits(back), words), (n, g, "inverse")


def test_planes_d4_refusals():
    lib = _lib.lib()
    h, w, n = 20, 40, 2
    src = torch.arange(n * h * w + 64, dtype=torch.float32, device=DEV)
    dst = torch.full((n * h * w + 64,), 5.0, device=DEV)
    st = _stream()
    calls = [((VP(0), h * w, VP(dst.data_ptr()), h * w, n, h, w, 1), "null pointer"),
             ((VP(src.data_ptr()), h * w, VP(0), h * w, n, h, w, 1), "null pointer"),
             ((VP(src.data_ptr()), h * w, VP(dst.data_ptr()), h * w, n, h, w, 8), "outside 0..7"),
             ((VP(src.data_ptr()), h * w, VP(dst.data_ptr()), h * w, n, h, w, -1), "outside 0..7"),
             ((VP(src.data_ptr()), h * w - 1, VP(dst.data_ptr()), h * w, n, h, w, 4), "smaller than a plane"),
             ((VP(src.data_ptr()), h * w, VP(dst.data_ptr()), h * w - 4, n, h, w, 4), "smaller than a plane"),
             ((VP(src.data_ptr()), h * w, VP(dst.data_ptr()), h * w, n, 0, w, 0), "bad plane shape")]
    for args, text in calls:
        assert lib.spei_planes_d4(*args, st) != 0
        assert text in lib.spei_last_error().decode(), text
    keep = src.clone()
    for off in (0, 16, n * h * w - 1):                                             # in place, shifted, the last float on the first
        assert lib.spei_planes_d4(VP(src.data_ptr()), h * w, VP(src.data_ptr() + 4 * off), h * w, n, h, w, 3, st) != 0
        assert "overlap" in lib.spei_last_error().decode()
    torch.cuda.synchronize()
    assert (dst == 5.0).all() and torch.equal(src, keep)                          # nothing was written: nothing ran
    x = src[:n * h * w].view(n, h, w)
    with pytest.raises(ValueError, match="0..7"):
        ops.planes_d4(x, 8)
    with pytest.raises(RuntimeError, match="overlap"):
        ops.planes_d4(x, 3, out=x)
    with pytest.raises(ValueError, match="contiguous planes"):
        ops.planes_d4(x[:, :, ::2], 1)


# ---- 2. spei_d4_mean -----------------------------------------------------------------------------------------------------------------
# 20x40, 60x100 and 64x36: the 16-byte path, one tile, edges in both axes, a tile edge at 32 of 36; 7x13 and 37x66: element by element
MEAN_SIZES = [(20, 40), (60, 100), (64, 36), (7, 13), (37, 66)]
TABLES = {1: [(0,), (7,)], 2: [(0, 1), (6, 3)], 4: [(0, 1, 2, 3), (5, 0, 3, 6)], 8: [tuple(range(8)), (7, 2, 5, 0, 3, 6, 1, 4)]}


def _terms(k, c, h, w, seed):
    """The K terms m_k [c, h, w] of a mean, in canonical orientation, with planted values that make the order of the sum, a NaN, an
    infinity against its opposite, and -0.0 visible; and the planted places."""
    rng = np.random.default_rng(seed)
    m = rng.uniform(-0.5, 1.5, (k, c, h, w)).astype(np.float32)
    order, nan, infs, zero = (0, 1, 2), (1, h - 1, w - 1), (2, h // 2, 0), (0, 0, w - 1)
    pattern = np.float32([1e8, 1.0, -1e8, 0.25, 3.0, -1e8, 1e8, 0.5])               # any other order of the first three gives another sum
    m[(slice(None),) + order] = pattern[:k]
    m[(k - 1,) + nan] = np.nan
    m[(0,) + infs] = np.inf
    if k > 1:
        m[(1,) + infs] = -np.inf
    m[(slice(None),) + zero] = -0.0
    return m, order, nan, infs, zero


@pytest.mark.parametrize("h, w", MEAN_SIZES, ids=[f"{h}x{w}" for h, w in MEAN_SIZES])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_d4_mean(k, h, w):
    c = 3
    terms, order, nan, infs, zero = _terms(k, c, h, w, seed=k * 100000 + h * 100 + w)
    for table in TABLES[k]:
        host = [R.t_op(terms[i], g) for i, g in enumerate(table)]                  # member i is T_g of its term
        members = [torch.from_numpy(a).to(DEV) for a in host]                      # separate allocations
        want = R.mean(host, table)
        got = ops.d4_mean(members, table)
        assert tuple(got.shape) == (c, h, w)
        assert R.same_bits_or_nan(got.cpu().numpy(), want), (table,)
        # what was planted is what the definition says of it
        assert np.isnan(want[nan]) and np.signbit(want[zero]) and want[zero] == 0.0
        assert np.isnan(want[infs]) if k > 1 else np.isposinf(want[infs])
        if k >= 4:                                                                 # the order is visible: the reversed table sums otherwise
            assert R.mean(host[::-1], table[::-1])[order] != want[order]
        # into a destination, and from members one float into their allocations (element by element): the same bits
        out = torch.full((c, h, w), -7.0, device=DEV)
        assert ops.d4_mean(members, table, out=out).data_ptr() == out.data_ptr()
        assert R.same_bits_or_nan(out.cpu().numpy(), want)
        odd = []
        for a in host:
            buf = torch.zeros(a.size + 1, device=DEV)
            buf[1:] = torch.from_numpy(a).to(DEV).reshape(-1)
            odd.append(buf[1:].view(a.shape))
        assert R.same_bits_or_nan(ops.d4_mean(odd, table).cpu().numpy(), want), (table, "unaligned")
    if k == 1:                                                                     # the inverse transform, copied as bits: NaN payloads survive
        words = _planes(c, h, w, seed=h + w)
        for g in (0, 3, 5):
            member = torch.from_numpy(R.t_op(words, g)).to(DEV).view(torch.float32)
            assert np.array_equal(_bits(ops.d4_mean([member], [g])), words), g


def test_d4_mean_refusals():
    lib = _lib.lib()
    c, h, w = 3, 20, 40
    members = [torch.ones(c, h, w, device=DEV) for _ in range(8)]
    dst = torch.full((c, h, w), 5.0, device=DEV)
    st = _stream()

    def call(ptrs, table, k, out=dst):
        return lib.spei_d4_mean((VP * len(ptrs))(*ptrs), (ctypes.c_int * len(table))(*table), k, VP(out.data_ptr()), c, h, w, st)

    ptrs = [m.data_ptr() for m in members]
    for k in (0, 3, 5, 16):
        assert call(ptrs * 2, list(range(8)) * 2, k) != 0
        assert "(1, 2, 4 or 8)" in lib.spei_last_error().decode()
    assert call(ptrs[:4], [0, 1, 8, 3], 4) != 0
    assert "member 2 has op 8" in lib.spei_last_error().decode()
    assert call(ptrs[:1] + [0], [0, 1], 2) != 0
    assert "member 1 is a null" in lib.spei_last_error().decode()
    assert call(ptrs[:2], [0, 1], 2, out=members[1]) != 0
    assert "dst overlaps member 1" in lib.spei_last_error().decode()
    assert lib.spei_d4_mean(None, (ctypes.c_int * 2)(0, 1), 2, VP(dst.data_ptr()), c, h, w, st) != 0
    assert "null pointer" in lib.spei_last_error().decode()
    torch.cuda.synchronize()
    assert (dst == 5.0).all() and all((m == 1.0).all() for m in members)          # nothing was written: nothing ran
    with pytest.raises(ValueError, match="1, 2, 4 or 8 members"):
        ops.d4_mean(members[:3], [0, 1, 2])
    with pytest.raises(ValueError, match="shape"):
        ops.d4_mean(members[:2], [0, 4])                                           # a 20x40 member cannot be the transposed one
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.d4_mean(members[:2], [0, 1], out=members[0])


# ---- 3. the clip loop ------------------------------------------------------------------------------------------------------------------
LABELS, CUTS = [0, 1, 0, 0, 0, 0], [3]     # a sharp frame in the first scene, none in the second
# Frame numbers with gaps in the second scene.  A scene without a sharp frame takes its references from its own far end, and those are
# zeroed only when more than 7 frame numbers away: counted in indices, a three-frame scene never routes to the no-reference branch,
# and the plan would hold no window with `zero_pre`.  With these numbers window 4 does, so both routings run.
NUMBERS = [0, 1, 2, 13, 23, 33]
MODES = {"f16-graph": ("f16", True), "f32-eager": ("f32", False)}


def _clip(n, h, w, seed=3):
    """uint8 [n,h,w,3]: the synthetic frames, shifted a little per frame (tests/test_gpu_video.py's)."""
    x = synth_frames(1, h, w, seed=seed)[0]
    return np.ascontiguousarray(np.stack([(torch.roll(x[i % 5], shifts=(i, -2 * i), dims=(1, 2)).permute(1, 2, 0).numpy() * 255)
                                          .round().astype(np.uint8) for i in range(n)]))


def _frames(run) -> np.ndarray:
    got = {i: t.cpu().numpy() for i, t in run}
    assert sorted(got) == list(range(len(got)))
    return np.stack([got[i] for i in range(len(got))])


@pytest.fixture(scope="module")
def nets():
    return {mode: video.load_model("synthetic", DEV, precision, graph=graph) for mode, (precision, graph) in MODES.items()}


def _window_input(frames_dev, keys) -> torch.Tensor:
    """The padded fp32 window input [1, 5, 3, Hp, Wp] of one window of one (cropped) clip: the frame ingest, zeros for `video.ZERO`."""
    h, w = frames_dev.shape[1:3]
    x = torch.zeros(1, len(keys), 3, ops.padded_size(h), ops.padded_size(w), device=DEV)
    for j, key in enumerate(keys):
        if key is not video.ZERO:
            ops.frames_u8_in(frames_dev[key], out=x[0, j])
    return x


def _member_outputs(run_member, frames, plan, k):
    """Per window of `plan`, the raw outputs of the members 0..k-1 (each still in its member's orientation): member g is
    `run_member(T_g(x), g, window)` on the ingested window input x, with the transform done in numpy."""
    frames_dev = torch.from_numpy(frames).to(DEV)
    outs = []
    for p in plan:
        x = _window_input(frames_dev, p["keys"]).cpu().numpy()
        outs.append([run_member(torch.from_numpy(R.t_op(x, g)).to(DEV), g, p).cpu().numpy() for g in range(k)])
    return outs


def _through_windows(net, tag):
    """`run_member` for `_member_outputs`: `forward_window` with a fresh encoder cache, in the arithmetic and graph setting of `net`."""
    enc = EncoderCache(EncoderCache().capacity * 8)

    def run_member(x, g, p):
        return net.forward_window(x, [(tag, g, key) for key in p["keys"]], enc, zero_ref=p["zero_pre"])[0]
    return run_member


@pytest.fixture(scope="module")
def clip_parts(nets):
    """The 6-frame 44x68 clip (padded to 60x80: the transposed members are 80x60, and a flipped member has its pad at the top or left),
    its plan and, per mode, every window's eight member outputs, computed once."""
    frames = _clip(6, 44, 68)
    plan = video.window_plan(LABELS, numbers=NUMBERS, cuts=CUTS)
    assert any(p["zero_pre"] for p in plan) and any(not p["zero_pre"] for p in plan)
    with torch.no_grad():
        parts = {mode: _member_outputs(_through_windows(net, "parts"), frames, plan, 8) for mode, net in nets.items()}
    return frames, plan, parts


def _egress(mean: np.ndarray, h, w) -> np.ndarray:
    return ops.frame_u8_out(torch.from_numpy(mean).to(DEV), h, w).cpu().numpy()


@pytest.mark.parametrize("k", [2, 8])
@pytest.mark.parametrize("mode", list(MODES))
def test_ensemble_clip_equals_its_composition(nets, clip_parts, mode, k):
    net = nets[mode]
    frames, plan, parts = clip_parts
    if k == 8:                                             # as a fresh model: what a clip of two frame shapes captures, from nothing
        torch.cuda.synchronize()
        net._graphs.clear()
    run = video.deblur_clip(net, frames, LABELS, numbers=NUMBERS, cuts=CUTS, ensemble=k)
    assert run.ensemble == k and run.tiles is None
    assert [(p["keys"], p["zero_pre"]) for p in run.plan] == [(p["keys"], p["zero_pre"]) for p in plan]
    assert any(p["zero_pre"] for p in run.plan) and any(not p["zero_pre"] for p in run.plan)
    got, counts = {}, []
    for i, t in run:
        got[i] = t.cpu().numpy()
        counts.append(len(net._graphs))
    assert sorted(got) == list(range(6)) and run.recomputed == []
    print(f"ensemble {k} {mode}: captured graphs after each frame handed out {counts}, GRAPH_LIMIT {net.GRAPH_LIMIT}")
    assert counts == sorted(counts), "a trim dropped the captured graphs in the middle of the clip"
    for f in range(6):
        want = _egress(R.mean(parts[mode][f][:k], list(range(k))), 44, 68)
        assert np.array_equal(got[f], want), f


@pytest.mark.parametrize("mode", list(MODES))
def test_ensemble_1_is_the_call_without_it(nets, mode):
    frames = _clip(6, 44, 68)
    ref = _frames(video.deblur_clip(nets[mode], frames, LABELS, numbers=NUMBERS, cuts=CUTS))
    run = video.deblur_clip(nets[mode], frames, LABELS, numbers=NUMBERS, cuts=CUTS, ensemble=1)
    assert run.ensemble == 1
    assert np.array_equal(_frames(run), ref)


def test_ensemble_with_feathered_tiles(nets):
    """80x120 in 2x2 tiles with feathered seams, two members, f32 eager: every tile's window is the composition above, and the tiles'
    means are stitched by `ops.tiles_out` with the plan."""
    net = nets["f32-eager"]
    labels = [0, 1, 0, 0]
    frames = _clip(4, 80, 120)
    tp = T.tile_plan(80, 120, (2, 2), 20, 8)
    run = video.deblur_clip(net, frames, labels, tiles=(2, 2), feather=8, ensemble=2)
    assert run.tiles == tp and run.tiles.feather == 8 and run.ensemble == 2
    got = _frames(run)
    plan = video.window_plan(labels)
    per_tile = []
    with torch.no_grad():
        for i in range(tp.rows):
            for j in range(tp.cols):
                crop = np.ascontiguousarray(frames[:, tp.y0[i]:tp.y0[i] + tp.th, tp.x0[j]:tp.x0[j] + tp.tw])
                per_tile.append(_member_outputs(_through_windows(net, ("tile", i, j)), crop, plan, 2))
    for f in range(4):
        means = [torch.from_numpy(R.mean(per_tile[t][f], [0, 1])).to(DEV) for t in range(tp.n)]
        assert np.array_equal(got[f], ops.tiles_out(means, tp, 8).cpu().numpy()), f


# ---- 4. a 16-bit pass that leaves the half range -----------------------------------------------------------------------------------------
def test_ensemble_non_finite_windows_recomputed():
    """One weight beyond +-65504 makes every f16 frame non-finite (tests/test_gpu_video.py::test_non_finite_windows_recomputed), in
    every member: the window is recomputed in bf16x3 with all K members, and the frame is the composition of those."""
    net = video.load_model("synthetic", DEV, "f16", graph=True)
    with torch.no_grad():
        net.recons_net.outBlock[3].weight[0, 0, 0, 0] = 1.0e5
    net.invalidate_packed()
    frames, labels = _clip(4, 37, 53), [1, 0, 0, 1]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        run = video.deblur_clip(net, frames, labels, ensemble=4)
        got = _frames(run)
    assert run.recomputed == [0, 1, 2, 3]
    assert sum("recomputed in bf16x3" in str(c.message) for c in caught) == 4
    assert (net.precision, net.corr_precision, net.use_graph) == ("f16", "top2", True)     # restored
    net.precision, net.corr_precision, net.use_graph = "bf16x3", "bf16x3", False
    with torch.no_grad():
        parts = _member_outputs(lambda x, g, p: net(x, routing=[p["zero_pre"]])[0], frames, run.plan, 4)
    for f in range(4):
        mean = R.mean(parts[f], [0, 1, 2, 3])
        assert np.isfinite(mean[:, :37, :53]).all()
        assert np.array_equal(got[f], _egress(mean, 37, 53)), f


# ---- 5. the command line -----------------------------------------------------------------------------------------------------------------
def test_cli_ensemble(nets, tmp_path, capsys):
    """`python -m speinet_amd.video --ensemble 2` (its `main`, in this process) writes the frames the library yields and names the mode."""
    from PIL import Image
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    frames = _clip(4, 40, 60, seed=13)
    for i in range(4):
        Image.fromarray(frames[i]).save(src / f"frame_{i:03d}.png")
    labels = np.asarray([0, 1, 0, 0])
    np.save(tmp_path / "labels.npy", labels)
    video.main(["--input", str(src), "--output", str(dst), "--model_path", "synthetic", "--labels", str(tmp_path / "labels.npy"),
                "--device", DEV, "--ensemble", "2"])
    text = capsys.readouterr().out
    assert "# ensemble 2: members 0..1" in text and "(f16, ensemble 2)" in text and text.count("> frame_") == 4
    ref = _frames(video.deblur_clip(nets["f16-graph"], frames, labels, ensemble=2))
    for i in range(4):
        assert np.array_equal(np.asarray(Image.open(dst / f"frame_{i:03d}.png").convert("RGB")), ref[i]), i
    with pytest.raises(SystemExit):
        video.main(["--input", str(src), "--output", str(dst), "--model_path", "synthetic", "--device", DEV, "--ensemble", "3"])
