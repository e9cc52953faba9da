"""GPU suite for the clip API (speinet_amd/video.py, csrc/frame_io.hip): the ingest and egress kernels bit for bit against the
harness's conversions, clips at multiples of 20 against the harness's PNGs, other sizes against `forward` on the reflect-padded
window, the detector's labels, device memory that does not grow with the clip, and the command line."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from speinet_amd import _lib, detector, inference, ops, selection, video      # noqa: E402
from speinet_amd.synth import synth_frames                                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _clip(T, h, w, seed=3):
    """uint8 [T,h,w,3]: the synthetic frames, shifted a little per frame (synth_clip's motion)."""
    x = synth_frames(1, h, w, seed=seed)[0]
    return np.stack([(torch.roll(x[i % 5], shifts=(i, -2 * i), dims=(1, 2)).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
                     for i in range(T)])


@pytest.fixture(scope="module")
def net32():
    return video.load_model("synthetic", DEV, "f32")


def _det_gray(frames_u8: np.ndarray) -> torch.Tensor:
    """spei_det_gray on the frames as fp32 0..255, the way the harness's labels_for feeds the detector."""
    rgb = torch.from_numpy(frames_u8.astype(np.float32)).permute(0, 3, 1, 2).contiguous().to(DEV)
    n, _, h, w = rgb.shape
    g = torch.empty(n, h, w, device=DEV)
    lib = _lib.lib()
    import ctypes as C
    _lib.check(lib.spei_det_gray(C.c_void_p(rgb.data_ptr()), C.c_void_p(g.data_ptr()), n, h, w,
                                 C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)), "spei_det_gray")
    return g


# ---- 1. ingest kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h, w", [(20, 20), (37, 53), (99, 141), (723, 1283)])
def test_ingest_kernel(h, w):
    rng = np.random.default_rng(h * 10007 + w)
    n = 3 if h < 700 else 2
    fr = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    hp, wp = video.padded_size(h), video.padded_size(w)
    ref = F.pad(selection.numpy2tensor(list(fr))[0], (0, wp - w, 0, hp - h), mode="reflect")
    dev = torch.from_numpy(fr).to(DEV)
    planes, gray = ops.frames_u8_in(dev, gray=True)
    assert planes.shape == (n, 3, hp, wp)
    assert torch.equal(planes.cpu(), ref)
    assert torch.equal(gray, _det_gray(fr))
    # one frame at a time, frames two apart in memory (frame stride), a source that starts on an odd byte, the gray plane alone
    one, _ = ops.frames_u8_in(dev[1])
    assert torch.equal(one[0], planes[1])
    big = torch.zeros(2 * n, h, w, 3, dtype=torch.uint8, device=DEV)
    big[::2] = dev
    assert torch.equal(ops.frames_u8_in(big[::2])[0], planes)
    buf = torch.zeros(n * h * w * 3 + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = dev.reshape(-1)
    assert torch.equal(ops.frames_u8_in(buf[1:].view(n, h, w, 3))[0], planes)
    p, g = ops.frames_u8_in(dev, gray=True, planes=False)
    assert p is None and torch.equal(g, gray)


def test_gray_independent_of_launch_shape():
    """Eight 723x1283 frames take some threads of spei_det_gray's grid-stride loop round twice: a pixel's gray value may not depend on
    that (the two loop versions once contracted the weighted sum differently), nor on the batch it is in."""
    fr = np.random.default_rng(1).integers(0, 256, (8, 723, 1283, 3), dtype=np.uint8)
    batch = _det_gray(fr)
    for i in (0, 5, 7):
        assert torch.equal(batch[i], _det_gray(fr[i:i + 1])[0]), i
    assert torch.equal(ops.frames_u8_in(torch.from_numpy(fr).to(DEV), gray=True, planes=False)[1], batch)


# ---- 2. egress kernel ------------------------------------------------------------------------------------------------------------
def _ties() -> np.ndarray:
    """float32 values v with fl(v * 255) == k + 0.5 exactly: round-half-even decides them."""
    out = []
    for k in range(255):
        v = np.float32((k + 0.5) / 255)
        for c in (v, np.nextafter(v, np.float32(1)), np.nextafter(v, np.float32(0))):
            if np.float32(c) * np.float32(255) == np.float32(k + 0.5):
                out.append(c)
                break
    return np.asarray(out, np.float32)


@pytest.mark.parametrize("h, w, hp, wp", [(37, 53, 40, 60), (40, 60, 40, 60), (37, 53, 37, 53), (720, 1280, 720, 1280)])
def test_egress_kernel_vs_numpy(h, w, hp, wp):
    """spei_frame_u8_out against `selection.tensor2numpy` (ties, values far outside [0, 1], the crop of a padded frame), its non-finite
    flag, and spei_frame_metrics on its frames against `selection.calc_psnr`: there is one fp32 -> uint8 kernel, the harness's too."""
    rng = np.random.default_rng(hp * wp)
    x = rng.uniform(-0.5, 1.5, (3, hp, wp)).astype(np.float32)
    ties = _ties()
    assert len(ties) > 200
    # the ties, exact 0 and 1, and values far outside [0, 1] at random places inside the crop
    sel = rng.choice(3 * h * w, size=len(ties) + 6, replace=False)
    c, r = np.divmod(sel, h * w)
    yy, xx = np.divmod(r, w)
    x[c, yy, xx] = np.concatenate([ties, np.float32([0.0, 1.0, -0.0, -3.0, 7.0, 255.0])])
    xt = torch.from_numpy(x)
    got = ops.frame_u8_out(xt.to(DEV), h, w).cpu().numpy()
    assert got.shape == (h, w, 3)
    assert np.array_equal(got, selection.tensor2numpy(xt[None, :, :h, :w]))
    assert int((np.abs(x[:, :h, :w] * 255 - np.round(x[:, :h, :w] * 255)) == 0.5).sum()) >= len(ties)
    flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)                     # cleared by the call
    ops.frame_u8_out(xt.to(DEV), h, w, nonfinite=flag)
    assert int(flag.item()) == 0
    if wp > w:                                                  # a NaN in the pad columns is not part of the crop
        xp = x.copy()
        xp[1, h - 1, w] = np.nan
        ops.frame_u8_out(torch.from_numpy(xp).to(DEV), h, w, nonfinite=flag)
        assert int(flag.item()) == 0
    # non-finite values: 0 in the frame, the flag set, and the metrics of the frame those of the numpy frame
    zeros = torch.zeros(h, w, 3, dtype=torch.uint8, device=DEV)
    for nf in ([(0, 1, 2, np.nan)], [(2, h - 1, w - 1, np.inf)], [(0, 1, 2, np.nan), (1, 3, 4, np.inf), (2, 5, 6, -np.inf)]):
        xn = x.copy()
        for c_, y_, x_, v in nf:
            xn[c_, y_, x_] = v
        got = ops.frame_u8_out(torch.from_numpy(xn).to(DEV), h, w, nonfinite=flag)
        xz = np.where(np.isfinite(xn), xn, np.float32(0))
        ref = selection.tensor2numpy(torch.from_numpy(xz)[None, :, :h, :w])
        assert np.array_equal(got.cpu().numpy(), ref)
        assert int(flag.item()) != 0
        psnr = ops.frame_metrics(got, zeros, 4)[0].item()
        assert abs(psnr - selection.calc_psnr(ref[4:-4, 4:-4], np.zeros_like(ref[4:-4, 4:-4]))) < 1e-9


# ---- 3. multiples of 20: the harness's PNGs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_clip_matches_harness(tmp_path, precision):
    T = 12
    data = inference.synth_clip(str(tmp_path), T, 100, 140)
    labels = np.asarray([1] + [0] * (T - 2) + [1])
    np.save(os.path.join(data, "label", "clip0.npy"), labels)
    plan = video.window_plan(labels)
    assert {p["zero_pre"] for p in plan} == {True, False}
    a = inference.build_args(["--data_path", data, "--model_path", "synthetic", "--result_path", str(tmp_path / "res"),
                              "--precision", precision])
    inf = inference.Inference(a)
    inf.logger.echo = False
    inf.infer()
    files = sorted(glob.glob(os.path.join(data, "blur", "clip0", "*.png")))
    frames = np.stack([inference._imread(f) for f in files])
    got = {}
    for i, t in video.deblur_clip(inf.net, frames, labels):
        assert t.shape == (100, 140, 3) and t.dtype == torch.uint8 and t.is_cuda
        got[i] = t.cpu().numpy()
    assert sorted(got) == list(range(T))
    for k in range(T):
        saved = inference._imread(os.path.join(str(tmp_path / "res"), "clip0", f"{k:06d}.png"))
        assert np.array_equal(got[k], saved), k


# ---- 4. other sizes: forward on the reflect-padded window ---------------------------------------------------------------------------
@pytest.mark.parametrize("h, w, labels", [(90, 130, [1, 1, 0, 0, 0, 0, 0, 0]), (33, 47, [0] * 8), (33, 47, [0, 0, 1, 0, 0, 1, 0, 0])])
def test_other_sizes(net32, h, w, labels):
    T = 8
    frames = _clip(T, h, w)
    hp, wp = video.padded_size(h), video.padded_size(w)
    out = torch.empty(T, h, w, 3, dtype=torch.uint8, device=DEV)
    got = list(video.deblur_clip(net32, frames, labels, out=out))
    assert [i for i, _ in got] == list(range(T))
    assert all(t.shape == (h, w, 3) and t.data_ptr() == out[i].data_ptr() for i, t in got)
    zero = np.zeros_like(frames[0])
    for p in video.window_plan(labels):
        imgs = [frames[i] for i in p["window"]] + [zero if p["zero_pre"] else frames[p["pre"]], zero if p["zero_sub"] else frames[p["sub"]]]
        x = F.pad(selection.numpy2tensor(imgs)[0], (0, wp - w, 0, hp - h), mode="reflect")[None].to(DEV)
        with torch.no_grad():
            y = net32(x, routing=[p["zero_pre"]])
        ref = selection.tensor2numpy(y[:, :, :h, :w])
        assert np.array_equal(out[p["index"]].cpu().numpy(), ref), p["index"]


# ---- 4b. a 16-bit pass that leaves the half range: recomputed in bf16x3, as the harness does ------------------------------------------
def test_non_finite_windows_recomputed(tmp_path):
    """One weight beyond +-65504 makes every f16 frame non-finite (tests/test_gpu_harness.py::test_harness_recomputes_non_finite_frames).
    deblur_clip recomputes each window in bf16x3 and records it: at 40x60 its frames equal the harness's PNGs (which the harness also
    recomputed), at 37x53 the bf16x3 forward on the reflect-padded window."""
    import warnings
    T, labels = 4, np.asarray([1, 0, 0, 1])
    data = inference.synth_clip(str(tmp_path), T, 40, 60)
    np.save(os.path.join(data, "label", "clip0.npy"), labels)
    a = inference.build_args(["--data_path", data, "--model_path", "synthetic", "--result_path", str(tmp_path / "res"), "--precision", "f16"])
    inf = inference.Inference(a)
    inf.logger.echo = False
    with torch.no_grad():
        inf.net.recons_net.outBlock[3].weight[0, 0, 0, 0] = 1.0e5
    inf.net.invalidate_packed()
    inf.infer()
    assert inf.range_retries == T
    frames = np.stack([inference._imread(f) for f in sorted(glob.glob(os.path.join(data, "blur", "clip0", "*.png")))])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        run = video.deblur_clip(inf.net, frames, labels)
        got = {i: t.cpu().numpy() for i, t in run}
    assert run.recomputed == list(range(T))
    assert sum("recomputed in bf16x3" in str(c.message) for c in caught) == T
    assert (inf.net.precision, inf.net.corr_precision, inf.net.use_graph) == ("f16", "top2", True)     # restored
    for k in range(T):
        assert np.array_equal(got[k], inference._imread(os.path.join(str(tmp_path / "res"), "clip0", f"{k:06d}.png"))), k
    # a size that is not a multiple of 20
    h, w = 37, 53
    small = frames[:, :h, :w].copy()
    got = {i: t.cpu().numpy() for i, t in video.deblur_clip(inf.net, small, labels)}
    zero = np.zeros_like(small[0])
    inf.net.precision, inf.net.corr_precision, inf.net.use_graph = "bf16x3", "bf16x3", False
    try:
        for p in video.window_plan(labels):
            imgs = [small[i] for i in p["window"]] + [zero if p["zero_pre"] else small[p["pre"]], zero if p["zero_sub"] else small[p["sub"]]]
            x = F.pad(selection.numpy2tensor(imgs)[0], (0, 60 - w, 0, 40 - h), mode="reflect")[None].to(DEV)
            with torch.no_grad():
                y = inf.net(x, routing=[p["zero_pre"]])
            assert torch.isfinite(y).all()
            assert np.array_equal(got[p["index"]], selection.tensor2numpy(y[:, :, :h, :w])), p["index"]
    finally:
        inf.net.precision, inf.net.corr_precision, inf.net.use_graph = "f16", "top2", True


# ---- 5. no labels: the LD detector -----------------------------------------------------------------------------------------------------
def _detector_clip(T, h, w, sharp):
    """uint8 [T,h,w,3] the LD detector labels sharp exactly at `sharp`: a 16-pixel sinusoidal checkerboard (which the logistic regression
    scores far above its threshold), moving one pixel per frame; every other frame box-blurred over 9 columns (far below it)."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for i in range(T):
        g = 127.5 + 127.5 * np.sin(2 * np.pi * (xx + i) / 16) * np.sin(2 * np.pi * (yy - i) / 16)
        f = np.stack([g, 0.9 * g + 12, 0.8 * g + 25], axis=2)
        if i not in sharp:
            f = sum(np.roll(f, s, axis=1) for s in range(-4, 5)) / 9
        out.append(np.round(f).clip(0, 255).astype(np.uint8))
    return np.stack(out)


def test_detector_labels(net32, tmp_path):
    from PIL import Image
    T, h, w = 20, 90, 130
    frames = _detector_clip(T, h, w, sharp=(0, 8))
    run = video.deblur_clip(net32, frames)
    outs = [t.cpu().numpy() for _, t in run]
    ref = detector.predict(detector.focus_measures(torch.from_numpy(frames).permute(0, 3, 1, 2).float().to(DEV)))
    assert set(ref.tolist()) == {0, 1}, ref
    assert np.array_equal(run.labels, ref)
    assert run.plan == video.window_plan(ref)
    assert {p["zero_pre"] for p in run.plan} == {True, False}      # both routing branches run
    # the same clip as a device tensor and as image files: same labels, same frames
    for src in (torch.from_numpy(frames).to(DEV), None):
        if src is None:
            for i in range(T):
                Image.fromarray(frames[i]).save(tmp_path / f"{i:04d}.png")
            src = sorted(str(p) for p in tmp_path.glob("*.png"))
        run2 = video.deblur_clip(net32, src)
        assert all(np.array_equal(t.cpu().numpy(), outs[i]) for i, t in run2)
        assert np.array_equal(run2.labels, ref)


# ---- 6. device memory does not grow with T ------------------------------------------------------------------------------------------
def test_memory_bounded():
    net = video.load_model("synthetic", DEV, "f32")          # a model of its own: no graphs of other shapes to trim mid-run
    frames = _clip(80, 60, 80, seed=11)
    labels = np.asarray([1 if i % 6 == 0 else 0 for i in range(80)])

    def peak(T):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        for _ in video.deblur_clip(net, frames[:T], labels[:T]):
            pass
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated()

    peak(40)                                                   # graph capture, packed weights
    p40 = max(peak(40), peak(40))                              # the allocator's timing noise at T = 40
    p80 = peak(80)
    print(f"max_memory_allocated: T=40 {p40 / 2**20:.3f} MiB, T=80 {p80 / 2**20:.3f} MiB")
    assert abs(p80 - p40) <= 0.1 * p40
    # forty more frames may not add what forty frames of any kind would: less than ONE window's fp32 input (5 padded frames, 288 KB;
    # forty uint8 frames are 576 KB, forty padded fp32 frames 2.3 MB)
    assert p80 - p40 < 5 * 3 * video.padded_size(60) * video.padded_size(80) * 4, (p40, p80)


# ---- 7. command line --------------------------------------------------------------------------------------------------------------------
def test_cli(net32, tmp_path):
    from PIL import Image
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    frames = _clip(6, 90, 130, seed=13)
    for i in range(6):
        Image.fromarray(frames[i]).save(src / f"frame_{i:03d}.png")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "speinet_amd.video", "--input", str(src), "--output", str(dst), "--model_path", "synthetic",
                        "--precision", "f32", "--device", DEV], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert not os.path.exists(tmp_path / "gt")
    names = sorted(os.listdir(dst))
    assert names == [f"frame_{i:03d}.png" for i in range(6)]
    lines = r.stdout.splitlines()
    assert sum(ln.startswith("> frame_") for ln in lines) == 6 and lines[-1].startswith("# 6 frames 130x90 in ")
    ref = dict(video.deblur_clip(net32, frames))              # the same clip through the library: the same pixels
    for i, n in enumerate(names):
        img = inference._imread(str(dst / n))
        assert img.shape == (90, 130, 3)
        assert np.array_equal(img, ref[i].cpu().numpy())


# ---- 8. the I/O launches of every clip geometry ---------------------------------------------------------------------------------------
IO_ENTRIES = ("spei_frames_u8_in", "spei_frames_u16_in", "spei_frame_u8_out", "spei_frame_u16_out", "spei_tiles_u8_in", "spei_tiles_u16_in",
              "spei_tiles_u8_out", "spei_tiles_u16_out", "spei_tiles_u8_blend", "spei_tiles_u16_blend", "spei_roi_paste_u8",
              "spei_roi_paste_u16", "spei_planes_d4", "spei_d4_mean")


def test_io_launches_per_geometry(monkeypatch):
    """The ingest, member and egress launches of a 4-frame clip, counted by entry point for every geometry: one ingest per frame of a
    window that is not zeroed (N_in over the clip, whatever the number of tiles or members), one egress per frame (T), one
    `planes_d4` per window and member after the first, one `d4_mean` per window and tile.  `tiles=(1, 1)`, `ensemble=1` and the
    rectangle that is the whole frame are the path without them, launch for launch."""
    seen = []
    orig = _lib.check

    def check(rc, what):
        seen.append(what)
        return orig(rc, what)
    monkeypatch.setattr(_lib, "check", check)
    net = video.load_model("synthetic", DEV, "f16", graph=True)
    labels, numbers, T = [1, 0, 0, 1], [0, 1, 12, 13], 4
    small, large = _clip(T, 40, 60), _clip(T, 80, 120)
    deep = small.astype(np.uint16) << 2
    cases = [
        (small, {}, lambda n: {"spei_frames_u8_in": n, "spei_frame_u8_out": T}),
        # the three "path without it" arguments, in two runs: `deblur_clip` refuses roi= together with tiles= before it looks at either
        (small, dict(tiles=(1, 1), ensemble=1), lambda n: {"spei_frames_u8_in": n, "spei_frame_u8_out": T}),
        (small, dict(ensemble=1, roi=(0, 0, 40, 60)), lambda n: {"spei_frames_u8_in": n, "spei_frame_u8_out": T}),
        (deep, dict(depth=10), lambda n: {"spei_frames_u16_in": n, "spei_frame_u16_out": T}),
        (large, dict(tiles=(2, 2)), lambda n: {"spei_tiles_u8_in": n, "spei_tiles_u8_out": T}),
        (large, dict(tiles=(2, 2), feather=8), lambda n: {"spei_tiles_u8_in": n, "spei_tiles_u8_blend": T}),
        (large, dict(roi=(10, 20, 40, 60)), lambda n: {"spei_tiles_u8_in": n, "spei_roi_paste_u8": T}),     # roi_in is the tile ingest
        (small, dict(ensemble=2), lambda n: {"spei_frames_u8_in": n, "spei_planes_d4": T, "spei_d4_mean": T, "spei_frame_u8_out": T}),
        (large, dict(tiles=(2, 2), ensemble=2),
         lambda n: {"spei_tiles_u8_in": n, "spei_planes_d4": T, "spei_d4_mean": 4 * T, "spei_tiles_u8_out": T}),
    ]
    for frames, kw, expected in cases:
        run = video.deblur_clip(net, frames, labels, numbers=numbers, **kw)
        assert {p["zero_pre"] for p in run.plan} == {True, False}, kw
        n_in = sum(key is not video.ZERO for p in run.plan for key in p["keys"])
        assert 0 < n_in < 5 * T, kw                            # some keys are ZERO
        seen.clear()
        got = [i for i, _ in run]
        torch.cuda.synchronize()
        assert got == list(range(T)) and run.recomputed == [], kw
        counts = {name: seen.count(name) for name in IO_ENTRIES}
        assert counts == {**dict.fromkeys(IO_ENTRIES, 0), **expected(n_in)}, kw
