"""The region of interest of the clip API (csrc/roi_io.hip; video.deblur_clip(..., roi=)) on one MI355X -> profiles/roi_bench.json.
Three measurements, by the protocol of tools/bench_tile_egress.py (device events around alternating blocks of launches, each block
queued behind a spin kernel, medians of 20 blocks, a fresh process per configuration):

  * paste: the one launch that writes a frame (ops.roi_paste) at 720p and 1080p, 8 and 12 bits, the rectangle the 2.39:1 picture area of
    the frame, feather 0 and 20, beside what it replaces in the same process: the frame egress (ops.frame_u8_out / frame_u16_out) on a
    frame of the rectangle's size plus a device-to-device copy of the whole frame.  The bar: 1.5 times that sum.
  * extent: spei_frame_extent (_u16) over 16 resident 720p frames beside spei_frame_pair_stats (_u16, with `prev`) on the same frames,
    which streams the same bytes; the C entry points into buffers allocated once.  The bar: 1.5 times.
  * clip: a synthetic 720p clip with 2.39:1 bars (536 active rows, padded to 540), synthetic weights, f16 with graphs, two passes, the
    second with every graph captured: frames/s and peak allocator memory for roi=None, the explicit rectangle and "auto", whose extra
    scan pass is included and also timed on its own.  No bar.

    python tools/bench_roi.py [--out <json>] [--timeout SECONDS] [--skip_clip] [--kind paste|extent|clip]

Every configuration runs in a fresh child process (this file with --child) under its own `timeout -k 10`; the parent never touches the
GPU, and the run stops at the first child that does not exit 0: nothing more is started on the device after that."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"720p": (720, 1280), "1080p": (1080, 1920)}
DEPTHS = (8, 12)
FEATHERS = (0, 20)
BAR = 1.5
BLOCKS, LAUNCHES = 20, 50
PLUG_CYCLES = 4_000_000          # a spin kernel in front of every timed block, long enough for the host to queue the block behind it
EXTENT_FRAMES = 16
CLIP_FRAMES = 8


def picture_area(h: int, w: int) -> tuple:
    """The 2.39:1 picture area of an h x w frame, centred, an even number of rows: (y0, x0, rh, rw)."""
    rh = int(round(w / 2.39 / 2)) * 2
    return (h - rh) // 2, 0, rh, w


def timed_blocks(modes: dict, launches: int) -> dict:
    """name -> (device us per call [BLOCKS], host us per call [BLOCKS]) of the callables in `modes`, in alternating blocks."""
    import time
    import torch
    us, host_us = {name: [] for name in modes}, {name: [] for name in modes}
    for _ in range(BLOCKS):                                # alternating blocks: drift of the clocks hits all alike
        for name, fn in modes.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(PLUG_CYCLES)                 # the block is queued behind a busy device: device time, not the launch rate
            t0.record()
            h0 = time.perf_counter()
            for _ in range(launches):
                fn()
            host_us[name].append((time.perf_counter() - h0) * 1e6 / launches)
            t1.record()
            t1.synchronize()
            us[name].append(t0.elapsed_time(t1) * 1e3 / launches)
    return {name: (us[name], host_us[name]) for name in modes}


def summary(us, host_us, nbytes=None) -> dict:
    import statistics
    med = statistics.median(us)
    rec = {"us_median": med, "us_min": min(us), "us_max": max(us), "host_us_per_launch_median": statistics.median(host_us)}
    if nbytes is not None:
        rec.update(bytes=nbytes, GB_per_s=nbytes / med / 1e3)
    return rec


def child_paste(a) -> dict:
    import numpy as np
    import torch
    from speinet_amd import ops
    h, w = SIZES[a.size]
    roi = picture_area(h, w)
    y0, x0, rh, rw = roi
    hp, wp = ops.padded_size(rh), ops.padded_size(rw)
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    src = torch.rand(3, hp, wp, device="cuda:0", generator=gen) * 1.2 - 0.1
    D = (1 << a.depth) - 1
    dtype = torch.uint8 if a.depth == 8 else torch.uint16
    frame = torch.from_numpy(np.random.default_rng(0).integers(0, D + 1, (h, w, 3)).astype(np.uint8 if a.depth == 8 else np.uint16)).to("cuda:0")
    out = torch.empty(h, w, 3, dtype=dtype, device="cuda:0")
    small = torch.empty(rh, rw, 3, dtype=dtype, device="cuda:0")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    deep = None if a.depth == 8 else a.depth

    def paste():
        ops.roi_paste(src, frame, roi, a.depth, a.feather, deep, out=out, nonfinite=flag)

    def replaced():                                        # the frame egress on a frame of the rectangle's size, and the whole frame copied
        if a.depth == 8:
            ops.frame_u8_out(src, rh, rw, out=small, nonfinite=flag)
        else:
            ops.frame_u16_out(src, rh, rw, a.depth, out=small, nonfinite=flag)
        out.copy_(frame)

    for fn in (paste, replaced):
        for _ in range(10):
            fn()
    paste()
    torch.cuda.synchronize()
    view = (lambda t: t if a.depth == 8 else t.view(torch.int16))           # the same bits: compared for equality only
    inside_ok = bool((view(out)[y0:y0 + rh][a.feather:rh - a.feather] == view(small)[a.feather:rh - a.feather]).all())
    outside_ok = bool((view(out)[:y0] == view(frame)[:y0]).all() and (view(out)[y0 + rh:] == view(frame)[y0 + rh:]).all())
    t = timed_blocks({"paste": paste, "replaced": replaced}, LAUNCHES)
    sample = 1 if a.depth == 8 else 2
    ramp_px = (2 * a.feather) * rw                         # the top and the bottom ramp: the sides lie on the frame's border
    paste_bytes = rh * rw * 3 * 4 + (h * w - rh * rw + ramp_px) * 3 * sample + h * w * 3 * sample
    replaced_bytes = rh * rw * 3 * 4 + rh * rw * 3 * sample + 2 * h * w * 3 * sample
    rec = {"kind": "paste", "size": a.size, "depth": a.depth, "feather": a.feather, "roi": list(roi), "device": torch.cuda.get_device_name(0),
           "blocks": BLOCKS, "launches_per_block": LAUNCHES, "paste": summary(*t["paste"], paste_bytes),
           "replaced": summary(*t["replaced"], replaced_bytes), "equal_inside_off_ramps": inside_ok, "equal_outside": outside_ok}
    rec["ratio"] = rec["paste"]["us_median"] / rec["replaced"]["us_median"]
    rec["bar"] = BAR
    rec["within_bar"] = rec["ratio"] <= BAR
    if not (inside_ok and outside_ok):
        rec["error"] = "the pasted frame differs from the frame egress inside the rectangle or from the input outside it"
    return rec


def child_extent(a) -> dict:
    import ctypes as C
    import numpy as np
    import torch
    from speinet_amd import _lib, ops
    h, w = SIZES["720p"]
    torch.cuda.set_device(0)
    D = (1 << a.depth) - 1
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, D + 1, (EXTENT_FRAMES, h, w, 3))
                              .astype(np.uint8 if a.depth == 8 else np.uint16)).to("cuda:0")
    prev = frames[-1].clone()
    deep = None if a.depth == 8 else a.depth
    rows, cols = ops.frame_extent(frames, deep)
    hist = torch.empty(EXTENT_FRAMES, 64, dtype=torch.int32, device="cuda:0")
    sad = torch.empty(EXTENT_FRAMES, dtype=torch.int64, device="cuda:0")
    # the C entry points themselves, into buffers allocated once: their clears and their one launch, nothing of the wrappers
    lib, vp = _lib.lib(), C.c_void_p
    st = vp(torch.cuda.current_stream().cuda_stream)
    stride = frames.stride(0) * frames.element_size()
    head = (vp(frames.data_ptr()), stride)
    tail = ((), (a.depth,))[a.depth > 8]
    fn_extent = lib.spei_frame_extent if a.depth == 8 else lib.spei_frame_extent_u16
    fn_pairs = lib.spei_frame_pair_stats if a.depth == 8 else lib.spei_frame_pair_stats_u16

    def extent(accumulate=0):
        _lib.check(fn_extent(*head, EXTENT_FRAMES, h, w, *tail, vp(rows.data_ptr()), vp(cols.data_ptr()), accumulate, st), "extent")

    def pair_stats():
        _lib.check(fn_pairs(*head, vp(prev.data_ptr()), EXTENT_FRAMES, h, w, *tail, vp(hist.data_ptr()), vp(sad.data_ptr()), st), "pair_stats")

    modes = {"extent": extent, "extent_accumulate": lambda: extent(1), "pair_stats": pair_stats}
    for fn in modes.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = timed_blocks(modes, 20)
    nbytes = frames.numel() * frames.element_size()
    rec = {"kind": "extent", "depth": a.depth, "frames": EXTENT_FRAMES, "H": h, "W": w, "device": torch.cuda.get_device_name(0),
           "blocks": BLOCKS, "launches_per_block": 20, "note": "the C entry points into buffers allocated once: two clears and one launch "
           "each; extent_accumulate clears nothing and finds its maxima already in the tables"}
    for name in modes:
        rec[name] = summary(*t[name], nbytes)
    rec["ratio"] = rec["extent"]["us_median"] / rec["pair_stats"]["us_median"]
    rec["bar"] = BAR
    rec["within_bar"] = rec["ratio"] <= BAR
    return rec


def child_clip(a) -> dict:
    import time
    import numpy as np
    import torch
    from speinet_amd import video
    h, w = SIZES["720p"]
    roi = picture_area(h, w)
    y0, _, rh, _ = roi
    torch.cuda.set_device(0)
    n = CLIP_FRAMES
    rng = np.random.default_rng(0)
    base = rng.integers(40, 256, (h + n, w + 2 * n, 3), dtype=np.uint8)             # no picture line at or below the bar level
    base = torch.from_numpy(base).to("cuda:0").float().permute(2, 0, 1)[None]
    base = torch.nn.functional.avg_pool2d(base, 5, stride=1, padding=2)[0].permute(1, 2, 0).round().to(torch.uint8)
    clip = torch.stack([base[i:i + h, 2 * i:2 * i + w] for i in range(n)]).contiguous()
    clip[:, :y0] = 16
    clip[:, y0 + rh:] = 16
    labels = [1 if i % 4 == 0 else 0 for i in range(n)]
    net = video.load_model("synthetic", "cuda:0", "f16", graph=True)
    out = torch.empty(n, h, w, 3, dtype=torch.uint8, device="cuda:0")
    how = {"none": None, "rect": roi, "auto": "auto"}[a.roi]
    scan = None
    if a.roi == "auto":                                    # the extra pass on its own: every frame of this clip is sampled (8 <= 64)
        video.active_area(clip, "cuda:0")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        video.active_area(clip, "cuda:0")
        torch.cuda.synchronize()
        scan = time.perf_counter() - t0
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    passes = []
    for _ in range(2):                                     # the second pass finds every graph captured: the steady rate of a long clip
        t0 = time.perf_counter()
        run = video.deblur_clip(net, clip, labels, out=out, roi=how)
        stamps = []
        for _ in run:
            torch.cuda.current_stream().synchronize()      # the frame is complete: its time
            stamps.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        passes.append(stamps)
    stamps, again = passes
    found = run.roi
    return {"kind": "clip", "roi_mode": a.roi, "roi": None if found is None else list(found), "frames": n, "H": h, "W": w, "precision": "f16",
            "graphs": True, "device": torch.cuda.get_device_name(0), "seconds_at_frame": stamps, "second_pass_seconds_at_frame": again,
            "second_pass_seconds_per_frame": again[-1] / n, "second_pass_fps": n / again[-1],
            "peak_allocated_MiB": torch.cuda.max_memory_allocated() / 2 ** 20, "scan_pass_seconds": scan,
            "bars_untouched": bool((out[:, :y0] == clip[:, :y0]).all() and (out[:, y0 + rh:] == clip[:, y0 + rh:]).all()),
            "recomputed": len(run.recomputed), "no_reference_windows": sum(p["zero_pre"] for p in run.plan)}


def child(a) -> None:
    try:
        rec = {"paste": child_paste, "extent": child_extent, "clip": child_clip}[a.kind](a)
    except Exception as e:                                 # recorded, and the run ends with this child
        rec = {"kind": a.kind, "error": f"{type(e).__name__}: {e}"[:600]}
    print("RESULT " + json.dumps(rec), flush=True)
    if "error" in rec:
        sys.exit(3)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_bench.json"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per configuration")
    ap.add_argument("--skip_clip", action="store_true", help="the kernel timings only")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kind", choices=("paste", "extent", "clip"))
    ap.add_argument("--size", choices=sorted(SIZES), default="720p")
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--feather", type=int, default=0)
    ap.add_argument("--roi", choices=("none", "rect", "auto"), default="none")
    a = ap.parse_args()
    if a.child:
        return child(a)
    jobs = [["--kind", "paste", "--size", size, "--depth", str(depth), "--feather", str(f)] for size in SIZES for depth in DEPTHS
            for f in FEATHERS]
    jobs += [["--kind", "extent", "--depth", str(depth)] for depth in DEPTHS]
    if not a.skip_clip:
        jobs += [["--kind", "clip", "--roi", mode] for mode in ("none", "rect", "auto")]
    if a.kind is not None:                                 # one kind of measurement only
        jobs = [j for j in jobs if j[1] == a.kind]
    res = {"method": f"one fresh process per configuration.  paste and extent: {BLOCKS} alternating blocks of launches per mode between two "
                     "device events, each block queued behind a spin kernel so that the device and not the host's launch rate is timed "
                     "(the host's time per launch is recorded beside it), us per launch = block time / launches, medians over blocks.  "
                     f"paste: ops.roi_paste on the 2.39:1 picture area against the frame egress of that rectangle plus a device-to-device "
                     f"copy of the whole frame, bar {BAR}.  extent: spei_frame_extent over {EXTENT_FRAMES} resident 720p frames against "
                     f"spei_frame_pair_stats with prev on the same frames, bar {BAR}.  clip: {CLIP_FRAMES} synthetic 720p frames with 2.39:1 "
                     "bars, resident on the device, synthetic weights, f16 with graphs, two passes, the second with every graph captured; "
                     "auto includes its scan pass, which is also timed alone",
           "runs": [], "stopped": None}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for job in jobs:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", *job]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        rec = json.loads(lines[-1][7:]) if lines else {"job": job}
        rec["exit"] = r.returncode
        if not lines:
            rec["stderr_tail"] = r.stderr[-600:]
        res["runs"].append(rec)
        print(json.dumps(rec), flush=True)
        json.dump(res, open(a.out, "w"), indent=1)         # after every child: a stop leaves what was measured
        if r.returncode != 0:
            res["stopped"] = f"{' '.join(job)} ended in {r.returncode}: nothing was started after it"
            break
    for kind in ("paste", "extent"):
        runs = [r for r in res["runs"] if r.get("kind") == kind and "ratio" in r]
        if runs:
            res[f"{kind}_worst_ratio"] = max(r["ratio"] for r in runs)
            res[f"{kind}_within_bar"] = all(r["within_bar"] for r in runs)
    json.dump(res, open(a.out, "w"), indent=1)
    print("done" if res["stopped"] is None else res["stopped"])
    if res["stopped"] is not None:
        sys.exit(1)


if __name__ == "__main__":
    main()
