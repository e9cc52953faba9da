"""Interlaced clips of the clip API (csrc/field_io.hip, the field entries of csrc/yuv_io.hip; video.deblur_clip(..., fields="split")) on
one MI355X -> profiles/fields_bench.json.  Three measurements, by the protocol of tools/bench_roi.py (device events around
alternating blocks of launches, each block queued behind a spin kernel, medians of 20 blocks of 50, a fresh process per configuration):

  * io: the field ingest (ops.fields_in) and the weave egress (ops.fields_out) of a 1920x1080 frame at 8 and 10 bits, beside the
    progressive launches on the same frame in the same process (ops.frames_u8_in / frames_u16_in, ops.frame_u8_out / frame_u16_out):
    the same bytes, whole frames against stride-2 rows.  The bar: 1.5 times.
  * yuv: the field-aware 4:2:0 conversions (both sitings, 8 and 10 bits, 1920x1080) beside the progressive conversion of the same
    layout, both directions.  The bar: 1.25 times.
  * clip: a synthetic 1080i clip of 8 resident frames, synthetic weights, f16 with graphs, two passes, the second with every graph
    captured: frames/s and peak allocator memory for fields="split" and for the same frames run progressive.  No bar.

    python tools/bench_fields.py [--out <json>] [--timeout SECONDS] [--skip_clip] [--kind io|yuv|clip]

Every configuration runs in a fresh child process (this file with --child) under its own `timeout -k 10`; the parent never touches the
GPU, and the run stops at the first child that does not exit 0: nothing more is started on the device after that."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_roi import BLOCKS, LAUNCHES, summary, timed_blocks      # noqa: E402  (the protocol, stated once)

H, W = 1080, 1920
DEPTHS = (8, 10)
BARS = {"io": 1.5, "yuv": 1.25}
CLIP_FRAMES = 8


def _frame(depth, seed=0):
    import numpy as np
    import torch
    D = (1 << depth) - 1
    return torch.from_numpy(np.random.default_rng(seed).integers(0, D + 1, (H, W, 3)).astype(np.uint8 if depth == 8 else np.uint16)).to("cuda:0")


def _pairs(rec, t, pairs, nbytes, bar):
    """The (new, old) pairs of one child: summaries, ratios, the bar."""
    for new, old in pairs:
        rec[new], rec[old] = summary(*t[new], nbytes[new]), summary(*t[old], nbytes[old])
        rec[f"ratio_{new}"] = rec[new]["us_median"] / rec[old]["us_median"]
    rec["ratio"] = max(rec[f"ratio_{new}"] for new, _ in pairs)
    rec["bar"] = bar
    rec["within_bar"] = rec["ratio"] <= bar


def child_io(a) -> dict:
    import torch
    from speinet_amd import ops
    torch.cuda.set_device(0)
    depth, deep = a.depth, None if a.depth == 8 else a.depth
    frame = _frame(depth)
    hp, wp, hfp = ops.padded_size(H), ops.padded_size(W), ops.padded_size(H // 2)
    whole = torch.empty(1, 3, hp, wp, device="cuda:0")
    halves = torch.empty(2, 3, hfp, wp, device="cuda:0")
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    src = torch.rand(3, hp, wp, device="cuda:0", generator=gen) * 1.2 - 0.1
    planes = [torch.rand(3, hfp, wp, device="cuda:0", generator=gen) * 1.2 - 0.1 for _ in (0, 1)]
    out = torch.empty(H, W, 3, dtype=frame.dtype, device="cuda:0")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    modes = {
        "fields_in": lambda: ops.fields_in(frame, halves, deep),
        "frames_in": (lambda: ops.frames_u8_in(frame, out=whole)) if depth == 8 else (lambda: ops.frames_u16_in(frame, depth, out=whole)),
        "fields_out": lambda: ops.fields_out(planes, H, W, depth, out=out, nonfinite=flag),
        "frame_out": ((lambda: ops.frame_u8_out(src, H, W, out=out, nonfinite=flag)) if depth == 8 else
                      (lambda: ops.frame_u16_out(src, H, W, depth, out=out, nonfinite=flag))),
    }
    for fn in modes.values():
        for _ in range(10):
            fn()
    modes["fields_in"]()
    torch.cuda.synchronize()
    top = (ops.frames_u8_in(frame[0::2].contiguous()) if depth == 8 else ops.frames_u16_in(frame[0::2].contiguous(), depth))[0][0]
    equal = bool(torch.equal(halves[0], top))
    t = timed_blocks(modes, LAUNCHES)
    sample = frame.element_size()
    packed = H * W * 3 * sample
    nbytes = {"fields_in": packed + 2 * 3 * hfp * wp * 4, "frames_in": packed + 3 * hp * wp * 4,
              "fields_out": packed + H * W * 3 * 4, "frame_out": packed + H * W * 3 * 4}
    rec = {"kind": "io", "depth": depth, "H": H, "W": W, "device": torch.cuda.get_device_name(0), "blocks": BLOCKS,
           "launches_per_block": LAUNCHES, "top_field_equals_frames_in": equal}
    _pairs(rec, t, (("fields_in", "frames_in"), ("fields_out", "frame_out")), nbytes, BARS["io"])
    if not equal:
        rec["error"] = "the field ingest differs from the frame ingest of the top field"
    return rec


def child_yuv(a) -> dict:
    import numpy as np
    import torch
    from speinet_amd import ops, y4m
    torch.cuda.set_device(0)
    depth, layout = a.depth, {"420jpeg": y4m.CENTER, "420mpeg2": y4m.LEFT}[a.layout]
    n = y4m.frame_bytes(H, W, layout)
    D = (1 << depth) - 1
    planar = torch.from_numpy(np.random.default_rng(1).integers(0, D + 1, n).astype(np.uint8 if depth == 8 else np.uint16)).to("cuda:0")
    rgb = _frame(depth, 2)
    rgb_out = torch.empty(1, H, W, 3, dtype=rgb.dtype, device="cuda:0")
    yuv_out = torch.empty(n, dtype=rgb.dtype, device="cuda:0")
    how = (layout, y4m.BT709, y4m.LIMITED)

    def to_rgb(fields):
        if depth == 8:
            return lambda: ops.yuv_to_rgb_u8(planar, H, W, *how, out=rgb_out, fields=fields)
        return lambda: ops.yuv_to_rgb_u16(planar, H, W, *how, depth, out=rgb_out, fields=fields)

    def from_rgb(fields):
        if depth == 8:
            return lambda: ops.rgb_u8_to_yuv(rgb, *how, out=yuv_out, fields=fields)
        return lambda: ops.rgb_u16_to_yuv(rgb, *how, depth, out=yuv_out, fields=fields)

    modes = {"fields_to_rgb": to_rgb(True), "to_rgb": to_rgb(False), "rgb_to_fields": from_rgb(True), "from_rgb": from_rgb(False)}
    for fn in modes.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    t = timed_blocks(modes, LAUNCHES)
    both = (n + H * W * 3) * rgb.element_size()
    rec = {"kind": "yuv", "depth": depth, "layout": a.layout, "H": H, "W": W, "device": torch.cuda.get_device_name(0), "blocks": BLOCKS,
           "launches_per_block": LAUNCHES}
    _pairs(rec, t, (("fields_to_rgb", "to_rgb"), ("rgb_to_fields", "from_rgb")), {k: both for k in modes}, BARS["yuv"])
    return rec


def child_clip(a) -> dict:
    import time
    import numpy as np
    import torch
    from speinet_amd import video
    torch.cuda.set_device(0)
    n = CLIP_FRAMES
    rng = np.random.default_rng(0)
    base = torch.from_numpy(rng.integers(0, 256, (H + 2 * n, W + 4 * n, 3), dtype=np.uint8)).to("cuda:0").float().permute(2, 0, 1)[None]
    base = torch.nn.functional.avg_pool2d(base, 5, stride=1, padding=2)[0].permute(1, 2, 0).round().to(torch.uint8)
    # 1080i: field p of frame i is the picture at instant 2 i + p, the picture moving by (1, 2) pixels per instant
    clip = torch.empty(n, H, W, 3, dtype=torch.uint8, device="cuda:0")
    for i in range(n):
        for p in (0, 1):
            k = 2 * i + p
            clip[i, p::2] = base[k:k + H, 2 * k:2 * k + W][p::2]
    labels = [1 if i % 4 == 0 else 0 for i in range(n)]
    net = video.load_model("synthetic", "cuda:0", "f16", graph=True)
    out = torch.empty(n, H, W, 3, dtype=torch.uint8, device="cuda:0")
    fields = "split" if a.fields == "split" else None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    passes = []
    for _ in range(2):                                     # the second pass finds every graph captured: the steady rate of a long clip
        t0 = time.perf_counter()
        run = video.deblur_clip(net, clip, labels, out=out, fields=fields)
        stamps = []
        for _ in run:
            torch.cuda.current_stream().synchronize()      # the frame is complete: its time
            stamps.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        passes.append(stamps)
    stamps, again = passes
    return {"kind": "clip", "fields": a.fields, "frames": n, "H": H, "W": W, "precision": "f16", "graphs": True,
            "device": torch.cuda.get_device_name(0), "seconds_at_frame": stamps, "second_pass_seconds_at_frame": again,
            "second_pass_seconds_per_frame": again[-1] / n, "second_pass_fps": n / again[-1],
            "peak_allocated_MiB": torch.cuda.max_memory_allocated() / 2 ** 20, "recomputed": len(run.recomputed),
            "no_reference_windows": sum(p["zero_pre"] for p in run.plan)}


def child(a) -> None:
    try:
        rec = {"io": child_io, "yuv": child_yuv, "clip": child_clip}[a.kind](a)
    except Exception as e:                                 # recorded, and the run ends with this child
        rec = {"kind": a.kind, "error": f"{type(e).__name__}: {e}"[:600]}
    print("RESULT " + json.dumps(rec), flush=True)
    if "error" in rec:
        sys.exit(3)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fields_bench.json"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per configuration")
    ap.add_argument("--skip_clip", action="store_true", help="the kernel timings only")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kind", choices=("io", "yuv", "clip"))
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--layout", choices=("420jpeg", "420mpeg2"), default="420jpeg")
    ap.add_argument("--fields", choices=("split", "progressive"), default="split")
    a = ap.parse_args()
    if a.child:
        return child(a)
    jobs = [["--kind", "io", "--depth", str(depth)] for depth in DEPTHS]
    jobs += [["--kind", "yuv", "--depth", str(depth), "--layout", layout] for layout in ("420jpeg", "420mpeg2") for depth in DEPTHS]
    if not a.skip_clip:
        jobs += [["--kind", "clip", "--fields", mode] for mode in ("progressive", "split")]
    if a.kind is not None:                                 # one kind of measurement only
        jobs = [j for j in jobs if j[1] == a.kind]
    res = {"method": f"one fresh process per configuration.  io and yuv: {BLOCKS} alternating blocks of {LAUNCHES} launches per mode between "
                     "two device events, each block queued behind a spin kernel so that the device and not the host's launch rate is timed "
                     "(the host's time per launch is recorded beside it), us per launch = block time / launches, medians over blocks.  "
                     f"io: ops.fields_in / ops.fields_out of a {W}x{H} frame against ops.frames_*_in / ops.frame_*_out of the same frame, "
                     f"bar {BARS['io']}.  yuv: the field-aware 4:2:0 conversions against the progressive ones of the same layout, bar "
                     f"{BARS['yuv']}.  clip: {CLIP_FRAMES} synthetic {W}x{H} interlaced frames, resident on the device, synthetic weights, "
                     "f16 with graphs, two passes, the second with every graph captured, fields=\"split\" against the same frames run "
                     "progressive; no bar",
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
    for kind in ("io", "yuv"):
        runs = [r for r in res["runs"] if r.get("kind") == kind and "ratio" in r]
        if runs:
            res[f"{kind}_worst_ratio"] = max(r["ratio"] for r in runs)
            res[f"{kind}_within_bar"] = all(r["within_bar"] for r in runs)
    clips = {r["fields"]: r for r in res["runs"] if r.get("kind") == "clip" and "second_pass_fps" in r}
    if len(clips) == 2:
        res["clip_fps"] = {k: v["second_pass_fps"] for k, v in clips.items()}
        res["clip_peak_allocated_MiB"] = {k: v["peak_allocated_MiB"] for k, v in clips.items()}
    json.dump(res, open(a.out, "w"), indent=1)
    print("done" if res["stopped"] is None else res["stopped"])
    if res["stopped"] is not None:
        sys.exit(1)


if __name__ == "__main__":
    main()
