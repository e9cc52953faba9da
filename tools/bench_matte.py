"""Mattes in the clip API (csrc/matte_io.hip spei_frame_matte_u8 / _u16; video.deblur_clip(..., matte=)) on one MI355X
-> profiles/matte_bench.json.  Two measurements, by the protocol of tools/bench_roi.py and tools/bench_keep.py (device events around
alternating blocks of launches, each block queued behind a spin kernel, medians of 20 blocks of 50 launches, a fresh process per
configuration):

  * launch: ops.frame_matte in place at 720p and 1080p for 8 -> 8 and 12 -> 12 bits, beside a device-to-device copy that moves the same
    HBM bytes in the same process.  The launch reads 7 and writes 3 bytes per pixel at 8 bits (the frame, the deblurred frame and
    the matte in, the frame out): the traffic of a copy of 5 bytes per pixel; at 16-bit samples in and out it reads 13 and writes 6,
    a copy of 9.5.  The bar, the project's for its streaming I/O launches: 1.5 times that copy.
  * clip: a synthetic 720p clip of 16 frames resident on the device, synthetic weights, f16 with graphs; wall time of a second pass
    with every graph captured.  A static matte of 255 everywhere (resident on the device) against no matte, three alternating
    repeats; the bar: the median with the matte may exceed the median without by at most the spread (max - min) of the three runs
    without, and by no less than 5 % of their median.  A per-frame matte with every other pair of frames empty is recorded as found
    and carries no bar.

    python tools/bench_matte.py [--out <json>] [--timeout SECONDS] [--kind launch|clip]

Every configuration runs in a fresh child process (this file with --child) under its own `timeout -k 10`; the parent never touches the
GPU, and the run stops at the first child that does not exit 0: nothing more is started on the device after that."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_roi import BLOCKS, LAUNCHES, SIZES, summary, timed_blocks      # noqa: E402

DEPTHS = (8, 12)                         # in and out alike
BAR = 1.5
CLIP_FRAMES = 16
REPEATS = 3


def child_launch(a) -> dict:
    import numpy as np
    import torch
    from speinet_amd import ops
    h, w = SIZES[a.size]
    torch.cuda.set_device(0)
    D = (1 << a.depth) - 1
    np_t = np.uint8 if a.depth == 8 else np.uint16
    rng = np.random.default_rng(0)
    frame_h, deb_h = (rng.integers(0, D + 1, (h, w, 3)).astype(np_t) for _ in range(2))
    matte_h = rng.integers(0, 256, (h, w)).astype(np.uint8)
    frame, deb, matte = (torch.from_numpy(x).to("cuda:0") for x in (frame_h, deb_h, matte_h))
    work = deb.clone()
    deep = None if a.depth == 8 else a.depth
    sample = frame.element_size()
    read_bytes, write_bytes = h * w * (6 * sample + 1), h * w * 3 * sample
    half = (read_bytes + write_bytes) // 2                 # a copy of this many bytes reads and writes as much as the launch moves
    big_src = torch.zeros(half, dtype=torch.uint8, device="cuda:0")
    big_dst = torch.empty_like(big_src)

    def blend():                                           # in place, as the clip loop calls it
        ops.frame_matte(frame, work, matte, a.depth, deep, out=work)

    def copy():
        big_dst.copy_(big_src)

    for fn in (blend, copy):
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    a64, b64, m64 = frame_h.astype(np.int64), deb_h.astype(np.int64), matte_h.astype(np.int64)[..., None]
    want = (a64 * (255 - m64) + b64 * m64 + 127) // 255
    equal = bool(np.array_equal(ops.frame_matte(frame, deb, matte, a.depth, deep).cpu().numpy().astype(np.int64), want))
    t = timed_blocks({"matte": blend, "copy": copy}, LAUNCHES)
    rec = {"kind": "launch", "size": a.size, "in_depth": a.depth, "out_depth": a.depth, "device": torch.cuda.get_device_name(0),
           "blocks": BLOCKS, "launches_per_block": LAUNCHES, "bytes_per_pixel_read": read_bytes / (h * w),
           "bytes_per_pixel_written": write_bytes / (h * w), "copy_bytes_per_pixel": half / (h * w),
           "matte": summary(*t["matte"], read_bytes + write_bytes), "copy": summary(*t["copy"], 2 * half), "equals_definition": equal}
    rec["ratio"] = rec["matte"]["us_median"] / rec["copy"]["us_median"]
    rec["bar"] = BAR
    rec["within_bar"] = rec["ratio"] <= BAR
    if not equal:
        rec["error"] = "the frame differs from (a * (255 - m) + b * m + 127) // 255"
    return rec


def child_clip(a) -> dict:
    import time
    import numpy as np
    import torch
    from speinet_amd import video
    h, w = SIZES["720p"]
    torch.cuda.set_device(0)
    n = CLIP_FRAMES
    base = np.random.default_rng(0).integers(0, 256, (h + n, w + 2 * n, 3), dtype=np.uint8)
    base = torch.from_numpy(base).to("cuda:0").float().permute(2, 0, 1)[None]
    base = torch.nn.functional.avg_pool2d(base, 5, stride=1, padding=2)[0].permute(1, 2, 0).round().to(torch.uint8)
    clip = torch.stack([base[i:i + h, 2 * i:2 * i + w] for i in range(n)]).contiguous()
    net = video.load_model("synthetic", "cuda:0", "f16", graph=True)
    out = torch.empty(n, h, w, 3, dtype=torch.uint8, device="cuda:0")
    labels = [0] * n
    full = torch.full((h, w), 255, dtype=torch.uint8, device="cuda:0")
    half = torch.zeros(n, h, w, dtype=torch.uint8, device="cuda:0")
    for i in range(n):
        if (i // 2) % 2 == 0:                              # alternating pairs: every other pair of frames has a subject
            half[i, h // 4:3 * h // 4, w // 4:3 * w // 4] = 255
    mattes = {"none": None, "full": full, "half_empty": half}

    def one(name) -> dict:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        run = video.deblur_clip(net, clip, labels, out=out, matte=mattes[name])
        for _ in run:
            pass
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return {"seconds": dt, "fps": n / dt, "peak_allocated_MiB": torch.cuda.max_memory_allocated() / 2 ** 20,
                "unmatted": len(run.unmatted), "recomputed": len(run.recomputed)}

    for name in mattes:                                    # the first pass captures the graphs
        one(name)
    rec = {"kind": "clip", "frames": n, "H": h, "W": w, "precision": "f16", "graphs": True, "device": torch.cuda.get_device_name(0), "runs": {}}
    pair = {"none": [], "full": []}
    for _ in range(REPEATS):                               # alternating: drift hits both alike
        for name in pair:
            pair[name].append(one(name))
    rec["runs"].update(pair)
    rec["runs"]["half_empty"] = [one("half_empty")]
    d, k = ([r["seconds"] for r in pair[name]] for name in ("none", "full"))
    spread = max(d) - min(d)
    allowance = max(spread, 0.05 * statistics.median(d))
    rec.update(none_median_s=statistics.median(d), full_median_s=statistics.median(k), none_spread_s=spread, allowance_s=allowance,
               full_minus_none_s=statistics.median(k) - statistics.median(d),
               within_bar=statistics.median(k) <= statistics.median(d) + allowance,
               half_empty_speedup=statistics.median(d) / rec["runs"]["half_empty"][0]["seconds"])
    return rec


def child(a) -> None:
    try:
        rec = {"launch": child_launch, "clip": child_clip}[a.kind](a)
    except Exception as e:                                 # recorded, and the run ends with this child
        rec = {"kind": a.kind, "error": f"{type(e).__name__}: {e}"[:600]}
    print("RESULT " + json.dumps(rec), flush=True)
    if "error" in rec:
        sys.exit(3)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matte_bench.json"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per configuration")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kind", choices=("launch", "clip"))
    ap.add_argument("--size", choices=sorted(SIZES), default="720p")
    ap.add_argument("--depth", type=int, default=8)
    a = ap.parse_args()
    if a.child:
        return child(a)
    jobs = [["--kind", "launch", "--size", size, "--depth", str(d)] for size in SIZES for d in DEPTHS]
    jobs += [["--kind", "clip"]]
    if a.kind is not None:
        jobs = [j for j in jobs if j[1] == a.kind]
    res = {"method": f"one fresh process per configuration.  launch: {BLOCKS} alternating blocks of {LAUNCHES} launches per mode between two "
                     "device events, each block queued behind a spin kernel so that the device and not the host's launch rate is timed "
                     "(the host's time per launch is recorded beside it), us per launch = block time / launches, medians over blocks; "
                     "ops.frame_matte in place on a buffer allocated once against a device-to-device copy of half the bytes the launch "
                     f"reads and writes (5 per pixel at 8 bits, 9.5 at 16-bit samples), bar {BAR}.  clip: {CLIP_FRAMES} synthetic 720p "
                     "frames resident on the device, all labelled blurry, synthetic weights, f16 with graphs; every variant runs once "
                     "untimed (its graphs are captured), then timed: wall time of a whole pass, frames/s = frames / time; no matte and a "
                     f"static matte of 255 {REPEATS} times, alternating; bar: median with the matte <= median without + max(spread of "
                     "the runs without, 5 % of their median); a per-frame matte with every other pair of frames empty once, no bar.  "
                     "Measured once",
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
    runs = [r for r in res["runs"] if r.get("kind") == "launch" and "ratio" in r]
    if runs:
        res["launch_worst_ratio"] = max(r["ratio"] for r in runs)
        res["launch_within_bar"] = all(r["within_bar"] for r in runs)
    json.dump(res, open(a.out, "w"), indent=1)
    print("done" if res["stopped"] is None else res["stopped"])
    if res["stopped"] is not None:
        sys.exit(1)


if __name__ == "__main__":
    main()
