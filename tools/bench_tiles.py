"""Throughput and device memory of the clip API with and without tiles (video.deblur_clip(..., tiles=), speinet_amd/tiles.py) on a
synthetic clip of a few frames at 1080p and 2160p, in f16, on one MI355X -> profiles/tiles_bench.json.

    python tools/bench_tiles.py [--out <json>] [--frames N] [--timeout SECONDS]

Every configuration runs in a fresh child process (this file with --child) under its own `timeout -k 10`, the tiled ones first and
untiled 2160p last: the untiled correlation of a 2160p frame is the one that may not fit.  The parent never touches the GPU.  A child
records frames/s over the whole clip (graph captures of the first windows included: with so few frames the figure is a lower bound
of the steady state), the frames/s of the clip's second half, and torch.cuda.max_memory_allocated; a Python exception in the child,
is a recorded result; an out-of-memory error is no failure (the child still exits 0), any other exception makes the child exit 3.
The run stops at the first child that does not exit 0 (124, 134, 137 and 139 among them: a time limit, an abort, a kill, a
segmentation fault): nothing more is started on the device after that."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"1080p": (1080, 1920), "2160p": (2160, 3840)}
ORDER = [("1080p", "auto"), ("1080p", "2x2"), ("2160p", "auto"), ("2160p", "2x2"), ("1080p", "none"), ("2160p", "none")]


def child(a) -> None:
    import numpy as np
    import torch
    from speinet_amd import tiles as tiling, video
    h, w = SIZES[a.size]
    rec = {"size": a.size, "tiles": a.tiles, "frames": a.frames}
    try:
        torch.cuda.set_device(0)
        rec["device"] = torch.cuda.get_device_name(0)
        rng = np.random.default_rng(0)
        base = rng.integers(0, 256, (h + a.frames, w + 2 * a.frames, 3), dtype=np.uint8)
        # a smooth random image moving a pixel or two per frame, on the device (no decode, no upload in the timed part)
        base = torch.from_numpy(base).to("cuda:0").float().permute(2, 0, 1)[None]
        base = torch.nn.functional.avg_pool2d(base, 5, stride=1, padding=2)[0].permute(1, 2, 0).round().to(torch.uint8)
        clip = torch.stack([base[i:i + h, 2 * i:2 * i + w] for i in range(a.frames)]).contiguous()
        labels = [1 if i % 4 == 0 else 0 for i in range(a.frames)]
        net = video.load_model("synthetic", "cuda:0", "f16", graph=True)
        run = video.deblur_clip(net, clip, labels, tiles=tiling.parse_tiles(a.tiles))
        rec["plan"] = None if run.tiles is None else {"rows": run.tiles.rows, "cols": run.tiles.cols, "th": run.tiles.th, "tw": run.tiles.tw}
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        stamps = [time.perf_counter()]
        for _, frame in run:
            torch.cuda.current_stream().synchronize()
            stamps.append(time.perf_counter())
        half = a.frames // 2
        rec.update(frames_per_s=a.frames / (stamps[-1] - stamps[0]), second_half_frames_per_s=(a.frames - half) / (stamps[-1] - stamps[half]),
                   max_memory_allocated_GB=torch.cuda.max_memory_allocated() / 1e9, recomputed=len(run.recomputed))
    except Exception as e:                                 # an out-of-memory error is a result; anything else also ends the run
        rec["error"] = f"{type(e).__name__}: {e}"[:600]
        rec["out_of_memory"] = isinstance(e, torch.OutOfMemoryError) or "out of memory" in str(e).lower()
    print("RESULT " + json.dumps(rec), flush=True)
    if "error" in rec and not rec["out_of_memory"]:
        sys.exit(3)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiles_bench.json"))
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--size", choices=sorted(SIZES))
    ap.add_argument("--tiles", default="none")
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"method": f"one fresh process per configuration, a synthetic clip of {a.frames} frames resident on the device, f16 with graphs, "
                     "labels given (every fourth frame sharp); frames/s = frames / wall time of the whole clip, graph captures included; "
                     "second_half_frames_per_s over the last half of the frames; max_memory_allocated of torch's allocator in the loop",
           "runs": [], "stopped": None}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for size, tiles in ORDER:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--size", size, "--tiles", tiles,
               "--frames", str(a.frames)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        rec = json.loads(lines[-1][7:]) if lines else {"size": size, "tiles": tiles}
        rec["exit"] = r.returncode
        if not lines:
            rec["stderr_tail"] = r.stderr[-600:]
        res["runs"].append(rec)
        print(json.dumps(rec), flush=True)
        json.dump(res, open(a.out, "w"), indent=1)         # after every child: a stop leaves what was measured
        if r.returncode != 0:
            res["stopped"] = f"{size} tiles={tiles} ended in {r.returncode}: nothing was started after it"
            break
    json.dump(res, open(a.out, "w"), indent=1)
    print("done" if res["stopped"] is None else res["stopped"])
    if res["stopped"] is not None:
        sys.exit(1)


if __name__ == "__main__":
    main()
