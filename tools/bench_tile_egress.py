"""The tile egress with hard and with feathered seams (ops.tiles_out on a plan with feather 0 and with feather = shave = 20;
csrc/tile_io.hip) on one MI355X -> profiles/tile_egress_bench.json.  Two measurements:

  * egress time: the one launch that stitches a frame, alone, on random tiles, timed with device events: 2160p 2x5, 2160p 2x2 and
    1080p 1x3, at 8 and 12 bits.  Hard and feathered launches alternate in blocks within one process; a block is queued while a
    spin kernel keeps the device busy, so the events see the launches back to back (each with the clear of its flag) and not the rate
    at which the host issues them; the figure per block is the time of the block over its launches, and the host's own time per
    launch is recorded beside it.  The bar: the feathered launch takes at most 1.25 times the hard one (medians over blocks).
    The bytes each launch must move are counted from the plan (4 per float read, every contributing tile once; 1 or 2 per sample
    written).
  * seam step: a 2160p 2x5 clip of six frames (tools/bench_tiles.py's clip, synthetic weights, f16) deblurred with hard and with
    feathered seams; per seam line the mean absolute difference, in 8-bit levels, between the two pixel rows (columns) on either side
    of it, and the same statistic one ramp width (2 * 20 pixels) before and after the seam as the baseline of ordinary picture content.
    No bar: synthetic weights say little about the seams of a trained checkpoint.

    python tools/bench_tile_egress.py [--out <json>] [--timeout SECONDS] [--skip_seams]

Every configuration runs in a fresh child process (this file with --child) under its own `timeout -k 10`; the parent never touches the
GPU, and the run stops at the first child that does not exit 0: nothing more is started on the device after that."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"1080p": (1080, 1920), "2160p": (2160, 3840)}
EGRESS = [("2160p", "2x5"), ("2160p", "2x2"), ("1080p", "1x3")]
DEPTHS = (8, 12)
FEATHER = 20
BAR = 1.25
BLOCKS, LAUNCHES = 20, 50
PLUG_CYCLES = 4_000_000          # a spin kernel in front of every timed block, long enough for the host to queue the block behind it


def launch_bytes(plan, depth: int) -> int:
    """Bytes one egress launch must move: every contributing float once per pixel, every output sample once."""
    import numpy as np
    from speinet_amd import tiles as tiling
    fy, fx = tiling.seam_ramps(plan)

    def sources(n, b, f):                                  # tiles per coordinate of one axis: 2 inside a ramp
        s = np.ones(n, np.int64)
        for k, fs in enumerate(f, start=1):
            s[b[k] - fs:b[k] + fs] = 2
        return s

    reads = int(np.outer(sources(plan.H, plan.yb, fy), sources(plan.W, plan.xb, fx)).sum())
    return reads * 3 * 4 + plan.H * plan.W * 3 * (1 if depth == 8 else 2)


def child_egress(a) -> dict:
    import statistics
    import time
    import torch
    from speinet_amd import ops, tiles as tiling
    h, w = SIZES[a.size]
    torch.cuda.set_device(0)
    hard = tiling.tile_plan(h, w, tiling.parse_tiles(a.tiles))
    soft = tiling.tile_plan(h, w, tiling.parse_tiles(a.tiles), feather=FEATHER)
    thp, twp = hard.padded
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    tiles = torch.rand(hard.n, 3, thp, twp, device="cuda:0", generator=gen) * 1.2 - 0.1
    out = torch.empty(h, w, 3, dtype=torch.uint8 if a.depth == 8 else torch.uint16, device="cuda:0")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    plans = {"hard": hard, "feathered": soft}
    frames = {}
    for name, plan in plans.items():                       # warm-up, and the two results side by side
        for _ in range(10):
            ops.tiles_out(tiles, plan, a.depth, out=out, nonfinite=flag)
        frames[name] = (out if a.depth == 8 else out.view(torch.int16)).clone()      # the same bits: compared for equality only
    torch.cuda.synchronize()
    fy, fx = tiling.seam_ramps(soft)
    ramp = torch.zeros(h, w, dtype=torch.bool, device="cuda:0")
    for k, f in enumerate(fy, start=1):
        ramp[hard.yb[k] - f:hard.yb[k] + f] = True
    for k, f in enumerate(fx, start=1):
        ramp[:, hard.xb[k] - f:hard.xb[k] + f] = True
    same_outside = bool((frames["hard"][~ramp] == frames["feathered"][~ramp]).all())
    us, host_us = {name: [] for name in plans}, {name: [] for name in plans}
    for _ in range(BLOCKS):                                # alternating blocks: drift of the clocks hits both alike
        for name, plan in plans.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(PLUG_CYCLES)                 # the block is queued behind a busy device: device time, not the launch rate
            t0.record()
            h0 = time.perf_counter()
            for _ in range(LAUNCHES):
                ops.tiles_out(tiles, plan, a.depth, out=out, nonfinite=flag)
            host_us[name].append((time.perf_counter() - h0) * 1e6 / LAUNCHES)
            t1.record()
            t1.synchronize()
            us[name].append(t0.elapsed_time(t1) * 1e3 / LAUNCHES)
    rec = {"kind": "egress", "size": a.size, "tiles": a.tiles, "depth": a.depth, "feather": FEATHER, "device": torch.cuda.get_device_name(0),
           "plan": {"rows": hard.rows, "cols": hard.cols, "th": hard.th, "tw": hard.tw}, "blocks": BLOCKS, "launches_per_block": LAUNCHES,
           "ramp_pixels": int(ramp.sum().item()), "pixels": h * w, "equal_outside_ramps": same_outside}
    for name, plan in plans.items():
        med = statistics.median(us[name])
        nbytes = launch_bytes(plan, a.depth)
        rec[name] = {"us_median": med, "us_min": min(us[name]), "us_max": max(us[name]), "bytes": nbytes, "GB_per_s": nbytes / med / 1e3,
                     "host_us_per_launch_median": statistics.median(host_us[name])}
    rec["ratio"] = rec["feathered"]["us_median"] / rec["hard"]["us_median"]
    rec["bytes_ratio"] = rec["feathered"]["bytes"] / rec["hard"]["bytes"]
    rec["bar"] = BAR
    rec["within_bar"] = rec["ratio"] <= BAR
    if not same_outside:
        rec["error"] = "the feathered frame differs from the hard one outside the ramps"
    return rec


def seam_steps(frames, plan, f: int) -> list:
    """Per inner seam: the mean |difference| across the seam line and across the two lines one ramp width (2 f) away, in levels."""
    import torch
    x = frames.to(torch.int16)                             # [T, H, W, 3]

    def step(axis: int, p: int) -> float:                  # between lines p - 1 and p of the axis
        lo, hi = x.select(axis, p - 1), x.select(axis, p)
        return float((hi - lo).abs().float().mean().item())

    out = []
    for axis, name, bounds in ((1, "row", plan.yb), (2, "column", plan.xb)):
        for s in range(1, len(bounds) - 1):
            b = bounds[s]
            out.append({"seam": f"{name} {b}", "step": step(axis, b), "baseline": 0.5 * (step(axis, b - 2 * f) + step(axis, b + 2 * f))})
    return out


def child_seams(a) -> dict:
    import numpy as np
    import torch
    from speinet_amd import tiles as tiling, video
    h, w = SIZES[a.size]
    torch.cuda.set_device(0)
    n = 6
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (h + n, w + 2 * n, 3), dtype=np.uint8)
    base = torch.from_numpy(base).to("cuda:0").float().permute(2, 0, 1)[None]
    base = torch.nn.functional.avg_pool2d(base, 5, stride=1, padding=2)[0].permute(1, 2, 0).round().to(torch.uint8)
    clip = torch.stack([base[i:i + h, 2 * i:2 * i + w] for i in range(n)]).contiguous()
    labels = [1 if i % 4 == 0 else 0 for i in range(n)]
    net = video.load_model("synthetic", "cuda:0", "f16", graph=True)
    out = torch.empty(n, h, w, 3, dtype=torch.uint8, device="cuda:0")
    run = video.deblur_clip(net, clip, labels, tiles=tiling.parse_tiles(a.tiles), feather=a.feather, out=out)
    for _ in run:
        pass
    torch.cuda.synchronize()
    plan = run.tiles
    seams = seam_steps(out, plan, FEATHER)
    return {"kind": "seams", "size": a.size, "tiles": a.tiles, "feather": a.feather, "frames": n, "device": torch.cuda.get_device_name(0),
            "plan": {"rows": plan.rows, "cols": plan.cols, "th": plan.th, "tw": plan.tw}, "recomputed": len(run.recomputed),
            "seams": seams, "mean_step": sum(s["step"] for s in seams) / len(seams),
            "mean_baseline": sum(s["baseline"] for s in seams) / len(seams),
            "input_baseline": sum(s["baseline"] for s in seam_steps(clip, plan, FEATHER)) / len(seams)}


def child(a) -> None:
    try:
        rec = child_egress(a) if a.kind == "egress" else child_seams(a)
    except Exception as e:                                 # recorded, and the run ends with this child
        rec = {"kind": a.kind, "size": a.size, "tiles": a.tiles, "error": f"{type(e).__name__}: {e}"[:600]}
    print("RESULT " + json.dumps(rec), flush=True)
    if "error" in rec:
        sys.exit(3)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_egress_bench.json"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per configuration")
    ap.add_argument("--skip_seams", action="store_true", help="the egress timings only")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kind", choices=("egress", "seams"))
    ap.add_argument("--size", choices=sorted(SIZES))
    ap.add_argument("--tiles", default="2x5")
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--feather", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a)
    jobs = [["--kind", "egress", "--size", size, "--tiles", tiles, "--depth", str(depth)] for size, tiles in EGRESS for depth in DEPTHS]
    if not a.skip_seams:
        jobs += [["--kind", "seams", "--size", "2160p", "--tiles", "2x5", "--feather", str(f)] for f in (0, FEATHER)]
    res = {"method": f"one fresh process per configuration.  egress: the stitch launch alone on random tiles, {BLOCKS} alternating blocks of "
                     f"{LAUNCHES} launches per mode between two device events, each block queued behind a spin kernel so that the device and not "
                     f"the host's launch rate is timed (the host's time per launch is recorded beside it), us per launch = block time / launches, ratio = feathered "
                     f"median / hard median (feather {FEATHER} = shave), bar {BAR}; bytes counted from the plan.  seams: a 2160p 2x5 "
                     "synthetic clip of six frames, synthetic weights, f16 with graphs; mean absolute difference in 8-bit levels across "
                     "each seam line, and across the lines 40 pixels before and after it (baseline)",
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
    egress = [r for r in res["runs"] if r.get("kind") == "egress" and "ratio" in r]
    if egress:
        res["worst_ratio"] = max(r["ratio"] for r in egress)
        res["within_bar"] = all(r["within_bar"] for r in egress)
    json.dump(res, open(a.out, "w"), indent=1)
    print("done" if res["stopped"] is None else res["stopped"])
    if res["stopped"] is not None:
        sys.exit(1)


if __name__ == "__main__":
    main()
