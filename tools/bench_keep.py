"""Sharp frames kept in the clip API (csrc/frame_io.hip spei_frame_requant; video.deblur_clip(..., sharp="keep")) on one MI355X
-> profiles/keep_bench.json.  Two measurements, by the protocol of tools/bench_roi.py (device events around alternating blocks of
launches, each block queued behind a spin kernel, medians of 20 blocks of 50 launches, a fresh process per configuration):

  * launch: ops.frame_requant at 720p and 1080p for 8 -> 8, 8 -> 10 and 12 -> 8 bits, beside a device-to-device copy of the larger of
    the launch's input and output bytes in the same process.  The bar: 1.5 times that copy.
  * clip: a synthetic 720p clip of 16 frames resident on the device, synthetic weights, f16 with graphs; frames/s over a second pass
    with every graph captured, and the peak of torch's allocator beside each run, with labels all blurry, half sharp (alternating
    pairs) and all sharp, under "deblur" and under "keep".  The all-blurry pair runs three times, alternating; the bar: the median
    "keep" time may exceed the median "deblur" time by at most the spread (max - min) of the three "deblur" repeats, and by no less
    than 5 % of it.  The half-sharp and all-sharp speed-ups are recorded as found and carry no bar.

    python tools/bench_keep.py [--out <json>] [--timeout SECONDS] [--kind launch|clip]

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

PAIRS = ((8, 8), (8, 10), (12, 8))
BAR = 1.5
CLIP_FRAMES = 16
REPEATS = 3
LABELS = {"all_blurry": [0] * CLIP_FRAMES, "half_sharp": [(i // 2) % 2 for i in range(CLIP_FRAMES)], "all_sharp": [1] * CLIP_FRAMES}


def child_launch(a) -> dict:
    import numpy as np
    import torch
    from speinet_amd import ops
    h, w = SIZES[a.size]
    torch.cuda.set_device(0)
    Din = (1 << a.in_depth) - 1
    np_in = np.uint8 if a.in_depth == 8 else np.uint16
    host = np.random.default_rng(0).integers(0, Din + 1, (h, w, 3)).astype(np_in)
    frame = torch.from_numpy(host).to("cuda:0")
    out = torch.empty(h, w, 3, dtype=torch.uint8 if a.out_depth == 8 else torch.uint16, device="cuda:0")
    in_bytes, out_bytes = frame.numel() * frame.element_size(), out.numel() * out.element_size()
    big_src = torch.zeros(max(in_bytes, out_bytes), dtype=torch.uint8, device="cuda:0")
    big_dst = torch.empty_like(big_src)
    deep = None if a.in_depth == 8 else a.in_depth

    def requant():
        ops.frame_requant(frame, a.out_depth, deep, out=out)

    def copy():                                            # the yardstick: the larger of the two sides, device to device
        big_dst.copy_(big_src)

    for fn in (requant, copy):
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    Dout = (1 << a.out_depth) - 1
    want = (host.astype(np.int64) * 2 * Dout + Din) // (2 * Din)
    equal = bool(np.array_equal(out.cpu().numpy().astype(np.int64), want))
    t = timed_blocks({"requant": requant, "copy": copy}, LAUNCHES)
    rec = {"kind": "launch", "size": a.size, "in_depth": a.in_depth, "out_depth": a.out_depth, "device": torch.cuda.get_device_name(0),
           "blocks": BLOCKS, "launches_per_block": LAUNCHES, "requant": summary(*t["requant"], in_bytes + out_bytes),
           "copy": summary(*t["copy"], 2 * max(in_bytes, out_bytes)), "equals_definition": equal}
    rec["ratio"] = rec["requant"]["us_median"] / rec["copy"]["us_median"]
    rec["bar"] = BAR
    rec["within_bar"] = rec["ratio"] <= BAR
    if not equal:
        rec["error"] = "the frame differs from (v * 2 * D_out + D_in) // (2 * D_in)"
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

    def one(labels, sharp) -> dict:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        run = video.deblur_clip(net, clip, labels, out=out, sharp=sharp)
        for _ in run:
            pass
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return {"seconds": dt, "fps": n / dt, "peak_allocated_MiB": torch.cuda.max_memory_allocated() / 2 ** 20, "kept": len(run.kept),
                "recomputed": len(run.recomputed)}

    for labels in LABELS.values():                         # the first pass of every plan captures its graphs
        for sharp in video.SHARP:
            one(labels, sharp)
    rec = {"kind": "clip", "frames": n, "H": h, "W": w, "precision": "f16", "graphs": True, "device": torch.cuda.get_device_name(0), "runs": {}}
    blurry = {sharp: [] for sharp in video.SHARP}
    for _ in range(REPEATS):                               # alternating: drift hits both alike
        for sharp in video.SHARP:
            blurry[sharp].append(one(LABELS["all_blurry"], sharp))
    rec["runs"]["all_blurry"] = blurry
    for name in ("half_sharp", "all_sharp"):
        rec["runs"][name] = {sharp: [one(LABELS[name], sharp)] for sharp in video.SHARP}
        d, k = (rec["runs"][name][sharp][0]["seconds"] for sharp in video.SHARP)
        rec[f"{name}_speedup"] = d / k
    d, k = ([r["seconds"] for r in blurry[sharp]] for sharp in video.SHARP)
    spread = max(d) - min(d)
    allowance = max(spread, 0.05 * statistics.median(d))
    rec.update(all_blurry_deblur_median_s=statistics.median(d), all_blurry_keep_median_s=statistics.median(k), deblur_spread_s=spread,
               allowance_s=allowance, keep_minus_deblur_s=statistics.median(k) - statistics.median(d),
               within_bar=statistics.median(k) <= statistics.median(d) + allowance)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keep_bench.json"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per configuration")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kind", choices=("launch", "clip"))
    ap.add_argument("--size", choices=sorted(SIZES), default="720p")
    ap.add_argument("--in_depth", type=int, default=8)
    ap.add_argument("--out_depth", type=int, default=8)
    a = ap.parse_args()
    if a.child:
        return child(a)
    jobs = [["--kind", "launch", "--size", size, "--in_depth", str(i), "--out_depth", str(o)] for size in SIZES for i, o in PAIRS]
    jobs += [["--kind", "clip"]]
    if a.kind is not None:
        jobs = [j for j in jobs if j[1] == a.kind]
    res = {"method": f"one fresh process per configuration.  launch: {BLOCKS} alternating blocks of {LAUNCHES} launches per mode between two "
                     "device events, each block queued behind a spin kernel so that the device and not the host's launch rate is timed "
                     "(the host's time per launch is recorded beside it), us per launch = block time / launches, medians over blocks; "
                     "ops.frame_requant into a buffer allocated once against a device-to-device copy of the larger of its input and "
                     f"output bytes, bar {BAR}.  clip: {CLIP_FRAMES} synthetic 720p frames resident on the device, synthetic weights, f16 "
                     "with graphs; every plan runs once untimed (its graphs are captured), then timed: wall time of a whole pass, "
                     f"frames/s = frames / time; the all-blurry pair {REPEATS} times, alternating; bar: median keep <= median deblur + "
                     "max(spread of the deblur repeats, 5 % of their median).  Measured once",
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
