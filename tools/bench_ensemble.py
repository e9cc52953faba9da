"""The geometric self-ensemble's two kernels and its cost in the clip API (ops.planes_d4, ops.d4_mean: csrc/ensemble_io.hip;
video.deblur_clip(..., ensemble=)) on one MI355X -> profiles/ensemble_bench.json.  Two measurements, by tools/bench_tile_egress.py's
protocol:

  * kernels: 15 fp32 planes of 720x1280 (the window input of a 720p clip).  The yardstick is a device-to-device `copy_` of the same
    planes in the same process: it moves the same bytes and owes nothing to the code under test.  `planes_d4` for ops 1, 3, 4 and 7,
    bar: at most 1.5 times the copy.  `d4_mean` of K = 8 members of those 15 planes (four of them transposed), bar: at most 1.5 times
    (K + 1) / 2 copies, since it reads K plane sets and writes one where a copy reads one and writes one; the three-plane mean of the
    clip loop is recorded beside it against a three-plane copy, without a bar.  All modes alternate in blocks within one process; a
    block is queued while a spin kernel keeps the device busy, so the events see the launches back to back and not the rate at which
    the host issues them; the figure per block is the time of the block over its launches; medians of 20 blocks.
  * clip: an 8-frame synthetic 720p clip, synthetic weights, f16 with graphs, one fresh process per K in 1, 2, 4, 8: frames/s over the
    last four frames and over the whole clip (captures included), the allocator's peak, the captured graphs at the end and whether
    they were ever trimmed, and (t_8 - t_4) / t_4 over the last four frames: the four 720-wide, 1280-tall members against the four
    upright ones.  Eight frames are few, and graphs are still being captured among the last four, so the same clip runs a second time
    in the same process with every graph in place: its seconds per frame, and the same ratio from them, are recorded beside the
    first pass's.  No bar.

    python tools/bench_ensemble.py [--out <json>] [--timeout SECONDS] [--skip_clips]

Every configuration runs in a fresh child process (this file with --child) under its own `timeout -k 10`; the parent never touches the
GPU, and the run stops at the first child that does not exit 0: nothing more is started on the device after that."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, PLANES = 720, 1280, 15
D4_OPS = (1, 3, 4, 7)
K = 8
BAR = 1.5
BLOCKS, LAUNCHES = 20, 20
PLUG_CYCLES = 4_000_000          # a spin kernel in front of every timed block, long enough for the host to queue the block behind it
CLIP_FRAMES = 8


def child_kernels(a) -> dict:
    import statistics
    import time
    import torch
    from speinet_amd import ensemble, ops
    torch.cuda.set_device(0)
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(PLANES, H, W, device=dev, generator=gen)
    flat, upright = torch.empty_like(x), torch.empty_like(x)
    turned = torch.empty(PLANES, W, H, device=dev)
    members = {c: [ops.planes_d4(torch.rand(c, H, W, device=dev, generator=gen), g) for g in range(K)] for c in (PLANES, 3)}
    mean_out = {c: torch.empty(c, H, W, device=dev) for c in (PLANES, 3)}
    x3, flat3 = x[:3], torch.empty(3, H, W, device=dev)
    table = list(range(K))
    modes = {"copy": lambda: flat.copy_(x), "copy_3_planes": lambda: flat3.copy_(x3)}
    for g in D4_OPS:
        modes[f"planes_d4_op{g}"] = (lambda g=g: ops.planes_d4(x, g, out=turned if g & 4 else upright))
    modes["d4_mean_k8"] = lambda: ops.d4_mean(members[PLANES], table, out=mean_out[PLANES])
    modes["d4_mean_k8_3_planes"] = lambda: ops.d4_mean(members[3], table, out=mean_out[3])
    for fn in modes.values():                              # warm-up
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    # the results are what the definition says (on the device, with torch's own flips)
    correct = all(torch.equal(ops.planes_d4(x, g), ensemble.apply(x, g).contiguous()) for g in D4_OPS)
    us, host_us = {name: [] for name in modes}, {name: [] for name in modes}
    for _ in range(BLOCKS):                                # alternating blocks: drift of the clocks hits all alike
        for name, fn in modes.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(PLUG_CYCLES)                 # the block is queued behind a busy device: device time, not the launch rate
            t0.record()
            h0 = time.perf_counter()
            for _ in range(LAUNCHES):
                fn()
            host_us[name].append((time.perf_counter() - h0) * 1e6 / LAUNCHES)
            t1.record()
            t1.synchronize()
            us[name].append(t0.elapsed_time(t1) * 1e3 / LAUNCHES)
    plane_bytes = H * W * 4
    moved = {"copy": 2 * PLANES, "copy_3_planes": 2 * 3, "d4_mean_k8": (K + 1) * PLANES, "d4_mean_k8_3_planes": (K + 1) * 3}
    rec = {"kind": "kernels", "device": torch.cuda.get_device_name(0), "planes": PLANES, "H": H, "W": W, "blocks": BLOCKS,
           "launches_per_block": LAUNCHES, "planes_d4_equals_torch": correct, "bar": BAR}
    for name in modes:
        med = statistics.median(us[name])
        nbytes = moved.get(name, 2 * PLANES) * plane_bytes
        rec[name] = {"us_median": med, "us_min": min(us[name]), "us_max": max(us[name]), "bytes": nbytes, "GB_per_s": nbytes / med / 1e3,
                     "host_us_per_launch_median": statistics.median(host_us[name])}
    copy = rec["copy"]["us_median"]
    for g in D4_OPS:
        r = rec[f"planes_d4_op{g}"]
        r["ratio_to_copy"] = r["us_median"] / copy
        r["within_bar"] = r["ratio_to_copy"] <= BAR
    r = rec["d4_mean_k8"]
    r["ratio_to_copies"] = r["us_median"] / (copy * (K + 1) / 2)          # against (K + 1) / 2 copies
    r["within_bar"] = r["ratio_to_copies"] <= BAR
    r = rec["d4_mean_k8_3_planes"]
    r["ratio_to_copies"] = r["us_median"] / (rec["copy_3_planes"]["us_median"] * (K + 1) / 2)
    rec["within_bar"] = all(rec[n]["within_bar"] for n in [f"planes_d4_op{g}" for g in D4_OPS] + ["d4_mean_k8"])
    if not correct:
        rec["error"] = "planes_d4 differs from torch's flips and transposition"
    return rec


def child_clip(a) -> dict:
    import time
    import numpy as np
    import torch
    from speinet_amd import video
    torch.cuda.set_device(0)
    n = CLIP_FRAMES
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (H + n, W + 2 * n, 3), dtype=np.uint8)
    base = torch.from_numpy(base).to("cuda:0").float().permute(2, 0, 1)[None]
    base = torch.nn.functional.avg_pool2d(base, 5, stride=1, padding=2)[0].permute(1, 2, 0).round().to(torch.uint8)
    clip = torch.stack([base[i:i + H, 2 * i:2 * i + W] for i in range(n)]).contiguous()
    labels = [1 if i % 4 == 0 else 0 for i in range(n)]
    net = video.load_model("synthetic", "cuda:0", "f16", graph=True)
    out = torch.empty(n, H, W, 3, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    passes = []
    for _ in range(2):                                     # the second pass finds every graph captured: the steady rate of a long clip
        run = video.deblur_clip(net, clip, labels, out=out, ensemble=a.ensemble)
        stamps, graphs = [], []
        t0 = time.perf_counter()
        for _ in run:
            torch.cuda.current_stream().synchronize()      # the frame is complete: its time
            stamps.append(time.perf_counter() - t0)
            graphs.append(len(net._graphs))
        torch.cuda.synchronize()
        passes.append((stamps, graphs))
    (stamps, graphs), (again, graphs_again) = passes
    last4 = (stamps[-1] - stamps[-5]) / 4
    return {"kind": "clip", "ensemble": a.ensemble, "frames": n, "H": H, "W": W, "precision": "f16", "graphs": True,
            "device": torch.cuda.get_device_name(0), "seconds_at_frame": stamps, "fps_last4": 1.0 / last4, "seconds_per_frame_last4": last4,
            "fps_whole_clip": n / stamps[-1], "second_pass_seconds_at_frame": again, "second_pass_seconds_per_frame": again[-1] / n,
            "second_pass_fps": n / again[-1], "peak_allocated_MiB": torch.cuda.max_memory_allocated() / 2 ** 20,
            "graphs_at_frame": graphs, "graphs_at_end": graphs[-1], "graph_limit": net.GRAPH_LIMIT,
            "trimmed": any(b < a_ for a_, b in zip(graphs + graphs_again, (graphs + graphs_again)[1:])), "recomputed": len(run.recomputed),
            "no_reference_windows": sum(p["zero_pre"] for p in run.plan)}


def child(a) -> None:
    try:
        rec = child_kernels(a) if a.kind == "kernels" else child_clip(a)
    except Exception as e:                                 # recorded, and the run ends with this child
        rec = {"kind": a.kind, "ensemble": a.ensemble, "error": f"{type(e).__name__}: {e}"[:600]}
    print("RESULT " + json.dumps(rec), flush=True)
    if "error" in rec:
        sys.exit(3)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_bench.json"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per configuration")
    ap.add_argument("--skip_clips", action="store_true", help="the kernel timings only")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kind", choices=("kernels", "clip"))
    ap.add_argument("--ensemble", type=int, default=1)
    a = ap.parse_args()
    if a.child:
        return child(a)
    jobs = [["--kind", "kernels"]]
    if not a.skip_clips:
        jobs += [["--kind", "clip", "--ensemble", str(k)] for k in (1, 2, 4, 8)]
    res = {"method": f"one fresh process per configuration.  kernels: {PLANES} fp32 planes of {H}x{W}; {BLOCKS} alternating blocks of {LAUNCHES} "
                     "launches per mode between two device events, each block queued behind a spin kernel so that the device and not the "
                     "host's launch rate is timed (the host's time per launch is recorded beside it), us per launch = block time / "
                     f"launches, medians over blocks; yardstick: a device-to-device copy_ of the same planes; bars: planes_d4 <= {BAR} x copy, "
                     f"d4_mean (K = {K}) <= {BAR} x (K + 1) / 2 copies.  clip: {CLIP_FRAMES} synthetic {H}x{W} frames, synthetic weights, f16 with "
                     "graphs; wall-clock time at every frame handed out, after a synchronisation of the stream, for the clip and for a second pass "
                     "over it in the same process (all graphs captured); no bar",
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
    kernels = [r for r in res["runs"] if r.get("kind") == "kernels" and "within_bar" in r]
    if kernels:
        res["within_bar"] = kernels[0]["within_bar"]
    clips = {r["ensemble"]: r for r in res["runs"] if r.get("kind") == "clip" and "seconds_per_frame_last4" in r}
    if 4 in clips and 8 in clips:
        t4, t8 = clips[4]["seconds_per_frame_last4"], clips[8]["seconds_per_frame_last4"]
        s4, s8 = clips[4]["second_pass_seconds_per_frame"], clips[8]["second_pass_seconds_per_frame"]
        res["transposed_members_cost"] = {"t4_seconds_per_frame": t4, "t8_seconds_per_frame": t8, "(t8-t4)/t4": (t8 - t4) / t4,
                                          "second_pass": {"t4_seconds_per_frame": s4, "t8_seconds_per_frame": s8, "(t8-t4)/t4": (s8 - s4) / s4}}
    json.dump(res, open(a.out, "w"), indent=1)
    print("done" if res["stopped"] is None else res["stopped"])
    if res["stopped"] is not None:
        sys.exit(1)


if __name__ == "__main__":
    main()
