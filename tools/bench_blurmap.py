"""Automatic blur mattes (csrc/blur_map.hip spei_blur_cells_u8 / _u16 and spei_blur_matte; video.deblur_clip(..., matte="auto")) on one
MI355X -> profiles/blurmap_bench.json.  By the protocol of tools/bench_roi.py and tools/bench_matte.py (device events around
alternating blocks of launches, each block queued behind a spin kernel, medians of 20 blocks, of 50 launches for the matte and of 10
for the cells, whose launches take 16 frames each; a fresh process per configuration).  Repeated launches see cache-warm buffers: 16 frames of 720p are 44 MB at 8 bits and 88 MB at 12, of 1080p 100 and
199 MB, against 256 MB of last-level cache, so neither kernel of the comparison reads every byte from HBM in this loop; both see the
same buffers in the same state, and the ratio is what is reported.

  * cells: ops.blur_cells on 16 resident frames at 720p and 1080p, 8 and 12 bits, beside ops.frame_pair_stats / _u16, the existing
    one-pass reduction over the same bytes, in the same process.  Both read each frame once; the cell kernel evaluates the luma 1.86
    times per pixel (a strip of 16x64 with its halo of 25x76 staged groups) and squares four terms.  The bar: 2.0 times.
  * matte: ops.blur_matte (three verdict maps, grow 1) at 720p and 1080p: one byte written per pixel.  Recorded, no bar.
  * clip: a synthetic 720p clip of 16 frames resident on the device, synthetic weights, f16 with graphs, second pass.  `matte=` a device
    [T,H,W] tensor of 255 against matte="auto" with thr=257, flat=0 (every cell lit: the same blend), no labels and cuts="auto", so
    the analysis pass counts in both; three alternating pairs; the bar: the median under "auto" may exceed the median under the given
    matte by at most the spread (max - min) of the given-matte runs, and by no less than 5 % of their median.
  * half: a clip whose frames are sharp in their right half under matte="auto", with and without roi="matte": frames/s and peak
    allocator memory, one run each, no bar.

    python tools/bench_blurmap.py [--out <json>] [--timeout SECONDS] [--kind cells|matte|clip|half]

With --kind only the configurations of that kind run, and their records REPLACE those of that kind in an existing output file: the
other records stay, and the file says so under "partial_runs".

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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_roi import BLOCKS, LAUNCHES, SIZES, summary, timed_blocks      # noqa: E402

DEPTHS = (8, 12)
BAR = 2.0
CLIP_FRAMES = 16
REPEATS = 3


def _scene(n, h, w, device):
    """n frames of h x w on the device: noise through a 5x5 mean, panned by (1, 2) pixels per frame."""
    import numpy as np
    import torch
    base = np.random.default_rng(0).integers(0, 256, (h + n, w + 2 * n, 3), dtype=np.uint8)
    base = torch.from_numpy(base).to(device).float().permute(2, 0, 1)[None]
    base = torch.nn.functional.avg_pool2d(base, 5, stride=1, padding=2)[0].permute(1, 2, 0).round().to(torch.uint8)
    return torch.stack([base[i:i + h, 2 * i:2 * i + w] for i in range(n)]).contiguous()


def child_cells(a) -> dict:
    import numpy as np
    import torch
    import blurmap_ref as BR
    from speinet_amd import ops
    h, w = SIZES[a.size]
    torch.cuda.set_device(0)
    n = CLIP_FRAMES
    D = (1 << a.depth) - 1
    frames_h = np.random.default_rng(0).integers(0, D + 1, (n, h, w, 3)).astype(np.uint8 if a.depth == 8 else np.uint16)
    frames = torch.from_numpy(frames_h).to("cuda:0")
    deep = None if a.depth == 8 else a.depth

    def cells():
        ops.blur_cells(frames, deep)

    def stats():
        ops.frame_pair_stats(frames) if deep is None else ops.frame_pair_stats_u16(frames, deep)

    for fn in (cells, stats):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    got, sums = ops.blur_cells(frames[:1], deep, sums=True)
    ref, ref_sums = BR.cells_of(frames_h[:1], a.depth)
    equal = bool(np.array_equal(got.cpu().numpy(), ref) and np.array_equal(sums.cpu().numpy(), ref_sums))
    launches = max(5, LAUNCHES // 5)                       # 16 frames per launch
    t = timed_blocks({"cells": cells, "pair_stats": stats}, launches)
    nbytes = frames.numel() * frames.element_size()
    rec = {"kind": "cells", "size": a.size, "depth": a.depth, "frames": n, "device": torch.cuda.get_device_name(0), "blocks": BLOCKS,
           "launches_per_block": launches, "bytes_read": nbytes, "cells": summary(*t["cells"], nbytes),
           "pair_stats": summary(*t["pair_stats"], nbytes), "equals_definition": equal}
    rec["ratio"] = rec["cells"]["us_median"] / rec["pair_stats"]["us_median"]
    rec["bar"] = BAR
    rec["within_bar"] = rec["ratio"] <= BAR
    if not equal:
        rec["error"] = "the cells differ from tests/blurmap_ref.py"
    return rec


def child_matte(a) -> dict:
    import numpy as np
    import torch
    import blurmap_ref as BR
    from speinet_amd import ops
    h, w = SIZES[a.size]
    torch.cuda.set_device(0)
    ch, cw = ops.blur_cell_shape(h, w)
    maps_h = np.where(np.random.default_rng(0).random((3, ch, cw)) < 0.2, 255, 0).astype(np.uint8)
    maps = torch.from_numpy(maps_h).to("cuda:0")
    out = torch.empty(h, w, dtype=torch.uint8, device="cuda:0")

    def matte():
        ops.blur_matte(maps, h, w, 1, out=out)

    for _ in range(10):
        matte()
    torch.cuda.synchronize()
    equal = bool(np.array_equal(out.cpu().numpy(), BR.matte_of(maps_h, h, w, 1)))
    t = timed_blocks({"matte": matte}, LAUNCHES)
    rec = {"kind": "matte", "size": a.size, "maps": 3, "grow": 1, "device": torch.cuda.get_device_name(0), "blocks": BLOCKS,
           "launches_per_block": LAUNCHES, "matte": summary(*t["matte"], h * w), "equals_definition": equal}
    if not equal:
        rec["error"] = "the matte differs from tests/blurmap_ref.py"
    return rec


def _one(video, torch, net, clip, out, **kw) -> dict:
    import time
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    run = video.deblur_clip(net, clip, out=out, cuts="auto", **kw)
    for _ in run:
        pass
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rec = {"seconds": dt, "fps": len(clip) / dt, "peak_allocated_MiB": torch.cuda.max_memory_allocated() / 2 ** 20,
           "unmatted": len(run.unmatted), "recomputed": len(run.recomputed), "roi": run.roi}
    if kw.get("matte") == "auto":
        rec["lit_cells"] = float((run.matte.cells != 0).mean())
    return rec


def child_clip(a) -> dict:
    import torch
    from speinet_amd import video
    h, w = SIZES["720p"]
    torch.cuda.set_device(0)
    n = CLIP_FRAMES
    clip = _scene(n, h, w, "cuda:0")
    net = video.load_model("synthetic", "cuda:0", "f16", graph=True)
    out = torch.empty(n, h, w, 3, dtype=torch.uint8, device="cuda:0")
    kinds = {"given": dict(matte=torch.full((n, h, w), 255, dtype=torch.uint8, device="cuda:0")),
             "auto": dict(matte="auto", matte_params=dict(thr=257, flat=0))}
    for kw in kinds.values():                              # the first pass captures the graphs
        _one(video, torch, net, clip, out, **kw)
    rec = {"kind": "clip", "frames": n, "H": h, "W": w, "precision": "f16", "graphs": True, "device": torch.cuda.get_device_name(0)}
    pair = {name: [] for name in kinds}
    for _ in range(REPEATS):                               # alternating: drift hits both alike
        for name, kw in kinds.items():
            pair[name].append(_one(video, torch, net, clip, out, **kw))
    rec["runs"] = pair
    g, k = ([r["seconds"] for r in pair[name]] for name in ("given", "auto"))
    spread = max(g) - min(g)
    allowance = max(spread, 0.05 * statistics.median(g))
    rec.update(given_median_s=statistics.median(g), auto_median_s=statistics.median(k), given_spread_s=spread, allowance_s=allowance,
               auto_minus_given_s=statistics.median(k) - statistics.median(g),
               within_bar=statistics.median(k) <= statistics.median(g) + allowance,
               all_lit=all(r["unmatted"] == 0 for r in pair["auto"]))
    return rec


def child_half(a) -> dict:
    import torch
    from speinet_amd import video
    h, w = SIZES["720p"]
    torch.cuda.set_device(0)
    n = CLIP_FRAMES
    # blocks of 8x8 pixels of random colour: step edges (white noise would not do: through a box its adjacent differences stay
    # uncorrelated, and the measure reads it as sharp, the grain blind spot); the left half through a 9-tap horizontal box
    blocks = torch.randint(0, 256, (n, h // 8, w // 8, 3), dtype=torch.uint8, device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(0))
    clip = blocks.repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()
    left = clip[:, :, :w // 2].float().permute(0, 3, 1, 2)
    left = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(left, (4, 4, 0, 0), mode="replicate"), (1, 9), stride=1)
    clip[:, :, :w // 2] = left.permute(0, 2, 3, 1).round().to(torch.uint8)
    net = video.load_model("synthetic", "cuda:0", "f16", graph=True)
    out = torch.empty(n, h, w, 3, dtype=torch.uint8, device="cuda:0")
    kinds = {"auto": dict(matte="auto"), "auto_roi_matte": dict(matte="auto", roi="matte")}
    rec = {"kind": "half", "frames": n, "H": h, "W": w, "precision": "f16", "graphs": True, "device": torch.cuda.get_device_name(0), "runs": {}}
    for name, kw in kinds.items():
        _one(video, torch, net, clip, out, **kw)           # the first pass captures the graphs
        rec["runs"][name] = _one(video, torch, net, clip, out, **kw)
    return rec


def child(a) -> None:
    try:
        rec = {"cells": child_cells, "matte": child_matte, "clip": child_clip, "half": child_half}[a.kind](a)
    except Exception as e:                                 # recorded, and the run ends with this child
        rec = {"kind": a.kind, "error": f"{type(e).__name__}: {e}"[:600]}
    print("RESULT " + json.dumps(rec), flush=True)
    if "error" in rec:
        sys.exit(3)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blurmap_bench.json"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per configuration")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kind", choices=("cells", "matte", "clip", "half"))
    ap.add_argument("--size", choices=sorted(SIZES), default="720p")
    ap.add_argument("--depth", type=int, default=8)
    a = ap.parse_args()
    if a.child:
        return child(a)
    jobs = [["--kind", "cells", "--size", size, "--depth", str(d)] for size in SIZES for d in DEPTHS]
    jobs += [["--kind", "matte", "--size", size] for size in SIZES]
    jobs += [["--kind", "clip"], ["--kind", "half"]]
    if a.kind is not None:
        jobs = [j for j in jobs if j[1] == a.kind]
    res = {"method": f"one fresh process per configuration.  cells and matte: {BLOCKS} alternating blocks of launches per mode between two "
                     "device events, each block queued behind a spin kernel so that the device and not the host's launch rate is timed, "
                     "us per launch = block time / launches, medians over blocks; repeated launches see cache-warm buffers (16 frames "
                     f"are 44 to 199 MB against 256 MB of last-level cache), alike for both kernels of a pair.  cells: ops.blur_cells on "
                     f"{CLIP_FRAMES} resident frames against ops.frame_pair_stats(_u16) on the same frames, bar {BAR}.  matte: "
                     "ops.blur_matte on three verdict maps, grow 1, no bar.  clip: 16 synthetic 720p frames resident on the device, no "
                     "labels and cuts=\"auto\" (the analysis pass counts in both), synthetic weights, f16 with graphs; every variant runs "
                     f"once untimed, then {REPEATS} alternating pairs of a given device matte of 255 and matte=\"auto\" with thr=257, "
                     "flat=0; bar: median under auto <= median under the given matte + max(spread of the given-matte runs, 5 % of their "
                     "median).  half: frames sharp in their right half under matte=\"auto\" with and without roi=\"matte\", second pass, "
                     "one run each, no bar.  Measured once",
           "runs": [], "stopped": None}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.kind is not None and os.path.exists(a.out):       # a run of one kind: the records of the other kinds stay
        old = json.load(open(a.out))
        res["runs"] = [r for r in old.get("runs", []) if r.get("kind") != a.kind]
        res["partial_runs"] = old.get("partial_runs", []) + [f"the records of kind {a.kind} come from a later run with --kind {a.kind}"]
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
    runs = [r for r in res["runs"] if r.get("kind") == "cells" and "ratio" in r]
    if runs:
        res["cells_worst_ratio"] = max(r["ratio"] for r in runs)
        res["cells_within_bar"] = all(r["within_bar"] for r in runs)
    json.dump(res, open(a.out, "w"), indent=1)
    print("done" if res["stopped"] is None else res["stopped"])
    if res["stopped"] is not None:
        sys.exit(1)


if __name__ == "__main__":
    main()
