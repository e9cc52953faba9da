"""The 4:2:2 and mono conversions of the clip API (csrc/yuv_io.hip: spei_planar_to_rgb_u8 / _u16, spei_rgb_u8_to_planar /
spei_rgb_u16_to_planar) on one MI355X -> profiles/yuv422_bench.json, by the protocol of tools/bench_roi.py: device events around
alternating blocks of launches, each block queued behind a spin kernel, medians of 20 blocks, a fresh process per configuration.

A configuration is a frame size (720p, 1080p), a depth (8, 10) and a direction ("in": one planar frame -> packed RGB; "out": one
packed RGB frame -> planar).  Each times four launches on the same frame in the same process: SPEI_YUV_422 and SPEI_YUV_MONO next to
the existing SPEI_YUV_420_LEFT and SPEI_YUV_444 (BT.709, limited range).  The planar frames of the way in are made from one random
RGB frame by the way out, so every layout carries the same picture.

The bar, for 4:2:2 only: at most 1.25 times the slower of the LEFT and the 4:4:4 launch.  Mono has no bar; its times are recorded.

    python tools/bench_yuv422.py [--out <json>] [--timeout SECONDS]

Every configuration runs in a fresh child process (this file with --child) under its own `timeout -k 10`; the parent never touches the
GPU, and the run stops at the first child that does not exit 0: nothing more is started on the device after that."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_roi import BLOCKS, LAUNCHES, SIZES, summary, timed_blocks        # noqa: E402  (the shared protocol)

DEPTHS = (8, 10)
DIRECTIONS = ("in", "out")
BAR = 1.25
LAYOUT_NAMES = {"422": 3, "mono": 4, "420_left": 1, "444": 2}                    # y4m.P422, MONO, LEFT, P444
MATRIX, RANGE = 1, 1                                                             # y4m.BT709, y4m.LIMITED


def child(a) -> None:
    try:
        rec = measure(a)
    except Exception as e:                                 # recorded, and the run ends with this child
        rec = {"size": a.size, "depth": a.depth, "direction": a.direction, "error": f"{type(e).__name__}: {e}"[:600]}
    print("RESULT " + json.dumps(rec), flush=True)
    if "error" in rec:
        sys.exit(3)


def measure(a) -> dict:
    import numpy as np
    import torch
    from speinet_amd import ops
    h, w = SIZES[a.size]
    torch.cuda.set_device(0)
    D = (1 << a.depth) - 1
    sample = 1 if a.depth == 8 else 2
    rgb = torch.from_numpy(np.random.default_rng(0).integers(0, D + 1, (h, w, 3)).astype(np.uint8 if a.depth == 8 else np.uint16)).to("cuda:0")

    def to_yuv(layout, out=None):
        if a.depth == 8:
            return ops.rgb_u8_to_yuv(rgb, layout, MATRIX, RANGE, out=out)
        return ops.rgb_u16_to_yuv(rgb, layout, MATRIX, RANGE, a.depth, out=out)

    def to_rgb(planar, layout, out=None):
        if a.depth == 8:
            return ops.yuv_to_rgb_u8(planar, h, w, layout, MATRIX, RANGE, out=out)
        return ops.yuv_to_rgb_u16(planar, h, w, layout, MATRIX, RANGE, a.depth, out=out)

    planar = {name: to_yuv(lay) for name, lay in LAYOUT_NAMES.items()}
    modes, nbytes = {}, {}
    for name, lay in LAYOUT_NAMES.items():
        if a.direction == "out":
            modes[name] = (lambda lay=lay, dst=torch.empty_like(planar[name]): to_yuv(lay, out=dst))
        else:
            modes[name] = (lambda lay=lay, src=planar[name], dst=torch.empty(1, h, w, 3, dtype=rgb.dtype, device="cuda:0"): to_rgb(src, lay, out=dst))
        nbytes[name] = (planar[name].numel() + h * w * 3) * sample
    for fn in modes.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    t = timed_blocks(modes, LAUNCHES)
    rec = {"size": a.size, "H": h, "W": w, "depth": a.depth, "direction": a.direction, "device": torch.cuda.get_device_name(0),
           "blocks": BLOCKS, "launches_per_block": LAUNCHES}
    for name in modes:
        rec[name] = summary(*t[name], nbytes[name])
    slower = max(rec["420_left"]["us_median"], rec["444"]["us_median"])
    rec["ratio_422"] = rec["422"]["us_median"] / slower
    rec["ratio_mono"] = rec["mono"]["us_median"] / slower
    rec["bar"] = BAR
    rec["within_bar"] = rec["ratio_422"] <= BAR
    return rec


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv422_bench.json"))
    ap.add_argument("--timeout", type=int, default=120, help="seconds per configuration")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--size", choices=sorted(SIZES), default="720p")
    ap.add_argument("--depth", type=int, choices=DEPTHS, default=8)
    ap.add_argument("--direction", choices=DIRECTIONS, default="in")
    a = ap.parse_args()
    if a.child:
        return child(a)
    jobs = [["--size", size, "--depth", str(depth), "--direction", d] for size in SIZES for depth in DEPTHS for d in DIRECTIONS]
    res = {"method": f"one fresh process per configuration (size, depth, direction).  {BLOCKS} alternating blocks of {LAUNCHES} launches per "
                     "layout between two device events, each block queued behind a spin kernel so that the device and not the host's "
                     "launch rate is timed (the host's time per launch is recorded beside it), us per launch = block time / launches, "
                     "medians over blocks.  in: one planar frame -> packed RGB; out: one packed RGB frame -> planar; BT.709 limited; "
                     "SPEI_YUV_422 and SPEI_YUV_MONO beside SPEI_YUV_420_LEFT and SPEI_YUV_444 on the same picture.  ratio_422 = the "
                     f"4:2:2 median over the slower of the LEFT and 4:4:4 medians, bar {BAR}; mono has no bar",
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
    runs = [r for r in res["runs"] if "ratio_422" in r]
    if runs:
        res["worst_ratio_422"] = max(r["ratio_422"] for r in runs)
        res["within_bar"] = all(r["within_bar"] for r in runs)
    json.dump(res, open(a.out, "w"), indent=1)
    print("done" if res["stopped"] is None else res["stopped"])
    if res["stopped"] is not None:
        sys.exit(1)


if __name__ == "__main__":
    main()
