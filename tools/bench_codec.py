"""Codec artefacts in blur synthesis (csrc/codec.hip; speinet_amd/codec.py) on one MI355X -> profiles/codec_bench.json.  By the protocol
of tools/bench_roi.py (device events around alternating blocks of launches, each block queued behind a spin kernel, medians of 20
blocks, a fresh process per configuration), on the C entry points into buffers allocated once:

  * frames: spei_codec_u8 in place on four 720p frames (with their gray planes) at quality 10, 50 and 90, beside
    spei_window_mean_light_u8 making four 720p output frames (runs of 1, 2, 7 and 15 frames, light srgb) — the yardstick of
    tools/bench_shake.py — and beside a device-to-device copy of the four frames' bytes.  No bar: the ratios are recorded.
  * train: swint training steps (batch 20, 200 x 200, synthetic weights) fed by data.SharpTrainLoader with prefetch, as `fit --dir_sharp
    --blur_light srgb` runs them, without and with `--blur_codec 30..90`, ALTERNATING, three pairs in one session: crops/s over the steps
    after the first two.  The stage counts as hidden behind the step only if the two medians differ by less than the spread (max - min)
    of the runs without it.

    python tools/bench_codec.py [--out <json>] [--timeout SECONDS] [--kind frames|train]

Every configuration runs in a fresh child process (this file with --child) under its own `timeout -k 10`; the parent never touches the
GPU, and the run stops at the first child that does not exit 0: nothing more is started on the device after that."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_roi import BLOCKS, summary, timed_blocks  # noqa: E402
from bench_shake import BATCH, H, LENGTHS, PATCH, STARTS, T, TRAIN_STEPS, W, _frames  # noqa: E402

QUALITIES = (10, 50, 90)
CODEC = "30..90"
PAIRS = 3


def child_frames(a) -> dict:
    import numpy as np
    import torch
    from speinet_amd import _lib, codec, light
    torch.cuda.set_device(0)
    dev, vp = "cuda:0", C.c_void_p
    M = len(STARTS)
    clip = torch.from_numpy(_frames(T, 0)).to(dev)
    runs_host = torch.tensor(list(zip(STARTS, LENGTHS)), dtype=torch.int32)
    runs = runs_host.to(dev)
    tab, tab_host = light.device_tables("srgb", dev)
    blur = torch.empty((M, H, W, 3), dtype=torch.uint8, device=dev)
    gt = torch.empty((M, H, W, 3), dtype=torch.uint8, device=dev)
    gray = torch.empty((M, H, W), device=dev)
    coded = clip[:M].clone()
    copy_dst = torch.empty_like(coded)
    q_dev, q_host = codec.device_qtabs(codec.quant_tables(a.quality)[None], dev)
    rec_host = torch.from_numpy(codec.records(M).view(np.uint8).copy())
    rec = rec_host.to(dev)
    lib = _lib.lib()
    st = vp(torch.cuda.current_stream().cuda_stream)
    p = lambda t: vp(t.data_ptr())                          # noqa: E731
    fns = {"window_light": lambda: _lib.check(lib.spei_window_mean_light_u8(p(clip), clip.stride(0), T, p(runs), p(runs_host), M, p(tab), p(tab_host),
                                                                            p(blur), p(gt), p(gray), H, W, st), "light"),
           "codec": lambda: _lib.check(lib.spei_codec_u8(p(coded), coded.stride(0), M, H, W, p(rec), p(rec_host), p(q_dev), p(q_host), 1, p(gray),
                                                         st), "codec"),
           "codec_no_gray": lambda: _lib.check(lib.spei_codec_u8(p(coded), coded.stride(0), M, H, W, p(rec), p(rec_host), p(q_dev), p(q_host), 1,
                                                                 vp(0), st), "codec"),
           "copy": lambda: copy_dst.copy_(coded)}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = timed_blocks(fns, 20)
    nbytes = M * H * W * 3
    out = {"kind": "frames", "quality": a.quality, "device": torch.cuda.get_device_name(0), "blocks": BLOCKS, "launches_per_block": 20,
           "frames": f"{M} frames of {H}x{W}; window_light: runs of {LENGTHS} frames", "mcus_per_frame": (H // 16) * (W // 16)}
    out.update({name: summary(*t[name], nbytes=2 * nbytes if name != "window_light" else None) for name in fns})
    out["us_per_720p_frame"] = out["codec"]["us_median"] / M
    out["multiple_of_the_light_entry"] = out["codec"]["us_median"] / out["window_light"]["us_median"]
    out["multiple_of_the_copy"] = out["codec"]["us_median"] / out["copy"]["us_median"]
    return out


def child_train(a) -> dict:
    import shutil
    import tempfile
    import time
    import torch
    from PIL import Image
    from speinet_amd import data
    from speinet_amd.fit import build_model
    from speinet_amd.loss import Loss
    from speinet_amd.trainer import Trainer
    torch.cuda.set_device(0)
    dev = "cuda:0"
    tmp = tempfile.mkdtemp()
    try:
        for c in range(2):
            os.makedirs(os.path.join(tmp, f"clip{c}"))
            distinct = _frames(10, c)
            for i in range(80):
                Image.fromarray(distinct[i % 10]).save(os.path.join(tmp, f"clip{c}", f"{i:06d}.png"), compress_level=1)
        cs = data.SharpClipSet(tmp, ratios=(0.5,), seed=0, references=False, patch=PATCH, light="srgb", codec=a.codec)
        loader = data.SharpTrainLoader(cs, data.SharpStore(cs, device=dev, log=None), BATCH, PATCH, seed=1, prefetch=True, rank=0, world=1)
        net = build_model("swint", dev, synthetic_seed=0)
        trainer = Trainer(net, Loss("1*L1+2*HEM", device=dev), lr=1e-4)
        stamps = []
        with torch.cuda.device(dev):
            done = 0
            while done < TRAIN_STEPS:                      # epochs of the small set until the steps are done, as fit's loop runs them
                for inp, gt in loader:
                    if inp.shape[0] != BATCH:
                        continue
                    trainer.step(inp, gt)
                    torch.cuda.synchronize()
                    stamps.append(time.perf_counter())
                    done += 1
                    if done == TRAIN_STEPS:
                        break
        steps = [b - a_ for a_, b in zip(stamps[1:], stamps[2:])]
        return {"kind": "train", "codec": a.codec, "summary": cs.summary().replace(tmp, "<tmp>"), "device": torch.cuda.get_device_name(0),
                "steps_timed": len(steps), "step_ms_median": sorted(steps)[len(steps) // 2] * 1e3, "step_ms_all": [s * 1e3 for s in steps],
                "crops_per_s": BATCH * len(steps) / (stamps[-1] - stamps[1]), "train_precision": net.train_precision}
    finally:
        shutil.rmtree(tmp)


def child(a) -> None:
    try:
        rec = {"frames": child_frames, "train": child_train}[a.kind](a)
    except Exception as e:                                 # recorded, and the run ends with this child
        rec = {"kind": a.kind, "error": f"{type(e).__name__}: {e}"[:600]}
    print("RESULT " + json.dumps(rec), flush=True)
    if "error" in rec:
        sys.exit(3)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_bench.json"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per configuration")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kind", choices=("frames", "train"))
    ap.add_argument("--quality", type=int, default=50)
    ap.add_argument("--codec", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    jobs = [["--kind", "frames", "--quality", str(q)] for q in QUALITIES]
    for _ in range(PAIRS):
        jobs += [["--kind", "train"], ["--kind", "train", "--codec", CODEC]]
    if a.kind is not None:
        jobs = [j for j in jobs if j[1] == a.kind]
    res = {"method": f"one fresh process per configuration.  frames: {BLOCKS} alternating blocks of 20 launches per entry between two device "
                     "events, each block queued behind a spin kernel so that the device and not the host's launch rate is timed, us per "
                     "launch = block time / launches, medians over blocks; the C entry points into buffers allocated once; the codec works "
                     "in place on its own output of the launch before (its cost does not depend on the bytes).  train: swint steps fed by "
                     f"SharpTrainLoader with prefetch, light srgb, without and with codec {CODEC} in alternation, wall clock per step with "
                     "a synchronize, the first two steps dropped",
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
    train = {c: [r["crops_per_s"] for r in res["runs"] if r.get("kind") == "train" and r.get("codec") == c and "crops_per_s" in r] for c in (None, CODEC)}
    if len(train[None]) >= 2 and train[CODEC]:
        spread = max(train[None]) - min(train[None])
        diff = abs(statistics.median(train[None]) - statistics.median(train[CODEC]))
        res["train"] = {"crops_per_s_without": train[None], "crops_per_s_with": train[CODEC], "median_without": statistics.median(train[None]),
                        "median_with": statistics.median(train[CODEC]), "spread_without": spread, "difference_of_medians": diff,
                        "hidden_behind_the_step": diff < spread}
    json.dump(res, open(a.out, "w"), indent=1)
    print("done" if res["stopped"] is None else res["stopped"])
    if res["stopped"] is not None:
        sys.exit(1)


if __name__ == "__main__":
    main()
