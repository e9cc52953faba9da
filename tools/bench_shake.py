"""Camera-shake blur in blur synthesis (csrc/shake.hip; speinet_amd/shake.py) on one MI355X -> profiles/shake_bench.json.  By the
protocol of tools/bench_roi.py (device events around alternating blocks of launches, each block queued behind a spin kernel, medians of
20 blocks, a fresh process per configuration), on the C entry points into buffers allocated once:

  * steady: every record at radius 0.  spei_window_mean_shake_u8 on four 720p runs (1, 2, 7 and 15 frames) beside
    spei_window_mean_light_u8 (gauss == NULL) and spei_window_mean_noise_u8 (with gauss) on the same runs, and
    spei_train_batch_runs_shake_u8 on a training batch of 20 windows of 200 x 200 (120 records) beside the light and noise entries.
    The bar: 1.5 times.  The steady path is meant to be the old path.
  * shaken: the four runs all shaken at radius 4, 8 and 16, with the dense table (every tap set) and with generated trajectory PSFs of
    that radius (one per run): device time per 720p frame, and the same as a multiple of the light entry's time on those runs.  No bar.
  * train: swint training steps (batch 20, 200 x 200, synthetic weights) fed by data.SharpTrainLoader with prefetch, as `fit --dir_sharp`
    runs them, with and without shake 4..24: crops/s over the steps after the first two.  No bar.

    python tools/bench_shake.py [--out <json>] [--timeout SECONDS] [--kind steady|shaken|train]

Every configuration runs in a fresh child process (this file with --child) under its own `timeout -k 10`; the parent never touches the
GPU, and the run stops at the first child that does not exit 0: nothing more is started on the device after that."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_roi import BAR, BLOCKS, summary, timed_blocks  # noqa: E402

H, W, T = 720, 1280, 25
STARTS, LENGTHS = (0, 1, 3, 10), (1, 2, 7, 15)
BATCH, PATCH, F = 20, 200, 5
RADII = (4, 8, 16)
LEVELS = (5e-3, 1e-2)                                      # shot coefficient and read deviation of the noise entries
TRAIN_STEPS = 12


def _frames(n, seed):
    import numpy as np
    r = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = np.empty((n, H, W, 3), np.uint8)
    for t in range(n):
        base = 128 + 70 * np.sin(0.031 * (xx + 2 * t)) * np.cos(0.047 * yy) + 30 * np.sin(0.4 * (xx + yy + t))
        out[t] = np.clip(base[..., None] * np.array([1.0, 0.9, 1.1]) + 12 * r.randn(H, W, 1), 0, 255)
    return out


def _dense(radius):
    import numpy as np
    n = 2 * radius + 1
    a = np.full((n, n), 65536 // (n * n), np.int64)
    a[radius, radius] += 65536 - a.sum()
    w = np.zeros((33, 33), np.uint32)
    w[16 - radius:17 + radius, 16 - radius:17 + radius] = a
    return w


def _setup(psfs, records):
    """The device and host buffers of the window-mean and train-batch entries for the shake `records` (one per run) over `psfs`."""
    import numpy as np
    import torch
    from speinet_amd import _lib, light, shake
    from speinet_amd.data import RUN_RECORD
    torch.cuda.set_device(0)
    dev, vp = "cuda:0", C.c_void_p
    clip = torch.from_numpy(_frames(T, 0)).to(dev)
    M = len(STARTS)
    keep = {"clip": clip}
    runs_host = torch.tensor(list(zip(STARTS, LENGTHS)), dtype=torch.int32)
    keep["runs"] = (runs_host.to(dev), runs_host)
    keep["tab"] = light.device_tables("srgb", dev)
    keep["gauss"] = light.device_gauss(dev)
    A, B = light.noise_levels(f"{LEVELS[0]}:{LEVELS[1]}", 0, 0)
    rng = np.random.RandomState(1)
    # the batch: BATCH windows of F input records and one gt record each, runs and crops drawn at random, every flag combination
    rows, run_of = [], []
    frame = H * W * 3
    for b in range(BATCH):
        y0, x0, flags = rng.randint(0, H - PATCH + 1), rng.randint(0, W - PATCH + 1), rng.randint(0, 8)
        for f in range(F):
            m = rng.randint(0, M)
            rows.append((clip.data_ptr() + STARTS[m] * frame, frame, W * 3, y0, x0, flags, H, W, LENGTHS[m], T - STARTS[m]))
            run_of.append(m)
    for b in range(BATCH):
        r = rows[b * F + F // 2]
        rows.append((clip.data_ptr() + 12 * frame, frame, W * 3, r[3], r[4], r[5], H, W, 1, T - 12))
        run_of.append(None)
    table = np.array(rows, dtype=RUN_RECORD)

    def pair(rec):
        host = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())
        return host.to(dev), host
    keep["table"] = pair(table)
    keep["noise_w"] = pair(light.noise_records(np.arange(M), 0, A, B))
    keep["noise_b"] = pair(light.noise_records([0 if m is None else m for m in run_of], 0, A, B))
    srec = np.array(records, dtype=shake.SHAKE_RECORD)
    sb = np.zeros(len(rows), dtype=shake.SHAKE_RECORD)
    sb["q16"] = 65536
    for k, m in enumerate(run_of):
        if m is not None:
            sb[k] = srec[m]
    keep["shake_w"], keep["shake_b"] = pair(srec), pair(sb)
    keep["psfs"] = shake.device_psfs(psfs, dev)
    keep["n_psf"] = int(psfs.shape[0])
    keep["blur"] = torch.empty((M, H, W, 3), dtype=torch.uint8, device=dev)
    keep["gt"] = torch.empty((M, H, W, 3), dtype=torch.uint8, device=dev)
    keep["gray"] = torch.empty((M, H, W), device=dev)
    keep["inp"] = torch.empty((BATCH * F, 3, PATCH, PATCH), device=dev)
    keep["bgt"] = torch.empty((BATCH, 3, PATCH, PATCH), device=dev)
    lib = _lib.lib()
    st = vp(torch.cuda.current_stream().cuda_stream)
    p = lambda t: vp(t.data_ptr() if t.numel() else 0)     # noqa: E731
    null = vp(0)
    w_head = (p(clip), clip.stride(0), T, p(keep["runs"][0]), p(keep["runs"][1]), M, p(keep["tab"][0]), p(keep["tab"][1]))
    w_tail = (p(keep["blur"]), p(keep["gt"]), p(keep["gray"]), H, W, st)
    b_head = (p(keep["table"][0]), p(keep["table"][1]), BATCH * F, BATCH, p(keep["tab"][0]), p(keep["tab"][1]))
    b_tail = (p(keep["inp"]), p(keep["bgt"]), PATCH, 1.0, st)
    gs = (p(keep["gauss"][0]), p(keep["gauss"][1]))
    no_noise = (null, null, null, null, 0, 0)
    sk = lambda which: (p(keep["psfs"][0]), p(keep["psfs"][1]), keep["n_psf"], p(keep[which][0]), p(keep[which][1]))     # noqa: E731

    def call(fn, name, *args):
        return lambda: _lib.check(fn(*args), name)
    fns = {"window_light": call(lib.spei_window_mean_light_u8, "light", *w_head, *w_tail),
           "window_noise": call(lib.spei_window_mean_noise_u8, "noise", *w_head, *gs, p(keep["noise_w"][0]), p(keep["noise_w"][1]), 3, 4, *w_tail),
           "window_shake": call(lib.spei_window_mean_shake_u8, "shake", *w_head, *no_noise, *sk("shake_w"), *w_tail),
           "window_shake_noise": call(lib.spei_window_mean_shake_u8, "shake", *w_head, *gs, p(keep["noise_w"][0]), p(keep["noise_w"][1]), 3, 4,
                                      *sk("shake_w"), *w_tail),
           "batch_light": call(lib.spei_train_batch_runs_light_u8, "light", *b_head, *b_tail),
           "batch_noise": call(lib.spei_train_batch_runs_noise_u8, "noise", *b_head, *gs, p(keep["noise_b"][0]), p(keep["noise_b"][1]), 3, 4, *b_tail),
           "batch_shake": call(lib.spei_train_batch_runs_shake_u8, "shake", *b_head, *no_noise, *sk("shake_b"), *b_tail),
           "batch_shake_noise": call(lib.spei_train_batch_runs_shake_u8, "shake", *b_head, *gs, p(keep["noise_b"][0]), p(keep["noise_b"][1]), 3, 4,
                                     *sk("shake_b"), *b_tail)}
    return keep, fns


def _time(fns, launches):
    import torch
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = timed_blocks(fns, launches)
    return {name: summary(*t[name]) for name in fns}


def child_steady(a) -> dict:
    import numpy as np
    import torch
    keep, fns = _setup(np.zeros((0, 33, 33), np.uint32), [(0, 0, 65536, 0)] * len(STARTS))
    rec = {"kind": "steady", "device": torch.cuda.get_device_name(0), "blocks": BLOCKS, "launches_per_block": 20,
           "window": f"{len(STARTS)} runs of {LENGTHS} frames at {H}x{W}", "batch": f"{BATCH} windows of {F} + 1 records at {PATCH}x{PATCH}"}
    rec.update(_time(fns, 20))
    rec["ratios"] = {"window_shake_to_light": rec["window_shake"]["us_median"] / rec["window_light"]["us_median"],
                     "window_shake_noise_to_noise": rec["window_shake_noise"]["us_median"] / rec["window_noise"]["us_median"],
                     "batch_shake_to_light": rec["batch_shake"]["us_median"] / rec["batch_light"]["us_median"],
                     "batch_shake_noise_to_noise": rec["batch_shake_noise"]["us_median"] / rec["batch_noise"]["us_median"]}
    rec["bar"] = BAR
    rec["within_bar"] = max(rec["ratios"].values()) <= BAR
    return rec


def child_shaken(a) -> dict:
    import numpy as np
    import torch
    from speinet_amd import shake
    M = len(STARTS)
    if a.psf == "dense":
        tabs = [_dense(a.radius)] * M
    else:                                                  # generated PSFs of the radius: the extent 2 (radius - 1) has floor(L / 2) + 1 = radius
        tabs = [shake.psf(str(2 * (a.radius - 1)), 0, 0, m)[0] for m in range(M)]
    psfs = np.stack(tabs).astype(np.uint32)
    records = [(m, a.radius, shake.q16_of(psfs[m]), 0) for m in range(M)]
    keep, fns = _setup(psfs, records)
    fns = {k: fns[k] for k in ("window_light", "window_shake", "window_shake_noise", "batch_light", "batch_shake")}
    rec = {"kind": "shaken", "psf": a.psf, "radius": a.radius, "taps_set": [int(np.count_nonzero(t)) for t in tabs],
           "device": torch.cuda.get_device_name(0), "blocks": BLOCKS, "launches_per_block": 5}
    rec.update(_time(fns, 5))
    rec["us_per_720p_frame"] = rec["window_shake"]["us_median"] / M
    rec["us_per_720p_frame_with_noise"] = rec["window_shake_noise"]["us_median"] / M
    rec["multiple_of_the_light_entry"] = rec["window_shake"]["us_median"] / rec["window_light"]["us_median"]
    rec["batch_multiple_of_the_light_entry"] = rec["batch_shake"]["us_median"] / rec["batch_light"]["us_median"]
    return rec


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
        t0 = time.perf_counter()
        cs = data.SharpClipSet(tmp, ratios=(0.5,), seed=0, references=False, patch=PATCH, light="srgb", shake=a.shake)
        plan_s = time.perf_counter() - t0
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
        return {"kind": "train", "shake": a.shake, "summary": cs.summary().replace(tmp, "<tmp>"), "device": torch.cuda.get_device_name(0),
                "steps_timed": len(steps), "step_ms_median": sorted(steps)[len(steps) // 2] * 1e3, "step_ms_all": [s * 1e3 for s in steps],
                "crops_per_s": BATCH * len(steps) / (stamps[-1] - stamps[1]), "plan_seconds": plan_s, "train_precision": net.train_precision}
    finally:
        shutil.rmtree(tmp)


def child(a) -> None:
    try:
        rec = {"steady": child_steady, "shaken": child_shaken, "train": child_train}[a.kind](a)
    except Exception as e:                                 # recorded, and the run ends with this child
        rec = {"kind": a.kind, "error": f"{type(e).__name__}: {e}"[:600]}
    print("RESULT " + json.dumps(rec), flush=True)
    if "error" in rec:
        sys.exit(3)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shake_bench.json"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per configuration")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kind", choices=("steady", "shaken", "train"))
    ap.add_argument("--radius", type=int, default=16)
    ap.add_argument("--psf", choices=("dense", "trajectory"), default="dense")
    ap.add_argument("--shake", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    jobs = [["--kind", "steady"]]
    jobs += [["--kind", "shaken", "--radius", str(r), "--psf", kind] for r in RADII for kind in ("dense", "trajectory")]
    jobs += [["--kind", "train"], ["--kind", "train", "--shake", "4..24"]]
    if a.kind is not None:
        jobs = [j for j in jobs if j[1] == a.kind]
    res = {"method": f"one fresh process per configuration.  steady and shaken: {BLOCKS} alternating blocks of launches per entry between two "
                     "device events, each block queued behind a spin kernel so that the device and not the host's launch rate is timed, us "
                     "per launch = block time / launches, medians over blocks; the C entry points into buffers allocated once, light srgb, "
                     f"noise levels {LEVELS}.  steady: every record at radius 0, bar {BAR} against the light and the noise entries.  shaken: "
                     "all four runs shaken.  train: swint steps fed by SharpTrainLoader with prefetch, wall clock per step with a "
                     "synchronize, the first two steps dropped",
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
    json.dump(res, open(a.out, "w"), indent=1)
    print("done" if res["stopped"] is None else res["stopped"])
    if res["stopped"] is not None:
        sys.exit(1)


if __name__ == "__main__":
    main()
