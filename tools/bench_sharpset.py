"""Cost of building a training batch from sharp footage (spei_train_batch_runs_u8, data.SharpTrainLoader) next to the batch of a
precomputed set (spei_train_batch_u8, data.TrainLoader) and to one swint training step, at batch 20 and patch 200 on resident 720p
clips -> profiles/sharpset_bench.json.

    python tools/bench_sharpset.py [--out <json>] [--frames 240]

Medians of alternating repeats; a host clock around work that ends in a torch.cuda.synchronize.  A "launch" figure is the time per
launch of LAUNCHES launches issued back to back over BATCHES different batches (their source bytes exceed the 256 MiB last-level
cache), record tables already on the device; a "loader" figure is one `_launch` per batch: the table on the host, its copy, the
launch."""
import argparse, json, os, shutil, statistics, sys, tempfile, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speinet_amd import blurset, data
from PIL import Image

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sharpset_bench.json"))
ap.add_argument("--frames", type=int, default=240, help="sharp 720p frames per clip (two clips)")
ARGS = ap.parse_args()
DEV = "cuda:0"
torch.cuda.set_device(0)
BATCH, PATCH, BATCHES, LAUNCHES, REPEATS = 20, 200, 4, 48, 7


def frames720(T, seed):
    r = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(720), np.arange(1280), indexing="ij")
    out = np.empty((T, 720, 1280, 3), np.uint8)
    for t in range(T):
        base = 128 + 70 * np.sin(0.031 * (xx + 2 * t)) * np.cos(0.047 * yy) + 30 * np.sin(0.4 * (xx + yy + t))
        out[t] = np.clip(base[..., None] * np.array([1.0, 0.9, 1.1]) + 12 * r.randn(720, 1280, 1), 0, 255)
    return out


tmp = tempfile.mkdtemp()
sharp_dir = os.path.join(tmp, "sharp")
for c in range(2):
    os.makedirs(os.path.join(sharp_dir, f"clip{c}"))
    distinct = frames720(10, c)
    for i in range(ARGS.frames):
        Image.fromarray(distinct[i % 10]).save(os.path.join(sharp_dir, f"clip{c}", f"{i:06d}.png"), compress_level=1)
print("sharp clips written", flush=True)


def prepared(loader, n):
    """n batches of the loader's next epoch as (device table, host table, input, gt) and the items they were made of."""
    batches = [b for b in loader.sampler.epoch() if len(b) == BATCH][:n]
    assert len(batches) == n, f"the epoch has fewer than {n} full batches"
    out = []
    for items in batches:
        rec = loader._records(items)
        host = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())
        out.append((host.to(DEV), host, torch.empty((BATCH, loader.F, 3, PATCH, PATCH), device=DEV), torch.empty((BATCH, 3, PATCH, PATCH), device=DEV)))
    return out, batches


def launches(loader, tables):
    def run():
        for k in range(LAUNCHES):
            dev, host, inp, gt = tables[k % len(tables)]
            loader._build(dev, host, BATCH * loader.F, BATCH, inp, gt, PATCH, 1.0)
    return run, LAUNCHES


def loads(loader, batches):
    def run():
        for items in batches:
            loader._launch(items)
    return run, len(batches)


variants, info = {}, {}
for ratio in (0.1, 0.5):
    cs = data.SharpClipSet(sharp_dir, ratios=(ratio,), seed=0, patch=PATCH)
    loader = data.SharpTrainLoader(cs, data.SharpStore(cs, device=DEV), BATCH, PATCH, seed=1, prefetch=False, rank=0, world=1)
    tables, batches = prepared(loader, BATCHES)
    rec = np.concatenate([loader._records(b)[:BATCH * loader.F] for b in batches])
    read = int((rec["length"] * ((rec["flags"] & data.F_ZERO) == 0)).sum()) / len(batches) * PATCH * PATCH * 3
    info[f"runs_ratio_{ratio}"] = {"summary": cs.summary(), "mean_run_of_an_input_record": float(rec["length"].mean()),
                                   "source_bytes_per_batch": read + BATCH * PATCH * PATCH * 3,
                                   "output_bytes_per_batch": BATCH * (loader.F + 1) * 3 * PATCH * PATCH * 4}
    variants[f"train_batch_runs_launch_ratio_{ratio}"] = launches(loader, tables)
    variants[f"sharp_loader_batch_ratio_{ratio}"] = loads(loader, batches)
    if ratio == 0.5:
        out_dir = os.path.join(tmp, "set")
        blurset.write_dataset(sharp_dir, out_dir, ratios=(ratio,), seed=0, device=DEV)
        ws = data.ClipSet(out_dir, True, patch=PATCH)
        wl = data.TrainLoader(ws, data.ClipStore(ws, device=DEV), BATCH, PATCH, seed=1, prefetch=False, rank=0, world=1)
        wt, wb = prepared(wl, BATCHES)
        variants["train_batch_u8_launch_written_set"] = launches(wl, wt)
        variants["loader_batch_written_set"] = loads(wl, wb)

times = {k: [] for k in variants}
with torch.cuda.device(DEV):
    for rep in range(REPEATS + 1):                             # the first round warms up
        for name, (run, n) in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t0) / n)
res = {"device": torch.cuda.get_device_name(0), "frame": "720x1280", "batch": BATCH, "patch": PATCH, "records_per_batch": BATCH * 6,
       "method": f"median of {REPEATS} alternating repeats after one warm-up round, host wall clock around a torch.cuda.synchronize; a "
                 f"launch figure is the time per launch of {LAUNCHES} back-to-back launches over {BATCHES} different batches, a loader "
                 "figure the time per batch of one _launch (host table, copy, launch) per batch; one process",
       "sets": info, "microseconds": {k: {"median": statistics.median(v) * 1e6, "all": [t * 1e6 for t in v]} for k, v in times.items()}}
for k, v in res["microseconds"].items():
    print(f"{k}: {v['median']:.1f} us", flush=True)

# one swint training step on a batch of the sharp loader (the step the launch is to be small against)
from speinet_amd.fit import build_model
from speinet_amd.loss import Loss
from speinet_amd.trainer import Trainer
cs = data.SharpClipSet(sharp_dir, ratios=(0.5,), seed=0, references=False, patch=PATCH)
loader = data.SharpTrainLoader(cs, data.SharpStore(cs, device=DEV, log=None), BATCH, PATCH, seed=1, prefetch=False, rank=0, world=1)
net = build_model("swint", DEV, synthetic_seed=0)
trainer = Trainer(net, Loss("1*L1+2*HEM", device=DEV), lr=1e-4)
steps = []
with torch.cuda.device(DEV):
    for k, (inp, gt) in enumerate(loader):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trainer.step(inp, gt)
        torch.cuda.synchronize()
        steps.append(time.perf_counter() - t0)
        if k == 5:
            break
step = statistics.median(steps[1:])
res["swint_training_step_ms"] = {"median": step * 1e3, "all": [t * 1e3 for t in steps[1:]], "train_precision": net.train_precision}
res["launch_share_of_the_step_percent"] = {k: v["median"] / 1e4 / step for k, v in res["microseconds"].items()}
print(json.dumps(res["swint_training_step_ms"]), json.dumps(res["launch_share_of_the_step_percent"]), flush=True)
shutil.rmtree(tmp)
os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
json.dump(res, open(ARGS.out, "w"), indent=1)
print("done")
