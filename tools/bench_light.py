"""Cost of averaging in linear light (spei_train_batch_runs_light_u8, spei_window_mean_light_u8; speinet_amd/light.py) next to the
code-value launches of the same build on the same inputs -> profiles/light_bench.json.

    python tools/bench_light.py [--out <json>] [--frames 240] [--noise <shot>:<read>]

The method of tools/bench_sharpset.py: medians of alternating repeats in one process, a host clock around work that ends in a
torch.cuda.synchronize.  Two workloads on two resident 720p clips:
  * the batch launch at batch 20 / patch 200 (120 records): the time per launch of LAUNCHES launches issued back to back over BATCHES
    different batches, record tables already on the device;
  * one window-mean launch over all 2 x frames frames cut into runs by blurset.plan_runs (ratio 0.5: about 70 runs of 480 frames), gray
    planes included.
The share of a swint training step is taken against the step recorded in profiles/sharpset_bench.json (it is not measured again).
`--noise <spec>` measures the cost of sensor noise instead (spei_train_batch_runs_noise_u8, spei_window_mean_noise_u8): the variants
are `code`, `srgb` and `srgb` with that noise, each noise launch next to its `srgb` counterpart on the same inputs, and the result goes
to profiles/noise_bench.json with the ratios to `srgb` beside those to `code`."""
import argparse, json, os, random, shutil, statistics, sys, tempfile, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speinet_amd import blurset, data, ops
from speinet_amd import light as _light
from PIL import Image

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="default: profiles/light_bench.json, or profiles/noise_bench.json with --noise")
ap.add_argument("--frames", type=int, default=240, help="sharp 720p frames per clip (two clips)")
ap.add_argument("--noise", default=None, help="a noise spec, e.g. 1e-3..1e-2:1e-3..1e-2: measure srgb with and without it")
ARGS = ap.parse_args()
if ARGS.out is None:
    ARGS.out = os.path.join(ROOT, "profiles", "noise_bench.json" if ARGS.noise else "light_bench.json")
DEV = "cuda:0"
torch.cuda.set_device(0)
BATCH, PATCH, BATCHES, LAUNCHES, REPEATS = 20, 200, 4, 48, 7
# (name of the variant, light, noise)
LIGHTS = (("code", "code", None), ("srgb", "srgb", None), ("srgb_noise", "srgb", ARGS.noise)) if ARGS.noise else \
    (("code", "code", None), ("srgb", "srgb", None), ("gamma:2.2", "gamma:2.2", None))


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

variants, info = {}, {}
store = None
for light, spec, noise in LIGHTS:
    cs = data.SharpClipSet(sharp_dir, ratios=(0.5,), seed=0, patch=PATCH, light=spec, noise=noise)
    if store is None:
        store = data.SharpStore(cs, device=DEV)
    store.clipset = cs                                             # one resident copy of the clips serves every light
    loader = data.SharpTrainLoader(cs, store, BATCH, PATCH, seed=1, prefetch=False, rank=0, world=1)
    batches = [b for b in loader.sampler.epoch() if len(b) == BATCH][:BATCHES]
    assert len(batches) == BATCHES
    tables = []
    for items in batches:
        rec = loader._records(items)
        host = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())
        nz = None
        if noise is not None:                                      # the noise records already on the device, as the run records are
            recs, seed = loader._staged
            nhost = torch.from_numpy(recs["noise"].view(np.uint8).reshape(-1).copy())
            nz = (nhost.to(DEV), nhost, seed)
        tables.append((host.to(DEV), host, torch.empty((BATCH, loader.F, 3, PATCH, PATCH), device=DEV), torch.empty((BATCH, 3, PATCH, PATCH), device=DEV), nz))
    if light == "code":
        rec = np.concatenate([loader._records(b)[:BATCH * loader.F] for b in batches])
        info["batch"] = {"summary": cs.summary().replace(tmp + os.sep, ""), "mean_run_of_an_input_record": float(rec["length"].mean())}

    def run(loader=loader, tables=tables):
        for k in range(LAUNCHES):
            dev, host, inp, gt, nz = tables[k % len(tables)]
            loader.ctx.train_batch_runs(dev, host, BATCH * loader.F, BATCH, inp, gt, PATCH, 1.0, light=loader.recipe.light, noise=nz)
    variants[f"train_batch_runs_launch_{light}"] = (run, LAUNCHES)

clip = torch.cat(store.frames)                                     # [2 * frames, 720, 1280, 3]
starts, lengths, _ = blurset.plan_runs(clip.shape[0], 0.5, rng=random.Random(0))
M = len(starts)
blur, gt = torch.empty((M, 720, 1280, 3), dtype=torch.uint8, device=DEV), torch.empty((M, 720, 1280, 3), dtype=torch.uint8, device=DEV)
info["window_mean"] = {"frames": int(clip.shape[0]), "runs": M, "mean_run": float(lengths.mean()),
                       "bytes_moved": int((clip.shape[0] + 2 * M) * 720 * 1280 * 3 + 4 * M * 720 * 1280)}
for light, spec, noise in LIGHTS:
    nz = None
    if noise is not None:
        nz = (_light.noise_records(np.arange(M), 0, *_light.noise_levels(noise, 0, 0)), 0)
        info["window_mean"]["noise"] = {"spec": _light.noise_name(noise), "A": int(nz[0]["A"][0]), "B": int(nz[0]["B"][0])}
    variants[f"window_mean_launch_{light}"] = (lambda spec=spec, nz=nz: ops.window_mean_u8(clip, starts, lengths, gray=True, blur=blur, gt=gt,
                                                                                        light=spec, noise=nz), 1)

times = {k: [] for k in variants}
with torch.cuda.device(DEV):
    for rep in range(REPEATS + 1):                                 # the first round warms up
        for name, (run, n) in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t0) / n)
us = {k: {"median": statistics.median(v) * 1e6, "all": [t * 1e6 for t in v]} for k, v in times.items()}
res = {"device": torch.cuda.get_device_name(0), "frame": "720x1280", "batch": BATCH, "patch": PATCH, "records_per_batch": BATCH * 6,
       "method": f"median of {REPEATS} alternating repeats after one warm-up round, host wall clock around a torch.cuda.synchronize; the "
                 f"batch figure is the time per launch of {LAUNCHES} back-to-back launches over {BATCHES} different batches, the "
                 "window-mean figure one launch (runs uploaded, gray planes allocated and written); one process",
       "inputs": info, "microseconds": us,
       "ratio_to_code": {k: us[k]["median"] / us[k.split("_launch_")[0] + "_launch_code"]["median"] for k in us if not k.endswith("_code")}}
if ARGS.noise:
    res["ratio_to_srgb"] = {k: us[k]["median"] / us[k[:-len("_noise")]]["median"] for k in us if k.endswith("_noise")}
    print(json.dumps(res["ratio_to_srgb"]), flush=True)
step = json.load(open(os.path.join(ROOT, "profiles", "sharpset_bench.json")))["swint_training_step_ms"]["median"]
res["swint_training_step_ms_from_sharpset_bench"] = step
res["batch_launch_share_of_the_step_percent"] = {k: v["median"] / 1e4 / (step / 1e3) for k, v in us.items() if k.startswith("train_batch")}
for k, v in us.items():
    print(f"{k}: {v['median']:.1f} us", flush=True)
print(json.dumps(res["ratio_to_code"]), json.dumps(res["batch_launch_share_of_the_step_percent"]), flush=True)
shutil.rmtree(tmp)
os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
json.dump(res, open(ARGS.out, "w"), indent=1)
print("done")
