"""Frames/s at 720p of detector.dataset_features (k = 11, 13, 201), of the focus-measure launches alone on resident gray planes, and
of blurset.synthesize -> profiles/blurset_detector_bench.json.

    python tools/bench_blurset.py [--parent-lib <libspeinet_hip.so of an earlier build>] [--out <json>]

With --parent-lib the earlier build's spei_det_features (its direct k x k box sums at every k) runs through the same Python pipeline in
the same process, for the comparison at k = 201."""
import ctypes as C, json, os, random, statistics, sys, tempfile, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speinet_amd import _lib, blurset, detector, ops
from PIL import Image

import argparse
ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blurset_detector_bench.json"))
ARGS = ap.parse_args()
DEV = "cuda:0"
torch.cuda.set_device(0)
lib = _lib.lib()
parent = C.CDLL(ARGS.parent_lib) if ARGS.parent_lib else None
for name in ("spei_det_ws_floats", "spei_det_features") if parent else ():
    res, args = _lib.SIGNATURES[name]
    getattr(parent, name).restype, getattr(parent, name).argtypes = res, args

def parent_gfm(gray, k=11):
    gray = gray.contiguous().float(); n, h, w = gray.shape
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty(n, 6, device=gray.device)
    ws = torch.empty(parent.spei_det_ws_floats(n, h, w, k), device=gray.device)
    rc = parent.spei_det_features(C.c_void_p(gray.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), n, h, w, k, st)
    assert rc == 0
    return out

def frames720(T, seed):
    r = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(720), np.arange(1280), indexing="ij")
    out = np.empty((T, 720, 1280, 3), np.uint8)
    for t in range(T):
        base = 128 + 70 * np.sin(0.031 * (xx + 2 * t)) * np.cos(0.047 * yy) + 30 * np.sin(0.4 * (xx + yy + t))
        out[t] = np.clip(base[..., None] * np.array([1.0, 0.9, 1.1]) + 12 * r.randn(720, 1280, 1), 0, 255)
    return out

res = {"device": torch.cuda.get_device_name(0), "frame": "720x1280", "method":
       "median of 5 timed repeats after one warm-up run, host wall clock around a torch.cuda.synchronize (dataset_features, synthesize "
       "from host) or HIP events on the stream (launches alone); one process, one otherwise idle MI355X; 'parent' = the previous "
       "commit's library loaded next to this one, its direct GRA7/STA3 box sums called through the same Python pipeline"}
T = 64
fr = frames720(T, 1)
tmp = tempfile.mkdtemp()
os.makedirs(os.path.join(tmp, "blur", "clip"))
for i, f in enumerate(fr):
    Image.fromarray(f).save(os.path.join(tmp, "blur", "clip", f"{i:06d}.png"), compress_level=1)

def wall(fn, reps=5):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts

def events(fn, reps=5):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b) / 1e3)
    return statistics.median(ts), ts

df = {}
for k in (11, 13, 201):
    m, ts = wall(lambda: detector.dataset_features(tmp, k, DEV))
    df[f"k{k}"] = {"frames_per_s": T / m, "seconds": ts}
    print("dataset_features", k, T / m, flush=True)
if parent:
    keep = detector.gray_focus_measures
    detector.gray_focus_measures = parent_gfm
    try:
        m, ts = wall(lambda: detector.dataset_features(tmp, 201, DEV), reps=3)
    finally:
        detector.gray_focus_measures = keep
    df["k201_parent_bruteforce"] = {"frames_per_s": T / m, "seconds": ts}
    print("dataset_features parent 201", T / m, flush=True)
res["dataset_features_png_720p_64_frames"] = df

_, gray = ops.frames_u8_in(torch.from_numpy(fr[:16]).to(DEV), gray=True, planes=False)
ln = {}
for k in (11, 13, 51, 101, 201):
    m, ts = events(lambda: detector.gray_focus_measures(gray, k))
    ln[f"k{k}"] = {"frames_per_s": 16 / m, "seconds": ts}
    print("launches", k, 16 / m, flush=True)
for k in (13, 201) if parent else ():
    m, ts = events(lambda: parent_gfm(gray, k), reps=3)
    ln[f"k{k}_parent_bruteforce"] = {"frames_per_s": 16 / m, "seconds": ts}
    print("launches parent", k, 16 / m, flush=True)
res["focus_measures_16_resident_gray_planes"] = ln

T2 = 240
src = frames720(8, 2)
big = np.concatenate([src] * (T2 // 8))
runs = blurset.plan_runs(T2, 0.5, rng=random.Random(1))
M = len(runs[0])
dev_src = torch.from_numpy(big).to(DEV)
m, ts = events(lambda: blurset.synthesize(dev_src, runs, DEV, chunk_frames=T2))
nbytes = (T2 + 2 * M) * 720 * 1280 * 3
sy = {"resident_source_one_launch": {"source_frames_per_s": T2 / m, "output_frames_per_s": M / m, "GB_per_s_minimum_traffic": nbytes / m / 1e9, "seconds": ts, "runs": M}}
m, ts = events(lambda: blurset.synthesize(dev_src, runs, DEV, gray=True, chunk_frames=T2))
sy["resident_source_with_gray_planes"] = {"source_frames_per_s": T2 / m, "output_frames_per_s": M / m, "seconds": ts}
m, ts = wall(lambda: blurset.synthesize(big, runs, DEV))
sy["host_array_source_chunks_of_64"] = {"source_frames_per_s": T2 / m, "output_frames_per_s": M / m, "seconds": ts}
res["synthesize_720p_240_frames"] = sy
print(json.dumps(sy), flush=True)
import shutil
shutil.rmtree(tmp)
json.dump(res, open(ARGS.out, "w"), indent=1)
print("done")
