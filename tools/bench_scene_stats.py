"""Cost of the scene-cut statistics on a 100-frame 720p clip that is resident on the device (so decode and PCIe do not hide it):
the labelling pass alone (focus measures), the combined pass (focus measures + pair statistics), the pair statistics alone, and the
pair-statistics kernel on one resident batch with its achieved bytes/s.

    python tools/bench_scene_stats.py [--parent-detector <detector.py of an earlier commit>] [--out <json>]

With --parent-detector the earlier commit's `clip_features` runs in the same process, alternating with this one's passes."""
import argparse, ctypes as C, importlib.util, json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speinet_amd import _lib, detector, video

ap = argparse.ArgumentParser()
ap.add_argument("--parent-detector", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_stats_bench.json"))
ap.add_argument("--frames", type=int, default=100)
ARGS = ap.parse_args()
DEV = torch.device("cuda:0")
torch.cuda.set_device(0)
H, W, T, B = 720, 1280, ARGS.frames, video.DETECT_BATCH

parent = None
if ARGS.parent_detector:
    spec = importlib.util.spec_from_file_location("speinet_amd._parent_detector", ARGS.parent_detector)
    parent = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = parent
    spec.loader.exec_module(parent)

r = np.random.RandomState(1)
yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
clip = torch.empty(T, H, W, 3, dtype=torch.uint8, device=DEV)
for t in range(T):
    base = 128 + 70 * np.sin(0.031 * (xx + 2 * t)) * np.cos(0.047 * yy) + 30 * np.sin(0.4 * (xx + yy + t))
    clip[t] = torch.from_numpy(np.clip(base[..., None] * np.array([1.0, 0.9, 1.1]) + 12 * r.randn(H, W, 1), 0, 255).astype(np.uint8)).to(DEV)
fr = video.frames_of(clip)

passes = {"labelling": lambda: detector.clip_pass(fr, DEV, 11, B, features=True, pair_stats=False),
          "combined": lambda: detector.clip_pass(fr, DEV, 11, B, features=True, pair_stats=True),
          "pair_stats_only": lambda: detector.clip_pass(fr, DEV, 11, B, features=False, pair_stats=True)}
if parent:
    passes["labelling_parent"] = lambda: parent.clip_features(fr, DEV, 11, B)
times = {k: [] for k in passes}
for rep in range(8):                                       # the passes in turn, so that drift hits them alike; repeat 0 is the warm-up
    for name, fn in passes.items():
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        if rep:
            times[name].append(time.perf_counter() - t0)

res = {"device": torch.cuda.get_device_name(0), "clip": f"{T} frames {W}x{H}, uint8, resident on the device", "method":
       "passes: host wall clock around a torch.cuda.synchronize, 7 timed repeats after one warm-up, the passes alternating in one "
       "process; kernel: HIP events around 50 back-to-back calls of spei_frame_pair_stats (two clears + one launch each) on 16 resident "
       "frames plus prev, median of 7"}
res["passes_ms_per_frame"] = {k: {"median": 1e3 * statistics.median(v) / T, "all": [1e3 * x / T for x in v]} for k, v in times.items()}

lib = _lib.lib()
hist = torch.empty(B, 64, dtype=torch.int32, device=DEV)
sad = torch.empty(B, dtype=torch.int64, device=DEV)
st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
frames, prev = clip[1:1 + B], clip[0]


def call():
    rc = lib.spei_frame_pair_stats(C.c_void_p(frames.data_ptr()), frames.stride(0), C.c_void_p(prev.data_ptr()), B, H, W,
                                   C.c_void_p(hist.data_ptr()), C.c_void_p(sad.data_ptr()), st)
    assert rc == 0


call(); torch.cuda.synchronize()
ks = []
for _ in range(7):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(50):
        call()
    b.record(); torch.cuda.synchronize(); ks.append(a.elapsed_time(b) / 1e3 / 50)
k = statistics.median(ks)
nbytes = 2 * B * H * W * 3                                 # every frame once as pair member a and once as member b
res["kernel_16_frames_with_prev"] = {"ms_per_call": 1e3 * k, "ms_per_frame": 1e3 * k / B, "bytes_read": nbytes, "GB_per_s": nbytes / k / 1e9,
                                     "all_ms_per_call": [1e3 * x for x in ks]}
print(json.dumps(res, indent=1), flush=True)
os.makedirs(os.path.dirname(ARGS.out), exist_ok=True)
json.dump(res, open(ARGS.out, "w"), indent=1)
