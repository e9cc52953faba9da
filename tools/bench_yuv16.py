"""Cost of the frame-path launches of the clip API at 8 bits and at 10 / 12 bits (csrc/yuv_io.hip, csrc/frame_io.hip): the five
16-bit launches (spei_yuv_to_rgb_u16, spei_rgb_u16_to_yuv, spei_frames_u16_in, spei_frame_u16_out, spei_frame_pair_stats_u16) next to
their uint8 siblings, at 720p and 1080p on one MI355X -> profiles/yuv16_bench.json.

    python tools/bench_yuv16.py [--out <json>] [--label <text>]

Medians of alternating repeats; a host clock around work that ends in a torch.cuda.synchronize.  A figure is the time per launch of
LAUNCHES launches issued back to back over SETS different sets of buffers (their bytes exceed the 256 MiB last-level cache, so a
launch streams from HBM), and the GB/s moved: the bytes the launch must read plus those it must write, computed from the shapes
here, over that time.  The launch includes the host side of the `ops` wrapper.  A tree without the 16-bit ops (the commit before
them) is timed on its uint8 launches alone: run there, the record is the baseline that shows whether the 8-bit path moved."""
import argparse, json, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speinet_amd import ops, y4m

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv16_bench.json"))
ap.add_argument("--label", default="", help="free text kept in the record (which tree was timed)")
ARGS = ap.parse_args()
DEV = "cuda:0"
torch.cuda.set_device(0)
LAUNCHES, REPEATS, BATCH = 96, 7, 4
LLC = 256 << 20
DEEP = hasattr(ops, "yuv_to_rgb_u16")
LAYOUT, MATRIX, RANGE = y4m.LEFT, y4m.BT709, y4m.LIMITED


def make(shape, dtype, hi, seed):
    """A device tensor of seeded random samples in [0, hi), made on the device."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, hi, shape, dtype=torch.uint8, device=DEV, generator=g)
    return torch.randint(0, hi, shape, dtype=torch.int16, device=DEV, generator=g).view(torch.uint16)


def variants_for(h, w):
    """name -> (callable(set index), bytes moved per launch, sets)."""
    hp, wp = ops.padded_size(h), ops.padded_size(w)
    ns = y4m.frame_bytes(h, w, LAYOUT)                    # samples of a planar 4:2:0 frame
    out = {}

    def add(name, moved, build, call):
        sets = max(2, -(-2 * LLC // moved))               # the sets' bytes exceed twice the last-level cache
        bufs = [build(k) for k in range(sets)]
        out[name] = ((lambda k, bufs=bufs, call=call: call(*bufs[k % len(bufs)])), moved, sets)

    for depth in (8, 10, 12) if DEEP else (8,):
        dt, b, hi = (torch.uint8, 1, 256) if depth == 8 else (torch.uint16, 2, 1 << depth)
        tag = "u8" if depth == 8 else f"u16_d{depth}"
        rgb_b, planar_b, f32_b = h * w * 3 * b, ns * b, 3 * hp * wp * 4
        if depth == 8:
            to_rgb = lambda p, o: ops.yuv_to_rgb_u8(p, h, w, LAYOUT, MATRIX, RANGE, out=o)
            to_yuv = lambda r, o: ops.rgb_u8_to_yuv(r, LAYOUT, MATRIX, RANGE, out=o)
            f_in = lambda r, o: ops.frames_u8_in(r, out=o)
            f_gray = lambda r: ops.frames_u8_in(r, gray=True, planes=False)
            f_out = lambda x, o: ops.frame_u8_out(x, h, w, out=o)
            stats = lambda r: ops.frame_pair_stats(r)
        else:
            to_rgb = lambda p, o, d=depth: ops.yuv_to_rgb_u16(p, h, w, LAYOUT, MATRIX, RANGE, d, out=o)
            to_yuv = lambda r, o, d=depth: ops.rgb_u16_to_yuv(r, LAYOUT, MATRIX, RANGE, d, out=o)
            f_in = lambda r, o, d=depth: ops.frames_u16_in(r, d, out=o)
            f_gray = lambda r, d=depth: ops.frames_u16_in(r, d, gray=True, planes=False)
            f_out = lambda x, o, d=depth: ops.frame_u16_out(x, h, w, d, out=o)
            stats = lambda r, d=depth: ops.frame_pair_stats_u16(r, d)
        add(f"yuv_to_rgb_{tag}_x{BATCH}", BATCH * (planar_b + rgb_b),
            lambda k: (make((BATCH, ns), dt, hi, k), torch.empty(BATCH, h, w, 3, dtype=dt, device=DEV)), to_rgb)
        add(f"rgb_to_yuv_{tag}", rgb_b + planar_b,
            lambda k: (make((h, w, 3), dt, hi, k), torch.empty(ns, dtype=dt, device=DEV)), to_yuv)
        add(f"frames_in_{tag}", rgb_b + f32_b,
            lambda k: (make((h, w, 3), dt, hi, k), torch.empty(1, 3, hp, wp, device=DEV)), f_in)
        add(f"frames_in_gray_only_{tag}_x{BATCH}", BATCH * (rgb_b + h * w * 4), lambda k: (make((BATCH, h, w, 3), dt, hi, k),), f_gray)
        add(f"frame_out_{tag}", f32_b + rgb_b,
            lambda k: (torch.rand(3, hp, wp, device=DEV), torch.empty(h, w, 3, dtype=dt, device=DEV)), f_out)
        # every frame but the first is read twice (as b of one pair, as a of the next): from the cache the second time at best
        add(f"frame_pair_stats_{tag}_x{BATCH}", BATCH * rgb_b, lambda k: (make((BATCH, h, w, 3), dt, hi, k),), stats)
    return out


res = {"device": torch.cuda.get_device_name(0), "label": ARGS.label, "deep_ops": DEEP, "layout": "420mpeg2 bt709 limited",
       "method": f"median of {REPEATS} alternating repeats after one warm-up round, host wall clock around a torch.cuda.synchronize; a "
                 f"figure is the time per launch of {LAUNCHES} back-to-back launches (ops wrapper included) over sets of buffers whose "
                 "bytes exceed twice the 256 MiB last-level cache; GB/s = bytes the launch must read and write / that time; one process",
       "sizes": {}}
for name, (h, w) in (("720p", (720, 1280)), ("1080p", (1080, 1920))):
    variants = variants_for(h, w)
    times = {k: [] for k in variants}
    with torch.cuda.device(DEV), torch.no_grad():
        for rep in range(REPEATS + 1):                         # the first round warms up
            for key, (run, moved, sets) in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(LAUNCHES):
                    run(k)
                torch.cuda.synchronize()
                if rep:
                    times[key].append((time.perf_counter() - t0) / LAUNCHES)
    rec = {}
    for key, (run, moved, sets) in variants.items():
        med = statistics.median(times[key])
        rec[key] = {"us_per_launch": med * 1e6, "all_us": [t * 1e6 for t in times[key]], "bytes_moved": moved, "GB_per_s": moved / med / 1e9,
                    "buffer_sets": sets}
        print(f"{name} {key}: {med * 1e6:.1f} us, {moved / med / 1e9:.0f} GB/s", flush=True)
    res["sizes"][name] = rec
    del variants
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
json.dump(res, open(ARGS.out, "w"), indent=1)
print("done")
