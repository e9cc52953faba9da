"""The command line between two pipes, spooled and streamed, on one MI355X -> profiles/stream_bench.json.

A synthetic 720p 8-bit 4:2:0 y4m clip of 120 frames (smooth fields in slow motion, every ninth frame and its successor sharp, the rest
box-blurred; made once, on the host) is written to the stdin of `python -m speinet_amd.video --input - --output - --model_path synthetic`
(f16 with graphs, the detector's labels) as fast as the child takes it, and its stdout is read to the end: once without `--stream`
(the pipe is spooled to a temporary file, analysed, then deblurred) and once with it, in alternating pairs, a fresh child per run.  Per
run: the wall time from the first input byte to the child's exit, the time from the first input byte to the first complete output frame,
and the child's peak resident set (`os.wait4`).

The bar, on the medians: the streamed total may exceed the spooled total by at most the spread (max - min) of the spooled runs, and by
no less than 5 % of it.  The first-frame latency and the resident set carry no bar.

    python tools/bench_stream.py [--out <json>] [--pairs N] [--frames T] [--timeout SECONDS]

The parent never touches the GPU; every child runs under its own time limit, and the run stops at the first child that does not exit
0: nothing more is started on the device after that."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 720, 1280


def clip_bytes(T: int) -> tuple:
    """(header, [frame records]) of the synthetic clip: planar 4:2:0 made here, on the host."""
    rng = np.random.default_rng(0)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    grain = rng.integers(0, 2, (H // 4, W // 4)).repeat(4, 0).repeat(4, 1).astype(np.float32) * 60.0
    records = []
    for i in range(T):
        y = 90.0 + 50.0 * np.sin((xx + 3 * i) / 37.0) * np.cos((yy - 2 * i) / 53.0) + np.roll(grain, (i, 2 * i), (0, 1))
        if i % 9 not in (0, 1):                                # blurred: a horizontal box of 9
            pad = np.pad(y, ((0, 0), (4, 4)), mode="edge")
            y = sum(pad[:, k:k + W] for k in range(9)) / 9.0
        u = 128.0 + 20.0 * np.sin((xx[::2, ::2] + i) / 91.0)
        v = 128.0 + 20.0 * np.cos((yy[::2, ::2] - i) / 77.0)
        records.append(b"FRAME\n" + b"".join(p.round().clip(16, 235).astype(np.uint8).tobytes() for p in (y, u, v)))
    return f"YUV4MPEG2 W{W} H{H} F25:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n".encode(), records


def run_once(head: bytes, records: list, stream: bool, timeout: float) -> dict:
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", str(int(timeout)), sys.executable, "-m", "speinet_amd.video", "--input", "-", "--output", "-",
           "--model_path", "synthetic", "--precision", "f16"] + (["--stream"] if stream else [])
    child = subprocess.Popen(cmd, cwd=ROOT, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    record = len(records[0])
    t = {}

    def feed():
        try:
            t["first_in"] = time.perf_counter()
            child.stdin.write(head)
            for r in records:
                child.stdin.write(r)
            child.stdin.close()
            t["last_in"] = time.perf_counter()
        except BrokenPipeError:
            pass

    log = []
    threads = [threading.Thread(target=feed, daemon=True), threading.Thread(target=lambda: log.append(child.stderr.read()), daemon=True)]
    for th in threads:
        th.start()
    child.stdout.readline()
    got = frames = 0
    while True:
        more = child.stdout.read(min(record - got, 1 << 20))
        if not more:
            break
        got += len(more)
        if got == record:
            frames, got = frames + 1, 0
            t.setdefault("first_out", time.perf_counter())
    _, status, usage = os.wait4(child.pid, 0)
    t["exit"] = time.perf_counter()
    child.returncode = os.waitstatus_to_exitcode(status)
    for th in threads:
        th.join(10)
    text = (log[0] if log else b"").decode(errors="replace")
    return {"mode": "streamed" if stream else "spooled", "exit": child.returncode, "frames_out": frames,
            "total_s": t["exit"] - t["first_in"], "first_frame_s": t.get("first_out", float("nan")) - t["first_in"],
            "input_taken_s": t.get("last_in", float("nan")) - t["first_in"], "peak_rss_MiB": usage.ru_maxrss / 1024.0,
            "log_tail": text.strip().splitlines()[-1:] if child.returncode == 0 else text.strip().splitlines()[-15:]}


def main() -> None:
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_bench.json"))
    p.add_argument("--pairs", type=int, default=3)
    p.add_argument("--frames", type=int, default=120)
    p.add_argument("--timeout", type=float, default=240.0, help="time limit of one child, in seconds")
    a = p.parse_args()
    head, records = clip_bytes(a.frames)
    runs, ok = [], True
    for pair in range(a.pairs):
        for stream in (False, True) if pair % 2 == 0 else (True, False):     # alternating, and the order within a pair too
            r = run_once(head, records, stream, a.timeout)
            runs.append(dict(r, pair=pair))
            print(json.dumps({k: v for k, v in runs[-1].items() if k != "log_tail"}), flush=True)
            ok = r["exit"] == 0 and r["frames_out"] == a.frames
            if not ok:
                break
        if not ok:
            break
    result = {"method": __doc__.split("\n\n")[1].replace("\n", " "), "frames": a.frames, "size": [H, W], "pairs": a.pairs, "runs": runs,
              "complete": ok}
    if ok:
        by = {m: [r for r in runs if r["mode"] == m] for m in ("spooled", "streamed")}
        med = {m: {k: statistics.median(r[k] for r in rs) for k in ("total_s", "first_frame_s", "peak_rss_MiB")} for m, rs in by.items()}
        spooled = [r["total_s"] for r in by["spooled"]]
        allowance = max(max(spooled) - min(spooled), 0.05 * med["spooled"]["total_s"])
        result.update(medians=med, spooled_spread_s=max(spooled) - min(spooled), allowance_s=allowance,
                      streamed_minus_spooled_s=med["streamed"]["total_s"] - med["spooled"]["total_s"],
                      within_bar=med["streamed"]["total_s"] <= med["spooled"]["total_s"] + allowance)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k not in ("runs", "method")}), flush=True)
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
