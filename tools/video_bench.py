#!/usr/bin/env python3
"""deblur_clip (speinet_amd/video.py) against the harness on the same synthetic clip on disk, in one process: one JSON line.

    python tools/video_bench.py [frames] [precision]

harness: `inference.harness_throughput` (PNG decode -> ... -> PSNR / SSIM -> PNG encode).  video: `deblur_clip` on the clip's label
file with the frames given as PNG paths (decoded on worker threads) and as a host uint8 array, outputs kept on the device.  Each
video figure is the second of two passes (the first captures the graphs), as the harness's is."""
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                     # noqa: E402
import torch                                           # noqa: E402

from speinet_amd import inference, video               # noqa: E402


def timed(net, frames, labels) -> float:
    for _ in video.deblur_clip(net, frames, labels):   # graph capture, page cache
        pass
    torch.cuda.synchronize()
    t0 = time.time()
    n = sum(1 for _ in video.deblur_clip(net, frames, labels))
    torch.cuda.synchronize()
    return n / (time.time() - t0)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    prec = sys.argv[2] if len(sys.argv) > 2 else "f16"
    line = {"harness_throughput": inference.harness_throughput(n, prec)["value"]}
    root = tempfile.mkdtemp(prefix="speinet_video_")
    try:
        data = inference.synth_clip(root, n, 720, 1280)
        paths = sorted(os.path.join(data, "blur", "clip0", f) for f in os.listdir(os.path.join(data, "blur", "clip0")))
        labels = np.load(os.path.join(data, "label", "clip0.npy"))
        net = video.load_model("synthetic", "cuda", prec)
        line["video_paths"] = timed(net, paths, labels)
        line["video_host_array"] = timed(net, np.stack([inference._imread(p) for p in paths]), labels)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line.update({"unit": "frames/s", "frames": n, "precision": prec,
                 "what": "deblur_clip vs the harness on a synthetic 1280x720 clip, label file given, outputs of deblur_clip kept on the device"})
    print(json.dumps(line))


if __name__ == "__main__":
    main()
