#!/usr/bin/env python3
"""Does feeding the training step from the dataset loader cost anything?  One process, one model, the same batch size and step count
three times:

    fixed_a, fixed_b   Trainer.step on ONE fixed device batch (what `bench.py --train` times), run twice: their difference is the
                       run-to-run spread
    loader             Trainer.step on the batches of speinet_amd.data.TrainLoader over a synthetic clip set resident on the device
                       (spei_train_batch_u8 builds batch k + 1 on a side stream while step k runs)

The fixed batch is the loader's first batch, so all legs see the same kind of content; for the full model the share of samples routed
to the no-reference branch is printed per leg (it changes the work of a step).  Wall-clock per step, device synchronised at both ends
of a leg.  Prints one JSON line.

    python tools/train_loader_bench.py [--model swint|speinet] [--batch 20] [--patch 200] [--precision bf16] [--steps 10] [--warmup 3]
                                       [--residency device|host] [--out file.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synth_tree(root: str, clips: int, frames: int, h: int, w: int, seed: int = 0) -> None:
    """blur / gt / label folders of smooth moving content with noise; every 6th frame labelled sharp, and a gap in clip 0's numbering."""
    from PIL import Image
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    for c in range(clips):
        name = f"{c:03d}"
        for kind in ("blur", "gt"):
            os.makedirs(os.path.join(root, kind, name))
        os.makedirs(os.path.join(root, "label"), exist_ok=True)
        for t in range(frames):
            base = np.stack([127 + 100 * np.sin((x + 3 * t + 40 * k) / (17.0 + c)) * np.cos((y - 2 * t) / (23.0 + k)) for k in range(3)], -1)
            num = t if (c or t < frames // 2) else t + 30
            for kind, noise in (("blur", 2.0), ("gt", 6.0)):
                img = np.clip(base + noise * rs.randn(h, w, 3), 0, 255).astype(np.uint8)
                Image.fromarray(img).save(os.path.join(root, kind, name, f"{num:08d}.png"), compress_level=1)
        np.save(os.path.join(root, "label", name + ".npy"), (np.arange(frames) % 6 == 2).astype(np.int64))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="swint", choices=("swint", "speinet"))
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--patch", type=int, default=200)
    ap.add_argument("--precision", default="bf16", choices=("f32", "bf16x3", "bf16"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--residency", default="device", choices=("device", "host"))
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--size", default="360x480")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from speinet_amd.data import ClipSet, ClipStore, TrainLoader
    from speinet_amd.fit import build_model
    from speinet_amd.loss import Loss
    from speinet_amd.trainer import Trainer
    dev = "cuda:0"
    h, w = (int(v) for v in a.size.split("x"))
    refs = a.model == "speinet"
    with tempfile.TemporaryDirectory() as root:
        synth_tree(root, a.clips, a.frames, h, w)
        cs = ClipSet(root, True, references=refs, patch=a.patch)
        store = ClipStore(cs, residency=a.residency, device=dev)
    net = build_model(a.model, dev, train_precision=a.precision, synthetic_seed=0)
    tr = Trainer(net, Loss("1*L1+2*HEM", device=dev), lr=1e-4)
    torch.manual_seed(0)
    np.random.seed(0)

    def zero_share(inp) -> float:
        return float((inp[:, 3].reshape(inp.shape[0], -1) == 0).all(dim=1).float().mean()) if refs else 0.0

    def batches():
        loader = TrainLoader(cs, store, a.batch, a.patch, seed=1)
        while True:
            for b in loader:
                if b[0].shape[0] == a.batch:             # full batches only: every step of every leg does the same amount of work
                    yield b

    first = next(batches())
    fixed = (first[0].clone(), first[1].clone())

    def leg(source) -> dict:
        share = []
        for _ in range(a.warmup):
            tr.step(*next(source))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            inp, gt = next(source)
            share.append(zero_share(inp))
            tr.step(inp, gt)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        return {"ms_per_step": round(ms, 3), "crops_per_s": round(a.batch / ms * 1e3, 2), "no_reference_share": round(float(np.mean(share)), 3)}

    def fixed_source():
        while True:
            yield fixed

    res = {"tool": "train_loader_bench", "model": a.model, "batch": a.batch, "patch": a.patch, "train_precision": a.precision,
           "steps": a.steps, "warmup": a.warmup, "residency": a.residency, "clip_set_bytes": store.nbytes,
           "clip_set": f"{a.clips} clips x {a.frames} frames of {w}x{h}", "device": torch.cuda.get_device_name(0)}
    res["fixed_a"] = leg(fixed_source())
    res["loader"] = leg(batches())
    res["fixed_b"] = leg(fixed_source())
    lo, hi = sorted((res["fixed_a"]["ms_per_step"], res["fixed_b"]["ms_per_step"]))
    res["loader_within_fixed_spread"] = bool(lo <= res["loader"]["ms_per_step"] <= hi)
    res["loader_vs_fixed_mean"] = round(res["loader"]["ms_per_step"] / ((lo + hi) / 2), 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
