#!/usr/bin/env python3
"""Training-step throughput per GEMM arithmetic (`model.train_precision`), one GPU, bench.py --train's protocol: the same synthetic
crops (seed 7 / 8, 3 frames for swint; the full model with every 4th crop reference-less), 1*L1 + 2*HEM, Adam 1e-4, warm-up steps,
HIP-event timing of forward / loss + backward / Adam.  Prints ONE JSON line.

    python tools/train_precision_bench.py --precision f32|bf16x3|bf16 [--model swint|speinet] [--batch 8] [--patch 200]
                                          [--steps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DTYPE = {"f32": "f32 (v_mfma_f32_32x32x2_f32)",
         "bf16x3": "bf16x3: split products on the 16-bit matrix pipe (2^-16 per product) for the forward, stride-1 data-gradient and "
                   "weight-gradient GEMMs",
         "bf16": "bf16: every GEMM (convs, transposed convs, linears, window attention; forward and backward) in single bf16 products, "
                 "fp32 accumulation"}


def main(argv=None):
    ap = argparse.ArgumentParser(prog="train_precision_bench.py")
    ap.add_argument("--precision", choices=["f32", "bf16x3", "bf16"], required=True)
    ap.add_argument("--model", choices=["swint", "speinet"], default="swint")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--patch", type=int, default=200)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from speinet_amd.loss import Loss
    from speinet_amd.speinet import default_args
    from speinet_amd.synth import synth_frames, synth_state_dict
    dev = "cuda:0"
    torch.cuda.set_device(0)
    args = default_args()
    args.n_sequence = 3
    if a.model == "speinet":
        from speinet_amd.speinet import SPEINet
        net = SPEINet(args=args)
        x = synth_frames(a.batch, a.patch, a.patch, seed=7, zero_ref=tuple(range(3, a.batch, 4))).contiguous().to(dev)
    else:
        from speinet_amd.swint import SPEINet
        net = SPEINet(n_sequence=3, args=args)
        x = synth_frames(a.batch, a.patch, a.patch, seed=7)[:, :3].contiguous().to(dev)
    net.load_state_dict(synth_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.to(dev).train()
    net.train_precision = a.precision
    gt = synth_frames(a.batch, a.patch, a.patch, seed=8)[:, 1].contiguous().to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, weight_decay=0.0)
    loss_fn = Loss("1*L1+2*HEM", device=dev)
    torch.manual_seed(0)
    np.random.seed(0)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    split = np.zeros(3)
    for it in range(a.warmup + a.steps):
        e = [ev() for _ in range(4)]
        e[0].record()
        out = net(x)
        e[1].record()
        opt.zero_grad()
        loss = loss_fn(out, gt)
        loss.backward()
        e[2].record()
        opt.step()
        e[3].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            split += [e[i].elapsed_time(e[i + 1]) for i in range(3)]
    split /= a.steps
    ms = float(split.sum())
    print(json.dumps({"metric": f"training crops/s, {a.model} model, fwd + loss + bwd + Adam", "value": a.batch * 1e3 / ms, "unit": "crops/s",
                      "precision": a.precision, "dtype": DTYPE[a.precision], "batch": a.batch, "patch": a.patch, "n_sequence": 3,
                      "steps": a.steps, "warmup": a.warmup, "ms_per_step": ms,
                      "ms": {"forward": float(split[0]), "loss_backward": float(split[1]), "adam": float(split[2])},
                      "loss": float(loss.item()), "data": "synthetic"}))


if __name__ == "__main__":
    main()
