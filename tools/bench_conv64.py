#!/usr/bin/env python3
"""The 64 -> 64 channel 5x5 layer at the half-resolution level of a 720p frame (360 x 640; the ResBlock convs of the second encoder /
decoder stage): weight-stationary kernel (csrc/conv64_ws16.hip) against the slab kernel, 1 and 7 stacked maps, fp32 and 16-bit input,
f16 and bf16.  PREC=f16|bf16 restricts the run to one format."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speinet_amd import pack                         # noqa: E402
from speinet_amd.ops import BMap, Ctx                # noqa: E402

H, W = 360, 640
dev = "cuda:0"
pw = pack.PackedW(torch.randn(25, 64, 64) * 0.02, dev)
b = torch.randn(64, device=dev) * 0.1


def timeit(name, fn, flops, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / n * 1e3
    print(f"{name:52s} {us:8.1f} us  {flops / us / 1e6:7.1f} TFLOP/s", flush=True)


for prec in ([os.environ["PREC"]] if os.environ.get("PREC") else ["f16", "bf16"]):
    ws, slab = Ctx(prec, device=dev), Ctx(prec, device=dev, conv64_ws=False)
    LP = torch.float16 if prec == "f16" else torch.bfloat16
    for maps in (1, 7):
        for in16 in (False, True):
            x = torch.randn(maps * H * W, 64, device=dev)
            x = x.to(LP) if in16 else x
            bm = BMap(x, maps, H, W, 64)
            fl = 2.0 * 25 * 64 * 64 * H * W * maps
            for name, c in (("weight-stationary", ws), ("slab", slab)):
                timeit(f"{prec} {name}, {maps} map(s), {'16-bit' if in16 else 'fp32'} in, 16-bit out",
                       lambda: c.igemm_batched(bm, pw, b, 64, 5, act=1, out_dtype=LP), fl)
