#!/usr/bin/env python3
"""Headline benchmark: deblurred 720p frames/s of the SPEINet per-sequence forward pass on MI355X.

  python bench.py --gpus N --steps K --warmup W
  (N > 1: one rank per GPU over RCCL.  Either the caller starts the ranks — `python -m torch.distributed.run --nproc-per-node N ...
  bench.py --gpus N ...`, as the driver does — or, with no RANK in the environment, bench.py starts them itself as child processes
  of a parent that never touches the GPU (speinet_amd.dist.launch_ranks) and passes rank 0's line through.  --gpus must equal the
  RCCL world size; a node with fewer GPUs than ranks is an error, never a 1-GPU line.)

A "step" is one forward of one synthetic [1,5,3,720,1280] window (BASELINE.json configs[1]) per rank, inputs already
resident in HBM.  Frames are independent, so ranks shard by frame with NO data-path collective (weak scaling);
RCCL carries only the barrier, the max-over-ranks time and an all-gather of per-rank output checksums.

Default arithmetic: `--precision f16 --corr-precision top2` — half operands on the 16-bit matrix pipe (the rate of the bf16
pipe BASELINE.json names, 11-bit instead of 8-bit significands) with the exact re-scored arg-max: the configuration whose
output stays within 1e-3 dB PSNR of the reference (tests/test_gpu_bf16.py asserts it against the reference's own 720p
outputs).  `--precision bf16` is configs[1] to the letter (3e-3 dB).

A plain run sets up, warms up, times the K steps, dumps the outputs if asked and prints its line: everything in it comes from
the timed region itself.  `--full` adds every measurement that needs runs of its own (marked [full] below; each still obeys its
--no-* / --cpu-baseline option): `reference_call`, `roofline.families`, `bf16_letter`, `f32_grade`, `harness`, `train` and
`cpu_baseline`, about a minute and a half more.

Rank 0 prints ONE JSON line.  Besides the contract fields it carries
  value / ms_per_step   wall clock of K timed steps (barrier + synchronize on both sides, MAX over ranks); the timed call
                 passes `routing=` (the caller knows whether frame 3 is zero; no host sync).  [full] `reference_call` times the same
                 K steps as the reference calls it, `forward(x)`: the routing test runs on the device and syncs once per call.
  step_ms        median / p10 / p90 of the K per-step GPU durations (HIP events on the launch stream; with K <= --inflight no
                 same-stream pair exists and it holds the wall-clock ms_per_step alone)
  --dump-outputs DIR   writes what the LAST timed step returned to its caller (rank 0: the [B,3,H,W] frames) as DIR/output.npy,
                 float32, at most 64 MB (a fixed seed-0 sample of flat indices beyond that, DIR/output_index.npy); the inputs are
                 seeded, so two builds run with the same arguments can be compared output for output
  roofline       the largest kernel (fused correlation arg-max, 37 % of the path's algorithmic FLOPs, one launch per frame):
                 FLOPs per launch / its average duration (`achieved`: the flops the dispatched kernel EXECUTES — the diagonal-sliding
                 kernel of round 3 computes each row-against-row term once, a third of the bmm's count, so the algorithmic count /
                 time (`algorithmic_equivalent_tflops`) exceeds the MFMA peak and is not a utilisation), measured LIVE in the timed region: a frame replays as
                 two hipGraph segments with that kernel launched directly between them, bracketed by HIP events on the launch
                 stream (`kernel` = the dispatch actually taken).  Peak = dense MFMA peak of the operand type
                 (MI355X_MICROARCH.md: 2500 TFLOP/s for bf16 / f16, 157.3 TFLOP/s f32).  `path_frac` prices the WHOLE frame
                 (F = 20.64 TFLOP) against the same peak.  `traffic` / `path_hbm_bytes_per_frame`: HBM bytes from
                 rocprofv3 PMC passes made OFFLINE with tools/pmc_traffic.py (FETCH_SIZE doubled as the guide prescribes for
                 wide coalesced reads on gfx950) and read from profiles/ — `traffic_source` names the file, null if absent.
                 [full] `families`: kernel time per family from 3 eager single-stream frames after the timed region; the
                 top-level fields then describe the family with the most kernel time (null in a plain run).
  --train        a second measurement, BASELINE.json configs[4] (trainer/trainer_swint.py on 200x200 crops, option/template.py:6-22):
                 `python bench.py --train [--model swint|speinet] [--batch 20] [--steps 5] [--warmup 2] [--cpu-baseline]` prints ONE
                 JSON line of its own — training crops/s (forward in train() mode, 1*L1+2*HEM, backward, Adam; N ranks under
                 torch.distributed.run average gradients over RCCL, weak scaling), the per-phase split by HIP events, and with
                 --cpu-baseline the oracle's train-mode graph under torch autograd on the host cores (2 crops)
  harness        [full] (N = 1, unless --no-harness) end-to-end frames/s of the inference harness (speinet_amd.inference, the counterpart of
                 inference_SPEINet.py) on a synthetic 720p clip ON DISK: PNG decode, selection, upload, forward with cross-window
                 encoder reuse, uint8, PSNR / SSIM, PNG encode — what a user of the reference's script gets per frame.
  cpu_baseline   [full] the oracle (CPU restatement of the reference, PyTorch fp32) timed on this host's cores, rank 0, N = 1: one untimed
                 and two timed 360x640 frames (threads, allocator, oneDNN primitives warm), then ONE 720p frame (the value).  Threads =
                 the physical cores of one socket, capped by the CPUs the process may use (affinity / cgroup quota); both numbers are
                 in the record.  If the probe predicts more than --cpu-budget seconds for the 720p frame the probe itself is
                 reported, scaled by the FLOP formula of BASELINE.md §2 and labelled "extrapolated".
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

H, W = 720, 1280
# /opt/skills/guides/MI355X_MICROARCH.md, chip-level parameters: dense matrix peaks (never the 2:1-sparsity figures)
PEAK_TFLOPS = {"f32": 157.3, "bf16": 2500.0, "bf16x3": 2500.0, "f16": 2500.0}
HBM_PEAK_GBS = 8000.0           # MI355X_MICROARCH.md: HBM3E ~8 TB/s
TRAFFIC_FILES = ("r04_traffic.json", "r03_traffic.json", "r02_traffic.json", "r01_traffic.json")


def path_flops(h: int, w: int) -> float:
    """F(HW) = 1.410e7*HW + 2304*(HW/16)^2  (`_forwardbs`, reference formulation)."""
    hw = h * w
    return 1.410e7 * hw + 2304.0 * (hw / 16.0) ** 2


def corr_flops(h: int, w: int) -> float:
    n3 = (h // 4) * (w // 4)
    return 2.0 * 1152.0 * n3 * n3     # [N3 x 1152] x [1152 x N3]


def traffic_bytes(precision: str, corr_precision: str):
    """(kernel bytes per launch, path bytes per frame, source file) from the newest offline PMC summary under profiles/."""
    for name in TRAFFIC_FILES:
        try:
            d = json.load(open(os.path.join(ROOT, "profiles", name)))
        except (OSError, ValueError):
            continue
        e = d.get(f"{precision}/{corr_precision if precision != 'f32' else 'f32'}")
        if e:
            return (e.get("hbm_bytes_per_launch"), e.get("path_hbm_bytes_per_frame"), f"profiles/{name} (offline rocprofv3 --pmc, {d.get('commit', 'n/a')})",
                    e.get("families_hbm_bytes_per_frame") or {})
    return None, None, None, {}


def physical_cores() -> int:
    """Physical cores visible to this process (unique (physical id, core id) pairs of /proc/cpuinfo; falls back to os.cpu_count())."""
    try:
        ids, cur = set(), {}
        for line in open("/proc/cpuinfo"):
            if ":" in line:
                k, v = (t.strip() for t in line.split(":", 1))
                cur[k] = v
            elif cur:
                ids.add((cur.get("physical id", "0"), cur.get("core id", cur.get("processor", "0"))))
                cur = {}
        if cur:
            ids.add((cur.get("physical id", "0"), cur.get("core id", cur.get("processor", "0"))))
        return max(1, len(ids))
    except OSError:
        return os.cpu_count() or 1


def socket_cores() -> int:
    """Physical cores of ONE socket (unique core ids under the first `physical id` of /proc/cpuinfo)."""
    try:
        per, cur = {}, {}
        for line in list(open("/proc/cpuinfo")) + ["\n"]:
            if ":" in line:
                k, v = (t.strip() for t in line.split(":", 1))
                cur[k] = v
            elif cur:
                per.setdefault(cur.get("physical id", "0"), set()).add(cur.get("core id", cur.get("processor", "0")))
                cur = {}
        return max(1, len(per[sorted(per)[0]])) if per else (os.cpu_count() or 1)
    except OSError:
        return os.cpu_count() or 1


def usable_cpus() -> int:
    """CPUs this process may run on: its affinity mask, capped by the cgroup CPU quota (cpu.max, v2; cpu.cfs_quota_us, v1)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(int(q) / int(per))))
    except (OSError, ValueError):
        try:
            q, per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read()), int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // per))
        except (OSError, ValueError):
            pass
    return n


def cpu_baseline(seed: int, mode: str, budget_s: float) -> dict:
    """The oracle (CPU restatement of the reference, PyTorch fp32) on this host: one untimed warm-up + two timed frames at 360x640
    (threads, allocator and oneDNN primitives warm; their spread is reported), then ONE timed frame at the bench size 1280x720 — the
    headline — unless the probe predicts it would exceed `budget_s`."""
    from oracle import speinet_oracle as O
    from speinet_amd.synth import state_dict_template, synth_frames, synth_state_dict
    phys, logical = physical_cores(), os.cpu_count() or 1
    socket, usable = socket_cores(), usable_cpus()
    # the physical cores of ONE socket — capped by what this process may actually use (CPU affinity / cgroup quota: a
    # 1-GPU box of the pool shares its host; more threads than usable CPUs time-slice and measure the scheduler)
    threads = max(1, min(socket, usable))
    torch.set_num_threads(threads)
    sd = synth_state_dict(state_dict_template(), seed=0)

    def run(h, w):
        x = synth_frames(1, h, w, seed=seed)
        with torch.no_grad():
            t0 = time.time()
            O.forward(x, sd, O.Cfg())
            return time.time() - t0

    sh, sw = 360, 640
    run(sh, sw)                                                 # warm-up, untimed
    probes = [run(sh, sw) for _ in range(2)]
    dt = min(probes)
    scale = path_flops(H, W) / path_flops(sh, sw)
    host = (f"{threads} threads = min(physical cores of one socket {socket}, CPUs this process may use {usable}); {phys} physical / {logical} "
            "logical cores visible")
    if mode == "720p" and dt * scale * 2.5 <= budget_s:       # measured: the quadratic term makes 720p ~2x the FLOP-scaled probe
        dt720 = run(H, W)
        return {"value": 1.0 / dt720, "unit": "frames/s", "cores": threads, "physical_cores": phys, "socket_physical_cores": socket,
                "usable_cpus": usable, "kind": "port",
                "sample": f"oracle (PyTorch fp32 CPU restatement), {host}: ONE {W}x{H} _forwardbs frame in {dt720:.1f} s after a warm-up "
                          f"and two timed {sw}x{sh} frames ({probes[0]:.2f} s, {probes[1]:.2f} s)"}
    return {"value": 1.0 / (dt * scale), "unit": "frames/s", "cores": threads, "physical_cores": phys, "socket_physical_cores": socket,
            "usable_cpus": usable, "kind": "port",
            "sample": f"EXTRAPOLATED: oracle, {host}: best of two timed {sw}x{sh} _forwardbs frames after a warm-up ({probes[0]:.2f} s, "
                      f"{probes[1]:.2f} s), scaled x{scale:.2f} to 720p by F(HW) of BASELINE.md (optimistic: the 57600^2 correlation does "
                      "not scale like FLOPs)"}


def conv_sub_records(conv_sub: dict, n_frames: int, conv_flops: float, peak: float) -> dict:
    """The conv family by what bounds it: `level1` = the 32-channel 5x5 layers at full resolution (+ the first / last conv), priced against
    HBM on the activation bytes they must move (input + output of every launch, weights excluded); `rest` = every other conv (64 / 128 /
    256 channels, 1x1 and 3x3 glue, stride-2 and transposed convs), priced against the matrix pipe on the family's remaining flops."""
    out = {}
    if not conv_sub or not n_frames:
        return out
    l1 = conv_sub.get("level1")
    if l1 and l1["events"]:
        ms = sum(s_.elapsed_time(e_) for s_, e_ in l1["events"]) / n_frames
        by, fl = l1["bytes"] / n_frames, l1["flops"] / n_frames
        out["level1"] = {"ms_per_frame": ms, "launches_per_frame": len(l1["events"]) / n_frames, "bound": "hbm",
                         "algorithmic_bytes_per_frame": by, "algorithmic_flops_per_frame": fl, "achieved": by / (ms * 1e-3) / 1e9,
                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         "mfma_frac": fl / (ms * 1e-3) / 1e12 / peak}
    rest = conv_sub.get("rest")
    if rest and rest["events"]:
        ms = sum(s_.elapsed_time(e_) for s_, e_ in rest["events"]) / n_frames
        fl = conv_flops - (l1["flops"] / n_frames if l1 else 0.0)
        out["rest"] = {"ms_per_frame": ms, "launches_per_frame": len(rest["events"]) / n_frames, "bound": "mfma",
                       "algorithmic_flops_per_frame": fl, "achieved": fl / (ms * 1e-3) / 1e12, "peak": peak, "unit": "TFLOP/s",
                       "frac": fl / (ms * 1e-3) / 1e12 / peak}
    return out


def family_records(fam_events: dict, n_frames: int, h: int, w: int, has_ref: bool, peak: float, fam_hbm: dict, diag: bool) -> dict:
    """Per kernel family: kernel ms per frame (HIP events around every launch, exclusive), launches, the ALGORITHMIC work per frame
    (conv 8.536 T, Swin linears + attention 4.455 T — both linear in H W —, correlation 2 x 1152 x (HW/16)^2; the
    streaming family = ResBlock gate statistics + gated sums: one read of x1 for the statistics, x + x1 read and x' written by the
    apply pass: 12 B per element of each of the frame's 72 (66 without a sharp reference) ResBlock maps) and what that makes of the
    roofline that bounds it."""
    if not n_frames:
        return {}
    hw = h * w
    scale = hw / float(H * W)
    blocks_per_level = (7 if has_ref else 6) * 3 + 3                  # encoder passes x 3 ResBlocks + the decoder's 3, per level
    work = {"conv": ("mfma", 8.536e12 * scale, "conv_slab / igemm / conv5 (every Conv2d, ConvTranspose2d; Swin's 3x3 convs)"),
            "swin": ("mfma", 4.455e12 * scale, "attn_pipe + mlp_pipe, both Swin calls of a frame per launch (72 Swin blocks: LayerNorm, q/kv/proj, W-MSA, MLP)"),
            "correlation": ("mfma", corr_flops(h, w), "corr_diag / corr_slab + reduce + re-score (SearchTransfer's bmm + max)"),
            "streaming": ("hbm", blocks_per_level * 56.0 * hw * 12.0, "gate_stats / gate_maps / resblock_apply (SE + triplet gates, gated residual sum)")}
    out = {}
    for fam, (bound, alg, kernels) in work.items():
        ev = fam_events.get(fam, [])
        if not ev:
            continue
        ms = sum(s_.elapsed_time(e_) for s_, e_ in ev) / n_frames
        rec = {"ms_per_frame": ms, "launches_per_frame": len(ev) / n_frames, "kernels": kernels, "bound": bound,
               "hbm_bytes_per_frame": fam_hbm.get(fam)}
        if bound == "mfma":
            rec.update(algorithmic_flops_per_frame=alg, achieved=alg / (ms * 1e-3) / 1e12, peak=peak, unit="TFLOP/s")
            if fam == "correlation" and diag:
                rec.update(executed_flops_per_frame=alg / 3.0, executed_tflops=alg / 3.0 / (ms * 1e-3) / 1e12,
                           note="the diagonal kernel executes a third of the bmm's flops (each row-against-row term once): frac prices the "
                                "algorithmic count and can exceed 1; executed_tflops / peak is the matrix-pipe utilisation")
        else:
            rec.update(algorithmic_bytes_per_frame=alg, achieved=alg / (ms * 1e-3) / 1e9, peak=8000.0, unit="GB/s")
        rec["frac"] = rec["achieved"] / rec["peak"]
        out[fam] = rec
    return out


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir: str, arrays: dict) -> dict:
    """Write each tensor as out_dir/<name>.npy in float32.  Over DUMP_LIMIT_BYTES in all, each keeps a fixed sample instead: flat
    indices drawn by a generator of seed 0, sorted and saved beside it as <name>_index.npy (int64), the same for every run of a shape."""
    os.makedirs(out_dir, exist_ok=True)
    total = sum(4 * t.numel() for t in arrays.values())
    sampled = total > DUMP_LIMIT_BYTES
    shapes = {}
    for name, t in arrays.items():
        a = t.detach().float().cpu()
        if sampled:
            keep = max(1, t.numel() * DUMP_LIMIT_BYTES // (3 * total))       # 4-byte values + 8-byte indices stay under the limit
            idx = torch.randperm(t.numel(), generator=torch.Generator().manual_seed(0))[:keep].sort().values
            a = a.reshape(-1)[idx]
            np.save(os.path.join(out_dir, name + "_index.npy"), idx.numpy())
        np.save(os.path.join(out_dir, name + ".npy"), a.numpy())
        shapes[name] = list(t.shape)
    return {"dir": out_dir, "shapes": shapes, "sampled": sampled}


def train_main(argv=None):
    """`bench.py --train ...`: training-step throughput (config 5), see the module docstring."""
    line = train_measure(argv)
    if line is not None:
        print(json.dumps(line))


def train_measure(argv=None):
    ap = argparse.ArgumentParser(prog="bench.py --train")
    ap.add_argument("--gpus", type=int, default=1, help="ranks (one per GPU, gradients averaged over RCCL); > 1 without RANK in the env: starts them")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--patch", type=int, default=200)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-baseline", action="store_true",
                    help="also time one training step of the oracle (CPU restatement, fp32, torch autograd) on the host cores: 2 crops")
    ap.add_argument("--precision", choices=["f32", "bf16x3"], default="bf16x3",
                    help="forward / data-gradient GEMMs of the step: bf16x3 = split products on the 16-bit matrix pipe (finer than the TF32 / "
                         "bf16 matmuls the reference trains with, main_SPEINet.py:12); f32 = the form G20-G22 pin to 1e-6")
    ap.add_argument("--model", choices=["swint", "speinet"], default="swint",
                    help="swint: model/swint.py (trainer_swint.py, config 5); speinet: model/speinet.py (trainer_swint_hsa_nsf.py), every "
                         "4th crop without a sharp reference")
    a = ap.parse_args(argv)
    if "RANK" not in os.environ and a.gpus > 1:
        from speinet_amd.dist import launch_ranks
        sys.exit(launch_ranks(os.path.abspath(__file__), ["--train", *(argv if argv is not None else sys.argv[1:])], a.gpus))
    if a.gpus != int(os.environ.get("WORLD_SIZE", "1")):
        raise SystemExit(f"bench.py --train: --gpus {a.gpus} but WORLD_SIZE={os.environ.get('WORLD_SIZE', '1')}")
    import numpy as np
    from speinet_amd.loss import Loss
    from speinet_amd.speinet import default_args
    from speinet_amd.swint import SPEINet
    from speinet_amd.synth import synth_frames, synth_state_dict
    from speinet_amd.trainer import allreduce_gradients, broadcast_buffers
    rank, world, local = (int(os.environ.get(k, d)) for k, d in (("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0")))
    dev = f"cuda:{local}"
    torch.cuda.set_device(local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", rank=rank, world_size=world)
    args = default_args()
    args.n_sequence = 3
    if a.model == "speinet":
        from speinet_amd.speinet import SPEINet as FullNet
        net = FullNet(args=args)
    else:
        net = SPEINet(n_sequence=3, args=args)
    net.load_state_dict(synth_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.to(dev).train()
    net.train_precision = a.precision
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, weight_decay=0.0)
    loss_fn = Loss("1*L1+2*HEM", device=dev)
    if a.model == "speinet":
        x = synth_frames(a.batch, a.patch, a.patch, seed=7 + 2 * rank, zero_ref=tuple(range(3, a.batch, 4))).contiguous().to(dev)
    else:
        x = synth_frames(a.batch, a.patch, a.patch, seed=7 + 2 * rank)[:, :3].contiguous().to(dev)
    gt = synth_frames(a.batch, a.patch, a.patch, seed=8 + 2 * rank)[:, 1].contiguous().to(dev)
    torch.manual_seed(rank)
    np.random.seed(rank)
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
        allreduce_gradients(net.parameters())
        e[2].record()
        opt.step()
        broadcast_buffers(net)
        e[3].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            split += [e[i].elapsed_time(e[i + 1]) for i in range(3)]
    split /= a.steps
    ms = float(split.sum())
    if dist is not None:
        t = torch.tensor([ms], device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        ms = float(t.item())
    cpu = None
    if rank == 0 and a.cpu_baseline:
        # the checker as a baseline: the oracle's train-mode graph + torch autograd on the host, fp32, a bounded sample
        import time
        from oracle import speinet_oracle as O
        from speinet_amd.train import drop_path_scales, speinet_drop_path_scales
        threads = min(os.cpu_count() or 1, 16)
        torch.set_num_threads(threads)
        nb = 2
        xs, gs = x[:nb].cpu(), gt[:nb].cpu()
        sd = {k: (v.detach().cpu().clone().requires_grad_(True) if v.is_floating_point() and "running_" not in k else v.detach().cpu())
              for k, v in net.state_dict().items()}
        if a.model == "speinet":
            sc = speinet_drop_path_scales(net.cfg.depths, [bool(v) for v in (xs[:, 3].reshape(nb, -1) == 0).all(dim=1).tolist()], 3)
            calls = sc.get(False, []) + sc.get(True, [])
        else:
            calls = drop_path_scales(net.cfg.depths, nb, 2)
        t0 = time.time()
        with O.train_mode(calls):
            o = (O.forward if a.model == "speinet" else O.forward_swint)(xs, sd, O.Cfg(n_sequence=3))
        Loss("1*L1+2*HEM", device="cpu")(o, gs).backward()
        dt = time.time() - t0
        cpu = {"value": nb / dt, "unit": "crops/s", "cores": threads, "kind": "port",
               "sample": f"oracle train-mode graph + torch autograd (fp32), forward + loss + backward of {nb} crops of {a.patch}x{a.patch} in {dt:.1f} s, no optimizer step"}
    line = None
    if rank == 0:
        line = {"metric": f"training crops/s, {a.model} model, fwd + loss + bwd + Adam", "value": world * a.batch * 1e3 / ms,
                "unit": "crops/s", "n_gpus": world, "batch_per_gpu": a.batch, "patch": a.patch, "n_sequence": 3, "ms_per_step": ms,
                "ms": {"forward": float(split[0]), "loss_backward": float(split[1]), "adam": float(split[2])},
                "loss": float(loss.item()), "dtype": "f32" if a.precision == "f32" else "bf16x3 (split products on the 16-bit matrix pipe, f32-grade): forward, data-gradient and weight-gradient GEMMs; everything else fp32",
                "data": "synthetic", "scaling": "weak", "cpu_baseline": cpu}
    if dist is not None:
        dist.destroy_process_group()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run every other measurement (reference_call, per-family kernel times, bf16 to the "
                         "letter, f32-grade, harness, training step, CPU baseline), each unless its own option below skips it")
    ap.add_argument("--cpu-baseline", choices=["720p", "sample", "none"], default="720p")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="same as --cpu-baseline none")
    ap.add_argument("--cpu-budget", type=float, default=240.0, help="seconds the 720p oracle frame may take (else: extrapolated probe)")
    ap.add_argument("--precision", choices=["f32", "bf16x3", "bf16", "f16"], default="f16",
                    help="arithmetic of the GEMM-shaped kernels: f16 (default) = half operands on the 16-bit matrix pipe, the "
                         "configuration that holds the 1e-3 dB PSNR bound; bf16 = BASELINE.json configs[1] to the letter (same "
                         "pipe, same rate, 8-bit significands: 3e-3 dB)")
    ap.add_argument("--corr-precision", choices=["bf16x3", "single", "top2"], default="top2",
                    help="correlation arg-max when --precision is not f32: top2 = 16-bit pass keeping two candidates + exact "
                         "re-score; single = 16-bit winner; bf16x3 = f32-grade scores (bf16 / bf16x3 only), 2.4x the kernel time")
    ap.add_argument("--no-harness", action="store_true", help="skip the end-to-end harness measurement (100 frames on disk, ~25 s)")
    ap.add_argument("--no-graph", action="store_true", help="launch kernels eagerly instead of replaying hipGraph segments")
    ap.add_argument("--streams", type=int, default=2, help="HIP streams for the independent neighbour-frame / reference branches of a frame")
    ap.add_argument("--branch", choices=["bs", "b"], default="bs", help="bs: with sharp reference (SearchTransfer); b: SelfTransfer")
    ap.add_argument("--batch", type=int, default=1, help="windows per forward call (BASELINE configs[1] is batch 1; B > 1 batches the encoder passes of all samples per layer)")
    ap.add_argument("--inflight", type=int, default=3,
                    help="frames in flight: consecutive steps alternate over this many launch streams (each its own captured graph instance), "
                         "so that the kernels of one frame fill the tails and launch gaps of the others (1: one frame at a time).  Round 4: three, "
                         "ungated (--gate none) — with the frame's Swin calls batched on one stream there is no second in-frame stream to fill the "
                         "chip any more, and three free-running frames measured +2.8 %% over round 3's two gated ones (same box)")
    ap.add_argument("--no-families", action="store_true", help="skip the per-family kernel-time pass (3 eager frames with HIP events around every launch)")
    ap.add_argument("--no-extras", action="store_true", help="skip the bf16-to-the-letter, f32-grade and training sub-records of the --full line")
    ap.add_argument("--free-overlap", action="store_true", help="(= --gate none, the default since round 4)")
    ap.add_argument("--gate", choices=["corr_end", "corr_start", "none"], default=None,
                    help="with --inflight > 1, when step i + 1 may start: after step i's correlation kernel (corr_end, round 3), when it starts "
                         "(corr_start), or at once (none)")
    ap.add_argument("--knobs", default="", help='experiments: JSON of extra speinet_amd.ops.Ctx fields, e.g. \'{"stage": {"glue": {"precision": "bf16x3"}}}\'')
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (rank 0) as DIR/<name>.npy, float32")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("bench.py: --steps must be >= 1")

    if "RANK" not in os.environ and args.gpus > 1:
        # one command for N GPUs: this parent never touches the GPU; it starts the N ranks (python -m torch.distributed.run ...
        # bench.py <the same arguments>) as a child, passes rank 0's JSON line through and exits with the worst rank's code
        from speinet_amd.dist import launch_ranks
        sys.exit(launch_ranks(os.path.abspath(__file__), sys.argv[1:], args.gpus))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if "RANK" in os.environ:            # launched by torch.distributed.run: one rank per GPU over RCCL, also for N = 1
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        assert dist.get_world_size() == world
    else:
        local = 0
        torch.cuda.set_device(0)
    if args.gpus != world:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: the line's n_gpus must be the RCCL world size "
                         "(`python bench.py --gpus N` starts its own ranks; under torch.distributed.run pass --gpus = --nproc-per-node)")
    dev = torch.device("cuda", local)

    from speinet_amd.speinet import SPEINet, default_args
    from speinet_amd.synth import state_dict_template, synth_frames, synth_state_dict

    h, w = args.height, args.width
    net = SPEINet(args=default_args())
    net.load_state_dict(synth_state_dict(state_dict_template(), seed=0), strict=True)
    net = net.to(dev).eval()
    net.precision, net.corr_precision = args.precision, args.corr_precision
    net.use_graph = not args.no_graph
    net.streams = args.streams
    if args.knobs:
        net.knobs = json.loads(args.knobs)
    # each rank deblurs its own frames (clip shard = rank); two distinct windows alternate so nothing is cached
    nb = max(1, args.batch)
    frames = [synth_frames(nb, h, w, seed=1234 + 17 * rank + i, zero_ref=tuple(range(nb)) if args.branch == "b" else ()).to(dev) for i in range(2)]
    routing = [args.branch == "b"] * nb

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    nfl = max(1, args.inflight)
    gate_mode = args.gate or "none"
    checksums = [torch.zeros(1, device=dev, dtype=torch.float64) for _ in range(nfl)]
    prof = {"corr_argmax": []}
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    # frames in flight: step i runs on launch stream i % nfl (its own captured graph instance), so that step i + 1's encoder passes
    # fill the chip under step i's correlation kernel and decoder; within a stream steps stay in order
    lanes = [torch.cuda.current_stream(dev)] + [torch.cuda.Stream(device=dev) for _ in range(nfl - 1)]

    def run_steps(n, **kw):
        gate, out = None, None
        for i in range(n):
            with torch.cuda.stream(lanes[i % nfl]):
                if gate is not None and nfl > 1 and gate_mode != "none":
                    # (round 3's policy, --gate corr_end: the next frame starts once this frame's correlation kernel — a full-chip MFMA
                    # kernel — is done, so that its encoder passes run beside THIS frame's decoder)
                    torch.cuda.current_stream().wait_event(gate)
                pr = kw.get("profile")
                local = pr if pr is not None else {"corr_argmax": []}
                out = net(frames[i % 2], **dict(kw, profile=local))
                gate = local["corr_argmax"][-1][1 if gate_mode == "corr_end" else 0]            # (B > 1: the last sample's)
                checksums[i % nfl].add_(out.double().sum())
                if pr is not None:
                    marks[i + 1].record()
        return out

    with torch.no_grad():
        run_steps(max(args.warmup, nfl), routing=routing)
        barrier()                                  # the warm-up frames of every launch stream are done before the sums are cleared
        for c in checksums:
            c.zero_()
        # ---- the timed region: EXACTLY `steps` forwards, the dominant kernel bracketed live by HIP events ----------------
        barrier()
        t0 = time.perf_counter()
        marks[0].record()
        last_out = run_steps(args.steps, routing=routing, profile=prof)
        barrier()
        dt = time.perf_counter() - t0
        dumped = dump_outputs(args.dump_outputs, {"output": last_out}) if args.dump_outputs and rank == 0 else None
        del last_out
        checksum = sum(checksums)
        # ---- [full] the same steps the way the reference calls forward: no routing hint (device test + one host sync per call) ----
        dt_ref_call = None
        if args.full:
            barrier()
            t1 = time.perf_counter()
            run_steps(args.steps)
            barrier()
            dt_ref_call = time.perf_counter() - t1
        # ---- [full] per-family kernel time: the same frames once more, eager on ONE stream with a HIP event pair around every launch of the
        # conv / swin / correlation / streaming kernels (exclusive times: nothing overlaps; not part of the timed region) ----------------
        fam_prof, fam_frames = {"families": {}}, 0
        if rank == 0 and args.full and not args.no_families:
            keep = (net.use_graph, net.streams)
            net.use_graph, net.streams = False, 1
            net(frames[0], routing=routing)                       # eager warm-up (allocator)
            torch.cuda.synchronize()
            for i in range(3):
                net(frames[i % 2], routing=routing, profile=fam_prof)
                fam_frames += nb
            torch.cuda.synchronize()
            net.use_graph, net.streams = keep
    step_ms = [marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps)] if nfl == 1 else \
              [marks[i].elapsed_time(marks[i + nfl]) / nfl for i in range(1, args.steps + 1 - nfl)]   # same-stream neighbours
    if not step_ms:                     # steps <= frames in flight: no same-stream pair to time, only the wall clock of the region
        step_ms = [1e3 * dt / args.steps]
    pairs = prof["corr_argmax"]
    corr_ms = sum(s.elapsed_time(e) for s, e in pairs) / max(1, len(pairs))
    assert len(pairs) == args.steps * nb, "the dominant kernel must be timed once per frame"

    from speinet_amd.dist import gather_metrics, max_over_ranks
    tmax = max_over_ranks(dt, dev, dist)
    tmax_ref = max_over_ranks(dt_ref_call, dev, dist) if args.full else None
    # the only payload that crosses xGMI: one [checksum, frames] row per rank
    gathered = gather_metrics(torch.cat((checksum, torch.tensor([float(args.steps)], device=dev, dtype=torch.float64))), dist)
    assert torch.isfinite(gathered).all(), "non-finite output"
    assert int(gathered[:, 1].sum().item()) == world * args.steps

    if rank == 0:
        fps = world * args.steps * nb / tmax
        # the diagonal-sliding kernel computes every row-against-row term once: a third of the bmm's multiply-adds reach the matrix
        # pipe.  `achieved` prices the flops the kernel EXECUTES (the honest MFMA utilisation); the bmm-equivalent rate is reported beside it
        kname = prof.get("corr_kernel") or ""
        exec_flops = corr_flops(h, w) / (3.0 if kname.startswith("corr_diag") else 1.0)
        ach = exec_flops / (corr_ms * 1e-3) / 1e12 if corr_ms > 0 else 0.0
        ach_alg = corr_flops(h, w) / (corr_ms * 1e-3) / 1e12 if corr_ms > 0 else 0.0
        peak = PEAK_TFLOPS[args.precision]
        dtype = args.precision if args.precision == "f32" else f"{args.precision} (correlation {args.corr_precision})"
        k_bytes, path_hbm, tsrc, fam_hbm = traffic_bytes(args.precision, args.corr_precision) if (h, w) == (H, W) else (None, None, None, {})
        qs = statistics.quantiles(step_ms, n=10) if len(step_ms) >= 2 else [step_ms[0]] * 9
        families = family_records(fam_prof["families"], fam_frames, h, w, args.branch == "bs", peak, fam_hbm, kname.startswith("corr_diag"))
        if "conv" in families:
            families["conv"]["by_bound"] = conv_sub_records(fam_prof.get("conv_sub"), fam_frames, families["conv"]["algorithmic_flops_per_frame"], peak)
        top = max(families, key=lambda k: families[k]["ms_per_frame"]) if families else None
        line = {
            "metric": "deblurred 720p frames/sec", "value": fps, "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * tmax / args.steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": dtype, "data": "synthetic",
            "config": {"workload": f"SPEINet.forward on synthetic {w}x{h} 5-frame windows, batch {nb} per GPU, "
                                   f"{'_forwardbs (SearchTransfer)' if args.branch == 'bs' else '_forwardb (SelfTransfer)'}, "
                                   "synthetic name-keyed weights seed 0", "frames_per_step_per_gpu": nb,
                       "sharding": "frames by rank, no data-path collective",
                       "launch": ("2 hipGraph segments + the correlation kernel per frame" if net.use_graph else "eager") + f", {args.streams} HIP streams"
                                 + (f"; {nfl} frames in flight" + {"corr_end": " (step i + 1 starts when step i's correlation kernel is done)",
                                                                     "corr_start": " (step i + 1 starts with step i's correlation kernel)",
                                                                     "none": " on their own streams, ungated"}[gate_mode] if nfl > 1 else "")},
            "step_ms": {"median": statistics.median(step_ms), "p10": qs[0], "p90": qs[8], "min": min(step_ms), "max": max(step_ms)},
            # the family with the most kernel time per frame; every family is in `families`, the correlation kernel —
            # the one launch per frame that can be bracketed live inside the timed region — keeps its own record
            "roofline": {**({"bound": families[top]["bound"], "kernel": f"{top} family: {families[top]['kernels']}",
                             "achieved": families[top]["achieved"], "peak": families[top]["peak"], "unit": families[top]["unit"],
                             "frac": families[top]["frac"], "traffic": families[top]["hbm_bytes_per_frame"],
                             "ms_per_frame": families[top]["ms_per_frame"],
                             "what": "achieved = the family's ALGORITHMIC flops (bytes) per frame / its kernel time per frame; kernel time = sum of "
                                     "HIP-event pairs around every launch of the family over 3 eager single-stream frames run right after the timed "
                                     "region (exclusive: nothing overlaps); traffic = the family's HBM bytes per frame from the offline PMC passes"}
                            if top else {"bound": "mfma", "kernel": None, "achieved": None, "peak": peak, "unit": "TFLOP/s", "frac": None, "traffic": None}),
                         "families": families, "traffic_source": tsrc,
                         "correlation_kernel": {
                             "kernel": prof.get("corr_kernel"), "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak,
                             "traffic": k_bytes, "launch_ms": corr_ms,
                             "launch_ms_source": "HIP events around the direct launch between the two graph segments, every timed step",
                             "algorithmic_flops_per_launch": corr_flops(h, w), "executed_flops_per_launch": exec_flops,
                             "algorithmic_equivalent_tflops": ach_alg,
                             "note": ("achieved = executed flops / launch time; the kernel shares each row-against-row term among the three patch rows "
                                      "that use it, so it executes a third of the algorithmic (bmm) count: the bmm-equivalent rate exceeds the MFMA peak")
                                     if exec_flops != corr_flops(h, w) else "achieved = algorithmic flops / launch time"},
                         "path_flops_per_frame": path_flops(h, w),
                         "path_frac": path_flops(h, w) * fps / world / 1e12 / peak,
                         "path_hbm_bytes_per_frame": path_hbm,
                         "path_hbm_frac": (path_hbm * fps / world / 8e12) if path_hbm else None},
            "checksum": float(gathered[:, 0].sum().item()),
        }
        if dumped is not None:
            line["dump_outputs"] = dumped
        if tmax_ref is not None:
            line["reference_call"] = {"value": world * args.steps * nb / tmax_ref, "unit": "frames/s", "ms_per_step": 1e3 * tmax_ref / args.steps,
                                      "note": "forward(x) without the routing hint: the frame-3 test runs on the device, one host sync per call"}
        extras = args.full and world == 1 and not args.no_extras and (h, w) == (H, W) and args.precision == "f16" and nb == 1
        if extras:
            # BASELINE.json configs[1] to the letter ("bf16 forward"): the same steps with bf16 operands (8-bit significands: 3e-3 dB)
            net.precision = "bf16"
            prof_b = {"corr_argmax": []}
            with torch.no_grad():
                run_steps(max(3, nfl), routing=routing)
                barrier()
                tb = time.perf_counter()
                run_steps(args.steps, routing=routing, profile=prof_b)
                barrier()
                dtb = time.perf_counter() - tb
            pb = prof_b["corr_argmax"]
            line["bf16_letter"] = {"value": args.steps / dtb, "unit": "frames/s", "ms_per_step": 1e3 * dtb / args.steps,
                                   "dtype": f"bf16 (correlation {args.corr_precision})", "corr_kernel": prof_b.get("corr_kernel"),
                                   "corr_launch_ms": sum(s_.elapsed_time(e_) for s_, e_ in pb) / max(1, len(pb)),
                                   "parity": "|dPSNR| vs the reference 3e-3 dB (tests/test_gpu_bf16.py bound 1e-2)"}
            # BASELINE.json configs[2] ("fp32, PSNR-matched"): the f32-grade arithmetic — split bf16x3 products on the 16-bit matrix pipe
            # (2^-16 per operand, fp32 accumulation; every kernel <= 2e-4 relative, frames within 1e-3 dB of the reference with the
            # correlation in the same arithmetic: tests/test_gpu_bf16.py, test_gpu_parity.py) — same frames, fewer steps (3x the time)
            net.precision, net.corr_precision = "bf16x3", "bf16x3"
            k32 = max(4, args.steps // 4)
            with torch.no_grad():
                run_steps(nfl + 1, routing=routing)
                barrier()
                t3 = time.perf_counter()
                run_steps(k32, routing=routing)
                barrier()
                dt3 = time.perf_counter() - t3
            line["f32_grade"] = {"value": k32 / dt3, "unit": "frames/s", "ms_per_step": 1e3 * dt3 / k32, "steps": k32,
                                 "dtype": "bf16x3 (split products, f32-grade; correlation bf16x3)",
                                 "parity": "|dPSNR| vs the reference <= 1e-3 dB, max |err| < 1e-3 (tests/test_gpu_parity.py, test_gpu_bf16.py)"}
            net.precision, net.corr_precision = args.precision, args.corr_precision
        if args.full and world == 1 and not args.no_harness and (h, w) == (H, W) and args.precision != "f32" and nb == 1:
            from speinet_amd.inference import harness_throughput
            del net, frames
            torch.cuda.empty_cache()
            with contextlib.redirect_stdout(sys.stderr):       # the harness logs its configuration; stdout carries the one JSON line
                line["harness"] = harness_throughput(100, args.precision)
        if extras:
            # BASELINE.json configs[4]: one training step of the swint model on 200x200 crops (trainer/trainer_swint.py), batch 20
            torch.cuda.empty_cache()
            tr = train_measure(["--batch", "20", "--steps", "3", "--warmup", "1"])
            line["train"] = {k: tr[k] for k in ("metric", "value", "unit", "batch_per_gpu", "patch", "ms_per_step", "ms", "dtype")}
        mode = "none" if args.no_cpu_baseline else args.cpu_baseline
        if args.full and world == 1 and mode != "none":
            line["cpu_baseline"] = cpu_baseline(1234, mode, args.cpu_budget)
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    if "--train" in sys.argv[1:]:
        train_main([v for v in sys.argv[1:] if v != "--train"])
    else:
        main()
