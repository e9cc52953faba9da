"""Harness counterpart of the reference's `inference_SPEINet.py`: same flags, data layout,
selection logic, uint8 round trip, PSNR/SSIM and log-line format — with the forward pass on the HIP path, an explicit
`--device`, presets that no longer clobber explicit paths, and clip sharding over ranks instead of DataParallel.

    <data_path>/{blur,gt}/<clip>/<frame>.png       [<data_path>/label/<clip>.npy  (0/1 per frame, 1 = sharp)]

Without a label file the LD detector (speinet_amd.detector, row a11) labels the frames on the GPU.
Each clip runs through the clip loop, `video.deblur_clip` (frames cropped to multiples of 20 as the reference does, references
zeroed by the frame numbers in the file names): decode-once prefetch of the frame files, cross-window encoder reuse, two windows in
flight, a bf16x3 recompute of a frame whose 16-bit pass left a non-finite value.  This module adds the dataset layout and the
metrics: the PSNR / SSIM of each deblurred frame against its ground truth (csrc/metrics.hip), landed in page-locked memory with the
frame, whose PNG encode runs on worker threads while the GPU deblurs the next windows; log lines are still written in frame order.
Reference: inference_SPEINet.py:193-237 (__init__), :338-429 (infer), :484-543 (metrics), :610-700 (flags / presets).
SSIM is restated with numpy (cv2 is absent): Gaussian 11x11, sigma 1.5, valid region — parity unpinned.
"""
from __future__ import annotations

import argparse
import collections
import functools
import glob
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import checkpoint, detector, ops, selection, video
from .clip import FrameCache, HostRing, imread, imwrite
from .dist import gather_metrics, shard_clips_by_length
from .speinet import SPEINet, default_args

_imread, _imwrite = imread, imwrite


def calc_ssim(img1: np.ndarray, img2: np.ndarray) -> float:
    """inference_SPEINet.py:502-543: the reference averages the same 3-channel value three times.  The 11x11 Gaussian
    window is outer(k, k): applied as two 1-D passes (scipy.ndimage, float64, GIL released), valid region only."""
    from scipy.ndimage import correlate1d
    ax = np.arange(11) - 5
    k = np.exp(-(ax ** 2) / (2 * 1.5 ** 2))
    k /= k.sum()
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    a, b = img1.astype(np.float64), img2.astype(np.float64)

    def filt(x):   # valid region only ([5:-5, 5:-5] of the reference's same-size filter2D)
        y = correlate1d(correlate1d(x, k, axis=0, mode="constant"), k, axis=1, mode="constant")
        return y[5:-5, 5:-5]

    mu1, mu2 = filt(a), filt(b)
    s1, s2, s12 = filt(a * a) - mu1 ** 2, filt(b * b) - mu2 ** 2, filt(a * b) - mu1 * mu2
    m = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 ** 2 + mu2 ** 2 + c1) * (s1 + s2 + c2))
    return float(m.mean())


class Logger:
    def __init__(self, result_dir: str, name: str, echo: bool = True):
        os.makedirs(result_dir, exist_ok=True)
        self.f = open(os.path.join(result_dir, name), "a")
        self.echo = echo

    def write_log(self, line: str) -> None:
        if self.echo:
            print(line)
        self.f.write(line + "\n")
        self.f.flush()


class Inference:
    def __init__(self, args):
        self.args = args
        self.n_seq = args.n_sequence
        self.device = torch.device(args.device)
        if self.device.type == "cuda":
            if self.device.index is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
            torch.cuda.set_device(self.device)      # worker threads and torch helpers default to the current device
        for k in ("data_path", "result_path"):
            if not getattr(args, k, None):
                raise ValueError(f"--{k} is not set and --default_data {getattr(args, 'default_data', None)!r} has no preset for it")
        self.rank, self.world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
        now = time.strftime("%Y-%m-%d %H:%M:%S", time.localtime())
        self.logger = Logger(args.result_path, f"inference_log_{now}_rank{self.rank}.txt", echo=self.rank == 0)
        for k in ("save_image", "border", "model_path", "data_path", "result_path"):
            self.logger.write_log(f"{k}: {getattr(args, k)}")
        self.net = SPEINet(in_channels=3, n_sequence=self.n_seq, out_channels=3, n_resblock=3, n_feat=32, device=str(self.device), args=args)
        if args.model_path and args.model_path != "synthetic":
            checkpoint.load_into(self.net, args.model_path, strict=True)                                      # strict, like :232
        else:
            from .synth import state_dict_template, synth_state_dict
            self.net.load_state_dict(synth_state_dict(state_dict_template(), seed=0))
        self.net = self.net.to(self.device).eval()
        self.net.precision = args.precision
        self.net.corr_precision = video.CORR_PRECISION[args.precision]
        self.net.use_graph = bool(getattr(args, "graph", True))      # one hipGraph per frame shape / routing
        self.net.streams = int(getattr(args, "streams", 1))
        workers = max(2, min(8, (os.cpu_count() or 4) // max(1, self.world)))
        self.pool = ThreadPoolExecutor(max_workers=workers, thread_name_prefix="speinet-post")     # ground-truth decodes, PNG encodes
        self.ring = HostRing(self.pool, 4 * video.PREFETCH)     # deblurred frames and their [PSNR, SSIM]

    def labels_for(self, clip: str, frames: list) -> np.ndarray:
        p = os.path.join(self.args.data_path, "label", clip + ".npy")
        if os.path.exists(p):
            return np.load(p)                                   # allow_pickle=False: plain int arrays only
        imgs = torch.from_numpy(np.stack([imread(f) for f in frames]).astype(np.float32)).permute(0, 3, 1, 2)
        feats = torch.cat([detector.focus_measures(imgs[i:i + 16].to(self.device), 11) for i in range(0, len(imgs), 16)])
        return detector.predict(feats)

    @staticmethod
    def _post(save_to: str, frame: torch.Tensor, met: torch.Tensor):
        """Worker thread, once the frame and its metrics have landed: encode the PNG.  Returns (PSNR, SSIM, seconds)."""
        t0 = time.time()
        if save_to:
            imwrite(save_to, frame.numpy())
        psnr, ssim = met.tolist()
        return psnr, ssim, time.time() - t0

    def infer(self):
        a = self.args
        self.range_retries = 0
        clips = sorted(os.listdir(os.path.join(a.data_path, "blur")))
        lengths = [len(glob.glob(os.path.join(a.data_path, "blur", c, "*"))) for c in clips]
        mine = shard_clips_by_length(lengths, self.world)[self.rank]
        stats = torch.zeros(3, dtype=torch.float64)             # sum psnr, sum ssim, frames
        for ci in mine:
            t_clip = time.time()
            clip = clips[ci]
            blur = sorted(glob.glob(os.path.join(a.data_path, "blur", clip, "*")))
            gts = sorted(glob.glob(os.path.join(a.data_path, "gt", clip, "*")))
            run = video.deblur_clip(self.net, blur, self.labels_for(clip, blur), crop=True,
                                    numbers=[selection.frame_number(f) for f in blur])
            H, W = run.frames.H, run.frames.W                   # the model needs multiples of 20 (reference crops to 4)
            gt_cache = FrameCache(self.pool, lambda p: imread(p)[:H, :W], self.device)
            if a.save_image:
                os.makedirs(os.path.join(a.result_path, clip), exist_ok=True)
            vp, vs = [], []
            pending = collections.deque()                       # (name, future, pre_time, forward_time, recomputed), frame order

            def flush(block: bool):
                while pending and (block or pending[0][1].done()):
                    name, fut, t_pre, t_fwd, redo = pending.popleft()
                    psnr, ssim, t_post = fut.result()
                    if redo:
                        # half operands do not saturate (+-65504): the clip loop recomputed the frame in split-bf16 arithmetic (fp32
                        # range, f32-grade) instead of aborting the clip; counted and logged
                        self.range_retries += 1
                        self.logger.write_log(f"# {clip}-{name}: non-finite value in the {a.precision} frame, recomputed in bf16x3 "
                                              f"({self.range_retries} so far)")
                    vp.append(psnr)
                    vs.append(ssim)
                    self.logger.write_log('> {}-{} PSNR={:.5}, SSIM={:.4} pre_time:{:.3}s, forward_time:{:.3}s, post_time:{:.3}s, total_time:{:.3}s'
                                          .format(clip, name, psnr, ssim, t_pre, t_fwd, t_post, t_pre + t_fwd + t_post))

            t_loop = time.time()
            for k, frame in run:
                gt_cache.request(gts[k:k + 2 * video.PREFETCH])
                # PSNR and SSIM on the 4-pixel-cropped frame (inference_SPEINet.py:405-410): three HIP launches (csrc/metrics.hip)
                met = ops.frame_metrics(frame, gt_cache.get_dev(gts[k]), 4)
                name = os.path.splitext(os.path.basename(blur[k]))[0]
                save_to = os.path.join(a.result_path, clip, name + ".png") if a.save_image else ""
                fut = self.ring.land(functools.partial(self._post, save_to), frame, met)
                pending.append((name, fut, *run.seconds[k], run.recomputed[-1:] == [k]))
                flush(block=len(pending) > 2 * video.PREFETCH)
            t_drain = time.time()
            flush(block=True)
            self.logger.write_log("# timing {}: setup {:.3f}s, {} windows enqueued in {:.3f}s, drain {:.3f}s".format(
                clip, t_loop - t_clip, len(blur), t_drain - t_loop, time.time() - t_drain))
            self.logger.write_log("# Video:{} AVG-PSNR={:.5}, AVG-SSIM={:.4}".format(clip, sum(vp) / len(vp), sum(vs) / len(vs)))
            stats += torch.tensor([sum(vp), sum(vs), float(len(vp))], dtype=torch.float64)
        dist = None
        if self.world > 1:
            import torch.distributed as dist
        allm = gather_metrics(stats.to(self.device) if self.world > 1 else stats, dist)
        tot = allm.sum(dim=0)
        if self.rank == 0 and tot[2] > 0:
            self.logger.write_log("# Total AVG-PSNR={:.5}, AVG-SSIM={:.4}".format(tot[0].item() / tot[2].item(), tot[1].item() / tot[2].item()))
        return tot


def synth_clip(root: str, n: int = 40, h: int = 720, w: int = 1280, seed: int = 5) -> str:
    """Write a synthetic n-frame clip in the reference's data layout (<root>/data/{blur,gt}/clip0/%06d.png + label/clip0.npy,
    every 6th frame labelled sharp) and return <root>/data: the input of `harness_throughput` and of tools/harness_bench.py."""
    from PIL import Image
    from .synth import synth_frames
    x = synth_frames(1, h, w, seed=seed)[0]
    for sub in ("blur", "gt"):
        os.makedirs(os.path.join(root, "data", sub, "clip0"), exist_ok=True)
    for i in range(n):
        img = (torch.roll(x[i % 5], shifts=(3 * i, -5 * i), dims=(1, 2)).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
        for sub in ("blur", "gt"):
            Image.fromarray(img).save(os.path.join(root, "data", sub, "clip0", f"{i:06d}.png"), compress_level=1)
    os.makedirs(os.path.join(root, "data", "label"), exist_ok=True)
    np.save(os.path.join(root, "data", "label", "clip0.npy"), np.asarray([1 if i % 6 == 0 else 0 for i in range(n)]))
    return os.path.join(root, "data")


def harness_throughput(frames: int = 100, precision: str = "f16", h: int = 720, w: int = 1280, extra_args=()) -> dict:
    """End-to-end frames/s of this harness on a synthetic clip ON DISK: PNG decode -> selection -> upload -> forward (with
    cross-window encoder reuse) -> uint8 -> PSNR / SSIM -> PNG encode, everything the reference's loop does per frame
    (inference_SPEINet.py:364-429).  One untimed pass first (graph capture, page cache), then one timed pass."""
    import re
    import shutil
    import tempfile
    root = tempfile.mkdtemp(prefix="speinet_clip_")
    try:
        data = synth_clip(root, frames, h, w)
        a = build_args(["--data_path", data, "--model_path", "synthetic", "--result_path", os.path.join(root, "res"), "--precision", precision,
                        *extra_args])
        inf = Inference(a)
        inf.logger.echo = False
        inf.infer()
        torch.cuda.synchronize()
        t0 = time.time()
        tot = inf.infer()
        torch.cuda.synchronize()
        dt = time.time() - t0
        n = int(tot[2])
        lines = [ln for f in glob.glob(os.path.join(root, "res", "inference_log*")) for ln in open(f) if ln.startswith(">")][-n:]
        mean = lambda key: sum(float(re.search(key + r":([\d.e-]+)s", ln).group(1)) for ln in lines) / max(1, len(lines))
        timing = [ln.strip()[2:] for f in glob.glob(os.path.join(root, "res", "inference_log*")) for ln in open(f) if ln.startswith("# timing")][-1:]
        return {"value": n / dt, "unit": "frames/s", "frames": n, "seconds": dt, "precision": precision, "timing": timing,
                "mean_ms": {k: 1e3 * mean(k) for k in ("pre_time", "forward_time", "post_time")},
                "what": f"speinet_amd.inference on a synthetic {w}x{h} clip on disk, PNG decode/encode, PSNR and SSIM included, "
                        "cross-window encoder reuse on"}
    finally:
        shutil.rmtree(root, ignore_errors=True)


PRESETS = {   # inference_SPEINet.py:626-697 (paths only fill in what the command line left at its default)
    "REDS": dict(data_path="./data/deblur/REDS_8x_Random/test", model_path="../experiment/model/model_best.pt", result_path="../infer_results/bsdtest_reds"),
    "GOPRO": dict(data_path="./data/deblur/GOPRO/test", model_path="../experiment/model/model_best.pt", result_path="../infer_results/gopro"),
    "BSD": dict(data_path="./data/deblur/BSDtest", model_path="./model/model_best.pt", result_path="../infer_results/BSDtest_finetune"),
    "BSDtest_all": dict(data_path="./data/deblur/BSDtest_all/BSD_3ms24ms", model_path="./model/model_best.pt", result_path="../infer_results/BSD_1ms8ms"),
}


def build_args(argv=None):
    p = argparse.ArgumentParser(description="SPEINet inference (MI355X)")
    p.add_argument("--save_image", action="store_true", default=True)
    p.add_argument("--no_save_image", dest="save_image", action="store_false")
    p.add_argument("--border", action="store_true", default=True)
    p.add_argument("--default_data", type=str, default="BSDtest_all")
    p.add_argument("--data_path", type=str, default=None)
    p.add_argument("--model_path", type=str, default=None)
    p.add_argument("--result_path", type=str, default=None)
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--precision", choices=["f32", "bf16x3", "bf16", "f16"], default="f32",
                   help="arithmetic of the GEMM-shaped kernels: f32 exact; bf16x3 f32-grade; f16 the throughput mode that holds "
                        "the 1e-3 dB PSNR bound; bf16 8-bit significands (speinet_amd/ops.py)")
    p.add_argument("--streams", type=int, default=1,
                   help="HIP streams for the independent branches of a frame (round 4: 1 — the frame's Swin calls run as one batch, the "
                        "second in-frame stream has nothing left to carry, and every extra stream competes for the 4 hardware queues)")
    p.add_argument("--no_graph", dest="graph", action="store_false", default=True, help="launch kernels eagerly (no hipGraph replay)")
    p.add_argument("--n_GPUs", type=int, default=1,
                   help="ranks, one per GPU, clips sharded over them (the reference's preset attribute n_GPUs, inference_SPEINet.py:626-697, "
                        "there DataParallel); > 1 without RANK in the environment: this process starts the ranks and waits for them")
    a = p.parse_args(argv)
    for k, v in PRESETS.get(a.default_data, {}).items():
        if getattr(a, k) is None:
            setattr(a, k, v)
    n_gpus = a.n_GPUs
    for k, v in vars(default_args()).items():
        setattr(a, k, v)
    a.n_GPUs = n_gpus
    return a


def main(argv=None):
    a = build_args(argv)
    if "RANK" not in os.environ and a.n_GPUs > 1:
        # one command for N GPUs: the parent (no GPU call) starts `python -m torch.distributed.run ... -m speinet_amd.inference <args>`
        import sys
        from .dist import launch_ranks
        raise SystemExit(launch_ranks("speinet_amd.inference", list(sys.argv[1:] if argv is None else argv), a.n_GPUs, module=True))
    if a.n_GPUs != int(os.environ.get("WORLD_SIZE", "1")):
        raise SystemExit(f"--n_GPUs {a.n_GPUs} but WORLD_SIZE={os.environ.get('WORLD_SIZE', '1')}")
    if "RANK" in os.environ:
        import torch.distributed as dist
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        a.device = f"cuda:{os.environ.get('LOCAL_RANK', '0')}"
        dist.init_process_group("nccl")
        try:
            Inference(a).infer()
        finally:
            dist.destroy_process_group()
        return
    Inference(a).infer()


if __name__ == "__main__":
    main()
