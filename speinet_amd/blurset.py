"""A training set from sharp high-frame-rate footage, the way the reference makes its GoProS-style sets: consecutive runs of 1..15
sharp frames are averaged into one blurry frame each; a run of at most `threshold` = 5 frames counts as sharp (label 1), the run's
middle frame is the ground truth (reference LD_detector/mix_choice_dataset.py:46-117, sharp_detector_params_estimation_parallel.py:
38-76).

    python -m speinet_amd.blurset --input <dir of clip folders> --output <dir> [--ratio 0.1 0.3 0.5] [--threshold 5] [--seed N]
                                  [--light code|srgb|gamma:<g>] [--noise <shot>:<read>] [--shake <len>|<lo>..<hi>] [--frames runs|single]
                                  [--codec <q>|<lo>..<hi>]

writes `<output>/blur/<clip>/<i>.png`, `<output>/gt/<clip>/<i>.png` and `<output>/label/<clip>.npy`: the layout `data.ClipSet`,
`speinet_amd.fit` and `python -m speinet_amd.detector fit` read.  The frame files are numbered with six digits: the loaders pair
frames and labels by sorted file name (as the reference's do, data/videodata_nfs.py:127-162), and the reference's own `0.png ..
123.png` do not sort in frame order.  `--light`, `--noise`, `--shake`, `--frames` and `--codec` are the blur-synthesis recipe:
speinet_amd.recipe states it (the default is the reference's average of code values, byte for byte; `--frames single` is the mode for
ordinary 24 / 30 fps footage and needs `--shake`); they change the frames under `blur/` only: ground truth, labels and layout stay.

  * `plan_runs`   — the reference's draw sequence on a `random.Random` of the caller's (no global state): runs and labels;
  * `plan_single` — `--frames single`: one run of length 1 per source frame, its label drawn on the caller's `random.Random`;
  * `plan_dataset` — that sequence for every clip of a directory on one `random.Random(seed)` (also data.SharpClipSet's, per epoch);
  * `synthesize`  — the averaging on the GPU (csrc/blurset.hip, one launch per chunk of the clip): frames cross PCIe once as uint8,
                    device memory is bounded by the chunk;
  * `write_dataset` — every clip folder of a directory, PNGs encoded on worker threads behind `clip.HostRing`.
"""
from __future__ import annotations

import argparse
import os
import random
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import codec as _codec
from . import ops
from . import shake as _shake
from .clip import IMAGE_EXTS, HostRing, frames_of, imwrite
from .recipe import Clip, Recipe, add_arguments, from_args

MAX_RUN = 15                     # spei_window_mean_u8's longest run
CHUNK_FRAMES = 64                # source frames resident per launch (a 720p frame is 2.8 MB)


def check_arguments(ratio, threshold: int, window_range) -> None:
    """The reference's check_arguments (sharp_detector_params_estimation_parallel.py:38-42), raising ValueError."""
    if len(window_range) != 2 or int(window_range[0]) < 1 or int(window_range[1]) > MAX_RUN:
        raise ValueError(f"window_range must be (low, high) with 1 <= low and high <= {MAX_RUN}; got {tuple(window_range)}")
    if threshold not in range(int(window_range[0]), int(window_range[1])):
        raise ValueError(f"threshold {threshold} must lie in range{tuple(window_range)}")
    if ratio is None:
        raise ValueError("ratio must not be None")
    if not 0 <= ratio <= 1:
        raise ValueError(f"ratio {ratio} must lie in [0, 1]")


def plan_runs(n_frames: int, ratio: float, threshold: int = 5, window_range=(1, 15), rng: random.Random = None):
    """The runs the reference's generate_blurry_sequence (:57-66) cuts a clip of n_frames into, in its draw order: per run
    `random() < ratio or remaining <= threshold` is the label, then `randint(low, threshold)` frames for a sharp run or
    `randint(threshold + 1, high)` for a blurry one (the last run takes what is left).  -> (starts, lengths, labels) int64 arrays.
    `rng`: a `random.Random`; seeded like the reference's `random.seed(seed)` it draws the reference's runs."""
    check_arguments(ratio, threshold, window_range)
    if n_frames < 1:
        raise ValueError(f"a clip needs at least one frame; got {n_frames}")
    if rng is None:
        raise ValueError("pass a random.Random (plan_runs touches no global random state)")
    starts, lengths, labels = [], [], []
    at = 0
    while at < n_frames:
        label = int((rng.random() < ratio) or (n_frames - at <= threshold))
        size = rng.randint(window_range[0], threshold) if label else rng.randint(threshold + 1, window_range[1])
        size = min(size, n_frames - at)
        starts.append(at)
        lengths.append(size)
        labels.append(label)
        at += size
    return np.asarray(starts, np.int64), np.asarray(lengths, np.int64), np.asarray(labels, np.int64)


def plan_single(n_frames: int, ratio: float, rng: random.Random = None):
    """The plan of ordinary-frame-rate footage (`frames="single"`): every source frame is its own run of length 1, labelled
    `int(rng.random() < ratio)` in frame order — 1 steady, 0 shaken (speinet_amd.shake) — on the caller's `random.Random`, as
    `plan_runs` draws its labels.  -> (starts, lengths, labels) int64 arrays."""
    if ratio is None or not 0 <= ratio <= 1:
        raise ValueError(f"ratio {ratio} must lie in [0, 1]")
    if n_frames < 1:
        raise ValueError(f"a clip needs at least one frame; got {n_frames}")
    if rng is None:
        raise ValueError("pass a random.Random (plan_single touches no global random state)")
    labels = [int(rng.random() < ratio) for _ in range(n_frames)]
    return np.arange(n_frames, dtype=np.int64), np.ones(n_frames, np.int64), np.asarray(labels, np.int64)


def _chunks(starts, lengths, chunk_frames: int):
    """Consecutive runs grouped so that each group reads at most chunk_frames source frames: (first run, last run + 1, lo, hi)."""
    i, M = 0, len(starts)
    while i < M:
        lo, hi, j = int(starts[i]), int(starts[i] + lengths[i]), i + 1
        while j < M and max(hi, int(starts[j] + lengths[j])) - min(lo, int(starts[j])) <= chunk_frames:
            lo, hi = min(lo, int(starts[j])), max(hi, int(starts[j] + lengths[j]))
            j += 1
        yield i, j, lo, hi
        i = j


def synthesize_chunks(frames, runs, device="cuda", gray: bool = False, chunk_frames: int = CHUNK_FRAMES, light="code", noise=None,
                      shake=None, codec=None):
    """Generator of (first run, blur uint8 [m,H,W,3], gt uint8 [m,H,W,3], gray [m,H,W] or None) on `device`, one item per chunk of
    consecutive runs; see `synthesize`."""
    clip = Clip.of(light, noise, shake, codec)                 # the one validation (speinet_amd.recipe)
    fr = frames if hasattr(frames, "on_device") else frames_of(frames)
    starts, lengths = (np.asarray(a, np.int64).reshape(-1) for a in runs[:2])
    if starts.size != lengths.size or starts.size == 0:
        raise ValueError(f"runs must be (starts, lengths) of one length >= 1; got {starts.size} and {lengths.size}")
    labels = np.asarray(runs[2] if len(runs) > 2 else [], np.int64).reshape(-1)
    if clip.recipe.shake is not None and labels.size != starts.size:
        raise ValueError("shake: runs must be (starts, lengths, labels): the runs labelled 0 are the shaken ones")
    quality = clip.quality                                     # one per clip: a pure function of (spec, seed, clip)
    qtabs = quality and _codec.quant_tables(quality)[None]
    if lengths.min() < 1 or lengths.max() > MAX_RUN or starts.min() < 0 or (starts + lengths).max() > fr.T:
        raise ValueError(f"every run must hold 1..{MAX_RUN} frames inside the clip of {fr.T}")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("speinet_amd.blurset runs on MI355X only (HIP kernels); there is no CPU path")
    chunk_frames = max(int(chunk_frames), MAX_RUN)
    H, W = fr.H, fr.W
    resident = torch.is_tensor(fr.items) and fr.items.is_cuda
    with torch.no_grad(), torch.cuda.device(dev), ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 4)) as pool:
        futs = {}
        plan = list(_chunks(starts, lengths, chunk_frames))
        if not resident:
            n_buf = max(hi - lo for _, _, lo, hi in plan)
            stage = [torch.empty(n_buf, H, W, 3, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            events = [None, None]
            src_buf = torch.empty(n_buf, H, W, 3, dtype=torch.uint8, device=dev)

        def want(c):
            for _, _, lo, hi in plan[c:c + 2]:
                for i in range(lo, hi):
                    if i not in futs and not fr.on_device(i):
                        futs[i] = pool.submit(fr.host, i)

        for c, (i, j, lo, hi) in enumerate(plan):
            if resident:
                src = fr.items[lo:hi, :H, :W]
                if src.stride()[1:] != (W * 3, 3, 1):
                    src = src.contiguous()
            else:
                want(c)
                st = stage[c % 2]
                if events[c % 2] is not None:
                    events[c % 2].synchronize()       # the upload issued two chunks ago
                host = [t for t in range(lo, hi) if not fr.on_device(t)]
                for t in host:
                    st[t - lo].numpy()[...] = futs.pop(t).result()
                if host:
                    src_buf[:hi - lo].copy_(st[:hi - lo], non_blocking=True)
                    events[c % 2] = torch.cuda.Event()
                    events[c % 2].record()
                for t in range(lo, hi):
                    if fr.on_device(t):
                        src_buf[t - lo].copy_(fr.device(t))
                src = src_buf[:hi - lo]
            ids = np.arange(i, j)                              # noise and PSFs depend on (seed, clip, run id) alone: not on the chunk
            blur, gt, g = ops.window_mean_u8(src, starts[i:j] - lo, lengths[i:j], gray=gray, light=clip.recipe.light,
                                             noise=clip.noise_records(ids), shake=clip.shake(ids, labels[i:j]))
            if quality is not None:                            # whole frames on the grid at (0, 0): nothing depends on the chunk
                ops.codec_u8(blur, _codec.records(j - i), qtabs, gray=g)
            yield i, blur, gt, g


def synthesize(frames, runs, device="cuda", gray: bool = False, chunk_frames: int = CHUNK_FRAMES, light="code", noise=None, shake=None,
               codec=None):
    """Average the runs of a clip on the GPU: `frames` in any form `clip.frames_of` accepts (uint8 [T,H,W,3] array or tensor on the
    host or the device, a list of frames, a list of image paths), `runs` = (starts, lengths[, labels]) as `plan_runs` returns them
    -> (blur uint8 [M,H,W,3], gt uint8 [M,H,W,3]) on `device`, and the detector's gray planes [M,H,W] as a third item when `gray`.
    blur[m] is the per-byte floor of the run's mean (the bytes the reference writes), gt[m] the run's middle frame.  The source
    frames are uploaded `chunk_frames` at a time; only the result is as long as the clip.  `light`: "srgb" or "gamma:<g>" averages in
    linear light (speinet_amd.light) instead; gt is unchanged and the gray planes are those of the encoded blur bytes.  `noise`: None, or
    `light.ClipNoise(spec, seed, clip[, first_run])` — the sensor noise of clip `clip` under `seed` at the levels of `spec`, run m
    carrying the id first_run + m; the result does not depend on `chunk_frames`.  `shake`: None, or `shake.ClipShake(spec, seed,
    clip[, first_run])` — camera shake (speinet_amd.shake) on the runs labelled 0 (`runs` must then carry its labels), one PSF per run
    drawn from (seed, clip, run id); it needs a linear light and does not depend on `chunk_frames` either.  `codec`: None, or
    `codec.ClipCodec(spec, seed, clip)` — every blur frame (any label, any light) goes through speinet_amd.codec's JPEG-style round trip
    at the clip's one quality, in place after the launch above (one more launch per chunk); gt is untouched and the gray planes are
    those of the coded bytes."""
    parts = list(synthesize_chunks(frames, runs, device, gray, chunk_frames, light, noise, shake, codec))
    out = (torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts]))
    return out + (torch.cat([p[3] for p in parts]),) if gray else out


def clip_folders(src_dir: str) -> list:
    """(clip name, its frames in file-name order) for every folder of images under src_dir."""
    clips = []
    for name in sorted(os.listdir(src_dir)):
        d = os.path.join(src_dir, name)
        if os.path.isdir(d):
            files = sorted(os.path.join(d, f) for f in os.listdir(d) if f.lower().endswith(IMAGE_EXTS))
            if files:
                clips.append((name, files))
    if not clips:
        raise ValueError(f"{src_dir}: no clip folder with image files (one folder of sharp frames per clip)")
    return clips


def plan_dataset(clip_lengths, ratios, seed: int = 0, threshold: int = 5, window_range=(1, 15), frames: str = "runs") -> list:
    """The draws of a whole directory on ONE `random.Random(seed)` (reference process_dataset, mix_choice_dataset.py:78-117): for every
    clip, in the clips' sorted order (`clip_lengths`: their frame counts in that order), `rng.choice(ratios)` — drawn only when there
    are several ratios (:79) — then the clip's `plan_runs`, or with `frames="single"` its `plan_single`.  -> one (ratio, (starts,
    lengths, labels)) per clip."""
    ratios = list(ratios)
    if not ratios:
        raise ValueError("give ratio or ratios")
    if frames not in _shake.FRAMES:
        raise ValueError(f"frames {frames!r}: expected 'runs' or 'single'")
    for r in ratios:
        check_arguments(r, threshold, window_range)
    rng = random.Random(seed)
    plans = []
    for n_frames in clip_lengths:
        r = rng.choice(ratios) if len(ratios) > 1 else ratios[0]
        plans.append((r, plan_single(int(n_frames), r, rng) if frames == "single" else plan_runs(int(n_frames), r, threshold, window_range, rng)))
    return plans


def write_dataset(src_dir: str, out_dir: str, ratio=None, ratios=None, seed: int = 0, threshold: int = 5, window_range=(1, 15),
                  device="cuda", chunk_frames: int = CHUNK_FRAMES, log=None, light="code", noise=None, shake=None,
                  frames: str = "runs", codec=None) -> list:
    """For every clip folder under src_dir write out_dir/blur/<clip>/<i>.png, out_dir/gt/<clip>/<i>.png and out_dir/label/<clip>.npy
    (reference process_dataset, mix_choice_dataset.py:78-117).  `ratio`: the share of sharp runs; `ratios`: several, one drawn per
    clip (:79) from the same `random.Random(seed)` that then draws the clip's runs (`plan_dataset`).  `light`, `noise`, `shake`, `frames`
    and `codec` are the recipe (speinet_amd.recipe.Recipe: specs, validated there): noise levels, PSFs and the JPEG quality are drawn
    from `seed`, the clip's index and the run's; none of them touches the plan, except that `frames="single"` plans with `plan_single`.
    They change the frames under blur/ only and are not recorded in the set.  -> one dict per clip (name, ratio, frames, labels; with
    noise also its `shot` and `read`, with a codec its `quality`)."""
    recipe = Recipe(light, noise, shake, frames, codec)
    clips = []
    for name, files in clip_folders(src_dir):
        try:
            clips.append((name, frames_of(files)))
        except ValueError as e:
            raise ValueError(f"clip {name}: {e}") from None
    plans = plan_dataset([fr.T for _, fr in clips], [ratio] if ratios is None else ratios, seed, threshold, window_range, recipe.frames)
    dev = torch.device(device)
    done = []
    os.makedirs(os.path.join(out_dir, "label"), exist_ok=True)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 4), thread_name_prefix="speinet-png") as writers, torch.cuda.device(dev):
        ring = HostRing(writers, n=16)
        for k, ((name, fr), (r, (starts, lengths, labels))) in enumerate(zip(clips, plans)):
            bdir, gdir = os.path.join(out_dir, "blur", name), os.path.join(out_dir, "gt", name)
            os.makedirs(bdir, exist_ok=True)
            os.makedirs(gdir, exist_ok=True)

            def save(b, g, pb, pg):
                imwrite(pb, b.numpy())
                imwrite(pg, g.numpy())

            draw = recipe.clip(seed, k)
            for i0, blur, gt, _ in synthesize_chunks(fr, (starts, lengths, labels), dev, False, chunk_frames, **draw.stages()):
                for m in range(blur.shape[0]):
                    fn = f"{i0 + m:06d}.png"
                    ring.land(lambda b, g, pb=os.path.join(bdir, fn), pg=os.path.join(gdir, fn): save(b, g, pb, pg), blur[m], gt[m])
            ring.drain()
            np.save(os.path.join(out_dir, "label", name + ".npy"), labels)
            d = draw.drawn()
            done.append({"name": name, "ratio": r, "source_frames": fr.T, "frames": int(labels.size), "labels": labels, **d})
            if log:
                said = recipe.describe(noise=lambda: f"shot {d['shot']:.3g} read {d['read']:.3g}", codec=lambda: f"quality {d['quality']}",
                                       shake=lambda: f"{recipe.shake} on {int((labels == 0).sum())} frames")
                log(f"> {name}: {fr.T} sharp frames -> {labels.size} frames, {int(labels.sum())} labelled sharp (ratio {r}, {said})")
    return done


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Make a blur / gt / label training set from folders of sharp high-frame-rate frames on an MI355X")
    p.add_argument("--input", required=True, help="a directory with one folder of sharp frames per clip (PNG / JPG / BMP, file-name order)")
    p.add_argument("--output", required=True, help="directory for blur/<clip>/, gt/<clip>/ and label/<clip>.npy")
    p.add_argument("--ratio", type=float, nargs="+", default=[0.5], help="share of sharp runs; several: one is drawn per clip")
    p.add_argument("--threshold", type=int, default=5, help="a run of at most this many frames is a sharp frame (label 1)")
    p.add_argument("--seed", type=int, default=0)
    add_arguments(p)                                           # --light --noise --shake --frames --codec
    p.add_argument("--device", default="cuda")
    return p


def main(argv=None) -> None:
    p = parser()
    a = p.parse_args(argv)
    recipe = from_args(p, a)
    t0 = time.time()
    done = write_dataset(a.input, a.output, ratios=a.ratio, seed=a.seed, threshold=a.threshold, device=a.device,
                         log=lambda s: print(s, flush=True), **recipe._asdict())
    n_src, n_out = sum(d["source_frames"] for d in done), sum(d["frames"] for d in done)
    said = recipe.describe(shake=lambda: f"{recipe.shake}, frames {recipe.frames}")
    print(f"# {len(done)} clips, {n_src} sharp frames -> {n_out} frames in {time.time() - t0:.2f}s, {said}", flush=True)


if __name__ == "__main__":
    main()
