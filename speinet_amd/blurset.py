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
123.png` do not sort in frame order.  `--light` (default `code`: the reference's average of code values, byte for byte) averages in
linear light instead, as an exposure does: speinet_amd.light has the integer arithmetic; the ground truth, labels and layout are the same.
`--noise <shot>:<read>` (with a linear `--light`; each side a number or `lo..hi`, drawn log-uniformly per clip) adds back the sensor
noise that averaging removed — shot coefficient and read deviation at full scale 1, speinet_amd.light has the contract.  The levels
are not fitted to any camera.  `--shake <len>` or `<lo>..<hi>` (with a linear `--light`; the blur extent in pixels, 2..30) correlates
every frame labelled blurry with a random camera-shake trajectory PSF of its own, in linear light before the noise — the blur a
hand-held camera adds inside one exposure; speinet_amd.shake has the contract.  `--frames single` is the mode for ordinary 24 / 30 fps
footage, where averaging runs gives ghost copies, not motion blur: every source frame is its own output frame, steady (label 1) with
probability `--ratio` and shaken otherwise; it needs `--shake`.  One PSF per frame, drawn independently (no camera path across
frames); extents and trajectory constants are not fitted to any camera.  `--codec <q>` or `<lo>..<hi>` (JPEG qualities 1..100, one drawn
per clip; any `--light`) puts every frame under `blur/` — the sharp-labelled ones too, never `gt/` — through a JPEG-style round trip
(YCbCr 4:2:0, 8x8 DCT, quality-scaled quantisation) as the last step, on the final bytes: the block edges and ringing of footage that
reaches the deblurrer out of a video or JPEG file; speinet_amd.codec has the contract.  The qualities and the proxy are untuned.

  * `plan_runs`   — the reference's draw sequence on a `random.Random` of the caller's (no global state): runs and labels;
  * `plan_single` — `--frames single`: one run of length 1 per source frame, its label drawn on the caller's `random.Random`;
  * `plan_dataset` — that sequence for every clip of a directory on one `random.Random(seed)` (also data.SharpClipSet's, per epoch);
  * `synthesize`  — the averaging on the GPU (csrc/blurset.hip, one launch per chunk of the clip): frames cross PCIe once as uint8,
                    device memory is bounded by the chunk;
  * `write_dataset` — every clip folder of a directory, PNGs encoded on worker threads behind `video.HostRing`.
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
from . import light as _light
from . import ops
from . import shake as _shake
from .video import IMAGE_EXTS, HostRing, _imwrite, frames_of

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
    if not _light.is_code(light):
        _light.tables(light)                              # a light without valid tables is refused before anything is read
    if noise is not None:
        noise = _light.ClipNoise(*noise)
        _light.check_noise(light, noise.spec)
        levels = _light.noise_levels(noise.spec, noise.seed, noise.clip)
    fr = frames if hasattr(frames, "on_device") else frames_of(frames)
    starts, lengths = (np.asarray(a, np.int64).reshape(-1) for a in runs[:2])
    if starts.size != lengths.size or starts.size == 0:
        raise ValueError(f"runs must be (starts, lengths) of one length >= 1; got {starts.size} and {lengths.size}")
    if shake is not None:
        shake = _shake.ClipShake(*shake)
        _shake.check(light, shake.spec)
        if len(runs) < 3 or np.asarray(runs[2]).size != starts.size:
            raise ValueError("shake: runs must be (starts, lengths, labels): the runs labelled 0 are the shaken ones")
        labels = np.asarray(runs[2], np.int64).reshape(-1)
    if codec is not None:                                  # one quality per clip: a pure function of (spec, seed, clip)
        codec = _codec.ClipCodec(*codec)
        qtabs = _codec.quant_tables(_codec.quality(codec.spec, codec.seed, codec.clip))[None]
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
            rec = None if noise is None else (_light.noise_records(np.arange(i, j) + noise.first_run, noise.clip, *levels), noise.seed)
            srec = None
            if shake is not None:                          # the PSFs depend on (seed, clip, run id) alone: not on the chunk
                ids = np.arange(i, j) + shake.first_run
                srec = (_shake.records(shake.spec, shake.seed, shake.clip, ids, labels[i:j]),
                        _shake.psf_table(shake.spec, shake.seed, shake.clip, ids, labels[i:j]))
            blur, gt, g = ops.window_mean_u8(src, starts[i:j] - lo, lengths[i:j], gray=gray, light=light, noise=rec, shake=srec)
            if codec is not None:                          # whole frames on the grid at (0, 0): nothing depends on the chunk
                ops.codec_u8(blur, _codec.records(j - i), qtabs, gray=g)
            yield i, blur, gt, g


def synthesize(frames, runs, device="cuda", gray: bool = False, chunk_frames: int = CHUNK_FRAMES, light="code", noise=None, shake=None,
               codec=None):
    """Average the runs of a clip on the GPU: `frames` in any form `video.frames_of` accepts (uint8 [T,H,W,3] array or tensor on the
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
    clip (:79) from the same `random.Random(seed)` that then draws the clip's runs (`plan_dataset`).  `light`: the light the runs are
    averaged in (speinet_amd.light; it changes the blur frames only, and is not recorded in the set).  `noise`: a spec "<shot>:<read>"
    (speinet_amd.light): sensor noise in that linear light, keyed by `seed`, the clip's index and the run's, at levels drawn per clip; it
    does not touch the plan.  `shake`: a spec "<lo>..<hi>" or "<len>" (speinet_amd.shake): camera-shake blur in that linear light on the
    frames labelled 0, one PSF per frame drawn from `seed`, the clip's index and the run's; it does not touch the plan either.
    `frames`: "runs" (the plan above) or "single" — for ordinary-frame-rate footage: every source frame is its own run of length 1
    (`plan_single`), steady (label 1) with probability `ratio`, shaken otherwise; it needs a shake spec.  `codec`: a spec "<q>" or
    "<lo>..<hi>" (speinet_amd.codec): every blur frame goes through the JPEG-style round trip at a quality drawn per clip from `seed` and
    the clip's index; it does not touch the plan and goes with any light.  -> one dict per clip (name, ratio, frames, labels; with noise
    also its `shot` and `read`, with a codec its `quality`)."""
    light = _light.name(light)
    if light != _light.CODE:
        _light.tables(light)
    _light.check_noise(light, noise)
    noise = _light.noise_name(noise)
    _shake.check(light, shake, frames)
    shake = _shake.name(shake)
    codec = _codec.name(codec)
    clips = []
    for name, files in clip_folders(src_dir):
        try:
            clips.append((name, frames_of(files)))
        except ValueError as e:
            raise ValueError(f"clip {name}: {e}") from None
    plans = plan_dataset([fr.T for _, fr in clips], [ratio] if ratios is None else ratios, seed, threshold, window_range, frames)
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
                _imwrite(pb, b.numpy())
                _imwrite(pg, g.numpy())

            clip_noise = None if noise is None else _light.ClipNoise(noise, seed, k)
            clip_shake = None if shake is None else _shake.ClipShake(shake, seed, k)
            clip_codec = None if codec is None else _codec.ClipCodec(codec, seed, k)
            for i0, blur, gt, _ in synthesize_chunks(fr, (starts, lengths, labels), dev, False, chunk_frames, light, clip_noise, clip_shake,
                                                     clip_codec):
                for m in range(blur.shape[0]):
                    fn = f"{i0 + m:06d}.png"
                    ring.land(lambda b, g, pb=os.path.join(bdir, fn), pg=os.path.join(gdir, fn): save(b, g, pb, pg), blur[m], gt[m])
            ring.drain()
            np.save(os.path.join(out_dir, "label", name + ".npy"), labels)
            done.append({"name": name, "ratio": r, "source_frames": fr.T, "frames": int(labels.size), "labels": labels})
            noisy = ""
            if noise is not None:
                done[-1]["shot"], done[-1]["read"] = _light.noise_draw(noise, seed, k)
                noisy = f", noise shot {done[-1]['shot']:.3g} read {done[-1]['read']:.3g}"
            if shake is not None:
                noisy += f", shake {shake} on {int((labels == 0).sum())} frames"
            if codec is not None:
                done[-1]["quality"] = _codec.quality(codec, seed, k)
                noisy += f", codec quality {done[-1]['quality']}"
            if log:
                log(f"> {name}: {fr.T} sharp frames -> {labels.size} frames, {int(labels.sum())} labelled sharp (ratio {r}, light {light}{noisy})")
    return done


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Make a blur / gt / label training set from folders of sharp high-frame-rate frames on an MI355X")
    p.add_argument("--input", required=True, help="a directory with one folder of sharp frames per clip (PNG / JPG / BMP, file-name order)")
    p.add_argument("--output", required=True, help="directory for blur/<clip>/, gt/<clip>/ and label/<clip>.npy")
    p.add_argument("--ratio", type=float, nargs="+", default=[0.5], help="share of sharp runs; several: one is drawn per clip")
    p.add_argument("--threshold", type=int, default=5, help="a run of at most this many frames is a sharp frame (label 1)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--light", default="code", help="the light the runs are averaged in: code (code values, the reference's sets), srgb or "
                                                   "gamma:<g> (linear light, as an exposure)")
    p.add_argument("--noise", default=None, help="sensor noise added in the linear --light: <shot>:<read>, the shot coefficient (at most 0.05) "
                                                 "and the read deviation (at most 0.1) at full scale 1, each a number or lo..hi (drawn "
                                                 "log-uniformly per clip); not fitted to any camera")
    p.add_argument("--shake", default=None, help="camera-shake blur applied in the linear --light to the frames labelled blurry: the blur "
                                                 "extent in pixels, <len> or <lo>..<hi> within 2..30 (one trajectory PSF is drawn per frame); "
                                                 "not fitted to any camera")
    p.add_argument("--frames", default="runs", choices=_shake.FRAMES, help="runs: average runs of 1..15 frames (high-frame-rate footage); "
                                                                           "single: every frame is its own output frame, shaken unless "
                                                                           "drawn steady with probability --ratio (ordinary footage; needs --shake)")
    p.add_argument("--codec", default=None, help="JPEG-style codec artefacts on every blur frame (never on gt), as the last step: the "
                                                 "quality, <q> or <lo>..<hi> within 1..100 (one is drawn per clip); goes with any --light; "
                                                 "untuned")
    p.add_argument("--device", default="cuda")
    return p


def main(argv=None) -> None:
    p = parser()
    a = p.parse_args(argv)
    try:
        light = _light.name(a.light)
        if light != _light.CODE:
            _light.tables(light)
    except ValueError as e:
        p.error(f"--light: {e}")
    try:
        noise = _light.noise_name(a.noise)
    except ValueError as e:
        p.error(f"--noise: {e}")
    if noise is not None and light == _light.CODE:
        p.error("--noise is added in linear light: pass --light srgb or --light gamma:<g> with it")
    try:
        shake = _shake.name(a.shake)
    except ValueError as e:
        p.error(f"--shake: {e}")
    if shake is not None and light == _light.CODE:
        p.error("--shake is applied in linear light: pass --light srgb or --light gamma:<g> with it")
    if a.frames == "single" and shake is None:
        p.error("--frames single makes every frame its own output frame: pass --shake with it, or every frame comes out sharp")
    try:
        codec = _codec.name(a.codec)
    except ValueError as e:
        p.error(f"--codec: {e}")
    t0 = time.time()
    done = write_dataset(a.input, a.output, ratios=a.ratio, seed=a.seed, threshold=a.threshold, device=a.device,
                         log=lambda s: print(s, flush=True), light=light, noise=noise, shake=shake, frames=a.frames,
                         codec=codec)
    n_src, n_out = sum(d["source_frames"] for d in done), sum(d["frames"] for d in done)
    print(f"# {len(done)} clips, {n_src} sharp frames -> {n_out} frames in {time.time() - t0:.2f}s, light {light}" + (f", noise {noise}" if noise else "")
          + (f", shake {shake}, frames {a.frames}" if shake else "") + (f", codec {codec}" if codec else ""), flush=True)


if __name__ == "__main__":
    main()
