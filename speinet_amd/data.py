"""Training data: the reference's blur / gt / label folders as GPU-resident clips, and batches built by one kernel launch.

    ClipSet      the dataset scan and the sample arithmetic of the reference's TRAINING loader (data/videodata_nfs.py), host only
    draw         the random crop / flip / rotate draws of one sample (util/utils.py get_patch + data_augment)
    ClipStore    every frame decoded once, kept as uint8 [T,H,W,3] per clip on the device (or in page-locked host memory)
    Sampler      the order of an epoch, its batches and their draws (host only; splits the batches over the ranks)
    TrainLoader  iterates (input, gt) device tensors: spei_train_batch_u8 (csrc/train_batch.hip) one batch ahead on a side stream

and, beyond the reference (which precomputes its blurry sets), the same loop fed from SHARP footage, the blur synthesised per batch:

    SharpClipSet      folders of sharp frames cut into runs as blurset.write_dataset cuts them, re-drawn for every epoch: epoch e is the
                      set write_dataset(seed = seed + e) would write under the same recipe, as ClipSet would scan it — but
                      nothing is written
    SharpStore        the sharp frames, decoded once, uint8 [T,H,W,3] per clip on the device
    run_records       one batch as spei_run_record: an input frame is a run of sharp frames, the ground truth the run's middle frame
    SharpTrainLoader  TrainLoader on that table and spei_train_batch_runs_u8, which averages each crop's run in its load phase

The reference decodes the five input frames and the ground truth of every sample again for every sample, on DataLoader workers
(`_load_file`).  Here a frame is decoded once; a batch costs the host one small record table and the device one launch.

What is reproduced and what is not: given a sample index and the draws (ix, iy, hflip, vflip, rot90), the tensors are bit-identical
to the reference's `__getitem__` (tests/golden/g24_loader.npz, recorded from the reference).  `draw` consumes a `random.Random` exactly
as `utils.get_patch` and `utils.data_augment` consume Python's global generator for one sample.  The draw STREAM of a reference run is
not reproduced and cannot be: its samples are drawn in DataLoader worker processes, each with its own generator state, in an order
that depends on the workers' scheduling.

Quirks of the reference's training loader that are kept (each pinned by G24), and that differ from the inference harness
(speinet_amd.video.window_plan, which reflect-pads the clip and zeroes both references):
  * the references of the window that starts at frame f are pre[f] and sub[f]: indexed by the window's FIRST frame, not its middle;
  * only the pre reference is zeroed, when its frame number (from the file names) is more than 7 from the window's LAST frame's; the
    sub reference is never zeroed;
  * no reflect padding: a clip of T frames gives T - n_seq + 1 windows; evaluation uses the same path and drops the last two samples
    of the set (`__len__` = num_frame - 2).
"""
from __future__ import annotations

import glob
import os
import random
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional

import numpy as np
import torch

from . import codec as _codec
from . import light as _light
from . import selection
from . import shake as _shake
from .clip import frames_of, imread
from .recipe import Recipe

MAX_GAP = 7
F_HFLIP, F_VFLIP, F_ROT90, F_ZERO = 1, 2, 4, 8                        # SPEI_CROP_* of include/speinet_hip.h
# spei_crop_record
RECORD = np.dtype([("src", "<u8"), ("pitch", "<i4"), ("y0", "<i4"), ("x0", "<i4"), ("flags", "<i4"), ("H", "<i4"), ("W", "<i4")])
assert RECORD.itemsize == 32
# spei_run_record
RUN_RECORD = np.dtype([("src", "<u8"), ("frame_stride", "<i8"), ("pitch", "<i4"), ("y0", "<i4"), ("x0", "<i4"), ("flags", "<i4"),
                       ("H", "<i4"), ("W", "<i4"), ("length", "<i4"), ("avail", "<i4")])
assert RUN_RECORD.itemsize == 48

Sample = namedtuple("Sample", "clip frames pre sub zero_pre names")
Draw = namedtuple("Draw", "ix iy hflip vflip rot90")


def _number(name: str) -> int:
    """Frame number of a `<clip>.<stem>` name (videodata_nfs.py:243-244 extract_frame_number)."""
    return int(name.split(".")[-1])


class Windows:
    """The sample arithmetic of the reference's loader over `self.clips` (dicts with T, names and, with references, pre and sub), given
    `self.train`, `self.n_seq` and `self.references`: what ClipSet scans from a written set and SharpClipSet plans share."""

    def _count(self, what: str) -> None:
        self.n_frames_video = [c["T"] for c in self.clips]
        # videodata_nfs.py:29
        self.num_frame = sum(self.n_frames_video) - (self.n_seq - 1) * len(self.clips)
        if len(self) <= 0:
            raise ValueError(f"{what}: {self.num_frame} windows give no {'training' if self.train else 'evaluation'} sample")

    def __len__(self) -> int:
        return self.num_frame * 2 if self.train else self.num_frame - 2     # videodata_nfs.py:209-213

    def _find_video_num(self, idx: int):
        for i, t in enumerate(self.n_frames_video):                         # videodata_nfs.py:221-226, :231
            n = t - self.n_seq + 1
            if idx < n:
                return i, idx
            idx -= n
        raise IndexError("sample index beyond the last clip")

    def sample(self, idx: int) -> Sample:
        if not 0 <= idx < len(self):
            raise IndexError(f"sample {idx} of {len(self)}")
        if self.train:
            idx %= self.num_frame                                           # videodata_nfs.py:215-217
        v, f = self._find_video_num(idx)
        clip = self.clips[v]
        frames = list(range(f, f + self.n_seq))
        if not self.references:
            return Sample(v, frames, None, None, False, [clip["names"][i] for i in frames])
        # videodata_nfs.py:237-238: the references of the window's FIRST frame
        pre, sub = clip["pre"][f], clip["sub"][f]
        names = [clip["names"][i] for i in frames + [pre, sub]]
        # videodata_nfs.py:254-257: frame_numbers[2] (the window's last frame when n_seq = 3) against the pre reference only
        zero_pre = abs(_number(names[2]) - _number(names[3])) > MAX_GAP
        return Sample(v, frames, pre, sub, zero_pre, names)


class ClipSet(Windows):
    """The scan of `dir_data` (blur/<clip>/*, gt/<clip>/*, label/<clip>.npy) and the samples the reference's loader makes of it.

    train                 training: clips truncated to n_frames_per_video, `len` = 2 * num_frame, idx taken modulo num_frame
    references            True: n_seq window frames + the pre and sub sharp references (model speinet); False: the window alone
                          (model swint, whose trainer ignores the blur map and label data/videodata.py also returns) — labels are
                          then not needed and not read.  The sample arithmetic is videodata_nfs.py's in both cases
    patch                 (optional) the crop size: frames smaller than it are refused here, at scan time
    """

    def __init__(self, dir_data: str, train: bool, n_sequence: int = 3, n_frames_per_video: int = 200, references: bool = True,
                 patch: Optional[int] = None):
        self.dir_data, self.train, self.n_seq, self.references = dir_data, bool(train), int(n_sequence), bool(references)
        if self.references and self.n_seq != 3:
            raise ValueError("samples with references are windows of 3 frames (the reference's zeroing test reads names 2 and 3: videodata_nfs.py:254)")
        # videodata_nfs.py:127-162 _scan: sorted globs, truncated in training
        gt_dirs = sorted(glob.glob(os.path.join(dir_data, "gt", "*")))
        blur_dirs = sorted(glob.glob(os.path.join(dir_data, "blur", "*")))
        if not blur_dirs or len(gt_dirs) != len(blur_dirs):
            raise ValueError(f"{dir_data}: {len(blur_dirs)} clips under blur/ and {len(gt_dirs)} under gt/ (need the same, at least one)")
        label_files: List[Optional[str]] = [None] * len(blur_dirs)
        if self.references:
            if not os.path.isdir(os.path.join(dir_data, "label")):
                # videodata_nfs.py:130-134: the reference's branch for this case uses undefined names
                raise ValueError(f"{dir_data}: no label/ directory (one <clip>.npy of 0/1 sharpness labels per clip).  Make the labels with "
                                 "the detector of `python -m speinet_amd.video` (speinet_amd.detector), or pass references=False")
            label_files = sorted(glob.glob(os.path.join(dir_data, "label", "*")))
            if len(label_files) != len(blur_dirs):
                raise ValueError(f"{dir_data}: {len(label_files)} label files for {len(blur_dirs)} clips")
            for lf, bd in zip(label_files, blur_dirs):         # the reference pairs them by sorted position alone
                if os.path.splitext(os.path.basename(lf))[0] != os.path.basename(bd):
                    raise ValueError(f"{dir_data}: label file {os.path.basename(lf)} stands where clip {os.path.basename(bd)}'s is expected")
        cut = slice(0, n_frames_per_video) if self.train else slice(None)
        self.clips = []
        for gd, bd, lf in zip(gt_dirs, blur_dirs, label_files):
            gts, blurs = sorted(glob.glob(os.path.join(gd, "*")))[cut], sorted(glob.glob(os.path.join(bd, "*")))[cut]
            name = os.path.basename(bd)
            if len(gts) != len(blurs):
                raise ValueError(f"clip {name}: {len(blurs)} blur frames and {len(gts)} gt frames")
            if len(blurs) < self.n_seq:
                raise ValueError(f"clip {name}: {len(blurs)} frames, fewer than one window of {self.n_seq}")
            try:
                fb, fg = frames_of(blurs), frames_of(gts)                # headers only; mixed sizes inside a clip raise here
            except ValueError as e:
                raise ValueError(f"clip {name}: {e}") from None
            if (fb.H, fb.W) != (fg.H, fg.W):
                raise ValueError(f"clip {name}: blur frames are {fb.W}x{fb.H}, gt frames {fg.W}x{fg.H}")
            if patch is not None and (fb.H < patch or fb.W < patch):
                raise ValueError(f"clip {name}: frames are {fb.W}x{fb.H}, smaller than the {patch}x{patch} patch")
            clip = {"name": name, "blur": blurs, "gt": gts, "T": len(blurs), "H": fb.H, "W": fb.W, "labels": None, "pre": None, "sub": None,
                    "names": [name + "." + os.path.splitext(os.path.basename(p))[0] for p in blurs]}       # videodata_nfs.py:241-242
            if self.references:
                lab = np.load(lf)[cut]
                if np.asarray(lab).reshape(-1).size != len(blurs):
                    raise ValueError(f"clip {name}: {np.asarray(lab).reshape(-1).size} labels ({lf}) for {len(blurs)} frames")
                clip["labels"] = [int(v) for v in np.asarray(lab).reshape(-1).tolist()]
                # videodata_nfs.py:154: return_BlurryIndices on the clip's own labels, NOT reflect-padded
                clip["pre"], clip["sub"] = selection.blurry_indices(clip["labels"])
            self.clips.append(clip)
        self._count(dir_data)

    def nbytes(self) -> int:
        """Bytes of every blur and gt frame as uint8 RGB (from the image headers)."""
        return sum(2 * c["T"] * c["H"] * c["W"] * 3 for c in self.clips)


class SharpClipSet(Windows):
    """Folders of sharp frames (`dir_sharp/<clip>/*`, as `python -m speinet_amd.blurset --input` takes them) as a training set whose
    blurry frames are never written.  `plan(epoch)` sets `clips` to what `blurset.write_dataset(dir_sharp, out, ratios=ratios,
    seed=seed + epoch, ...)` followed by `ClipSet(out, True, ...)` would give — per source clip the runs of `blurset.plan_dataset`,
    label 1 for a run of at most `threshold` frames, names `<clip>.<run index, six digits>`, truncated to n_frames_per_video RUNS,
    pre / sub from the truncated labels — so `len()` and `sample(idx)` are ClipSet's on that set.  A virtual clip also carries `starts`
    and `lengths` (the runs' sharp frames) and `source` (its index in `sharp`, the scanned folders).  `light`, `noise`, `shake`, `frames`
    and `codec` are write_dataset's: the recipe (speinet_amd.recipe.Recipe, kept as `recipe`; the five read back as attributes).  Only
    `frames="single"` touches the runs (`blurset.plan_single`); every plan draws, under its own seed, what `Recipe.clip` gives a clip:
    `noise` of a virtual clip (its a, r, A and B), `shake` (its spei_shake_record per run, indexing `psfs`, the plan's one uint32
    [n,33,33] table) and `quality`, each only with its stage.  The constructor plans epoch 0."""

    def __init__(self, dir_sharp: str, ratios=(0.5,), threshold: int = 5, window_range=(1, 15), seed: int = 0, n_sequence: int = 3,
                 n_frames_per_video: int = 200, references: bool = True, patch: Optional[int] = None, light="code", noise=None,
                 shake=None, frames: str = "runs", codec=None):
        from .blurset import clip_folders
        self.dir_data, self.train, self.n_seq, self.references = dir_sharp, True, int(n_sequence), bool(references)
        if self.references and self.n_seq != 3:
            raise ValueError("samples with references are windows of 3 frames (the reference's zeroing test reads names 2 and 3: videodata_nfs.py:254)")
        self.ratios, self.threshold, self.window_range = list(ratios), int(threshold), tuple(window_range)    # checked by plan_dataset
        self.seed, self.n_frames_per_video = int(seed), int(n_frames_per_video)
        self.recipe = Recipe(light, noise, shake, frames, codec)
        self.sharp = []
        for name, files in clip_folders(dir_sharp):
            try:
                fr = frames_of(files)                                        # headers only; mixed sizes inside a clip raise here
            except ValueError as e:
                raise ValueError(f"clip {name}: {e}") from None
            if patch is not None and (fr.H < patch or fr.W < patch):
                raise ValueError(f"clip {name}: frames are {fr.W}x{fr.H}, smaller than the {patch}x{patch} patch")
            self.sharp.append({"name": name, "files": files, "T": fr.T, "H": fr.H, "W": fr.W})
        self.plan(0)

    light, noise, shake, frames, codec = (property(lambda self, f=f: getattr(self.recipe, f)) for f in Recipe._fields)

    def plan(self, epoch: int) -> None:
        from .blurset import plan_dataset
        plans = plan_dataset([c["T"] for c in self.sharp], self.ratios, self.seed + epoch, self.threshold, self.window_range, self.frames)
        clips, psfs, n_psf = [], [], 0
        for k, (src, (ratio, (starts, lengths, labels))) in enumerate(zip(self.sharp, plans)):
            cut = slice(0, self.n_frames_per_video)
            starts, lengths, labels = starts[cut], lengths[cut], [int(v) for v in labels[cut]]
            if len(labels) < self.n_seq:
                raise ValueError(f"clip {src['name']}: the plan of epoch {epoch} cuts its {src['T']} frames into {len(labels)} runs, fewer "
                                 f"than one window of {self.n_seq}")
            clip = {"name": src["name"], "source": k, "ratio": ratio, "T": len(labels), "H": src["H"], "W": src["W"], "starts": starts,
                    "lengths": lengths, "labels": labels, "pre": None, "sub": None,
                    "names": [f"{src['name']}.{m:06d}" for m in range(len(labels))]}
            if self.references:
                clip["pre"], clip["sub"] = selection.blurry_indices(labels)
            draw = self.recipe.clip(self.seed + epoch, k)
            shaken = draw.shake(np.arange(len(labels)), labels, base=n_psf)      # the clip's records index the plan's one table
            if shaken is not None:
                psfs.append(shaken[1])
                n_psf += shaken[1].shape[0]
            made = {"noise": draw.noise, "shake": shaken and shaken[0], "quality": draw.quality}
            clip.update({key: v for key, v in made.items() if v is not None})
            clips.append(clip)
        self.psfs = np.concatenate(psfs) if psfs else None                   # uint32 [n,33,33]: every PSF of the plan (SharpTrainLoader uploads it once)
        self.clips, self.epoch = clips, epoch
        self._count(f"{self.dir_data} (epoch {epoch})")

    def summary(self) -> str:
        """One line on the current plan: its runs, how many are labelled sharp and the light they are averaged in."""
        runs, sharp = sum(c["T"] for c in self.clips), sum(sum(c["labels"]) for c in self.clips)
        q = [c.get("quality") for c in self.clips]
        said = self.recipe.describe(shake=lambda: f"{self.shake} on {sum(int((c['shake']['radius'] > 0).sum()) for c in self.clips)} runs "
                                                  f"(frames {self.frames})",
                                    codec=lambda: f"{self.codec} (qualities {min(q)}..{max(q)})")
        return f"Plan {self.epoch} of {self.dir_data}: {runs} runs of {sum(c['T'] for c in self.sharp)} sharp frames, {sharp} labelled sharp, {said}"

    def noise_lines(self) -> list:
        """One line per clip on the levels the current plan drew for it; empty without noise."""
        return [f"> {c['name']}: noise shot {c['noise'][0]:.3g} read {c['noise'][1]:.3g}" for c in self.clips if self.noise is not None]

    def nbytes(self) -> int:
        """Bytes of every sharp frame as uint8 RGB (from the image headers)."""
        return sum(c["T"] * c["H"] * c["W"] * 3 for c in self.sharp)


def draw(rng: random.Random, ih: int, iw: int, patch: int, augment: bool = True) -> Draw:
    """The draws of one training sample, consumed from `rng` as the reference consumes Python's global generator: get_patch's
    `ix = randrange(0, iw - ip + 1)`, then `iy` (util/utils.py:17-18), then — unless `--no_augment` — data_augment's three
    `random() < 0.5` for hflip, vflip, rot90, all three always drawn (util/utils.py:51-53)."""
    ix = rng.randrange(0, iw - patch + 1)
    iy = rng.randrange(0, ih - patch + 1)
    if not augment:
        return Draw(ix, iy, False, False, False)
    hflip = rng.random() < 0.5
    vflip = rng.random() < 0.5
    rot90 = rng.random() < 0.5
    return Draw(ix, iy, hflip, vflip, rot90)


def usable_cpus() -> int:
    """CPUs this process may use (its affinity mask, and OMP_NUM_THREADS where a job scheduler set it) — not the machine's count."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    env = os.environ.get("OMP_NUM_THREADS", "")
    if env.isdigit() and int(env) > 0:
        n = min(n, int(env))
    return max(1, min(n, 32))


class ClipStore:
    """Every frame of a ClipSet decoded once (PIL, on a thread pool) and kept as one contiguous uint8 [T,H,W,3] tensor per clip,
    blur and gt: `residency="device"` on `device`, `residency="host"` in page-locked host memory.

    The bytes are summed from the image headers BEFORE anything is loaded and compared with `budget_bytes` (device residency; default
    half of the device's free memory, read once, here).  Over budget is a MemoryError: the mode is never switched silently."""

    def __init__(self, clipset: ClipSet, residency: str = "device", device="cuda:0", budget_bytes: Optional[int] = None, log=print):
        if residency not in ("device", "host"):
            raise ValueError(f"residency must be 'device' or 'host', got {residency!r}")
        self.clipset, self.residency, self.device = clipset, residency, torch.device(device)
        self.nbytes = clipset.nbytes()
        if residency == "device":
            self._admit(budget_bytes, "use residency='host' (page-locked host memory, patches uploaded per batch)")
        self.blur, self.gt = [], []
        with ThreadPoolExecutor(max_workers=usable_cpus()) as pool:
            for clip in clipset.clips:
                for key, dst in (("blur", self.blur), ("gt", self.gt)):
                    dst.append(self._load(pool, clip, clip[key]))
        if log is not None:
            log(f"ClipStore: {len(clipset.clips)} clips, {sum(c['T'] for c in clipset.clips)} blur/gt pairs, {self.nbytes} bytes, "
                f"residency {residency}")

    def _admit(self, budget_bytes: Optional[int], otherwise: str) -> None:
        if budget_bytes is None:
            budget_bytes = torch.cuda.mem_get_info(self.device)[0] // 2
        if self.nbytes > budget_bytes:
            raise MemoryError(f"{self.clipset.dir_data}: the clips are {self.nbytes} bytes as uint8, the budget for device residency is "
                              f"{budget_bytes} bytes; {otherwise}")

    def _load(self, pool, clip, paths) -> torch.Tensor:
        T, H, W = clip["T"], clip["H"], clip["W"]
        host = torch.empty((T, H, W, 3), dtype=torch.uint8, pin_memory=self.residency == "host")
        arr = host.numpy()

        def one(i):
            img = imread(paths[i])
            if img.shape != (H, W, 3):
                raise ValueError(f"{paths[i]} decodes to {img.shape}, its header said {W}x{H}")
            arr[i] = img
        list(pool.map(one, range(T)))
        return host if self.residency == "host" else host.to(self.device)


class SharpStore(ClipStore):
    """Every sharp frame of a SharpClipSet decoded once and kept as one uint8 [T,H,W,3] device tensor per source clip (`frames`, in the
    order of `clipset.sharp`), under ClipStore's budget rule.  Device residency only: a record reads up to 15 rectangles."""

    def __init__(self, clipset: "SharpClipSet", device="cuda:0", budget_bytes: Optional[int] = None, log=print):
        self.clipset, self.residency, self.device = clipset, "device", torch.device(device)
        self.nbytes = clipset.nbytes()
        self._admit(budget_bytes, "a set that does not fit is trained from disk: write it once with `python -m speinet_amd.blurset` and "
                                  "pass `--dir_data` (host residency is built for written sets only)")
        with ThreadPoolExecutor(max_workers=usable_cpus()) as pool:
            self.frames = [self._load(pool, clip, clip["files"]) for clip in clipset.sharp]
        if log is not None:
            log(f"SharpStore: {len(clipset.sharp)} clips, {sum(c['T'] for c in clipset.sharp)} sharp frames, {self.nbytes} bytes, "
                f"residency device")


class Sampler:
    """The order of an epoch and its draws, on the host.  The permutation is a `torch.randperm(len)` from a generator seeded once with
    `seed`; the draws come from one `random.Random(seed)`, consumed in the permutation's order for EVERY sample of the epoch, so all
    ranks hold the same plan; rank r of `world` takes every world-th batch of it (batch k with k % world == r)."""

    def __init__(self, clipset: ClipSet, batch: int, patch: int = 200, seed: int = 1, augment: bool = True,
                 rank: Optional[int] = None, world: Optional[int] = None):
        if batch <= 0 or patch <= 0 or patch % 4:
            raise ValueError(f"batch {batch} must be positive and patch {patch} a positive multiple of 4")
        for c in clipset.clips:
            if c["H"] < patch or c["W"] < patch:
                raise ValueError(f"clip {c['name']}: frames are {c['W']}x{c['H']}, smaller than the {patch}x{patch} patch")
        if rank is None or world is None:
            import torch.distributed as dist
            on = dist.is_available() and dist.is_initialized()
            rank, world = (dist.get_rank(), dist.get_world_size()) if on else (0, 1)
        self.clipset, self.batch, self.patch, self.augment, self.rank, self.world = clipset, batch, patch, augment, rank, world
        self.gen = torch.Generator().manual_seed(seed)
        self.rng = random.Random(seed)

    def n_batches(self) -> int:
        """Batches of one epoch over all ranks (the last may be partial: DataLoader's drop_last=False)."""
        return -(-len(self.clipset) // self.batch)

    def __len__(self) -> int:
        return len(range(self.rank, self.n_batches(), self.world))

    def epoch(self) -> list:
        """This rank's batches of the next epoch: a list of lists of (sample index, Sample, Draw)."""
        cs = self.clipset
        order = torch.randperm(len(cs), generator=self.gen).tolist()
        items = []
        for idx in order:
            s = cs.sample(idx)
            c = cs.clips[s.clip]
            items.append((idx, s, draw(self.rng, c["H"], c["W"], self.patch, self.augment)))
        batches = [items[i:i + self.batch] for i in range(0, len(items), self.batch)]
        return batches[:self.n_batches()][self.rank::self.world]


class SharpSampler(Sampler):
    """Sampler over a SharpClipSet: `epoch()` number e (0, 1, ...) first makes the set `plan(e)` (`replan=False`: plan 0 every time), then
    draws order and crops as Sampler does, so calling `epoch()` once per finished epoch — Fit's resume loop — lands on the right plan.
    The number of runs changes with the plan: with `world` > 1 an epoch is cut to the largest number of batches that divides by `world`
    (all ranks still consume the same draws), and `n_batches()` reports that number for the plan in force."""

    def __init__(self, clipset: "SharpClipSet", batch: int, patch: int = 200, seed: int = 1, augment: bool = True,
                 rank: Optional[int] = None, world: Optional[int] = None, replan: bool = True):
        super().__init__(clipset, batch, patch, seed, augment, rank, world)
        self.replan, self.epochs = replan, 0

    def n_batches(self) -> int:
        n = super().n_batches()
        return n - n % self.world

    def epoch(self) -> list:
        self.clipset.plan(self.epochs if self.replan else 0)
        self.epochs += 1
        return super().epoch()


def batch_records(clipset: ClipSet, store: ClipStore, items, patch: int) -> np.ndarray:
    """The record table of one batch for frames that live where `store` keeps them: B * F input records (F = n_seq + 2, or n_seq
    without references; sample-major), then B gt records (the middle frame's).  All frames of a sample share offsets and flags; only a
    pre reference carries the zero flag.  One row of numpy writes per sample, not per record."""
    n_seq, refs = clipset.n_seq, clipset.references
    F = n_seq + (2 if refs else 0)
    B = len(items)
    rec = np.zeros(B * F + B, dtype=RECORD)
    inp, gt = rec[:B * F].reshape(B, F), rec[B * F:]
    frames = np.empty((B, F), dtype=np.uint64)
    shared = np.empty((B, 7), dtype=np.int64)             # per sample: H, W, y0, x0, flags, clip, the pre reference's zero flag
    for b, (_idx, s, d) in enumerate(items):
        c = clipset.clips[s.clip]
        frames[b] = list(s.frames) + ([s.pre, s.sub] if refs else [])
        flags = (F_HFLIP if d.hflip else 0) | (F_VFLIP if d.vflip else 0) | (F_ROT90 if d.rot90 else 0)
        shared[b] = (c["H"], c["W"], d.iy, d.ix, flags, s.clip, F_ZERO if (refs and s.zero_pre) else 0)
    H, W = shared[:, 0], shared[:, 1]
    fbytes = (H * W * 3).astype(np.uint64)
    blur_base = np.array([store.blur[c].data_ptr() for c in shared[:, 5]], dtype=np.uint64)
    gt_base = np.array([store.gt[c].data_ptr() for c in shared[:, 5]], dtype=np.uint64)
    inp["src"] = blur_base[:, None] + frames * fbytes[:, None]
    gt["src"] = gt_base + frames[:, n_seq // 2] * fbytes
    for part, col in ((inp, lambda v: v[:, None]), (gt, lambda v: v)):
        part["pitch"], part["y0"], part["x0"], part["flags"] = col(W * 3), col(shared[:, 2]), col(shared[:, 3]), col(shared[:, 4])
        part["H"], part["W"] = col(H), col(W)
    if refs:
        inp["flags"][:, n_seq] |= shared[:, 6].astype(np.int32)
    return rec


def run_records(clipset: SharpClipSet, store: SharpStore, items) -> np.ndarray:
    """`batch_records` for a SharpClipSet under its CURRENT plan, as spei_run_record: B * F input records — the window's runs and, with
    references, the pre and sub runs (only pre may carry the zero flag) — then B gt records: a run of length 1 at the middle run's middle
    frame, start + length // 2.  `avail` counts the sharp frames from the record's first frame to the end of its clip."""
    n_seq, refs = clipset.n_seq, clipset.references
    F = n_seq + (2 if refs else 0)
    B = len(items)
    rec = np.zeros(B * F + B, dtype=RUN_RECORD)
    inp, gt = rec[:B * F].reshape(B, F), rec[B * F:]
    for b, (_idx, s, d) in enumerate(items):
        c = clipset.clips[s.clip]
        sharp = store.frames[c["source"]]                   # uint8 [T,H,W,3]
        T, H, W, _ = sharp.shape
        runs = np.asarray(list(s.frames) + ([s.pre, s.sub] if refs else []), dtype=np.int64)
        start, length = c["starts"][runs], c["lengths"][runs]
        mid = start[n_seq // 2] + length[n_seq // 2] // 2
        flags = (F_HFLIP if d.hflip else 0) | (F_VFLIP if d.vflip else 0) | (F_ROT90 if d.rot90 else 0)
        base, fstride = sharp.data_ptr(), sharp.stride(0)
        for part in (inp[b], gt[b:b + 1]):
            part["frame_stride"], part["pitch"], part["y0"], part["x0"], part["flags"] = fstride, sharp.stride(1), d.iy, d.ix, flags
            part["H"], part["W"] = H, W
        inp[b]["src"], inp[b]["length"], inp[b]["avail"] = (base + start * fstride).astype(np.uint64), length, T - start
        gt[b]["src"], gt[b]["length"], gt[b]["avail"] = base + int(mid) * fstride, 1, T - mid
        if refs and s.zero_pre:
            inp[b]["flags"][n_seq] |= F_ZERO
    return rec


def run_noise_records(clipset: SharpClipSet, items) -> np.ndarray:
    """The spei_noise_record table beside `run_records`' table, record for record: the run's index in its clip's plan, the clip's index
    in the scanned folders and the levels the plan drew for the clip.  A gt record (a run of length 1: no noise) carries its window's
    middle run."""
    n_seq, refs = clipset.n_seq, clipset.references
    F = n_seq + (2 if refs else 0)
    B = len(items)
    rec = np.zeros(B * F + B, dtype=_light.NOISE_RECORD)
    inp, gt = rec[:B * F].reshape(B, F), rec[B * F:]
    for b, (_idx, s, _d) in enumerate(items):
        c = clipset.clips[s.clip]
        inp[b]["run"] = list(s.frames) + ([s.pre, s.sub] if refs else [])
        gt[b]["run"] = s.frames[n_seq // 2]
        for part in (inp[b], gt[b:b + 1]):
            part["clip"], part["A"], part["B"] = c["source"], c["noise"][2], c["noise"][3]
    return rec


def run_shake_records(clipset: SharpClipSet, items) -> np.ndarray:
    """The spei_shake_record table beside `run_records`' table, record for record: the record the plan made for the run (its PSF's index
    in `clipset.psfs`, radius and q16).  A gt record (a run of length 1 on the copy path) carries the delta: radius 0."""
    n_seq, refs = clipset.n_seq, clipset.references
    F = n_seq + (2 if refs else 0)
    B = len(items)
    rec = np.zeros(B * F + B, dtype=_shake.SHAKE_RECORD)
    rec["q16"] = 65536
    inp = rec[:B * F].reshape(B, F)
    for b, (_idx, s, _d) in enumerate(items):
        inp[b] = clipset.clips[s.clip]["shake"][list(s.frames) + ([s.pre, s.sub] if refs else [])]
    return rec


def run_codec_records(clipset: SharpClipSet, items, rec: np.ndarray) -> np.ndarray:
    """The spei_codec_record table beside the INPUT records of `run_records`' table `rec`, record for record: the tables of the clip's
    quality (index quality - 1 of `codec.all_tables`), the grid offsets oy = y0 % 16, ox = x0 % 16 — the full frame's grid — and the table
    record's flags.  Ground truth is never coded: it has no record."""
    F = clipset.n_seq + (2 if clipset.references else 0)
    B = len(items)
    out = np.zeros(B * F, dtype=_codec.CODEC_RECORD)
    inp = rec[:B * F]
    out["oy"], out["ox"], out["flags"] = inp["y0"] % 16, inp["x0"] % 16, inp["flags"]
    out["qtab"] = np.repeat([clipset.clips[s.clip]["quality"] - 1 for _idx, s, _d in items], F)
    return out


class TrainLoader:
    """Iterates (input [B,F,3,P,P], gt [B,3,P,P]) fp32 device tensors of one epoch per `iter()`.

    A batch is made by `_launch`: the record table is written into one slot of a small ring of page-locked buffers, copied to the
    device, and the batch is built by ONE launch of spei_train_batch_u8, all on a side stream; the consumer's stream waits on the
    batch's event.  With `prefetch` the whole of `_launch` for batch k + 1 — the host part (the table, and for host residency the
    staging copies) as well as the launch — runs on a worker thread that is started when batch k is handed out, so it overlaps step k
    on both the host and the device; without it, `_launch` runs in the consumer's thread when the batch is asked for.  The output
    tensors are allocated on the side stream and handed to the consumer's stream with `record_stream`.  A slot is rewritten only after
    its event has completed (the discipline of clip.FrameCache).  Host residency: the patch rectangles of the batch are first copied,
    row range by row range, into the slot's page-locked staging buffer and uploaded with one asynchronous copy; the records then point
    into the uploaded rectangles (offsets rebased to 0) and go through the same kernel, so the results are bit-identical."""
    RING = 3
    RECORD = RECORD                  # the table's record type; SharpTrainLoader's is RUN_RECORD

    def __init__(self, clipset: ClipSet, store: ClipStore, batch: int, patch: int = 200, seed: int = 1, augment: bool = True,
                 rgb_range: float = 1, prefetch: bool = True, rank: Optional[int] = None, world: Optional[int] = None, sampler=None):
        from . import ops
        if store.clipset is not clipset:
            raise ValueError("the ClipStore was loaded from another ClipSet")
        self.clipset, self.store, self.batch, self.patch, self.rgb_range, self.prefetch = clipset, store, batch, patch, float(rgb_range), prefetch
        self.sampler = Sampler(clipset, batch, patch, seed, augment, rank, world) if sampler is None else sampler
        self.device = store.device
        self.F = clipset.n_seq + (2 if clipset.references else 0)
        self.ctx = ops.Ctx(device=self.device)
        n_rec = batch * (self.F + 1)
        with torch.cuda.device(self.device):
            self.side = torch.cuda.Stream(device=self.device)
            self.slots = []
            for _ in range(self.RING):
                slot = {"host": torch.empty(n_rec * self.RECORD.itemsize, dtype=torch.uint8, pin_memory=True),
                        "dev": torch.empty(n_rec * self.RECORD.itemsize, dtype=torch.uint8, device=self.device), "event": None}
                if store.residency == "host":
                    slot["stage"] = torch.empty((n_rec, patch, patch, 3), dtype=torch.uint8, pin_memory=True)
                    slot["stage_dev"] = torch.empty((n_rec, patch, patch, 3), dtype=torch.uint8, device=self.device)
                self.slots.append(slot)
        self.launched = 0
        self.worker = ThreadPoolExecutor(max_workers=1, thread_name_prefix="train-batch") if prefetch else None

    def __len__(self) -> int:
        return len(self.sampler)

    def _records(self, items) -> np.ndarray:
        return batch_records(self.clipset, self.store, items, self.patch)

    def _build(self, *args) -> None:
        self.ctx.train_batch(*args)

    def _launch(self, items):
        """Build one batch on the side stream (from whichever thread calls); returns (input, gt, event)."""
        P, F, B = self.patch, self.F, len(items)
        with torch.cuda.device(self.device), torch.cuda.stream(self.side):
            slot = self.slots[self.launched % self.RING]
            self.launched += 1
            if slot["event"] is not None:
                slot["event"].synchronize()                   # the launch issued RING batches ago: long finished
            rec = self._records(items)
            n = rec.size
            inp = torch.empty((B, F, 3, P, P), device=self.device)         # blocks of the side stream: see __iter__
            gt = torch.empty((B, 3, P, P), device=self.device)
            if self.store.residency == "host":
                stage = slot["stage"]
                for r in range(n):
                    if rec["flags"][r] & F_ZERO:
                        continue
                    b = r // F if r < B * F else r - B * F
                    _idx, s, d = items[b]
                    if r < B * F:
                        k = r - b * F
                        f = (list(s.frames) + [s.pre, s.sub])[k]
                        src = self.store.blur[s.clip]
                    else:
                        f, src = s.frames[self.clipset.n_seq // 2], self.store.gt[s.clip]
                    stage[r].copy_(src[f, d.iy:d.iy + P, d.ix:d.ix + P])
                slot["stage_dev"][:n].copy_(stage[:n], non_blocking=True)
                base = slot["stage_dev"].data_ptr()
                rec["src"] = np.uint64(base) + np.arange(n, dtype=np.uint64) * np.uint64(P * P * 3)
                rec["pitch"], rec["y0"], rec["x0"], rec["H"], rec["W"] = P * 3, 0, 0, P, P
            host = slot["host"][:n * self.RECORD.itemsize]
            host.numpy()[...] = rec.view(np.uint8).reshape(-1)
            dev = slot["dev"][:n * self.RECORD.itemsize]
            dev.copy_(host, non_blocking=True)
            self._build(dev, host, B * F, B, inp, gt, P, self.rgb_range)
            ev = torch.cuda.Event()
            ev.record(self.side)
            slot["event"] = ev
        return inp, gt, ev

    def __iter__(self):
        batches = self.sampler.epoch()
        submit = self.worker.submit if self.prefetch else None
        pending = submit(self._launch, batches[0]) if batches and self.prefetch else None
        try:
            for k, items in enumerate(batches):
                if self.prefetch:
                    inp, gt, ev = pending.result()
                    # batch k + 1: table, staging and launch on the worker thread, while the consumer runs step k
                    pending = submit(self._launch, batches[k + 1]) if k + 1 < len(batches) else None
                else:
                    inp, gt, ev = self._launch(items)
                main = torch.cuda.current_stream(self.device)
                main.wait_event(ev)
                inp.record_stream(main)                       # allocated on the side stream, used (and later freed) by the consumer's
                gt.record_stream(main)
                yield inp, gt
        finally:
            if pending is not None:                           # an abandoned epoch: let the launch in flight finish before the ring moves on
                pending.result()


class SharpTrainLoader(TrainLoader):
    """TrainLoader fed from sharp footage: the table is `run_records`, the launch spei_train_batch_runs_u8, which averages the run of
    every crop in its load phase; ring, side stream and prefetch thread are TrainLoader's.  Every `iter()` is one epoch under its own
    plan (SharpSampler; `replan=False`: plan 0 throughout).  All launches of an epoch are issued before the next one is planned.  The
    set's recipe picks the launch (`Ctx.train_batch_runs`: _light_, _noise_ or _shake_u8; with a codec spei_train_batch_codec_f32 follows
    in place on the input, on the same stream).  Uploaded here, once: the light's tables, the gauss table, the tables of all 100
    qualities; once per plan, ahead of its first launch: the plan's PSF table.  The records of the active stages (`STAGES`) are built
    with the run records, one batch ahead, under the seed of the plan in force, and travel through rings of their own beside the table's."""
    RECORD = RUN_RECORD
    # key, its records beside `run_records`' table, their type, records per sample beyond the F inputs (gt is never coded)
    STAGES = (("noise", lambda cs, items, rec: run_noise_records(cs, items), _light.NOISE_RECORD, 1),
              ("shake", lambda cs, items, rec: run_shake_records(cs, items), _shake.SHAKE_RECORD, 1),
              ("codec", run_codec_records, _codec.CODEC_RECORD, 0))

    def __init__(self, clipset: SharpClipSet, store: SharpStore, batch: int, patch: int = 200, seed: int = 1, augment: bool = True,
                 rgb_range: float = 1, prefetch: bool = True, rank: Optional[int] = None, world: Optional[int] = None, replan: bool = True):
        super().__init__(clipset, store, batch, patch, seed, augment, rgb_range, prefetch, rank, world,
                         sampler=SharpSampler(clipset, batch, patch, seed, augment, rank, world, replan))
        recipe = self.recipe = clipset.recipe
        self.stages = [row for row in self.STAGES if getattr(recipe, row[0]) is not None]
        self._psfs, self._psfs_epoch = None, None               # the plan's PSF table on the device and the plan it belongs to
        with torch.cuda.device(self.device):
            if recipe.light != _light.CODE:
                _light.device_tables(recipe.light, self.device)
            if recipe.noise is not None:
                _light.device_gauss(self.device)
            if recipe.codec is not None:
                self._qtabs = _codec.device_qtabs(_codec.all_tables(), self.device)
            for key, _make, dtype, extra in self.stages:
                nb = batch * (self.F + extra) * dtype.itemsize
                for slot in self.slots:
                    slot[key + "_host"] = torch.empty(nb, dtype=torch.uint8, pin_memory=True)
                    slot[key + "_dev"] = torch.empty(nb, dtype=torch.uint8, device=self.device)

    def _records(self, items) -> np.ndarray:
        rec = run_records(self.clipset, self.store, items)
        # consumed by the `_build` of the same `_launch`: the active stages' records and the seed of the plan in force
        self._staged = {key: make(self.clipset, items, rec) for key, make, _dtype, _extra in self.stages}, self.clipset.seed + self.clipset.epoch
        return rec

    def _build(self, *args) -> None:
        slot = self.slots[(self.launched - 1) % self.RING]     # `_launch`'s slot: its event has been waited for
        recs, seed = self._staged

        def ring(key: str):
            """The stage's records through the slot's page-locked buffer into its device buffer; -> (device, host) views."""
            rec = recs[key]
            host, dev = slot[key + "_host"][:rec.nbytes], slot[key + "_dev"][:rec.nbytes]
            host.numpy()[...] = rec.view(np.uint8).reshape(-1)
            dev.copy_(host, non_blocking=True)
            return dev, host

        noise = ring("noise") + (seed,) if "noise" in recs else None
        if "shake" in recs and self._psfs_epoch != self.clipset.epoch:   # once per plan, on the side stream, ahead of the plan's first launch
            self._psfs, self._psfs_epoch = _shake.device_psfs(self.clipset.psfs, self.device), self.clipset.epoch
        shake = ring("shake") + (self._psfs,) if "shake" in recs else None
        self.ctx.train_batch_runs(*args, light=self.recipe.light, noise=noise, shake=shake)
        if "codec" in recs:                                    # in place on the input the launch above wrote, on the same stream
            _table, _host, n_in, _n_gt, inp, _gt, P, rgb_range = args
            self.ctx.train_batch_codec(inp, n_in, P, rgb_range, *ring("codec"), self._qtabs)
