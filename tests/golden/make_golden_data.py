#!/usr/bin/env python3
"""G24: the REFERENCE's training loader (data/videodata_nfs.py VIDEODATA, util/utils.py get_patch / data_augment / np2Tensor /
calc_psnr) on a small synthetic data set, recorded into tests/golden/g24_loader.npz.

The data set is built in a temporary directory: three clips of 9, 14 and 12 frames of 48x64 (smooth content, so the archive stays
small), file stems that are frame numbers — clip 001 jumps from 6 to 20 in the middle — and label patterns that hit every branch of
the reference selection: no sharp frame (000), several sharp frames close together plus one more than 7 frames away (001), exactly one
sharp frame (002).  Training truncates clip 001 to 13 frames (n_frames_per_video = 13); evaluation reads all 14.

Recorded:
  * the frames and labels themselves (tests rebuild the directory tree from them);
  * for EVERY training idx and every evaluation idx: the five file names `_load_file` returns and whether its pre reference (inputs[-2])
    came back all-zero;
  * for random.seed(SEED) and a list of idx, patch_size 40, size_must_mode 4: `__getitem__`'s input tensor [5,3,40,40] and the middle
    frame's gt tensor [3,40,40] (float32, exact), with augmentation on and — after another random.seed(SEED) — off;
  * utils.calc_psnr of a few float pairs, with the pairs.
While generating it is checked that all eight flip / rotate combinations and both a zeroed and a non-zeroed pre reference occur among
the recorded augmented samples (SEED and the idx list were picked so that they do).

`imageio` is not a dependency of this repository: a stand-in module with a PIL-backed `imread` is put into sys.modules before the
reference's loader is imported.  The reference is imported at generation time only; nothing of its text is committed.

Run:  python tests/golden/make_golden_data.py        (needs the reference; writes tests/golden/g24_loader.npz)
"""
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SPEINET_REFERENCE", "/root/reference")
SEED = 161
PATCH = 40
H, W = 48, 64
N_FRAMES_PER_VIDEO = 13
CLIPS = {
    "000": {"numbers": list(range(9)), "labels": [0] * 9},
    "001": {"numbers": list(range(7)) + list(range(20, 27)), "labels": [0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1]},
    "002": {"numbers": list(range(100, 112)), "labels": [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]},
}
TRAIN_IDX = [0, 3, 8, 11, 14, 19, 25, 30, 55]
PLAIN_IDX = [2, 20]


def frame(clip: int, t: int, gt: bool) -> np.ndarray:
    """Smooth, with no symmetry a flip or a rotation could hide behind and no two crops alike."""
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([(3 * x + 5 * y + (x * y) // 16 + 40 * c + 7 * t + 50 * clip + (90 if gt else 0)) % 256 for c in range(3)], axis=-1)
    return img.astype(np.uint8)


def build_tree(root: str) -> dict:
    out = {}
    for ci, (name, spec) in enumerate(CLIPS.items()):
        for kind in ("blur", "gt"):
            os.makedirs(os.path.join(root, kind, name))
        for t, num in enumerate(spec["numbers"]):
            for kind in ("blur", "gt"):
                Image.fromarray(frame(ci, t, kind == "gt")).save(os.path.join(root, kind, name, f"{num:08d}.png"))
        os.makedirs(os.path.join(root, "label"), exist_ok=True)
        np.save(os.path.join(root, "label", name + ".npy"), np.asarray(spec["labels"], dtype=np.int64))
        out[f"numbers/{name}"] = np.asarray(spec["numbers"])
        out[f"labels/{name}"] = np.asarray(spec["labels"], dtype=np.int64)
        out[f"blur/{name}"] = np.stack([frame(ci, t, False) for t in range(len(spec["numbers"]))])
        out[f"gt/{name}"] = np.stack([frame(ci, t, True) for t in range(len(spec["numbers"]))])
    return out


def restate(img: np.ndarray, iy: int, ix: int, h: bool, v: bool, r: bool) -> np.ndarray:
    c = img[iy:iy + PATCH, ix:ix + PATCH]
    if h:
        c = c[:, ::-1]
    if v:
        c = c[::-1]
    if r:
        c = np.rot90(c)
    return c


def main():
    stand_in = types.ModuleType("imageio")
    stand_in.imread = lambda path: np.asarray(Image.open(path))
    sys.modules["imageio"] = stand_in
    sys.path.insert(0, REF)
    from data.videodata_nfs import VIDEODATA
    import util.utils as utils

    with tempfile.TemporaryDirectory() as root:
        res = build_tree(root)
        args = types.SimpleNamespace(n_sequence=3, n_frames_per_video=N_FRAMES_PER_VIDEO, dir_data=root, dir_data_test=root, test_every=1000,
                                     batch_size=2, process=False, patch_size=PATCH, size_must_mode=4, no_augment=False, rgb_range=1,
                                     n_colors=3)
        train = VIDEODATA(args, name="g24", train=True)
        evalset = VIDEODATA(args, name="g24", train=False)
        for tag, ds in (("train", train), ("eval", evalset)):
            names, zero = [], []
            for idx in range(len(ds)):
                inputs, _gts, _labels, filenames = ds._load_file(idx)
                assert inputs.shape[0] == 5 and inputs[:3].any(axis=(1, 2, 3)).all() and inputs[4].any()
                names.append(filenames)
                zero.append(not inputs[-2].any())
            res[f"{tag}/len"], res[f"{tag}/num_frame"] = len(ds), ds.num_frame
            res[f"{tag}/names"], res[f"{tag}/zero_pre"] = np.asarray(names), np.asarray(zero)
        random.seed(SEED)
        aug_in, aug_gt = [], []
        for idx in TRAIN_IDX:
            i, g, _l, _f = train[idx]
            aug_in.append(i.numpy())
            aug_gt.append(g[1].numpy())
        args.no_augment = True
        random.seed(SEED)
        pl_in, pl_gt = [], []
        for idx in PLAIN_IDX:
            i, g, _l, _f = train[idx]
            pl_in.append(i.numpy())
            pl_gt.append(g[1].numpy())
        res.update(seed=SEED, patch=PATCH, n_frames_per_video=N_FRAMES_PER_VIDEO, aug_idx=np.asarray(TRAIN_IDX), aug_input=np.stack(aug_in),
                   aug_gt=np.stack(aug_gt), plain_idx=np.asarray(PLAIN_IDX), plain_input=np.stack(pl_in), plain_gt=np.stack(pl_gt))
        # coverage of the recorded augmented samples: recover the flags from the gt tensor (the gt frame is never zeroed)
        combos, zeros = set(), set()
        for k, idx in enumerate(TRAIN_IDX):
            _inp, gts, _l, names = train._load_file(idx)
            want = np.round(aug_gt[k].transpose(1, 2, 0) * 255).astype(np.uint8)
            hits = [(h, v, r) for h in (0, 1) for v in (0, 1) for r in (0, 1) for iy in range(H - PATCH + 1) for ix in range(W - PATCH + 1)
                    if np.array_equal(restate(gts[1], iy, ix, h, v, r), want)]
            assert len(hits) == 1, (idx, hits)
            combos.add(hits[0])
            zeros.add(bool(res["train/zero_pre"][idx]))
            assert (not aug_in[k][3].any()) == bool(res["train/zero_pre"][idx])
        assert len(combos) == 8, f"only {sorted(combos)} among the recorded samples: pick another SEED / idx list"
        assert zeros == {True, False}, zeros
    # calc_psnr on float pairs (the validation metric: unclamped float output against the float ground truth, shave 4)
    rs = np.random.RandomState(24)
    for k, (h, w, noise) in enumerate(((16, 24, 0.05), (20, 20, 0.3), (16, 24, 0.0))):
        a = rs.rand(1, 3, h, w).astype(np.float32)
        b = (a + noise * rs.randn(1, 3, h, w)).astype(np.float32)
        res[f"psnr/a{k}"], res[f"psnr/b{k}"] = a, b
        res[f"psnr/value{k}"] = float(utils.calc_psnr(torch.from_numpy(a), torch.from_numpy(b), rgb_range=1))
    res["psnr/n"] = 3
    path = os.path.join(HERE, "g24_loader.npz")
    np.savez_compressed(path, **res)
    print(f"g24_loader: train len {res['train/len']}, eval len {res['eval/len']}, {int(res['train/zero_pre'].sum())} zeroed pre references in "
          f"training, {len(TRAIN_IDX)} augmented + {len(PLAIN_IDX)} plain samples, psnr {[round(res[f'psnr/value{k}'], 3) for k in range(3)]}, "
          f"{os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
