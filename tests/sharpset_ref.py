"""Numpy restatement of one output frame of spei_train_batch_runs_u8 (csrc/train_batch.hip), and helpers the sharp-footage tests
share.  Not a test."""
import os
import random

import numpy as np


def run_patch(frames_u8, start, length, y0, x0, P, hflip, vflip, rot90, zero, rgb_range):
    """frames_u8 [T,H,W,3] -> float32 [3,P,P]: the per-byte floor of the mean of frames start .. start + length - 1 in integer
    arithmetic, then crop, [:, ::-1] if hflip, [::-1, :] if vflip, np.rot90 if rot90 — the reference's order, as the header of
    train_batch.hip states it — then np.float32(u) * np.float32(rgb_range / 255)."""
    if zero:
        return np.zeros((3, P, P), np.float32)
    u = np.floor(frames_u8[start:start + length].astype(np.int64).sum(axis=0) / length).astype(np.int64)
    assert np.array_equal(u, frames_u8[start:start + length].astype(np.int64).sum(axis=0) // length)
    img = u[y0:y0 + P, x0:x0 + P]
    if hflip:
        img = img[:, ::-1]
    if vflip:
        img = img[::-1, :]
    if rot90:
        img = np.rot90(img)
    return np.ascontiguousarray(img.transpose(2, 0, 1)).astype(np.float32) * np.float32(rgb_range / 255)


def moving_clip(seed, T, h, w):
    """T uint8 frames of a drifting pattern with noise: consecutive frames differ, so a run's mean is not one of its frames."""
    r = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = np.empty((T, h, w, 3), np.uint8)
    for t in range(T):
        base = 128 + 70 * np.sin(0.5 * (xx + 1.3 * t) + seed) * np.cos(0.3 * yy) + 40 * np.sin(0.8 * (xx + yy) - 0.4 * t)
        out[t] = np.clip(np.stack([base, 0.9 * base + 10, 1.05 * base - 8], axis=-1) + 6 * r.randn(h, w, 3), 0, 255)
    return out


def write_sharp(root, clips):
    """clips: name -> uint8 [T,H,W,3]; writes root/<name>/<i:05d>.png."""
    from PIL import Image
    for name, frames in clips.items():
        os.makedirs(os.path.join(root, name))
        for i, f in enumerate(frames):
            Image.fromarray(f).save(os.path.join(root, name, f"{i:05d}.png"), compress_level=1)
    return root


def replay(lengths, ratios, seed, threshold=5, window_range=(1, 15)):
    """blurset.write_dataset's draws, written out by hand on one random.Random(seed): per clip (in sorted order) rng.choice(ratios) only
    when there are several, then generate_blurry_sequence's label / randint pairs.  -> [(ratio, starts, lengths, labels)]."""
    rng = random.Random(seed)
    out = []
    for n in lengths:
        ratio = rng.choice(ratios) if len(ratios) > 1 else ratios[0]
        at, runs = 0, []
        while at < n:
            label = int(rng.random() < ratio or n - at <= threshold)
            size = min(rng.randint(window_range[0], threshold) if label else rng.randint(threshold + 1, window_range[1]), n - at)
            runs.append((at, size, label))
            at += size
        out.append((ratio,) + tuple(np.asarray(col, np.int64) for col in zip(*runs)))
    return out


def write_set_numpy(out, clips, ratios, seed, threshold=5):
    """The set blurset.write_dataset(seed=seed) writes from `clips` (name -> frames), made with numpy: np.mean(...).astype(np.uint8),
    six-digit names, labels from the replayed plan."""
    from PIL import Image
    names = sorted(clips)
    os.makedirs(os.path.join(out, "label"))
    for name, (_ratio, starts, lengths, labels) in zip(names, replay([len(clips[n]) for n in names], list(ratios), seed, threshold)):
        for kind in ("blur", "gt"):
            os.makedirs(os.path.join(out, kind, name))
        for m, (s, n) in enumerate(zip(starts, lengths)):
            blur = np.mean(clips[name][s:s + n], axis=0).astype(np.uint8)
            Image.fromarray(blur).save(os.path.join(out, "blur", name, f"{m:06d}.png"), compress_level=1)
            Image.fromarray(clips[name][s + n // 2]).save(os.path.join(out, "gt", name, f"{m:06d}.png"), compress_level=1)
        np.save(os.path.join(out, "label", name + ".npy"), labels)
    return out
