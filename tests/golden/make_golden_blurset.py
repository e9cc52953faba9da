#!/usr/bin/env python3
"""G25 / G26 — golden vectors for the data-set synthesis and the detector fit, produced by the REFERENCE's own functions in
LD_detector/sharp_detector_params_estimation_parallel.py (generate_blurry_sequence :50-76, estimate_parameters :239-250).

  g25_blurset.npz       a seeded clip of 60 uint8 frames 24x36 and, per (ratio, seed), generate_blurry_sequence's blurry frames
                        (float32, as returned), labels and gt frames (integer-valued, stored as uint8)
  g26_detector_fit.npz  a feature matrix of the six measures (oracle.detector_oracle.features on the truncated blurry frames of
                        synthetic clips whose motion and noise vary, so that the classes overlap), its labels, coef_ / intercept_ /
                        n_iter_ of estimate_parameters(...)[0] (sklearn LogisticRegression()), and the hold-out rows of
                        train_test_split(test_size=0.1, random_state=4000) (:273)

The script's absent imports are stubbed; it also calls torch.cuda.set_device(6) at import, which is stubbed for the import only."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_golden import REF  # noqa: E402

PAIRS = ((0.5, 4000), (0.1, 7))


def import_estimation():
    for n in ("tqdm", "ptwt", "pywt", "torchvision", "imageio", "pandas"):
        try:
            importlib.import_module(n)
        except Exception:
            m = types.ModuleType(n)
            m.tqdm = lambda it, **k: it
            m.wavedec2 = None
            sys.modules[n] = m
    sys.path.insert(0, os.path.join(REF, "LD_detector"))
    keep = torch.cuda.set_device
    torch.cuda.set_device = lambda *a, **k: None
    try:
        import sharp_detector_params_estimation_parallel as est
    finally:
        torch.cuda.set_device = keep
    return est


def moving_clip(r, T, h, w, speed, noise):
    """T uint8 frames [h,w,3]: a texture that moves `speed` pixels per frame, plus per-frame noise."""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ph = r.uniform(0, 6.28, size=4)
    fr = []
    for t in range(T):
        x = xx + speed * t
        base = 128 + 60 * np.sin(0.55 * x + ph[0]) * np.cos(0.35 * yy + ph[1]) + 40 * np.sin(0.9 * (x + yy) + ph[2]) + 25 * np.sign(np.sin(0.3 * x + ph[3]))
        img = np.stack([base, 0.9 * base + 10, 1.05 * base - 8], axis=-1) + noise * r.randn(h, w, 3)
        fr.append(np.clip(img, 0, 255).astype(np.uint8))
    return fr


def main():
    est = import_estimation()
    from oracle import detector_oracle as D
    r = np.random.RandomState(25)
    clip = moving_clip(r, 60, 24, 36, 0.8, 6.0)
    out = {"frames": np.stack(clip), "ratios": np.array([p[0] for p in PAIRS]), "seeds": np.array([p[1] for p in PAIRS])}
    for i, (ratio, seed) in enumerate(PAIRS):
        blurry, labels, gt = est.generate_blurry_sequence(list(clip), (1, 15), ratio, 5, seed)
        g = gt.numpy()
        assert np.array_equal(g, g.astype(np.uint8))
        out[f"blurry_{i}"] = blurry.numpy()                       # [M,3,H,W] float32
        out[f"labels_{i}"] = labels.numpy()
        out[f"gt_{i}"] = g.astype(np.uint8)                       # [M,3,H,W]
    np.savez_compressed(os.path.join(HERE, "g25_blurset.npz"), **out)
    print("g25:", {k: v.shape for k, v in out.items()})

    r = np.random.RandomState(26)
    feats, labs = [], []
    for c in range(12):
        frames = moving_clip(r, 240, 40, 56, r.uniform(0.0, 1.2), r.uniform(2.0, 14.0))
        blurry, labels, _ = est.generate_blurry_sequence(frames, (1, 15), 0.5, 5, 100 + c)
        u8 = blurry.numpy().astype(np.uint8).astype(np.float32)   # the bytes the reference writes (mix_choice_dataset.py:104)
        feats.append(D.features(torch.from_numpy(u8), 11).numpy())
        labs.append(labels.numpy())
    x, y = np.concatenate(feats).astype(np.float32), np.concatenate(labs).astype(np.int64)
    model = est.estimate_parameters(x, y)[0]
    from sklearn.model_selection import train_test_split
    _, test_idx = train_test_split(np.arange(len(y)), test_size=0.1, random_state=4000)
    np.savez_compressed(os.path.join(HERE, "g26_detector_fit.npz"), features=x, labels=y, coef=model.coef_[0], intercept=model.intercept_,
                        n_iter=model.n_iter_, holdout_seed=np.array(4000), test_idx=test_idx)
    acc = (model.predict(x) == y).mean()
    print(f"g26: {x.shape[0]} rows, {int(y.sum())} sharp; sklearn n_iter {model.n_iter_}, training accuracy {acc:.3f}")


if __name__ == "__main__":
    main()
