"""LD sharpness detector at inference time: when a clip has no `label/<clip>.npy`, the harness
computes six focus measures per frame on the GPU and labels a frame sharp iff a logistic regression says so
(reference inference_SPEINet.py:177-189, 315-322, 349-353).

The arithmetic runs in speinet_amd/csrc/detector.hip; this module only allocates buffers and applies the 7-number
logistic regression.  The default weights are those of LD_detector/pickle/LogisticRegression_0.5_11.pkl, read from the raw
pickle bytes with `pickletools` (the pickle is never loaded) and cross-checked against LD_detector/output.csv:158.

The training side (reference LD_detector/sharp_detector_params_estimation_parallel.py, LD_detector_gopros_train.py,
run_detector.sh) fits those seven numbers to other footage and writes the label files the training loader reads:

    python -m speinet_amd.detector fit   --dir_data <dir with blur/ label/> [--kernel_size 11 | 3 5 7 11 51 101 201] --out detector.json
    python -m speinet_amd.detector label --dir_data <dir with blur/> [--detector detector.json]

`fit` with several kernel sizes is the reference's sweep: one CSV row per size, the parameters with the best hold-out F1 are
saved.  `label` writes `label/<clip>.npy` (0/1 per frame of `blur/<clip>`, in file-name order).  A model is a small JSON file
(`DetectorParams`), never a pickle.
"""
from __future__ import annotations

import argparse
import ctypes as C
import dataclasses
import json
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .clip import IMAGE_EXTS, frames_of

DETECT_BATCH = 16                # frames per launch of a streaming feature pass (the harness's batch)

FEATURES = ("LAP1", "MIS3", "WAV1", "GRA7", "STA3", "DCT3")
LR_COEF = (-0.11971818612047416, -1.2293425023576632, 0.0044214112366378735, -0.042858891031731176,
           0.12867998448379486, 1.5577974574202265)
LR_INTERCEPT = -1.5940041517368388


def focus_measures(frames: torch.Tensor, kernel_size: int = 11) -> torch.Tensor:
    """frames [N,3,H,W] float32 with 0..255 values on a ROCm device -> [N,6] float32 (order of FEATURES)."""
    if not frames.is_cuda:
        raise RuntimeError("speinet_amd.detector runs on MI355X only (HIP kernels); there is no CPU path")
    frames = frames.contiguous().float()
    n, c, h, w = frames.shape
    assert c == 3
    lib = _lib.lib()
    with torch.cuda.device(frames.device):       # kernels launch on the current device: make it the tensor's
        st = C.c_void_p(torch.cuda.current_stream(frames.device).cuda_stream)
        gray = torch.empty(n, h, w, device=frames.device)
        _lib.check(lib.spei_det_gray(C.c_void_p(frames.data_ptr()), C.c_void_p(gray.data_ptr()), n, h, w, st), "spei_det_gray")
        return gray_focus_measures(gray, kernel_size)


def gray_focus_measures(gray: torch.Tensor, kernel_size: int = 11) -> torch.Tensor:
    if not gray.is_cuda:
        raise RuntimeError("speinet_amd.detector runs on MI355X only (HIP kernels); there is no CPU path")
    gray = gray.contiguous().float()
    n, h, w = gray.shape
    lib = _lib.lib()
    with torch.cuda.device(gray.device):
        st = C.c_void_p(torch.cuda.current_stream(gray.device).cuda_stream)
        out = torch.empty(n, 6, device=gray.device)
        ws = torch.empty(lib.spei_det_ws_floats(n, h, w, kernel_size), device=gray.device)
        _lib.check(lib.spei_det_features(C.c_void_p(gray.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), n, h, w,
                                         kernel_size, st), "spei_det_features")
    return out


@dataclasses.dataclass(frozen=True)
class DetectorParams:
    """The logistic regression of the LD detector: 1 (sharp) iff coef . measures(kernel_size) + intercept > 0."""
    coef: Tuple[float, ...]
    intercept: float
    kernel_size: int = 11

    def __post_init__(self):
        coef = tuple(float(c) for c in self.coef)
        if len(coef) != len(FEATURES):
            raise ValueError(f"a detector has {len(FEATURES)} coefficients {FEATURES}; got {len(coef)}")
        if int(self.kernel_size) < 1 or int(self.kernel_size) % 2 == 0:
            raise ValueError(f"kernel_size must be odd and positive; got {self.kernel_size}")
        object.__setattr__(self, "coef", coef)
        object.__setattr__(self, "intercept", float(self.intercept))
        object.__setattr__(self, "kernel_size", int(self.kernel_size))

    def save(self, path: str) -> None:
        with open(path, "w") as f:
            json.dump({"features": list(FEATURES), "coef": list(self.coef), "intercept": self.intercept, "kernel_size": self.kernel_size},
                      f, indent=1)

    @classmethod
    def load(cls, path: str) -> "DetectorParams":
        with open(path) as f:
            d = json.load(f)
        if list(d.get("features", FEATURES)) != list(FEATURES):
            raise ValueError(f"{path}: measures {d['features']} are not this detector's {list(FEATURES)}")
        return cls(tuple(d["coef"]), d["intercept"], d["kernel_size"])


DEFAULT = DetectorParams(LR_COEF, LR_INTERCEPT, 11)


def predict(features, params: Optional[DetectorParams] = None) -> np.ndarray:
    """sklearn LogisticRegression.predict on the six measures: 1 (sharp) iff w.f + b > 0.  `params` None: the reference's GoPro model."""
    p = DEFAULT if params is None else params
    f = features.detach().double().cpu().numpy() if torch.is_tensor(features) else np.asarray(features, dtype=np.float64)
    return ((f @ np.asarray(p.coef) + p.intercept) > 0).astype(np.int64)


def clip_batches(fr, device, batch: int = DETECT_BATCH):
    """One streaming pass over a clip (`clip.frames_of`'s result; a `clip.StreamFrames` is read as it arrives: `fr.upto` waits for
    the next batch's frames or the stream's end): yields (first frame index, uint8 [n,H,W,3] device view) for every
    `batch` frames in turn, on the current stream of `device`.  Host frames are uploaded from two page-locked staging buffers (image
    paths decoded on worker threads two batches ahead), device-resident frames copied on the device.  The frames of a y4m clip are
    staged and uploaded as their planar bytes and made RGB on the device (`fr.rgb`: ops.yuv_to_rgb_u8, or ops.yuv_to_rgb_u16 for a
    deep clip).  A deep clip (`fr.depth` 10 or 12) yields uint16 frames: its samples never pass through 8 bits.  The view is of ONE
    buffer that the next batch overwrites: device memory is bounded by one batch.  The consumer sets grad mode and the current device."""
    dev, B = torch.device(device), batch
    H, W = fr.H, fr.W
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 4)) as pool:
        futs = {}

        def want(upto):
            for i in range(done, upto):           # frames below `done` were yielded: a stream has given them up
                if i not in futs and not fr.on_device(i):
                    futs[i] = pool.submit(fr.host, i)

        shape = (B, H, W, 3) if fr.yuv is None else (B, fr.items.frame_bytes)
        stage = [torch.empty(shape, dtype=fr.dtype if fr.yuv is None else torch.uint8, pin_memory=True) for _ in range(2)]
        events = [None, None]
        dev_batch = torch.empty(B, H, W, 3, dtype=fr.dtype, device=dev)
        dev_planar = None if fr.yuv is None else torch.empty(shape, dtype=torch.uint8, device=dev)
        b = i0 = done = 0
        while True:
            n = fr.upto(i0 + B) - i0                  # a stream waits here for its next B frames, or for its end
            if n <= 0:
                break
            want(i0 + n if fr.T is None else min(i0 + 2 * B, fr.T))      # a stream has read no further
            st = stage[b % 2]
            if events[b % 2] is not None:
                events[b % 2].synchronize()           # the upload issued two batches ago
            host = [i for i in range(i0, i0 + n) if not fr.on_device(i)]
            for i in host:
                st[i - i0].numpy()[...] = futs.pop(i).result()
            if host:
                if dev_planar is None:
                    dev_batch[:n].copy_(st[:n], non_blocking=True)
                else:
                    dev_planar[:n].copy_(st[:n], non_blocking=True)
                    fr.rgb(dev_planar[:n], out=dev_batch[:n])
                events[b % 2] = torch.cuda.Event()
                events[b % 2].record()
            for i in range(i0, i0 + n):
                if fr.on_device(i):
                    dev_batch[i - i0].copy_(fr.device(i))
            yield i0, dev_batch[:n]
            b, i0, done = b + 1, i0 + n, i0 + n


def clip_analysis(fr, device, kernel_size: int = 11, batch: int = DETECT_BATCH, features: bool = True, pair_stats: bool = False,
                  blur=None):
    """The analysis of a clip batch by batch, for a whole clip (`clip_pass`) and for a stream (speinet_amd.video, as its frames
    arrive): per `clip_batches` batch, yields (first frame index, the six focus measures [n,6] float32 or None when not `features`,
    the batch's `ops.frame_pair_stats` (sad [n] int64, or [n-1] for the first batch; hist [n,64] int64) or None when not
    `pair_stats`), on the current stream of `device`.  A deep clip goes through `ops.frames_u16_in` and `ops.frame_pair_stats_u16`
    (its sad is in units of the clip's own depth).  The last frame of a batch is kept as `prev` of the next, so a pair that straddles
    two batches is counted like any other: device memory is bounded by one batch plus one frame.  The consumer sets grad mode and the
    current device around every `next`.
    `blur` (a `blurmap.BlurParams`; None: what is yielded is exactly the above): every yield carries a fourth item, the batch's blur
    verdict maps, uint8 [n,ch,cw] on the device (`ops.blur_cells` with the parameters' `thr` and `flat`: one more launch per batch on
    the frames as this pass sees them), for `deblur_clip(..., matte="auto")`.  With neither `features` nor `pair_stats` the pass
    measures the cells alone: for a clip whose labels and cuts were given that is one more upload of a host clip."""
    from . import ops
    dev = torch.device(device)
    if pair_stats and batch < 2:
        raise ValueError("pair statistics need batches of at least 2 frames (the first batch has no frame before it)")
    prev = None
    for i0, frames in clip_batches(fr, dev, batch):
        feats = stats = None
        if features:
            if fr.depth == 8:
                _, gray = ops.frames_u8_in(frames, gray=True, planes=False)
            else:
                _, gray = ops.frames_u16_in(frames, fr.depth, gray=True, planes=False)
            feats = gray_focus_measures(gray, kernel_size)
        if pair_stats:
            if fr.depth == 8:
                stats = ops.frame_pair_stats(frames, prev if i0 else None)
            else:
                stats = ops.frame_pair_stats_u16(frames, fr.depth, prev if i0 else None)
            if fr.T is None or i0 + len(frames) < fr.T:      # a stream that has not ended may have a next batch
                prev = torch.empty_like(frames[-1]) if prev is None else prev
                prev.copy_(frames[-1])
        if blur is None:
            yield i0, feats, stats
        else:
            yield i0, feats, stats, ops.blur_cells(frames, None if fr.depth == 8 else fr.depth, blur.thr, blur.flat)


def clip_pass(fr, device, kernel_size: int = 11, batch: int = DETECT_BATCH, features: bool = True, pair_stats: bool = False, blur=None,
              cells=None):
    """One `clip_analysis` pass over a whole clip: the six focus measures of every frame ([T,6] float32, or None when not `features`),
    the pair statistics of `ops.frame_pair_stats` over the whole clip ((sad int64 [T-1], hist int64 [T,64]), or None when not
    `pair_stats`), or both, all on `device`.  With `blur` (a `blurmap.BlurParams`) the pass also measures the blur cells, and
    `cells(first frame index, verdict maps)` is called with every batch's."""
    dev = torch.device(device)
    feats, sads, hists = [], [], []
    with torch.no_grad(), torch.cuda.device(dev):
        for i0, f, st, *maps in clip_analysis(fr, dev, kernel_size, batch, features, pair_stats, blur):
            if maps:
                cells(i0, maps[0])
            if features:
                feats.append(f)
            if pair_stats:
                sads.append(st[0])
                hists.append(st[1])
    return (torch.cat(feats) if features else None), ((torch.cat(sads), torch.cat(hists)) if pair_stats else None)


def clip_features(fr, device, kernel_size: int = 11, batch: int = DETECT_BATCH) -> torch.Tensor:
    """The six measures of every frame of a clip (`clip.frames_of`'s result), `batch` frames at a time: uint8 upload from two
    page-locked staging buffers, gray planes (spei_frames_u8_in), focus measures.  Image paths are decoded on worker threads two
    batches ahead.  [T,6] float32 on `device`; device memory is bounded by one batch."""
    return clip_pass(fr, device, kernel_size, batch)[0]


def _clips(dir_data: str) -> list:
    """(clip name, its frames in file-name order) for every folder under dir_data/blur, as data.ClipSet scans them."""
    root = os.path.join(dir_data, "blur")
    if not os.path.isdir(root):
        raise ValueError(f"{dir_data}: no blur/ directory (one folder of frames per clip)")
    clips = []
    for name in sorted(os.listdir(root)):
        d = os.path.join(root, name)
        if os.path.isdir(d):
            files = sorted(os.path.join(d, f) for f in os.listdir(d) if f.lower().endswith(IMAGE_EXTS))
            if files:
                clips.append((name, files))
    if not clips:
        raise ValueError(f"{root}: no clip folder with image files")
    return clips


def dataset_features(dir_data: str, kernel_size: int = 11, device="cuda"):
    """The six measures of every frame of every `blur/<clip>` under dir_data, streamed through `clip_features` (reference
    collate_all_vars, sharp_detector_params_estimation_parallel.py:221-237, on frames that are already blurred).
    -> (features [N,6] float32, labels [N] int64 from label/<clip>.npy or None when a clip has none, clip names, frames per clip)."""
    feats, labels, names, counts = [], [], [], []
    for name, files in _clips(dir_data):
        try:
            fr = frames_of(files)
        except ValueError as e:
            raise ValueError(f"clip {name}: {e}") from None
        feats.append(clip_features(fr, device, kernel_size).cpu().numpy())
        names.append(name)
        counts.append(fr.T)
        lf = os.path.join(dir_data, "label", name + ".npy")
        if labels is not None and os.path.isfile(lf):
            lab = np.asarray(np.load(lf)).reshape(-1).astype(np.int64)
            if lab.size != fr.T:
                raise ValueError(f"clip {name}: {lab.size} labels ({lf}) for {fr.T} frames")
            labels.append(lab)
        else:
            labels = None
    return np.concatenate(feats).astype(np.float32), (None if labels is None else np.concatenate(labels)), names, counts


def label_dataset(dir_data: str, params: Optional[DetectorParams] = None, device="cuda") -> list:
    """Write label/<clip>.npy (int64 0/1 per frame, 1 = sharp) for every clip under dir_data/blur; returns the files written."""
    p = DEFAULT if params is None else params
    feats, _, names, counts = dataset_features(dir_data, p.kernel_size, device)
    pred = predict(feats, p)
    os.makedirs(os.path.join(dir_data, "label"), exist_ok=True)
    out, at = [], 0
    for name, n in zip(names, counts):
        path = os.path.join(dir_data, "label", name + ".npy")
        np.save(path, pred[at:at + n])
        out.append(path)
        at += n
    return out


# ---- fitting (reference estimate_parameters :239-250, model1 only: the reference ships and uses the logistic model) ----

def _design(features, labels):
    x = np.asarray(features, dtype=np.float64)
    y = np.asarray(labels).reshape(-1)
    if x.ndim != 2 or x.shape[1] != len(FEATURES) or x.shape[0] != y.size:
        raise ValueError(f"features must be [N,{len(FEATURES)}] with one label each; got {x.shape} and {y.size} labels")
    if not np.isin(y, (0, 1)).all() or y.min() == y.max():
        raise ValueError("labels must be 0 / 1 and hold both classes")
    if not np.isfinite(x).all():
        raise ValueError("features hold a non-finite value")
    return x, y.astype(np.float64)


def objective(params: DetectorParams, features, labels) -> float:
    """sklearn's default LogisticRegression objective (C = 1, L2, unpenalised intercept): sum log(1 + exp(-y~ z)) + |w|^2 / 2."""
    x, y = _design(features, labels)
    w = np.asarray(params.coef)
    z = x @ w + params.intercept
    return float(np.logaddexp(0.0, -(2.0 * y - 1.0) * z).sum() + 0.5 * w @ w)


def fit_logistic(features, labels, kernel_size: int = 11, tol: float = 1e-11, max_iter: int = 200) -> DetectorParams:
    """The minimiser of `objective` in float64 by a damped Newton iteration on 7 unknowns.  The six measures differ by orders of
    magnitude (WAV1 is a sum over the frame, the others means over windows), so the iteration runs on centred columns scaled to unit
    deviation, u = w * s: the penalty becomes sum (u_j / s_j)^2 / 2 and the centring moves into the unpenalised intercept.  Stops when
    the max-norm of the gradient in (u, b) is below `tol` or a step no longer lowers the objective."""
    x, y = _design(features, labels)
    mu, s = x.mean(axis=0), x.std(axis=0)
    s = np.where(s > 0, s, 1.0)
    a = np.concatenate([(x - mu) / s, np.ones((x.shape[0], 1))], axis=1)
    pen = np.concatenate([1.0 / s ** 2, [0.0]])
    sign = 2.0 * y - 1.0

    def f(t):
        return np.logaddexp(0.0, -sign * (a @ t)).sum() + 0.5 * (pen * t * t).sum()

    t = np.zeros(7)
    ft = f(t)
    for _ in range(max_iter):
        p = 0.5 * (1.0 + np.tanh(0.5 * (a @ t)))           # sigmoid without overflow
        g = a.T @ (p - y) + pen * t
        if np.abs(g).max() < tol:
            break
        hess = (a * (p * (1.0 - p))[:, None]).T @ a + np.diag(pen)
        step = np.linalg.solve(hess + 1e-12 * np.eye(7), g)
        lam, moved = 1.0, False
        while lam > 1e-10:
            cand = t - lam * step
            fc = f(cand)
            if fc <= ft:
                moved = not np.array_equal(cand, t)
                t, ft = cand, fc
                break
            lam *= 0.5
        if not moved:
            break
    w = t[:6] / s
    return DetectorParams(tuple(w.tolist()), float(t[6] - (w * mu).sum()), kernel_size)


def holdout_split(n: int, seed: int, test_size: float = 0.1):
    """(train, test) row indices of sklearn's train_test_split(..., test_size, random_state=seed) (the reference's :273):
    a RandomState(seed) permutation whose first ceil(test_size * n) rows are the hold-out."""
    n_test = int(np.ceil(test_size * n))
    perm = np.random.RandomState(seed).permutation(n)
    return perm[n_test:], perm[:n_test]


def report(params: DetectorParams, features, labels) -> dict:
    """The reference's report on a set of rows (:253-264 calculate_metrics, :288-291): confusion counts, accuracy, recall, precision, F1
    of the class sharp = 1.  (The reference's prints pass the prediction as y_true, so its "recall" is this precision and vice versa.)"""
    y = np.asarray(labels).reshape(-1).astype(np.int64)
    p = predict(features, params)
    tp, tn = int(((p == 1) & (y == 1)).sum()), int(((p == 0) & (y == 0)).sum())
    fp, fn = int(((p == 1) & (y == 0)).sum()), int(((p == 0) & (y == 1)).sum())
    recall = tp / (tp + fn) if tp + fn else 0.0
    precision = tp / (tp + fp) if tp + fp else 0.0
    f1 = 2 * precision * recall / (precision + recall) if precision + recall else 0.0
    return {"n": int(y.size), "tp": tp, "tn": tn, "fp": fp, "fn": fn, "accuracy": (tp + tn) / max(1, y.size), "recall": recall,
            "precision": precision, "f1": f1}


def fit_with_holdout(features, labels, kernel_size: int = 11, seed: int = 4000, test_size: float = 0.1):
    """Fit on the training rows of `holdout_split`, report on its hold-out (the reference's __main__, :273-291; its default seed)."""
    x, y = np.asarray(features), np.asarray(labels).reshape(-1)
    train, test = holdout_split(y.size, seed, test_size)
    params = fit_logistic(x[train], y[train], kernel_size)
    return params, report(params, x[test], y[test])


CSV_COLUMNS = ("kernel_size", "frames", "tp", "tn", "fp", "fn", "accuracy", "recall", "precision", "f1", "coef", "intercept")


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Fit the LD sharpness detector to a labelled data set, or label a data set with it")
    sub = ap.add_subparsers(dest="cmd", required=True)
    pf = sub.add_parser("fit", help="fit the logistic regression on blur/<clip> frames and label/<clip>.npy")
    pf.add_argument("--dir_data", required=True)
    pf.add_argument("--kernel_size", type=int, nargs="+", default=[11], help="one size, or several (the sweep: best hold-out F1 is saved)")
    pf.add_argument("--out", required=True, help="the detector's JSON file")
    pf.add_argument("--csv", default=None, help="one row per kernel size (default: <out>.csv)")
    pf.add_argument("--seed", type=int, default=4000, help="seed of the 10 %% hold-out split")
    pf.add_argument("--device", default="cuda")
    pl = sub.add_parser("label", help="write label/<clip>.npy for every clip under blur/")
    pl.add_argument("--dir_data", required=True)
    pl.add_argument("--detector", default=None, help="a detector JSON file (default: the reference's GoPro model, kernel 11)")
    pl.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    if a.cmd == "label":
        for path in label_dataset(a.dir_data, DetectorParams.load(a.detector) if a.detector else None, a.device):
            print(f"> {path}", flush=True)
        return
    best, rows = None, []
    for k in a.kernel_size:
        feats, labels, names, counts = dataset_features(a.dir_data, k, a.device)
        if labels is None:
            raise SystemExit(f"--dir_data {a.dir_data}: a clip has no label/<clip>.npy; fitting needs labels")
        params, rep = fit_with_holdout(feats, labels, k, a.seed)
        rows.append([k, len(labels), rep["tp"], rep["tn"], rep["fp"], rep["fn"], rep["accuracy"], rep["recall"], rep["precision"], rep["f1"],
                     " ".join(repr(c) for c in params.coef), repr(params.intercept)])
        print(f"> kernel {k}: {len(labels)} frames, hold-out {rep['n']}: accuracy {rep['accuracy']:.3f} recall {rep['recall']:.3f} "
              f"precision {rep['precision']:.3f} F1 {rep['f1']:.3f}", flush=True)
        if best is None or rep["f1"] > best[1]:
            best = (params, rep["f1"])
    with open(a.csv or a.out + ".csv", "w") as f:
        f.write(",".join(CSV_COLUMNS) + "\n")
        for r in rows:
            f.write(",".join(str(v) for v in r) + "\n")
    best[0].save(a.out)
    print(f"# saved {a.out}: kernel {best[0].kernel_size}, hold-out F1 {best[1]:.3f}", flush=True)


if __name__ == "__main__":
    main()
