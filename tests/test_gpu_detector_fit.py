"""GPU suite: the detector's box path for k >= 13 (running column sums + row prefix sums, csrc/detector.hip) against the oracle, the
bits of k <= 11 against the parent commit's, and the whole chain sharp footage -> data set -> fitted detector -> labels -> clip API.

Box path: all six measures for k in {13, 51, 101, 201} against oracle.detector_oracle at rtol 2e-4 (tests/test_gpu_detector.py).  That
bound is the slack of the fp32 oracle, which is itself up to 2.4e-5 away from float64 at these sizes (at 720p, k = 201: 8.4e-6 on GRA7,
6.1e-6 on STA3); it is not the kernels' error, which is 5.5e-8 (GRA7) / 6.4e-9 (STA3) there.  The tight bound, against float64 and per
measure, is in tests/test_gpu_detector_f64.py."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import detector_oracle as D      # noqa: E402
from speinet_amd import blurset, detector, ops  # noqa: E402

DEV = "cuda:0"

# The six measures (LAP1, MIS3, WAV1, GRA7, STA3, DCT3) of the parent commit's build, as float.hex(): g13_k<k> for the four gray frames
# of golden G13, p720_k<k> for `_frame720()` through frames_u8_in(gray=True).  Recorded on an MI355X before the box path was added.
PARENT_BITS = {
    "g13_k3": [
        ["0x1.0318d8p+0", "0x1.60f38ep+1", "0x1.c85d9ep+6", "0x1.5faa72p-1", "0x1.996ff0p-7", "0x1.9673f0p-2"],
        ["0x1.dff224p+1", "0x1.b56740p+2", "0x1.07db30p+8", "0x1.915b0cp-1", "0x1.7b376ap-5", "0x1.672ba2p+1"],
        ["0x1.3fb236p+3", "0x1.5ef056p+3", "0x1.9d1270p+8", "0x1.503d1ep+0", "0x1.f932e6p-4", "0x1.ff36aep+2"],
        ["0x1.429496p+4", "0x1.e7a124p+3", "0x1.1eb9a4p+9", "0x1.017dfep+1", "0x1.fdc1b6p-3", "0x1.a466f0p+3"],
    ],
    "p720_k3": [
        ["0x1.86997ep-1", "0x1.b5b78cp+1", "0x1.191130p+14", "0x1.1b0dc2p-3", "0x1.349f32p-7", "0x1.2ed762p+1"],
    ],
    "g13_k5": [
        ["0x1.d3c7bep+1", "0x1.03bc52p+3", "0x1.c85d9ep+6", "0x1.950312p+1", "0x1.3f5d2cp-4", "0x1.3b628ep+1"],
        ["0x1.6b44b6p+3", "0x1.367338p+4", "0x1.07db30p+8", "0x1.ddd7e0p+1", "0x1.85e512p-3", "0x1.87d982p+3"],
        ["0x1.c6691ap+4", "0x1.ec600ap+4", "0x1.9d1270p+8", "0x1.88ed3ep+2", "0x1.ecfa1ap-2", "0x1.98d894p+4"],
        ["0x1.c6c5f2p+5", "0x1.5514b6p+5", "0x1.1eb9a4p+9", "0x1.131352p+3", "0x1.d6967ep-1", "0x1.75c3a4p+4"],
    ],
    "p720_k5": [
        ["0x1.153ef8p+1", "0x1.30c7b8p+3", "0x1.191130p+14", "0x1.70cb78p-1", "0x1.5795f4p-5", "0x1.6311a6p+3"],
    ],
    "g13_k7": [
        ["0x1.6291fep+2", "0x1.e0c5e6p+3", "0x1.c85d9ep+6", "0x1.4d921ap+2", "0x1.99abaep-3", "0x1.0245fap+3"],
        ["0x1.4775a8p+4", "0x1.2a3d1cp+5", "0x1.07db30p+8", "0x1.bf5c0cp+2", "0x1.ee2cbap-2", "0x1.ef8a18p+4"],
        ["0x1.b43eeep+5", "0x1.ddd3e4p+5", "0x1.9d1270p+8", "0x1.848b56p+3", "0x1.45cd12p+0", "0x1.96443ap+4"],
        ["0x1.b7545ep+6", "0x1.4bbcb6p+6", "0x1.1eb9a4p+9", "0x1.0480cep+4", "0x1.24905ap+1", "0x1.10b080p+3"],
    ],
    "p720_k7": [
        ["0x1.001856p+2", "0x1.2888ccp+4", "0x1.191130p+14", "0x1.75516ep+0", "0x1.0ddaecp-3", "0x1.4cdfdap+4"],
    ],
    "g13_k11": [
        ["0x1.dfcb66p+3", "0x1.2d1ef8p+5", "0x1.c85d9ep+6", "0x1.f5a876p+3", "0x1.d58116p-1", "0x1.ee1d6ap+4"],
        ["0x1.9d1d1ap+5", "0x1.72a09cp+6", "0x1.07db30p+8", "0x1.4ee288p+4", "0x1.36d56ap+1", "0x1.d90288p+4"],
        ["0x1.0e184cp+7", "0x1.2787aep+7", "0x1.9d1270p+8", "0x1.fa156ep+4", "0x1.47a334p+2", "0x1.3643d6p+1"],
        ["0x1.0d0174p+8", "0x1.98e0fap+7", "0x1.1eb9a4p+9", "0x1.66ffacp+5", "0x1.bf4aacp+2", "0x1.cf8420p+5"],
    ],
    "p720_k11": [
        ["0x1.3c3180p+3", "0x1.6e2038p+5", "0x1.191130p+14", "0x1.d515f8p+1", "0x1.6e66d4p-1", "0x1.331b26p+3"],
    ],
}


def _frame720():
    r = np.random.RandomState(720)
    yy, xx = np.meshgrid(np.arange(720), np.arange(1280), indexing="ij")
    base = 128 + 70 * np.sin(0.031 * xx) * np.cos(0.047 * yy) + 30 * np.sin(0.4 * (xx + yy))
    return np.clip(base[..., None] * np.array([1.0, 0.9, 1.1]) + 12 * r.randn(720, 1280, 3), 0, 255).astype(np.uint8)


def _bits(rows):
    return np.array([[float.fromhex(v) for v in row] for row in rows], dtype=np.float32)


@pytest.mark.parametrize("k", [3, 5, 7, 11])
def test_small_kernels_keep_the_parent_bits(golden_dir, k):
    g13 = np.load(os.path.join(golden_dir, "g13_detector.npz"))
    g = torch.from_numpy(g13["gray"])[:, 0].to(DEV)
    assert np.array_equal(detector.gray_focus_measures(g, k).cpu().numpy(), _bits(PARENT_BITS[f"g13_k{k}"]))
    _, g720 = ops.frames_u8_in(torch.from_numpy(_frame720()).to(DEV), gray=True, planes=False)
    assert np.array_equal(detector.gray_focus_measures(g720, k).cpu().numpy(), _bits(PARENT_BITS[f"p720_k{k}"]))


def _textured(h, w, n, seed):
    r = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.stack([np.clip(128 + 90 * np.sin(0.05 * (i + 1) * yy) * np.cos(0.08 * xx) + (3 + 10 * i) * r.randn(3, h, w), 0, 255)
                     for i in range(n)]).astype(np.float32)


@pytest.mark.parametrize("k", [13, 51, 101, 201])
def test_box_path_vs_oracle(k):
    for h, w, n in ((k + 3, k + 3, 3), (k + 40, 2 * k + 17, 2), (720, 1280, 1)):
        t = torch.from_numpy(_textured(h, w, n, k + h))
        g = D.gray(t)
        out = detector.focus_measures(t.to(DEV), k).cpu().numpy()
        again = detector.focus_measures(t.to(DEV), k).cpu().numpy()
        assert np.array_equal(out, again), "the fixed summation order must reproduce bit for bit"
        for col, ref in enumerate((D.lap1(g, k), D.mis3(g, k), D.wav1(g), D.gra7(g, k), D.sta3(g, k), D.dct3(g, k))):
            err = np.abs(out[:, col] - ref.numpy()) / np.abs(ref.numpy())
            print(f"k={k} {h}x{w} {detector.FEATURES[col]}: max rel err {err.max():.3e}")
            np.testing.assert_allclose(out[:, col], ref.numpy(), rtol=2e-4, err_msg=f"{detector.FEATURES[col]} k={k} {h}x{w}")


def test_all_six_measures_vs_oracle_k13():
    t = torch.from_numpy(_textured(97, 131, 3, 1))
    np.testing.assert_allclose(detector.focus_measures(t.to(DEV), 13).cpu().numpy(), D.features(t, 13).numpy(), rtol=2e-4)


def test_workspace_grows_for_the_box_path_only():
    from speinet_amd import _lib
    lib = _lib.lib()
    assert lib.spei_det_ws_floats(2, 100, 120, 13) - lib.spei_det_ws_floats(2, 100, 120, 11) >= 2 * 2 * 100 * 120
    g = torch.rand(1, 30, 30, device=DEV)
    with pytest.raises(RuntimeError, match="must be odd and fit"):
        detector.gray_focus_measures(g, 29)


def _moving_clip(seed, T, h, w, speed, noise):
    r = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ph = r.uniform(0, 6.28, size=4)
    out = np.empty((T, h, w, 3), np.uint8)
    for t in range(T):
        x = xx + speed * t
        base = 128 + 60 * np.sin(0.55 * x + ph[0]) * np.cos(0.35 * yy + ph[1]) + 40 * np.sin(0.9 * (x + yy) + ph[2]) + 25 * np.sign(np.sin(0.3 * x + ph[3]))
        img = np.stack([base, 0.9 * base + 10, 1.05 * base - 8], axis=-1) + noise * r.randn(h, w, 3)
        out[t] = np.clip(img, 0, 255)
    return out


CLIPS = ((0.9, 4.0), (0.6, 8.0), (1.1, 6.0), (0.8, 10.0))         # (pixels per frame, noise) of the synthetic sharp clips


@pytest.fixture(scope="module")
def net32():
    from speinet_amd.video import load_model
    return load_model("synthetic", DEV, "f32", graph=False)


def test_sharp_footage_to_fitted_detector_to_clip_api(tmp_path, net32):
    from PIL import Image
    from speinet_amd import data, video
    src, out = str(tmp_path / "sharp"), str(tmp_path / "set")
    for c, (speed, noise) in enumerate(CLIPS):
        os.makedirs(os.path.join(src, f"clip{c}"))
        for i, f in enumerate(_moving_clip(40 + c, 500, 40, 60, speed, noise)):
            Image.fromarray(f).save(os.path.join(src, f"clip{c}", f"{i:05d}.png"), compress_level=1)
    done = blurset.write_dataset(src, out, ratios=[0.3, 0.5], seed=11, device=DEV)
    assert [d["name"] for d in done] == ["clip0", "clip1", "clip2", "clip3"]

    # the written set is the reference's: same runs from the same seed, the kernel's bytes on disk, labels in file order
    rng = random.Random(11)
    for c, d in enumerate(done):
        ratio = rng.choice([0.3, 0.5])
        starts, lengths, labels = blurset.plan_runs(500, ratio, rng=rng)
        assert d["ratio"] == ratio and np.array_equal(d["labels"], labels)
        assert np.array_equal(np.load(os.path.join(out, "label", f"clip{c}.npy")), labels)
        clip = _moving_clip(40 + c, 500, 40, 60, *CLIPS[c])
        files = sorted(os.listdir(os.path.join(out, "blur", f"clip{c}")))
        assert len(files) == len(labels) == len(os.listdir(os.path.join(out, "gt", f"clip{c}")))
        for m in (0, len(labels) // 2, len(labels) - 1):
            s, n = int(starts[m]), int(lengths[m])
            want = (clip[s:s + n].astype(np.int64).sum(axis=0) // n).astype(np.uint8)
            assert np.array_equal(np.asarray(Image.open(os.path.join(out, "blur", f"clip{c}", files[m]))), want)
            assert np.array_equal(np.asarray(Image.open(os.path.join(out, "gt", f"clip{c}", files[m]))), clip[s + n // 2])

    cs = data.ClipSet(out, train=True, patch=40)                 # the training loader scans it without error
    assert [c["T"] for c in cs.clips] == [d["frames"] for d in done]
    assert [c["labels"] for c in cs.clips] == [d["labels"].tolist() for d in done]

    det_json = str(tmp_path / "detector.json")
    detector.main(["fit", "--dir_data", out, "--kernel_size", "7", "13", "--out", det_json, "--device", DEV])
    fitted = detector.DetectorParams.load(det_json)
    assert fitted.kernel_size in (7, 13)
    assert len(open(det_json + ".csv").read().strip().splitlines()) == 3

    truth = np.concatenate([d["labels"] for d in done])
    for d in done:
        os.remove(os.path.join(out, "label", d["name"] + ".npy"))
    detector.main(["label", "--dir_data", out, "--detector", det_json, "--device", DEV])
    written = np.concatenate([np.load(os.path.join(out, "label", d["name"] + ".npy")) for d in done])
    assert written.shape == truth.shape
    _, hold = detector.holdout_split(len(truth), 4000)
    majority = max(truth[hold].mean(), 1 - truth[hold].mean())
    acc = (written[hold] == truth[hold]).mean()
    print(f"hold-out of {len(hold)}: accuracy {acc:.3f}, majority class {majority:.3f}; kernel {fitted.kernel_size}")
    assert acc > majority

    # the clip API: the fitted detector's labels make the plan; no argument = the default model, frame for frame
    files = [os.path.join(out, "blur", "clip1", f) for f in sorted(os.listdir(os.path.join(out, "blur", "clip1")))][:8]
    feats = detector.clip_features(video.frames_of(files), torch.device(DEV), fitted.kernel_size)
    run = video.deblur_clip(net32, files, detector=fitted)
    assert np.array_equal(run.labels, detector.predict(feats, fitted))
    assert run.plan == video.window_plan(run.labels)
    plain = [f.cpu().numpy() for _, f in video.deblur_clip(net32, files)]
    dflt_run = video.deblur_clip(net32, files, detector=detector.DEFAULT)
    dflt = [f.cpu().numpy() for _, f in dflt_run]
    assert np.array_equal(dflt_run.labels, detector.predict(detector.clip_features(video.frames_of(files), torch.device(DEV), 11)))
    assert len(plain) == len(dflt) == 8 and all(np.array_equal(a, b) for a, b in zip(plain, dflt))
