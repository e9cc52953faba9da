"""Host suite: the detector's fit / label side.  `fit_logistic` against the reference's sklearn fit on golden G26
(tests/golden/make_golden_blurset.py): it must reach an objective no higher than the reference's coefficients do, and a gradient
below 1e-8 in column-scaled coordinates (float64 Newton on 7 unknowns: a convergence statement)."""
import os

import numpy as np
import pytest

from speinet_amd import detector


@pytest.fixture(scope="module")
def g26(golden_dir):
    return np.load(os.path.join(golden_dir, "g26_detector_fit.npz"))


def _scaled_gradient(params, x, y):
    """Gradient of sum log(1 + exp(-y~ z)) + |w|^2 / 2 in the coordinates u = w * s (s = column deviation) and the intercept."""
    x = np.asarray(x, np.float64)
    w, s = np.asarray(params.coef), x.std(axis=0)
    p = 1.0 / (1.0 + np.exp(-(x @ w + params.intercept)))
    return np.concatenate([s * (x.T @ (p - y) + w), [(p - y).sum()]])


def test_fit_reaches_the_minimum_the_reference_stops_short_of(g26):
    x, y = g26["features"], g26["labels"]
    ref = detector.DetectorParams(tuple(g26["coef"]), float(g26["intercept"][0]), 11)
    fit = detector.fit_logistic(x, y)
    f_fit, f_ref = detector.objective(fit, x, y), detector.objective(ref, x, y)
    g = np.abs(_scaled_gradient(fit, x, y)).max()
    agree = (detector.predict(x, fit) == detector.predict(x, ref)).mean()
    print(f"objective: fit {f_fit:.6f} reference {f_ref:.6f} (sklearn n_iter {g26['n_iter']}); scaled gradient {g:.3e}; "
          f"decisions agree on {100 * agree:.2f} % of {len(y)} rows")
    assert f_fit <= f_ref
    assert g < 1e-8
    assert fit.kernel_size == 11


def test_objective_is_sklearns(g26):
    x, y = g26["features"].astype(np.float64), g26["labels"]
    p = detector.DetectorParams((0.1, -0.2, 1e-4, 0.3, -0.4, 0.5), -0.7, 11)
    z = x @ np.asarray(p.coef) + p.intercept
    want = np.log1p(np.exp(-(2 * y - 1) * z)).sum() + 0.5 * np.sum(np.square(p.coef))
    assert abs(detector.objective(p, x, y) - want) < 1e-9 * want


def test_holdout_is_the_references_split(g26):
    x, y = g26["features"], g26["labels"]
    train, test = detector.holdout_split(len(y), int(g26["holdout_seed"]))
    assert np.array_equal(test, g26["test_idx"])
    assert sorted(np.concatenate([train, test]).tolist()) == list(range(len(y)))
    params, rep = detector.fit_with_holdout(x, y, 11, int(g26["holdout_seed"]))
    assert rep["n"] == len(test) == rep["tp"] + rep["tn"] + rep["fp"] + rep["fn"]
    pred = detector.predict(x[test], params)
    assert rep["tp"] == int(((pred == 1) & (y[test] == 1)).sum()) and rep["fn"] == int(((pred == 0) & (y[test] == 1)).sum())
    assert rep["accuracy"] == (pred == y[test]).mean()
    assert rep["accuracy"] > max(y[test].mean(), 1 - y[test].mean())          # better than the majority class on rows it never saw


def test_fit_refuses_bad_input(g26):
    x, y = g26["features"], g26["labels"]
    for bad in ((x[:, :5], y), (x, y[:-1]), (x, np.ones_like(y)), (x, y + 1)):
        with pytest.raises(ValueError):
            detector.fit_logistic(*bad)


def test_params_json_round_trip(tmp_path):
    p = detector.DetectorParams((0.1 + 1e-17, -1.2293425023576632, 4.4214112366378735e-03, 1e-300, 1 / 3, 2 ** 0.5), -1.5940041517368388, 51)
    path = str(tmp_path / "detector.json")
    p.save(path)
    assert detector.DetectorParams.load(path) == p
    assert detector.DEFAULT == detector.DetectorParams(detector.LR_COEF, detector.LR_INTERCEPT, 11)
    with pytest.raises(ValueError):
        detector.DetectorParams((1.0, 2.0), 0.0, 11)
    with pytest.raises(ValueError):
        detector.DetectorParams(detector.LR_COEF, 0.0, 12)


def test_predict_default_params(golden_dir):
    r = np.random.RandomState(3)
    f = np.abs(r.randn(64, 6)) * [30.0, 8.0, 4000.0, 0.05, 0.05, 4.0]        # the measures' scales on G13's frames
    assert np.array_equal(detector.predict(f), detector.predict(f, detector.DEFAULT))
    assert np.array_equal(detector.predict(f), ((f @ np.asarray(detector.LR_COEF) + detector.LR_INTERCEPT) > 0).astype(np.int64))
    assert 0 < detector.predict(f).sum() < len(f)


def _toy_tree(root, clips):
    from PIL import Image
    r = np.random.RandomState(0)
    for name, n in clips.items():
        os.makedirs(os.path.join(root, "blur", name))
        for i in range(n):
            Image.fromarray(r.randint(0, 255, (24, 32, 3)).astype(np.uint8)).save(os.path.join(root, "blur", name, f"{i:06d}.png"))


def test_label_writes_one_file_per_clip(tmp_path, monkeypatch):
    import torch
    clips = {"a": 5, "b": 17, "c": 2}
    _toy_tree(str(tmp_path), clips)
    calls = []

    def fake_features(fr, device, kernel_size=11, batch=16):          # there is no CPU path: the measures are mocked
        calls.append((fr.T, kernel_size))
        r = np.random.RandomState(fr.T)
        return torch.from_numpy(np.abs(r.randn(fr.T, 6)) * [30.0, 8.0, 4000.0, 0.05, 0.05, 4.0]).float()

    monkeypatch.setattr(detector, "clip_features", fake_features)
    params = detector.DetectorParams(detector.LR_COEF, detector.LR_INTERCEPT, 7)
    params.save(str(tmp_path / "d.json"))
    detector.main(["label", "--dir_data", str(tmp_path), "--detector", str(tmp_path / "d.json"), "--device", "cpu"])
    assert calls == [(5, 7), (17, 7), (2, 7)]
    for name, n in clips.items():
        lab = np.load(str(tmp_path / "label" / (name + ".npy")))
        assert lab.shape == (n,) and lab.dtype == np.int64 and np.isin(lab, (0, 1)).all()
        assert np.array_equal(lab, detector.predict(fake_features(type("F", (), {"T": n}), "cpu"), params))
    feats, labels, names, counts = detector.dataset_features(str(tmp_path), 7, "cpu")
    assert names == ["a", "b", "c"] and counts == [5, 17, 2] and feats.shape == (24, 6) and feats.dtype == np.float32
    assert labels.shape == (24,)
