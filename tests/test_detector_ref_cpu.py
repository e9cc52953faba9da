"""CPU suite for tests/detector_ref.py, the float64 reference of the GPU detector tests (test_gpu_detector_f64.py): it agrees with
the reference project's recorded outputs and with the fp32 oracle, the case table it shares with the GPU test sees every deliberately
wrong variant of it, and the labels the GPU test compares are not decided by rounding."""
import os

import numpy as np
import pytest
import torch

import detector_ref as R
from oracle import detector_oracle as D
from speinet_amd import detector

G13_COLUMNS = ((0, "lap1"), (1, "mis3"), (3, "gra7"), (4, "sta3"), (5, "dct3"))


def _rel(a, b):
    return float((np.abs(a - b) / np.abs(b)).max())


def test_reference_vs_recorded_outputs(golden_dir):
    """Golden G13 holds the reference project's own fp32 outputs for four 64x80 gray frames, k = 11 and 7.  Largest relative distance
    of the float64 restatement, measured: LAP1 1.54e-7, MIS3 1.02e-7, GRA7 1.15e-7, STA3 1.37e-7, DCT3 2.68e-7 (a few fp32 roundings of
    the recorded values; an off-by-one moves a measure by 1e-3 or more, see the variants below).  Asserted at twice that."""
    g13 = np.load(os.path.join(golden_dir, "g13_detector.npz"))
    bound = {"lap1": 2 * 1.54e-7, "mis3": 2 * 1.02e-7, "gra7": 2 * 1.15e-7, "sta3": 2 * 1.37e-7, "dct3": 2 * 2.68e-7}
    for k in (11, 7):
        m = R.measures(g13["gray"][:, 0], k)
        for col, name in G13_COLUMNS:
            d = _rel(m[:, col], g13[f"{name}_k{k}"].astype(np.float64))
            print(f"k={k} {name}: {d:.3e}")
            assert d <= bound[name], f"{name} k={k}: {d:.3e}"


def _frames(h, w):
    r = np.random.RandomState(h)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.stack([np.clip(128 + 90 * np.sin(0.05 * (i + 1) * yy) * np.cos(0.08 * xx) + (3 + 10 * i) * r.randn(3, h, w), 0, 255)
                     for i in range(3)]).astype(np.float32)


# largest relative distance of oracle.detector_oracle.features (fp32 torch) from float64 over the textured frames of
# test_gpu_detector.py::test_features_vs_oracle (64x80, 97x131, 200x320; k = 11), measured here, per measure (order of FEATURES)
ORACLE_DISTANCE = (1.66e-7, 1.05e-7, 4.01e-8, 1.98e-7, 1.24e-7, 4.95e-7)


@pytest.mark.parametrize("h,w", [(64, 80), (97, 131), (200, 320)])
def test_reference_vs_fp32_oracle(h, w):
    """The fp32 oracle on the existing textured cases (the frames of test_features_vs_oracle, k = 11) against float64 on the oracle's
    own gray plane: asserted at twice the distance measured here (ORACLE_DISTANCE).  WAV1 is float64 in both; its distance is the
    oracle's last rounding to fp32.  At k = 11 the oracle's own error is a few fp32 roundings; at k = 201 and 720p it reaches 2.4e-5,
    which is why test_gpu_detector.py and test_gpu_detector_fit.py compare with it at 2e-4 only."""
    t = torch.from_numpy(_frames(h, w))
    got = D.features(t, 11).double().numpy()
    ref = R.measures(D.gray(t)[:, 0].numpy(), 11)
    d = (np.abs(got - ref) / np.abs(ref)).max(axis=0)
    print(f"{h}x{w}: " + " ".join(f"{f}={e:.3e}" for f, e in zip(R.FEATURES, d)))
    assert (d <= 2 * np.asarray(ORACLE_DISTANCE)).all(), d


def test_wav1_is_the_oracles():
    g = R.texture(37, 52, 2, 3)
    ours = R.measures(g, 11)[:, 2]
    theirs = D.wav1(torch.from_numpy(g)[:, None]).double().numpy()          # float64 inside, returned as fp32
    assert _rel(ours, theirs) < 2.0 ** -23


@pytest.fixture(scope="module")
def table():
    """(frames, float64 measures, allowed |kernel - float64|) of every content of every case, computed once."""
    out = {}
    for k, h, w, n in R.CASES:
        for name in R.CONTENTS:
            x = R.content(name, k, h, w, n)
            ref, terms = R.measures_and_terms(x, k)
            out[(k, h, w, name)] = (x, ref, R.bound(ref, terms, k, name))
    return out


def _seen_by(table, variant, want_path=None):
    """Cases of the table where `variant` moves a measure by more than 10 times what the GPU test allows: [(case, measure, ratio)]."""
    hits = []
    for (k, h, w, name), (x, ref, allowed) in table.items():
        if want_path is not None and R.path_of(k) != want_path:
            continue
        moved = np.abs(R.measures(x, k, variant) - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(allowed > 0, moved / allowed, np.where(moved > 0, np.inf, 0.0)).max(axis=0)
        if ratio.max() > 10:
            hits.append(((k, h, w, name), R.FEATURES[int(ratio.argmax())], float(ratio.max())))
    return hits


@pytest.mark.parametrize("variant", sorted(R.VARIANTS))
def test_the_table_sees_every_variant(table, variant):
    """Every wrong restatement moves at least one measure of at least one case by more than 10 times the GPU test's allowance for it --
    and does so on both box paths (k < 13 and k >= 13), which share no box code."""
    for path in ("direct", "scan"):
        hits = _seen_by(table, variant, path)
        print(f"{variant} [{path}]: {len(hits)} cases, first {hits[:3]}")
        assert hits, f"no case with {path} box sums sees: {R.VARIANTS[variant]}"


def test_the_definition_is_not_a_variant(table):
    (x, ref, _) = table[(13, 65, 300, "texture")]
    assert np.array_equal(R.measures(x, 13), ref)
    with pytest.raises(KeyError):
        R.measures(x, 13, "no_such_variant")


def test_impulse_positions():
    g = R.impulses(65, 300, 13)                    # ch = 65 = H: (ch, cw) lies outside the frame
    assert [tuple(np.argwhere(f)[0]) for f in g] == [(0, 0), (64, 299), (64, 298)]
    g = R.impulses(33, 257, 13)
    assert [tuple(np.argwhere(f)[0]) for f in g] == [(0, 0), (32, 256), (25, 246), (26, 247)]


def test_labels_are_not_decided_by_rounding():
    """The default model on the float64 measures of the table's noisy-texture and smooth-bright cases at k = 11: a frame whose margin
    |w.f + b| is within sum |w_i| tol_i |f_i| is left out of the GPU label comparison; at most 10 % of the frames may be."""
    p = detector.DEFAULT
    out, total = 0, 0
    for (k, h, w, n), name in R.LABEL_CASES:
        f = R.measures(R.content(name, k, h, w, n), k)
        out += int(R.left_out(f, p.coef, p.intercept, k).sum())
        total += len(f)
    assert total >= 12 and out <= 0.1 * total, f"{out} of {total} frames left out"
