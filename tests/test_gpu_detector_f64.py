"""GPU suite: the six focus measures of csrc/detector.hip against float64 (tests/detector_ref.py) at the shapes where the kernels
change path -- 16 x 16 tiles, the switch to the box path at k = 13, its 32-row (k >= 65: k/2+1-row) column segments, 256-column colsum
blocks and 64-column scan steps, the crop (H/k)*k and the DCT3 window count ((H-3)/k) -- and on content that is not a noisy texture:
smooth and bright, all zeros, constant 1.0, single impulses at the corners and at the crop edge.  The case table, the contents and the
tolerances are in tests/detector_ref.py; tests/test_detector_ref_cpu.py shows that the table sees an off-by-one in each of them.

The kernels are driven through `detector.gray_focus_measures`: the gray plane is the input and holds exact values.

Largest error against float64 measured on an MI355X over the whole table (|kernel - float64| / |float64|; on the zero, constant and
impulse frames over max(|float64|, largest per-pixel term)), and the case it comes from; the tolerance of each measure is 8 times its
figure (detector_ref.MEASURED, detector_ref.TOL):

    k < 13 (direct box sums, sequential DCT3 window sum)      k >= 13 (running box sums, telescoped DCT3 window sum)
    LAP1  9.12e-8  3, 17x33 smooth       tol 7.3e-7            1.29e-7  13, 33x257 smooth        tol 1.0e-6
    MIS3  1.12e-7  11, 97x131 texture    tol 9.0e-7            8.56e-8  13, 65x300 texture       tol 6.8e-7
    WAV1  2.48e-7  11, 97x131 ones       tol 2.0e-6            3.80e-7  201, 204x204 ones        tol 3.0e-6
    GRA7  1.28e-7  11, 14x14 texture     tol 1.0e-6            1.95e-7  201, 204x204 impulses    tol 1.6e-6
    STA3  1.38e-6  11, 14x14 smooth      tol 1.1e-5            2.51e-6  201, 230x440 smooth      tol 2.0e-5
    DCT3  3.04e-5  3, 6x6 smooth         tol 2.4e-4            1.75e-7  201, 204x204 smooth      tol 1.4e-6

Two findings above 1e-5, both DCT3, both the same accumulation: the window sum of the 4x4 mask responses cancels down to the corners of
the window (the responses telescope), so it is small against the responses it adds, and the sequential fp32 sum of det_dct_kernel keeps
their rounding.  For k >= 13 it lost up to 3.2e-5 (k = 65, 100x140 texture; 1.9e-5 at k = 201, 230x440), found with a CPU restatement
of the loop; the kernel now takes the telescoped sum there (differences of pixel values first) and the figure is 1.75e-7.  k <= 11 must
keep its bits (test_small_kernels_keep_the_parent_bits), so the loop stays: 3.04e-5 on the 6x6 smooth frame with its single window,
where DCT3 is 6.2e-5, the window sum 7.8e-3, and each of its nine responses adds eight pixel values near 0.8 that round at 6e-8 each; the
next largest DCT3 error on that path is 9.8e-6 (6x6 texture), 1.9e-6 from 14x14 up.  The smooth frames carry the largest STA3 errors
too (g - box(g) is small against g there), under 1e-5.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import detector_ref as R                      # noqa: E402
from speinet_amd import _lib, detector        # noqa: E402

DEV = "cuda:0"


def kernel_measures(gray: np.ndarray, k: int) -> np.ndarray:
    return detector.gray_focus_measures(torch.from_numpy(gray).to(DEV), k).cpu().numpy()


def case_errors(k, h, w, n, name):
    """(kernel [N,6] float32, float64 reference, allowed |difference|, |difference| over max(|ref|, the absolute scale)) of one
    content of one case; the last is the figure the tolerances were derived from."""
    x = R.content(name, k, h, w, n)
    out = kernel_measures(x, k)
    ref, terms = R.measures_and_terms(x, k)
    err = np.abs(out.astype(np.float64) - ref)
    scale = np.maximum(np.abs(ref), terms) if name in R.ABSOLUTE else np.abs(ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(scale > 0, err / scale, np.where(err > 0, np.inf, 0.0))
    return out, ref, R.bound(ref, terms, k, name), rel


@pytest.mark.parametrize("k,h,w,n", R.CASES)
def test_six_measures_vs_float64(k, h, w, n):
    bad = []
    for name in R.CONTENTS:
        out, ref, allowed, rel = case_errors(k, h, w, n, name)
        print(f"k={k} {h}x{w} {name}: max err " + " ".join(f"{f}={e:.2e}" for f, e in zip(R.FEATURES, rel.max(axis=0))))
        assert np.isfinite(out).all(), f"{name}: {out}"
        if name == "zeros":
            assert np.array_equal(out, np.zeros_like(out)), f"a black frame must measure 0.0 exactly: {out}"
        if name == "ones":
            assert np.array_equal(out[:, 5], np.zeros_like(out[:, 5])), f"every 4x4 mask response of a constant cancels in fp32: {out[:, 5]}"
        over = np.abs(out.astype(np.float64) - ref) > allowed
        for i, f in zip(*np.nonzero(over)):
            bad.append(f"{name} frame {i} {R.FEATURES[f]}: kernel {out[i, f]!r} float64 {ref[i, f]!r} relative {rel[i, f]:.3e} "
                       f"(tolerance {R.TOL[R.path_of(k)][f]:.1e})")
    assert not bad, "\n".join(bad)


def _five_frames(k, h, w):
    """Five frames of one size that each hold different content."""
    t = R.texture(h, w, 2, 5 + k)
    return np.concatenate([t, R.smooth(h, w, 1), np.ones((1, h, w), np.float32), R.impulses(h, w, k)[2:3]])


@pytest.mark.parametrize("k,h,w", [(11, 97, 131), (13, 65, 300)])
def test_batched_launch_reproduces_single_launches(k, h, w):
    x = _five_frames(k, h, w)
    assert len({f.tobytes() for f in x}) == 5
    batched = kernel_measures(x, k)
    for i in range(5):
        alone = kernel_measures(x[i:i + 1], k)
        assert np.array_equal(batched[i].view(np.int32), alone[0].view(np.int32)), f"frame {i}: batched {batched[i]} alone {alone[0]}"


@pytest.mark.parametrize("k", [11, 13])
def test_workspace_is_written_before_it_is_read_and_not_overrun(k):
    n, h, w, spare = 3, 33, 257, 4096
    lib = _lib.lib()
    gray = torch.from_numpy(R.texture(h, w, n, k)).to(DEV)
    floats = lib.spei_det_ws_floats(n, h, w, k)
    assert floats > 0
    outs = []
    for fill in (float("nan"), 0.0):
        ws = torch.full((floats + spare,), fill, device=DEV)
        out = torch.empty(n, 6, device=DEV)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.spei_det_features(C.c_void_p(gray.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), n, h, w, k, st),
                   "spei_det_features")
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
        tail = ws[floats:].cpu().numpy()
        assert (np.isnan(tail) if fill != 0.0 else tail == 0.0).all(), "the kernels wrote past spei_det_ws_floats"
    assert np.isfinite(outs[0]).all(), f"a workspace value was read before it was written: {outs[0]}"
    assert np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32))
    assert np.array_equal(outs[0].view(np.int32), kernel_measures(gray.cpu().numpy(), k).view(np.int32))


def test_labels_match_the_float64_labels():
    p = detector.DEFAULT
    compared = 0
    for (k, h, w, n), name in R.LABEL_CASES:
        x = R.content(name, k, h, w, n)
        ref = R.measures(x, k)
        keep = ~R.left_out(ref, p.coef, p.intercept, k)
        out = kernel_measures(x, k)
        assert np.array_equal(detector.predict(out)[keep], detector.predict(ref)[keep]), f"{name} {h}x{w}"
        compared += int(keep.sum())
    assert compared > 0
