"""The six focus measures of the LD detector restated in float64 numpy, from the definition in the header comment of
speinet_amd/csrc/detector.hip (not from the kernels): zero padding, the k x k mean divided by k^2 with the padded zeros counted, the
non-overlapping floor windows of lp_pool2d, DCT3 on the valid 4x4 response, WAV1 as oracle/detector_oracle.py's `wav1`.  Box sums come
from a float64 summed-area table, so k = 201 costs what k = 3 costs.  A helper of test_detector_ref_cpu.py and
test_gpu_detector_f64.py, which share the case table, the frame contents and the tolerances below.

`VARIANTS` names deliberately wrong restatements (an off-by-one each).  They are negative controls: the case table must be able to see
every one of them (test_detector_ref_cpu.py), or a kernel with that mistake would pass."""
import numpy as np

FEATURES = ("LAP1", "MIS3", "WAV1", "GRA7", "STA3", "DCT3")

DB6_DEC_LO = (-0.00107730108499558, 0.004777257511010651, 0.0005538422009938016, -0.031582039318031156,
              0.02752286553001629, 0.09750160558707936, -0.12976686756709563, -0.22626469396516913,
              0.3152503517092432, 0.7511339080215775, 0.4946238903983854, 0.11154074335008017)

VARIANTS = {
    "box_one_column_short": "the k x k box covers columns [-h, h-1] instead of [-h, h]",
    "right_clamp_w_minus_2": "the box's right edge is clamped at column W-2 instead of W-1",
    "crop_from_minus_1": "the window-covered region is ((H-1)/k)*k x ((W-1)/k)*k instead of (H/k)*k x (W/k)*k",
    "replicate_padding": "the frame is extended by its edge values instead of zeros",
    "dct_windows_from_w": "DCT3 has (H/k) x (W/k) windows instead of ((H-3)/k) x ((W-3)/k)",
    "wav_even_samples": "the DWT keeps the even samples of the full convolution instead of the odd ones",
}

BOX_SCAN_K = 13            # detector.hip: k < 13 sums the box directly, k >= 13 takes running column sums and row prefix sums


def path_of(k: int) -> str:
    return "direct" if k < BOX_SCAN_K else "scan"


# Largest |kernel - float64| over |float64| measured on an MI355X over the whole case table, per code path and measure (order of
# FEATURES); for the contents of ABSOLUTE the difference is taken over max(|float64|, largest per-pixel term).  Where each comes from
# is in the docstring of test_gpu_detector_f64.py.
MEASURED = {
    "direct": (9.12e-8, 1.12e-7, 2.48e-7, 1.28e-7, 1.38e-6, 3.04e-5),
    "scan": (1.29e-7, 8.56e-8, 3.80e-7, 1.95e-7, 2.51e-6, 1.75e-7),
}
# The tolerance of the GPU comparison: 8 times the measured error, room for another summation order and no more.
TOL = {path: tuple(8.0 * e for e in errs) for path, errs in MEASURED.items()}

# (k, H, W, frames per content): each shape is the smallest that reaches its edge
CASES = (
    (3, 6, 6, 3), (3, 17, 33, 3),                                        # minimum k + 3; partial 16 x 16 tiles
    (11, 14, 14, 3), (11, 97, 131, 3),                                   # last direct-box k; ragged
    (13, 16, 16, 3), (13, 33, 257, 3), (13, 64, 64, 3), (13, 65, 300, 3),  # first box-path k; one past a 32-row segment, a 256-column
                                                                         # colsum block and a 64-column scan step; exact multiples
    (51, 54, 54, 3), (51, 70, 129, 3),                                   # window over two segments; box wider than half the frame
    (65, 68, 68, 3), (65, 100, 140, 3),                                  # first k with seg = k/2 + 1
    (201, 204, 204, 3), (201, 230, 440, 3),                              # one window; k/2 clamps at both sides of every row
    (13, 40, 3840, 1), (37, 40, 3840, 1),                                # 4K-wide rows: 60 scan steps, the largest row prefix values
)
CONTENTS = ("texture", "smooth", "zeros", "ones", "impulses")
ABSOLUTE = ("zeros", "ones", "impulses")       # contents where a measure can be tiny or zero: atol = tol * max |per-pixel term|


def seed_of(k: int, h: int, w: int) -> int:
    return 1000 * k + h + w


def texture(h: int, w: int, n: int, seed: int) -> np.ndarray:
    """The suite's noisy texture (test_gpu_detector.py) as the fp32 gray plane in 0..1 its frames give: [n,h,w]."""
    r = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    f = np.stack([np.clip(128 + 90 * np.sin(0.05 * (i + 1) * yy) * np.cos(0.08 * xx) + (3 + 10 * i) * r.randn(3, h, w), 0, 255)
                  for i in range(n)]).astype(np.float32)
    return ((np.float32(0.2989) * f[:, 0] + np.float32(0.587) * f[:, 1] + np.float32(0.114) * f[:, 2]) / np.float32(255)).astype(np.float32)


def smooth(h: int, w: int, n: int) -> np.ndarray:
    """Smooth and bright: the uint8 values round(200 + 30 sin cos) over 255."""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    f = np.stack([np.rint(200 + 30 * np.sin(0.05 * (i + 1) * yy) * np.cos(0.08 * xx + 0.3 * i)) for i in range(n)])
    return (f.astype(np.float32) / np.float32(255)).astype(np.float32)


def impulses(h: int, w: int, k: int) -> np.ndarray:
    """One frame per position: a single 1.0 at (0,0), (H-1,W-1), (ch-1,cw-1) and, where it is inside the frame, (ch,cw)."""
    ch, cw = (h // k) * k, (w // k) * k
    pos = [(0, 0), (h - 1, w - 1), (ch - 1, cw - 1)] + ([(ch, cw)] if ch < h and cw < w else [])
    g = np.zeros((len(pos), h, w), np.float32)
    for i, (y, x) in enumerate(pos):
        g[i, y, x] = 1.0
    return g


def content(name: str, k: int, h: int, w: int, n: int) -> np.ndarray:
    """The fp32 gray frames [*,h,w] of one content of one case (`impulses` has one frame per position, whatever n)."""
    if name == "texture":
        return texture(h, w, n, seed_of(k, h, w))
    if name == "smooth":
        return smooth(h, w, n)
    if name == "zeros":
        return np.zeros((n, h, w), np.float32)
    if name == "ones":
        return np.ones((n, h, w), np.float32)
    if name == "impulses":
        return impulses(h, w, k)
    raise KeyError(name)


def _sat_box(vp: np.ndarray, h_out: int, w_out: int, k: int, short: bool) -> np.ndarray:
    """Sums of vp (the map extended by k/2 on every side) over the k x k box around every pixel of the h_out x w_out map."""
    n = vp.shape[0]
    sat = np.zeros((n, vp.shape[1] + 1, vp.shape[2] + 1))
    sat[:, 1:, 1:] = vp.cumsum(axis=1).cumsum(axis=2)
    y0, y1 = np.arange(h_out), np.arange(h_out) + k
    x0, x1 = np.arange(w_out), np.arange(w_out) + k - (1 if short else 0)
    return sat[:, y1][:, :, x1] - sat[:, y0][:, :, x1] - sat[:, y1][:, :, x0] + sat[:, y0][:, :, x0]


def _analysis(t: np.ndarray, filt, axis: int, keep: int) -> np.ndarray:
    """pywt 'zero' mode along one axis: the full convolution with `filt`, every second sample from `keep`."""
    t = np.moveaxis(t, axis, -1)
    length = t.shape[-1]
    tp = np.zeros(t.shape[:-1] + (length + 22,))
    tp[..., 11:11 + length] = t
    full = sum(filt[b] * tp[..., 11 - b:11 - b + length + 11] for b in range(12))
    return np.moveaxis(full[..., keep::2], -1, axis)


def measures_and_terms(gray, k: int, variant=None):
    """gray [N,H,W] float32 -> (the six measures [N,6] float64, the largest |per-pixel term| of each [N,6] float64).  A term is what
    the measure sums: lap8^2, the 8-neighbour contrast, |LH|+|HL|+|HH| of one coefficient, a squared box deviation, a squared window sum.
    `variant`: None for the definition, or a key of VARIANTS for that mistake."""
    if variant is not None and variant not in VARIANTS:
        raise KeyError(variant)
    g = np.asarray(gray)
    assert g.dtype == np.float32 and g.ndim == 3, "the reference takes the fp32 gray plane the kernel sees"
    g = g.astype(np.float64)
    n, H, W = g.shape
    assert k >= 1 and k % 2 == 1 and H >= k + 3 and W >= k + 3
    h = k // 2
    mode = "edge" if variant == "replicate_padding" else "constant"
    ch, cw = (H // k) * k, (W // k) * k
    nwin = (H // k) * (W // k)
    if variant == "crop_from_minus_1":
        ch, cw = ((H - 1) // k) * k, ((W - 1) // k) * k

    p = np.pad(g, ((0, 0), (1, 1), (1, 1)), mode=mode)
    v = [[p[:, a:a + H, b:b + W] for b in range(3)] for a in range(3)]
    c = v[1][1]
    nbrs = [v[a][b] for a in range(3) for b in range(3) if (a, b) != (1, 1)]
    lap2 = (sum(nbrs) - 8.0 * c) ** 2
    mis = sum(np.abs(c - q) for q in nbrs)
    gx = (v[0][0] - v[0][2]) + 2.0 * (v[1][0] - v[1][2]) + (v[2][0] - v[2][2])
    gy = (v[0][0] + 2.0 * v[0][1] + v[0][2]) - (v[2][0] + 2.0 * v[2][1] + v[2][2])
    sob = np.sqrt(gx * gx + gy * gy)

    def boxdev2(m):
        mp = np.pad(m, ((0, 0), (h, h), (h, h)), mode=mode)
        if variant == "right_clamp_w_minus_2":
            mp[:, :, h + W - 1] = 0.0
        return (m - _sat_box(mp, H, W, k, variant == "box_one_column_short") / float(k * k)) ** 2

    gd = g
    nwy, nwx = (H - 3) // k, (W - 3) // k
    if variant == "dct_windows_from_w":
        nwy, nwx = H // k, W // k
        gd = np.pad(g, ((0, 0), (0, 3), (0, 3)))
    rh, rw = gd.shape[1] - 3, gd.shape[2] - 3
    sgn = (1.0, 1.0, -1.0, -1.0)
    resp = sum(sgn[a] * sgn[b] * gd[:, a:a + rh, b:b + rw] for a in range(4) for b in range(4))
    dct = resp[:, :nwy * k, :nwx * k].reshape(n, nwy, k, nwx, k).sum(axis=(2, 4)) ** 2

    lo = np.asarray(DB6_DEC_LO)
    hi = np.asarray([(-1) ** (i + 1) * DB6_DEC_LO[11 - i] for i in range(12)])
    keep = 0 if variant == "wav_even_samples" else 1
    lo_w, hi_w = _analysis(g, lo, 2, keep), _analysis(g, hi, 2, keep)
    wav = np.abs(_analysis(lo_w, hi, 1, keep)) + np.abs(_analysis(hi_w, lo, 1, keep)) + np.abs(_analysis(hi_w, hi, 1, keep))

    crop = [t[:, :ch, :cw] for t in (lap2, mis, boxdev2(sob), boxdev2(g))]
    flat = lambda t: t.reshape(n, -1)                                                              # noqa: E731
    out = np.stack([flat(crop[0]).sum(1) / nwin, flat(crop[1]).sum(1) / nwin, flat(wav).sum(1), flat(crop[2]).sum(1) / nwin,
                    flat(crop[3]).sum(1) / nwin, flat(dct).sum(1) / (nwy * nwx)], axis=1)
    terms = np.stack([flat(crop[0]).max(1), flat(crop[1]).max(1), flat(wav).max(1), flat(crop[2]).max(1), flat(crop[3]).max(1),
                      flat(dct).max(1)], axis=1)
    return out, terms


def measures(gray, k: int, variant=None) -> np.ndarray:
    """gray [N,H,W] float32 -> the six measures [N,6] float64 (order of FEATURES)."""
    return measures_and_terms(gray, k, variant)[0]


def left_out(feat, coef, intercept, k: int) -> np.ndarray:
    """Frames [N] bool whose label the tolerances cannot pin: the margin |w.f + b| of the logistic regression on the float64 measures
    `feat` [N,6] is within sum |w_i| tol_i |f_i|, what a kernel inside its tolerances can move the score by."""
    f, w = np.asarray(feat, dtype=np.float64), np.asarray(coef, dtype=np.float64)
    return np.abs(f @ w + intercept) <= (np.abs(w) * np.asarray(TOL[path_of(k)]) * np.abs(f)).sum(axis=1)


LABEL_CASES = tuple((c, name) for c in CASES if c[0] == 11 for name in ("texture", "smooth"))       # default model: k = 11


def bound(ref: np.ndarray, terms: np.ndarray, k: int, name: str) -> np.ndarray:
    """The allowed |kernel - float64| [N,6] of one content of one case: tol * |ref|, and for the contents of ABSOLUTE, where a measure
    can be tiny against the terms it sums, tol * max |per-pixel term| where that is larger."""
    tol = np.asarray(TOL[path_of(k)])
    rel = tol * np.abs(ref)
    return np.maximum(rel, tol * terms) if name in ABSOLUTE else rel
