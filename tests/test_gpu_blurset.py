"""GPU suite: the run-average kernel spei_window_mean_u8 (csrc/blurset.hip) and `blurset.synthesize` on it: bit-exact against numpy
`sum // length` and the frame copy, on the reference's own outputs (golden G25) and on shapes that take the 16-byte path (H * W a
multiple of 16) and the per-pixel path; the gray plane bit-equal to frames_u8_in's on the kernel's own blurry frames."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from speinet_amd import _lib, blurset, ops      # noqa: E402

DEV = "cuda:0"


def _expect(frames, starts, lengths):
    blur = np.stack([(frames[s:s + n].astype(np.int64).sum(axis=0) // n).astype(np.uint8) for s, n in zip(starts, lengths)])
    gt = np.stack([frames[s + n // 2] for s, n in zip(starts, lengths)])
    return blur, gt


def _gray_of(u8):
    """The detector's gray plane of uint8 frames [N,H,W,3]: frames_u8_in(gray=True), or, for frames too small for its reflect padding
    (the pad to a multiple of 20 must be smaller than the frame), spei_det_gray on the frames as fp32 0..255, which the header
    declares bit-identical."""
    n, h, w, _ = u8.shape
    if ops.padded_size(h) - h < h and ops.padded_size(w) - w < w:
        return ops.frames_u8_in(u8, gray=True, planes=False)[1]
    rgb = u8.permute(0, 3, 1, 2).float().contiguous()
    g = torch.empty(n, h, w, device=u8.device)
    _lib.check(_lib.lib().spei_det_gray(C.c_void_p(rgb.data_ptr()), C.c_void_p(g.data_ptr()), n, h, w,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "spei_det_gray")
    return g


def _check(frames, starts, lengths, src=None):
    src = torch.from_numpy(frames).to(DEV) if src is None else src
    blur, gt, gray = ops.window_mean_u8(src, starts, lengths, gray=True)
    want_blur, want_gt = _expect(frames, starts, lengths)
    assert np.array_equal(blur.cpu().numpy(), want_blur)
    assert np.array_equal(gt.cpu().numpy(), want_gt)
    assert torch.equal(gray, _gray_of(blur))
    plain = ops.window_mean_u8(src, starts, lengths)
    assert plain[2] is None and torch.equal(plain[0], blur) and torch.equal(plain[1], gt)


def test_g25_reference_outputs(golden_dir):
    g25 = np.load(os.path.join(golden_dir, "g25_blurset.npz"))
    frames = g25["frames"]
    for i, (ratio, seed) in enumerate(zip(g25["ratios"], g25["seeds"])):
        runs = blurset.plan_runs(len(frames), float(ratio), rng=random.Random(int(seed)))
        for source in (frames, torch.from_numpy(frames), torch.from_numpy(frames).to(DEV), [f for f in frames]):
            for chunk in (64, 15):
                blur, gt = blurset.synthesize(source, runs, DEV, chunk_frames=chunk)
                assert np.array_equal(blur.cpu().numpy(), g25[f"blurry_{i}"].transpose(0, 2, 3, 1).astype(np.uint8))
                assert np.array_equal(gt.cpu().numpy(), g25[f"gt_{i}"].transpose(0, 2, 3, 1))
        blur, gt, gray = blurset.synthesize(frames, runs, DEV, gray=True)
        assert torch.equal(gray, ops.frames_u8_in(blur, gray=True, planes=False)[1])


@pytest.mark.parametrize("h,w", [(20, 20), (37, 53), (1, 1), (1, 16), (3, 7), (64, 48), (720, 1280)])
def test_kernel_bit_exact(h, w):
    r = np.random.RandomState(h * 1000 + w)
    T = 40 if h * w < 100000 else 33
    frames = r.randint(0, 256, (T, h, w, 3)).astype(np.uint8)
    frames[1] = 255                                               # the largest sums
    frames[2] = 255
    starts = [0, 0, 1, 3, 5, T - 15, T - 1, T - 2, 7]
    lengths = [1, 15, 2, 2, 15, 15, 1, 2, 7]                      # 1, 2 and 15; three runs end at the last frame; runs may overlap
    _check(frames, starts, lengths)


def test_every_length_and_quotient():
    """Every length 1..15 on frames that hold every byte value, so that every sum of equal bytes and many mixed sums are divided."""
    r = np.random.RandomState(7)
    frames = r.randint(0, 256, (15, 32, 32, 3)).astype(np.uint8)
    frames[:, :16, :16, 0] = np.arange(256, dtype=np.uint8).reshape(16, 16)
    _check(frames, [0] * 15, list(range(1, 16)))


def test_misaligned_and_strided_sources_take_the_pixel_path():
    r = np.random.RandomState(9)
    frames = r.randint(0, 256, (20, 16, 16, 3)).astype(np.uint8)
    starts, lengths = [0, 4, 10, 18], [4, 6, 8, 2]
    flat = torch.zeros(20 * 16 * 16 * 3 + 64, dtype=torch.uint8, device=DEV)
    off = flat[3:3 + frames.size].view(20, 16, 16, 3)             # base address 3 bytes past an aligned one
    off.copy_(torch.from_numpy(frames))
    _check(frames, starts, lengths, src=off)
    wide = torch.zeros(20, 16 * 16 * 3 + 8, dtype=torch.uint8, device=DEV)
    wide[:, :16 * 16 * 3] = torch.from_numpy(frames).to(DEV).view(20, -1)
    strided = wide[:, :16 * 16 * 3].view(20, 16, 16, 3)           # frame stride 776 bytes: a multiple of 8, not of 16
    assert strided.stride(0) == 16 * 16 * 3 + 8
    _check(frames, starts, lengths, src=strided)


def test_bad_arguments_launch_nothing():
    lib = _lib.lib()
    src = torch.zeros(10, 20, 20, 3, dtype=torch.uint8, device=DEV)
    blur = torch.full((2, 20, 20, 3), 7, dtype=torch.uint8, device=DEV)
    gt = torch.full((2, 20, 20, 3), 7, dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(runs, src_p=None, blur_p=None, gt_p=None, runs_null=False):
        host = torch.tensor(runs, dtype=torch.int32)
        dev = host.to(DEV)
        rc = lib.spei_window_mean_u8(C.c_void_p(src.data_ptr() if src_p is None else src_p), src.stride(0), 10,
                                     C.c_void_p(0 if runs_null else dev.data_ptr()), C.c_void_p(host.data_ptr()), host.shape[0],
                                     C.c_void_p(blur.data_ptr() if blur_p is None else blur_p),
                                     C.c_void_p(gt.data_ptr() if gt_p is None else gt_p), C.c_void_p(0), 20, 20, st)
        torch.cuda.synchronize()
        return rc, lib.spei_last_error().decode()

    for runs, kw, text in (([[0, 0], [1, 2]], {}, "length 0"), ([[0, 16], [1, 2]], {}, "length 16"), ([[0, 2], [8, 3]], {}, "leaves the clip"),
                           ([[-1, 2], [1, 2]], {}, "leaves the clip"), ([[0, 2], [1, 2]], {"src_p": 0}, "null pointer"),
                           ([[0, 2], [1, 2]], {"blur_p": 0}, "null pointer"), ([[0, 2], [1, 2]], {"gt_p": 0}, "null pointer"),
                           ([[0, 2], [1, 2]], {"runs_null": True}, "null pointer")):
        rc, err = call(runs, **kw)
        assert rc != 0 and text in err, (runs, kw, rc, err)
        assert int(blur.min()) == 7 and int(blur.max()) == 7 and int(gt.min()) == 7 and int(gt.max()) == 7
    with pytest.raises(RuntimeError, match="leaves the clip"):
        ops.window_mean_u8(src, [0, 9], [2, 2])
    with pytest.raises(ValueError):
        blurset.synthesize(src, ([0, 9], [2, 2]), DEV)
    rc, _ = call([[0, 2], [8, 2]])
    assert rc == 0 and int(blur.max()) == 0
