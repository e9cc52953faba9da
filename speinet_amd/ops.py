"""Thin tensor-level wrappers over the C-ABI (include/speinet_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every arithmetic step is one of the HIP
kernels in speinet_amd/csrc.  There is no fallback: a missing library or a failed call raises.

All state of a call lives in a `Ctx` (arithmetic mode, storage knobs, device, optional per-op timing hook): there is
NO process-global mode — two models with different modes can run from two threads (the reference's nn.DataParallel
calls `forward` from one Python thread per device, model/__init__.py:19-20; SURVEY.md §8b "threading").
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Optional

import numpy as np
import torch

from . import _lib, y4m
from . import codec as _codec
from . import light as _light
from . import shake as _shake
from .pack import BF16, F16, F32, LP_DTYPE, PackedW, fmt_of

ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
CONV, CONV_T = 0, 1

# Arithmetic of the GEMM-shaped kernels (convolutions, linears, correlation); everything else is always fp32.
#   "f32"    v_mfma_f32_32x32x2_f32, exact fp32 (the PSNR-parity configuration)
#   "bf16x3" split-bf16 products on v_mfma_f32_32x32x16_bf16: f32-grade results at 3/16 of the f32 MFMA cost
#   "bf16"   single bf16 products, fp32 accumulate (BASELINE.json configs[1] as written: 8-bit significands)
#   "f16"    single IEEE-half products, fp32 accumulate: the same matrix-pipe rate with 11-bit significands — the
#            throughput configuration that also holds the 1e-3 dB PSNR bound; range +-65504
# Correlation arg-max when precision != "f32" (16-bit products use the format of `precision`, bf16 unless "f16"):
#   "bf16x3" f32-grade scores;  "single" one 16-bit product per MAC (the winner may flip between near-ties);
#   "top2"   single products keeping the TWO best candidates of every query, then an exact re-score of both on the fp32
#            maps with fp64 accumulation (spei_corr_rescore): f32-grade winners and S at the cost of the 16-bit kernel
PRECISIONS = ("f32", "bf16x3", "bf16", "f16")
CORR_PRECISIONS = ("bf16x3", "single", "top2")
_CORR_ALIASES = {"bf16": "single", "bf16r": "top2", "f16": "single"}


class FMap:
    """NHWC feature map view (fp32, or bf16 / half for GEMM-only intermediates): rows = pixels, `C` channels starting at
    column `off` of a [H*W, ld] buffer."""
    __slots__ = ("t", "H", "W", "C", "ld", "off")

    def __init__(self, t: torch.Tensor, H: int, W: int, C_: int, off: int = 0):
        assert t.is_cuda and t.dtype in (torch.float32, torch.bfloat16, torch.float16) and t.is_contiguous() and t.dim() == 2 and t.shape[0] == H * W
        self.t, self.H, self.W, self.C, self.ld, self.off = t, H, W, C_, t.shape[1], off
        assert off + C_ <= self.ld

    @staticmethod
    def empty(H: int, W: int, C_: int, device, dtype=torch.float32) -> "FMap":
        return FMap(torch.empty(H * W, C_, device=device, dtype=dtype), H, W, C_)

    @property
    def lp(self) -> bool:
        """Stored as 16-bit (bf16 or half)."""
        return self.t.dtype != torch.float32

    @property
    def fmt(self) -> int:
        return fmt_of(self.t.dtype)

    def view(self, off: int, C_: int) -> "FMap":
        return FMap(self.t, self.H, self.W, C_, self.off + off)

    @property
    def ptr(self) -> int:
        return self.t.data_ptr() + self.t.element_size() * self.off

    def dense(self) -> torch.Tensor:
        """[H, W, C] copy-free when the view spans the whole buffer."""
        return self.t[:, self.off:self.off + self.C].float().reshape(self.H, self.W, self.C)

    def nchw(self) -> torch.Tensor:
        return self.dense().permute(2, 0, 1).unsqueeze(0).contiguous()

    @staticmethod
    def from_nchw(x: torch.Tensor) -> "FMap":
        """[1,C,H,W] or [C,H,W] -> NHWC map (test helper; the forward pass itself never converts through torch)."""
        if x.dim() == 4:
            x = x[0]
        c, h, w = x.shape
        return FMap(x.permute(1, 2, 0).reshape(h * w, c).contiguous().float(), h, w, c)


class BMap:
    """`B` dense NHWC maps of one shape stacked in one buffer [B*H*W, C] (fp32 or the mode's 16-bit format): the frame's encoder
    passes through one layer, launched together (gridDim.y = map; csrc/conv_slab16.hip, resblock.hip).  `map(b)` is map b as an FMap
    view."""
    __slots__ = ("t", "B", "H", "W", "C")

    def __init__(self, t: torch.Tensor, B: int, H: int, W: int, C_: int):
        assert t.is_cuda and t.is_contiguous() and t.shape == (B * H * W, C_)
        self.t, self.B, self.H, self.W, self.C = t, B, H, W, C_

    @staticmethod
    def empty(B: int, H: int, W: int, C_: int, device, dtype=torch.float32) -> "BMap":
        return BMap(torch.empty(B * H * W, C_, device=device, dtype=dtype), B, H, W, C_)

    @property
    def fmt(self) -> int:
        return fmt_of(self.t.dtype)

    def map(self, b: int) -> FMap:
        n = self.H * self.W
        return FMap(self.t[b * n:(b + 1) * n], self.H, self.W, self.C)


def _vp(p) -> C.c_void_p:
    return C.c_void_p(p)


APPLY_MAX_ROUTES = 16          # SPEI_APPLY_MAX_ROUTES


class _ApplyRoute(C.Structure):
    """SpeiApplyRoute (include/speinet_hip.h)."""
    _fields_ = [("out32", C.c_void_p), ("out16", C.c_void_p), ("ld32", C.c_int32), ("src", C.c_int32), ("partner", C.c_int32),
                ("reserved", C.c_int32)]


class _timed:
    def __init__(self, ctx: "Ctx", name: str):
        self.on = ctx.profile is not None and name in ctx.profile
        self.ctx, self.name = ctx, name

    def __enter__(self):
        if self.on:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record(torch.cuda.current_stream(self.ctx.device))
        return self

    def __exit__(self, *a):
        if self.on:
            self.e.record(torch.cuda.current_stream(self.ctx.device))
            self.ctx.profile[self.name].append((self.s, self.e))
        return False


def _tensor_bytes(x) -> int:
    t = x.t if hasattr(x, "t") else x
    return t.numel() * t.element_size() if torch.is_tensor(t) else 0


def _conv_sub(method: str, a, k, out):
    """(sub-family, flops, activation bytes) of one conv-family launch: the 32-channel 5x5 layers at full resolution (the ResBlock convs of
    level 1 and the first / last conv) move 0.4-1.6 GB per launch for 0.3 TFLOP — their roofline is HBM, not the matrix pipe."""
    if method == "conv5_in":
        return "level1", 2.0 * 25 * 3 * 32 * a[0].shape[-2] * a[0].shape[-1], _tensor_bytes(a[0]) + _tensor_bytes(out)
    if method == "conv5_out":
        return "level1", 2.0 * 25 * 32 * 3 * a[0].H * a[0].W, _tensor_bytes(a[0]) + 12 * a[0].H * a[0].W
    src, n = a[0], a[3]
    ks = a[4] if len(a) > 4 else k.get("ksize", 1)
    if n == 32 and src.C == 32 and ks == 5 and k.get("stride", a[5] if len(a) > 5 else 1) == 1:
        maps = getattr(src, "B", 1)
        return "level1", 2.0 * 25 * 32 * 32 * maps * src.H * src.W, _tensor_bytes(src) + _tensor_bytes(out)
    return "rest", 0.0, 0


def _family(name: str):
    """Time every call of a leaf launch method when the caller asked for it: `profile["families"]` = {family: [(start, end), ...]} gets
    one HIP event pair per call on the launch stream (eager, single-stream passes only: bench.py's per-family roofline record); the
    conv family also by sub-family (`profile["conv_sub"]`: events, flops, bytes)."""
    def deco(fn):
        def wrapper(self, *a, **k):
            pr = self.profile
            if pr is None or "families" not in pr:
                return fn(self, *a, **k)
            st = torch.cuda.current_stream(self.device)
            s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s_.record(st)
            out = fn(self, *a, **k)
            e_.record(st)
            pr["families"].setdefault(name, []).append((s_, e_))
            if name == "conv":
                sub, fl, by = _conv_sub(fn.__name__, a, k, out)
                rec = pr.setdefault("conv_sub", {}).setdefault(sub, {"events": [], "flops": 0.0, "bytes": 0})
                rec["events"].append((s_, e_))
                rec["flops"] += fl
                rec["bytes"] += by
            return out
        wrapper.__name__, wrapper.__doc__ = fn.__name__, fn.__doc__
        return wrapper
    return deco


def frame_metrics(u8: torch.Tensor, gt_hwc: torch.Tensor, border: int = 4) -> torch.Tensor:
    """Harness metrics of one frame on the device (csrc/metrics.hip; reference inference_SPEINet.py:484-543): float64 [PSNR, SSIM] of
    the uint8 [H,W,3] frame `u8` (`frame_u8_out`'s) against gt_hwc on the border-cropped region, three launches on the current stream
    of the tensors' device, no host sync."""
    assert u8.is_cuda and u8.dtype == torch.uint8 and u8.dim() == 3 and u8.shape[2] == 3 and u8.is_contiguous()
    h, w = u8.shape[:2]
    assert gt_hwc.shape == u8.shape and gt_hwc.dtype == torch.uint8 and gt_hwc.device == u8.device and gt_hwc.is_contiguous()
    lib = _lib.lib()
    n = lib.spei_frame_metrics_ws_doubles(h, w, border)
    if n < 0:
        raise ValueError(f"frame {w}x{h} with border {border} is smaller than the 11x11 SSIM window")
    dev = u8.device
    ws = torch.empty(n, dtype=torch.float64, device=dev)
    res = torch.empty(2, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.spei_frame_metrics(_vp(u8.data_ptr()), _vp(gt_hwc.data_ptr()), h, w, border, _vp(ws.data_ptr()), _vp(res.data_ptr()),
                                          st), "spei_frame_metrics")
    return res


def padded_size(n: int) -> int:
    """The model's frame size for a frame dimension of n: the next multiple of 20 (two stride-2 stages, then 5x5 windows)."""
    return -(-n // 20) * 20


def _frames_in(fr: torch.Tensor, dtype, depth: Optional[int], out: Optional[torch.Tensor], gray: bool, planes: bool):
    """`frames_u8_in` (`depth` None) and `frames_u16_in` on frames of `dtype`."""
    assert fr.is_cuda and fr.dtype == dtype and fr.dim() in (3, 4) and (planes or gray)
    if fr.dim() == 3:
        fr = fr.unsqueeze(0)
    n, h, w, c = fr.shape
    assert c == 3 and fr.stride()[1:] == (w * 3, 3, 1), "frames must be packed [H,W,3] (any frame stride)"
    hp, wp = padded_size(h), padded_size(w)
    dev = fr.device
    if planes:
        if out is None:
            out = torch.empty(n, 3, hp, wp, device=dev)
        assert out.is_cuda and out.device == dev and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n * 3 * hp * wp
    else:
        out = None
    g = torch.empty(n, h, w, device=dev) if gray else None
    lib = _lib.lib()
    name = "spei_frames_u8_in" if depth is None else "spei_frames_u16_in"
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(getattr(lib, name)(_vp(fr.data_ptr()), fr.element_size() * fr.stride(0), _vp(out.data_ptr() if out is not None else 0),
                                      _vp(g.data_ptr() if g is not None else 0), n, h, w, *(() if depth is None else (depth,)), st), name)
    return out, g


def frames_u8_in(u8: torch.Tensor, out: Optional[torch.Tensor] = None, gray: bool = False, planes: bool = True):
    """uint8 frames [N,H,W,3] (or one [H,W,3]; each frame packed, any frame stride) on the device -> (fp32 [N,3,Hp,Wp] reflect-padded
    to multiples of 20 with `numpy2tensor`'s values, or None when not `planes`; the detector's gray plane [N,H,W], or None when not
    `gray`).  `out` (optional): the planes' destination, contiguous, N*3*Hp*Wp floats.  One launch on the current stream (csrc/frame_io.hip)."""
    return _frames_in(u8, torch.uint8, None, out, gray, planes)


def _pair_stats(fr: torch.Tensor, dtype, depth: Optional[int], prev: Optional[torch.Tensor]):
    """`frame_pair_stats` (`depth` None) and `frame_pair_stats_u16` on frames of `dtype`."""
    assert fr.is_cuda and fr.dtype == dtype and fr.dim() == 4
    n, h, w, c = fr.shape
    assert c == 3 and fr.stride()[1:] == (w * 3, 3, 1), "frames must be packed [H,W,3] (any frame stride)"
    dev = fr.device
    assert prev is None or (prev.device == dev and prev.dtype == dtype and tuple(prev.shape) == (h, w, 3) and prev.is_contiguous())
    pairs = n if prev is not None else n - 1
    hist = torch.empty(n, 64, dtype=torch.int32, device=dev)
    sad = torch.empty(pairs, dtype=torch.int64, device=dev)
    lib = _lib.lib()
    name = "spei_frame_pair_stats" if depth is None else "spei_frame_pair_stats_u16"
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(getattr(lib, name)(_vp(fr.data_ptr()), fr.element_size() * fr.stride(0), _vp(prev.data_ptr() if prev is not None else 0),
                                      n, h, w, *(() if depth is None else (depth,)), _vp(hist.data_ptr()), _vp(sad.data_ptr()), st), name)
    return sad, hist.long()


def frame_pair_stats(u8: torch.Tensor, prev: Optional[torch.Tensor] = None):
    """Pair statistics of consecutive uint8 frames [N,H,W,3] on the device (each frame packed, any frame stride), optionally with the
    packed frame `prev` [H,W,3] before them, on the integer luma Y = (77 R + 150 G + 29 B + 128) >> 8 (csrc/frame_io.hip) ->
    (sad int64 [N-1], or [N] with `prev` (pair 0 is then (prev, frame 0)): the sum over pixels of |Y_a - Y_b| per consecutive pair;
    hist int64 [N,64]: pixels per value of Y >> 2).  Exact integers.  One launch on the current stream, no host sync."""
    return _pair_stats(u8, torch.uint8, None, prev)


def _depth(depth: int) -> int:
    if depth not in (10, 12):
        raise ValueError(f"depth must be 10 or 12 (bits per sample in uint16 words), got {depth!r}")
    return int(depth)


def frames_u16_in(u16: torch.Tensor, depth: int, out: Optional[torch.Tensor] = None, gray: bool = False, planes: bool = True):
    """`frames_u8_in` for deep frames: uint16 [N,H,W,3] (or one [H,W,3]; each frame packed, any frame stride) of `depth` 10 or 12 bits,
    D = 2^depth - 1 (a word above D reads as D) -> (fp32 [N,3,Hp,Wp] = v * float32(1 / D), reflect-padded, or None when not `planes`;
    the detector's gray plane [N,H,W] of the frames as fp32 v * float32(255 / D), or None when not `gray`).  One launch on the
    current stream (csrc/frame_io.hip)."""
    return _frames_in(u16, torch.uint16, _depth(depth), out, gray, planes)


def frame_pair_stats_u16(u16: torch.Tensor, depth: int, prev: Optional[torch.Tensor] = None):
    """`frame_pair_stats` for deep frames: uint16 [N,H,W,3] of `depth` 10 or 12 bits (and optionally the packed frame `prev` before
    them), on the depth-bit luma Yd = (77 R + 150 G + 29 B + 128) >> 8 -> (sad int64 over Yd, 2^(depth-8) times the 8-bit unit;
    hist int64 [N,64]: pixels per value of Yd >> (depth - 6)).  Exact integers.  One launch on the current stream, no host sync."""
    return _pair_stats(u16, torch.uint16, _depth(depth), prev)


def _stage_args(light, noise, shake, dev, put):
    """What `window_mean_u8` and `Ctx.train_batch_runs` share: -> (the infix of the entry to call — "" for the light `code`, "_light",
    "_noise" or "_shake" —, its arguments between the run table and the outputs: the light's tables; gauss table, noise records and
    keys; PSFs and shake records —, and the tensors those arguments point into, for the caller to hold until it has launched).
    `noise`: None or (records, seed); `shake`: None or (records, PSFs as an array or a `shake.device_psfs` pair); `put(what, records,
    record dtype)` -> the caller's records as (device, host) uint8 tensors.  A shake launch without noise takes NULL for the noise
    group, a table without PSFs NULL for the table."""
    if noise is not None and _light.is_code(light):
        raise ValueError("noise is added in linear light: give a light 'srgb' or 'gamma:<g>' beside it (--light / --blur_light), not 'code'")
    if shake is not None and _light.is_code(light):
        raise ValueError("shake is applied in linear light: give a light 'srgb' or 'gamma:<g>' beside it (--light / --blur_light), not 'code'")
    if _light.is_code(light):
        return "", [], []
    keep = []                                                # every tensor an argument points into: the caller holds it over the launch

    def p(*tensors):
        keep.extend(tensors)
        return [C.c_void_p(t.data_ptr()) for t in tensors]

    args = p(*_light.device_tables(light, dev))
    if noise is not None:
        args += p(*_light.device_gauss(dev), *put("noise", noise[0], _light.NOISE_RECORD)) + list(_light.key_of(noise[1]))
    elif shake is not None:
        args += [None] * 4 + [0, 0]
    if shake is not None:
        psf_dev, psf_host = shake[1] if isinstance(shake[1], tuple) else _shake.device_psfs(shake[1], dev)
        n_psf = psf_host.numel() // (_shake.SIDE * _shake.SIDE)
        args += (p(psf_dev, psf_host) if n_psf else [None, None]) + [n_psf] + p(*put("shake", shake[0], _shake.SHAKE_RECORD))
    return "_shake" if shake is not None else "_noise" if noise is not None else "_light", args, keep


def window_mean_u8(u8: torch.Tensor, starts, lengths, gray: bool = False, blur: Optional[torch.Tensor] = None,
                   gt: Optional[torch.Tensor] = None, light=None, noise=None, shake=None):
    """The reference's blur synthesis on resident frames (csrc/blurset.hip): uint8 frames [T,H,W,3] on the device (each frame packed,
    any frame stride) and M runs `starts[m]`, `lengths[m]` (1..15 frames, inside the clip) -> (blur uint8 [M,H,W,3] = the per-byte
    integer mean of each run, gt uint8 [M,H,W,3] = the run's middle frame `start + length // 2`, the detector's gray plane [M,H,W] of
    the blurry frames or None when not `gray`).  `blur` / `gt` (optional): contiguous destinations.  One launch on the current stream;
    the runs are checked on the host before it.  `light`: None or "code" is that launch (spei_window_mean_u8); "srgb" or "gamma:<g>"
    averages in linear light (speinet_amd.light, spei_window_mean_light_u8), the gray plane still that of the encoded bytes.  `noise`:
    None, or (records, seed) — one speinet_amd.light.NOISE_RECORD per run (its run and clip ids and the clip's levels A, B) and the
    seed that keys the generator: sensor noise is added in that linear light (spei_window_mean_noise_u8); with "code" a ValueError.
    `shake`: None (exactly the launches above), or (records, psf_table) — one speinet_amd.shake.SHAKE_RECORD per run and the uint32
    [n,33,33] PSFs they index (an array, or a (device, host) pair of `shake.device_psfs`): the run's linear mean is correlated with its
    PSF before the noise and the encode (spei_window_mean_shake_u8); with "code" a ValueError."""
    assert u8.is_cuda and u8.dtype == torch.uint8 and u8.dim() == 4
    t, h, w, c = u8.shape
    assert c == 3 and u8.stride()[1:] == (w * 3, 3, 1), "frames must be packed [H,W,3] (any frame stride)"
    runs_host = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(starts), np.asarray(lengths)], axis=1).astype(np.int32)))
    m = runs_host.shape[0]
    dev = u8.device
    for name, buf in (("blur", blur), ("gt", gt)):
        assert buf is None or (buf.device == dev and buf.dtype == torch.uint8 and tuple(buf.shape) == (m, h, w, 3) and buf.is_contiguous()), name
    blur = torch.empty(m, h, w, 3, dtype=torch.uint8, device=dev) if blur is None else blur
    gt = torch.empty(m, h, w, 3, dtype=torch.uint8, device=dev) if gt is None else gt
    g = torch.empty(m, h, w, device=dev) if gray else None
    lib = _lib.lib()
    with torch.cuda.device(dev):
        runs = runs_host.to(dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def put(what, rec, dtype):                           # the caller's arrays, uploaded per call
            rec = np.ascontiguousarray(rec, dtype=dtype).reshape(-1)
            if rec.size != m:
                raise ValueError(f"{what}: {rec.size} records for {m} runs")
            host = torch.from_numpy(rec.view(np.uint8).copy())
            return host.to(dev), host

        infix, stages, _held = _stage_args(light, noise, shake, dev, put)
        _lib.check(getattr(lib, f"spei_window_mean{infix}_u8")(_vp(u8.data_ptr()), u8.stride(0), t, _vp(runs.data_ptr()), _vp(runs_host.data_ptr()), m,
                                                              *stages, _vp(blur.data_ptr()), _vp(gt.data_ptr()),
                                                              _vp(g.data_ptr() if g is not None else 0), h, w, st), f"spei_window_mean{infix}_u8")
    return blur, gt, g


def _qtabs(qtabs, dev):
    """(device, host, n) of quantisation tables given as a uint16 [n,2,64] array or as a `codec.device_qtabs` pair."""
    q_dev, q_host = qtabs if isinstance(qtabs, tuple) else _codec.device_qtabs(qtabs, dev)
    assert q_dev.is_cuda and q_dev.device == dev and not q_host.is_cuda and q_host.dtype == q_dev.dtype == torch.int16 \
        and q_host.is_contiguous() and q_dev.is_contiguous() and q_host.numel() == q_dev.numel() and q_host.numel() % 128 == 0
    return q_dev, q_host, q_host.numel() // 128


def codec_u8(frames: torch.Tensor, records, qtabs, gray: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The JPEG-style round trip of speinet_amd.codec IN PLACE on uint8 frames [N,H,W,3] on the device (each frame packed, any frame
    stride; csrc/codec.hip, spei_codec_u8): `records` one speinet_amd.codec.CODEC_RECORD per frame (its tables' index, the grid offsets
    oy, ox in 0..15, flags 0 or codec.SKIP), `qtabs` the uint16 [n,2,64] tables they index (an array, or a (device, host) pair of
    `codec.device_qtabs`).  `gray` (optional): the frames' contiguous fp32 [N,H,W] gray planes, rewritten for every coded frame to
    `frames_u8_in`'s plane of the new bytes.  One launch on the current stream; records and tables are checked on the host before it.
    -> frames."""
    assert frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4
    n, h, w, c = frames.shape
    assert c == 3 and frames.stride()[1:] == (w * 3, 3, 1), "frames must be packed [H,W,3] (any frame stride)"
    dev = frames.device
    assert gray is None or (gray.device == dev and gray.dtype == torch.float32 and tuple(gray.shape) == (n, h, w) and gray.is_contiguous())
    rec = np.ascontiguousarray(records, dtype=_codec.CODEC_RECORD).reshape(-1)
    if rec.size != n:
        raise ValueError(f"codec: {rec.size} records for {n} frames")
    with torch.cuda.device(dev):
        rec_host = torch.from_numpy(rec.view(np.uint8).copy())
        rec_dev = rec_host.to(dev)
        q_dev, q_host, n_qtab = _qtabs(qtabs, dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.lib().spei_codec_u8(_vp(frames.data_ptr()), frames.stride(0), n, h, w, _vp(rec_dev.data_ptr()), _vp(rec_host.data_ptr()),
                                            _vp(q_dev.data_ptr()), _vp(q_host.data_ptr()), n_qtab, _vp(gray.data_ptr() if gray is not None else 0),
                                            st), "spei_codec_u8")
    return frames


def _frame_out(x: torch.Tensor, h: int, w: int, depth: Optional[int], out: Optional[torch.Tensor], nonfinite: Optional[torch.Tensor]):
    """`frame_u8_out` (`depth` None) and `frame_u16_out`."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[0] == 3 and x.is_contiguous()
    dtype = torch.uint8 if depth is None else torch.uint16
    hp, wp = x.shape[1:]
    if out is None:
        out = torch.empty(h, w, 3, dtype=dtype, device=x.device)
    assert out.device == x.device and out.dtype == dtype and tuple(out.shape) == (h, w, 3) and out.is_contiguous()
    assert nonfinite is None or (nonfinite.device == x.device and nonfinite.dtype == torch.int32 and nonfinite.numel() >= 1)
    lib = _lib.lib()
    name = "spei_frame_u8_out" if depth is None else "spei_frame_u16_out"
    with torch.cuda.device(x.device):
        st = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(getattr(lib, name)(_vp(x.data_ptr()), _vp(out.data_ptr()), _vp(nonfinite.data_ptr() if nonfinite is not None else 0),
                                      h, w, hp, wp, *(() if depth is None else (depth,)), st), name)
    return out


def frame_u8_out(x: torch.Tensor, h: int, w: int, out: Optional[torch.Tensor] = None,
                 nonfinite: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [3,Hp,Wp] on the device -> its top-left h x w crop as uint8 [h,w,3] (`tensor2numpy`'s values, 0 for a non-finite value).
    `out` (optional): a packed uint8 [h,w,3] destination.  `nonfinite` (optional): an int32 device tensor whose first element becomes
    nonzero iff the crop held a NaN or an infinity.  Launches on the current stream (csrc/frame_io.hip), no host sync."""
    return _frame_out(x, h, w, None, out, nonfinite)


def frame_u16_out(x: torch.Tensor, h: int, w: int, depth: int, out: Optional[torch.Tensor] = None,
                  nonfinite: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`frame_u8_out` for deep frames: fp32 [3,Hp,Wp] on the device -> its top-left h x w crop as uint16 [h,w,3] of `depth` 10 or 12
    bits, round_half_even(clamp(x * D, 0, D)) with D = 2^depth - 1, 0 for a non-finite value.  `out` (optional): a packed uint16
    [h,w,3] destination.  `nonfinite`: as in `frame_u8_out`.  Launches on the current stream (csrc/frame_io.hip), no host sync."""
    return _frame_out(x, h, w, _depth(depth), out, nonfinite)


def _int_table(values, n: int, what: str):
    """A host table of n ints for the tile entry points (read during the call)."""
    vals = [int(v) for v in values]
    if len(vals) != n:
        raise ValueError(f"the tile plan's {what} has {len(vals)} entries, not {n}")
    return (C.c_int * n)(*vals)


def tiles_in(frame: torch.Tensor, plan, out: torch.Tensor, depth: Optional[int] = None) -> torch.Tensor:
    """One packed frame [H,W,3] on the device, uint8 (`depth` None) or uint16 of `depth` 10 or 12 bits -> every tile of `plan` (a
    `tiles.TilePlan`, or anything with its fields) as fp32 planes in `out` [plan.n, 3, thp, twp]: tile k = i * cols + j is
    bit-identical to `frames_u8_in` / `frames_u16_in` on the crop frame[y0[i] : y0[i] + th, x0[j] : x0[j] + tw], reflect pad included.
    `out` may be a view with any tile stride (a multiple of 4 floats) whose tiles are contiguous, such as x[:, j] of the window inputs
    [n, n_seq + 2, 3, thp, twp] of all tiles.  One launch on the current stream (csrc/tile_io.hip), no host sync."""
    deep = frame.dtype == torch.uint16
    assert frame.is_cuda and frame.dtype in (torch.uint8, torch.uint16) and frame.dim() == 3 and frame.shape[2] == 3 and frame.is_contiguous()
    if deep:
        depth = _depth(depth)
    elif depth is not None:
        raise ValueError(f"depth= applies to uint16 frames only; the frame is {frame.dtype}")
    h, w = frame.shape[:2]
    if (h, w) != (plan.H, plan.W):
        raise ValueError(f"the tile plan is for a {plan.W}x{plan.H} frame, the frame is {w}x{h}")
    thp, twp = padded_size(plan.th), padded_size(plan.tw)
    n = plan.rows * plan.cols
    assert out.is_cuda and out.device == frame.device and out.dtype == torch.float32 and tuple(out.shape) == (n, 3, thp, twp)
    assert out.stride()[1:] == (thp * twp, twp, 1), "every tile of out must be contiguous (any tile stride)"
    y0, x0 = _int_table(plan.y0, plan.rows, "y0"), _int_table(plan.x0, plan.cols, "x0")
    lib = _lib.lib()
    with torch.cuda.device(frame.device):
        st = C.c_void_p(torch.cuda.current_stream(frame.device).cuda_stream)
        stride = out.stride(0) if n > 1 else 3 * thp * twp
        if deep:
            _lib.check(lib.spei_tiles_u16_in(_vp(frame.data_ptr()), h, w, _vp(out.data_ptr()), stride, y0, x0, plan.rows, plan.cols,
                                             plan.th, plan.tw, depth, st), "spei_tiles_u16_in")
        else:
            _lib.check(lib.spei_tiles_u8_in(_vp(frame.data_ptr()), h, w, _vp(out.data_ptr()), stride, y0, x0, plan.rows, plan.cols,
                                            plan.th, plan.tw, st), "spei_tiles_u8_in")
    return out


def tiles_out(tiles, plan, out_depth: int = 8, out: Optional[torch.Tensor] = None,
              nonfinite: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The tiles of `plan` (plan.n contiguous fp32 [3,thp,twp] tensors on one device, or one tensor of them; tile k = i * cols + j)
    -> the stitched frame, uint8 [H,W,3] for `out_depth` 8 and uint16 for 10 and 12: pixel (y, x) of band [yb[i], yb[i+1]) x
    [xb[j], xb[j+1]) has `frame_u8_out` / `frame_u16_out`'s value of tile (i, j) at (y - y0[i], x - x0[j]).
    `out` (optional): the packed destination.  `nonfinite` (optional): an int32 device tensor whose first element becomes nonzero iff
    a value that a pixel was made from was a NaN or an infinity (that pixel is 0).  Which pixels are read depends on the plan's
    `feather` (a missing field means 0):
      * 0 — hard seams, no blending (`spei_tiles_u8_out` / `spei_tiles_u16_out`): every tile is read in its band only, a tile's
        margin outside its band never;
      * > 0 — feathered seams (`spei_tiles_u8_blend` / `spei_tiles_u16_blend`): inside the ramp of `tiles.seam_ramps(plan)` pixels
        on either side of an inner seam the two tiles of the seam are read and blended (four where a row and a column ramp cross),
        so a tile is read in its band and in the ramps next to it; the rest of its margin and its reflect pad never.  A pixel
        outside every ramp is the hard stitch's, bit for bit.
    One launch on the current stream (csrc/tile_io.hip), no host sync."""
    n = plan.rows * plan.cols
    tiles = list(tiles)
    if len(tiles) != n:
        raise ValueError(f"the tile plan has {n} tiles, got {len(tiles)}")
    thp, twp = padded_size(plan.th), padded_size(plan.tw)
    dev = tiles[0].device
    for t in tiles:
        assert t.is_cuda and t.device == dev and t.dtype == torch.float32 and tuple(t.shape) == (3, thp, twp) and t.is_contiguous()
    if out_depth not in y4m.DEPTHS:
        raise ValueError(f"out_depth must be 8, 10 or 12, got {out_depth!r}")
    dtype = torch.uint8 if out_depth == 8 else torch.uint16
    h, w = plan.H, plan.W
    if out is None:
        out = torch.empty(h, w, 3, dtype=dtype, device=dev)
    assert out.device == dev and out.dtype == dtype and tuple(out.shape) == (h, w, 3) and out.is_contiguous()
    assert nonfinite is None or (nonfinite.device == dev and nonfinite.dtype == torch.int32 and nonfinite.numel() >= 1)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in tiles])
    tabs = (_int_table(plan.y0, plan.rows, "y0"), _int_table(plan.x0, plan.cols, "x0"),
            _int_table(plan.yb, plan.rows + 1, "yb"), _int_table(plan.xb, plan.cols + 1, "xb"))
    flag = _vp(nonfinite.data_ptr() if nonfinite is not None else 0)
    feather = getattr(plan, "feather", 0)
    if isinstance(feather, bool) or not isinstance(feather, int) or feather < 0:
        raise ValueError(f"the tile plan's feather must be a whole number >= 0, got {feather!r}")
    lib = _lib.lib()
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if feather > 0:
            size = (plan.rows, plan.cols, thp, twp, int(plan.th), int(plan.tw), feather)
            if out_depth == 8:
                _lib.check(lib.spei_tiles_u8_blend(ptrs, _vp(out.data_ptr()), flag, h, w, *tabs, *size, st), "spei_tiles_u8_blend")
            else:
                _lib.check(lib.spei_tiles_u16_blend(ptrs, _vp(out.data_ptr()), flag, h, w, *tabs, *size, out_depth, st),
                           "spei_tiles_u16_blend")
        elif out_depth == 8:
            _lib.check(lib.spei_tiles_u8_out(ptrs, _vp(out.data_ptr()), flag, h, w, *tabs, plan.rows, plan.cols, thp, twp, st),
                       "spei_tiles_u8_out")
        else:
            _lib.check(lib.spei_tiles_u16_out(ptrs, _vp(out.data_ptr()), flag, h, w, *tabs, plan.rows, plan.cols, thp, twp, out_depth, st),
                       "spei_tiles_u16_out")
    return out


def fields_in(frame: torch.Tensor, out: torch.Tensor, depth: Optional[int] = None) -> torch.Tensor:
    """One packed woven frame [H,W,3] on the device (H even), uint8 (`depth` None) or uint16 of `depth` 10 or 12 bits -> both fields
    as fp32 planes in `out` [2, 3, hp, wp], hp / wp = H / 2 and W rounded up to multiples of 20: field p is bit-identical to
    `frames_u8_in` / `frames_u16_in` on frame[p::2].contiguous(), the field's own reflect pad included.  `out` may be a view with any
    field stride (a multiple of 4 floats) whose fields are contiguous, such as x[:, j] of the window inputs [2, n_seq + 2, 3, hp, wp]
    of both fields.  One launch on the current stream (csrc/field_io.hip), no host sync."""
    deep = frame.dtype == torch.uint16
    assert frame.is_cuda and frame.dtype in (torch.uint8, torch.uint16) and frame.dim() == 3 and frame.shape[2] == 3 and frame.is_contiguous()
    if deep:
        depth = _depth(depth)
    elif depth is not None:
        raise ValueError(f"depth= applies to uint16 frames only; the frame is {frame.dtype}")
    h, w = frame.shape[:2]
    if h % 2:
        raise ValueError(f"a frame of {h} rows does not split into two fields: H must be even")
    hp, wp = padded_size(h // 2), padded_size(w)
    assert out.is_cuda and out.device == frame.device and out.dtype == torch.float32 and tuple(out.shape) == (2, 3, hp, wp)
    assert out.stride()[1:] == (hp * wp, wp, 1), "every field of out must be contiguous (any field stride)"
    lib = _lib.lib()
    with torch.cuda.device(frame.device):
        st = C.c_void_p(torch.cuda.current_stream(frame.device).cuda_stream)
        if deep:
            _lib.check(lib.spei_fields_u16_in(_vp(frame.data_ptr()), h, w, _vp(out.data_ptr()), out.stride(0), depth, st), "spei_fields_u16_in")
        else:
            _lib.check(lib.spei_fields_u8_in(_vp(frame.data_ptr()), h, w, _vp(out.data_ptr()), out.stride(0), st), "spei_fields_u8_in")
    return out


def fields_out(fields, h: int, w: int, out_depth: int = 8, out: Optional[torch.Tensor] = None,
               nonfinite: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The two fields of a frame (contiguous fp32 [3,hp,wp] tensors on one device: top, bottom) -> the woven frame, uint8 [h,w,3] for
    `out_depth` 8 and uint16 for 10 and 12 (h even): row 2 r + p is row r of `frame_u8_out` / `frame_u16_out`'s h / 2 x w crop of
    field p.  `out` (optional): the packed destination.  `nonfinite` (optional): an int32 device tensor whose first element becomes
    nonzero iff either field's crop held a NaN or an infinity (that sample is 0).  One launch on the current stream
    (csrc/field_io.hip), no host sync."""
    top, bottom = fields
    dev = top.device
    for t in (top, bottom):
        assert t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.dim() == 3 and t.shape == top.shape and t.shape[0] == 3
        assert t.is_contiguous()
    if out_depth not in y4m.DEPTHS:
        raise ValueError(f"out_depth must be 8, 10 or 12, got {out_depth!r}")
    if h % 2:
        raise ValueError(f"a frame of {h} rows is not the weave of two fields: H must be even")
    dtype = torch.uint8 if out_depth == 8 else torch.uint16
    hp, wp = top.shape[1:]
    if out is None:
        out = torch.empty(h, w, 3, dtype=dtype, device=dev)
    assert out.device == dev and out.dtype == dtype and tuple(out.shape) == (h, w, 3) and out.is_contiguous()
    assert nonfinite is None or (nonfinite.device == dev and nonfinite.dtype == torch.int32 and nonfinite.numel() >= 1)
    flag = _vp(nonfinite.data_ptr() if nonfinite is not None else 0)
    lib = _lib.lib()
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if out_depth == 8:
            _lib.check(lib.spei_fields_u8_out(_vp(top.data_ptr()), _vp(bottom.data_ptr()), _vp(out.data_ptr()), flag, h, w, hp, wp, st),
                       "spei_fields_u8_out")
        else:
            _lib.check(lib.spei_fields_u16_out(_vp(top.data_ptr()), _vp(bottom.data_ptr()), _vp(out.data_ptr()), flag, h, w, hp, wp,
                                               out_depth, st), "spei_fields_u16_out")
    return out


ROI_FEATHER_MAX = 200


def _rect(roi, h: int, w: int) -> tuple:
    """(y0, x0, rh, rw) of a rectangle inside an h x w frame, as ints; ValueError otherwise."""
    vals = tuple(roi) if isinstance(roi, (tuple, list)) else ()
    if len(vals) != 4 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in vals):
        raise ValueError(f"a rectangle is four whole numbers (y0, x0, h, w), got {roi!r}")
    y0, x0, rh, rw = (int(v) for v in vals)
    if rh < 1 or rw < 1 or y0 < 0 or x0 < 0 or y0 + rh > h or x0 + rw > w:
        raise ValueError(f"the rectangle {(y0, x0, rh, rw)} is empty or lies outside the {w}x{h} frame")
    return y0, x0, rh, rw


def roi_in(frame: torch.Tensor, roi, out: torch.Tensor, depth: Optional[int] = None) -> torch.Tensor:
    """One packed frame [H,W,3] on the device, uint8 (`depth` None) or uint16 of `depth` 10 or 12 bits -> the rectangle `roi` =
    (y0, x0, h, w) of it as fp32 planes in `out` [3, hp, wp] (contiguous; hp, wp = h, w rounded up to multiples of 20): bit-identical
    to `frames_u8_in` / `frames_u16_in` on the crop frame[y0 : y0 + h, x0 : x0 + w], reflect pad included.  It is `tiles_in` with a
    table of one tile at (y0, x0): one launch on the current stream (csrc/tile_io.hip), no host sync."""
    from types import SimpleNamespace
    assert frame.dim() == 3
    y0, x0, rh, rw = _rect(roi, *frame.shape[:2])
    plan = SimpleNamespace(H=int(frame.shape[0]), W=int(frame.shape[1]), rows=1, cols=1, th=rh, tw=rw, y0=(y0,), x0=(x0,))
    assert out.dim() == 3 and out.is_contiguous()
    tiles_in(frame, plan, out.unsqueeze(0), depth)
    return out


def roi_paste(x: torch.Tensor, frame: torch.Tensor, roi, out_depth: int = 8, feather: int = 0, in_depth: Optional[int] = None,
              out: Optional[torch.Tensor] = None, nonfinite: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The model's output for a rectangle, pasted into the input frame: `x` fp32 [3,hp,wp] on the device (contiguous; hp, wp = h, w
    rounded up to multiples of 20), `frame` the packed input frame [H,W,3], uint8 (`in_depth` None) or uint16 of `in_depth` 10 or 12
    bits, `roi` = (y0, x0, h, w) -> the output frame, uint8 [H,W,3] for `out_depth` 8 and uint16 for 10 and 12.  Inside the rectangle
    it holds `frame_u8_out` / `frame_u16_out`'s value of x[:, y - y0, x - x0], outside it the input sample at the output depth,
    (min(v, D_in) * 2 * D_out + D_in) // (2 * D_in) with D = 2^depth - 1 (the identity at equal depths).  `feather` N in
    0..min(200, h // 2, w // 2): N > 0 blends the two over the N pixels inside every side of the rectangle that is not a side of the
    frame (include/speinet_hip.h has the weights); every pixel off the ramps keeps the hard paste's bits.  `out` (optional): the packed
    destination; it may not overlap `frame` or `x`.  `nonfinite` (optional): an int32 device tensor whose first element becomes nonzero
    iff a value of x inside the h x w crop was a NaN or an infinity (that sample is 0); the pad of x is never read.  One launch on the
    current stream writes the whole frame (csrc/roi_io.hip), no host sync."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[0] == 3 and x.is_contiguous()
    deep = frame.dtype == torch.uint16
    assert frame.device == x.device and frame.dtype in (torch.uint8, torch.uint16) and frame.dim() == 3 and frame.shape[2] == 3
    assert frame.is_contiguous()
    if deep:
        in_depth = _depth(in_depth)
    elif in_depth not in (None, 8):
        raise ValueError(f"in_depth= applies to uint16 frames only; the frame is {frame.dtype}")
    else:
        in_depth = 8
    if isinstance(out_depth, bool) or out_depth not in y4m.DEPTHS:
        raise ValueError(f"out_depth must be 8, 10 or 12, got {out_depth!r}")
    h, w = (int(v) for v in frame.shape[:2])
    y0, x0, rh, rw = _rect(roi, h, w)
    hp, wp = padded_size(rh), padded_size(rw)
    if tuple(x.shape[1:]) != (hp, wp):
        raise ValueError(f"the planes are {tuple(x.shape[1:])}, a {rh}x{rw} rectangle rounds up to {(hp, wp)}")
    fmax = min(ROI_FEATHER_MAX, rh // 2, rw // 2)
    if isinstance(feather, bool) or not isinstance(feather, (int, np.integer)) or not 0 <= feather <= fmax:
        raise ValueError(f"feather must be a whole number in 0..{fmax} (at most {ROI_FEATHER_MAX} and half of the {rh}x{rw} rectangle), "
                         f"got {feather!r}")
    dtype = torch.uint8 if out_depth == 8 else torch.uint16
    if out is None:
        out = torch.empty(h, w, 3, dtype=dtype, device=x.device)
    assert out.device == x.device and out.dtype == dtype and tuple(out.shape) == (h, w, 3) and out.is_contiguous()
    assert nonfinite is None or (nonfinite.device == x.device and nonfinite.dtype == torch.int32 and nonfinite.numel() >= 1)
    flag = _vp(nonfinite.data_ptr() if nonfinite is not None else 0)
    lib = _lib.lib()
    with torch.cuda.device(x.device):
        st = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        head = (_vp(x.data_ptr()), _vp(frame.data_ptr()), in_depth, _vp(out.data_ptr()), flag, h, w, y0, x0, rh, rw, hp, wp, int(feather))
        if out_depth == 8:
            _lib.check(lib.spei_roi_paste_u8(*head, st), "spei_roi_paste_u8")
        else:
            _lib.check(lib.spei_roi_paste_u16(*head, out_depth, st), "spei_roi_paste_u16")
    return out


def frame_requant(frame: torch.Tensor, out_depth: int, in_depth: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A packed frame at another depth: `frame` [H,W,3] on the device (contiguous), uint8 (`in_depth` None) or uint16 of `in_depth` 10
    or 12 bits -> the frame at `out_depth`, uint8 [H,W,3] for 8 and uint16 for 10 and 12, every sample
    (min(v, D_in) * 2 * D_out + D_in) // (2 * D_in) with D = 2^depth - 1: what `roi_paste` writes outside its rectangle, a copy at
    equal depths (a word above D_in reads as D_in).  `out` (optional): the packed destination; it may not overlap `frame`.  One launch
    on the current stream (csrc/frame_io.hip), no host sync."""
    assert frame.is_cuda and frame.dtype in (torch.uint8, torch.uint16) and frame.dim() == 3 and frame.shape[2] == 3
    assert frame.is_contiguous()
    if frame.dtype == torch.uint16:
        in_depth = _depth(in_depth)
    elif in_depth not in (None, 8):
        raise ValueError(f"in_depth= applies to uint16 frames only; the frame is {frame.dtype}")
    else:
        in_depth = 8
    if isinstance(out_depth, bool) or out_depth not in y4m.DEPTHS:
        raise ValueError(f"out_depth must be 8, 10 or 12, got {out_depth!r}")
    h, w = (int(v) for v in frame.shape[:2])
    dtype = torch.uint8 if out_depth == 8 else torch.uint16
    if out is None:
        out = torch.empty(h, w, 3, dtype=dtype, device=frame.device)
    assert out.device == frame.device and out.dtype == dtype and tuple(out.shape) == (h, w, 3) and out.is_contiguous()
    with torch.cuda.device(frame.device):
        st = C.c_void_p(torch.cuda.current_stream(frame.device).cuda_stream)
        _lib.check(_lib.lib().spei_frame_requant(_vp(frame.data_ptr()), in_depth, _vp(out.data_ptr()), int(out_depth), h, w, st),
                   "spei_frame_requant")
    return out


def frame_matte(frame: torch.Tensor, deb: torch.Tensor, matte: torch.Tensor, out_depth: int, in_depth: Optional[int] = None,
                invert: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The deblurred frame where a matte says, the input elsewhere: `frame` the packed input frame [H,W,3] on the device (contiguous),
    uint8 (`in_depth` None) or uint16 of `in_depth` 10 or 12 bits; `deb` the deblurred frame [H,W,3] at `out_depth`, uint8 for 8 and
    uint16 for 10 and 12 (a word above D_out reads as D_out); `matte` uint8 [H,W], contiguous -> the frame at `out_depth` with every
    sample (a * (255 - m) + b * m + 127) // 255, a = `frame_requant`'s sample of `frame`, b = the sample of `deb`, m = the pixel's
    matte byte, or 255 - m under `invert`: exact integers; m = 0 gives a, m = 255 gives b.  `out` (optional): the packed destination;
    it may be `deb` itself (in place) and may not overlap anything otherwise.  One launch on the current stream (csrc/matte_io.hip),
    no host sync."""
    assert frame.is_cuda and frame.dtype in (torch.uint8, torch.uint16) and frame.dim() == 3 and frame.shape[2] == 3
    assert frame.is_contiguous()
    if frame.dtype == torch.uint16:
        in_depth = _depth(in_depth)
    elif in_depth not in (None, 8):
        raise ValueError(f"in_depth= applies to uint16 frames only; the frame is {frame.dtype}")
    else:
        in_depth = 8
    if isinstance(out_depth, bool) or out_depth not in y4m.DEPTHS:
        raise ValueError(f"out_depth must be 8, 10 or 12, got {out_depth!r}")
    h, w = (int(v) for v in frame.shape[:2])
    dtype = torch.uint8 if out_depth == 8 else torch.uint16
    if not (deb.device == frame.device and deb.dtype == dtype and tuple(deb.shape) == (h, w, 3) and deb.is_contiguous()):
        raise ValueError(f"deb must be a contiguous {str(dtype).split('.')[-1]} [{h},{w},3] tensor on {frame.device} (out_depth {out_depth}), "
                         f"got {deb.dtype} {tuple(deb.shape)}")
    if not (matte.device == frame.device and matte.dtype == torch.uint8 and tuple(matte.shape) == (h, w) and matte.is_contiguous()):
        raise ValueError(f"matte must be a contiguous uint8 [{h},{w}] tensor on {frame.device}, got {matte.dtype} {tuple(matte.shape)}")
    if out is None:
        out = torch.empty(h, w, 3, dtype=dtype, device=frame.device)
    assert out.device == frame.device and out.dtype == dtype and tuple(out.shape) == (h, w, 3) and out.is_contiguous()
    lib = _lib.lib()
    with torch.cuda.device(frame.device):
        st = C.c_void_p(torch.cuda.current_stream(frame.device).cuda_stream)
        head = (_vp(frame.data_ptr()), in_depth, _vp(deb.data_ptr()), _vp(matte.data_ptr()), int(bool(invert)), _vp(out.data_ptr()), h, w)
        if out_depth == 8:
            _lib.check(lib.spei_frame_matte_u8(*head, st), "spei_frame_matte_u8")
        else:
            _lib.check(lib.spei_frame_matte_u16(*head, int(out_depth), st), "spei_frame_matte_u16")
    return out


BLUR_CELL = 16                  # the cell of the blur map: 16x16 pixels (csrc/blur_map.hip)
BLUR_MAPS_MAX = 8               # verdict maps one `blur_matte` launch joins
BLUR_GROW_MAX = 4


def blur_cell_shape(h: int, w: int) -> tuple:
    """(ch, cw) = (ceil(h / 16), ceil(w / 16)): the cell grid of an h x w frame."""
    return (int(h) + BLUR_CELL - 1) // BLUR_CELL, (int(w) + BLUR_CELL - 1) // BLUR_CELL


def blur_cells(frames: torch.Tensor, depth: Optional[int] = None, thr: int = 192, flat: int = 2, sums: bool = False):
    """The blur verdict of every 16x16 cell of packed frames [N,H,W,3] on the device (any frame stride), uint8 (`depth` None) or uint16
    of `depth` 10 or 12 bits (a word above D = 2^depth - 1 reads as D) -> cells uint8 [N,ch,cw], 255 = blurred, with ch = ceil(H / 16),
    cw = ceil(W / 16) (edge cells are partial: n < 256 pixels); with `sums` -> (cells, int64 [N,ch,cw,4]), the cell's four sums
    (sum D_h, sum V_h, sum D_v, sum V_v).  Integers throughout, on the luma Y = (77 R + 150 G + 29 B + 128) >> 8 at the frame's
    depth, taken at the clamped index outside the frame.  Per pixel, horizontally: d = 9 (Y(y,x) - Y(y,x-1)),
    b = Y(y,x+4) - Y(y,x-5) (the adjacent difference of the 9-tap box sums centred on x and x - 1), D_h = d d,
    V_h = max(0, d d - b b): how much of the adjacent-pixel variation a 9-tap box removes.  Vertically the same with y and x exchanged.
    A direction is textured iff sum D >= 81 flat^2 n << 2 (depth - 8) (its RMS adjacent difference is at least `flat` 8-bit levels)
    and blurred iff textured and 256 sum V < thr sum D; a cell is lit iff either direction is blurred.  `thr` 0..257 (0 lights
    nothing, 257 every textured direction with sum D > 0), `flat` 0..255.  One launch on the current stream (csrc/blur_map.hip), no
    host sync."""
    assert frames.is_cuda and frames.dtype in (torch.uint8, torch.uint16) and frames.dim() == 4
    deep = frames.dtype == torch.uint16
    if deep:
        depth = _depth(depth)
    elif depth not in (None, 8):
        raise ValueError(f"depth= applies to uint16 frames only; the frames are {frames.dtype}")
    n, h, w, c = frames.shape
    assert c == 3 and frames.stride()[1:] == (w * 3, 3, 1), "frames must be packed [H,W,3] (any frame stride)"
    dev = frames.device
    ch, cw = blur_cell_shape(h, w)
    cells = torch.empty(n, ch, cw, dtype=torch.uint8, device=dev)
    s = torch.empty(n, ch, cw, 4, dtype=torch.int64, device=dev) if sums else None
    lib = _lib.lib()
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        head = (_vp(frames.data_ptr()), frames.element_size() * frames.stride(0), n, h, w)
        tail = (int(thr), int(flat), _vp(cells.data_ptr()), _vp(s.data_ptr() if sums else 0), st)
        if deep:
            _lib.check(lib.spei_blur_cells_u16(*head, depth, *tail), "spei_blur_cells_u16")
        else:
            _lib.check(lib.spei_blur_cells_u8(*head, *tail), "spei_blur_cells_u8")
    return (cells, s) if sums else cells


def blur_matte(cells: torch.Tensor, H: int, W: int, grow: int = 1, out: Optional[torch.Tensor] = None,
               cell_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The pixel matte of verdict maps: `cells` uint8 [n,ch,cw] on the device (contiguous; n = 1..8, (ch, cw) the cell grid of an
    H x W frame) -> uint8 [H,W].  The maps are joined by their maximum, cell by cell (the hold), dilated by `grow` cells (0..4: the
    maximum over a (2 grow + 1)^2 neighbourhood, zeros outside), and interpolated bilinearly between cell centres in exact integers:
    u = 2 y + 17, i0 = u // 32 - 1, i1 = i0 + 1 (both clamped into 0..ch-1), wy = u % 32, the same for x with j0, j1, wx, and
    m = ((32-wy)(32-wx) c[i0][j0] + (32-wy) wx c[i0][j1] + wy (32-wx) c[i1][j0] + wy wx c[i1][j1] + 512) // 1024: all-255 gives 255,
    all-0 gives 0, the ramp between a lit and an unlit cell is 16 pixels wide.  `out` (optional): the matte's destination, contiguous;
    `cell_out` (optional): uint8 [ch,cw], receives the held and dilated cell map.  One launch on the current stream
    (csrc/blur_map.hip), no host sync."""
    assert cells.is_cuda and cells.dtype == torch.uint8 and cells.dim() == 3 and cells.is_contiguous()
    H, W = int(H), int(W)
    n, (ch, cw) = cells.shape[0], blur_cell_shape(H, W)
    if tuple(cells.shape[1:]) != (ch, cw):
        raise ValueError(f"cells has shape {tuple(cells.shape)}; a {W}x{H} frame has {ch}x{cw} cells")
    dev = cells.device
    if out is None:
        out = torch.empty(H, W, dtype=torch.uint8, device=dev)
    assert out.device == dev and out.dtype == torch.uint8 and tuple(out.shape) == (H, W) and out.is_contiguous()
    assert cell_out is None or (cell_out.device == dev and cell_out.dtype == torch.uint8 and tuple(cell_out.shape) == (ch, cw)
                                and cell_out.is_contiguous())
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.lib().spei_blur_matte(_vp(cells.data_ptr()), n, int(grow), H, W, _vp(out.data_ptr()),
                                              _vp(cell_out.data_ptr() if cell_out is not None else 0), st), "spei_blur_matte")
    return out


def frame_extent(frames: torch.Tensor, depth: Optional[int] = None, out=None):
    """The extent of the picture in packed frames [N,H,W,3] on the device (any frame stride), uint8 (`depth` None) or uint16 of `depth`
    10 or 12 bits -> (rowmax int32 [H], colmax int32 [W]): the maximum over every row, and over every column, of all N frames of the
    integer luma of `frame_pair_stats` / `frame_pair_stats_u16`, Y = (77 R + 150 G + 29 B + 128) >> 8.  `out` (optional): the
    (rowmax, colmax) of an earlier call, which the maxima then JOIN (a clip is scanned batch by batch); None: fresh tables, cleared on
    the stream.  Exact integers.  One launch on the current stream (csrc/roi_io.hip), no host sync."""
    assert frames.is_cuda and frames.dtype in (torch.uint8, torch.uint16) and frames.dim() == 4
    deep = frames.dtype == torch.uint16
    if deep:
        depth = _depth(depth)
    elif depth not in (None, 8):
        raise ValueError(f"depth= applies to uint16 frames only; the frames are {frames.dtype}")
    n, h, w, c = frames.shape
    assert c == 3 and frames.stride()[1:] == (w * 3, 3, 1), "frames must be packed [H,W,3] (any frame stride)"
    dev = frames.device
    if out is None:
        rowmax, colmax = torch.empty(h, dtype=torch.int32, device=dev), torch.empty(w, dtype=torch.int32, device=dev)
    else:
        rowmax, colmax = out
        for t, size in ((rowmax, h), (colmax, w)):
            assert t.device == dev and t.dtype == torch.int32 and tuple(t.shape) == (size,) and t.is_contiguous()
    lib = _lib.lib()
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        tail = (_vp(rowmax.data_ptr()), _vp(colmax.data_ptr()), 0 if out is None else 1, st)
        if deep:
            _lib.check(lib.spei_frame_extent_u16(_vp(frames.data_ptr()), 2 * frames.stride(0), n, h, w, depth, *tail), "spei_frame_extent_u16")
        else:
            _lib.check(lib.spei_frame_extent(_vp(frames.data_ptr()), frames.stride(0), n, h, w, *tail), "spei_frame_extent")
    return rowmax, colmax


def planes_d4(x: torch.Tensor, op: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Member `op` (0..7, speinet_amd/ensemble.py) of every plane of `x`: fp32 [..., H, W] on the device -> `ensemble.apply(x, op)` as a
    contiguous tensor, [..., W, H] for op & 4, copied as bits.  `x` may be a view whose planes are contiguous and evenly spaced (any
    leading shape that collapses to one plane stride, such as a contiguous tensor or a slice of its first axis); `out` (optional): a
    destination of the result's shape with such planes that does not overlap `x`.  One launch on the current stream
    (csrc/ensemble_io.hip), no host sync."""
    from . import ensemble
    op = ensemble.check_op(op)
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() >= 2
    h, w = x.shape[-2:]
    shape = tuple(x.shape[:-2]) + ensemble.shape_of(h, w, op)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    assert out.device == x.device and out.dtype == torch.float32 and tuple(out.shape) == shape
    n = x.numel() // (h * w)
    strides = []
    for t, (r, c) in ((x, (h, w)), (out, shape[-2:])):
        flat = t.reshape(n, r, c)
        if flat.data_ptr() != t.data_ptr() or flat.stride()[1:] != (c, 1):
            raise ValueError(f"planes_d4 needs contiguous planes at one stride; got shape {tuple(t.shape)} with strides {t.stride()}")
        strides.append(flat.stride(0) if n > 1 else h * w)
    lib = _lib.lib()
    with torch.cuda.device(x.device):
        st = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(lib.spei_planes_d4(_vp(x.data_ptr()), strides[0], _vp(out.data_ptr()), strides[1], n, h, w, op, st), "spei_planes_d4")
    return out


def d4_mean(members, member_ops, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The ensemble mean of K = 1, 2, 4 or 8 members: contiguous fp32 [C, H, W] tensors on one device, [C, W, H] where the member's op
    (0..7, `member_ops[k]`) transposes; member k is T_op of its term.  Returns `out` [C, H, W] (allocated if None; it must not overlap a
    member): the float32 sum of `ensemble.invert(members[k], member_ops[k])` in the order given, starting from the first, times
    1 / K; K = 1 is the inverse transform, copied as bits.  One launch on the current stream (csrc/ensemble_io.hip), no host sync."""
    from . import ensemble
    members, member_ops = list(members), [ensemble.check_op(g) for g in member_ops]
    k = len(members)
    if k not in ensemble.SIZES or len(member_ops) != k:
        raise ValueError(f"d4_mean takes 1, 2, 4 or 8 members and one op per member, got {k} members and {len(member_ops)} ops")
    dev = members[0].device
    for t in members:
        assert t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.dim() == 3 and t.is_contiguous()
    c = members[0].shape[0]
    h, w = ensemble.shape_of(*members[0].shape[1:], member_ops[0])          # a transposition is its own inverse on shapes
    for t, g in zip(members, member_ops):
        if tuple(t.shape) != (c,) + ensemble.shape_of(h, w, g):
            raise ValueError(f"member with op {g} has shape {tuple(t.shape)}, not {(c,) + ensemble.shape_of(h, w, g)}")
    if out is None:
        out = torch.empty(c, h, w, dtype=torch.float32, device=dev)
    assert out.device == dev and out.dtype == torch.float32 and tuple(out.shape) == (c, h, w) and out.is_contiguous()
    ptrs = (C.c_void_p * k)(*[t.data_ptr() for t in members])
    lib = _lib.lib()
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.spei_d4_mean(ptrs, (C.c_int * k)(*member_ops), k, _vp(out.data_ptr()), c, h, w, st), "spei_d4_mean")
    return out


def yuv_frame_bytes(h: int, w: int, layout: int) -> int:
    """Bytes of one planar YUV frame: Y [h][w], then U and V, [ceil(h/2)][ceil(w/2)] each for 4:2:0, [h][ceil(w/2)] each for 4:2:2,
    [h][w] each for 4:4:4; the Y plane alone for mono."""
    return y4m.frame_bytes(h, w, layout)


def _yuv_entry(layout: int, name: str, planar: str, fields: bool = False) -> str:
    """The C-ABI entry of a conversion for a layout: `name` (spei_yuv_* / spei_*_to_yuv) takes 4:2:0 and 4:4:4, `planar` 4:2:2 and
    mono (csrc/yuv_io.hip: one kernel template behind both).  `fields`: the entry for a woven interlaced frame, which takes every
    layout (spei_yuv_fields_to_rgb_* / spei_rgb_*_to_yuv_fields: `name` with `yuv` read as `yuv_fields`)."""
    if fields:
        return name.replace("yuv", "yuv_fields")
    return planar if layout in (y4m.P422, y4m.MONO) else name


def yuv_to_rgb_u8(planar: torch.Tensor, h: int, w: int, layout: int, matrix: int, range: int,
                  out: Optional[torch.Tensor] = None, fields: bool = False) -> torch.Tensor:
    """Planar uint8 YUV frames on the device, [N, frame_bytes] (rows any stride apart) or one [frame_bytes], as in a y4m FRAME payload
    -> packed RGB uint8 [N,h,w,3] (csrc/yuv_io.hip: integer arithmetic, defined bit for bit in include/speinet_hip.h).  `layout`,
    `matrix`, `range`: the constants of speinet_amd.y4m (SPEI_YUV_*; P422 and MONO go to spei_planar_to_rgb_u8).  `out` (optional): a contiguous uint8 [N,h,w,3] destination.
    `fields`: the frames are interlaced, two woven fields each (spei_yuv_fields_to_rgb_u8): field p of the result, its rows p::2, is
    this conversion of field p's own planar picture (Y rows p::2 and, for 4:2:0, chroma-plane rows p::2; h % 4 == 0 there); the other
    layouts convert row by row and give the progressive result.  One launch on the current stream, no host sync."""
    assert planar.is_cuda and planar.dtype == torch.uint8 and planar.dim() in (1, 2)
    fr = planar if planar.dim() == 2 else planar.unsqueeze(0)
    n, nb = fr.shape
    assert nb == yuv_frame_bytes(h, w, layout) and fr.stride(1) == 1, "frames must be packed planar frames (any frame stride)"
    dev = planar.device
    if out is None:
        out = torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev)
    assert out.device == dev and out.dtype == torch.uint8 and tuple(out.shape) == (n, h, w, 3) and out.is_contiguous()
    lib = _lib.lib()
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        entry = _yuv_entry(layout, "spei_yuv_to_rgb_u8", "spei_planar_to_rgb_u8", fields)
        _lib.check(getattr(lib, entry)(_vp(fr.data_ptr()), fr.stride(0), _vp(out.data_ptr()), n, h, w, layout, matrix, range, st), entry)
    return out


def rgb_u8_to_yuv(rgb: torch.Tensor, layout: int, matrix: int, range: int, out: Optional[torch.Tensor] = None,
                  fields: bool = False) -> torch.Tensor:
    """One packed RGB uint8 frame [h,w,3] on the device -> its planar YUV frame, uint8 [frame_bytes], a y4m FRAME payload
    (csrc/yuv_io.hip; the inverse definition of `yuv_to_rgb_u8`).  `out` (optional): a contiguous uint8 [frame_bytes] destination.
    `fields`: the frame is two woven fields (spei_rgb_u8_to_yuv_fields): field p of the planar frame is this conversion of the RGB
    rows p::2, as in `yuv_to_rgb_u8`.  One launch on the current stream, no host sync."""
    assert rgb.is_cuda and rgb.dtype == torch.uint8 and rgb.dim() == 3 and rgb.shape[2] == 3 and rgb.is_contiguous()
    h, w = rgb.shape[:2]
    nb = yuv_frame_bytes(h, w, layout)
    dev = rgb.device
    if out is None:
        out = torch.empty(nb, dtype=torch.uint8, device=dev)
    assert out.device == dev and out.dtype == torch.uint8 and tuple(out.shape) == (nb,) and out.is_contiguous()
    lib = _lib.lib()
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        entry = _yuv_entry(layout, "spei_rgb_u8_to_yuv", "spei_rgb_u8_to_planar", fields)
        _lib.check(getattr(lib, entry)(_vp(rgb.data_ptr()), _vp(out.data_ptr()), h, w, layout, matrix, range, st), entry)
    return out


def yuv_to_rgb_u16(planar: torch.Tensor, h: int, w: int, layout: int, matrix: int, range: int, depth: int,
                   out: Optional[torch.Tensor] = None, fields: bool = False) -> torch.Tensor:
    """`yuv_to_rgb_u8` for deep frames: planar uint16 YUV frames of `depth` 10 or 12 bits on the device, [N, frame samples] (rows any
    stride apart) or one [frame samples] (`yuv_frame_bytes(h, w, layout)` samples: a deep y4m FRAME payload viewed as uint16) ->
    packed RGB uint16 [N,h,w,3] (csrc/yuv_io.hip; the deep rule of include/speinet_hip.h).  `out` (optional): a contiguous uint16
    [N,h,w,3] destination.  `fields`: as in `yuv_to_rgb_u8` (spei_yuv_fields_to_rgb_u16).  One launch on the current stream, no host
    sync."""
    assert planar.is_cuda and planar.dtype == torch.uint16 and planar.dim() in (1, 2)
    depth = _depth(depth)
    fr = planar if planar.dim() == 2 else planar.unsqueeze(0)
    n, ns = fr.shape
    assert ns == yuv_frame_bytes(h, w, layout) and fr.stride(1) == 1, "frames must be packed planar frames (any frame stride)"
    dev = planar.device
    if out is None:
        out = torch.empty(n, h, w, 3, dtype=torch.uint16, device=dev)
    assert out.device == dev and out.dtype == torch.uint16 and tuple(out.shape) == (n, h, w, 3) and out.is_contiguous()
    lib = _lib.lib()
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        entry = _yuv_entry(layout, "spei_yuv_to_rgb_u16", "spei_planar_to_rgb_u16", fields)
        _lib.check(getattr(lib, entry)(_vp(fr.data_ptr()), 2 * fr.stride(0), _vp(out.data_ptr()), n, h, w, layout, matrix, range, depth, st),
                   entry)
    return out


def rgb_u16_to_yuv(rgb: torch.Tensor, layout: int, matrix: int, range: int, depth: int, out: Optional[torch.Tensor] = None,
                   fields: bool = False) -> torch.Tensor:
    """`rgb_u8_to_yuv` for deep frames: one packed RGB uint16 frame [h,w,3] of `depth` 10 or 12 bits on the device -> its planar YUV
    frame, uint16 [frame samples], whose bytes are a deep y4m FRAME payload.  `out` (optional): a contiguous uint16 destination.
    `fields`: as in `rgb_u8_to_yuv` (spei_rgb_u16_to_yuv_fields).  One launch on the current stream, no host sync."""
    assert rgb.is_cuda and rgb.dtype == torch.uint16 and rgb.dim() == 3 and rgb.shape[2] == 3 and rgb.is_contiguous()
    depth = _depth(depth)
    h, w = rgb.shape[:2]
    ns = yuv_frame_bytes(h, w, layout)
    dev = rgb.device
    if out is None:
        out = torch.empty(ns, dtype=torch.uint16, device=dev)
    assert out.device == dev and out.dtype == torch.uint16 and tuple(out.shape) == (ns,) and out.is_contiguous()
    lib = _lib.lib()
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        entry = _yuv_entry(layout, "spei_rgb_u16_to_yuv", "spei_rgb_u16_to_planar", fields)
        _lib.check(getattr(lib, entry)(_vp(rgb.data_ptr()), _vp(out.data_ptr()), h, w, layout, matrix, range, depth, st), entry)
    return out


def psnr_f32(a: torch.Tensor, b: torch.Tensor, shave: int = 4, rgb_range: float = 1.0) -> torch.Tensor:
    """The reference's validation metric on float frames (csrc/metrics.hip spei_psnr_f32; util/utils.py:81-92 calc_psnr): a, b fp32
    [3,H,W] on the device -> float64 [2] = (sum of squared differences over [shave:-shave] in float64, number of terms).  Two launches on
    the current stream, no host sync; `psnr_of` turns the pair into dB on the host."""
    assert a.is_cuda and a.dtype == torch.float32 and a.dim() == 3 and a.shape[0] == 3 and a.is_contiguous()
    assert b.shape == a.shape and b.dtype == torch.float32 and b.device == a.device and b.is_contiguous()
    lib = _lib.lib()
    dev = a.device
    ws = torch.empty(PSNR_WS_DOUBLES, dtype=torch.float64, device=dev)
    res = torch.empty(2, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.spei_psnr_f32(_vp(a.data_ptr()), _vp(b.data_ptr()), a.shape[1], a.shape[2], shave, float(rgb_range), _vp(ws.data_ptr()),
                                     _vp(res.data_ptr()), st), "spei_psnr_f32")
    return res


PSNR_WS_DOUBLES = 256          # SPEI_PSNR_WS_DOUBLES


def psnr_of(sq_sum: float, count: float) -> float:
    """calc_psnr's last lines (util/utils.py:88-92): 100 for identical frames, else 20 log10(1 / sqrt(mse))."""
    import math
    mse = sq_sum / count
    return 100.0 if mse == 0 else 20 * math.log10(1.0 / math.sqrt(mse))


CORR_DIAG_WS_MAX = 8 << 30     # bytes of candidate pairs the diagonal correlation kernel may use before the slab kernel takes over


class CorrPlan:
    """A prepared K11 launch (see Ctx.corr_plan): `launch()` runs the arg-max kernel — bracketed by the profile events — and
    whatever must follow it on the same stream (the exact re-score of the "top2" form)."""
    __slots__ = ("ctx", "s", "arg", "kernel", "main", "post", "keep")

    def __init__(self, ctx, s, arg, kernel, main, post, keep):
        self.ctx, self.s, self.arg, self.kernel, self.main, self.post, self.keep = ctx, s, arg, kernel, main, post, keep

    def launch(self, profile: Optional[dict] = None) -> None:
        ctx = self.ctx if profile is None else self.ctx.replace(profile=profile)
        st = ctx._stream()
        if ctx.profile is not None:
            ctx.profile["corr_kernel"] = self.kernel
        fam = ctx.profile is not None and "families" in ctx.profile
        if fam:
            f0, f1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            f0.record(torch.cuda.current_stream(ctx.device))
        with _timed(ctx, "corr_argmax"):
            for fn, name, args in self.main:
                _lib.check(fn(*args, st), name)
        for fn, name, args in self.post:
            _lib.check(fn(*args, st), name)
        if fam:
            f1.record(torch.cuda.current_stream(ctx.device))
            ctx.profile["families"].setdefault("correlation", []).append((f0, f1))


@dataclasses.dataclass(frozen=True, slots=True, eq=False)
class Ctx:
    """Everything one forward call needs to know besides its tensors.  Immutable; `replace` derives a variant.  The knobs default to the
    shipping configuration; parity ablations switch them off one at a time (tools/ablate_parity.py).  "16-bit" below = the
    single-product modes "bf16" / "f16"."""
    ACT_NONE, ACT_RELU, ACT_GELU = ACT_NONE, ACT_RELU, ACT_GELU
    CONV, CONV_T = CONV, CONV_T
    # stages of an f16 frame that run in split (bf16x3) arithmetic by default, see `split_decode`
    SPLIT_STAGES = ("glue", "dec2")

    # see PRECISIONS / CORR_PRECISIONS above
    precision: str = "f32"
    corr_precision: str = "bf16x3"
    # the ROCm device every tensor of the call lives on; kernels are launched on torch's current stream OF THAT DEVICE, and every
    # pointer handed to the C-ABI is checked against it.  None: the current device
    device: Optional[torch.device] = None
    # 16-bit: tensors that ONLY feed the next GEMM / the attention kernel live in HBM as 16-bit
    bf16_storage: bool = True
    # 16-bit: the ResBlock's conv2 output (read by the gate statistics and the apply pass) is 16-bit
    x1_bf16: bool = True
    # 16-bit: LayerNorm -> fc1 -> GELU -> fc2 -> +x in one kernel (mlp_fused16.hip)
    fuse_mlp: bool = True
    # 16-bit: LayerNorm -> q/kv GEMMs -> window attention -> proj -> +x in one kernel (attn_fused16.hip)
    fuse_attn: bool = True
    # 16-bit: relu(conv1x1(bicubic_up(x))) evaluated as relu(bicubic_up(conv1x1(x)))
    commute_upconv: bool = True
    # the same in every arithmetic mode: set by stage overrides that run single layers of a 16-bit frame in split arithmetic (the
    # f32-grade MODES keep the reference's order of operations)
    commute_any: bool = False
    # "f16" with corr "top2": the candidate pass of the correlation runs on bf16 operands (True) instead of f16.  The fp32 re-score
    # decides the winner and S either way (G14: 16 more of 57600 positions differ, dPSNR +1e-6 dB); bf16 operands let the chip hold a
    # ~7 % higher MFMA clock on the slab kernel (tools/bench_corr.py); on the diagonal kernel, which is not limited by the matrix pipe,
    # the difference is 1-5 % (2.60-2.73 vs 2.73-2.76 ms)
    corr_bf16: bool = True
    # corr "top2", reference map at least as high as the query map (SearchTransfer's maps of one size, SelfTransfer's rotated landscape
    # map): the candidate pass is the diagonal-sliding kernel (corr_diag16.hip): each row-against-row term of the 3x3-patch score is
    # computed once and shared by the three patch rows that use it — a third of the bmm's flops, same fp32 sums.  Off: the slab kernel
    corr_diag: bool = True
    # "f16": decoder_second (3 ResBlocks at H/4, 128 channels) and the 1x1 / 3x3 glue convolutions of `_decode` (conv_lv*, search*:
    # model/speinet.py:92-119) run in split arithmetic (bf16x3, f32-grade).  They are 2.4 % of the frame's FLOPs and where the
    # half-operand error weighs most on the `_forwardb` branch: |dPSNR| against the reference on that branch 0.9-1.07e-3 dB ->
    # 1.4-4.6e-4 (every golden <= 4.6e-4; profiles/r03_parity_ablation.txt), for 1.35 ms of a 30.3 ms frame.  Off: round 2's arithmetic
    # (tests then hold 1e-3 dB with no margin on that branch)
    split_decode: bool = True
    # 16-bit: the frame's 7 encoder passes (6 without a sharp reference) go through every layer of the three encoder stages in ONE launch
    # per layer (gridDim.y = pass; engine.enc_batched) instead of one launch per pass and layer: bit-identical frames, ~1000 fewer
    # launches per frame, and at H/4 a launch has 3150 workgroups instead of 450 (three resident rounds instead of half of one).
    # Off: round 2's per-pass launches on two streams
    batch_enc: bool = True
    # 16-bit, with fuse_attn: the fused attention branch with four windows per workgroup and a batch of maps per launch
    # (spei_attn_win4_16).  Off: round 2's two-window kernel, one map per launch (spei_attn_fused16)
    attn_win4: bool = True
    # 16-bit: the 32 -> 32 channel 5x5 convolutions (the ResBlock convs at full resolution: inBlock, outBlock) on the weight-stationary
    # persistent kernel (spei_conv32_ws16: the layer's 51 KB of weights live in each wave's registers, nothing streams from L2 in the
    # main loop).  Off: the slab kernel, which runs these layers at its weight intake
    conv32_ws: bool = True
    # 16-bit: the 64 -> 64 channel 5x5 convolutions (the ResBlock convs at half resolution) on the weight-stationary persistent kernel
    # (spei_conv64_ws16: the four waves of a workgroup hold the layer's 205 KB of weights between them).  None: follow conv32_ws, so
    # conv32_ws=False still puts every 5x5 layer on the slab kernel
    conv64_ws: Optional[bool] = None
    # 16-bit: the 256 -> 256 channel 3x3 convolutions of the Swin body (RSTB tail, conv_after_body) on fp32 token maps whose height is a
    # multiple of 6 and width a multiple of 16 as a persistent pipelined kernel (spei_conv3x3_256_pipe16)
    conv3_pipe: bool = True
    # 16-bit: a map whose every reader stages it as the operand of a single-product 16-bit conv is written in that conv's
    # `inter_dtype()` by its producer: the last ResBlock of the batched encoder stacks (routed apply: 16-bit maps for the
    # next stage's head conv, fp32 only for the sharp reference, the level-3 pair sums straight into their destinations), the
    # full-resolution glue maps of `decode`, and the Swin entry's two LayerNorms in one launch.  The consumers round the same values
    # while staging, so frames are bit-identical.  Off: fp32 maps at these hand-offs, the launches of before
    handoff16: bool = True
    # {stage name: {field: value}} overrides applied by `for_stage` (engine: "enc", "swin", "search", "decode", and inside "decode" the
    # stacks "dec2" (decoder_second), "dec1" (decoder_first), "out" (outBlock) and its final conv "tail")
    stage: Optional[dict] = None
    # None, or {op name: [(start_event, end_event), ...]} filled on the launch stream (bench.py)
    profile: Optional[dict] = None
    # None, or a dict that receives intermediate device tensors by name ("arg", "s": what SearchTransfer decided) for the parity
    # tests; eager launches only
    capture: Optional[dict] = None

    def __post_init__(self):
        put = object.__setattr__
        if self.precision not in PRECISIONS:
            raise ValueError(f"unknown precision {self.precision!r}")
        put(self, "corr_precision", _CORR_ALIASES.get(self.corr_precision, self.corr_precision))
        if self.corr_precision not in CORR_PRECISIONS:
            raise ValueError(f"unknown correlation precision {self.corr_precision!r}")
        cur = torch.cuda.current_device() if torch.cuda.is_available() else 0
        device = torch.device("cuda", cur) if self.device is None else torch.device(self.device)
        if device.type != "cuda":
            raise RuntimeError("speinet_amd runs on MI355X only (HIP kernels); there is no CPU path")
        put(self, "device", torch.device("cuda", cur) if device.index is None else device)
        for k in _BOOL_KNOBS:
            if type(getattr(self, k)) is not bool:
                put(self, k, bool(getattr(self, k)))
        if self.conv64_ws is not None:
            put(self, "conv64_ws", bool(self.conv64_ws))
        put(self, "stage", dict(self.stage) if self.stage else {})

    def replace(self, **kw) -> "Ctx":
        return dataclasses.replace(self, **kw)

    def for_stage(self, name: str) -> "Ctx":
        o = self.stage.get(name)
        if o is None and self.split_decode and self.precision == "f16" and name in self.SPLIT_STAGES:
            o = {"precision": "bf16x3", "commute_any": True}
        return self.replace(**o) if o else self

    # ---- plumbing ----------------------------------------------------------------------------------------------
    def _tp(self, t: Optional[torch.Tensor]) -> C.c_void_p:
        if t is None:
            return C.c_void_p(0)
        assert t.is_cuda and t.is_contiguous()
        assert t.device == self.device, f"tensor on {t.device}, call context on {self.device}"
        return C.c_void_p(t.data_ptr())

    def _fp(self, f: Optional[FMap]) -> C.c_void_p:
        if f is None:
            return C.c_void_p(0)
        assert f.t.device == self.device, f"feature map on {f.t.device}, call context on {self.device}"
        return C.c_void_p(f.ptr)

    def _stream(self) -> C.c_void_p:
        # kernels run on the CURRENT HIP device: the caller (SPEINet.forward, detector, tests) holds
        # `torch.cuda.device(ctx.device)`; checked here so a foreign-device launch fails loudly instead of faulting
        assert torch.cuda.current_device() == self.device.index, \
            f"current device cuda:{torch.cuda.current_device()} != call context {self.device}"
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @property
    def lp16(self) -> bool:
        """A single-product 16-bit mode ("bf16" or "f16")."""
        return self.precision in ("bf16", "f16")

    @property
    def fmt(self) -> int:
        """16-bit operand format of the matrix-pipe kernels (SPEI_BF16 / SPEI_F16)."""
        return F16 if self.precision == "f16" else BF16

    def inter_dtype(self) -> torch.dtype:
        """Storage type of GEMM-only intermediates (x-hat, q, kv, attention output, MLP hidden, ResBlock conv1 output)."""
        return LP_DTYPE[self.fmt] if (self.lp16 and self.bf16_storage) else torch.float32

    # ---- K15 / K1 / first and last conv ------------------------------------------------------------------------
    def any_nonzero(self, x: torch.Tensor, flag: torch.Tensor) -> None:
        _lib.check(_lib.lib().spei_any_nonzero(self._tp(x), x.numel(), self._tp(flag), self._stream()), "spei_any_nonzero")

    def train_batch(self, table: torch.Tensor, table_host: torch.Tensor, n_in: int, n_gt: int, input: torch.Tensor, gt: torch.Tensor,
                    patch: int, rgb_range: float = 1.0) -> None:
        """One training batch from a table of crop records (csrc/train_batch.hip; speinet_amd.data.RECORD): `table` the records on the
        device, `table_host` the same bytes in host memory (every rectangle is checked against its frame there, before the launch);
        input fp32 [n_in,3,P,P] and gt fp32 [n_gt,3,P,P] (any leading shape) are written on the current stream."""
        nb = (n_in + n_gt) * 32
        assert table.dtype == torch.uint8 and table.numel() >= nb and not table_host.is_cuda and table_host.dtype == torch.uint8 \
            and table_host.is_contiguous() and table_host.numel() >= nb
        assert input.dtype == torch.float32 and input.numel() == n_in * 3 * patch * patch
        assert gt.dtype == torch.float32 and gt.numel() == n_gt * 3 * patch * patch
        _lib.check(_lib.lib().spei_train_batch_u8(self._tp(table), C.c_void_p(table_host.data_ptr()), n_in, n_gt, self._tp(input), self._tp(gt),
                                                  patch, float(rgb_range), self._stream()), "spei_train_batch_u8")

    def train_batch_runs(self, table: torch.Tensor, table_host: torch.Tensor, n_in: int, n_gt: int, input: torch.Tensor,
                         gt: torch.Tensor, patch: int, rgb_range: float = 1.0, light=None, noise=None, shake=None) -> None:
        """`train_batch` on run records (speinet_amd.data.RUN_RECORD, 48 bytes each): every output frame is the crop of the per-byte
        integer mean of a run of 1..15 consecutive resident frames — spei_window_mean_u8's bytes, never written to memory.  `light`:
        None or "code" is that launch; "srgb" or "gamma:<g>" averages in linear light (speinet_amd.light,
        spei_train_batch_runs_light_u8: `window_mean_u8(light=...)`'s bytes).  `noise`: None, or (records, records_host, seed) — one
        speinet_amd.light.NOISE_RECORD (24 bytes) per record of the table as uint8 tensors on the device and on the host, and the seed
        that keys the generator: sensor noise in that linear light (spei_train_batch_runs_noise_u8: `window_mean_u8(light=, noise=)`'s
        bytes); with "code" a ValueError.  `shake`: None (exactly the launches above), or (records, records_host, (psfs, psfs_host)) — one
        speinet_amd.shake.SHAKE_RECORD (16 bytes) per record of the table as uint8 tensors on the device and on the host, and the PSF
        table as `shake.device_psfs` returns it: camera shake in that linear light (spei_train_batch_runs_shake_u8:
        `window_mean_u8(light=, noise=, shake=)`'s bytes); with "code" a ValueError."""
        nb = (n_in + n_gt) * 48
        assert table.dtype == torch.uint8 and table.numel() >= nb and not table_host.is_cuda and table_host.dtype == torch.uint8 \
            and table_host.is_contiguous() and table_host.numel() >= nb
        assert input.dtype == torch.float32 and input.numel() == n_in * 3 * patch * patch
        assert gt.dtype == torch.float32 and gt.numel() == n_gt * 3 * patch * patch

        def put(what, pair, dtype):                          # the caller's ring tensors, already on their way
            rec, rec_host = pair
            nr = (n_in + n_gt) * dtype.itemsize
            assert rec.device == self.device and rec.dtype == torch.uint8 and rec.numel() >= nr and not rec_host.is_cuda \
                and rec_host.dtype == torch.uint8 and rec_host.is_contiguous() and rec_host.numel() >= nr, what
            return pair

        infix, stages, _held = _stage_args(light, noise and (noise[:2], noise[2]), shake and (shake[:2], shake[2]), self.device, put)
        _lib.check(getattr(_lib.lib(), f"spei_train_batch_runs{infix}_u8")(self._tp(table), C.c_void_p(table_host.data_ptr()), n_in, n_gt, *stages,
                                                                          self._tp(input), self._tp(gt), patch, float(rgb_range), self._stream()),
                   f"spei_train_batch_runs{infix}_u8")

    def train_batch_codec(self, input: torch.Tensor, n_in: int, patch: int, rgb_range: float, records: torch.Tensor,
                          records_host: torch.Tensor, qtabs) -> None:
        """The JPEG-style round trip of speinet_amd.codec IN PLACE on the fp32 input [n_in,3,P,P] (any leading shape) that `train_batch_runs`
        wrote (csrc/codec.hip, spei_train_batch_codec_f32): `records` / `records_host` one speinet_amd.codec.CODEC_RECORD (16 bytes) per
        input record as uint8 tensors on the device and on the host — its tables' index, oy = y0 % 16, ox = x0 % 16 and the table
        record's flags — and `qtabs` the tables as `codec.device_qtabs` returns them.  One launch on the current stream; an `rgb_range`
        whose values do not give their bytes back is a RuntimeError."""
        nb = n_in * 16
        assert records.dtype == torch.uint8 and records.numel() >= nb and not records_host.is_cuda and records_host.dtype == torch.uint8 \
            and records_host.is_contiguous() and records_host.numel() >= nb
        assert input.dtype == torch.float32 and input.numel() == n_in * 3 * patch * patch
        q_dev, q_host, n_qtab = _qtabs(qtabs, self.device)
        _lib.check(_lib.lib().spei_train_batch_codec_f32(self._tp(input), n_in, patch, float(rgb_range), self._tp(records),
                                                         C.c_void_p(records_host.data_ptr()), self._tp(q_dev), C.c_void_p(q_host.data_ptr()), n_qtab,
                                                         self._stream()), "spei_train_batch_codec_f32")

    def rl_prior(self, img: torch.Tensor, iters: int, lam: float = 0.01) -> torch.Tensor:
        """img [3,H,W] -> [3,H,W]."""
        c, h, w = img.shape
        out = torch.empty_like(img)
        scratch = torch.empty_like(img)
        _lib.check(_lib.lib().spei_rl_prior(self._tp(img), self._tp(out), self._tp(scratch), c, h, w, iters, lam, self._stream()),
                   "spei_rl_prior")
        return out

    @_family("conv")
    def conv5_in(self, img: torch.Tensor, w: torch.Tensor, b: torch.Tensor, out: Optional[FMap] = None) -> FMap:
        c, h, wd = img.shape
        assert c == 3
        if out is None:
            out = FMap.empty(h, wd, b.numel(), img.device)
        assert (out.H, out.W, out.C, out.ld, out.off) == (h, wd, b.numel(), b.numel(), 0) and not out.lp
        _lib.check(_lib.lib().spei_conv5_in(self._tp(img), self._tp(w), self._tp(b), self._fp(out), h, wd, b.numel(), self._stream()),
                   "spei_conv5_in")
        return out

    @_family("conv")
    def conv5_out(self, f: FMap, w: torch.Tensor, b: torch.Tensor, out: torch.Tensor, w32=None,
                  b32: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Last conv, NHWC 32 channels -> three NCHW planes.  w32 / b32 (weights zero-padded to 32 output channels,
        packed): the 16-bit modes run the layer on the slab kernel."""
        assert out.shape == (3, f.H, f.W) and out.is_contiguous() and out.dtype == torch.float32
        if self.lp16 and w32 is not None and f.C == 32:
            _lib.check(_lib.lib().spei_conv5_out_slab16(self.fmt, self._fp(f), f.ld, f.fmt, self._tp(w32.frag(self.fmt)), self._tp(b32),
                                                       self._tp(out), f.H, f.W, self._stream()), "spei_conv5_out_slab16")
            return out
        if f.lp:                                   # the fp32 kernel reads fp32 maps (only reached through a stage override)
            f = FMap(f.t.float(), f.H, f.W, f.C, f.off)
        _lib.check(_lib.lib().spei_conv5_out(self._fp(f), f.ld, self._tp(w), self._tp(b), self._tp(out), f.H, f.W, f.C, self._stream()),
                   "spei_conv5_out")
        return out

    # ---- the GEMM family ---------------------------------------------------------------------------------------
    def _conv3_pipe_ok(self, a, w, N: int, ksize: int, stride: int, act: int, residual, out) -> bool:
        """The persistent 3x3 / 256-channel kernel takes the call: dense fp32 maps, 6 x 16 pixel tiles cover the map, 16-bit single products."""
        return (self.conv3_pipe and self.lp16 and ksize == 3 and stride == 1 and N == 256 and a.C == 256 and act == ACT_NONE
                and a.H % 6 == 0 and a.W % 16 == 0 and a.H * a.W <= (1 << 21) and a.t.dtype == torch.float32 and getattr(a, "ld", 256) == 256
                and getattr(a, "off", 0) == 0 and getattr(w, "fhi", None) is not None and tuple(w.shape) == (9, 256, 256)
                and (out is None or (out.t.dtype == torch.float32 and getattr(out, "ld", 256) == 256 and getattr(out, "off", 0) == 0
                                     and out.t.data_ptr() != a.t.data_ptr()))
                and (residual is None or (residual.t.dtype == torch.float32 and getattr(residual, "ld", 256) == 256 and getattr(residual, "off", 0) == 0)))

    def _persistent_conv(self, a, w, bias, N: int, ksize: int, stride: int, act: int, residual, out, batch: int) -> bool:
        """Launch the persistent kernel that takes this conv layer, if one does: the pipelined 3x3 / 256-channel kernel or the
        weight-stationary 5x5 kernels for 32 / 64 channels.  a, out, residual: FMaps (batch 1) or BMaps of `batch` maps, each spanning
        its whole buffer, `out` not `a`; the caller has a one-source conv without row scale or LayerNorm staging.  False: nothing
        launched, the slab kernel runs the layer."""
        tp, lib, f = self._tp, _lib.lib(), self.fmt
        if self._conv3_pipe_ok(a, w, N, ksize, stride, act, residual, out):
            _lib.check(lib.spei_conv3x3_256_pipe16(f, tp(a.t), tp(w.frag(f)), tp(bias), tp(residual.t) if residual is not None else _vp(0),
                                                   tp(out.t), batch, a.H, a.W, self._stream()), "spei_conv3x3_256_pipe16")
            return True
        if not (ksize == 5 and stride == 1 and a.C == N and residual is None and act in (ACT_NONE, ACT_RELU) and w.fhi is not None
                and (getattr(a, "ld", N), getattr(a, "off", 0), getattr(out, "ld", N), getattr(out, "off", 0)) == (N, 0, N, 0)
                and a.t.data_ptr() != out.t.data_ptr()):
            return False
        if N == 32 and self.conv32_ws_available():
            # the 32-channel 5x5 layers: weight-stationary persistent kernel (csrc/conv32_ws16.hip)
            _lib.check(lib.spei_conv32_ws16(f, tp(a.t), a.fmt, tp(w.frag(f)), tp(bias), tp(out.t), out.fmt, batch, a.H, a.W, act,
                                            self._stream()), "spei_conv32_ws16")
            return True
        if N == 64 and self.conv64_ws_available():
            # the 64-channel 5x5 layers: weight-stationary persistent kernel (csrc/conv64_ws16.hip)
            _lib.check(lib.spei_conv64_ws16(f, tp(a.t), a.fmt, tp(w.frag(f)), tp(bias), tp(out.t), out.fmt, batch, a.H, a.W, act,
                                            self._stream()), "spei_conv64_ws16")
            return True
        return False

    @_family("conv")
    def igemm(self, a0: FMap, w, bias: Optional[torch.Tensor], N: int, ksize: int = 1, stride: int = 1,
              mode: int = CONV, act: int = ACT_NONE, a1: Optional[FMap] = None, residual: Optional[FMap] = None,
              rowscale: Optional[torch.Tensor] = None, out: Optional[FMap] = None, out_dtype=torch.float32,
              ln_input: bool = False) -> FMap:
        prec = self.precision
        pad = ksize // 2
        if mode == CONV:
            ho, wo = (a0.H + 2 * pad - ksize) // stride + 1, (a0.W + 2 * pad - ksize) // stride + 1
        else:
            ho, wo = a0.H * stride, a0.W * stride
        if out is None:
            out = FMap.empty(ho, wo, N, a0.t.device, out_dtype)
        assert out.H == ho and out.W == wo and out.C == N
        k0, k1 = a0.C, (a1.C if a1 is not None else 0)
        slab = prec != "f32" and mode == CONV
        assert slab or (mode == CONV_T and self.lp16) or not (a0.lp or out.lp), \
            "16-bit activations are only supported by the slab kernel"
        assert a1 is None or a1.t.dtype == a0.t.dtype
        assert residual is None or not residual.lp
        assert all(f.t.dtype in (torch.float32, LP_DTYPE[self.fmt]) for f in (a0, out)), "16-bit tensors must be in the mode's format"
        if torch.is_tensor(w):
            w = PackedW(w, a0.t.device)
        assert not ln_input or (slab and w.fhi is not None), "ln_input is a feature of the slab kernel"
        assert tuple(w.shape) == (ksize * ksize, N, k0 + k1), (tuple(w.shape), ksize, N, k0, k1)
        if a1 is not None:
            assert (a1.H, a1.W) == (a0.H, a0.W)
        if residual is not None:
            assert (residual.H, residual.W, residual.C) == (ho, wo, N)
        if rowscale is not None:
            assert rowscale.numel() == ho * wo
        tp, fp = self._tp, self._fp
        srcs = (fp(a0), a0.ld, k0, fp(a1), a1.ld if a1 is not None else 0, k1)
        lib = _lib.lib()
        if (mode == CONV and a1 is None and rowscale is None and not ln_input
                and self._persistent_conv(a0, w, bias, N, ksize, stride, act, residual, out, 1)):
            return out
        if (mode == CONV_T and self.lp16 and ksize == 3 and stride == 2 and a1 is None and residual is None
                and rowscale is None and N % 32 == 0 and k0 % 32 == 0):
            # stride-2 transposed conv = four stride-1 convs (one per output parity) on the slab kernel
            cf = w.convT_class_frags(self.fmt)
            _lib.check(lib.spei_convt2_slab16(self.fmt, fp(a0), a0.ld, k0, a0.fmt, tp(cf[(0, 0)]), tp(cf[(0, 1)]), tp(cf[(1, 0)]),
                                              tp(cf[(1, 1)]), tp(bias), fp(out), out.ld, out.fmt, a0.H, a0.W, N, act,
                                              self._stream()), "spei_convt2_slab16")
        elif (mode == CONV_T and prec == "bf16x3" and ksize == 3 and stride == 2 and a1 is None and residual is None
                and rowscale is None and N % 32 == 0 and k0 % 32 == 0 and not a0.lp and not out.lp):
            # the same in split arithmetic (the transposed conv that ends decoder_second inside an f16 frame's split stages; round 1's igemm
            # kernel took 327 us for it)
            _hi, _lo, ph, pl = w.convT_class_frags_split()
            _lib.check(lib.spei_convt2_slab16x3(fp(a0), a0.ld, k0, ph, pl, tp(bias), fp(out), out.ld, a0.H, a0.W, N, act, self._stream()),
                       "spei_convt2_slab16x3")
        elif prec == "f32":
            _lib.check(lib.spei_igemm_f32(*srcs, tp(w.f32), tp(bias), fp(out), out.ld, fp(residual), residual.ld if residual is not None else 0,
                                          tp(rowscale), a0.H, a0.W, ho, wo, N, ksize, stride, pad, mode, act, self._stream()), "spei_igemm_f32")
        elif slab and w.fhi is not None:
            dims = (a0.H * a0.W, 1, ho * wo, 1) if (ksize == 1 and stride == 1) else (a0.H, a0.W, ho, wo)
            _lib.check(lib.spei_conv_slab16(
                self.fmt, *srcs, a0.fmt, tp(w.frag(self.fmt)), tp(w.flo) if prec == "bf16x3" else _vp(0), tp(bias), fp(out), out.ld,
                out.fmt, fp(residual), residual.ld if residual is not None else 0,
                tp(rowscale), *dims, N, ksize, stride, pad, act, int(ln_input), self._stream()), "spei_conv_slab16")
        else:
            raise ValueError(f"no {prec} kernel for N={N} K={k0 + k1} ksize={ksize} stride={stride} mode={mode}: N and K must be multiples "
                             "of 32; transposed convs 3x3 stride 2")
        return out

    def linear(self, x: torch.Tensor, w, b: Optional[torch.Tensor], act: int = ACT_NONE,
               residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, out_dtype=torch.float32,
               ln_input: bool = False) -> torch.Tensor:
        """Token-space linear: x [M,K] -> [M,N]; w [N,K]."""
        m, k = x.shape
        if torch.is_tensor(w):
            w = PackedW(w.reshape(1, *w.shape), x.device)
        n = w.shape[1]
        if out is None:
            out = torch.empty(m, n, device=x.device, dtype=out_dtype)
        self.igemm(FMap(x, m, 1, k), w, b, n, act=act, ln_input=ln_input,
                   residual=FMap(residual, m, 1, n) if residual is not None else None, out=FMap(out, m, 1, n))
        return out

    # ---- ResBlock (K3) -----------------------------------------------------------------------------------------
    @_family("streaming")
    def resblock_gates(self, x1: FMap, pk: dict):
        dev = x1.t.device
        lib = _lib.lib()
        tp = self._tp
        assert x1.off == 0 and x1.ld == x1.C
        s = torch.empty(x1.C, device=dev)
        g1 = torch.empty(x1.H, x1.C, device=dev)
        g2 = torch.empty(x1.W, x1.C, device=dev)
        ws = torch.empty(lib.spei_gate_ws_floats(x1.H, x1.W, x1.C), device=dev)
        _lib.check(lib.spei_resblock_gates(self._fp(x1), x1.fmt, x1.H, x1.W, x1.C, tp(pk["se_w1"]), tp(pk["se_b1"]), tp(pk["se_w2"]),
                                           tp(pk["se_b2"]), tp(pk["cw_w"]), tp(pk["cw_bn"]), tp(pk["hc_w"]), tp(pk["hc_bn"]),
                                           tp(s), tp(g1), tp(g2), tp(ws), self._stream()), "spei_resblock_gates")
        return s, g1, g2

    def resblock(self, x: FMap, pk: dict, extra: Optional[FMap] = None, out: Optional[FMap] = None) -> FMap:
        """x + SE(x1) + TE(x1), x1 = conv5(relu(conv5(x)))  (reference model/block.py:127-140)."""
        idt = self.inter_dtype()
        c = x.C
        assert x.off == 0 and x.ld == c
        t = self.igemm(x, pk["w1"], pk["b1"], c, ksize=5, act=ACT_RELU, out_dtype=idt)   # only conv2 reads it
        x1 = self.igemm(t, pk["w2"], pk["b2"], c, ksize=5, out_dtype=idt if self.x1_bf16 else torch.float32)
        s, g1, g2 = self.resblock_gates(x1, pk)
        if out is None:
            out = FMap.empty(x.H, x.W, c, x.t.device)
        if extra is not None:
            assert extra.off == 0 and extra.ld == c
        self._apply(x, x1, s, g1, g2, extra, out, c)
        return out

    @_family("streaming")
    def _apply(self, x, x1, s, g1, g2, extra, out, c):
        _lib.check(_lib.lib().spei_resblock_apply(self._fp(x), self._fp(x1), x1.fmt, self._tp(s), self._tp(g1), self._tp(g2),
                                                  self._fp(extra), self._fp(out), out.ld, x.H, x.W, c, self._stream()),
                   "spei_resblock_apply")

    # ---- the same stacks on several maps per launch (the frame's encoder passes) -------------------------------------------------
    def batched_available(self) -> bool:
        """One launch per layer for all maps of a BMap (the frame's encoder passes): the single-product 16-bit modes on the slab kernel."""
        return self.batched_kernels() and self.x1_bf16 and self.bf16_storage and self.batch_enc

    def conv32_ws_available(self) -> bool:
        """The weight-stationary kernel for 32 -> 32 channel 5x5 layers (single-product 16-bit modes)."""
        return self.lp16 and self.conv32_ws

    def conv64_ws_available(self) -> bool:
        """The weight-stationary kernel for 64 -> 64 channel 5x5 layers (single-product 16-bit modes; `conv64_ws` None follows `conv32_ws`)."""
        return self.lp16 and (self.conv32_ws if self.conv64_ws is None else self.conv64_ws)

    def batched_kernels(self) -> bool:
        """`igemm_batched` can run (what the batched Swin calls need; `batch_enc` only decides about the encoder passes)."""
        return self.lp16

    @_family("conv")
    def igemm_batched(self, a: BMap, w, bias: torch.Tensor, N: int, ksize: int, stride: int = 1, act: int = ACT_NONE,
                      out_dtype=torch.float32, residual: Optional[BMap] = None, out: Optional[BMap] = None) -> BMap:
        """One conv layer on every map of `a` in one launch (gridDim.y = map).  residual: fp32 maps of the output shape added in the
        epilogue; it may be `out` itself (each workgroup reads the residual of its own pixels before it writes them), never `a`."""
        assert self.batched_kernels() and not torch.is_tensor(w) and w.fhi is not None
        pad = ksize // 2
        ho, wo = (a.H + 2 * pad - ksize) // stride + 1, (a.W + 2 * pad - ksize) // stride + 1
        assert tuple(w.shape) == (ksize * ksize, N, a.C) and a.t.dtype in (torch.float32, LP_DTYPE[self.fmt])
        if out is None:
            out = BMap.empty(a.B, ho, wo, N, a.t.device, out_dtype)
        assert (out.B, out.H, out.W, out.C) == (a.B, ho, wo, N) and out.t.data_ptr() != a.t.data_ptr()
        if residual is not None:
            assert (residual.B, residual.H, residual.W, residual.C) == (a.B, ho, wo, N) and residual.t.dtype == torch.float32
            assert residual.t.data_ptr() != a.t.data_ptr()
        tp = self._tp
        if self._persistent_conv(a, w, bias, N, ksize, stride, act, residual, out, a.B):
            return out
        _lib.check(_lib.lib().spei_conv_slab16_batched(self.fmt, tp(a.t), a.C, a.fmt, tp(w.frag(self.fmt)), _vp(0), tp(bias), tp(out.t), out.fmt,
                                                       tp(residual.t) if residual is not None else _vp(0), a.B, a.H, a.W, ho, wo, N, ksize,
                                                       stride, pad, act, self._stream()),
                   "spei_conv_slab16_batched")
        return out

    def resblock_batched(self, x: BMap, pk: dict, routes: Optional[list] = None) -> Optional[BMap]:
        """`resblock` on every map of x: conv1, conv2, gate statistics, gate maps and the gated sum are ONE launch each.  `routes`: see
        `_gates_apply_batched`."""
        idt = self.inter_dtype()
        c, dev = x.C, x.t.device
        lib = _lib.lib()
        tp = self._tp
        t = self.igemm_batched(x, pk["w1"], pk["b1"], c, 5, act=ACT_RELU, out_dtype=idt)
        x1 = self.igemm_batched(t, pk["w2"], pk["b2"], c, 5, out_dtype=idt)
        del t
        return self._gates_apply_batched(x, x1, pk, routes)

    @_family("streaming")
    def _gates_apply_batched(self, x: BMap, x1: BMap, pk: dict, routes: Optional[list] = None) -> Optional[BMap]:
        """Gate statistics, gate maps and the gated sum x' of every map.  `routes` None: x' of all maps as one fp32 BMap.  Else a list of at
        most APPLY_MAX_ROUTES tuples (src, partner, out32, out16) and nothing is returned: x' of map `src` — plus x' of map `partner`
        unless that is None — goes to the fp32 FMap `out32` (any row stride) and / or, rounded to the mode's 16-bit format, to the dense
        16-bit FMap `out16` (spei_resblock_apply_routed); maps that no route names are not written."""
        c, dev = x.C, x.t.device
        lib = _lib.lib()
        tp = self._tp
        s = torch.empty(x.B, c, device=dev)
        g1 = torch.empty(x.B, x.H, c, device=dev)
        g2 = torch.empty(x.B, x.W, c, device=dev)
        ws = torch.empty(x.B * lib.spei_gate_ws_floats(x.H, x.W, c), device=dev)
        _lib.check(lib.spei_resblock_gates_batched(tp(x1.t), x1.fmt, x.B, x.H, x.W, c, tp(pk["se_w1"]), tp(pk["se_b1"]), tp(pk["se_w2"]),
                                                   tp(pk["se_b2"]), tp(pk["cw_w"]), tp(pk["cw_bn"]), tp(pk["hc_w"]), tp(pk["hc_bn"]),
                                                   tp(s), tp(g1), tp(g2), tp(ws), self._stream()), "spei_resblock_gates_batched")
        if routes is not None:
            assert self.lp16 and 1 <= len(routes) <= APPLY_MAX_ROUTES
            arr = (_ApplyRoute * len(routes))()
            for r, (src, partner, o32, o16) in zip(arr, routes):
                assert 0 <= src < x.B and (partner is None or (0 <= partner < x.B and partner != src)) and (o32 is not None or o16 is not None)
                for o, dt in ((o32, torch.float32), (o16, LP_DTYPE[self.fmt])):
                    assert o is None or ((o.H, o.W, o.C) == (x.H, x.W, c) and o.t.dtype == dt and o.t.device == self.device)
                assert o16 is None or (o16.ld, o16.off) == (c, 0)
                r.src, r.partner = src, -1 if partner is None else partner
                r.out32, r.ld32 = (o32.ptr, o32.ld) if o32 is not None else (None, 0)
                r.out16 = o16.ptr if o16 is not None else None
            _lib.check(lib.spei_resblock_apply_routed(self.fmt, tp(x.t), tp(x1.t), x1.fmt, tp(s), tp(g1), tp(g2), arr, len(routes), x.B,
                                                      x.H, x.W, c, self._stream()), "spei_resblock_apply_routed")
            return None
        out = BMap.empty(x.B, x.H, x.W, c, dev)
        _lib.check(lib.spei_resblock_apply_batched(tp(x.t), tp(x1.t), x1.fmt, tp(s), tp(g1), tp(g2), tp(out.t), x.B, x.H, x.W, c,
                                                   self._stream()), "spei_resblock_apply_batched")
        return out

    # ---- Swin (K6-K9) ------------------------------------------------------------------------------------------
    def ln_fused_available(self) -> bool:
        """LayerNorm folded into the staging of the following 256-wide linear (slab kernel, every mode but f32)."""
        return self.precision != "f32"

    def attn_fused_available(self) -> bool:
        return self.lp16 and self.fuse_attn and self.bf16_storage

    def mlp_fused_available(self) -> bool:
        return self.lp16 and self.fuse_mlp

    def swin_multi_available(self) -> bool:
        """The Swin calls of a frame as one batch over stacked maps (engine.swin_multi): needs the batched attention kernel."""
        return self.attn_fused_available() and self.attn_win4 and self.mlp_fused_available() and self.batched_kernels()

    @_family("swin")
    def attn_fused(self, x: torch.Tensor, yhat: torch.Tensor, bk: dict, H: int, W: int, shift: int, out: torch.Tensor) -> torch.Tensor:
        """out = x + proj(window_attention(...))  (reference model/swinir.py:238-278); in place when out is x.  x, yhat, out:
        [B * H * W, 256], B >= 1 equally sized maps stacked (the Swin calls of a frame share the block's weights); B > 1 needs the
        batched four-window kernel (`attn_win4`)."""
        assert x.shape[0] % (H * W) == 0 and x.shape[1] == 256 and x.dtype == torch.float32 and out.shape == x.shape and out.dtype == torch.float32
        f = self.fmt
        assert yhat.shape == x.shape and yhat.dtype == LP_DTYPE[f]
        tp = self._tp
        batch = x.shape[0] // (H * W)
        if self.attn_win4:
            _lib.check(_lib.lib().spei_attn_win4_16(f, tp(x), tp(out), tp(yhat), tp(bk["wq"].frag(f)), tp(bk["bq"]), tp(bk["wkv"].frag(f)),
                                                    tp(bk["bkv"]), tp(bk["wproj"].frag(f)), tp(bk["bproj"]), tp(bk["relbias"]), batch, H, W,
                                                    shift, self._stream()), "spei_attn_win4_16")
            return out
        assert batch == 1, "the two-window kernel takes one map per launch"
        _lib.check(_lib.lib().spei_attn_fused16(f, tp(x), tp(out), tp(yhat), tp(bk["wq"].frag(f)), tp(bk["bq"]), tp(bk["wkv"].frag(f)),
                                                tp(bk["bkv"]), tp(bk["wproj"].frag(f)), tp(bk["bproj"]), tp(bk["relbias"]), H, W, shift,
                                                self._stream()), "spei_attn_fused16")
        return out

    @_family("swin")
    def mlp_fused(self, x: torch.Tensor, w1, b1: torch.Tensor, w2, b2: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """out = x + fc2(gelu(fc1(LN(x))))  (reference model/swinir.py:279); in place when out is x."""
        assert x.shape[1] == 256 and x.dtype == torch.float32 and out.shape == x.shape and out.dtype == torch.float32
        assert tuple(w1.shape) == (1, 512, 256) and tuple(w2.shape) == (1, 256, 512)
        tp = self._tp
        f = self.fmt
        _lib.check(_lib.lib().spei_mlp_fused16(f, tp(x), tp(out), tp(w1.frag(f)), tp(b1), tp(w2.frag(f)), tp(b2), x.shape[0], self._stream()),
                   "spei_mlp_fused16")
        return out

    def layernorm(self, x: torch.Tensor, g: Optional[torch.Tensor] = None, b: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, out_dtype=torch.float32) -> torch.Tensor:
        assert x.shape[1] == 256 and x.is_contiguous() and x.dtype == torch.float32
        if out is None:
            out = torch.empty(x.shape, device=x.device, dtype=out_dtype)
        tp = self._tp
        _lib.check(_lib.lib().spei_layernorm256(tp(x), tp(out), fmt_of(out.dtype), tp(g), tp(b), x.shape[0], self._stream()),
                   "spei_layernorm256")
        return out

    def layernorm_twice(self, x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, out_dtype=torch.float32) -> torch.Tensor:
        """layernorm(layernorm(x, g, b), out_dtype=out_dtype) in one launch, the first result in registers: the same bits."""
        assert x.shape[1] == 256 and x.is_contiguous() and x.dtype == torch.float32 and g.numel() == b.numel() == 256
        out = torch.empty(x.shape, device=x.device, dtype=out_dtype)
        tp = self._tp
        _lib.check(_lib.lib().spei_layernorm256_twice(tp(x), tp(out), fmt_of(out.dtype), tp(g), tp(b), x.shape[0], self._stream()),
                   "spei_layernorm256_twice")
        return out

    def window_attention(self, q: torch.Tensor, kv: torch.Tensor, relbias: torch.Tensor, H: int, W: int, shift: int,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
        assert q.shape == (H * W, 256) and kv.shape == (H * W, 512) and relbias.shape == (8, 25, 25)
        if out is None:
            out = torch.empty_like(q)
        assert q.dtype == kv.dtype == out.dtype
        tp = self._tp
        _lib.check(_lib.lib().spei_window_attention(tp(q), tp(kv), fmt_of(q.dtype), tp(relbias), tp(out), H, W, shift,
                                                    self._stream()), "spei_window_attention")
        return out

    # ---- SearchTransfer (K10-K12) ------------------------------------------------------------------------------
    def patch_invnorm(self, f: FMap) -> torch.Tensor:
        inv = torch.empty(f.H * f.W, device=f.t.device)
        _lib.check(_lib.lib().spei_patch_invnorm(self._fp(f), f.ld, self._tp(inv), f.H, f.W, f.C, self._stream()), "spei_patch_invnorm")
        return inv

    def corr_plan(self, lr: FMap, ref: FMap, inv_lr: torch.Tensor, inv_ref: torch.Tensor) -> "CorrPlan":
        """Everything of K11 except the arg-max kernel itself: output / workspace allocation and the one-off 16-bit
        conversion of the two maps.  `plan.launch()` then runs the dominant kernel of the path (timed by `profile`), so a
        caller can place it between two captured graph segments and bracket it with HIP events (bench.py)."""
        lib = _lib.lib()
        dev = lr.t.device
        tp, fp = self._tp, self._fp
        n = lr.H * lr.W
        s = torch.empty(n, device=dev)
        arg = torch.empty(n, device=dev, dtype=torch.int32)
        dims = (lr.H, lr.W, ref.H, ref.W, lr.C)
        rescore = self.precision != "f32" and self.corr_precision == "top2" and lr.C == 128
        # the diagonal kernel keeps one candidate pair per (query, diagonal, reference tile): 415 MB at 720p, ~34 GB at 4K — beyond the
        # budget (a quarter of the device's free memory, at most 8 GiB) the slab kernel takes over (its workspace is per query only)
        diag, diag_floats = False, 0
        if rescore and self.corr_diag and ref.H >= lr.H:
            diag_floats = lib.spei_corr_diag_ws_floats(lr.H, lr.W, ref.H, ref.W)
            diag = 4 * diag_floats <= min(torch.cuda.mem_get_info(dev)[0] // 4, CORR_DIAG_WS_MAX)
        ws = torch.empty(diag_floats if diag else lib.spei_corr_ws_floats(n), device=dev)
        if self.precision == "f32":
            args = (fp(lr), lr.ld, fp(ref), ref.ld, tp(inv_lr), tp(inv_ref), *dims, tp(s), tp(arg), tp(ws))
            return CorrPlan(self, s, arg, "corr_argmax_kernel (f32 MFMA)", [(lib.spei_corr_argmax, "spei_corr_argmax", args)], [],
                            (lr, ref, inv_lr, inv_ref, ws))
        split = self.corr_precision == "bf16x3"
        f16 = BF16 if (rescore and self.corr_bf16) else self.fmt
        assert f16 == BF16 or (not split and lr.C == 128), "f16 correlation: slab kernel, single / top2"
        parts = []
        for f in (lr, ref):
            hi = torch.empty(f.H * f.W, f.C, device=dev, dtype=LP_DTYPE[f16])
            lo = torch.empty_like(hi) if split else None
            _lib.check(lib.spei_split16(f16, fp(f), f.ld, tp(hi), tp(lo), f.H * f.W, f.C, self._stream()), "spei_split16")
            parts += [hi, lo]
        fname = "f16" if f16 == F16 else "bf16"
        if rescore:
            arg2 = torch.empty(n, device=dev, dtype=torch.int32)
            s2 = torch.empty(n, device=dev)
            if diag:
                main = (lib.spei_corr_diag_top2_16, "spei_corr_diag_top2_16",
                        (f16, tp(parts[0]), tp(parts[2]), tp(inv_ref), *dims, tp(s), tp(arg), tp(s2), tp(arg2), tp(ws)))
            else:
                main = (lib.spei_corr_slab_top2_16, "spei_corr_slab_top2_16",
                        (f16, tp(parts[0]), tp(parts[2]), tp(inv_lr), tp(inv_ref), *dims, tp(s), tp(arg), tp(s2), tp(arg2), tp(ws)))
            post = (lib.spei_corr_rescore, "spei_corr_rescore",
                    (fp(lr), lr.ld, fp(ref), ref.ld, tp(inv_lr), tp(inv_ref), *dims, tp(s), tp(arg), tp(s2), tp(arg2)))
            return CorrPlan(self, s, arg, f"corr_{'diag' if diag else 'slab'}_kernel<top2, {fname}>", [main], [post],
                            (lr, ref, inv_lr, inv_ref, ws, parts, s2, arg2))
        args = (tp(parts[0]), tp(parts[1]), tp(parts[2]), tp(parts[3]), tp(inv_lr), tp(inv_ref), *dims, tp(s), tp(arg), tp(ws))
        if lr.C == 128:
            main = (lib.spei_corr_slab16, "spei_corr_slab16", (f16, *args))
            kname = f"corr_slab_kernel<{'bf16x3' if split else 'top1, ' + fname}>"
        else:
            main = (lib.spei_corr_argmax_bf16, "spei_corr_argmax_bf16", args)
            kname = f"corr_bf16_kernel<{'bf16x3' if split else 'bf16'}>"
        return CorrPlan(self, s, arg, kname, [main], [], (lr, ref, inv_lr, inv_ref, ws, parts))

    def corr_argmax(self, lr: FMap, ref: FMap, inv_lr: torch.Tensor, inv_ref: torch.Tensor):
        plan = self.corr_plan(lr, ref, inv_lr, inv_ref)
        plan.launch()
        return plan.s, plan.arg

    def gather_fold(self, ref: FMap, arg: torch.Tensor, H3: int, W3: int, Hr3: int, Wr3: int, s: int) -> FMap:
        assert ref.H == Hr3 * s and ref.W == Wr3 * s
        out = FMap.empty(H3 * s, W3 * s, ref.C, ref.t.device)
        _lib.check(_lib.lib().spei_gather_fold(self._fp(ref), ref.ld, self._tp(arg), self._fp(out), out.ld, H3, W3, Hr3, Wr3, ref.C, s,
                                               self._stream()), "spei_gather_fold")
        return out

    # ---- glue (K13-K14) ----------------------------------------------------------------------------------------
    def rot90(self, f: FMap) -> FMap:
        out = FMap.empty(f.W, f.H, f.C, f.t.device)
        _lib.check(_lib.lib().spei_rot90(self._fp(f), f.ld, self._fp(out), f.H, f.W, f.C, self._stream()), "spei_rot90")
        return out

    def upsample(self, f: FMap, s: int, act: int = ACT_NONE, out_dtype=torch.float32) -> FMap:
        """out_dtype: fp32, or the 16-bit format of the single-product convs that are the map's only readers (x2 only)."""
        out = FMap.empty(f.H * s, f.W * s, f.C, f.t.device, out_dtype)
        if out_dtype == torch.float32:
            _lib.check(_lib.lib().spei_upsample_bicubic(self._fp(f), f.ld, self._fp(out), out.ld, f.H, f.W, f.C, s, act, self._stream()),
                       "spei_upsample_bicubic")
        else:
            _lib.check(_lib.lib().spei_upsample_bicubic_fmt(self._fp(f), f.ld, self._fp(out), out.ld, out.fmt, f.H, f.W, f.C, s, act,
                                                            self._stream()), "spei_upsample_bicubic_fmt")
        return out

    def up_conv1x1_relu(self, f: FMap, w, b: torch.Tensor, n: int, s: int = 2, out_dtype=torch.float32) -> FMap:
        """relu(conv1x1(bicubic_up(f))) (reference model/speinet.py:96-97,108-109, model/SearchTransfer.py:73-76).  Both maps
        are linear and the bicubic weights sum to 1, so the 16-bit modes run the conv first, at 1/s^2 of the pixels and with
        half the bytes through the upsampler; the f32-grade modes keep the reference's order of operations."""
        if (self.lp16 and self.commute_upconv) or self.commute_any:
            return self.upsample(self.igemm(f, w, b, n), s, act=ACT_RELU, out_dtype=out_dtype)
        return self.igemm(self.upsample(f, s), w, b, n, act=ACT_RELU, out_dtype=out_dtype)

    def add(self, a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        if out is None:
            out = torch.empty_like(a)
        assert out.shape == a.shape == b.shape and out.dtype == a.dtype == torch.float32
        _lib.check(_lib.lib().spei_add(self._tp(a), self._tp(b), self._tp(out), a.numel(), self._stream()), "spei_add")
        return out


_BOOL_KNOBS = tuple(f.name for f in dataclasses.fields(Ctx) if f.type in (bool, "bool"))      # Ctx.__post_init__ coerces these to bool
