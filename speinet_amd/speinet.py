"""Drop-in for the reference's ``model/speinet.py``: same class name, constructor, ``forward`` contract,
``make_model(args)`` factory and 1020-entry ``state_dict`` layout — but ``forward``
runs hand-written gfx950 kernels through the C-ABI in include/speinet_hip.h.

The sub-modules below exist to hold parameters under the reference's names (reference
model/recons_video_ori.py:16-84, model/block.py:8-140, model/swinir.py:64-149,163-213,421-484,620-761,
model/SearchTransfer.py:6-11,53-57); none of their ``forward`` methods is ever called.  Weights are re-packed
into kernel layouts on first use after every (re)load (speinet_amd/pack.py), never in the checkpoint.

There is deliberately NO CPU path: a tensor that is not on a ROCm device, or a missing libspeinet_hip.so,
raises.  The CPU restatement lives in oracle/ and is test infrastructure only.
"""
from __future__ import annotations

import inspect
import os
from types import SimpleNamespace
from typing import Optional, Sequence

import torch
import torch.nn as nn

from . import _lib, engine, ops, pack


# ---------------------------------------------------------------------------------------------------------
# parameter containers (names == reference names)
# ---------------------------------------------------------------------------------------------------------
class _BasicConv(nn.Module):
    def __init__(self, cin, cout, k, relu):
        super().__init__()
        layers = [nn.Conv2d(cin, cout, k, padding=k // 2)]
        if relu:
            layers.append(nn.ReLU(inplace=True))
        self.main = nn.Sequential(*layers)


class _SE(nn.Module):
    def __init__(self, c, reduction=4):
        super().__init__()
        mid = int(c / reduction)
        self.fc = nn.Sequential(nn.Linear(c, mid), nn.ReLU(inplace=True), nn.Linear(mid, c), nn.Sigmoid())


class _GateConv(nn.Module):
    def __init__(self, k):
        super().__init__()
        self.conv = nn.Conv2d(2, 1, k, padding=(k - 1) // 2, bias=False)
        self.bn = nn.BatchNorm2d(1, eps=1e-5, momentum=0.01, affine=True)


class _Gate(nn.Module):
    def __init__(self, k):
        super().__init__()
        self.conv = _GateConv(k)


class _Triplet(nn.Module):
    def __init__(self):
        super().__init__()
        self.cw = _Gate(7)
        self.hc = _Gate(5)


class _ResBlock(nn.Module):
    def __init__(self, c, k=5):
        super().__init__()
        self.main = nn.Sequential(_BasicConv(c, c, k, True), _BasicConv(c, c, k, False))
        self.se = _SE(c, 4)
        self.te = _Triplet()


class _Recons(nn.Module):
    def __init__(self, in_ch, out_ch, n_resblock, nf, k=5):
        super().__init__()
        rb = lambda c: [_ResBlock(c, k) for _ in range(n_resblock)]
        head = lambda ci, co, s: nn.Sequential(nn.Conv2d(ci, co, k, stride=s, padding=k // 2), nn.ReLU(inplace=True))
        tail = lambda ci, co: nn.Sequential(nn.ConvTranspose2d(ci, co, 3, stride=2, padding=1, output_padding=1), nn.ReLU(inplace=True))
        self.inBlock = nn.Sequential(head(in_ch, nf, 1), *rb(nf))
        self.encoder_first = nn.Sequential(head(nf, nf * 2, 2), *rb(nf * 2))
        self.encoder_second = nn.Sequential(head(nf * 2, nf * 4, 2), *rb(nf * 4))
        self.decoder_second = nn.Sequential(*rb(nf * 4), tail(nf * 4, nf * 2))
        self.decoder_first = nn.Sequential(*rb(nf * 2), tail(nf * 2, nf))
        self.outBlock = nn.Sequential(*rb(nf), nn.Conv2d(nf, out_ch, k, padding=k // 2))


class _WindowAttention(nn.Module):
    def __init__(self, dim, ws, heads):
        super().__init__()
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * ws - 1) * (2 * ws - 1), heads))
        self.register_buffer("relative_position_index", pack.rel_pos_index(ws))
        self.qkv_x = nn.Linear(dim, dim * 2)
        self.qkv_y = nn.Linear(dim, dim)
        self.proj = nn.Linear(dim, dim)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)


class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


def _shift_mask(h: int, w: int, ws: int, shift: int) -> torch.Tensor:
    """calculate_mask (reference model/swinir.py:215-236) — kept only as the checkpoint buffer ``attn_mask``;
    the kernel derives the mask from coordinates."""
    def region(n):
        r = torch.zeros(n, dtype=torch.long)
        r[n - ws:n - shift] = 1
        r[n - shift:] = 2
        return r
    reg = (3 * region(h)[:, None] + region(w)[None, :]).view(h // ws, ws, w // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)
    d = reg[:, None, :] - reg[:, :, None]
    return torch.where(d != 0, torch.tensor(-100.0), torch.tensor(0.0))


class _SwinBlock(nn.Module):
    def __init__(self, dim, res, heads, ws, shift, mlp_ratio):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attn = _WindowAttention(dim, ws, heads)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio))
        self.register_buffer("attn_mask", _shift_mask(res, res, ws, shift) if shift > 0 else None)


class _BasicLayer(nn.Module):
    def __init__(self, dim, res, depth, heads, ws, mlp_ratio):
        super().__init__()
        self.blocks = nn.ModuleList([_SwinBlock(dim, res, heads, ws, 0 if i % 2 == 0 else ws // 2, mlp_ratio) for i in range(depth)])


class _RSTB(nn.Module):
    def __init__(self, dim, res, depth, heads, ws, mlp_ratio):
        super().__init__()
        self.residual_group = _BasicLayer(dim, res, depth, heads, ws, mlp_ratio)
        self.conv = nn.Conv2d(dim, dim, 3, 1, 1)


class _PatchEmbed(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.norm = nn.LayerNorm(dim)


class _SwinIR(nn.Module):
    def __init__(self, in_chans, img_size, ws, depths, embed_dim, heads, mlp_ratio):
        super().__init__()
        self.conv_first = nn.Conv2d(in_chans, embed_dim, 3, 1, 1)
        self.patch_embed = _PatchEmbed(embed_dim)
        self.layers = nn.ModuleList([_RSTB(embed_dim, img_size, depths[i], heads[i], ws, mlp_ratio) for i in range(len(depths))])
        self.norm = nn.LayerNorm(embed_dim)
        self.conv_after_body = nn.Conv2d(embed_dim, embed_dim, 3, 1, 1)
        self.conv_last = nn.Conv2d(embed_dim, in_chans, 3, 1, 1)


class _Transfer(nn.Module):
    def __init__(self, nf=32):
        super().__init__()
        self.search1 = nn.Conv2d(nf * 4, nf * 2, 1)
        self.search2 = nn.Conv2d(nf * 2, nf, 1)


def default_args() -> SimpleNamespace:
    """The hyper-parameters of the reference's SPEINet template / inference presets
    (option/template.py:3-21, inference_SPEINet.py:626-697)."""
    return SimpleNamespace(n_colors=3, n_sequence=3, patch_size=200, n_feat=32, n_resblock=3, size_must_mode=4,
                           window_size=5, depths=[6] * 6, embed_dim=256, num_heads=[8] * 6, mlp_ratio=2,
                           resi_connection="1conv", rgb_range=1, n_GPUs=1, cpu=False)


# ---------------------------------------------------------------------------------------------------------
class SPEINet(nn.Module):
    """Same signature as reference model/speinet.py:29-31; ``forward`` as :150-168."""

    def __init__(self, in_channels=3, n_sequence=3, out_channels=3, n_resblock=3, n_feat=32,
                 load_flow_net=False, load_recons_net=False, flow_pretrain_fn='', recons_pretrain_fn='',
                 is_mask_filter=False, device='cuda', args=None):
        super().__init__()
        if args is None:
            args = default_args()
        if in_channels != 3 or out_channels != 3 or n_feat != 32 or n_sequence != 3:
            # n_sequence == 1 (reference model/speinet.py:87-89) cannot run in the reference either: its forward tests frame 3 and
            # reads the sharp frame at index n_sequence + 1 of an [B, n_sequence + 2, ...] input (:71, :124).  The single-frame
            # form that does run is model/swint.py with n_sequence = 1 -> speinet_amd.swint.
            raise ValueError("speinet_amd builds the published configuration: 3 colours, n_feat=32, n_sequence=3 "
                             "(n_sequence 1 / 5: see speinet_amd.swint)")
        if args.window_size != 5 or args.embed_dim != 256 or any(h != 8 for h in args.num_heads):
            raise ValueError("speinet_amd kernels are built for window 5, embed_dim 256, 8 heads")
        if getattr(args, "resi_connection", "1conv") != "1conv":
            raise ValueError("only resi_connection='1conv' is built")
        self.n_sequence = n_sequence
        self.device = device
        self.is_mask_filter = is_mask_filter
        self.cfg = SimpleNamespace(n_sequence=n_sequence, n_feat=n_feat, n_resblock=n_resblock, window_size=args.window_size,
                                   embed_dim=args.embed_dim, depths=tuple(args.depths), num_heads=tuple(args.num_heads),
                                   mlp_ratio=args.mlp_ratio, rgb_range=float(args.rgb_range), patch_size=args.patch_size)
        self.swin = _SwinIR(n_feat * 4, args.patch_size // 4, args.window_size, list(args.depths), args.embed_dim,
                            list(args.num_heads), args.mlp_ratio)
        self.recons_net = _Recons(in_channels, out_channels, n_resblock, n_feat)
        self.SearchTransfer = _Transfer(n_feat)
        self.SelfTransfer = _Transfer(n_feat)
        nf = n_feat
        self.conv_lv1 = nn.Conv2d(nf * 2, nf, 1)
        self.conv_lv2 = nn.Conv2d(nf * 4, nf * 2, 1)
        self.conv_lv3 = nn.Conv2d(nf * 8, nf * 4, 1)
        self.fusion = nn.Conv2d(nf * 4 * n_sequence, nf * 4, 1)
        self.connect = nn.Conv2d(nf * 8, nf * 4, 1)
        self.search3 = nn.Conv2d(nf * 2, nf * 2, 3, 1, 1)
        self.search2 = nn.Conv2d(nf * 4, nf * 2, 1)
        self.search1 = nn.Conv2d(nf * 4, nf * 2, 1)
        self.search43 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.search33 = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.search23 = nn.Conv2d(nf * 4, nf, 1)
        self.search13 = nn.Conv2d(nf * 2, nf, 1)
        if load_recons_net:
            self.recons_net.load_state_dict(torch.load(recons_pretrain_fn, weights_only=True))
        self._packed = {}            # device -> packed weights (speinet_amd/pack.py), rebuilt after invalidate_packed()
        self._generation = 0
        # arithmetic of the GEMM-shaped kernels: "f32" (exact, PSNR parity), "bf16x3" (f32-grade, 5x cheaper) or
        # "bf16" (throughput config); correlation: "bf16x3" | "bf16" | "bf16r" (bf16 + exact re-score of near-ties);
        # see speinet_amd/ops.py.  Not part of the reference signature; read once per forward call into an ops.Ctx.
        self.precision = os.environ.get("SPEINET_PRECISION", "f32")
        self.corr_precision = os.environ.get("SPEINET_CORR_PRECISION", "bf16x3")
        self.use_graph = os.environ.get("SPEINET_GRAPH", "0") == "1"     # hipGraph replay of a whole frame
        self.streams = int(os.environ.get("SPEINET_STREAMS", "1"))        # HIP streams for the independent frame branches
        self.knobs = {}              # extra ops.Ctx fields (parity ablations, tools/ablate_parity.py)
        self.train_precision = os.environ.get("SPEINET_TRAIN_PRECISION", "f32")   # GEMMs of the training graph: "f32" | "bf16x3" | "bf16" (train.py)
        self._graphs = {}
        self._graph_devices = set()  # devices that hold captured graphs (synchronised before the graphs are dropped)
        self._side_streams = {}      # (device index, n) -> side streams, owned by this model
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.invalidate_packed())

    # ---- weight packing cache -----------------------------------------------------------------------
    def invalidate_packed(self) -> None:
        """Drop the packed weights and captured graphs.  Called automatically after `load_state_dict` and after
        `.to()` / `.cuda()` / `.float()` (`_apply`); call it yourself after editing parameters in place
        (`p.data.mul_()`, an optimizer step): in-place edits are invisible to the module.

        A replay of one of the graphs, or an eager launch on the prefetch / side streams, may still be reading the packed weights
        and the graphs' static buffers by raw pointer (they were allocated on the main stream, the caching allocator would hand
        them to the next main-stream allocation): every device that holds any is synchronised before they are dropped."""
        if self._packed or self._graphs:
            for key in {str(k) for k in self._packed} | {str(d) for d in self._graph_devices}:
                torch.cuda.synchronize(torch.device(key))
        self._packed = {}
        self._graphs = {}
        self._graph_devices = set()
        self._generation += 1
        from .train import drop_split_cache
        drop_split_cache(self)           # the training graph's packed bf16 halves, kept on the parameters (train._split_frags)

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self.invalidate_packed()
        return out

    def _pack(self, device):
        device = torch.device(device)
        key = str(device)
        if key not in self._packed:
            self._packed[key] = pack.pack_all(self.state_dict(), self.cfg, device)
        return self._packed[key]

    def _ctx(self, device, profile=None, capture=None) -> ops.Ctx:
        return ops.Ctx(self.precision, self.corr_precision, device=device, profile=profile, capture=capture, **self.knobs)

    def _sides(self, device) -> list:
        return engine.side_streams(self, device)

    def _mode_key(self, device):
        return (self.precision, self.corr_precision, int(self.streams), str(device), self._generation, repr(sorted(self.knobs.items())))

    def _check_input(self, x: torch.Tensor, batch1: bool = False) -> None:
        if x.dim() != 5 or x.shape[1] != self.n_sequence + 2 or x.shape[2] != 3 or (batch1 and x.shape[0] != 1):
            raise ValueError(f"expected [{'1' if batch1 else 'B'},{self.n_sequence + 2},3,H,W], got {tuple(x.shape)}")
        h, w = x.shape[-2:]
        if h % 20 or w % 20:
            raise ValueError(f"H and W must be multiples of 20 (two stride-2 stages, then 5x5 windows); got {h}x{w}")
        if not x.is_cuda:
            raise RuntimeError("speinet_amd.SPEINet runs on MI355X only (HIP kernels); there is no CPU path")

    def _route(self, ctx: ops.Ctx, x: torch.Tensor) -> list:
        """`_forwardx` (reference :70-73): True where frame 3 is identically zero.  One device reduction per
        sample, ONE host sync for the batch (the reference syncs twice through `.any()`)."""
        b = x.shape[0]
        flags = torch.empty(b, dtype=torch.int32, device=x.device)
        for i in range(b):
            ctx.any_nonzero(x[i, 3], flags[i:i + 1])
        return [v == 0 for v in flags.tolist()]

    def forward(self, x: torch.Tensor, routing: Optional[Sequence[bool]] = None, profile: Optional[dict] = None,
                capture: Optional[dict] = None, drop_path_scales: Optional[dict] = None) -> torch.Tensor:
        """x [B, n_sequence+2, 3, H, W] fp32 in [0,1] -> [B, 3, H, W] (unclamped).

        ``routing`` (optional, beyond the reference signature): per-sample "frame 3 is all zero" decisions when the
        caller already knows them (the harness zeroes the frame itself), which removes the host sync.
        ``profile`` (optional): {op name: []} filled with HIP event pairs around those ops (eager launches only).
        ``capture`` (optional): a dict that receives SearchTransfer's arg-max / weight map (parity tests; eager only).
        ``drop_path_scales`` (optional, train() mode): the DropPath factors (`train.speinet_drop_path_scales`); drawn from torch's
        CPU generator in the reference's order when not given.
        """
        self._check_input(x)
        if _wants_autograd(self, x):
            # the differentiable fp32 graph (HIP forward AND backward kernels, speinet_amd/train.py): train() mode runs the gates'
            # BatchNorm(1) on batch statistics and DropPath, as the reference module does under
            # trainer/trainer_swint_hsa_nsf.py:27-40; eval() with `autograd = True` (or an input that requires grad) is the same
            # graph with running statistics.  An optimizer step may follow either way: the packed inference weights are stale.
            from . import train
            self.invalidate_packed()
            return train.forward_speinet(self, x, scales=drop_path_scales)
        _lib.lib()
        h, w = x.shape[-2:]
        with torch.cuda.device(x.device):           # kernels launch on the CURRENT device: make it the tensor's
            ctx = self._ctx(x.device, profile, capture)
            x = x.contiguous().float()
            P = self._pack(x.device)
            zero_ref = list(routing) if routing is not None else self._route(ctx, x)
            if self.use_graph and capture is None:
                return self._forward_graph(ctx, x, P, zero_ref, profile)
            out = torch.empty(x.shape[0], 3, h, w, device=x.device, dtype=torch.float32)
            sides = self._sides(x.device)
            for plan in self._steps(ctx, x, P, zero_ref, out, sides):
                plan.launch()
            return out

    def _steps(self, ctx: ops.Ctx, x, P, zero_ref, out, sides):
        """The batch as a generator of prepared correlation launches, one per sample: the encoder passes of ALL samples batched per layer
        where the mode allows it (engine.forward_batch_steps), else one sample after the other."""
        if ctx.for_stage("enc").batched_available():
            yield from engine.forward_batch_steps(ctx, x, P, self.n_sequence, list(zero_ref), out, sides)
        else:
            for b in range(x.shape[0]):
                yield from engine.forward_sample_steps(ctx, x[b], P, self.n_sequence, not zero_ref[b], out[b], sides)

    def forward_window(self, x: torch.Tensor, keys: Sequence, cache: "EncoderCache", zero_ref: bool) -> torch.Tensor:
        """One window of a clip with cross-window reuse of the per-frame encoder work (not part of the
        reference API).  x [1, n_sequence+2, 3, H, W]; keys: one hashable id per frame of x (e.g. its file name) — frames
        with equal ids MUST have equal pixels; cache: an `EncoderCache` the caller keeps per clip.  Bit-identical to
        `forward(x)`: the same kernels run on the same operands, only less often.  The encoder passes that are missing
        run eagerly; everything after them replays as one hipGraph when `use_graph` is set."""
        self._check_input(x, batch1=True)
        if len(keys) != self.n_sequence + 2:
            raise ValueError(f"expected {self.n_sequence + 2} keys")
        _lib.lib()
        with torch.cuda.device(x.device):
            return self._forward_window(x, keys, cache, zero_ref)

    def _prefetch_stream(self, device) -> "torch.cuda.Stream":
        return engine.model_streams(self, ("prefetch", torch.device(device).index), device, 1)[0]

    def prefetch_window(self, x: torch.Tensor, keys: Sequence, cache: "EncoderCache", zero_ref: bool) -> None:
        """Start the encoder passes a later `forward_window(x, keys, cache, zero_ref)` will need, on the prefetch stream: called for
        window k+1 BEFORE `forward_window` of window k, they run under window k's fuse-and-decode graph (same kernels, same operands:
        the frames do not change)."""
        self._check_input(x, batch1=True)
        _lib.lib()
        with torch.cuda.device(x.device):
            self._forward_window(x, keys, cache, zero_ref, pieces_only=True)

    def _forward_window(self, x, keys, cache, zero_ref, pieces_only: bool = False):
        h, w = x.shape[-2:]
        ctx = self._ctx(x.device)
        x = x.contiguous().float()
        P = self._pack(x.device)
        sides = self._sides(x.device)
        n, mid = self.n_sequence, self.n_sequence // 2
        tag = (h, w) + self._mode_key(x.device)

        # the per-frame encoder pieces: eager launches, or (use_graph) one captured graph per piece and frame shape — a new
        # frame then costs three replays instead of ~150 launches from Python (the harness was host-bound on them)
        G = self._graphed if self.use_graph else (lambda name, ins, fn: fn(*ins))

        # The pieces run on a stream of their own (always the same one: their captured graphs share static buffers).  A caller that
        # knows the next window (`prefetch_window`) gets that window's encoder passes UNDER the current window's fuse-and-decode
        # graph: every cache entry carries the event recorded on the prefetch stream when it was produced, and the main stream waits
        # for the events of the entries THIS window consumes only — not for the prefetch stream's tail, which by then holds the next
        # window's passes (round 2 waited for the tail: fuse(k-1), enc(k+1), fuse(k) ran strictly in turn).
        main = torch.cuda.current_stream(x.device)
        pf = self._prefetch_stream(x.device)
        pf.wait_stream(main)                         # x is ready (the caller assembled it on the main stream)
        x.record_stream(pf)
        used = []                                    # (value, event) of every cache entry this window reads

        def piece(key, make):
            hit = cache.get(key)
            if hit is None:
                v = make()
                ev = torch.cuda.Event()
                ev.record(pf)
                hit = cache.put(key, (v, ev))
            used.append(hit)
            return hit[0]

        def raw(i):
            return piece((tag, keys[i], "raw"), lambda: G(("raw", h, w), [x[0, i]], lambda fr: [engine.encode_raw(ctx, fr, P)])[0])

        def summed(i, iters):
            return piece((tag, keys[i], iters),
                         lambda: G(("sum", iters, h, w), [x[0, i], raw(i)], lambda fr, e: [engine.encode_sum(ctx, fr, iters, e, P)])[0])

        with torch.cuda.stream(pf):
            if ctx.for_stage("enc").batched_available():
                f_mid, feats, lv = self._window_pieces_batched(ctx, x, keys, cache, zero_ref, P, tag, G, pf, used)
            else:
                f_mid = summed(mid, 5)
                feats = [summed(i, 1) for i in range(n) if i != mid]
                lv = None
                if not zero_ref:
                    lv = piece((tag, keys[n + 1], "ref"),
                               lambda: tuple(G(("pyr", h, w), [x[0, n + 1]], lambda fr: list(engine.reference_pyramid(ctx, fr, P)))))
        for f in [f_mid] + feats + list(lv or ()):   # produced on `pf`, consumed (and possibly freed by the cache) under `main`
            f.t.record_stream(main)
        if pieces_only:
            return None
        for _, ev in used:
            main.wait_event(ev)
        out = torch.empty(1, 3, h, w, device=x.device, dtype=torch.float32)
        if not self.use_graph:
            engine.fuse_and_decode(ctx, f_mid, feats, lv, P, n, out[0], sides)
            return out
        # one captured instance per launch stream: a caller that keeps several windows in flight (inference.py) replays from several
        # streams, and each needs its own static buffers
        gkey = ("window", h, w, bool(zero_ref), torch.cuda.current_stream(x.device).cuda_stream) + self._mode_key(x.device)
        g = self._graphs.get(gkey)
        if g is None:
            clone = lambda f: ops.FMap(f.t.clone(), f.H, f.W, f.C)
            s_mid, s_feats = clone(f_mid), [clone(f) for f in feats]
            s_lv = tuple(clone(f) for f in lv) if lv is not None else None
            s_out = torch.empty_like(out)
            g = self._capture(gkey, x.device, ([s_mid] + s_feats + list(s_lv or ()), s_out),
                              lambda: engine.fuse_and_decode_steps(ctx, s_mid, s_feats, s_lv, P, n, s_out[0], sides))
        s_in, s_out = g.statics
        for d, f in zip(s_in, [f_mid] + feats + list(lv or ())):
            d.t.copy_(f.t)
        g.replay()
        return s_out.clone()

    def _window_pieces_batched(self, ctx, x, keys, cache, zero_ref, P, tag, G, pf, used):
        """The encoder passes a window still misses — enc(frame), enc(RL_1(frame)), enc(RL_5(frame)), the sharp frame's pyramid — as ONE
        batched pass (engine.enc_batched: one launch per layer for all of them; per map bit-identical to a pass of its own and to the
        passes `forward` batches), then the sums enc(RL(frame)) + enc(frame).  Steady state of a clip: three maps per window (the new
        frame raw and RL-1, the new middle frame RL-5), four when a new sharp frame arrives.  Cache keys, hit / miss accounting and the
        results are those of the one-pass-at-a-time form."""
        from .ops import FMap
        h, w = x.shape[-2:]
        h3, w3 = h // 4, w // 4
        n, mid = self.n_sequence, self.n_sequence // 2
        plan, have = [], {}          # plan: (cache key, frame index, RL iterations or 0, keep the three levels)

        def lookup(key):
            if key in have:
                return have[key]
            hit = cache.get(key)
            if hit is not None:
                used.append(hit)
                have[key] = hit[0]
            return have.get(key)

        sums = [(mid, 5)] + [(i, 1) for i in range(n) if i != mid]
        for i, it in sums:
            if lookup((tag, keys[i], it)) is None:
                if lookup((tag, keys[i], "raw")) is None and not any(pk == (tag, keys[i], "raw") for pk, *_ in plan):
                    plan.append(((tag, keys[i], "raw"), i, 0, False))
                if not any(pk == (tag, keys[i], ("rl", it)) for pk, *_ in plan):
                    plan.append(((tag, keys[i], ("rl", it)), i, it, False))
        if not zero_ref and lookup((tag, keys[n + 1], "ref")) is None:
            plan.append(((tag, keys[n + 1], "ref"), n + 1, 0, True))
        if plan:
            sig = tuple((it, lv_) for _, _, it, lv_ in plan)

            def run(*fr):
                maps = [ctx.rl_prior(f, it, 0.01) if it else f for f, (_, _, it, _) in zip(fr, plan)]
                lv1, lv2, lv3 = engine.enc_batched(ctx, maps, P)
                outs = []
                for j, (_, _, _, levels) in enumerate(plan):
                    outs += [lv1.map(j), lv2.map(j), lv3.map(j)] if levels else [lv3.map(j)]
                return outs

            outs = iter(G(("pieces", sig, h, w), [x[0, i] for _, i, _, _ in plan], run))
            ev = torch.cuda.Event()
            made = {}
            for pk, _, _, levels in plan:
                made[pk] = tuple(next(outs) for _ in range(3)) if levels else next(outs)
            for i, it in sums:                         # enc(RL_it(frame)) + enc(frame): the operand order of engine.forward_batch_steps
                ks = (tag, keys[i], it)
                if ks not in have:
                    rl = made[(tag, keys[i], ("rl", it))]
                    raw = made.get((tag, keys[i], "raw"))
                    raw = raw if raw is not None else have[(tag, keys[i], "raw")]
                    made[ks] = FMap(ctx.add(rl.t, raw.t), h3, w3, 128)
            ev.record(pf)
            for pk, v in made.items():
                if not (isinstance(pk[2], tuple) and pk[2][0] == "rl"):      # the bare enc(RL(frame)) maps are not reused
                    hit = cache.put(pk, (v, ev))
                    used.append(hit)
                    have[pk] = v
        f_mid = have[(tag, keys[mid], 5)]
        feats = [have[(tag, keys[i], 1)] for i in range(n) if i != mid]
        lv = None if zero_ref else have[(tag, keys[n + 1], "ref")]
        return f_mid, feats, lv

    GRAPH_LIMIT = 24                   # captured instances a model keeps (frame, window and piece graphs together)

    def _trim_graphs(self) -> None:
        if len(self._graphs) >= self.GRAPH_LIMIT:
            torch.cuda.synchronize()           # a replay of one of them may still be running (other stream, earlier window)
            self._graphs.clear()

    def _capture(self, key: tuple, device, statics, run) -> "_Graphed":
        """Capture `run()` — a piece of the forward pass on the caller's static buffers `statics` — as hipGraphs and keep it as
        `self._graphs[key]`.  `run` is a plain function that returns its outputs, or a generator that yields prepared correlation launches
        (ops.CorrPlan) and may return outputs.  n plans give n + 1 graph segments in one memory pool, [g_0] plan_0 [g_1] ... plan_{n-1} [g_n]:
        the plans are launched directly between the replays, so a caller can bracket the path's dominant kernel with HIP events on the
        launch stream (`profile`, bench.py) inside the very run it times."""
        def steps():
            r = run()
            return (yield from r) if inspect.isgenerator(r) else r

        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):           # warm-up off the capture: sets kernel attributes, fills the allocator
            for plan in steps():
                plan.launch()
        torch.cuda.current_stream().wait_stream(side)
        segs, pool, it, result = [], None, steps(), None
        while True:
            gseg = torch.cuda.CUDAGraph()
            plan = None
            with torch.cuda.graph(gseg, pool=pool):
                try:
                    plan = next(it)
                except StopIteration as end:
                    result = end.value
            pool = gseg.pool()
            segs.append((gseg, plan))
            if plan is None:
                break
            plan.launch()                       # once, eagerly: the next segment is captured behind real data
        self._trim_graphs()
        self._graph_devices.add(str(device))
        g = self._graphs[key] = _Graphed(segs, statics, result)
        return g

    def _graphed(self, name: tuple, inputs: list, fn) -> list:
        """`fn(*inputs) -> [FMap, ...]` through a hipGraph captured once per (name, mode): inputs (tensors or FMaps) are copied
        into the graph's static buffers, the outputs are returned as fresh copies (they go into the caller's cache)."""
        FMap = ops.FMap
        buf = lambda v: v if torch.is_tensor(v) else v.t
        dev = buf(inputs[0]).device
        key = ("piece",) + name + self._mode_key(dev)
        g = self._graphs.get(key)
        if g is None:
            s_in = [v.clone() if torch.is_tensor(v) else FMap(v.t.clone(), v.H, v.W, v.C, v.off) for v in inputs]
            g = self._capture(key, dev, s_in, lambda: fn(*s_in))
        for d, v in zip(g.statics, inputs):
            buf(d).copy_(buf(v))
        return [FMap(f.t.clone(), f.H, f.W, f.C, f.off) for f in g.replay()]

    def _forward_graph(self, ctx: ops.Ctx, x: torch.Tensor, P: dict, zero_ref: list, profile: Optional[dict] = None) -> torch.Tensor:
        """Replay the ~1500 launches of a frame as hipGraphs (captured once per shape / routing / precision): the per-launch
        host cost (ctypes + hipLaunch, ~10 us each) otherwise leaves the GPU idle ~15 % of a frame.  A batch of B frames is B + 1 graph
        segments around the B correlation arg-max launches (`_capture`)."""
        # one captured instance per launch stream: a caller that keeps two frames in flight (bench.py --inflight 2: frame i + 1's
        # encoder passes under frame i's correlation / decoder) calls forward from two streams, and each needs its own static buffers
        key = (tuple(x.shape), tuple(zero_ref), torch.cuda.current_stream(x.device).cuda_stream) + self._mode_key(x.device)
        g = self._graphs.get(key)
        if g is None:
            static_x = x.clone()
            static_out = torch.empty(x.shape[0], 3, x.shape[-2], x.shape[-1], device=x.device, dtype=torch.float32)
            sides, cctx = self._sides(x.device), ctx.replace(profile=None)
            g = self._capture(key, x.device, (static_x, static_out), lambda: self._steps(cctx, static_x, P, zero_ref, static_out, sides))
        static_x, static_out = g.statics
        static_x.copy_(x)
        g.replay(profile)
        return static_out.clone()


class _Graphed:
    """One captured instance (`SPEINet._capture`): the graph segments, each with the correlation launch that follows it (None after the
    last), the caller's static buffers and what the captured piece returned."""
    __slots__ = ("segs", "statics", "result")

    def __init__(self, segs, statics, result):
        self.segs, self.statics, self.result = segs, statics, result

    def replay(self, profile: Optional[dict] = None):
        for gseg, plan in self.segs:
            gseg.replay()
            if plan is not None:
                plan.launch(profile)
        return self.result


def _wants_autograd(model: nn.Module, x: torch.Tensor) -> bool:
    """Which graph a `forward` call builds.  train() mode: always the differentiable one (the reference trainer's step).  eval():
    only when the caller asks for gradients — the input requires grad, or `model.autograd = True` — and autograd is recording;
    a plain eval() call outside `torch.no_grad()` (the reference's trainers do evaluate under no_grad, trainer_swint_hsa_nsf.py:57)
    stays on the inference path in the model's `precision`, with a warning per call site unless `model.autograd = False` says it is meant: saving every activation of a 720p frame for a
    backward nobody asked for is what round 2 did there."""
    if model.training:
        return True
    if not torch.is_grad_enabled():
        return False
    want = getattr(model, "autograd", None)           # None: not stated; True / False: the caller's explicit choice
    if x.requires_grad or want:
        return True
    if want is None and any(p.requires_grad for p in model.parameters()):
        import warnings                               # once per call site (Python's default filter), not once per model
        warnings.warn("speinet_amd: eval()-mode forward with autograd recording runs the INFERENCE kernels (no graph is built, unlike the "
                      "reference nn.Module); set `model.autograd = True` to differentiate (or pass an input that requires grad, or call "
                      "model.train()), `model.autograd = False` to silence this", stacklevel=4)
    return False


class EncoderCache:
    """Per-clip LRU store of per-frame encoder results for `SPEINet.forward_window` (device tensors; a 720p entry is
    30 MB, a reference pyramid 207 MB)."""

    def __init__(self, capacity: int = 24):
        import collections
        self.capacity = capacity
        self.items = collections.OrderedDict()
        self.hits = self.misses = 0

    def get(self, key):
        v = self.items.get(key)
        if v is None:
            self.misses += 1
            return None
        self.items.move_to_end(key)
        self.hits += 1
        return v

    def put(self, key, value):
        self.items[key] = value
        self.items.move_to_end(key)
        while len(self.items) > self.capacity:
            self.items.popitem(last=False)
        return value

    def clear(self):
        self.items.clear()


def make_model(args):
    """reference model/speinet.py:18-26."""
    device = 'cpu' if getattr(args, "cpu", False) else 'cuda'
    return SPEINet(in_channels=args.n_colors, n_sequence=args.n_sequence, out_channels=args.n_colors,
                   n_resblock=args.n_resblock, n_feat=args.n_feat, load_recons_net=False, recons_pretrain_fn='',
                   is_mask_filter=True, device=device, args=args)
