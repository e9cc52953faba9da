"""The training-step kernels at the shapes one training step runs them at, against float64 evaluated on the device.

The op-level tests of test_gpu_train.py, test_gpu_grad.py and test_gpu_train_bf16.py run on toy maps (at most 60x40 at batch 3), where
the weight gradients are cut into ~10 pixel chunks and LayerNorm's backward has about one row per wave.  The step stacks its encoder
passes into one batch (`train.encoder(..., groups=n)`), so at the benchmark's crop step (swint: batch 20 of 200x200, n_sequence 3;
speinet: batch 8, samples 3 and 7 without a reference frame, as `bench.py --train` builds them) the same kernels run 255-chunk weight
gradients, 9 400 pixels per fp32 wave accumulator, 49 LayerNorm rows per wave and 4 000 attention windows per launch.

  1. TABLE: every distinct op call of one training step of each model, under the layer it stands for.  test_shape_table_covers_the_step
     runs both models forward + backward in all three train precisions, records every call (and the HIP entries it reached) and
     asserts that the recorded set IS the table: a model change cannot leave a shape untested.
  2. The regimes the table reaches (chunk counts, pixels per wave, rows per wave), from Python mirrors of the launchers' plans whose
     constants are read from the HIP source (test_mirrored_plan_constants).
  3. One case per table entry and precision: forward and every gradient against float64 on the device (per-tap shifted GEMMs for the
     convolutions), at the bounds of the toy-shape tests; each case asserts the HIP route it ran.
  4. Sensitivity: each weight-gradient case computes, from the float64 reference, the error ONE dropped pixel chunk (the kernel's own
     chunk plan) or ONE dropped tap row would cause, and asserts its bound sits 10x below that; the same for one LayerNorm block
     partial and one window's relative-position-bias partial.
  5. Without the gpu mark: the per-tap references against F.conv2d / F.conv_transpose2d autograd on the CPU, and the chunk plans.
"""
import math
import os
import re
import time
import zlib

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = ("f32", "bf16x3", "bf16")

# bounds of the toy-shape tests this file scales up
TOL = {"f32": (1e-5, 2e-5), "bf16x3": (3e-5, 1e-4)}          # test_gpu_grad.TOL: GEMM forward, gradients (relative L2)
CONTRACT, ATTN, INFER, CONTROL = 2e-5, 1e-3, 1.5e-2, 1e-5    # test_gpu_train_bf16: rounded-operand contract (max-abs relative)
LN_TOL, GELU_TOL, ROWSCALE_TOL = (2e-6, 5e-6), (2e-6, 2e-6), (1e-6, 3e-6)   # test_gpu_train
ATTN_TOL, SEARCH_TOL, BICUBIC_TOL = (3e-6, 1e-5), (3e-6, 1e-6, 2e-5), (2e-6, 3e-6)
CONV_IN_TOL = (1e-5, 2e-5)                                    # test_gpu_grad.test_conv_in_backward
GATE_TOL = (2e-6, 5e-6, 2e-5)                                 # test_gpu_grad.test_gated_sum_backward_with_tied_maxima
MARGIN = 10.0                                                 # a dropped chunk / tap row / partial must exceed the bound this often


def E(model, layer, op, **shape):
    return (model, layer, op, shape)


# ---- 1. the shape table -------------------------------------------------------------------------------------------------------------
# speinet: "ref" = the samples with a sharp reference (_forwardbs: 6 samples, 7 encoder passes each, SearchTransfer), "noref" = the two
# without (_forwardb: 6 passes each, SelfTransfer).  Row counts M are token / pixel rows of the stacked batch.
TABLE = [
    # ---- swint ----
    E('swint', 'recons_net.inBlock.0', '_ConvIn', B=60, H=200, W=200, K=3, N=32),
    E('swint', 'recons_net.encoder_second.0', '_Conv2d', B=60, H=100, W=100, K=64, N=128, ksize=5, stride=2, relu=True, residual=False),
    E('swint', 'recons_net.encoder_first.1-2.main.1', '_Conv2d', B=60, H=100, W=100, K=64, N=64, ksize=5, stride=1, relu=False, residual=False),
    E('swint', 'recons_net.encoder_first.1-2.main.0 (+relu)', '_Conv2d', B=60, H=100, W=100, K=64, N=64, ksize=5, stride=1, relu=True, residual=False),
    E('swint', 'recons_net.inBlock.1-2.main.1', '_Conv2d', B=60, H=200, W=200, K=32, N=32, ksize=5, stride=1, relu=False, residual=False),
    E('swint', 'recons_net.inBlock.1-2.main.0 (+relu)', '_Conv2d', B=60, H=200, W=200, K=32, N=32, ksize=5, stride=1, relu=True, residual=False),
    E('swint', 'recons_net.encoder_first.0', '_Conv2d', B=60, H=200, W=200, K=32, N=64, ksize=5, stride=2, relu=True, residual=False),
    E('swint', 'recons_net.encoder_second.1-2.main.1', '_Conv2d', B=60, H=50, W=50, K=128, N=128, ksize=5, stride=1, relu=False, residual=False),
    E('swint', 'recons_net.encoder_second.1-2.main.0 (+relu)', '_Conv2d', B=60, H=50, W=50, K=128, N=128, ksize=5, stride=1, relu=True, residual=False),
    E('swint', 'swin.conv_first', '_Conv2d', B=40, H=50, W=50, K=128, N=256, ksize=3, stride=1, relu=False, residual=False),
    E('swint', 'swin.conv_last', '_Conv2d', B=40, H=50, W=50, K=256, N=128, ksize=3, stride=1, relu=False, residual=True),
    E('swint', 'swin.layers.*.conv + conv_after_body', '_Conv2d', B=40, H=50, W=50, K=256, N=256, ksize=3, stride=1, relu=False, residual=True),
    E('swint', 'recons_net.decoder_first.0-1.main.1', '_Conv2d', B=20, H=100, W=100, K=64, N=64, ksize=5, stride=1, relu=False, residual=False),
    E('swint', 'recons_net.decoder_first.0-1.main.0 (+relu)', '_Conv2d', B=20, H=100, W=100, K=64, N=64, ksize=5, stride=1, relu=True, residual=False),
    E('swint', 'recons_net.outBlock.0-1.main.1 + outBlock.2 (3 outputs padded to 32)', '_Conv2d', B=20, H=200, W=200, K=32, N=32, ksize=5, stride=1, relu=False, residual=False),
    E('swint', 'recons_net.outBlock.0-1.main.0 (+relu)', '_Conv2d', B=20, H=200, W=200, K=32, N=32, ksize=5, stride=1, relu=True, residual=False),
    E('swint', 'recons_net.decoder_second.0-1.main.1', '_Conv2d', B=20, H=50, W=50, K=128, N=128, ksize=5, stride=1, relu=False, residual=False),
    E('swint', 'recons_net.decoder_second.0-1.main.0 (+relu)', '_Conv2d', B=20, H=50, W=50, K=128, N=128, ksize=5, stride=1, relu=True, residual=False),
    E('swint', 'recons_net.encoder_second.*.gates', '_GatedSum', C=128, B=60, H=50, W=50, groups=3),
    E('swint', 'recons_net.inBlock.*.gates', '_GatedSum', C=32, B=60, H=200, W=200, groups=3),
    E('swint', 'recons_net.encoder_first.*.gates', '_GatedSum', C=64, B=60, H=100, W=100, groups=3),
    E('swint', 'recons_net.decoder_second.*.gates', '_GatedSum', C=128, B=20, H=50, W=50, groups=1),
    E('swint', 'recons_net.outBlock.*.gates', '_GatedSum', C=32, B=20, H=200, W=200, groups=1),
    E('swint', 'recons_net.decoder_first.*.gates', '_GatedSum', C=64, B=20, H=100, W=100, groups=1),
    E('swint', 'recons_net.decoder_first.-1', '_ConvT2d', B=20, H=100, W=100, K=64, N=32),
    E('swint', 'recons_net.decoder_second.-1', '_ConvT2d', B=20, H=50, W=50, K=128, N=64),
    E('swint', 'swin.patch_embed.norm + norm1 + norm2 + norm', '_LayerNorm', M=100000),
    E('swint', 'swin.*.attn.qkv_y', '_Linear', M=100000, K=256, N=256, residual=False, rowscale=False),
    E('swint', 'swin.*.attn.proj (block 0: no DropPath)', '_Linear', M=100000, K=256, N=256, residual=True, rowscale=False),
    E('swint', 'swin.*.attn.proj', '_Linear', M=100000, K=256, N=256, residual=True, rowscale=True),
    E('swint', 'swin.*.attn.qkv_x + mlp.fc1', '_Linear', M=100000, K=256, N=512, residual=False, rowscale=False),
    E('swint', 'swin.*.mlp.fc2 (block 0: no DropPath)', '_Linear', M=100000, K=512, N=256, residual=True, rowscale=False),
    E('swint', 'swin.*.mlp.fc2', '_Linear', M=100000, K=512, N=256, residual=True, rowscale=True),
    E('swint', 'conv', '_Linear', M=50000, K=384, N=128, residual=False, rowscale=False),
    E('swint', 'swin.*.mlp.act', '_Gelu', M=100000, C=512),
    E('swint', 'swin.*.attn (shift 0)', '_WindowAttention', B=40, H=50, W=50, shift=0),
    E('swint', 'swin.*.attn (shift 2)', '_WindowAttention', B=40, H=50, W=50, shift=2),
    # ---- speinet ----
    E('speinet', 'ref: recons_net.inBlock.0', '_ConvIn', B=42, H=200, W=200, K=3, N=32),
    E('speinet', 'noref: recons_net.inBlock.0', '_ConvIn', B=12, H=200, W=200, K=3, N=32),
    E('speinet', 'ref: recons_net.encoder_second.0', '_Conv2d', B=42, H=100, W=100, K=64, N=128, ksize=5, stride=2, relu=True, residual=False),
    E('speinet', 'ref: recons_net.encoder_first.1-2.main.1', '_Conv2d', B=42, H=100, W=100, K=64, N=64, ksize=5, stride=1, relu=False, residual=False),
    E('speinet', 'ref: recons_net.encoder_first.1-2.main.0 (+relu)', '_Conv2d', B=42, H=100, W=100, K=64, N=64, ksize=5, stride=1, relu=True, residual=False),
    E('speinet', 'ref: recons_net.inBlock.1-2.main.1', '_Conv2d', B=42, H=200, W=200, K=32, N=32, ksize=5, stride=1, relu=False, residual=False),
    E('speinet', 'ref: recons_net.inBlock.1-2.main.0 (+relu)', '_Conv2d', B=42, H=200, W=200, K=32, N=32, ksize=5, stride=1, relu=True, residual=False),
    E('speinet', 'ref: recons_net.encoder_first.0', '_Conv2d', B=42, H=200, W=200, K=32, N=64, ksize=5, stride=2, relu=True, residual=False),
    E('speinet', 'ref: recons_net.encoder_second.1-2.main.1', '_Conv2d', B=42, H=50, W=50, K=128, N=128, ksize=5, stride=1, relu=False, residual=False),
    E('speinet', 'ref: recons_net.encoder_second.1-2.main.0 (+relu)', '_Conv2d', B=42, H=50, W=50, K=128, N=128, ksize=5, stride=1, relu=True, residual=False),
    E('speinet', 'noref: recons_net.encoder_second.0', '_Conv2d', B=12, H=100, W=100, K=64, N=128, ksize=5, stride=2, relu=True, residual=False),
    E('speinet', 'noref: recons_net.encoder_first.1-2.main.1', '_Conv2d', B=12, H=100, W=100, K=64, N=64, ksize=5, stride=1, relu=False, residual=False),
    E('speinet', 'noref: recons_net.encoder_first.1-2.main.0 (+relu)', '_Conv2d', B=12, H=100, W=100, K=64, N=64, ksize=5, stride=1, relu=True, residual=False),
    E('speinet', 'noref: recons_net.inBlock.1-2.main.1', '_Conv2d', B=12, H=200, W=200, K=32, N=32, ksize=5, stride=1, relu=False, residual=False),
    E('speinet', 'noref: recons_net.inBlock.1-2.main.0 (+relu)', '_Conv2d', B=12, H=200, W=200, K=32, N=32, ksize=5, stride=1, relu=True, residual=False),
    E('speinet', 'noref: recons_net.encoder_first.0', '_Conv2d', B=12, H=200, W=200, K=32, N=64, ksize=5, stride=2, relu=True, residual=False),
    E('speinet', 'noref: recons_net.encoder_second.1-2.main.1', '_Conv2d', B=12, H=50, W=50, K=128, N=128, ksize=5, stride=1, relu=False, residual=False),
    E('speinet', 'noref: recons_net.encoder_second.1-2.main.0 (+relu)', '_Conv2d', B=12, H=50, W=50, K=128, N=128, ksize=5, stride=1, relu=True, residual=False),
    E('speinet', 'ref: swin.conv_first', '_Conv2d', B=12, H=50, W=50, K=128, N=256, ksize=3, stride=1, relu=False, residual=False),
    E('speinet', 'ref: swin.conv_last', '_Conv2d', B=12, H=50, W=50, K=256, N=128, ksize=3, stride=1, relu=False, residual=True),
    E('speinet', 'ref: swin.layers.*.conv + conv_after_body', '_Conv2d', B=12, H=50, W=50, K=256, N=256, ksize=3, stride=1, relu=False, residual=True),
    E('speinet', 'ref: search1 + search2 + SelfTransfer.search1', '_Conv2d', B=6, H=100, W=100, K=128, N=64, ksize=1, stride=1, relu=True, residual=False),
    E('speinet', 'ref: search3', '_Conv2d', B=6, H=100, W=100, K=64, N=64, ksize=3, stride=1, relu=True, residual=False),
    E('speinet', 'ref: recons_net.decoder_first.0-1.main.1', '_Conv2d', B=6, H=100, W=100, K=64, N=64, ksize=5, stride=1, relu=False, residual=False),
    E('speinet', 'ref: recons_net.decoder_first.0-1.main.0 (+relu)', '_Conv2d', B=6, H=100, W=100, K=64, N=64, ksize=5, stride=1, relu=True, residual=False),
    E('speinet', 'ref: search43 + search33 (32->32)', '_Conv2d', B=6, H=200, W=200, K=32, N=32, ksize=3, stride=1, relu=True, residual=False),
    E('speinet', 'ref: recons_net.outBlock.0-1.main.1 + outBlock.2 (3 outputs padded to 32)', '_Conv2d', B=6, H=200, W=200, K=32, N=32, ksize=5, stride=1, relu=False, residual=False),
    E('speinet', 'ref: recons_net.outBlock.0-1.main.0 (+relu)', '_Conv2d', B=6, H=200, W=200, K=32, N=32, ksize=5, stride=1, relu=True, residual=False),
    E('speinet', 'ref: search13 + SelfTransfer.search2', '_Conv2d', B=6, H=200, W=200, K=64, N=32, ksize=1, stride=1, relu=True, residual=False),
    E('speinet', 'ref: search33', '_Conv2d', B=6, H=200, W=200, K=64, N=32, ksize=3, stride=1, relu=True, residual=False),
    E('speinet', 'ref: recons_net.decoder_second.0-1.main.1', '_Conv2d', B=6, H=50, W=50, K=128, N=128, ksize=5, stride=1, relu=False, residual=False),
    E('speinet', 'ref: recons_net.decoder_second.0-1.main.0 (+relu)', '_Conv2d', B=6, H=50, W=50, K=128, N=128, ksize=5, stride=1, relu=True, residual=False),
    E('speinet', 'noref: swin.conv_first', '_Conv2d', B=4, H=50, W=50, K=128, N=256, ksize=3, stride=1, relu=False, residual=False),
    E('speinet', 'noref: swin.conv_last', '_Conv2d', B=4, H=50, W=50, K=256, N=128, ksize=3, stride=1, relu=False, residual=True),
    E('speinet', 'noref: swin.layers.*.conv + conv_after_body', '_Conv2d', B=4, H=50, W=50, K=256, N=256, ksize=3, stride=1, relu=False, residual=True),
    E('speinet', 'noref: search1 + search2 + SelfTransfer.search1', '_Conv2d', B=2, H=100, W=100, K=128, N=64, ksize=1, stride=1, relu=True, residual=False),
    E('speinet', 'noref: search3', '_Conv2d', B=2, H=100, W=100, K=64, N=64, ksize=3, stride=1, relu=True, residual=False),
    E('speinet', 'noref: recons_net.decoder_first.0-1.main.1', '_Conv2d', B=2, H=100, W=100, K=64, N=64, ksize=5, stride=1, relu=False, residual=False),
    E('speinet', 'noref: recons_net.decoder_first.0-1.main.0 (+relu)', '_Conv2d', B=2, H=100, W=100, K=64, N=64, ksize=5, stride=1, relu=True, residual=False),
    E('speinet', 'noref: search43 + search33 (32->32)', '_Conv2d', B=2, H=200, W=200, K=32, N=32, ksize=3, stride=1, relu=True, residual=False),
    E('speinet', 'noref: recons_net.outBlock.0-1.main.1 + outBlock.2 (3 outputs padded to 32)', '_Conv2d', B=2, H=200, W=200, K=32, N=32, ksize=5, stride=1, relu=False, residual=False),
    E('speinet', 'noref: recons_net.outBlock.0-1.main.0 (+relu)', '_Conv2d', B=2, H=200, W=200, K=32, N=32, ksize=5, stride=1, relu=True, residual=False),
    E('speinet', 'noref: search13 + SelfTransfer.search2', '_Conv2d', B=2, H=200, W=200, K=64, N=32, ksize=1, stride=1, relu=True, residual=False),
    E('speinet', 'noref: search33', '_Conv2d', B=2, H=200, W=200, K=64, N=32, ksize=3, stride=1, relu=True, residual=False),
    E('speinet', 'noref: recons_net.decoder_second.0-1.main.1', '_Conv2d', B=2, H=50, W=50, K=128, N=128, ksize=5, stride=1, relu=False, residual=False),
    E('speinet', 'noref: recons_net.decoder_second.0-1.main.0 (+relu)', '_Conv2d', B=2, H=50, W=50, K=128, N=128, ksize=5, stride=1, relu=True, residual=False),
    E('speinet', 'ref: recons_net.encoder_second.*.gates', '_GatedSum', C=128, B=42, H=50, W=50, groups=7),
    E('speinet', 'ref: recons_net.inBlock.*.gates', '_GatedSum', C=32, B=42, H=200, W=200, groups=7),
    E('speinet', 'ref: recons_net.encoder_first.*.gates', '_GatedSum', C=64, B=42, H=100, W=100, groups=7),
    E('speinet', 'noref: recons_net.encoder_second.*.gates', '_GatedSum', C=128, B=12, H=50, W=50, groups=6),
    E('speinet', 'noref: recons_net.inBlock.*.gates', '_GatedSum', C=32, B=12, H=200, W=200, groups=6),
    E('speinet', 'noref: recons_net.encoder_first.*.gates', '_GatedSum', C=64, B=12, H=100, W=100, groups=6),
    E('speinet', 'ref: recons_net.decoder_second.*.gates', '_GatedSum', C=128, B=6, H=50, W=50, groups=1),
    E('speinet', 'ref: recons_net.outBlock.*.gates', '_GatedSum', C=32, B=6, H=200, W=200, groups=1),
    E('speinet', 'ref: recons_net.decoder_first.*.gates', '_GatedSum', C=64, B=6, H=100, W=100, groups=1),
    E('speinet', 'noref: recons_net.decoder_second.*.gates', '_GatedSum', C=128, B=2, H=50, W=50, groups=1),
    E('speinet', 'noref: recons_net.outBlock.*.gates', '_GatedSum', C=32, B=2, H=200, W=200, groups=1),
    E('speinet', 'noref: recons_net.decoder_first.*.gates', '_GatedSum', C=64, B=2, H=100, W=100, groups=1),
    E('speinet', 'ref: recons_net.decoder_first.-1', '_ConvT2d', B=6, H=100, W=100, K=64, N=32),
    E('speinet', 'ref: recons_net.decoder_second.-1', '_ConvT2d', B=6, H=50, W=50, K=128, N=64),
    E('speinet', 'noref: recons_net.decoder_first.-1', '_ConvT2d', B=2, H=100, W=100, K=64, N=32),
    E('speinet', 'noref: recons_net.decoder_second.-1', '_ConvT2d', B=2, H=50, W=50, K=128, N=64),
    E('speinet', 'ref: swin.patch_embed.norm + norm1 + norm2 + norm', '_LayerNorm', M=30000),
    E('speinet', 'noref: swin.patch_embed.norm + norm1 + norm2 + norm', '_LayerNorm', M=10000),
    E('speinet', 'ref: conv_lv1', '_Linear', M=240000, K=64, N=32, residual=False, rowscale=False),
    E('speinet', 'noref: conv_lv1', '_Linear', M=80000, K=64, N=32, residual=False, rowscale=False),
    E('speinet', 'ref: conv_lv2', '_Linear', M=60000, K=128, N=64, residual=False, rowscale=False),
    E('speinet', 'ref: swin.*.attn.qkv_y', '_Linear', M=30000, K=256, N=256, residual=False, rowscale=False),
    E('speinet', 'ref: swin.*.attn.proj (block 0: no DropPath)', '_Linear', M=30000, K=256, N=256, residual=True, rowscale=False),
    E('speinet', 'ref: swin.*.attn.proj', '_Linear', M=30000, K=256, N=256, residual=True, rowscale=True),
    E('speinet', 'ref: swin.*.attn.qkv_x + mlp.fc1', '_Linear', M=30000, K=256, N=512, residual=False, rowscale=False),
    E('speinet', 'ref: swin.*.mlp.fc2 (block 0: no DropPath)', '_Linear', M=30000, K=512, N=256, residual=True, rowscale=False),
    E('speinet', 'ref: swin.*.mlp.fc2', '_Linear', M=30000, K=512, N=256, residual=True, rowscale=True),
    E('speinet', 'noref: conv_lv2', '_Linear', M=20000, K=128, N=64, residual=False, rowscale=False),
    E('speinet', 'ref: conv_lv3', '_Linear', M=15000, K=256, N=128, residual=False, rowscale=False),
    E('speinet', 'ref: fusion', '_Linear', M=15000, K=384, N=128, residual=False, rowscale=False),
    E('speinet', 'noref: swin.*.attn.qkv_y', '_Linear', M=10000, K=256, N=256, residual=False, rowscale=False),
    E('speinet', 'noref: swin.*.attn.proj (block 0: no DropPath)', '_Linear', M=10000, K=256, N=256, residual=True, rowscale=False),
    E('speinet', 'noref: swin.*.attn.proj', '_Linear', M=10000, K=256, N=256, residual=True, rowscale=True),
    E('speinet', 'noref: swin.*.attn.qkv_x + mlp.fc1', '_Linear', M=10000, K=256, N=512, residual=False, rowscale=False),
    E('speinet', 'noref: swin.*.mlp.fc2 (block 0: no DropPath)', '_Linear', M=10000, K=512, N=256, residual=True, rowscale=False),
    E('speinet', 'noref: swin.*.mlp.fc2', '_Linear', M=10000, K=512, N=256, residual=True, rowscale=True),
    E('speinet', 'noref: conv_lv3', '_Linear', M=5000, K=256, N=128, residual=False, rowscale=False),
    E('speinet', 'noref: fusion', '_Linear', M=5000, K=384, N=128, residual=False, rowscale=False),
    E('speinet', 'ref: swin.*.mlp.act', '_Gelu', M=30000, C=512),
    E('speinet', 'noref: swin.*.mlp.act', '_Gelu', M=10000, C=512),
    E('speinet', 'ref: swin.*.attn (shift 0)', '_WindowAttention', B=12, H=50, W=50, shift=0),
    E('speinet', 'ref: swin.*.attn (shift 2)', '_WindowAttention', B=12, H=50, W=50, shift=2),
    E('speinet', 'noref: swin.*.attn (shift 0)', '_WindowAttention', B=4, H=50, W=50, shift=0),
    E('speinet', 'noref: swin.*.attn (shift 2)', '_WindowAttention', B=4, H=50, W=50, shift=2),
    E('speinet', 'ref: SearchTransfer', '_SearchTransfer', B=6, H=50, W=50, Hr=50, Wr=50, transfer=True),
    E('speinet', 'noref: SelfTransfer', '_SearchTransfer', B=2, H=50, W=50, Hr=50, Wr=50, transfer=False),
    E('speinet', 'ref: bicubic(f_v3) + bicubic(f_lv2)', '_Bicubic', B=6, H=100, W=100, C=64, scale=2),
    E('speinet', 'ref: bicubic(S, 2)', '_Bicubic', B=6, H=50, W=50, C=1, scale=2),
    E('speinet', 'ref: bicubic(S, 4)', '_Bicubic', B=6, H=50, W=50, C=1, scale=4),
    E('speinet', 'ref: bicubic(f_lv3)', '_Bicubic', B=6, H=50, W=50, C=128, scale=2),
    E('speinet', 'noref: bicubic(f_v3) + bicubic(f_lv2) + SelfTransfer bicubic(t2)', '_Bicubic', B=2, H=100, W=100, C=64, scale=2),
    E('speinet', 'noref: bicubic(S, 2)', '_Bicubic', B=2, H=50, W=50, C=1, scale=2),
    E('speinet', 'noref: bicubic(S, 4)', '_Bicubic', B=2, H=50, W=50, C=1, scale=4),
    E('speinet', 'noref: bicubic(f_lv3) + SelfTransfer bicubic(ff)', '_Bicubic', B=2, H=50, W=50, C=128, scale=2),
    E('speinet', 'ref: * bicubic(S, 4)', '_RowScale', M=240000, C=32),
    E('speinet', 'noref: * bicubic(S, 4)', '_RowScale', M=80000, C=32),
    E('speinet', 'ref: * bicubic(S, 2)', '_RowScale', M=60000, C=64),
    E('speinet', 'noref: * bicubic(S, 2)', '_RowScale', M=20000, C=64),
    E('speinet', 'ref: * S', '_RowScale', M=15000, C=128),
    E('speinet', 'noref: * S', '_RowScale', M=5000, C=128),
]

KEYS = {"_Conv2d": ("B", "H", "W", "K", "N", "ksize", "stride", "relu", "residual"), "_ConvT2d": ("B", "H", "W", "K", "N"),
        "_ConvIn": ("B", "H", "W", "K", "N"), "_Linear": ("M", "K", "N", "residual", "rowscale"), "_LayerNorm": ("M",),
        "_Gelu": ("M", "C"), "_WindowAttention": ("B", "H", "W", "shift"), "_GatedSum": ("C", "B", "H", "W", "groups"),
        "_SearchTransfer": ("B", "H", "W", "Hr", "Wr", "transfer"), "_Bicubic": ("B", "H", "W", "C", "scale"), "_RowScale": ("M", "C")}


def entry_key(op, shape):
    assert set(shape) == set(KEYS[op]), (op, shape)
    return (op,) + tuple(shape[k] for k in KEYS[op])


def call_key(op, a):
    """The table key of one `Function.apply(*a)` call of speinet_amd.train."""
    if op == "_Conv2d":
        x, w, b, r, B, H, W, ks, st, relu = a
        return (op, B, H, W, w.shape[1], w.shape[0], ks, st, bool(relu), r is not None)
    if op == "_ConvT2d":
        return (op, a[3], a[4], a[5], a[1].shape[0], a[1].shape[1])
    if op == "_ConvIn":
        return (op, a[0].shape[0], a[0].shape[2], a[0].shape[3], a[1].shape[1], a[1].shape[0])
    if op == "_Linear":
        return (op, a[0].shape[0], a[1].shape[1], a[1].shape[0], a[3] is not None, a[4] is not None)
    if op == "_LayerNorm":
        return (op, a[0].shape[0])
    if op in ("_Gelu", "_RowScale"):
        return (op, a[0].shape[0], a[0].shape[1])
    if op == "_WindowAttention":
        return (op,) + tuple(a[3:7])
    if op == "_GatedSum":
        assert a[5], "the training step runs the gates on batch statistics"
        return (op, a[1].shape[1], a[2], a[3], a[4], a[6])
    if op == "_SearchTransfer":
        return (op,) + tuple(a[4:9]) + (a[2] is not None,)
    if op == "_Bicubic":
        return (op, a[1], a[2], a[3], a[0].shape[1], a[4])
    raise KeyError(op)


def table_keys(model):
    keys = [entry_key(op, s) for m, _, op, s in TABLE if m == model]
    assert len(keys) == len(set(keys)), "duplicate table entries"
    return set(keys)


def test_table_entries_are_distinct():
    for model in ("swint", "speinet"):
        table_keys(model)
    assert {op for _, _, op, _ in TABLE} == set(KEYS)


# ---- 2. the launchers' chunk plans, mirrored ----------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


# constants of csrc/backward.hip (wgrad_slices, conv_wgrad_run) and csrc/swin_bwd.hip (spei_ln_bwd_blocks); test_mirrored_plan_constants
# reads them back from the source
WG_1X1_TARGET, WG_1X1_MIN, WG_1X1_MAX = 512, 8, 64            # 1x1: slices for ~512 workgroups, clamped to [8, 64]
WG_ROW_TARGET, WG_ROW_MIN, WG_ROW_MAX, WG_FLOOR = 2048, 16, 256, 64   # tap rows: ~2048 workgroups, [16, 256], then at least 64
WG_STRIDED = 64                                               # 16-bit, stride 2: 64 slices
WG_SEG_ALIGN, WG_SEG_MIN = 4, 4                               # 16-bit chunks: 16-pixel segments, a multiple of 4 (one per wave)
WG_F32_CHUNKS, WG_F32_ALIGN, WG_F32_MIN = 64, 8, 64           # fp32: pixels in at most 64 chunks, a multiple of 8, at least 64
LN_ROWS_PER_BLOCK, LN_MAX_BLOCKS = 4, 512                     # LayerNorm backward: a wave per row, 4 waves, at most 512 blocks


def _src(name):
    with open(os.path.join(ROOT, "speinet_amd", "csrc", name)) as f:
        return f.read()


def _grab(text, pattern):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return tuple(int(v) for v in (found[0] if isinstance(found[0], tuple) else (found[0],)))


def test_mirrored_plan_constants():
    """The plans below are the launchers' (csrc/backward.hip wgrad_slices / conv_wgrad_run, csrc/swin_bwd.hip spei_ln_bwd_blocks)."""
    b, s = _src("backward.hip"), _src("swin_bwd.hip")
    assert _grab(b, r"const int want = cdiv\((\d+), per\);") == (WG_1X1_TARGET,)
    assert _grab(b, r"return want < (\d+) \? \d+ : \(want > (\d+) \? \d+ : want\);") == (WG_1X1_MIN, WG_1X1_MAX)
    assert _grab(b, r"int want = cdiv\((\d+), per_slice\);") == (WG_ROW_TARGET,)
    assert _grab(b, r"want = want < (\d+) \? \d+ : \(want > (\d+) \? \d+ : want\);") == (WG_ROW_MIN, WG_ROW_MAX)
    assert _grab(b, r"return want > (\d+) \? want : \d+;\n}") == (WG_FLOOR,)
    assert _grab(b, r"const int want = rows \? wgrad_slices\(N, K, ksize\) : (\d+);") == (WG_STRIDED,)
    assert _grab(b, r"chunk = \(\(chunk \+ 3\) / (\d+)\) \* \d+;\n\s+if \(chunk < (\d+)\) chunk") == (WG_SEG_ALIGN, WG_SEG_MIN)
    assert _grab(b, r"int chunk = cdiv\(M, (\d+)\);") == (WG_F32_CHUNKS,)
    assert _grab(b, r"chunk = \(\(chunk \+ 7\) / (\d+)\) \* \d+;\n\s+if \(chunk < (\d+)\) chunk") == (WG_F32_ALIGN, WG_F32_MIN)
    assert _grab(s, r"const int64_t b = \(M \+ 3\) / (\d+);\n\s+return b < (\d+)") == (LN_ROWS_PER_BLOCK, LN_MAX_BLOCKS)


def wgrad_slices(N, K, ks):
    if ks == 1:
        per = _cdiv(_cdiv(N, 32), 2) * _cdiv(_cdiv(K, 32), 2)
        return min(max(_cdiv(WG_1X1_TARGET, per), WG_1X1_MIN), WG_1X1_MAX)
    want = min(max(_cdiv(WG_ROW_TARGET, ks * _cdiv(N, 32) * _cdiv(K, 32)), WG_ROW_MIN), WG_ROW_MAX)
    return max(want, WG_FLOOR)


def ln_bwd_blocks(M):
    return min(max(_cdiv(M, LN_ROWS_PER_BLOCK), 1), LN_MAX_BLOCKS)


def wgrad_plan(form, N, K, ks, stride, Hout, Wout, batch):
    """The chunk plan of one spei_conv_wgrad_*_batched call (N <= 256): form "f32" cuts the M output pixels into `chunk` pixel spans,
    the 16-bit forms cut the 16-pixel segments of the output rows into `chunk` segment spans; kernel: which kernel takes the chunks."""
    M = batch * Hout * Wout
    if form == "f32":
        chunk = max(_cdiv(_cdiv(M, WG_F32_CHUNKS), WG_F32_ALIGN) * WG_F32_ALIGN, WG_F32_MIN)
        n = _cdiv(M, chunk)
        return dict(form=form, kernel="fp32", unit="px", chunk=chunk, nchunks=n, wave_px=chunk // 4, Wout=Wout, nseg_row=None, M=M)
    rows = stride == 1
    nseg_row = _cdiv(Wout, 16)
    nseg = batch * Hout * nseg_row
    want = wgrad_slices(N, K, ks) if rows else WG_STRIDED
    chunk = max(_cdiv(_cdiv(nseg, want), WG_SEG_ALIGN) * WG_SEG_ALIGN, WG_SEG_MIN)
    kernel = "per-tap" if not rows else ("1x1" if ks == 1 else "tap-row")
    return dict(form=form, kernel=kernel, unit="seg", chunk=chunk, nchunks=_cdiv(nseg, chunk), slices=want, wave_px=chunk // 4 * 16,
                Wout=Wout, nseg_row=nseg_row, nseg=nseg, M=M)


def chunk_rows(plan, c):
    """Indices (into the stacked output-pixel rows of the wgrad's dY operand) of the pixels chunk c sums."""
    if plan["unit"] == "px":
        return torch.arange(c * plan["chunk"], min(plan["M"], (c + 1) * plan["chunk"]))
    sg = torch.arange(c * plan["chunk"], min(plan["nseg"], (c + 1) * plan["chunk"]))
    nsr, wo = plan["nseg_row"], plan["Wout"]
    ox = (sg % nsr)[:, None] * 16 + torch.arange(16)[None]
    idx = (sg // nsr)[:, None] * wo + ox
    return idx[ox < wo]


def wgrad_calls(op, s, prec):
    """(form, N, K, ksize, stride, Hout, Wout, batch) of every weight-gradient launch the entry's backward makes (train._wgrad: at most
    256 output channels per launch)."""
    form16 = "bf16" if prec == "bf16" else "f32"
    if op == "_Conv2d":
        ho, wo = (s["H"] - 1) // s["stride"] + 1, (s["W"] - 1) // s["stride"] + 1
        calls = [(prec, s["N"], s["K"], s["ksize"], s["stride"], ho, wo, s["B"])]
    elif op == "_ConvT2d":                       # the stride-2 Conv2d view: dY = the input rows x, N = K channels
        calls = [(form16, s["K"], s["N"], 3, 2, s["H"], s["W"], s["B"])]
    elif op == "_ConvIn":
        calls = [(form16, s["N"], s["K"], 5, 1, s["H"], s["W"], s["B"])]
    elif op == "_Linear":
        calls = [(prec, min(256, s["N"] - n0), s["K"], 1, 1, 1, s["M"], 1) for n0 in range(0, s["N"], 256)]
    else:
        return []
    return [(("f32" if f == "f32" else f), n, k, ks, st, ho, wo, b) for f, n, k, ks, st, ho, wo, b in calls]


def test_chunk_plans_partition_the_pixels():
    """chunk_rows of all chunks of a plan is every output pixel once (the span the sensitivity checks zero is a real chunk)."""
    for form, N, K, ks, st, ho, wo, b in [("f32", 32, 32, 5, 1, 37, 45, 3), ("bf16x3", 32, 32, 5, 1, 37, 45, 3), ("bf16", 64, 32, 1, 1, 11, 100, 2),
                                          ("bf16", 64, 32, 5, 2, 9, 21, 2), ("bf16x3", 256, 512, 1, 1, 1, 10000, 1)]:
        p = wgrad_plan(form, N, K, ks, st, ho, wo, b)
        allr = torch.cat([chunk_rows(p, c) for c in range(p["nchunks"])])
        assert torch.equal(allr.sort()[0], torch.arange(b * ho * wo)), (form, N, K, ks)


def test_table_reaches_the_crop_step_regimes():
    """The cases below test the regimes the issue names, not toy versions of them."""
    plans = [(op, s, prec, wgrad_plan(*c)) for _, _, op, s in TABLE for prec in PRECS for c in wgrad_calls(op, s, prec)]
    row = lambda ks, n=None: [p for op, s, _, p in plans if p["kernel"] == "tap-row" and s.get("ksize") == ks and (n is None or s["N"] == n)]
    # 16-bit tap-row weight gradient at >= 200 chunks: ksize 5 (swint level 1) and ksize 3 (speinet search43 / search33 at 200x200)
    assert max(p["nchunks"] for p in row(5)) >= 200 and max(p["nchunks"] for p in row(3)) >= 200
    assert any(p["nchunks"] >= 200 and s["B"] == 60 and s["K"] == 32 for op, s, _, p in plans if p["kernel"] == "tap-row" and s.get("ksize") == 5)
    # above 64 chunks on a 64-channel layer
    assert max(p["nchunks"] for p in row(5, 64)) > 64
    # the 1x1 form with a 64-slice plan and >= 60 chunks (speinet's narrow 1x1 convs)
    assert any(p["slices"] == 64 and p["nchunks"] >= 60 for op, s, _, p in plans if p["kernel"] == "1x1" and op == "_Conv2d")
    # the fp32 form at 64 chunks of more than 8 000 pixels per wave
    assert any(p["nchunks"] == 64 and p["wave_px"] > 8000 for _, _, _, p in plans if p["form"] == "f32")
    # LayerNorm backward at >= 40 rows per wave
    assert max(s["M"] / (4 * ln_bwd_blocks(s["M"])) for _, _, op, s in TABLE if op == "_LayerNorm") >= 40
    big = sorted({(p["kernel"], p["nchunks"], p["wave_px"]) for _, _, _, p in plans}, key=lambda t: -t[1])[:6]
    print("largest chunk plans (kernel, chunks, pixels per wave):", big)


# ---- float64 references: per-tap shifted GEMMs ----------------------------------------------------------------------------------------
def _tap(t, ty, tx, ho, wo, s):
    """The input pixels tap (ty, tx) of a stride-s convolution reads for the ho x wo outputs, from the padded map t [B, Hp, Wp, C]."""
    return t[:, ty:ty + s * (ho - 1) + 1:s, tx:tx + s * (wo - 1) + 1:s]


def _out_size(H, W, ks, s):
    p = ks // 2
    return (H + 2 * p - ks) // s + 1, (W + 2 * p - ks) // s + 1


def conv_fwd64(x, w, B, H, W, s):
    """Conv2d(K -> N, ks, stride s, padding ks // 2), no bias: x [B*H*W, K], w [N, K, ks, ks] -> [B*ho*wo, N], one matmul per tap."""
    N, K, ks, _ = w.shape
    p = ks // 2
    ho, wo = _out_size(H, W, ks, s)
    xp = F.pad(x.view(B, H, W, K), (0, 0, p, p, p, p))
    y = x.new_zeros(B * ho * wo, N)
    for ty in range(ks):
        for tx in range(ks):
            y += _tap(xp, ty, tx, ho, wo, s).reshape(-1, K) @ w[:, :, ty, tx].t()
    return y


def conv_dgrad64(dz, w, B, H, W, s):
    """Data gradient of conv_fwd64 for the output gradient dz [B*ho*wo, N]: dx [B*H*W, K], each tap's dz W_t added back at its pixels."""
    N, K, ks, _ = w.shape
    p = ks // 2
    ho, wo = _out_size(H, W, ks, s)
    dxp = dz.new_zeros(B, H + 2 * p, W + 2 * p, K)
    for ty in range(ks):
        for tx in range(ks):
            _tap(dxp, ty, tx, ho, wo, s).add_((dz @ w[:, :, ty, tx]).view(B, ho, wo, K))
    return dxp[:, p:p + H, p:p + W].reshape(B * H * W, K)


def conv_wgrad64(x, dz, ks, B, H, W, s, spans=()):
    """Weight gradient of conv_fwd64: dw [N, K, ks, ks], per tap dz^T X_t; and for each span (indices of dz rows) that span's share."""
    K, N = x.shape[1], dz.shape[1]
    p = ks // 2
    ho, wo = _out_size(H, W, ks, s)
    xp = F.pad(x.view(B, H, W, K), (0, 0, p, p, p, p))
    dw = x.new_empty(N, K, ks, ks)
    parts = [x.new_empty(N, K, ks, ks) for _ in spans]
    for ty in range(ks):
        for tx in range(ks):
            v = _tap(xp, ty, tx, ho, wo, s).reshape(-1, K)
            dw[:, :, ty, tx] = dz.t() @ v
            for part, idx in zip(parts, spans):
                part[:, :, ty, tx] = dz[idx].t() @ v[idx]
    return dw, parts


def convt_fwd64(x, w, B, H, W):
    """ConvTranspose2d(K -> N, 3, stride 2, padding 1, output_padding 1), no bias: the adjoint of the stride-2 Conv2d(N -> K) on the
    2H x 2W map whose weight is the same tensor read as [out = K][in = N]."""
    return conv_dgrad64(x, w, B, 2 * H, 2 * W, 2)


# ---- device-side comparison -----------------------------------------------------------------------------------------------------------
def _bf(t):
    """A GEMM operand as the "bf16" kernels multiply it: the fp32 value rounded to bf16 (nearest even), in float64."""
    return t.float().bfloat16().double()


def _d64(t):
    return t.detach().double()


def rel2(a, ref):
    return ((_d64(a) - ref).norm() / ref.norm().clamp_min(1e-300)).item()


def relmax(a, ref):
    return ((_d64(a) - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


class Checks:
    """Collects every comparison of a case, prints them, and fails at the end with all that missed (one run shows every miss)."""

    def __init__(self, title):
        self.title, self.lines, self.fails = title, [], []

    def below(self, what, err, bound, extra=""):
        self.lines.append(f"{what} {err:.2e} (bound {bound:.2g}){extra}")
        if not err < bound:
            self.fails.append(f"{what}: {err:.3e} >= {bound:.0e}")

    def above(self, what, val, floor, extra=""):
        self.lines.append(f"{what} {val:.2e} (> {floor:.0e}){extra}")
        if not val > floor:
            self.fails.append(f"{what}: {val:.3e} <= {floor:.0e}")

    def done(self):
        print(f"\n  {self.title}\n    " + "\n    ".join(self.lines))
        assert not self.fails, f"{self.title}: " + "; ".join(self.fails)


def gemm_result(ck, prec, what, got, exact, rounded=None, got32=None, bound=None, f32_form=False):
    """One GEMM result.  f32 / bf16x3: relative L2 from float64 on the unrounded operands.  bf16: the rounded-operand contract
    (max-abs relative), unrounded float64 within the inference bound, and the control: away from the f32 run.  f32_form: the result
    runs in fp32 whatever the mode (the modes' fp32 forms), so it takes the f32 bound.  Returns the bound used."""
    if prec == "bf16" and not f32_form:
        ck.below(f"{what} vs bf16-operand float64", relmax(got, rounded), CONTRACT)
        ck.below(f"{what} vs float64", relmax(got, exact), INFER)
        ck.above(f"{what} vs the f32 run", ((_d64(got) - _d64(got32)).abs().max() / rounded.abs().max()).item(), CONTROL)
        return CONTRACT
    ck.below(f"{what}", rel2(got, exact), bound)
    return bound


def sensitivity(ck, what, plan, dw, parts, bound, metric, ks):
    """The error one dropped chunk (parts: the float64 shares of the chunks tested) or one dropped tap row would leave in dw, in the
    metric of the bound, at least MARGIN times the bound."""
    size = (lambda t: t.norm().item() / dw.norm().item()) if metric == "l2" else (lambda t: t.abs().max().item() / dw.abs().max().item())
    chunk = min(size(p) for p in parts)
    row = min(size(dw[:, :, ty]) for ty in range(ks)) if ks > 1 else float("inf")
    worst = min(chunk, row)
    ck.above(f"{what}: one dropped chunk ({plan['kernel']}, {plan['nchunks']} chunks of {plan['wave_px']} px per wave) / tap row "
             f"moves it by {chunk:.1e} / {row:.1e}; margin over the bound", worst / bound, MARGIN)


def plan_spans(plan, dev):
    """The last chunk and a middle one: the far end of the partials (an offset bug past slice 64) and an interior one."""
    return [chunk_rows(plan, c).to(dev) for c in sorted({plan["nchunks"] - 1, plan["nchunks"] // 2})]


def _gen(entry_k):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(entry_k).encode()))


def _randn(gen, *shape, scale=1.0):
    return torch.randn(*shape, device=DEV, generator=gen).mul_(scale)


def _prec_ctx(prec):
    from speinet_amd import train as T
    import contextlib

    @contextlib.contextmanager
    def cm():
        tok = T._PREC.set(prec)
        try:
            yield
        finally:
            T._PREC.reset(tok)
    return cm()


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


def _relu_flips(ck, y, z):
    """ReLU decisions of the HIP forward against float64's pre-activation: within round-off of zero they may fall either way (the
    bound of test_conv_forward_backward); the float64 backward then takes HIP's mask."""
    mask = y > 0
    flips = int((mask != (z > 0)).sum().item())
    ck.below("ReLU decisions that differ", flips, max(2, y.numel() // 20000) + 1)
    return mask.double()


# ---- 3. the per-op cases --------------------------------------------------------------------------------------------------------------
def _expected_routes(op, s, prec):
    """The C-ABI entries (their `_lib.check` names) one forward + backward of the entry must reach in `prec`."""
    wg = "spei_conv_wgrad_batched"
    if op == "_Conv2d":
        b16 = prec in ("bf16x3", "bf16")
        fwd = {"spei_pack_split16", "spei_conv_slab16_batched"} if b16 else {"spei_igemm_f32_batched"}
        if s["stride"] == 1:
            dgrad = {"spei_pack_split16", "spei_conv_slab16_batched"} if b16 else {"spei_igemm_f32_batched"}
        else:
            dgrad = {"spei_conv_s2_adjoint_slab16"} if prec == "bf16" else {"spei_igemm_f32_batched"}
        return fwd | dgrad | {wg} | ({"spei_relu_bwd"} if s["relu"] else set())
    if op == "_ConvT2d":
        if prec == "bf16":
            return {"spei_convt2_slab16", "spei_pack_split16", "spei_conv_slab16_batched", "spei_relu_bwd", wg}
        return {"spei_igemm_f32_batched", "spei_relu_bwd", wg}
    if op == "_ConvIn":
        return {"spei_conv5_in", "spei_relu_bwd", wg}
    if op == "_Linear":
        gemm = {"spei_pack_split16", "spei_conv_slab16"} if prec in ("bf16x3", "bf16") else {"spei_igemm_f32_batched"}
        return gemm | {wg} | ({"spei_scale_rows"} if s["rowscale"] else set())
    if op == "_LayerNorm":
        return {"spei_layernorm256", "spei_layernorm256_bwd"}
    if op == "_Gelu":
        return {"spei_gelu_fwd", "spei_gelu_bwd"}
    if op == "_WindowAttention":
        return {"spei_window_attention16_train" if prec == "bf16" else "spei_window_attention_batched", "spei_window_attention_bwd"}
    if op == "_GatedSum":
        return {"spei_plane_stats_batched", "spei_gate_maps_fwd", "spei_resblock_apply_batched", "spei_gate_maps_bwd",
                "spei_resblock_apply_bwd_batched"}
    if op == "_SearchTransfer":
        return {"spei_patch_invnorm", "spei_corr_argmax", "spei_corr_s_bwd_lr", "spei_search_bwd_ref"} | \
            ({"spei_gather_fold"} if s["transfer"] else set())
    if op == "_Bicubic":
        return {"spei_upsample_bicubic", "spei_upsample_bicubic_bwd"}
    if op == "_RowScale":
        return {"spei_scale_rows", "spei_rowdot"}
    raise KeyError(op)


def case_conv2d(ck, s, prec, gen, run):
    from speinet_amd import train as T
    B, H, W, K, N, ks, st, relu, res = (s[k] for k in KEYS["_Conv2d"])
    ho, wo = _out_size(H, W, ks, st)
    x = _randn(gen, B * H * W, K)
    w = _randn(gen, N, K, ks, ks, scale=1.0 / math.sqrt(K * ks * ks))
    b = _randn(gen, N, scale=0.1)
    r = _randn(gen, B * ho * wo, N) if res else None
    g = _randn(gen, B * ho * wo, N)

    def hip(p):
        xl, wl, bl = _leaf(x), _leaf(w), _leaf(b)
        rl = _leaf(r) if res else None
        with _prec_ctx(p):
            y = T._Conv2d.apply(xl, wl, bl, rl, B, H, W, ks, st, relu)
        y.backward(g)
        return y.detach(), xl.grad, wl.grad, bl.grad, (rl.grad if res else None)

    got = run(lambda: hip(prec))
    got32 = hip("f32") if prec == "bf16" else None
    plan = wgrad_plan(*wgrad_calls("_Conv2d", s, prec)[0])
    spans = plan_spans(plan, x.device)
    refs = {}
    for name, rnd in (("exact", _d64), ("rounded", _bf)) if prec == "bf16" else (("exact", _d64),):
        z = conv_fwd64(rnd(x), rnd(w), B, H, W, st) + _d64(b) + (_d64(r) if res else 0)
        if relu:
            mask = _relu_flips(ck, got[0], z) if name == ("rounded" if prec == "bf16" else "exact") else (got[0] > 0).double()
            z = z.clamp_min(0)
            gz = _d64(g) * mask
        else:
            gz = _d64(g)
        dw, parts = conv_wgrad64(rnd(x), rnd(gz), ks, B, H, W, st, spans if name == "exact" else ())
        refs[name] = (z, conv_dgrad64(rnd(gz), rnd(w), B, H, W, st), dw, gz.sum(0), parts, [gz[i].sum(0) for i in spans])
        del z, gz
    ex, rd = refs["exact"], refs.get("rounded", (None,) * 4)
    tf, tb = TOL.get(prec, (None, None))
    gemm_result(ck, prec, "forward", got[0], ex[0], rd[0], got32 and got32[0], tf)
    gemm_result(ck, prec, "data gradient", got[1], ex[1], rd[1], got32 and got32[1], tb)
    wb = gemm_result(ck, prec, "weight gradient", got[2], ex[2], rd[2], got32 and got32[2], tb)
    metric = "max" if prec == "bf16" else "l2"
    sensitivity(ck, "weight gradient", plan, ex[2], ex[4], wb, metric, ks)
    bb = CONTRACT if prec == "bf16" else tb
    ck.below("bias gradient", (relmax if prec == "bf16" else rel2)(got[3], ex[3]), bb)
    db_chunk = min((p.abs().max() / ex[3].abs().max() if prec == "bf16" else p.norm() / ex[3].norm()).item() for p in ex[5])
    ck.above(f"bias gradient: one dropped chunk moves it by {db_chunk:.1e}; margin over the bound", db_chunk / bb, MARGIN)
    if res:
        ck.below("residual gradient (passed through)", rel2(got[4], _d64(g)), 1e-12)


def case_convt2d(ck, s, prec, gen, run):
    from speinet_amd import train as T
    B, H, W, K, N = (s[k] for k in KEYS["_ConvT2d"])
    x = _randn(gen, B * H * W, K)
    w = _randn(gen, K, N, 3, 3, scale=1.0 / math.sqrt(K * 9 / 4))
    b = _randn(gen, N, scale=0.1)
    g = _randn(gen, B * 4 * H * W, N)

    def hip(p):
        xl, wl, bl = _leaf(x), _leaf(w), _leaf(b)
        with _prec_ctx(p):
            y = T._ConvT2d.apply(xl, wl, bl, B, H, W)
        y.backward(g)
        return y.detach(), xl.grad, wl.grad, bl.grad

    got = run(lambda: hip(prec))
    got32 = hip("f32") if prec == "bf16" else None
    plan = wgrad_plan(*wgrad_calls("_ConvT2d", s, prec)[0])
    spans = plan_spans(plan, x.device)
    refs = {}
    for name, rnd in (("exact", _d64), ("rounded", _bf)) if prec == "bf16" else (("exact", _d64),):
        z = convt_fwd64(rnd(x), rnd(w), B, H, W) + _d64(b)
        mask = _relu_flips(ck, got[0], z) if name == ("rounded" if prec == "bf16" else "exact") else (got[0] > 0).double()
        gz = _d64(g) * mask
        # the weight gradient is the stride-2 Conv2d's, with dZ as its input map and x as its output gradient
        dw, parts = conv_wgrad64(rnd(gz), rnd(x), 3, B, 2 * H, 2 * W, 2, spans if name == "exact" else ())
        refs[name] = (z.clamp_min(0), conv_fwd64(rnd(gz), rnd(w), B, 2 * H, 2 * W, 2), dw, gz.sum(0), parts)
        del z, gz
    ex, rd = refs["exact"], refs.get("rounded", (None,) * 4)
    f32_form = prec != "bf16"                 # bf16x3 keeps the stride-2 transposed forms in fp32
    tf, tb = TOL["f32"]
    gemm_result(ck, prec, "forward", got[0], ex[0], rd[0], got32 and got32[0], tf, f32_form)
    gemm_result(ck, prec, "data gradient", got[1], ex[1], rd[1], got32 and got32[1], tb, f32_form)
    wb = gemm_result(ck, prec, "weight gradient", got[2], ex[2], rd[2], got32 and got32[2], tb, f32_form)
    sensitivity(ck, "weight gradient", plan, ex[2], ex[4], wb, "max" if prec == "bf16" else "l2", 3)
    ck.below("bias gradient", (relmax if prec == "bf16" else rel2)(got[3], ex[3]), CONTRACT if prec == "bf16" else tb)


def case_convin(ck, s, prec, gen, run):
    from speinet_amd import train as T
    B, H, W, K, N = (s[k] for k in KEYS["_ConvIn"])
    frames = torch.rand(B, K, H, W, device=DEV, generator=gen)
    w = _randn(gen, N, K, 5, 5, scale=0.1)
    b = _randn(gen, N, scale=0.1)
    g = _randn(gen, B * H * W, N)
    x = frames.permute(0, 2, 3, 1).reshape(-1, K)

    def hip(p):
        wl, bl = _leaf(w), _leaf(b)
        with _prec_ctx(p):
            y = T._ConvIn.apply(frames, wl, bl)
        y.backward(g)
        return y.detach(), wl.grad, bl.grad

    got = run(lambda: hip(prec))
    got32 = hip("f32") if prec == "bf16" else None
    plan = wgrad_plan(*wgrad_calls("_ConvIn", s, prec)[0])
    spans = plan_spans(plan, x.device)
    z = conv_fwd64(_d64(x), _d64(w), B, H, W, 1) + _d64(b)
    mask = _relu_flips(ck, got[0], z)
    ck.below("forward (fp32 in every mode)", rel2(got[0], z.clamp_min(0)), CONV_IN_TOL[0])
    del z
    gz = _d64(g) * mask
    dw, parts = conv_wgrad64(_d64(x), gz, 5, B, H, W, 1, spans)
    rd = conv_wgrad64(_bf(x), _bf(gz), 5, B, H, W, 1)[0] if prec == "bf16" else None
    # the weight gradient: bf16 in "bf16", the fp32 form in the other two modes
    wb = gemm_result(ck, prec, "weight gradient", got[1], dw, rd, got32 and got32[1], CONV_IN_TOL[1], prec != "bf16")
    sensitivity(ck, "weight gradient", plan, dw, parts, wb, "max" if prec == "bf16" else "l2", 5)
    ck.below("bias gradient", (relmax if prec == "bf16" else rel2)(got[2], gz.sum(0)), CONTRACT if prec == "bf16" else CONV_IN_TOL[1])


def case_linear(ck, s, prec, gen, run):
    from speinet_amd import train as T
    M, K, N, res, rsc = (s[k] for k in KEYS["_Linear"])
    x = _randn(gen, M, K)
    w = _randn(gen, N, K, scale=1.0 / math.sqrt(K))
    b = _randn(gen, N, scale=0.1)
    r = _randn(gen, M, N) if res else None
    rs = (torch.rand(M, device=DEV, generator=gen) < 0.9).float() / 0.9 if rsc else None     # DropPath: 0 or 1 / keep per row
    g = _randn(gen, M, N)

    def hip(p):
        xl, wl, bl = _leaf(x), _leaf(w), _leaf(b)
        rl = _leaf(r) if res else None
        with _prec_ctx(p):
            y = T._Linear.apply(xl, wl, bl, rl, rs)
        y.backward(g)
        return y.detach(), xl.grad, wl.grad, bl.grad, (rl.grad if res else None)

    got = run(lambda: hip(prec))
    got32 = hip("f32") if prec == "bf16" else None
    gs = _d64(g * rs[:, None]) if rsc else _d64(g)          # spei_scale_rows: the factor applied to dY in fp32
    plans = [wgrad_plan(*c) for c in wgrad_calls("_Linear", s, prec)]
    spans = plan_spans(plans[0], x.device)
    refs = {}
    for name, rnd in (("exact", _d64), ("rounded", _bf)) if prec == "bf16" else (("exact", _d64),):
        y = rnd(x) @ rnd(w).t() + _d64(b)
        if rsc:
            y = y * _d64(rs)[:, None]
        if res:
            y = y + _d64(r)
        refs[name] = (y, rnd(gs) @ rnd(w), rnd(gs).t() @ rnd(x))
        del y
    ex, rd = refs["exact"], refs.get("rounded", (None,) * 3)
    parts = [(gs[i].t() @ _d64(x)[i])[:, :, None, None] for i in spans]
    tf, tb = TOL.get(prec, (None, None))
    gemm_result(ck, prec, "forward", got[0], ex[0], rd[0], got32 and got32[0], tf)
    gemm_result(ck, prec, "data gradient", got[1], ex[1], rd[1], got32 and got32[1], tb)
    wb = gemm_result(ck, prec, "weight gradient", got[2], ex[2], rd[2], got32 and got32[2], tb)
    sensitivity(ck, "weight gradient", plans[0], ex[2][:, :, None, None], parts, wb, "max" if prec == "bf16" else "l2", 1)
    ck.below("bias gradient", (relmax if prec == "bf16" else rel2)(got[3], gs.sum(0)), CONTRACT if prec == "bf16" else tb)
    if res:
        ck.below("residual gradient (passed through)", rel2(got[4], _d64(g)), 1e-12)


def case_layernorm(ck, s, prec, gen, run):
    from speinet_amd import train as T
    M = s["M"]
    x = _randn(gen, M, 256, scale=1.7).add_(0.3)
    gamma, beta = _randn(gen, 256), _randn(gen, 256)
    g = _randn(gen, M, 256)

    def hip():
        xl, gl, bl = _leaf(x), _leaf(gamma), _leaf(beta)
        with _prec_ctx(prec):
            y = T._LayerNorm.apply(xl, gl, bl)
        y.backward(g)
        return y.detach(), xl.grad, gl.grad, bl.grad

    got = run(hip)
    x64, g64, b64 = (_d64(t).requires_grad_(True) for t in (x, gamma, beta))
    y = F.layer_norm(x64, (256,), g64, b64, 1e-5)
    dx, dg, db = torch.autograd.grad(y, (x64, g64, b64), _d64(g))
    ck.below("forward", rel2(got[0], y.detach()), LN_TOL[0])
    ck.below("data gradient", rel2(got[1], dx), LN_TOL[1])
    ck.below("dgamma", rel2(got[2], dg), LN_TOL[1])
    ck.below("dbeta", rel2(got[3], db), LN_TOL[1])
    # one block partial: block k sums the rows of waves 4k .. 4k + 3, i.e. rows m with (m // 4) % blocks == k
    nb = ln_bwd_blocks(M)
    xhat = F.layer_norm(_d64(x), (256,), eps=1e-5)
    both = torch.cat([dg, db])
    m = torch.arange(M, device=DEV)
    drop = []
    for k in (0, nb - 1):
        rows = m[(m // 4) % nb == k]
        drop.append((torch.cat([(_d64(g)[rows] * xhat[rows]).sum(0), _d64(g)[rows].sum(0)]).norm() / both.norm()).item())
    ck.above(f"LayerNorm ({nb} blocks, {M / (4 * nb):.1f} rows per wave): one dropped block partial moves dgamma / dbeta by "
             f"{min(drop):.1e}; margin over the bound", min(drop) / LN_TOL[1], MARGIN)


def case_gelu(ck, s, prec, gen, run):
    from speinet_amd import train as T
    pre = _randn(gen, s["M"], s["C"], scale=2.5)
    g = _randn(gen, s["M"], s["C"])

    def hip():
        pl = _leaf(pre)
        with _prec_ctx(prec):
            y = T._Gelu.apply(pl)
        y.backward(g)
        return y.detach(), pl.grad

    got = run(hip)
    p64 = _d64(pre).requires_grad_(True)
    y = F.gelu(p64)
    (d,) = torch.autograd.grad(y, p64, _d64(g))
    ck.below("forward", rel2(got[0], y.detach()), GELU_TOL[0])
    ck.below("gradient", rel2(got[1], d), GELU_TOL[1])


def case_rowscale(ck, s, prec, gen, run):
    from speinet_amd import train as T
    x, sv, g = _randn(gen, s["M"], s["C"]), _randn(gen, s["M"]), _randn(gen, s["M"], s["C"])

    def hip():
        xl, sl = _leaf(x), _leaf(sv)
        with _prec_ctx(prec):
            y = T._RowScale.apply(xl, sl)
        y.backward(g)
        return y.detach(), xl.grad, sl.grad

    got = run(hip)
    x64, s64, g64 = _d64(x), _d64(sv), _d64(g)
    ck.below("forward", rel2(got[0], x64 * s64[:, None]), ROWSCALE_TOL[0])
    ck.below("dx", rel2(got[1], g64 * s64[:, None]), ROWSCALE_TOL[0])
    ck.below("ds (row dot products)", rel2(got[2], (g64 * x64).sum(1)), ROWSCALE_TOL[1])


def _nchw(rows, B, H, W):
    return rows.view(B, H, W, -1).permute(0, 3, 1, 2)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def case_bicubic(ck, s, prec, gen, run):
    from speinet_amd import train as T
    B, H, W, c, sc = (s[k] for k in KEYS["_Bicubic"])
    x, g = _randn(gen, B * H * W, c), _randn(gen, B * sc * sc * H * W, c)

    def hip():
        xl = _leaf(x)
        with _prec_ctx(prec):
            y = T._Bicubic.apply(xl, B, H, W, sc)
        y.backward(g)
        return y.detach(), xl.grad

    got = run(hip)
    x64 = _nchw(_d64(x), B, H, W).requires_grad_(True)
    y = F.interpolate(x64, scale_factor=sc, mode="bicubic")
    (d,) = torch.autograd.grad(y, x64, _nchw(_d64(g), B, sc * H, sc * W))
    ck.below("forward", rel2(got[0], _rows(y.detach())), BICUBIC_TOL[0])
    ck.below("adjoint", rel2(got[1], _rows(d)), BICUBIC_TOL[1])


def case_window_attention(ck, s, prec, gen, run):
    from speinet_amd import train as T
    from test_gpu_train_bf16 import _attn_ref
    B, H, W, shift = (s[k] for k in KEYS["_WindowAttention"])
    m = B * H * W
    q = _randn(gen, m, 256, scale=0.35 if prec == "bf16" else 0.6)      # the scales of the toy-shape tests
    kv, rb, g = _randn(gen, m, 512), _randn(gen, 8, 25, 25, scale=0.5), _randn(gen, m, 256)

    def hip(p):
        ql, kl, rl = _leaf(q), _leaf(kv), _leaf(rb)
        with _prec_ctx(p):
            out = T._WindowAttention.apply(ql, kl, rl, B, H, W, shift)
        out.backward(g)
        return out.detach(), ql.grad, kl.grad, rl.grad

    got = run(lambda: hip(prec))
    ident = lambda t: t
    ex, _ = _attn_ref(_d64(q), _d64(kv), _d64(rb), _d64(g), B, H, W, shift, ident)
    names = ("out", "dq", "dkv", "drelbias")
    if prec == "bf16":
        got32 = hip("f32")
        rd, slack = _attn_ref(_d64(q), _d64(kv), _d64(rb), _d64(g), B, H, W, shift, _bf)
        for i, what in enumerate(names):
            # entries of P / dS within round-off of a bf16 tie may round the other way: their ulp is allowed (test_gpu_train_bf16)
            d = ((_d64(got[i]) - rd[i]).abs() - slack[i]).clamp_min(0)
            ck.below(f"{what} vs bf16-operand float64 beyond the tie slack", (d.max() / rd[i].abs().max()).item(), ATTN)
            ck.below(f"{what} vs float64", relmax(got[i], ex[i]), INFER)
            ck.above(f"{what} vs the f32 run", ((_d64(got[i]) - _d64(got32[i])).abs().max() / rd[i].abs().max()).item(), CONTROL)
        bound, metric = ATTN, "max"
    else:
        for i, what in enumerate(names):
            ck.below(what, rel2(got[i], ex[i]), ATTN_TOL[0] if i == 0 else ATTN_TOL[1])
        bound, metric = ATTN_TOL[1], "l2"
    # one window's dbias_part: window (0, 0) of the shifted frame of sample 0 (inside the map, no mask), as a one-window call
    yy = (torch.arange(5, device=DEV) + shift) % H
    xx = (torch.arange(5, device=DEV) + shift) % W
    idx = (yy[:, None] * W + xx[None]).reshape(-1)
    one = _attn_ref(_d64(q)[idx], _d64(kv)[idx], _d64(rb), _d64(g)[idx], 1, 5, 5, 0, ident)[0][3]
    size = (one.norm() / ex[3].norm() if metric == "l2" else one.abs().max() / ex[3].abs().max()).item()
    ck.above(f"drelbias ({B * (H // 5) * (W // 5)} windows): one missing window partial moves it by {size:.1e}; margin over the bound",
             size / bound, MARGIN)


def case_gated_sum(ck, s, prec, gen, run):
    from speinet_amd import train as T
    from test_gpu_grad import _gate_params, _gated_sum_torch
    c, B, H, W, groups = (s[k] for k in KEYS["_GatedSum"])
    x, x1, dout = (_randn(gen, B, H, W, c) for _ in range(3))
    prm = _gate_params(c, c * 10 + W)
    run_idx = (7, 8, 12, 13)

    def hip():
        xg, x1g = _leaf(x.view(-1, c)), _leaf(x1.view(-1, c))
        pd = [t.clone().to(DEV).requires_grad_(i not in run_idx) for i, t in enumerate(prm)]
        with _prec_ctx(prec):
            out = T._GatedSum.apply(xg, x1g, B, H, W, True, groups, *pd)
        out.backward(dout.view(-1, c))
        return out.detach(), xg.grad, x1g.grad, pd

    got = run(hip)
    x64, x164 = _d64(x).requires_grad_(True), _d64(x1).requires_grad_(True)
    p64 = [t.double().to(DEV).requires_grad_(i not in run_idx) for i, t in enumerate(prm)]
    out64 = _gated_sum_torch(x64, x164, p64, groups, True)[0]
    grads = torch.autograd.grad(out64, [x164] + [t for t in p64 if t.requires_grad], _d64(dout))
    ck.below("output", rel2(got[0], out64.detach().view(-1, c)), GATE_TOL[0])
    ck.below("dx (passed through)", rel2(got[1], _d64(dout).view(-1, c)), 1e-12)
    ck.below("dx1", rel2(got[2], grads[0].view(-1, c)), GATE_TOL[1])
    gp = grads[1:]
    gscale = max(t.norm().item() for t in gp)
    got_p = [t.grad for i, t in enumerate(got[3]) if i not in run_idx]
    names = ("se_w1", "se_b1", "se_w2", "se_b2", "cw_w", "cw_g", "cw_b", "hc_w", "hc_g", "hc_b")
    # The two 2 -> 1 convolution weights (cw_w, hc_w) are sums over a BatchNorm group's N = (B / groups) * H * C (resp. C * W) gate-map
    # elements of dt * z, dt the BatchNorm backward in fp32 (csrc/gates_train.hip gm_bwd_dt_kernel; the sums themselves are fp64,
    # and rounding the plane statistics to fp32 moves the float64 reference by < 1e-8).  The gradient is orthogonal to the weight
    # (BatchNorm's scale invariance), so it is a cancelling sum: the fp32 rounding of the N terms dt (a few operations of 2^-24 each)
    # adds up as sqrt(N) 2^-24 relative to the terms, against a gradient of the terms' size.  Bound: 4 sqrt(N) 2^-24, not below the
    # toy-shape bound (N = 128 000: 8.5e-5, measured up to 2.4e-5; at the toy shapes N <= 10 000 and the bound stays 2e-5).  One of the
    # kernel's 32 element chunks dropped would move these gradients by ~1/sqrt(32).
    n_el = {"cw_w": (B // groups) * H * c, "hc_w": (B // groups) * c * W}
    for a, e, nm in zip(got_p, gp, names):
        err = (_d64(a) - e).norm().item() / max(e.norm().item(), 1e-3 * gscale)
        if nm in n_el:
            ck.below(f"{nm} (N = {n_el[nm]} per group)", err, max(GATE_TOL[2], 4 * math.sqrt(n_el[nm]) * 2.0 ** -24))
        else:
            ck.below(nm, err, GATE_TOL[2])
    ck.below("running buffers", max((_d64(got[3][i]) - p64[i].detach()).abs().max().item() for i in run_idx), 1e-6)


def _search_at(lr, ref3, ref2, ref1, arg):
    """_search_transfer_ref's S and transfers evaluated at a given arg-max [n, hw] (the kernel's): S = the normalised correlation there."""
    n, c, h, w = lr.shape
    a = F.normalize(F.unfold(lr, 3, padding=1), dim=1)
    bq = F.normalize(F.unfold(ref3, 3, padding=1), dim=1)
    s = (bq.gather(2, arg[:, None].expand(-1, bq.shape[1], -1)) * a).sum(1)
    outs = []
    for rf, sc in ((ref3, 1), (ref2, 2), (ref1, 4)):
        if rf is None:
            outs.append(None)
            continue
        u = F.unfold(rf, 3 * sc, padding=sc, stride=sc)
        t = torch.gather(u, 2, arg.unsqueeze(1).expand(-1, u.shape[1], -1))
        outs.append(F.fold(t, (h * sc, w * sc), 3 * sc, padding=sc, stride=sc) / 9.0)
    return s.view(n, h, w), outs


def case_search_transfer(ck, s, prec, gen, run):
    from speinet_amd import train as T
    from test_gpu_train import _search_transfer_ref
    B, H, W, Hr, Wr, transfer = (s[k] for k in KEYS["_SearchTransfer"])
    # queries that share a common direction v and a reference with three hot spots (3 x 3 patches near v): most queries pick one of
    # them, so the per-position query lists of the backward are hundreds long, as on real features (random maps give lists of ~1)
    v = _randn(gen, 128)
    lr = _randn(gen, B * H * W, 128, scale=0.7).add_(v)
    refs = [_randn(gen, B * sc * sc * Hr * Wr, cc) for sc, cc in ((1, 128), (2, 64), (4, 32))] if transfer else None
    if transfer:
        r3 = refs[0].view(B, Hr, Wr, 128)
        for y, x in ((10, 10), (Hr // 2 + 5, Wr // 2 + 10), (Hr - 10, 12)):
            r3[:, y - 1:y + 2, x - 1:x + 2] = _randn(gen, B, 3, 3, 128, scale=0.1).add_(v)
    gs = [_randn(gen, B * H * W)] + ([_randn(gen, B * sc * sc * H * W, cc) for sc, cc in ((1, 128), (2, 64), (4, 32))] if transfer else [])

    def hip():
        if transfer:
            dl = [_leaf(lr)] + [_leaf(t) for t in refs]
            with _prec_ctx(prec):
                S, T3, T2, T1, A = T._SearchTransfer.apply(*dl, B, H, W, Hr, Wr)
            tot = sum((o * gg).sum() for o, gg in zip((S, T3, T2, T1), gs))
        else:
            dl = [_leaf(lr)]
            ref = dl[0].view(B, H, W, -1).transpose(1, 2).flip(1).reshape(B * H * W, -1)
            with _prec_ctx(prec):
                S, T3, T2, T1, A = T._SearchTransfer.apply(dl[0], ref, None, None, B, H, W, W, H)
            tot = (S * gs[0]).sum()
        tot.backward()
        return [S.detach()] + ([T3.detach(), T2.detach(), T1.detach()] if transfer else []), A.detach(), [t.grad for t in dl]

    outs, A, grads = run(hip)
    lr64 = _nchw(_d64(lr), B, H, W).requires_grad_(True)
    if transfer:
        r64 = [_nchw(_d64(t), B, sc * Hr, sc * Wr).requires_grad_(True) for t, sc in zip(refs, (1, 2, 4))]
        r3, r2, r1 = r64
    else:
        r64 = []
        r3, r2, r1 = lr64.transpose(2, 3).flip(2), None, None
    s_max, _, _, _, arg64 = _search_transfer_ref(lr64.detach(), r3.detach(), None, None)
    arg = A.view(B, H * W).long()
    s_k, tt = _search_at(lr64, r3, r2, r1, arg)
    gap = (s_max.reshape(B, -1) - s_k.detach().reshape(B, -1)).max().item()
    n_other = int((arg != arg64).sum().item())
    # where the kernel's arg-max differs from float64's, its score is within fp32 round-off of the maximum (a legal near-tie)
    ck.below(f"arg-max score gap to the float64 maximum ({n_other} of {arg.numel()} queries on another position)", gap, 2e-6)
    longest = max(int(torch.bincount(a).max().item()) for a in arg)
    if transfer:
        ck.above("longest per-position query list", longest, 500)
    else:
        ck.lines.append(f"longest per-position query list {longest}")
    ck.below("S", rel2(outs[0], s_k.detach().reshape(-1)), SEARCH_TOL[0])
    for o, t, nm in zip(outs[1:], tt, ("T_lv3", "T_lv2", "T_lv1")):
        ck.below(nm, rel2(o, _rows(t.detach())), SEARCH_TOL[1])
    tot = (s_k.reshape(-1) * _d64(gs[0])).sum()
    if transfer:
        for t, gg, sc, cc in zip(tt, gs[1:], (1, 2, 4), (128, 64, 32)):
            tot = tot + (t * _nchw(_d64(gg), B, sc * H, sc * W)).sum()
    ref_grads = torch.autograd.grad(tot, [lr64] + r64)
    for a, e, nm in zip(grads, ref_grads, ("d lr", "d ref3", "d ref2", "d ref1")):
        ck.below(nm, rel2(a, _rows(e)), SEARCH_TOL[2])


CASE = {"_Conv2d": case_conv2d, "_ConvT2d": case_convt2d, "_ConvIn": case_convin, "_Linear": case_linear, "_LayerNorm": case_layernorm,
        "_Gelu": case_gelu, "_RowScale": case_rowscale, "_Bicubic": case_bicubic, "_WindowAttention": case_window_attention,
        "_GatedSum": case_gated_sum, "_SearchTransfer": case_search_transfer}


def _case_id(entry, prec):
    model, _, op, s = entry
    return f"{model}-{op.strip('_')}-" + "-".join(f"{k}{int(v) if isinstance(v, bool) else v}" for k, v in s.items()) + f"-{prec}"


CASES = [(e, p) for e in TABLE for p in PRECS]


@pytest.fixture
def _device_budget(request):
    """Each GPU case starts from an empty cache and reports its peak device memory and time; a per-op case stays under 40 GiB (the
    coverage test runs whole training steps: its peak is the benchmark's own)."""
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    print(f"\n  [{request.node.name}] peak {peak:.2f} GiB, {time.time() - t0:.1f} s")
    torch.cuda.empty_cache()
    if request.node.name.startswith("test_op_at_step_shape"):
        assert peak < 40, f"peak device memory {peak:.1f} GiB"


@pytest.fixture
def _routes(monkeypatch):
    """The `_lib.check` names (one per C-ABI launch) seen while the fixture is active."""
    from speinet_amd import _lib
    seen = []
    orig = _lib.check

    def check(rc, what):
        seen.append(what)
        return orig(rc, what)
    monkeypatch.setattr(_lib, "check", check)
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("entry,prec", CASES, ids=[_case_id(e, p) for e, p in CASES])
def test_op_at_step_shape(entry, prec, _device_budget, _routes):
    """One table entry in one train precision: forward and every gradient against float64 on the device, the route it ran, and (for
    the weight gradients, LayerNorm and window attention) that its bound would see one dropped partial."""
    model, layer, op, s = entry
    ck = Checks(f"{model} {layer} [{op} {s}] {prec}")

    def run(fn):
        _routes.clear()
        out = fn()
        torch.cuda.synchronize()
        ck.routes = set(_routes)
        return out

    with torch.cuda.device(DEV):
        CASE[op](ck, s, prec, _gen(entry_key(op, s)), run)
    want = _expected_routes(op, s, prec)
    ck.lines.append(f"route: {sorted(ck.routes)}")
    if ck.routes != want:
        ck.fails.append(f"route {sorted(ck.routes)} != {sorted(want)}")
    ck.done()


# ---- 1b. the table is the step --------------------------------------------------------------------------------------------------------
def _bench_model(which):
    """The model and batch of `bench.py --train --model <which>` (synthetic weights, 200x200 crops)."""
    from speinet_amd.speinet import default_args
    from speinet_amd.synth import synth_frames, synth_state_dict
    args = default_args()
    args.n_sequence = 3
    if which == "swint":
        from speinet_amd.swint import SPEINet
        net = SPEINet(n_sequence=3, args=args)
        x = synth_frames(20, 200, 200, seed=7)[:, :3].contiguous()
    else:
        from speinet_amd.speinet import SPEINet
        net = SPEINet(args=args)
        x = synth_frames(8, 200, 200, seed=7, zero_ref=tuple(range(3, 8, 4))).contiguous()
    net.load_state_dict(synth_state_dict(net.state_dict(), seed=0), strict=True)
    return net.to(DEV).train(), x.to(DEV)


@pytest.mark.gpu
def test_shape_table_covers_the_step(monkeypatch, _device_budget):
    """One forward + backward of each model at the benchmark's crop step in each train precision, every Function call recorded (by
    wrapping `apply`) with the C-ABI entries its forward reached: the set of calls is TABLE's, in every precision."""
    from speinet_amd import _lib, train as T
    calls, stack = {}, []
    orig_check = _lib.check

    def check(rc, what):
        if stack:
            stack[-1].add(what)
        return orig_check(rc, what)
    monkeypatch.setattr(_lib, "check", check)
    for op in KEYS:
        cls = getattr(T, op)

        def wrapped(*a, _op=op, _orig=cls.apply):
            key = call_key(_op, a)
            stack.append(set())
            try:
                return _orig(*a)
            finally:
                calls.setdefault(key, set()).update(stack.pop())
        monkeypatch.setattr(cls, "apply", wrapped)
    for which in ("swint", "speinet"):
        net, x = _bench_model(which)
        want = table_keys(which)
        for prec in PRECS:
            calls.clear()
            net.train_precision = prec
            net.zero_grad()
            torch.manual_seed(0)
            out = net(x)
            out.square().mean().backward()
            torch.cuda.synchronize()
            got = set(calls)
            print(f"\n  {which} {prec}: {len(got)} distinct calls")
            for k in sorted(got, key=str):
                print(f"    {k}: {sorted(calls[k])}")
            assert got == want, f"{which} {prec}: not in the table {sorted(got - want, key=str)}; not run {sorted(want - got, key=str)}"
        del net, x, out


# ---- 5. the references themselves (CPU) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,K,N,ks,stride", [(2, 9, 11, 3, 5, 5, 1), (1, 8, 7, 4, 6, 3, 1), (2, 6, 10, 5, 3, 1, 1),
                                                 (2, 9, 13, 4, 6, 5, 2), (1, 11, 7, 3, 4, 3, 2), (2, 10, 8, 4, 4, 1, 2)])
def test_tap_gemm_conv_reference_matches_conv2d(B, H, W, K, N, ks, stride):
    """conv_fwd64 / conv_dgrad64 / conv_wgrad64 (and the chunk shares of conv_wgrad64) = F.conv2d and its autograd, float64."""
    g = torch.Generator().manual_seed(B * 100 + H * 10 + ks + stride)
    x = torch.randn(B, K, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(N, K, ks, ks, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, stride=stride, padding=ks // 2)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    ho, wo = y.shape[2:]
    xr, dyr = _rows(x.detach()), _rows(dy)
    mine = conv_fwd64(xr, w.detach(), B, H, W, stride)
    halves = [torch.arange(0, B * ho * wo // 2), torch.arange(B * ho * wo // 2, B * ho * wo)]
    mdw, parts = conv_wgrad64(xr, dyr, ks, B, H, W, stride, halves)
    close = lambda a, b: torch.allclose(a, b, rtol=1e-12, atol=1e-12 * b.abs().max().item())
    assert close(mine, _rows(y.detach()))
    assert close(conv_dgrad64(dyr, w.detach(), B, H, W, stride), _rows(dx))
    assert close(mdw, dw) and close(parts[0] + parts[1], dw)


@pytest.mark.parametrize("B,H,W,K,N", [(2, 5, 7, 4, 3), (1, 6, 6, 3, 5)])
def test_tap_gemm_conv_transpose_reference_matches_conv_transpose2d(B, H, W, K, N):
    """convt_fwd64 and the ConvT2d gradients built from the Conv2d references (as case_convt2d uses them) = F.conv_transpose2d."""
    g = torch.Generator().manual_seed(B + H + W + K)
    x = torch.randn(B, K, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(K, N, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose2d(x, w, stride=2, padding=1, output_padding=1)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    xr, dyr = _rows(x.detach()), _rows(dy)
    close = lambda a, b: torch.allclose(a, b, rtol=1e-12, atol=1e-12 * b.abs().max().item())
    assert close(convt_fwd64(xr, w.detach(), B, H, W), _rows(y.detach()))
    assert close(conv_fwd64(dyr, w.detach(), B, 2 * H, 2 * W, 2), _rows(dx))
    assert close(conv_wgrad64(dyr, xr, 3, B, 2 * H, 2 * W, 2)[0], dw)
