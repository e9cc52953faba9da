/*
 * speinet_hip.h — C-ABI of the MI355X (gfx950) kernels behind SPEINet's per-sequence forward pass.
 *
 * The reference (yangt1013/SPEINet) is pure PyTorch: it has no FFI for this path, so this header *defines*
 * the boundary underneath the drop-in Python class (last row).  Each entry point names the
 * reference code it replaces (file:line relative to the reference tree).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch allocates; the library never
 *     allocates, frees or synchronises), every call is asynchronous on `stream`;
 *   - feature maps are NHWC fp32 ("pixel rows": [H][W][C], C contiguous) with an explicit row stride `ld*`
 *     in floats so channel-concatenated buffers are addressed in place; frames are NCHW fp32 planes;
 *   - packed weights are [tap][Cout][Cin] fp32 (speinet_amd/pack.py builds them once per checkpoint);
 *   - return 0 on success, <0 on error: -1 bad argument / unsupported shape, -2 launch failure; the text
 *     is available from spei_last_error() (thread local).
 */
#ifndef SPEINET_HIP_H
#define SPEINET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* spei_stream_t; /* hipStream_t */

#define SPEI_ACT_NONE 0
#define SPEI_ACT_RELU 1
#define SPEI_ACT_GELU 2 /* exact erf GELU (nn.GELU default, reference model/swinir.py:14-19) */

/* Element formats.  16-bit entry points take `fmt` = SPEI_BF16 or SPEI_F16: the operand type of the matrix pipe
 * (v_mfma_f32_32x32x16_bf16 / _f16, same rate, fp32 accumulation; half keeps 11 significand bits instead of 8 at a
 * range of +-65504).  `*_fmt` arguments say how a tensor is stored in HBM: SPEI_F32 or the call's 16-bit format. */
#define SPEI_F32 0
#define SPEI_BF16 1
#define SPEI_F16 2

#define SPEI_CONV 0
#define SPEI_CONV_TRANSPOSED 1 /* ConvTranspose2d(k, stride, pad=k/2, output_padding=stride-1) */

int spei_version(void);
const char* spei_last_error(void);
const char* spei_arch(void); /* "gfx950" */

/* K15 — routing test `torch.all(x[:,3]==0)` (model/speinet.py:70-73).  flag[0] := 1 if any element != 0. */
int spei_any_nonzero(const float* x, int64_t n, int32_t* flag, spei_stream_t stream);

/* K1 — r_l_per_channel(img, box5/25, iters, lam) (model/rcl.py:22-51).  img/out: [C][H][W]; scratch same size. */
int spei_rl_prior(const float* img, float* out, float* scratch, int C, int H, int W, int iters, float lam,
                  spei_stream_t stream);

/* K2 head — first conv 5x5 pad 2, Cin=3 NCHW planes -> NHWC [H][W][Cout], +bias, ReLU
 * (model/recons_video_ori.py:28-32).  w: [25][Cout][3] packed, Cout == 32. */
int spei_conv5_in(const float* img_chw, const float* w, const float* bias, float* out_hwc, int H, int W,
                  int Cout, spei_stream_t stream);

/* K2 tail — last conv 5x5 pad 2, NHWC [H][W][32] -> NCHW [3][H][W], +bias, no activation
 * (model/recons_video_ori.py:75-77).  w: [25][3][Cin] packed. */
int spei_conv5_out(const float* in_hwc, int ldi, const float* w, const float* bias, float* out_chw, int H,
                   int W, int Cin, spei_stream_t stream);

/* K2/K4/K5/K6/K9 — implicit-GEMM convolution / linear on f32 MFMA:
 *   out[m][n] = epi( sum_t sum_k A[src(m,t)][k] * w[t][n][k] ),  m = oy*Wout+ox, k over cat(a0[:, :k0], a1[:, :k1])
 *   epi(v) = (act(v + bias[n])) * rowscale[m] + residual[m][n]      (rowscale / residual optional)
 * Replaces nn.Conv2d / nn.ConvTranspose2d / nn.Linear call sites: model/block.py:26-47, model/swinir.py:18-29,
 * 105-108,467,667,716,742, model/speinet.py:55-66,93-119, model/recons_video_ori.py:44-71.
 * Constraints: k0, k1 multiples of 32; N multiple of 32; lda*, ldo, ldr multiples of 4. */
int spei_igemm_f32(const float* a0, int lda0, int k0, const float* a1, int lda1, int k1, const float* w,
                   const float* bias, float* out, int ldo, const float* residual, int ldr,
                   const float* rowscale, int Hin, int Win, int Hout, int Wout, int N, int ksize, int stride,
                   int pad, int mode, int act, spei_stream_t stream);

/* The same on `batch` equally sized maps stored one after the other (a0 / a1 / out / residual rows and rowscale entries of sample b
 * start at b * map size): one launch, blockIdx.z = sample (the training step's batches of 200x200 crops give single maps of only
 * 2 500 .. 40 000 pixels — a launch per sample leaves most of the chip idle). */
int spei_igemm_f32_batched(const float* a0, int lda0, int k0, const float* a1, int lda1, int k1, const float* w,
                           const float* bias, float* out, int ldo, const float* residual, int ldr,
                           const float* rowscale, int Hin, int Win, int Hout, int Wout, int N, int ksize, int stride,
                           int pad, int mode, int act, int batch, spei_stream_t stream);

/* Same contract for SPEI_CONV (stride 1/2) and linears on the 16-bit matrix pipe (v_mfma_f32_32x32x16_bf16 / _f16, fp32
 * accumulate), bf16 or half operands (`fmt`), slab-resident: the
 * input tile + halo is staged once into LDS as 16-bit and the weights stream from HBM/L2 in MFMA fragment order
 * (wfrag: [N/32][tap][K/16][64][8] 16-bit, see speinet_amd/pack.py).  Linears: pass Hin = Hout = M, Win = Wout = 1.
 * a_fmt / out_fmt: the activations (both sources) / the output are stored as fp32 or as `fmt` in HBM — 16-bit for
 * tensors that only feed the next GEMM or the attention kernel; residual, rowscale and bias stay fp32.
 * wfrag_lo == NULL: one 16-bit product per MAC ("bf16" / "f16"); wfrag_lo != NULL: the split product al*wh + ah*wl + ah*wh
 * ("bf16x3", f32-grade at 3/16 of the f32 MFMA cost; SPEI_BF16 with fp32 activations only).
 * ln_input: LayerNorm(256) without affine (model/swinir.py:244, affine folded into the weights) is applied to each
 * 256-wide fp32 input row while it is staged, so the normalised tokens never exist in HBM. */
int spei_conv_slab16(int fmt, const void* a0, int lda0, int k0, const void* a1, int lda1, int k1, int a_fmt,
                     const void* wfrag_hi, const void* wfrag_lo, const float* bias, void* out, int ldo, int out_fmt,
                     const float* residual, int ldr, const float* rowscale, int Hin, int Win, int Hout, int Wout,
                     int N, int ksize, int stride, int pad, int act, int ln_input, spei_stream_t stream);

/* The same convolution on `batch` dense maps in ONE launch (gridDim.y = map): the frame's 7 encoder passes go through every layer of
 * model/recons_video_ori.py:26-56 with the same weights (model/speinet.py:82-83,125-131).  a0 [batch][Hin*Win][k0], out
 * [batch][Hout*Wout][N], fp32 or `fmt` each; wfrag_lo != NULL: the split (bf16x3) form on fp32 maps (the training step's forward and
 * data-gradient convolutions, speinet_amd/train.py); residual: NULL or [batch][Hout*Wout][N] fp32, added in the epilogue.  Per map the tiles and the arithmetic are those of
 * spei_conv_slab16 (bit-identical results); a launch has batch x the workgroups (several resident rounds instead of half of one at
 * H/4) and a frame needs 1/batch of the launches. */
int spei_conv_slab16_batched(int fmt, const void* a0, int k0, int a_fmt, const void* wfrag, const void* wfrag_lo, const float* bias,
                             void* out, int out_fmt, const float* residual, int batch, int Hin, int Win, int Hout, int Wout, int N,
                             int ksize, int stride, int pad, int act, spei_stream_t stream);

/* 32 -> 32 channel 5x5 convolution (stride 1, zero padding 2), weight-stationary (round 4, csrc/conv32_ws16.hip): the two convs of a
 * ResBlock at full resolution (model/block.py:26-47,127-131 in model/recons_video_ori.py:26-43 inBlock and :72-75 outBlock) — every wave
 * keeps the layer's 50 weight fragments in registers for the whole launch, one persistent workgroup per CU walks over 16 x 32 pixel
 * tiles of all `batch` maps and double-buffers the tiles' slabs in LDS.  a: [batch][H*W][32] fp32 or `fmt`; wfrag: the layer's weights
 * in fragment order (as spei_conv_slab16 takes them); bias [32] or NULL; out: [batch][H*W][32] `fmt` or fp32, must not be `a`;
 * act: SPEI_ACT_NONE / SPEI_ACT_RELU.  Same operand rounding as spei_conv_slab16, fp32 sums in (tap, channel) order. */
int spei_conv32_ws16(int fmt, const void* a, int a_fmt, const void* wfrag, const float* bias, void* out, int out_fmt, int batch,
                     int H, int W, int act, spei_stream_t stream);

/* 64 -> 64 channel 5x5 convolution (stride 1, zero padding 2), weight-stationary (csrc/conv64_ws16.hip): the two convs of a ResBlock at
 * half resolution (model/block.py:26-47,127-131) — the four waves of a workgroup hold the layer's 200 weight fragments between them
 * (wave w: output channels [32 (w >> 1), +32), input-channel half w & 1) in registers for the whole launch, one persistent workgroup per CU
 * walks over 6 x 32 pixel tiles of all `batch` maps, double-buffers the tiles' slabs in LDS and adds the two input-channel halves through
 * LDS.  a: [batch][H*W][64] fp32 or `fmt`; wfrag: the layer's weights in fragment order (as spei_conv_slab16 takes them); bias [64] or
 * NULL; out: [batch][H*W][64] `fmt` or fp32, must not be `a`; act: SPEI_ACT_NONE / SPEI_ACT_RELU.  Same operand rounding as
 * spei_conv_slab16, fp32 sums in (tap, channel) order per input-channel half, then half 0 + half 1 + bias. */
int spei_conv64_ws16(int fmt, const void* a, int a_fmt, const void* wfrag, const float* bias, void* out, int out_fmt, int batch,
                     int H, int W, int act, spei_stream_t stream);

/* Fused Swin MLP branch (model/swinir.py:12-29 Mlp.forward + the `x + mlp(norm2(x))` tail of :279), 16-bit matrix pipe:
 * out = x + fc2(GELU(fc1(LayerNorm256(x)))), LayerNorm affine folded into w1/b1 (pack.py); w*_frag in MFMA fragment
 * order; the normalised tokens and the 512-wide hidden activations live only in LDS.  x, out: [M][256] fp32, may alias. */
int spei_mlp_fused16(int fmt, const float* x, float* out, const void* w1_frag, const float* b1, const void* w2_frag,
                     const float* b2, int64_t M, spei_stream_t stream);

/* ConvTranspose2d(k = 3, stride 2, padding 1, output_padding 1) on the slab kernel (reference model/recons_video_ori.py:58-71,
 * the tails of decoder_second / decoder_first): the four output-parity classes are stride-1 convolutions over the input
 * grid with 1 / 2 / 2 / 4 taps, written with pixel stride 2.  wfrag<py><px>: fragment-ordered 16-bit weights of class
 * (oy % 2, ox % 2) (speinet_amd/pack.py).  a0 [Hin*Win][lda0] fp32 or `fmt`, out [2Hin*2Win][ldo] fp32 or `fmt`. */
int spei_convt2_slab16(int fmt, const void* a0, int lda0, int k0, int a_fmt, const void* wfrag00, const void* wfrag01,
                       const void* wfrag10, const void* wfrag11, const float* bias, void* out, int ldo, int out_fmt,
                       int Hin, int Win, int N, int act, spei_stream_t stream);

/* The same transposed conv in split (bf16x3, f32-grade) arithmetic: fp32 in, fp32 out; whi4 / wlo4: the four class weights (order (0,0),
 * (0,1), (1,0), (1,1)) as bf16 high halves and low halves (= bf16(w - hi)) in fragment order.  Replaces the round-1 igemm path for the
 * ConvTranspose2d that ends decoder_second inside an f16 frame's split stages (model/recons_video_ori.py:59-70, model/speinet.py:99). */
int spei_convt2_slab16x3(const float* a0, int lda0, int k0, const void* const* whi4, const void* const* wlo4, const float* bias,
                         float* out, int ldo, int Hin, int Win, int N, int act, spei_stream_t stream);

/* 3x3 convolution 256 -> 256 channels (stride 1, padding 1) on a batch of fp32 token maps: the `conv(blocks(x)) + x` tail of every
 * residual Swin group and conv_after_body (reference model/swinir.py:467,483-484,742) as a persistent, software-pipelined kernel — one
 * workgroup per CU walks 6 x 16 pixel tiles, every weight fragment feeds three MFMAs, the next tile's halo is staged inside the
 * current tile's 144 k-steps (round 4; conv_slab_kernel took 190 us per launch for the frame's two maps).  x, out, residual (or NULL;
 * may alias out): [batch][H*W][256] fp32, x != out; w_frag: fragment-ordered 16-bit weights [8][9][16][64][8] (pack.py); bias [256] or
 * NULL.  H % 6 == 0, W % 16 == 0, H*W <= 2^21. */
int spei_conv3x3_256_pipe16(int fmt, const float* x, const void* w_frag, const float* bias, const float* residual, float* out,
                            int batch, int H, int W, spei_stream_t stream);

/* Last conv (model/recons_video_ori.py:75-77: 5x5, 32 -> 3 channels, NHWC in, three NCHW fp32 planes out) on the
 * slab kernel: wfrag = fragment-ordered weights zero-padded to 32 output channels, bias32 = bias padded to 32. */
int spei_conv5_out_slab16(int fmt, const void* in, int ldi, int in_fmt, const void* wfrag, const float* bias32, float* out_chw,
                          int H, int W, spei_stream_t stream);

/* Fused attention branch of a Swin block (model/swinir.py:238-278 + :115-149): out = x + proj(W-MSA(q = yhat Wq,
 * [k,v] = LayerNorm(x) Wkv)) with cyclic shift `shift`, 5x5 windows, 8 heads; x,out [H*W][256] fp32 (may alias), yhat
 * [H*W][256] `fmt` (LayerNorm of y without affine); w*_frag in MFMA fragment order with the LayerNorm affine and the q
 * scale folded in (pack.py); relbias [8][25][25].  q, k, v, the attention matrix and its output never reach HBM. */
int spei_attn_fused16(int fmt, const float* x, float* out, const void* yhat, const void* wq_frag, const float* bq,
                      const void* wkv_frag, const float* bkv, const void* wproj_frag, const float* bproj,
                      const float* relbias, int H, int W, int shift, spei_stream_t stream);

/* The same attention branch (model/swinir.py:238-278, :115-149) over a BATCH of equally sized maps that share the block's weights
 * — the two Swin calls of a frame, model/speinet.py:84 — in one launch, four windows per 256-thread workgroup (round 4): every
 * weight fragment fetched from L2 feeds four MFMAs instead of two, one 100-row token slab per workgroup (y-hat, then LayerNorm(x),
 * then the attention output) so that two workgroups still share a CU.  x, out: [batch][H*W][256] fp32 (may alias), yhat
 * [batch][H*W][256] `fmt`; weights, biases, relbias as spei_attn_fused16.  Per map the result differs from spei_attn_fused16 in
 * fp32 rounding only (the residual enters the projection sum first instead of last). */
int spei_attn_win4_16(int fmt, const float* x, float* out, const void* yhat, const void* wq_frag, const float* bq,
                      const void* wkv_frag, const float* bkv, const void* wproj_frag, const float* bproj,
                      const float* relbias, int batch, int H, int W, int shift, spei_stream_t stream);

/* Harness metrics of one deblurred frame (inference_SPEINet.py:484-500 calc_PSNR, :502-543 calc_SSIM): result[0] = PSNR, result[1] =
 * SSIM of out_hwc (the uint8 frame of spei_frame_u8_out) against gt_hwc, both [H][W][3] uint8, on the region cropped by `border` pixels
 * on every side (the reference crops 4).  PSNR from the exact integer squared error (inf for identical frames); SSIM: 11x11 Gaussian
 * window (sigma 1.5), valid region, float64 sums, mean over channels and positions.
 * ws: spei_frame_metrics_ws_doubles(H, W, border) doubles (-1: the cropped frame is smaller than the window). */
int64_t spei_frame_metrics_ws_doubles(int H, int W, int border);
int spei_frame_metrics(const unsigned char* out_hwc, const unsigned char* gt_hwc, int H, int W, int border, double* ws, double* result,
                       spei_stream_t stream);

/* K3 — ResBlock gates (model/block.py:8-24 SE, 71-96 ZPool+AttentionGate1/2, 108-124 TripletAttention).
 * x1: conv2 output [H][W][C] stored as x1_fmt (SPEI_F32 / SPEI_BF16 / SPEI_F16).  Workspace `ws` floats: spei_gate_ws_floats(H,W,C).
 * Produces s[C], g1[H][C], g2[W][C] such that ResBlock = x + x1*s + (x1*g1 + x1*g2).
 * gate params (packed by speinet_amd/pack.py): se_w1[C/4][C], se_b1[C/4], se_w2[C][C/4], se_b2[C],
 * cw_w[2][7][7], cw_bn[2] = {scale, shift}, hc_w[2][5][5], hc_bn[2]. */
int64_t spei_gate_ws_floats(int H, int W, int C);
int spei_resblock_gates(const void* x1, int x1_fmt, int H, int W, int C, const float* se_w1, const float* se_b1,
                        const float* se_w2, const float* se_b2, const float* cw_w, const float* cw_bn,
                        const float* hc_w, const float* hc_bn, float* s, float* g1, float* g2, float* ws,
                        spei_stream_t stream);
/* out = x + x1*s + (x1*g1 + x1*g2) [+ extra]   (model/block.py:136-140; `extra` fuses speinet.py:84,132) */
int spei_resblock_apply(const float* x, const void* x1, int x1_fmt, const float* s, const float* g1, const float* g2,
                        const float* extra, float* out, int ldo, int H, int W, int C, spei_stream_t stream);

/* spei_resblock_gates / spei_resblock_apply on `batch` dense maps in one launch each (gridDim.y = map): x1 [batch][H*W][C];
 * s [batch][C], g1 [batch][H][C], g2 [batch][W][C]; ws: batch x spei_gate_ws_floats(H, W, C) floats; x, out [batch][H*W][C] fp32.
 * Per map the arithmetic (and every partial-sum order) is that of the single-map entry points. */
int spei_resblock_gates_batched(const void* x1, int x1_fmt, int batch, int H, int W, int C, const float* se_w1, const float* se_b1,
                                const float* se_w2, const float* se_b2, const float* cw_w, const float* cw_bn, const float* hc_w,
                                const float* hc_bn, float* s, float* g1, float* g2, float* ws, spei_stream_t stream);
int spei_resblock_apply_batched(const float* x, const void* x1, int x1_fmt, const float* s, const float* g1, const float* g2, float* out,
                                int batch, int H, int W, int C, spei_stream_t stream);

/* The batched apply with a route per launched map instead of one dense fp32 output (the hand-offs between the encoder stacks).  Route i
 * computes x' = x + x1*s + (x1*g1 + x1*g2) of map `src` — plus x' of map `partner` when partner >= 0 (speinet.py:84,132: the pair
 * sums enc(RL(x)) + enc(x); a partner needs no route of its own) — and writes it to `out32` (fp32, row stride `ld32` floats; NULL: not
 * written) and / or, rounded to `fmt`, to `out16` (dense [H*W][C]; NULL: not written).  x' is evaluated exactly as by
 * spei_resblock_apply, so out32 holds that entry point's bits (with `extra` = the partner's x') and out16 their rounding.  The
 * routes are read on the host during the call (at most SPEI_APPLY_MAX_ROUTES) and travel to the kernel by value. */
#define SPEI_APPLY_MAX_ROUTES 16
typedef struct {
    float* out32;
    void* out16;
    int32_t ld32;
    int32_t src;
    int32_t partner; /* -1: none */
    int32_t reserved;
} SpeiApplyRoute;
typedef struct {
    SpeiApplyRoute r[SPEI_APPLY_MAX_ROUTES];
} SpeiApplyRoutes;
int spei_resblock_apply_routed(int fmt, const float* x, const void* x1, int x1_fmt, const float* s, const float* g1, const float* g2,
                               const SpeiApplyRoute* routes, int nroutes, int batch, int H, int W, int C, spei_stream_t stream);

/* K7 — LayerNorm over C=256, eps 1e-5 (model/swinir.py:244-245,279,528-529,776).  gamma/beta may be NULL
 * (affine folded into the following linear by pack.py); out_fmt: y is fp32, or 16-bit when it only feeds a GEMM. */
int spei_layernorm256(const float* x, void* y, int out_fmt, const float* gamma, const float* beta, int64_t M,
                      spei_stream_t stream);
/* y = LayerNorm(LayerNorm(x) * gamma + beta) without affine, stored as out_fmt: the two spei_layernorm256 launches of the Swin entry
 * (patch-embed norm, then norm1 of the y side) with the first result held in registers; the same expressions in the same order. */
int spei_layernorm256_twice(const float* x, void* y, int out_fmt, const float* gamma, const float* beta, int64_t M,
                            spei_stream_t stream);

/* K8 — window attention core: cyclic shift, 5x5 partition, softmax(q k^T + relbias + shift mask) v, reverse
 * (model/swinir.py:115-149, 215-236, 250-275).  q [H*W][256] (scale folded), kv [H*W][512] (K then V, head major),
 * relbias [8][25][25] pre-gathered, out [H*W][256]; heads = 8, head_dim = 32, window 5.  io_fmt: q, kv and out
 * are fp32 or 16-bit in HBM (the arithmetic stays fp32 on the f32 MFMA). */
int spei_window_attention(const void* q, const void* kv, int io_fmt, const float* relbias, void* out, int H, int W,
                          int shift, spei_stream_t stream);
int spei_window_attention_batched(const void* q, const void* kv, int io_fmt, const float* relbias, void* out, int H, int W,
                                  int shift, int batch, spei_stream_t stream);   /* batch maps stored one after the other */

/* K10 — 1 / max(||unfold3x3(f)[p]||_2, 1e-12) per position (F.normalize, model/SearchTransfer.py:30-31). */
int spei_patch_invnorm(const float* f, int ldf, float* inv, int H, int W, int C, spei_stream_t stream);

/* K11 — fused correlation + max/argmax over the reference index j (model/SearchTransfer.py:33-34, 68-69):
 *   S[i] = max_j <P_ref[j], P_lr[i]> * inv_ref[j] * inv_lr[i],  arg[i] = lowest maximising j.
 * R is never materialised.  Workspace floats: spei_corr_ws_floats(Hl*Wl).  C must be 128. */
int64_t spei_corr_ws_floats(int64_t n_lr);
int spei_corr_argmax(const float* lr, int ldl, const float* ref, int ldr, const float* inv_lr,
                     const float* inv_ref, int Hl, int Wl, int Hr, int Wr, int C, float* S, int32_t* arg,
                     float* ws, spei_stream_t stream);

/* K11 on the 16-bit pipe.  spei_split16 converts a map once: hi = fmt(x), lo = fmt(x - hi) (lo may be NULL);
 * outputs are dense [M][C] 16-bit.  spei_corr_argmax_bf16 (tile-restaging form, bf16 only): lo pointers NULL -> single
 * bf16 products, else bf16x3. */
int spei_split16(int fmt, const float* x, int ld, void* hi, void* lo, int64_t M, int C, spei_stream_t stream);
int spei_corr_argmax_bf16(const void* lr_hi, const void* lr_lo, const void* ref_hi, const void* ref_lo,
                          const float* inv_lr, const float* inv_ref, int Hl, int Wl, int Hr, int Wr, int C, float* S,
                          int32_t* arg, float* ws, spei_stream_t stream);

/* Slab-resident form (C == 128): the query block and the streamed reference blocks live in LDS with their 1-pixel
 * halo, so the 3x3 unfold is LDS addressing, not memory traffic.  lo pointers: NULL, or (SPEI_BF16 only) the bf16x3 split. */
int spei_corr_slab16(int fmt, const void* lr_hi, const void* lr_lo, const void* ref_hi, const void* ref_lo,
                     const float* inv_lr, const float* inv_ref, int Hl, int Wl, int Hr, int Wr, int C, float* S,
                     int32_t* arg, float* ws, spei_stream_t stream);

/* Exact arg-max at 16-bit cost (ops.Ctx corr_precision "top2").  spei_corr_slab_top2_16: the slab kernel with single
 * 16-bit products keeping the TWO best candidates of every query: arg / arg2 (arg2 = -1: no second candidate) with their
 * approximate, un-normalised-by-inv_lr scores S / S2.  spei_corr_rescore then re-scores both candidates on the fp32 maps
 * with fp64 accumulation and overwrites S (= dot * inv_ref[j] * inv_lr[i], fp32) and arg (ties -> lowest index): the
 * winner no longer depends on 16-bit rounding (model/SearchTransfer.py:33-34 computes R in fp32).
 * Candidate scores: S / S2 carry a position tag in their low five or six mantissa bits (the score itself is truncated there).
 * Ties in a candidate pass (both forms): arg and arg2 are always two different positions holding the two best truncated scores, but
 * which of several positions of EQUAL truncated score is kept, and in which order, is implementation-defined — inside a tile the
 * tag orders them (a positive score goes to the lower position, a negative one to the higher), across tiles the forms differ.
 * Only spei_corr_rescore's output follows the lowest-index rule. */
int spei_corr_slab_top2_16(int fmt, const void* lr16, const void* ref16, const float* inv_lr, const float* inv_ref,
                           int Hl, int Wl, int Hr, int Wr, int C, float* S, int32_t* arg, float* S2, int32_t* arg2,
                           float* ws, spei_stream_t stream);
/* Diagonal-sliding form of the candidate pass (csrc/corr_diag16.hip) for a reference map at least as high as the query
 * map (Hr >= Hl: SearchTransfer's maps of one size, SelfTransfer's rotated landscape map): the score of (y, x) against
 * (y', x') is the sum of three row-against-row terms shared along the diagonal y' - y, so each term is computed once — a
 * third of the flops of model/SearchTransfer.py:33's bmm reach the matrix pipe, every score is still the full 9 C-term
 * fp32 sum.  Same outputs as spei_corr_slab_top2_16 (feed spei_corr_rescore); workspace floats:
 * spei_corr_diag_ws_floats(Hl, Wl, Hr, Wr). */
int64_t spei_corr_diag_ws_floats(int Hl, int Wl, int Hr, int Wr);
int spei_corr_diag_top2_16(int fmt, const void* lr16, const void* ref16, const float* inv_ref, int Hl, int Wl, int Hr, int Wr,
                           int C, float* S, int32_t* arg, float* S2, int32_t* arg2, float* ws, spei_stream_t stream);
int spei_corr_rescore(const float* lr, int ldl, const float* ref, int ldr, const float* inv_lr, const float* inv_ref,
                      int Hl, int Wl, int Hr, int Wr, int C, float* S, int32_t* arg, const float* S2, const int32_t* arg2,
                      spei_stream_t stream);

/* K12 — gather the best-matching reference patch and overlap-add (unfold -> bis -> fold / 9,
 * model/SearchTransfer.py:36-46).  scale s in {1,2,4}: patch 3s, stride s, pad s. */
int spei_gather_fold(const float* ref, int ldr, const int32_t* arg, float* out, int ldo, int H3, int W3,
                     int Hr3, int Wr3, int C, int s, spei_stream_t stream);

/* SelfTransfer's reference map x.transpose(2,3).flip(2) (model/SearchTransfer.py:60): [H][W][C] -> [W][H][C]. */
int spei_rot90(const float* in, int ldi, float* out, int H, int W, int C, spei_stream_t stream);

/* K13 — F.interpolate(mode='bicubic', align_corners=False), A=-0.75, scale s in {2,4}
 * (model/speinet.py:96,99,108,111,113; model/SearchTransfer.py:73,75).  act: SPEI_ACT_NONE, or SPEI_ACT_RELU applied to
 * the interpolated value — relu(conv1x1(up(x))) == relu(up(conv1x1(x) + b)) (both maps are linear, the bicubic weights
 * sum to 1), which the throughput mode uses to run those 1x1 convs at a quarter of the pixels. */
int spei_upsample_bicubic(const float* in, int ldi, float* out, int ldo, int H, int W, int C, int s, int act,
                          spei_stream_t stream);
/* The same with the output stored as out_fmt (SPEI_F32, SPEI_BF16 or SPEI_F16; `ldo` in elements): the interpolated (and rectified)
 * fp32 value rounded to nearest even, for maps whose only readers are operands of single-product 16-bit convs.  A 16-bit output
 * needs s == 2, C, ldi and ldo multiples of 4, `in` 16-byte and `out` 8-byte aligned. */
int spei_upsample_bicubic_fmt(const float* in, int ldi, void* out, int ldo, int out_fmt, int H, int W, int C, int s, int act,
                              spei_stream_t stream);

/* K14 — out = a + b over n floats. */
int spei_add(const float* a, const float* b, float* out, int64_t n, spei_stream_t stream);

/* ---- backward kernels: first slice of the training step (the reference obtains these from torch.autograd
 * inside trainer/trainer_swint_hsa_nsf.py:34-40 `loss.backward()`).  fp32, fixed-order reductions (bitwise reproducible).
 * The DATA gradient of a convolution is spei_igemm_f32(mode = SPEI_CONV_TRANSPOSED) on dY with w[t][k][n] = W[t][n][k]. ---- */

/* Weight (and bias) gradient of Conv2d(K -> N, k, stride, pad = k/2) (model/block.py:26-47, recons_video_ori.py:28-71):
 * dw[t][n][k] = sum_m dy[m][n] * x[src(m,t)][k], dbias[n] = sum_m dy[m][n] (dbias may be NULL).  x [Hin*Win][ldx] NHWC,
 * dy [Hout*Wout][ldy]; ws: spei_wgrad_ws_floats(...) floats.  N <= 256; K, N need not be multiples of 32. */
int64_t spei_wgrad_ws_floats(int Hout, int Wout, int N, int K, int ksize);
int spei_conv_wgrad_f32(const float* x, int ldx, const float* dy, int ldy, float* dw, float* dbias, float* ws, int Hin, int Win,
                        int Hout, int Wout, int N, int K, int ksize, int stride, int pad, spei_stream_t stream);

/* The same summed over `batch` equally sized maps stored one after the other (x: batch * Hin*Win rows, dy: batch * Hout*Wout rows):
 * one launch, one fixed-order reduction over all samples' pixels. */
int spei_conv_wgrad_f32_batched(const float* x, int ldx, const float* dy, int ldy, float* dw, float* dbias, float* ws, int Hin, int Win,
                                int Hout, int Wout, int N, int K, int ksize, int stride, int pad, int batch, spei_stream_t stream);

/* Training: a weight in the reference's layout (Conv2d [N][K][ks][ks] / Linear [N][K], fp32) -> the split pair
 * hi = bf16(w), lo = bf16(w - hi) in the slab kernels' fragment order, one launch.  mode 0: the forward GEMM weight
 * [tap][N][K]; mode 1: the stride-1 data-gradient weight (taps reversed, channel axes swapped: [tap][K][N]).  The
 * weights of a training step change every optimizer step (trainer/trainer_swint.py:39-44).  frag_lo == NULL: only
 * hi = bf16(w) (round to nearest even) is written — the single fragment of train_precision = "bf16". */
int spei_pack_split16(const float* w, int N, int K, int ksize, int mode, void* frag_hi, void* frag_lo, spei_stream_t stream);

/* The same weight / bias gradient with the products split on the 16-bit matrix pipe (a = ah + al in bf16: al*bh + ah*bl + ah*bh,
 * fp32 accumulation: 2^-16 relative per product; speinet_amd/train.py `train_precision = "bf16x3"`): three v_mfma_f32_32x32x16_bf16 per
 * 16 pixels where the fp32 kernel issues eight v_mfma_f32_32x32x2_f32.  Arguments, workspace and summation order as
 * spei_conv_wgrad_f32_batched. */
int spei_conv_wgrad_bf16x3_batched(const float* x, int ldx, const float* dy, int ldy, float* dw, float* dbias, float* ws, int Hin, int Win,
                                   int Hout, int Wout, int N, int K, int ksize, int stride, int pad, int batch, spei_stream_t stream);

/* The same weight gradient in single products (speinet_amd/train.py `train_precision = "bf16"`, the arithmetic of the reference's
 * main_SPEINet.py:12 `set_float32_matmul_precision('medium')`): dY and X rounded once to bf16 (round to nearest even), one
 * v_mfma_f32_32x32x16_bf16 per 16 pixels, fp32 accumulation; the bias gradient stays an fp32 column sum.  Replaces the weight
 * gradients of loss.backward() (trainer/trainer_swint.py:42) for every Conv2d / ConvTranspose2d / Linear.  Arguments, workspace,
 * partial layout and fixed summation order as spei_conv_wgrad_bf16x3_batched (bitwise reproducible). */
int spei_conv_wgrad_bf16_batched(const float* x, int ldx, const float* dy, int ldy, float* dw, float* dbias, float* ws, int Hin, int Win,
                                 int Hout, int Wout, int N, int K, int ksize, int stride, int pad, int batch, spei_stream_t stream);

/* Data gradient of a stride-2 Conv2d (k = 3 or 5, padding k / 2; model/recons_video_ori.py:40-56 encoder heads, whose
 * loss.backward() it replaces) on the slab kernel: the adjoint (transposed) convolution of dY [batch][Hin][Win][k0] fp32, split
 * into the four output-parity classes, each a stride-1 convolution over the dY grid with <= 9 taps, written with pixel stride 2
 * into out [batch][2Hin][2Win][N] fp32 (the caller crops an odd input size).  wfrag4: the fragment-ordered bf16 weights of the
 * classes (oy % 2, ox % 2) = 00, 01, 10, 11 (speinet_amd/train.py `_s2_adjoint_frags`): taps ky, kx with (p + pad - k) even,
 * ky-major.  Operands rounded once to bf16, fp32 accumulation. */
int spei_conv_s2_adjoint_slab16(const float* dy, int k0, const void* const* wfrag4, float* out, int N, int Hin, int Win, int ksize,
                                int batch, spei_stream_t stream);

/* ReLU backward on the output of a fused conv + ReLU: dz = dy where y > 0, else 0 (n floats, n % 4 == 0). */
int spei_relu_bwd(const float* y, const float* dy, float* dz, int64_t n, spei_stream_t stream);

/* Plane statistics of the ResBlock gates, training form (model/block.py:71-73 ZPool over W and over H, :8-24 SE pooling):
 * prod == 0: rowmax, rowmean [H][C] (over x), colmax, colmean [W][C] (over y), mean [C] of a [H][W][C], and the int32 arg-max of
 * each maximum: rowarg [H][C] the LOWEST x, colarg [W][C] the LOWEST y among the maximal elements (torch.max(dim)'s index, which
 * receives the maximum's whole gradient however many elements tie);
 * prod == 1: the plain sums of a * b over x, over y and over the map into rowmean / colmean / mean (rowmax = colmax = rowarg =
 * colarg = NULL): with a = dOut and b = x1 these are the gradients of g1, g2 and s of out = x + x1 * (s + g1 + g2).
 * ws: spei_plane_ws_floats(H, W, C) floats.  C in {32, 64, 128}. */
int64_t spei_plane_ws_floats(int H, int W, int C);
int spei_plane_stats(const float* a, const float* b, int prod, int H, int W, int C, float* rowmax, int* rowarg, float* rowmean,
                     float* colmax, int* colarg, float* colmean, float* mean, float* ws, spei_stream_t stream);

/* The same for `batch` equally sized maps stored one after the other (a, b: batch * H*W rows; outputs [batch][H][C], [batch][W][C],
 * [batch][C]); ws: batch * spei_plane_ws_floats(H, W, C) floats. */
int spei_plane_stats_batched(const float* a, const float* b, int prod, int H, int W, int C, float* rowmax, int* rowarg, float* rowmean,
                             float* colmax, int* colarg, float* colmean, float* mean, float* ws, int batch, spei_stream_t stream);

/* Backward of the gated residual sum through x1 (model/block.py:136-140): dx1 = dOut * (s + g1 + g2) + the pooled statistics'
 * gradients routed back (means spread evenly, each maximum's to its ONE arg-max element rowarg / colarg of spei_plane_stats).
 * dx = dOut needs no kernel. */
int spei_resblock_apply_bwd(const float* dout, const float* s, const float* g1, const float* g2, const int* rowarg, const int* colarg,
                            const float* d_rowmax, const float* d_rowmean, const float* d_colmax, const float* d_colmean,
                            const float* d_mean, float* dx1, int H, int W, int C, spei_stream_t stream);
/* The same for `batch` dense maps stored one after the other (and their statistics / gate maps likewise) in one launch. */
int spei_resblock_apply_bwd_batched(const float* dout, const float* s, const float* g1, const float* g2, const int* rowarg,
                                    const int* colarg, const float* d_rowmax, const float* d_rowmean, const float* d_colmax,
                                    const float* d_colmean, const float* d_mean, float* dx1, int batch, int H, int W, int C,
                                    spei_stream_t stream);

/* The gate maps of a ResBlock from its plane statistics, forward and backward, for the training step (model/block.py:8-24 SEBlock,
 * :49-68 BasicConv1 = 2->1 conv + BatchNorm2d(1), :75-96 AttentionGate1/2, :116-119 TripletAttention) — BatchNorm on batch statistics
 * with its running buffers moved (momentum 0.01, unbiased variance) when bn_train, on the running statistics otherwise:
 *   s [N][C] = sigmoid(W2 relu(W1 mean + b1) + b2);  g1 [N][H][C] = BN(conv7x7([rowmax, rowmean]));  g2 [N][W][C] = BN(conv5x5([colmax^T,
 *   colmean^T]))^T.   N = groups x B samples, BatchNorm statistics per group of B consecutive samples, running buffers moved once per
 * group in group order.  prm: HOST array of 10 device pointers se_w1 [C/4][C], se_b1, se_w2 [C][C/4], se_b2, cw_w [2][7][7], cw_g, cw_b,
 * hc_w [2][5][5], hc_g, hc_b; run: HOST array of 4 device pointers cw_rm, cw_rv, hc_rm, hc_rv (scalars).  saved
 * (spei_gate_train_saved_floats): what the backward needs (conv outputs, SE hidden layer, the statistics used); ws
 * (spei_gate_train_ws_floats floats, 8-byte aligned).  The backward returns the gradients of the five statistics and of the ten
 * parameters packed in prm order (spei_gate_train_nparams floats).  float64 sums in a fixed order: bitwise reproducible. */
int64_t spei_gate_train_saved_floats(int N, int groups, int H, int W, int C);
int64_t spei_gate_train_ws_floats(int N, int groups, int H, int W, int C);
int spei_gate_train_nparams(int C);
int spei_gate_maps_fwd(const float* rowmax, const float* rowmean, const float* colmax, const float* colmean, const float* mean,
                       const float* const* prm, float* const* run, int N, int groups, int H, int W, int C, int bn_train,
                       int update_running, float* s, float* g1, float* g2, float* saved, float* ws, spei_stream_t stream);
int spei_gate_maps_bwd(const float* rowmax, const float* rowmean, const float* colmax, const float* colmean, const float* mean,
                       const float* const* prm, float* const* run, int N, int groups, int H, int W, int C, int bn_train,
                       const float* s, const float* saved, const float* ds, const float* dg1, const float* dg2, float* d_rowmax,
                       float* d_rowmean, float* d_colmax, float* d_colmean, float* d_mean, float* dprm, float* ws,
                       spei_stream_t stream);

/* ---- backward of the cross-window-attention SwinIR blocks (model/swinir.py:238-281 under loss.backward(), the training step of
 * trainer/trainer_swint.py:34-44).  fp32; fixed-order reductions. ---- */

/* nn.LayerNorm(256) backward: dx [M][256] from x (the layer's input; mean / rstd are recomputed), gamma (NULL = no affine) and dy.
 * part [spei_ln_bwd_blocks(M)][2][256]: per-block partial sums of dgamma (= dy * xhat) and dbeta (= dy); the caller adds the
 * blocks in index order. */
int64_t spei_ln_bwd_blocks(int64_t M);
int spei_layernorm256_bwd(const float* x, const float* gamma, const float* dy, float* dx, float* part, int64_t M, spei_stream_t stream);

/* nn.GELU (erf form) on a saved pre-activation, and dpre = dy * gelu'(pre).  n floats, n % 4 == 0. */
int spei_gelu_fwd(const float* pre, float* out, int64_t n, spei_stream_t stream);
int spei_gelu_bwd(const float* pre, const float* dy, float* dpre, int64_t n, spei_stream_t stream);

/* WindowAttention core backward (model/swinir.py:115-149): q [H*W][256] pre-scaled, kv [H*W][512], relbias [8][25][25], dout
 * [H*W][256] = gradient of spei_window_attention's output -> dq [H*W][256], dkv [H*W][512] and dbias_part [nwin][8][25][25]
 * (the gradient of relbias is the sum over the windows).  Same window partition / cyclic shift / mask as the forward.  `batch`
 * equally sized maps stored one after the other are processed in one launch (dbias_part [batch][nwin][8][25][25]). */
int spei_window_attention_bwd(const float* q, const float* kv, const float* relbias, const float* dout, float* dq, float* dkv,
                              float* dbias_part, int H, int W, int shift, int batch, spei_stream_t stream);

/* Window attention for training in bf16 on the 16-bit matrix pipe (speinet_amd/train.py `train_precision = "bf16"`;
 * model/swinir.py:115-149 under train() mode and loss.backward()).  Forward: q, kv fp32 in HBM, rounded once to bf16 while staged,
 * S = Q K^T and O = P V each as two v_mfma_f32_32x32x16_bf16 per (window, head) (25 tokens padded to 32), softmax, relative bias and
 * shift mask in fp32, P rounded to bf16 as the second product's operand, out fp32.  Backward: P recomputed from q / k (never
 * stored); dP = dO V^T, dV = P^T dO, dQ = dS K, dK = dS^T Q on the same MFMA with P and dS rounded to bf16 as operands; dbias_part
 * holds the fp32 dS.  Arguments, layouts, mask, shift and the dbias_part layout as spei_window_attention_batched /
 * spei_window_attention_bwd. */
int spei_window_attention16_train(const float* q, const float* kv, const float* relbias, float* out, int H, int W, int shift, int batch,
                                  spei_stream_t stream);
int spei_window_attention16_bwd(const float* q, const float* kv, const float* relbias, const float* dout, float* dq, float* dkv,
                                float* dbias_part, int H, int W, int shift, int batch, spei_stream_t stream);

/* out[m][n] = x[m][n] * rowscale[m] (the DropPath factor of model/swinir.py:278-279 applied to a branch gradient).  N % 4 == 0. */
int spei_scale_rows(const float* x, const float* rowscale, float* out, int64_t M, int N, spei_stream_t stream);

/* ---- backward of SearchTransfer / SelfTransfer and the decoder glue (model/SearchTransfer.py:24-79, model/speinet.py:92-120 under
 * loss.backward(), trainer/trainer_swint_hsa_nsf.py:34-40).  Gather form, fixed summation order. ---- */

/* Gradient of S (the maximal normalised 3x3-patch correlation, spei_corr_argmax) with respect to the query map lr [H*W][C]:
 * dlr from dS [H*W], the forward's S / arg and the two inverse patch norms (spei_patch_invnorm).  C % 4 == 0. */
int spei_corr_s_bwd_lr(const float* lr, const float* ref, const float* inv_lr, const float* inv_ref, const float* S, const int32_t* arg,
                       const float* dS, float* dlr, int H, int W, int Hr, int Wr, int C, spei_stream_t stream);

/* Gradient with respect to a REFERENCE map at scale s in {1,2,4} ([Hr3*s * Wr3*s][C]): the adjoint of spei_gather_fold (dT
 * [H3*s * W3*s][C], or NULL) plus, at s == 1, the gradient of S through the reference patches (dS, or NULL; then ref / lr /
 * inv_lr / inv_ref / S are read).  order [H3*W3]: the queries sorted by arg (stable); start [Hr3*Wr3 + 1]: first entry of each
 * reference position's list. */
int spei_search_bwd_ref(const float* ref, const float* dT, const float* lr, const float* inv_lr, const float* inv_ref, const float* S,
                        const float* dS, const int32_t* order, const int32_t* start, float* dref, int H3, int W3, int Hr3, int Wr3,
                        int C, int s, spei_stream_t stream);

/* Adjoint of spei_upsample_bicubic (act NONE): dy [H*s * W*s][C] -> dx [H*W][C], s in {2,4}. */
int spei_upsample_bicubic_bwd(const float* dy, float* dx, int H, int W, int C, int s, spei_stream_t stream);

/* out[m] = sum_n a[m][n] * b[m][n] (the gradient of a per-row scale such as `* weight_S`, model/speinet.py:93). */
int spei_rowdot(const float* a, const float* b, float* out, int64_t M, int N, spei_stream_t stream);

/* Row a11 — LD sharpness detector features (inference_SPEINet.py:54-189).  spei_det_gray: [N][3][H][W] fp32 0..255 ->
 * gray [N][H][W] in 0..1 (ITU-R 601 weights).  spei_det_features: gray -> out [N][6] = LAP1, MIS3, WAV1, GRA7, STA3, DCT3
 * with window size k (odd; the reference uses 11 and sweeps 3..201).  ws: spei_det_ws_floats(N,H,W,k) floats.  k <= 11 sums each
 * k x k box of GRA7 / STA3 directly; k >= 13 takes running column sums and row prefix sums (cost independent of k). */
int spei_det_gray(const float* rgb, float* gray, int N, int H, int W, spei_stream_t stream);
int64_t spei_det_ws_floats(int N, int H, int W, int k);
int spei_det_features(const float* gray, float* out, float* ws, int N, int H, int W, int k, spei_stream_t stream);

/* ---- frame I/O of the clip API (speinet_amd/video.py; reference inference_SPEINet.py:466-482 numpy2tensor / tensor2numpy) ---- */

/* N uint8 [H][W][3] frames, frame_stride bytes apart (rows packed) -> dst fp32 [N][3][Hp][Wp], Hp / Wp = H / W rounded up to
 * multiples of 20, values u * (float)(1/255); the bottom / right pad reflects (torch F.pad mode "reflect": row H + j reads row
 * H - 2 - j), which needs Hp - H < H and Wp - W < W.  dst 16-byte aligned, or NULL.  gray (or NULL): [N][H][W], the detector's
 * gray plane of the unpadded frames, bit-identical to spei_det_gray on the frames as fp32 0..255.  dst and gray may not both be NULL. */
int spei_frames_u8_in(const unsigned char* src, int64_t frame_stride, float* dst, float* gray, int N, int H, int W, spei_stream_t stream);

/* fp32 [3][Hp][Wp] -> dst uint8 [H][W][3], the top-left crop (H <= Hp, W <= Wp) as round_half_even(clamp(x * 255, 0, 255)),
 * 0 for a non-finite value (reference inference_SPEINet.py:477-482 tensor2numpy).  nonfinite (or NULL): one int, cleared on the
 * stream, then nonzero iff the crop held a NaN or an infinity. */
int spei_frame_u8_out(const float* src, unsigned char* dst, int* nonfinite, int H, int W, int Hp, int Wp, spei_stream_t stream);

/* Pair statistics of consecutive frames, for the clip API's scene-cut rule (video.find_cuts; an extension beyond the reference): src =
 * N >= 1 uint8 [H][W][3] frames, frame_stride bytes apart (rows packed; the frame-size bound of spei_frames_u8_in); prev (or NULL): one
 * more packed frame, the one before frame 0.  On the integer luma Y = (77 R + 150 G + 29 B + 128) >> 8:
 * hist[n][64] = the number of pixels of frame n with Y >> 2 == b (each row sums to H * W); sad[p] = the sum over pixels of
 * |Y_a - Y_b| of consecutive pair p: N - 1 pairs, or N with prev, pair 0 then being (prev, frame 0).  N == 1 needs prev.  Both are
 * cleared on the stream first.  Integer arithmetic only: the result is exact, whatever the launch shape and the order of the sums. */
int spei_frame_pair_stats(const unsigned char* src, int64_t frame_stride, const unsigned char* prev, int N, int H, int W, int* hist,
                          int64_t* sad, spei_stream_t stream);

/* Deep frames: `depth` d = 10 or 12 bits per sample in little-endian 16-bit words, D = 2^d - 1; a word above D is read as D, so the
 * result is defined for all 65536 words.  frame_stride stays in BYTES and must be even; every uint16 pointer 2-byte aligned.
 * spei_frames_u16_in: as spei_frames_u8_in on N packed uint16 [H][W][3] frames, values (float)v * (float)(1.0 / D) (one float32
 *   multiply), the same reflect pad; gray (or NULL) is bit-identical to spei_det_gray on the frames as fp32 (float)v * (float)(255.0 / D):
 *   the focus measures see the usual 0..255 scale with the extra bits kept.
 * spei_frame_u16_out: as spei_frame_u8_out, dst packed uint16 [H][W][3] = round_half_even(clamp(x * D, 0, D)) in float32, 0 for a
 *   non-finite value; the same optional flag.
 * spei_frame_pair_stats_u16: as spei_frame_pair_stats on the d-bit luma Yd = (77 R + 150 G + 29 B + 128) >> 8: hist bin Yd >> (d - 6)
 *   (64 bins), sad over Yd (2^(d-8) times the 8-bit unit).  Integers throughout. */
int spei_frames_u16_in(const uint16_t* src, int64_t frame_stride, float* dst, float* gray, int N, int H, int W, int depth,
                       spei_stream_t stream);
int spei_frame_u16_out(const float* src, uint16_t* dst, int* nonfinite, int H, int W, int Hp, int Wp, int depth, spei_stream_t stream);
int spei_frame_pair_stats_u16(const uint16_t* src, int64_t frame_stride, const uint16_t* prev, int N, int H, int W, int depth, int* hist,
                              int64_t* sad, spei_stream_t stream);

/* ---- tile I/O of the clip API's large-frame mode (speinet_amd/tiles.py; the reference's forward_chop, inference_SPEINet.py:545-607,
 * is the 2x2 case) ----
 * A frame is deblurred as a grid of rows x cols (1..8 each) overlapping tiles of ONE shape th x tw, tile k = i * cols + j at rows
 * y0[i].. and columns x0[j].., and stitched with hard seams: tile (i, j) owns the band [yb[i], yb[i+1]) x [xb[j], xb[j+1]).  Every
 * `*_host` table is a HOST array, read during the call and passed to the kernel by value: it may be freed when the call returns.
 * A bad table (rows or cols out of range, a tile outside the frame, a band outside its tile, bands that do not span the frame)
 * returns non-zero before anything is launched.
 * spei_tiles_u8_in: src one packed uint8 [H][W][3] frame -> for every tile k, fp32 [3][thp][twp] at dst + k * tile_stride (floats;
 *   thp / twp = th / tw rounded up to multiples of 20; tile_stride >= 3 * thp * twp and a multiple of 4, dst 16-byte aligned),
 *   bit-identical to spei_frames_u8_in on the packed crop src[y0[i] : y0[i] + th][x0[j] : x0[j] + tw], its reflect pad included
 *   (which needs thp - th < th and twp - tw < tw).  One launch.
 * spei_tiles_u16_in: the same on a packed uint16 frame of `depth` 10 or 12, bit-identical to spei_frames_u16_in on the crop.
 * spei_tiles_u8_out: tiles_host = rows * cols device pointers to fp32 [3][thp][twp] (twp a multiple of 4) -> dst packed uint8
 *   [H][W][3]: pixel (y, x) of band (i, j) is spei_frame_u8_out's value of tile[i * cols + j][c][y - y0[i]][x - x0[j]].  nonfinite
 *   (or NULL): one int, cleared on the stream, then nonzero iff a pixel of a band (an OWNED pixel) was a NaN or an infinity; what
 *   a tile holds outside its band is never read.  One launch.
 * spei_tiles_u16_out: the same with spei_frame_u16_out's values for `depth` 10 or 12, dst packed uint16.
 * spei_tiles_u8_blend / spei_tiles_u16_blend: spei_tiles_u8_out / spei_tiles_u16_out with FEATHERED seams: the margins that two
 *   neighbouring tiles compute past their seam are blended over a ramp instead of being thrown away.  th, tw: the tile's real size
 *   (thp, twp must be th, tw rounded up to multiples of 20; th <= H, tw <= W); feather 0..200.  Per axis of n pixels, r tiles of real
 *   length t, origins o[0..r), band bounds b[0..r], the inner seam s = 1..r-1 lies at b[s] between tile s-1 and tile s, with the
 *   half-width
 *     f_s = max(0, min(feather, b[s] - o[s], o[s-1] + t - b[s],
 *                      (b[s] - b[s-1]) / 2 where s > 1, else b[1] - b[0],
 *                      (b[s+1] - b[s]) / 2 where s < r-1, else b[r] - b[r-1]))                         (integer division)
 *   (and b[s] - o[s-1], o[s] + t - b[s], which bind only in a table whose origins do not increase), so the ramp
 *   [b[s] - f_s, b[s] + f_s) lies on real pixels of both tiles, never on their reflect pad, and inside the two bands next to the
 *   seam: a band with seams on both sides gives each at most half of itself, a band at the frame's edge all of itself, so the ramps
 *   of an axis never overlap and none leaves the frame.  For every plan of tiles.tile_plan,
 *   f_s == feather whenever feather <= shave.  f_s == 0 is a hard seam.  A pixel p of the ramp of seam s has the low tile s-1, the
 *   high tile s and the weight
 *     w = fl32(fl32(2 * (p - b[s] + f_s) + 1) * fl32(1 / (4 f_s)))      (the reciprocal rounded once from double, on the host)
 *   which runs from 1 / (4 f) to (4 f - 1) / (4 f), symmetric about the seam, never 0 or 1.  In two dimensions the blend is
 *   separable: with a, b, c, d the values of the tiles (low row, low column), (low row, high column), (high row, low column), (high
 *   row, high column) at the pixel, v = lerp(lerp(a, b, wx), lerp(c, d, wx), wy) in float32 with lerp(lo, hi, w) = fma(w, hi - lo, lo),
 *   and the sample is spei_frame_u8_out's (u16_out's) value of v.  Outside a row ramp only a, b contribute, outside a column ramp
 *   only a, c; a pixel outside every ramp has the band's owner alone and is bit-identical to spei_tiles_u8_out's.  At most four
 *   tiles contribute to a pixel.  nonfinite: nonzero iff a CONTRIBUTING value of some pixel was a NaN or an infinity, and that pixel
 *   is 0; what no pixel reads (the rest of the margins, the reflect pad) may hold anything.  One launch. */
int spei_tiles_u8_in(const unsigned char* src, int H, int W, float* dst, int64_t tile_stride, const int* y0_host, const int* x0_host,
                     int rows, int cols, int th, int tw, spei_stream_t stream);
int spei_tiles_u16_in(const uint16_t* src, int H, int W, float* dst, int64_t tile_stride, const int* y0_host, const int* x0_host,
                      int rows, int cols, int th, int tw, int depth, spei_stream_t stream);
int spei_tiles_u8_out(const float* const* tiles_host, unsigned char* dst, int* nonfinite, int H, int W, const int* y0_host,
                      const int* x0_host, const int* yb_host, const int* xb_host, int rows, int cols, int thp, int twp,
                      spei_stream_t stream);
int spei_tiles_u16_out(const float* const* tiles_host, uint16_t* dst, int* nonfinite, int H, int W, const int* y0_host,
                       const int* x0_host, const int* yb_host, const int* xb_host, int rows, int cols, int thp, int twp, int depth,
                       spei_stream_t stream);
int spei_tiles_u8_blend(const float* const* tiles_host, unsigned char* dst, int* nonfinite, int H, int W, const int* y0_host,
                        const int* x0_host, const int* yb_host, const int* xb_host, int rows, int cols, int thp, int twp, int th, int tw,
                        int feather, spei_stream_t stream);
int spei_tiles_u16_blend(const float* const* tiles_host, uint16_t* dst, int* nonfinite, int H, int W, const int* y0_host,
                         const int* x0_host, const int* yb_host, const int* xb_host, int rows, int cols, int thp, int twp, int th, int tw,
                         int feather, int depth, spei_stream_t stream);

/* ---- field I/O of the clip API's interlaced mode (video.deblur_clip(..., fields="split"); an extension beyond the reference, which
 * knows progressive frames only) ----
 * A woven frame [H][W][3] of even height H holds two fields of H / 2 rows: field p (0 = top, 1 = bottom) is its rows p, p + 2, ...
 * (f[p::2]), the same W, the same depth.  Each parity is deblurred as a clip of its own, so a window runs as two parts of one shape,
 * hp x wp = H / 2 and W rounded up to multiples of 20.  Field order (top or bottom field first) does not enter.
 * spei_fields_u8_in: src one packed uint8 [H][W][3] frame -> for p = 0, 1 the fp32 planes [3][hp][wp] at dst + p * field_stride
 *   (floats; field_stride >= 3 * hp * wp and a multiple of 4, dst 16-byte aligned), bit-identical to spei_frames_u8_in on the packed
 *   copy of field p, its reflect pad included: the pad is the FIELD's, padded field row H / 2 + j reads field row H / 2 - 2 - j
 *   (frame row 2 (H / 2 - 2 - j) + p), which needs hp - H / 2 < H / 2 and wp - W < W.  One launch.
 * spei_fields_u16_in: the same on a packed uint16 frame of `depth` 10 or 12, bit-identical to spei_frames_u16_in on the field.
 * spei_fields_u8_out: top, bottom = the fp32 planes [3][hp][wp] of field 0 and field 1 -> dst packed uint8 [H][W][3]: row 2 r + p is
 *   row r of spei_frame_u8_out's H / 2 x W crop of plane p.  nonfinite (or NULL): one int, cleared on the stream, then nonzero iff a
 *   value of EITHER field's crop was a NaN or an infinity (that sample is 0); what a plane holds in its pad is never read.  One
 *   launch, every sample of dst written once.
 * spei_fields_u16_out: the same with spei_frame_u16_out's values for `depth` 10 or 12, dst packed uint16.
 * Non-zero before anything is launched: a null pointer, an odd H, a frame beyond the size bound of spei_frames_u8_in, a field that
 * cannot reflect-pad, planes smaller than the crop, a misaligned pointer or stride, an unknown depth. */
int spei_fields_u8_in(const unsigned char* src, int H, int W, float* dst, int64_t field_stride, spei_stream_t stream);
int spei_fields_u16_in(const uint16_t* src, int H, int W, float* dst, int64_t field_stride, int depth, spei_stream_t stream);
int spei_fields_u8_out(const float* top, const float* bottom, unsigned char* dst, int* nonfinite, int H, int W, int hp, int wp,
                       spei_stream_t stream);
int spei_fields_u16_out(const float* top, const float* bottom, uint16_t* dst, int* nonfinite, int H, int W, int hp, int wp, int depth,
                        spei_stream_t stream);

/* ---- geometric self-ensemble of the clip API (speinet_amd/ensemble.py, video.deblur_clip(..., ensemble=); the reference's
 * forward_x8, util/network_utils.py:308-341, which it never calls) ----
 * Member `op` in 0..7, the reference's enumeration: bit 0 reverses the columns of a plane (a[:, ::-1], its 'v'), bit 1 reverses the
 * rows (a[::-1, :], its 'h'), bit 2 transposes.  T_op applies them in that order, so T_op of an [H][W] plane is [W][H] for op & 4:
 *     T_op(a)[i][j] = a[fy(j)][fx(i)] for op & 4, else a[fy(i)][fx(j)],   fx(p) = op & 1 ? W - 1 - p : p,  fy(p) = op & 2 ? H - 1 - p : p
 * and T_op^-1 transposes first and then flips.  An ensemble of K in {1, 2, 4, 8} uses the members 0..K-1 (2: the frame and its mirror;
 * 4: the flips, one frame shape; 8: also the four transposed members).  With m_k = T_k^-1(model(T_k(x))) its result is
 *     R = fl32((((m_0 + m_1) + m_2) + ... + m_{K-1})) * 2^-log2 K
 * in float32: a sequential sum that starts from m_0 (not from 0.0) and an exact scale, so R is defined bit for bit wherever it is
 * finite and is NaN wherever that sum is NaN.
 * spei_planes_d4: plane p of dst (at dst + p * dst_stride, [H][W], or [W][H] for op & 4) = T_op of plane p of src (at src + p *
 *   src_stride, [H][W]); strides in floats, each at least H * W.  Values are copied as bits: NaN payloads and -0.0 survive.  Any
 *   H, W >= 1; 16-byte accesses on both sides where H, W and both strides are multiples of 4 and both bases 16-byte aligned, element
 *   by element otherwise.  Null pointers, an op outside 0..7, a stride smaller than a plane, and src and dst ranges that overlap
 *   return non-zero before anything is launched.  One launch, no workspace.
 * spei_d4_mean: members_host = K device pointers, ops_host = K ops: HOST arrays, read during the call and passed to the kernel by
 *   value.  Member k is a packed fp32 [C][H][W], or [C][W][H] where ops_host[k] & 4: T_op of its term.  dst packed [C][H][W] = R above
 *   with m_k = T_{ops_host[k]}^-1(member k), summed in TABLE order; K = 1 is the inverse transform alone, copied as bits.  The same
 *   alignment split (dst and every member 16-byte aligned).  K outside {1, 2, 4, 8}, an op outside 0..7, a null member and a dst
 *   that overlaps a member return non-zero before anything is launched.  One launch, no workspace, no atomics. */
int spei_planes_d4(const float* src, int64_t src_stride, float* dst, int64_t dst_stride, int64_t n_planes, int H, int W, int op,
                   spei_stream_t stream);
int spei_d4_mean(const float* const* members_host, const int* ops_host, int K, float* dst, int C, int H, int W, spei_stream_t stream);

/* ---- region of interest of the clip API (video.deblur_clip(..., roi=); an extension beyond the reference) ----
 * Only the rectangle [y0, y0 + h) x [x0, x0 + w) of every frame is deblurred (ingested by spei_tiles_u8_in / spei_tiles_u16_in with
 * a 1x1 table at (y0, x0)); the rest of the frame is the input's.  With D = 2^depth - 1,
 *     requant(v) = (min(v, D_in) * 2 * D_out + D_in) / (2 * D_in)          (integer division: v * D_out / D_in rounded half up)
 * is the input sample at the output depth, the identity where the depths are equal.
 * spei_roi_paste_u8: src = the model's fp32 [3][hp][wp], hp / wp = h / w rounded up to multiples of 20 (16-byte aligned); frame = the
 *   packed input frame [H][W][3] of in_depth 8 (uint8), 10 or 12 (little-endian 16-bit words, 2-byte aligned; a word above D_in reads
 *   as D_in); dst = the packed uint8 output frame [H][W][3].  ONE launch writes every sample of dst, in a single pass: outside the
 *   rectangle requant(frame), inside it, with feather == 0, spei_frame_u8_out's value of src[c][y - y0][x - x0]; with y0 = x0 = 0,
 *   h = H, w = W the result is bit-identical to spei_frame_u8_out's.  nonfinite (or NULL): one int, cleared on the stream, then
 *   nonzero iff a value of src inside the h x w crop was a NaN or an infinity; that sample is 0.  What src holds in its pad is never
 *   read.
 *   feather = N > 0 blends the model's output with the input over the N pixels inside every side of the rectangle that is not also a
 *   side of the frame (a side on the frame's border has no seam, so it gets no ramp).  Per axis a pixel at distance d = 0..N-1 from
 *   such a side has the weight
 *     wa = fl32(fl32(2 d + 1) * fl32(1 / (2 N)))                            (the reciprocal rounded once from double, on the host)
 *   and wa = 1 elsewhere; N <= min(200, h / 2, w / 2), so the two ramps of an axis never overlap.  With wt = fl32(wy * wx), m the
 *   model's value and o = fl32((float)min(v, D_in) * fl32(1 / D_in)) the input's, the sample is the egress quantisation
 *   (spei_frame_u8_out's) of fmaf(wt, m - o, o) where wt != 1, and of m itself where wt == 1: every pixel outside the ramps keeps
 *   the hard paste's bits.  The flag, and a 0 sample, follow m, not the blend's result.
 *   Non-zero before anything is launched: a null src, frame or dst; an in_depth outside {8, 10, 12}; a rectangle outside the frame or
 *   with h or w below 1; hp, wp not the rounded-up sizes; a feather outside 0..min(200, h / 2, w / 2); a dst that overlaps frame or src.
 * spei_roi_paste_u16: the same with a packed uint16 dst of `depth` 10 or 12 and spei_frame_u16_out's quantisation. */
int spei_roi_paste_u8(const float* src, const void* frame, int in_depth, unsigned char* dst, int* nonfinite, int H, int W, int y0, int x0,
                      int h, int w, int hp, int wp, int feather, spei_stream_t stream);
int spei_roi_paste_u16(const float* src, const void* frame, int in_depth, uint16_t* dst, int* nonfinite, int H, int W, int y0, int x0,
                       int h, int w, int hp, int wp, int feather, int depth, spei_stream_t stream);

/* A frame the clip API keeps (video.deblur_clip(..., sharp="keep"); an extension beyond the reference, which deblurs every frame):
 * the packed input frame [H][W][3] at the output depth, dst[i] = requant(src[i]) as defined above for every one of the 3 * H * W
 * samples; at equal depths a copy (a 16-bit word above D_in still reads as D_in).  src: in_depth 8 (bytes), 10 or 12 (little-endian
 * 16-bit words, 2-byte aligned); dst: out_depth 8, 10 or 12 likewise.  The frame is a flat run of independent samples: where both
 * bases are 16-byte aligned a thread moves the side with the wider samples as one 16-byte access and the other side as one access of
 * the same samples (16 samples for 8 -> 8 bits, 8 otherwise); element by element otherwise and behind the last whole run.  One
 * launch, no workspace, no atomics.  Non-zero before anything is launched: a null pointer; a depth outside {8, 10, 12}; H or W below
 * 1, or a frame beyond the size bound of spei_frames_u8_in; a deep pointer on an odd address; a dst that overlaps src. */
int spei_frame_requant(const void* src, int in_depth, void* dst, int out_depth, int H, int W, spei_stream_t stream);

/* A matte of the clip API (video.deblur_clip(..., matte=); an extension beyond the reference): an 8-bit mask [H][W] says how much of
 * the deblurred frame every pixel gets.  frame = the packed input frame [H][W][3] of in_depth 8 (bytes), 10 or 12 (little-endian
 * 16-bit words, 2-byte aligned; a word above D_in reads as D_in); deb = the packed deblurred frame [H][W][3] at the output depth (a
 * 16-bit word above D_out reads as D_out); matte = H * W bytes, one per pixel, rows packed.  With a = requant(frame sample) as
 * defined above, b = the sample of deb and m = the pixel's matte byte, or 255 - m where invert != 0, every one of the 3 * H * W
 * samples of dst is
 *     (a * (255 - m) + b * m + 127) / 255                                   (integer division; at most 4095 * 255 + 127)
 * so m = 0 gives a (spei_frame_requant's value), m = 255 gives b, a == b gives a for every m, and swapping a with b under the
 * inverted matte gives the same value.  dst == deb is allowed (in place: a thread reads the 4 pixels of its group from all three
 * sources before it writes them).  A group's 12 samples move as three words where W % 4 == 0 and the frame's base lies on a 4-byte
 * (8-byte for 16-bit samples) boundary, sample by sample otherwise; its 4 matte bytes as one dword where W % 4 == 0 and matte is
 * 4-byte aligned, byte by byte otherwise.  One launch, no workspace, no atomics.  Non-zero before anything is launched: a null
 * pointer; an in_depth outside {8, 10, 12}; H or W below 1, or 3 * H * W >= 2^31; 16-bit data on an odd address; a dst that overlaps
 * deb other than dst == deb, or that overlaps frame or matte.
 * spei_frame_matte_u16: the same with deb and dst packed uint16 of `depth` 10 or 12 (anything else is refused). */
int spei_frame_matte_u8(const void* frame, int in_depth, const unsigned char* deb, const unsigned char* matte, int invert,
                        unsigned char* dst, int H, int W, spei_stream_t stream);
int spei_frame_matte_u16(const void* frame, int in_depth, const uint16_t* deb, const unsigned char* matte, int invert, uint16_t* dst,
                         int H, int W, int depth, spei_stream_t stream);

/* Automatic blur mattes of the clip API (video.deblur_clip(..., matte="auto"), speinet_amd/blurmap.py; an extension beyond the
 * reference, so no reference code is cited): where in a frame is the picture blurred?  Integers throughout; tests/blurmap_ref.py is
 * the numpy statement.  src = N packed uint8 [H][W][3] frames, frame_stride bytes apart (rows packed), 1 <= N <= 65535.  The frame
 * is cut into cells of 16x16 pixels, ch = ceil(H / 16) by cw = ceil(W / 16); the edge cells are partial, n < 256 pixels.  On the
 * luma Y = (77 R + 150 G + 29 B + 128) >> 8 of spei_frame_pair_stats, taken at the clamped index outside the frame, per pixel
 *     horizontally  d = 9 * (Y(y,x) - Y(y,x-1)),  b = Y(y,x+4) - Y(y,x-5)    (b: the adjacent difference of two 9-tap box sums)
 *     vertically    d = 9 * (Y(y,x) - Y(y-1,x)),  b = Y(y+4,x) - Y(y-5,x)
 *     D = d * d,  V = max(0, d * d - b * b)
 * and per cell the four sums over its pixels, sums[N][ch][cw][4] = (sum D_h, sum V_h, sum D_v, sum V_v) as int64 (sums may be NULL).
 * A direction is textured iff sum D >= (81 * flat^2 * n) << (2 * (depth - 8)) and blurred iff textured and 256 * sum V < thr * sum D;
 * cells[N][ch][cw] is 255 where either direction is blurred and 0 elsewhere.  thr = 0 lights nothing; thr = 257 lights every
 * textured direction with sum D > 0.  One launch: a workgroup stages the luma of a strip of four cells and its halo in LDS, one wave
 * reduces one cell; no workspace, no atomics, exact whatever the launch order.  A group's 12 samples move as three words where
 * W % 4 == 0 and the base and the stride lie on a 4-byte (8-byte for 16-bit samples) boundary, sample by sample otherwise.
 * Non-zero before anything is launched: src or cells NULL; N outside 1..65535; H or W below 1, 3 * H * W >= 2^31 or more than 65535
 * rows of cells; N > 1 with a stride below one frame; thr outside 0..257; flat outside 0..255; sums off an 8-byte boundary; cells
 * or sums overlapping src or each other.
 * spei_blur_cells_u16: the same on uint16 frames of `depth` 10 or 12 (anything else is refused; frame_stride in BYTES and even, src
 * 2-byte aligned, a word above D reads as D), on the depth-bit luma.
 * spei_blur_matte: cells = n verdict maps [n][ch][cw] (1 <= n <= 8) for H x W frames -> matte[H][W], one byte per pixel.  The maps
 * are joined by their maximum, cell by cell (the hold over a window's frames), dilated by `grow` cells (0..4: the maximum over a
 * (2 * grow + 1)^2 neighbourhood, zeros outside the grid; cell_out[ch][cw], or NULL, receives this map), and interpolated between
 * cell centres: with u = 2 * y + 17, i0 = u / 32 - 1, i1 = i0 + 1 (both clamped into 0..ch-1), wy = u % 32, and j0, j1, wx from x
 * alike,
 *     m = ((32-wy) * (32-wx) * c[i0][j0] + (32-wy) * wx * c[i0][j1] + wy * (32-wx) * c[i1][j0] + wy * wx * c[i1][j1] + 512) / 1024
 * so an all-255 map gives 255 everywhere, an all-0 map 0, and the ramp between a lit and an unlit cell is 16 pixels wide.  One
 * launch (a workgroup first puts the dilated cells its 16x64 pixel tile needs into LDS); dword stores where W % 4 == 0 and matte is
 * 4-byte aligned, byte stores otherwise.  Non-zero before anything is launched: cells or matte NULL; n outside 1..8; grow outside
 * 0..4; H or W below 1 or H * W >= 2^31; matte or cell_out overlapping cells or each other. */
int spei_blur_cells_u8(const unsigned char* src, int64_t frame_stride, int N, int H, int W, int thr, int flat, unsigned char* cells,
                       int64_t* sums, spei_stream_t stream);
int spei_blur_cells_u16(const uint16_t* src, int64_t frame_stride, int N, int H, int W, int depth, int thr, int flat,
                        unsigned char* cells, int64_t* sums, spei_stream_t stream);
int spei_blur_matte(const unsigned char* cells, int n, int grow, int H, int W, unsigned char* matte, unsigned char* cell_out,
                    spei_stream_t stream);

/* The extent of the picture in N packed uint8 [H][W][3] frames, frame_stride bytes apart (rows packed; the frame-size bound of
 * spei_frames_u8_in), for the clip API's bar rule (video.find_bars): on the integer luma of spei_frame_pair_stats,
 * Y = (77 R + 150 G + 29 B + 128) >> 8, rowmax[y] (H ints) is the maximum of Y over row y of all N frames and colmax[x] (W ints) the
 * maximum over column x.  accumulate == 0 clears both on the stream first; otherwise the maxima join what is there, so a clip is
 * scanned batch by batch.  An integer maximum commutes: the result is exact, whatever the launch shape and the order of the updates.
 * spei_frame_extent_u16: the same on uint16 frames of `depth` 10 or 12 (frame_stride in BYTES and even, src 2-byte aligned, a word
 * above D reads as D), on the d-bit luma of spei_frame_pair_stats_u16. */
int spei_frame_extent(const unsigned char* src, int64_t frame_stride, int N, int H, int W, int* rowmax, int* colmax, int accumulate,
                      spei_stream_t stream);
int spei_frame_extent_u16(const uint16_t* src, int64_t frame_stride, int N, int H, int W, int depth, int* rowmax, int* colmax,
                          int accumulate, spei_stream_t stream);

/* ---- planar YUV frames of the clip API (speinet_amd/y4m.py, speinet_amd/video.py; an extension beyond the reference) ---- */

#define SPEI_YUV_420_CENTER 0 /* 4:2:0, chroma sample at the centre of its 2x2 block (y4m C420jpeg, and bare C420) */
#define SPEI_YUV_420_LEFT 1   /* 4:2:0, chroma co-sited with the even column, between the two rows (y4m C420mpeg2) */
#define SPEI_YUV_444 2        /* 4:4:4 (y4m C444) */
#define SPEI_YUV_422 3        /* 4:2:2, chroma co-sited with the even column of its own row (y4m C422, C422p10, C422p12) */
#define SPEI_YUV_MONO 4       /* the Y plane alone (y4m Cmono, Cmono10, Cmono12) */
#define SPEI_YUV_BT601 0
#define SPEI_YUV_BT709 1
#define SPEI_YUV_FULL 0    /* Y, U, V in 0..255 */
#define SPEI_YUV_LIMITED 1 /* Y in 16..235, U and V in 16..240 */

/* A planar frame is the Y plane [H][W], then U, then V: [ceil(H/2)][ceil(W/2)] each for 4:2:0, [H][W] each for 4:4:4; uint8, packed,
 * as in a y4m FRAME payload; H and W may be odd.  An RGB frame is packed uint8 [H][W][3] (what spei_frames_u8_in takes).
 * Integer arithmetic only, so the result is defined bit for bit.  Q14 coefficients, round(c * 16384), per (matrix, range):
 *                 yr    yg    yb |    ur    ug   ub |   vr    vg    vb | yo |    cy |    rv |    gu     gv |    bu
 *   601 full    4899  9617  1868 | -2765 -5427 8192 | 8192 -6860 -1332 |  0 | 16384 | 22970 | -5638 -11700 | 29032
 *   601 limited 4207  8260  1604 | -2428 -4768 7196 | 7196 -6026 -1170 | 16 | 19077 | 26149 | -6419 -13320 | 33050
 *   709 full    3483 11718  1183 | -1877 -6315 8192 | 8192 -7441  -751 |  0 | 16384 | 25802 | -3069  -7670 | 30402
 *   709 limited 2991 10064  1016 | -1649 -5547 7196 | 7196 -6536  -660 | 16 | 19077 | 29372 | -3494  -8731 | 34610
 * `>>` floors.  Clipping: RGB and full range to [0,255], limited range to [16,235] (Y) and [16,240] (U, V).
 *
 * spei_yuv_to_rgb_u8: src = N planar frames, frame_stride bytes apart -> dst = N packed RGB frames.  The chroma of a pixel is formed
 * times 16, U16 and V16, neighbour indices clamped to the plane: 4:4:4: 16 U[y][x].  4:2:0 rows, both sitings: j = y >> 1 and the
 * other row j - 1 (y even) or j + 1 (y odd), weights 3 : 1.  Columns, CENTER: the same with i = x >> 1.  Columns, LEFT: 4 : 0 at even
 * x, 2 : 2 of columns i and i + 1 at odd x.  With yy = cy * 16 * (Y - yo), u = U16 - 2048, v = V16 - 2048:
 *   R = clip((yy + rv v + 2^17) >> 18), G = clip((yy + gu u + gv v + 2^17) >> 18), B = clip((yy + bu u + 2^17) >> 18).
 * spei_rgb_u8_to_yuv: one packed RGB frame -> one planar frame.  Y = clip(((yr R + yg G + yb B + 2^13) >> 14) + yo) per pixel.
 * 4:4:4: U = clip(((ur R + ug G + ub B + 2^13) >> 14) + 128), V likewise.  4:2:0 CENTER: the same on the channel sums over rows 2j,
 * 2j + 1 and columns 2i, 2i + 1, with 2^15 and >> 16.  4:2:0 LEFT: on the sums over rows 2j, 2j + 1 of c[2i-1] + 2 c[2i] + c[2i+1],
 * with 2^16 and >> 17.  Indices clamped to the frame.  The 4:2:0 resampling is this project's own definition. */
int spei_yuv_to_rgb_u8(const unsigned char* src, int64_t frame_stride, unsigned char* dst, int N, int H, int W, int layout, int matrix,
                       int range, spei_stream_t stream);
int spei_rgb_u8_to_yuv(const unsigned char* src, unsigned char* dst, int H, int W, int layout, int matrix, int range,
                       spei_stream_t stream);

/* The same two conversions on deep samples: `depth` d = 10 or 12, s = d - 8, D = 2^d - 1, samples in little-endian 16-bit words (a
 * word above D is read as D); a planar frame and a packed RGB frame are laid out as above with uint16 elements, frame_stride in BYTES
 * (even), every pointer 2-byte aligned.  The rule that makes every row, exact rationals rounded to nearest (no value is an exact
 * half; at d = 8 it gives the table above): Kr, Kb = 0.299, 0.114 (BT.601) or 0.2126, 0.0722 (BT.709), Kg = 1 - Kr - Kb; full range
 * ly = lc = 1, yo = 0; limited range ly = 219 2^s / D, lc = 224 2^s / D, yo = 16 2^s; the chroma zero is 128 2^s in both ranges;
 *   yr = rnd(16384 Kr ly), yb = rnd(16384 Kb ly), yg = rnd(16384 ly) - yr - yb
 *   ub = vr = rnd(16384 lc / 2), ur = -rnd(16384 lc Kr / (2 (1 - Kb))), ug = -ub - ur, vb = -rnd(16384 lc Kb / (2 (1 - Kr))), vg = -vr - vb
 *   cy = rnd(16384 / ly), rv = rnd(16384 2 (1 - Kr) / lc), bu = rnd(16384 2 (1 - Kb) / lc),
 *   gu = -rnd(16384 2 Kb (1 - Kb) / (Kg lc)), gv = -rnd(16384 2 Kr (1 - Kr) / (Kg lc)).
 * Full range therefore reuses the 8-bit full rows at every depth.  Limited range:
 *                    yr    yg    yb |    ur    ug   ub |   vr    vg    vb |  yo |    cy |    rv |    gu     gv |    bu
 *   d 10 601 limited 4195  8236  1599 | -2421 -4754 7175 | 7175 -6008 -1167 |  64 | 19133 | 26226 | -6438 -13359 | 33148
 *   d 10 709 limited 2983 10034  1013 | -1644 -5531 7175 | 7175 -6517  -658 |  64 | 19133 | 29459 | -3504  -8757 | 34711
 *   d 12 601 limited 4192  8229  1598 | -2420 -4750 7170 | 7170 -6004 -1166 | 256 | 19147 | 26245 | -6442 -13369 | 33172
 *   d 12 709 limited 2981 10026  1012 | -1643 -5527 7170 | 7170 -6513  -657 | 256 | 19147 | 29480 | -3507  -8763 | 34737
 * Chroma up- and down-sampling are those of the 8-bit entries (3 : 1 rows, the CENTER and LEFT column rules, clamped indices, the
 * 16-fold U16 / V16, the box and [1 2 1] sums with their shifts).
 * spei_yuv_to_rgb_u16: yy = cy * 16 * (Y - yo), u = U16 - (2048 << s), v = V16 - (2048 << s),
 *   R = clip((yy + rv v + 2^17) >> 18, 0, D), G = clip((yy + gu u + gv v + 2^17) >> 18, 0, D), B = clip((yy + bu u + 2^17) >> 18, 0, D).
 *   These sums do NOT fit int32 at 12-bit limited range (|yy + rv v| reaches 2.3e9): they are taken in 64 bits.
 * spei_rgb_u16_to_yuv: the 8-bit expressions with `+ yo` and `+ (128 << s)` (the sums stay below 2.7e8); full range clips to [0, D],
 *   limited range to [16 2^s, 235 2^s] (Y) and [16 2^s, 240 2^s] (U, V). */
int spei_yuv_to_rgb_u16(const uint16_t* src, int64_t frame_stride, uint16_t* dst, int N, int H, int W, int layout, int matrix, int range,
                        int depth, spei_stream_t stream);
int spei_rgb_u16_to_yuv(const uint16_t* src, uint16_t* dst, int H, int W, int layout, int matrix, int range, int depth,
                        spei_stream_t stream);

/* 4:2:2 and mono frames: the four conversions above on layout = SPEI_YUV_422 or SPEI_YUV_MONO (any other layout is refused here, as
 * the four entries above refuse these two), with their arguments, checks, coefficient rows, clipping limits, yo, chroma zero and deep
 * rule (s = depth - 8, D = 2^depth - 1, a word above D reads as D; s = 0 and D = 255 for the u8 entries).  Indices are clamped to the
 * plane or frame.
 * SPEI_YUV_422: a planar frame is Y [H][W], then U, then V, [H][ceil(W/2)] each.  A chroma sample is co-sited with the even column of
 * its own row: no vertical subsampling, no siting option.
 *   YUV -> RGB, with i = x >> 1: even x: U16 = 16 U[y][i]; odd x: U16 = 8 (U[y][i] + U[y][i+1]); V likewise, then the R, G, B
 *   expressions above.  This is LEFT's column rule (4 : 0 at even x, 2 : 2 at odd x) without a row step.
 *   RGB -> YUV: Y per pixel as above.  Per row y and chroma column i, S_c = c[y][2i-1] + 2 c[y][2i] + c[y][2i+1] for each channel c,
 *   U = clip(((ur S_R + ug S_G + ub S_B + 2^15) >> 16) + (128 << s)), V likewise.  Every product and sum fits int32 (|sum| < 1.4e8
 *   at 12 bits).
 * SPEI_YUV_MONO: a planar frame is the Y plane [H][W] alone.
 *   YUV -> RGB: U16 = V16 = 2048 << s, so R = G = B = clip((cy * 16 * (Y - yo) + 2^17) >> 18, 0, D); `matrix` is checked and has no
 *   effect.
 *   RGB -> YUV: the Y expression alone, with the matrix's luma row.
 * Like the 4:2:0 rule, the 4:2:2 resampling is this project's own definition, not a bit-match of swscale. */
int spei_planar_to_rgb_u8(const unsigned char* src, int64_t frame_stride, unsigned char* dst, int N, int H, int W, int layout, int matrix,
                          int range, spei_stream_t stream);
int spei_rgb_u8_to_planar(const unsigned char* src, unsigned char* dst, int H, int W, int layout, int matrix, int range,
                          spei_stream_t stream);
int spei_planar_to_rgb_u16(const uint16_t* src, int64_t frame_stride, uint16_t* dst, int N, int H, int W, int layout, int matrix, int range,
                           int depth, spei_stream_t stream);
int spei_rgb_u16_to_planar(const uint16_t* src, uint16_t* dst, int H, int W, int layout, int matrix, int range, int depth,
                           spei_stream_t stream);

/* Interlaced frames (the clip API's fields="split"): the conversions above on a woven frame, any of the five layouts, with the
 * arguments and checks of the entries above.  Field p (0, 1) of a frame is a planar picture of its own: the Y rows p :: 2 and, for
 * 4:2:0, the chroma-plane rows p :: 2 (chroma row j of the frame's plane belongs to field j & 1), so a field of a 4:2:0 frame has
 * H / 2 luma and H / 4 chroma rows and H must be a multiple of 4 (anything else is refused with a message that names H).
 * spei_yuv_fields_to_rgb_u8 / _u16: the woven RGB frame whose rows p :: 2 are spei_yuv_to_rgb_u8 / _u16 applied to field p's picture:
 *   with r = y >> 1 the field row of frame row y, the 3 : 1 row rule takes field chroma rows j = r >> 1 and j - 1 (r even) or j + 1
 *   (r odd), clamped to 0 .. H / 4 - 1, which are the plane's rows 2 j + p: no chroma of one field reaches a row of the other.
 * spei_rgb_u8_to_yuv_fields / _u16: the planar frame whose field pictures are spei_rgb_u8_to_yuv / _u16 of the RGB rows p :: 2: Y per
 *   pixel; chroma-plane row 2 j + p from RGB rows 4 j + p and 4 j + p + 2.
 * 4:4:4, 4:2:2 and mono convert every row on its own: there the result is that of the progressive entries, bit for bit, any H. */
int spei_yuv_fields_to_rgb_u8(const unsigned char* src, int64_t frame_stride, unsigned char* dst, int N, int H, int W, int layout,
                              int matrix, int range, spei_stream_t stream);
int spei_rgb_u8_to_yuv_fields(const unsigned char* src, unsigned char* dst, int H, int W, int layout, int matrix, int range,
                              spei_stream_t stream);
int spei_yuv_fields_to_rgb_u16(const uint16_t* src, int64_t frame_stride, uint16_t* dst, int N, int H, int W, int layout, int matrix,
                               int range, int depth, spei_stream_t stream);
int spei_rgb_u16_to_yuv_fields(const uint16_t* src, uint16_t* dst, int H, int W, int layout, int matrix, int range, int depth,
                               spei_stream_t stream);

/* ---- training on a dataset (speinet_amd/data.py, speinet_amd/fit.py) ---- */

/* One output frame of a training batch: a P x P rectangle of one uint8 [H][W][3] frame on the device. */
#define SPEI_CROP_HFLIP 1 /* [:, ::-1] */
#define SPEI_CROP_VFLIP 2 /* [::-1, :] */
#define SPEI_CROP_ROT90 4 /* np.rot90: counter-clockwise, out[i][j] = in[j][P-1-i] */
#define SPEI_CROP_ZERO 8  /* the frame is all zeros; nothing is read */
typedef struct {
    uint64_t src;  /* device address of the frame's first byte */
    int32_t pitch; /* bytes from one row to the next (>= 3 W) */
    int32_t y0, x0; /* top-left corner of the rectangle */
    int32_t flags; /* SPEI_CROP_* */
    int32_t H, W;  /* the frame's size: the rectangle is checked against it on the host */
} spei_crop_record;

/* The batch the reference's loader builds per sample on its workers (util/utils.py:8-65 get_patch, np2Tensor, data_augment;
 * data/videodata_nfs.py:180-207 __getitem__), in one launch: record r < n_in -> input [n_in][3][P][P], record n_in + r -> gt
 * [n_gt][3][P][P], both fp32 and 16-byte aligned.  Value (float)u * (float)(rgb_range / 255), bit-identical to np2Tensor; geometry
 * in the reference's order: crop, hflip, vflip, rot90.  P % 4 == 0 (the reference's size_must_mode = 4 crop is then the identity).
 * table: n_in + n_gt records on the device; table_host: the same records in HOST memory, against which every rectangle is checked
 * before anything is launched (a record that leaves its frame is an error, never a kernel's fault). */
int spei_train_batch_u8(const spei_crop_record* table, const spei_crop_record* table_host, int n_in, int n_gt, float* input, float* gt,
                        int P, float rgb_range, spei_stream_t stream);

/* One output frame of a training batch made from SHARP footage (speinet_amd.data.SharpTrainLoader; an extension beyond the reference,
 * which precomputes its blurry sets): the P x P rectangle of the per-byte mean of `length` consecutive uint8 [H][W][3] frames.
 * sizeof(spei_run_record) == 48. */
typedef struct {
    uint64_t src;         /* device address of the first byte of the run's FIRST frame */
    int64_t frame_stride; /* bytes from one frame to the next (>= H * pitch unless length == 1) */
    int32_t pitch;        /* bytes from one row to the next (>= 3 W) */
    int32_t y0, x0;       /* top-left corner of the rectangle */
    int32_t flags;        /* SPEI_CROP_* */
    int32_t H, W;         /* the frames' size: the rectangle is checked against it on the host */
    int32_t length;       /* frames in the run, 1..15 */
    int32_t avail;        /* frames from src to the end of its clip (>= length) */
} spei_run_record;

/* spei_train_batch_u8 on runs: per byte of the rectangle u = floor(sum of that byte over the run's frames / length) in integer
 * arithmetic — the bytes of spei_window_mean_u8's blur[m] — then (float)u * (float)(rgb_range / 255); geometry, the zero flag, the
 * output layout and the arguments as spei_train_batch_u8.  A ground-truth record is a run of length 1 at the run's middle frame
 * (start + length / 2).  Every record is checked on table_host before anything is launched: flag bits, the rectangle inside its
 * frame, pitch, frame stride, 1 <= length <= 15, length <= avail. */
int spei_train_batch_runs_u8(const spei_run_record* table, const spei_run_record* table_host, int n_in, int n_gt, float* input, float* gt,
                             int P, float rgb_range, spei_stream_t stream);

/* The reference's validation metric (util/utils.py:81-92 calc_psnr, trainer/trainer_swint_hsa_nsf.py:73) on the model's FLOAT output,
 * unclamped and unquantised: a, b fp32 [3][H][W]; d = a / rgb_range - b / rgb_range in fp32 over rows and columns [shave, size - shave);
 * result[0] = the sum of d * d in float64 (fixed order), result[1] = the number of terms.  PSNR = 100 if the sum is 0, else
 * 20 log10(1 / sqrt(sum / count)).  ws: SPEI_PSNR_WS_DOUBLES doubles. */
#define SPEI_PSNR_WS_DOUBLES 256
int spei_psnr_f32(const float* a, const float* b, int H, int W, int shave, float rgb_range, double* ws, double* result,
                  spei_stream_t stream);

/* ---- making a data set from sharp footage (speinet_amd/blurset.py) ---- */

/* The reference's blur synthesis (LD_detector/mix_choice_dataset.py:46-71, :99-108; sharp_detector_params_estimation_parallel.py:50-76)
 * in one launch: src = T packed uint8 [H][W][3] frames, frame_stride bytes apart; runs = M pairs (start, length) of int32 on the
 * device, 1 <= length <= 15, start + length <= T; runs_host: the same pairs in HOST memory, checked before anything is launched.
 * Per run m: blur[m] = floor(sum of the run's frames / length) per byte (== np.mean -> float32 -> astype(uint8)), gt[m] = frame
 * start + length / 2, both uint8 [M][H][W][3] packed; gray (or NULL): [M][H][W] fp32, the detector's gray plane of blur[m],
 * bit-identical to spei_frames_u8_in's.  16-byte accesses when H * W % 16 == 0 and every pointer and the stride are 16-byte aligned. */
int spei_window_mean_u8(const unsigned char* src, int64_t frame_stride, int T, const int* runs, const int* runs_host, int M,
                        unsigned char* blur, unsigned char* gt, float* gray, int H, int W, spei_stream_t stream);

/* ---- blur synthesis in linear light (speinet_amd/light.py; an extension beyond the reference, whose scripts average code values) ---- */

/* A sensor integrates light and applies its transfer curve afterwards; the two entries below average a run in LINEAR light, in integer
 * arithmetic.  A light is 512 uint32 words, `tables` on the device and `tables_host` the same words in HOST memory: lin[256], then
 * thr[256], made once on the host in float64 from the light's forward transfer f with S = 2^24 - 1:
 *   lin[c] = rint(S f(c / 255))            the linear value of code c
 *   thr[c] = rint(S f((c - 0.5) / 255))    the linear value of the boundary between codes c - 1 and c (c >= 1; thr[0] is never read)
 * Valid iff lin[0] == 0, lin[255] <= S and lin[c-1] < thr[c] <= lin[c] for c = 1..255; then both tables increase strictly and
 * encode(lin[c]) == c.  Validity is checked on tables_host before anything is launched: a kernel never meets a table that could make
 * it misbehave.  Per byte position of a run of `length` frames:
 *   L    = floor(sum of lin[byte] over the run / length)     (the sum is at most 15 S < 2^28)
 *   blur = #{ c in 1..255 : thr[c] <= L }                     (the largest code whose lower boundary is at or below L)
 * A run of length 1 returns its bytes (encode(lin[c]) == c).  Everything else — gt, the gray plane of the ENCODED bytes, the checks of
 * runs_host, the access paths — is spei_window_mean_u8's. */
int spei_window_mean_light_u8(const unsigned char* src, int64_t frame_stride, int T, const int* runs, const int* runs_host, int M,
                              const uint32_t* tables, const uint32_t* tables_host, unsigned char* blur, unsigned char* gt, float* gray,
                              int H, int W, spei_stream_t stream);

/* spei_train_batch_runs_u8 with the run averaged in linear light: u = the blur byte defined above — the bytes of
 * spei_window_mean_light_u8's blur[m] — then (float)u * (float)(rgb_range / 255).  Records, geometry, the zero flag, the output
 * layout and every check of table_host as spei_train_batch_runs_u8; tables / tables_host as above. */
int spei_train_batch_runs_light_u8(const spei_run_record* table, const spei_run_record* table_host, int n_in, int n_gt,
                                   const uint32_t* tables, const uint32_t* tables_host, float* input, float* gt, int P, float rgb_range,
                                   spei_stream_t stream);

/* ---- sensor noise in blur synthesis (speinet_amd/light.py; an extension beyond the reference) ---- */

/* The mean of n frames carries 1 / n of one frame's noise variance.  The two entries below are the light entries above with that
 * noise added back in LINEAR light, between the average and the encode, in integer arithmetic; S = 2^24 - 1 as above.
 * Random words: Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85, ten
 *   rounds).  For the pixel at column x, row y of the FULL source frame (before any crop, flip or rotation) of output frame `run` of
 *   clip `clip`: counter (x, y, run, clip), key (key0, key1) = (seed & 0xffffffff, (seed >> 32) & 0xffffffff); output words 0, 1, 2
 *   serve the R, G and B bytes, word 3 is unused.  Nothing depends on launch geometry, chunking, crop position or augmentation.
 * Gaussian: `gauss` on the device and `gauss_host` the same words in HOST memory are 1025 int32, made once on the host in float64:
 *   t[i] = round(4096 * inv_cdf(min(max(i / 1024, 2^-13), 1 - 2^-13)))     (the standard normal quantile in Q12)
 *   Valid iff strictly increasing and |t[i]| < 2^15.  For a 32-bit word w: i = w >> 22, f = (w >> 10) & 4095,
 *   z = (t[i] (4096 - f) + t[i + 1] f + 2048) >> 12   (arithmetic shift).
 * Noise: per byte position of a run of n frames with linear mean L (as defined above) and the record's A < 2^20, B < 2^42:
 *   V     = floor((A L + B) (n - 1) / n)       (64-bit; V < 2^45)
 *   sigma = isqrt(V)                           (the mathematical integer square root)
 *   d     = (sigma z + 2048) >> 12             (arithmetic shift)
 *   L'    = clamp(L + d, 0, S),  blur = encode(L')
 *   The factor (n - 1) / n tops the average's noise up to the level of one source frame: a run of length 1 — every ground-truth
 *   record — has d = 0 and returns its bytes (it takes the copy path and reads neither table).  A = B = 0 gives the light entry's bytes.
 * Levels: a clip with shot coefficient a and read deviation r (full scale 1, variance a x + r^2) has A = rint(a S), B = rint(r^2 S^2).
 * The gauss table and every record (A < 2^20, B < 2^42, reserved == 0) are checked on the host copies before anything is launched,
 * beside every check of the light entries.  sizeof(spei_noise_record) == 24. */
typedef struct {
    uint32_t run, clip; /* the output frame's index in its clip's plan; the clip's index */
    uint32_t A;         /* shot term, < 2^20 */
    uint32_t reserved;  /* 0 */
    uint64_t B;         /* read term, < 2^42 */
} spei_noise_record;

/* spei_window_mean_light_u8 with noise: noise / noise_host hold M records, one per run. */
int spei_window_mean_noise_u8(const unsigned char* src, int64_t frame_stride, int T, const int* runs, const int* runs_host, int M,
                              const uint32_t* tables, const uint32_t* tables_host, const int32_t* gauss, const int32_t* gauss_host,
                              const spei_noise_record* noise, const spei_noise_record* noise_host, uint32_t key0, uint32_t key1,
                              unsigned char* blur, unsigned char* gt, float* gray, int H, int W, spei_stream_t stream);

/* spei_train_batch_runs_light_u8 with noise: noise / noise_host hold n_in + n_gt records, one per record of the table; the pixel
 * coordinates are those of the record's frame, (x0 + column, y0 + row) of the rectangle before flips and rotation. */
int spei_train_batch_runs_noise_u8(const spei_run_record* table, const spei_run_record* table_host, int n_in, int n_gt,
                                   const uint32_t* tables, const uint32_t* tables_host, const int32_t* gauss, const int32_t* gauss_host,
                                   const spei_noise_record* noise, const spei_noise_record* noise_host, uint32_t key0, uint32_t key1,
                                   float* input, float* gt, int P, float rgb_range, spei_stream_t stream);

/* ---- camera-shake blur in blur synthesis (speinet_amd/shake.py; an extension beyond the reference) ---- */

/* The blur a hand-held camera adds inside one exposure: the run's linear mean is correlated with a point-spread function (PSF) before
 * the noise and the encode, in integer arithmetic.  Lm(y, x, c) is the linear mean defined above, floor(sum of lin[byte] / n), at pixel
 * (y, x) of the FULL source frame [H][W].  A PSF is w[dy][dx], -r <= dy, dx <= r, radius r in 0..16: unsigned Q16 weights that sum to
 * exactly 65536.
 *   Lb(y, x, c) = (sum over dy, dx of w[dy][dx] Lm(clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1), c) + 2^15) >> 16
 *   The sum is exact (below 2^40 + 2^15: a 64-bit accumulator).  A correlation, not a flipped convolution: the weight at (dy, dx)
 *   multiplies the pixel dy rows below and dx columns to the right.  Coordinates clamp to the FRAME, never to a crop: the halo of a
 *   training crop reads the real neighbours outside the crop.  r = 0 (the delta PSF) gives Lb = Lm: the light / noise entry's bytes.
 * Without noise blur = encode(Lb).  With noise the formulas above run on Lb with the variance generalised — the PSF averages noise
 * away too: X = A Lb + B, q16 = floor(sum of w^2 / 2^16) (at most 65536),
 *   V = X - ceil(X q16 / (n 2^16))       (64-bit; X q16 < 2^61)
 *   which for the delta PSF (q16 = 65536) is floor(X (n - 1) / n), the V above.  sigma, z, d, L', the counter (x, y, run, clip) of the
 *   OUTPUT pixel in its full frame and encode are unchanged.  The gray plane is that of the final encoded bytes; a zero record stays zero.
 * `psfs` on the device and `psfs_host` the same words in HOST memory are n_psf tables of uint32 [33][33], centre at [16][16]: entry
 * [16 + dy][16 + dx] holds w[dy][dx].  One spei_shake_record per run / per table record: a record with radius == 0 ignores `psf` and
 * must carry q16 == 65536 (ground-truth records are such records).  Checked on the host copies before anything is launched, beside
 * every check of the light and noise entries: radius <= 16, psf < n_psf, every weight outside the radius 0, the sum 65536, q16 as
 * defined, reserved == 0; a bad record is an error that names the record.  psfs / psfs_host may be NULL when n_psf == 0.
 * sizeof(spei_shake_record) == 16. */
typedef struct {
    uint32_t psf;      /* index of the record's table in psfs */
    uint32_t radius;   /* 0..16; 0: the delta, no table is read */
    uint32_t q16;      /* floor(sum of w^2 / 2^16); 65536 for radius 0 */
    uint32_t reserved; /* 0 */
} spei_shake_record;

/* spei_window_mean_noise_u8 with shake: shake / shake_host hold M records, one per run.  gauss == NULL: no noise — gauss_host, noise,
 * noise_host and the keys are ignored and blur = encode(Lb).  With every record at radius 0 this is spei_window_mean_noise_u8's (or,
 * gauss == NULL, spei_window_mean_light_u8's) launch. */
int spei_window_mean_shake_u8(const unsigned char* src, int64_t frame_stride, int T, const int* runs, const int* runs_host, int M,
                              const uint32_t* tables, const uint32_t* tables_host, const int32_t* gauss, const int32_t* gauss_host,
                              const spei_noise_record* noise, const spei_noise_record* noise_host, uint32_t key0, uint32_t key1,
                              const uint32_t* psfs, const uint32_t* psfs_host, int n_psf, const spei_shake_record* shake,
                              const spei_shake_record* shake_host, unsigned char* blur, unsigned char* gt, float* gray, int H, int W,
                              spei_stream_t stream);

/* spei_train_batch_runs_noise_u8 with shake: shake / shake_host hold n_in + n_gt records, one per record of the table; the halo of a
 * rectangle is read from the record's frame [H][W], clamped at the frame's edges.  gauss == NULL and all-radius-0 tables as above. */
int spei_train_batch_runs_shake_u8(const spei_run_record* table, const spei_run_record* table_host, int n_in, int n_gt,
                                   const uint32_t* tables, const uint32_t* tables_host, const int32_t* gauss, const int32_t* gauss_host,
                                   const spei_noise_record* noise, const spei_noise_record* noise_host, uint32_t key0, uint32_t key1,
                                   const uint32_t* psfs, const uint32_t* psfs_host, int n_psf, const spei_shake_record* shake,
                                   const spei_shake_record* shake_host, float* input, float* gt, int P, float rgb_range,
                                   spei_stream_t stream);

/* ---- codec artefacts in blur synthesis (speinet_amd/codec.py; an extension beyond the reference) ---- */

/* A JPEG-style round trip of the synthesis's INPUT frames, on the final encoded bytes: YCbCr 4:2:0, 8x8 DCT, quantisation by quality-
 * scaled tables, dequantisation, inverse DCT, back to RGB.  Everything is int32, `>>` is an arithmetic shift (it floors), and the
 * result is defined bit for bit.  speinet_amd/codec.py's docstring is the definition; in short:
 * Grid: MCUs are 16 x 16 pixels; one corner of the grid sits at (-oy, -ox) of the frame or rectangle, 0 <= oy, ox < 16.  A sample outside
 *   the frame or rectangle is the nearest one inside (coordinates clamp).  An MCU reads and writes only its own pixels.
 * Colour: BT.601 full range, the Q14 constants of the `601 full` row above and the CENTER rule: Y = (yr R + yg G + yb B + 2^13) >> 14
 *   per pixel; Cb, Cr on the 2 x 2 channel sums with + 2^15, >> 16, + 128 and a clip to 0..255.  Back: chroma is REPLICATED,
 *   U16 = 16 Cb[y >> 1][x >> 1] (no bilinear taps), then R = clip((yy + rv v + 2^17) >> 18) and likewise G, B as in spei_yuv_to_rgb_u8.
 * Transform: D[u][x] = rint(8192 a(u) cos((2x + 1) u pi / 16)), a(0) = sqrt(1/8), a(u > 0) = 1/2.  Per 8 x 8 block of s = value - 128:
 *   T[y][u] = (sum_x D[u][x] s[y][x] + 2^9) >> 10             |sum| <= 2 965 504
 *   F[v][u] = (sum_y D[v][y] T[y][u] + 2^12) >> 13            |sum| <= 67 094 528; the coefficient in Q3
 *   q = sign(F) ((|F| + 4 Q) / (8 Q)), truncating division; G = q Q
 *   U[y][u] = (sum_v D[v][y] G[v][u] + 2^9) >> 10             |sum| <= 24 908 791
 *   r[y][x] = (sum_u D[u][x] U[y][u] + 2^15) >> 16            |sum| <= 526 417 325;  sample = clip(r + 128, 0, 255)
 * Tables: `qtabs` on the device and `qtabs_host` the same words in HOST memory are n_qtab tables of uint16 [2][64], luminance then
 *   chrominance, row-major [v][u], every entry in 1..255 (speinet_amd.codec.quant_tables: ITU-T T.81 Annex K scaled by libjpeg's rule).
 * Checked on the host copies before anything is launched: qtab < n_qtab, oy, ox < 16, only known flag bits, every table entry in
 * 1..255; a bad record is an error that names the record.  sizeof(spei_codec_record) == 16. */
#define SPEI_CODEC_SKIP 16 /* the record's frame is left alone */
typedef struct {
    uint32_t qtab;   /* index of the record's tables in qtabs */
    uint32_t oy, ox; /* 0..15: the grid's corner at (-oy, -ox) */
    uint32_t flags;  /* SPEI_CROP_HFLIP | VFLIP | ROT90 | ZERO, SPEI_CODEC_SKIP */
} spei_codec_record;

/* The round trip in place on N packed uint8 [H][W][3] frames, frame_stride bytes apart; records / records_host hold N records whose
 * flags are 0 or SPEI_CODEC_SKIP.  A SKIP record leaves its frame and its gray plane alone.  gray (or NULL): [N][H][W] fp32, rewritten
 * for every coded frame, bit-identical to spei_frames_u8_in's gray plane of the new bytes. */
int spei_codec_u8(unsigned char* frames, int64_t frame_stride, int N, int H, int W, const spei_codec_record* records,
                  const spei_codec_record* records_host, const uint16_t* qtabs, const uint16_t* qtabs_host, int n_qtab, float* gray,
                  spei_stream_t stream);

/* The round trip in place on the fp32 [n_in][3][P][P] input tensor a spei_train_batch_runs_* entry wrote; records / records_host hold
 * n_in records.  With s = (float)(rgb_range / 255) and inv = (float)(255 / rgb_range) the byte of a value v is (int)(v * inv + 0.5f);
 * that this returns u from (float)u * s for all 256 codes is verified on the host before the launch, and an rgb_range for which it
 * does not is an error.  The round trip runs on the P x P rectangle in SOURCE orientation: the record's SPEI_CROP_* flags say how the
 * stored plane is flipped and rotated (spei_train_batch_u8's geometry), and its bytes u' are written back as (float)u' * s.  A ZERO
 * record stays zero, a SKIP record is left alone.  With oy = y0 % 16, ox = x0 % 16 the grid is the FULL frame's: every MCU wholly inside
 * the rectangle equals spei_codec_u8 on the whole frame bit for bit; the partial MCUs on the rectangle's border ring replicate the
 * RECTANGLE's edge, not the frame's real neighbours. */
int spei_train_batch_codec_f32(float* input, int n_in, int P, float rgb_range, const spei_codec_record* records,
                               const spei_codec_record* records_host, const uint16_t* qtabs, const uint16_t* qtabs_host, int n_qtab,
                               spei_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
