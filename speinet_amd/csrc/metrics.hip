// Harness metrics of one deblurred frame on the device (reference inference_SPEINet.py:484-500 calc_PSNR, :502-543 calc_SSIM): PSNR and
// SSIM of the uint8 [H][W][3] frame that is written to disk (spei_frame_u8_out, frame_io.hip) against the ground-truth frame on the
// border-cropped region — three small launches instead of the ~45 torch kernels of round 3 (float64 band-matrix GEMMs for the Gaussian
// window: 0.95 ms of rocBLAS per window, 2.2 ms in all; profiles/r04_harness_*).  Arithmetic: integers where the reference has
// integers (the squared differences, summed exactly in float64), float64 for the SSIM window sums and the means, as numpy does it.
// SSIM: 11x11 Gaussian (sigma 1.5) = outer(k, k) applied as a row pass and a column pass, valid region only; per channel; the mean over
// all channels and positions (the reference averages the same 3-channel value three times).  HBM-bound: each frame is read once per
// kernel (2.8 MB).
#include "common.h"

namespace {

constexpr int TW = 32, TH = 8, R = 5, KS = 2 * R + 1;     // output tile, window radius

__global__ __launch_bounds__(256) void sq_diff_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, int H,
                                                       int W, int border, double* __restrict__ part) {
    // one thread = one byte: sum of (a - b)^2 over the cropped region
    const int n = H * W * 3;
    long long sq = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int p = i / 3, y = p / W, x = p - y * W;
        if (y >= border && y < H - border && x >= border && x < W - border) {
            const int d = (int)a[i] - (int)b[i];
            sq += d * d;
        }
    }
    // block reduction (fixed order): lanes, then waves; every partial is an integer below 2^53, so the sums are exact
    __shared__ double s_sq[4];
    double dsq = (double)sq;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dsq += __shfl_xor(dsq, o, 64);
    if ((threadIdx.x & 63) == 0) s_sq[threadIdx.x >> 6] = dsq;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (s_sq[0] + s_sq[1]) + (s_sq[2] + s_sq[3]);
}

struct Gauss { double k[KS]; };

__global__ __launch_bounds__(256) void ssim_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, int H, int W,
                                                    int border, Gauss g, double* __restrict__ part) {
    // cropped image: rows / columns [border, H - border) x [border, W - border); valid outputs: another R inside
    const int ch = H - 2 * border, cw = W - 2 * border, oh = ch - 2 * R, ow = cw - 2 * R;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int ox0 = blockIdx.x * TW, oy0 = blockIdx.y * TH;
    __shared__ float pa[TH + 2 * R][TW + 2 * R], pb[TH + 2 * R][TW + 2 * R];
    __shared__ double hb[5][TH + 2 * R][TW];
    double acc = 0.0;
    for (int c = 0; c < 3; ++c) {
        for (int i = threadIdx.x; i < (TH + 2 * R) * (TW + 2 * R); i += 256) {
            const int py = i / (TW + 2 * R), px = i - py * (TW + 2 * R);
            const int y = min(oy0 + py, ch - 1) + border, x = min(ox0 + px, cw - 1) + border;
            const size_t o = ((size_t)y * W + x) * 3 + c;
            pa[py][px] = (float)a[o];
            pb[py][px] = (float)b[o];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < (TH + 2 * R) * TW; i += 256) {
            const int py = i >> 5, px = i & 31;
            double s1 = 0, s2 = 0, s11 = 0, s22 = 0, s12 = 0;
#pragma unroll
            for (int t = 0; t < KS; ++t) {
                const double va = pa[py][px + t], vb = pb[py][px + t], w = g.k[t];
                s1 += w * va; s2 += w * vb; s11 += w * (va * va); s22 += w * (vb * vb); s12 += w * (va * vb);
            }
            hb[0][py][px] = s1; hb[1][py][px] = s2; hb[2][py][px] = s11; hb[3][py][px] = s22; hb[4][py][px] = s12;
        }
        __syncthreads();
        if (oy0 + ty < oh && ox0 + tx < ow) {
            double m1 = 0, m2 = 0, e11 = 0, e22 = 0, e12 = 0;
#pragma unroll
            for (int t = 0; t < KS; ++t) {
                const double w = g.k[t];
                m1 += w * hb[0][ty + t][tx]; m2 += w * hb[1][ty + t][tx];
                e11 += w * hb[2][ty + t][tx]; e22 += w * hb[3][ty + t][tx]; e12 += w * hb[4][ty + t][tx];
            }
            const double c1 = (0.01 * 255) * (0.01 * 255), c2 = (0.03 * 255) * (0.03 * 255);
            const double v1 = e11 - m1 * m1, v2 = e22 - m2 * m2, v12 = e12 - m1 * m2;
            acc += ((2 * m1 * m2 + c1) * (2 * v12 + c2)) / ((m1 * m1 + m2 * m2 + c1) * (v1 + v2 + c2));
        }
        __syncthreads();
    }
    __shared__ double s_acc[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) s_acc[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = (s_acc[0] + s_acc[1]) + (s_acc[2] + s_acc[3]);
}

__global__ __launch_bounds__(256) void metrics_final_kernel(const double* __restrict__ part_sq, int n_sq, const double* __restrict__ part_ssim,
                                                             int n_ssim, double n_px, double n_ssim_px, double* __restrict__ result) {
    __shared__ double s[2][4];
    double sq = 0, ss = 0;
    for (int i = threadIdx.x; i < n_sq; i += 256) sq += part_sq[i];
    for (int i = threadIdx.x; i < n_ssim; i += 256) ss += part_ssim[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sq += __shfl_xor(sq, o, 64); ss += __shfl_xor(ss, o, 64);
    }
    if ((threadIdx.x & 63) == 0) { s[0][threadIdx.x >> 6] = sq; s[1][threadIdx.x >> 6] = ss; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double tsq = (s[0][0] + s[0][1]) + (s[0][2] + s[0][3]), tss = (s[1][0] + s[1][1]) + (s[1][2] + s[1][3]);
        const double mse = tsq / n_px;
        result[0] = mse == 0.0 ? INFINITY : 20.0 * log10(255.0 / sqrt(mse));     // calc_PSNR (inf on identical frames)
        result[1] = tss / n_ssim_px;
    }
}

constexpr int SQ_BLOCKS = 512;

// calc_psnr of the training loop (util/utils.py:81-92): the float frames themselves, shaved; d in fp32 as numpy computes it, d * d exact
// in float64, summed in a fixed order (lanes, waves, then the blocks' partials in the second launch)
__global__ __launch_bounds__(256) void psnr_f32_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W, int shave,
                                                        float rgb_range, double* __restrict__ part) {
    const int ch = H - 2 * shave, cw = W - 2 * shave;
    const int64_t n = (int64_t)3 * ch * cw;
    double sq = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / cw;                         // c * ch + y
        const int x = (int)(i - row * cw), c = (int)(row / ch), y = (int)(row - (int64_t)c * ch);
        const int64_t o = ((int64_t)c * H + y + shave) * W + x + shave;
        const float d = __fsub_rn(__fdiv_rn(a[o], rgb_range), __fdiv_rn(b[o], rgb_range));
        sq += (double)d * (double)d;
    }
    __shared__ double s_sq[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
    if ((threadIdx.x & 63) == 0) s_sq[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (s_sq[0] + s_sq[1]) + (s_sq[2] + s_sq[3]);
}

__global__ __launch_bounds__(256) void psnr_f32_final_kernel(const double* __restrict__ part, double count, double* __restrict__ result) {
    __shared__ double s[4];
    double sq = part[threadIdx.x];                         // SPEI_PSNR_WS_DOUBLES == 256 partials
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
        result[0] = (s[0] + s[1]) + (s[2] + s[3]);
        result[1] = count;
    }
}

static_assert(SPEI_PSNR_WS_DOUBLES == 256, "psnr_f32_final_kernel reads one partial per thread");

}  // namespace

extern "C" int spei_psnr_f32(const float* a, const float* b, int H, int W, int shave, float rgb_range, double* ws, double* result,
                             spei_stream_t stream) {
    SPEI_REQUIRE(a && b && ws && result, "spei_psnr_f32: null pointer");
    SPEI_REQUIRE(shave >= 0 && H - 2 * shave > 0 && W - 2 * shave > 0 && (int64_t)H * W < (1ll << 29),
                 "spei_psnr_f32: %dx%d shaved by %d leaves nothing to score", H, W, shave);
    SPEI_REQUIRE(rgb_range > 0.0f, "spei_psnr_f32: rgb_range %g must be positive", (double)rgb_range);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(psnr_f32_kernel, dim3(SPEI_PSNR_WS_DOUBLES), dim3(256), 0, st, a, b, H, W, shave, rgb_range, ws);
    hipLaunchKernelGGL(psnr_f32_final_kernel, dim3(1), dim3(256), 0, st, ws, 3.0 * (H - 2 * shave) * (double)(W - 2 * shave), result);
    SPEI_CHECK_LAUNCH("spei_psnr_f32");
    return 0;
}

extern "C" int64_t spei_frame_metrics_ws_doubles(int H, int W, int border) {
    const int oh = H - 2 * border - 2 * R, ow = W - 2 * border - 2 * R;
    if (oh <= 0 || ow <= 0) return -1;
    return (int64_t)SQ_BLOCKS + (int64_t)cdiv(ow, TW) * cdiv(oh, TH);
}

extern "C" int spei_frame_metrics(const unsigned char* out_hwc, const unsigned char* gt_hwc, int H, int W, int border, double* ws,
                                  double* result, spei_stream_t stream) {
    SPEI_REQUIRE(out_hwc && gt_hwc && ws && result, "spei_frame_metrics: null pointer");
    SPEI_REQUIRE(border >= 0 && H - 2 * border - 2 * R > 0 && W - 2 * border - 2 * R > 0 && (int64_t)H * W < (1ll << 29),
                 "spei_frame_metrics: %dx%d with border %d leaves no valid SSIM window", H, W, border);
    hipStream_t st = (hipStream_t)stream;
    Gauss g;
    double sum = 0;
    for (int i = 0; i < KS; ++i) { g.k[i] = exp(-((i - R) * (i - R)) / (2.0 * 1.5 * 1.5)); sum += g.k[i]; }
    for (int i = 0; i < KS; ++i) g.k[i] /= sum;
    const int oh = H - 2 * border - 2 * R, ow = W - 2 * border - 2 * R;
    const dim3 tiles(cdiv(ow, TW), cdiv(oh, TH));
    double* part_ssim = ws + SQ_BLOCKS;
    hipLaunchKernelGGL(sq_diff_kernel, dim3(SQ_BLOCKS), dim3(256), 0, st, out_hwc, gt_hwc, H, W, border, ws);
    hipLaunchKernelGGL(ssim_kernel, tiles, dim3(256), 0, st, out_hwc, gt_hwc, H, W, border, g, part_ssim);
    hipLaunchKernelGGL(metrics_final_kernel, dim3(1), dim3(256), 0, st, ws, SQ_BLOCKS, part_ssim, (int)(tiles.x * tiles.y),
                       (double)(H - 2 * border) * (W - 2 * border) * 3.0, (double)oh * ow * 3.0, result);
    SPEI_CHECK_LAUNCH("spei_frame_metrics");
    return 0;
}
