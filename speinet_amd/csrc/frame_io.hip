// Frame I/O of the clip API (speinet_amd/video.py): uint8 frames of any size in, uint8 frames of the same size out.
//
//   spei_frames_u8_in  — N uint8 [H][W][3] frames -> fp32 [N][3][Hp][Wp], Hp / Wp the next multiples of 20, values u * (float)(1/255)
//                        (reference inference_SPEINet.py:466-475 numpy2tensor: float64 -> float32, then mul_(1/255) in float32);
//                        the bottom / right pad reflects (torch F.pad mode "reflect", as SwinIR's check_image_size pads to window
//                        multiples): padded row H + j reads row H - 2 - j, column W + j reads column W - 2 - j.  Optionally the
//                        LD detector's gray plane [N][H][W] of the unpadded frame, bit-identical to spei_det_gray on the same frame
//                        as fp32 0..255 (one shared expression, spei_gray_px).
//   spei_frame_u8_out  — fp32 [3][Hp][Wp] -> the top-left H x W crop as uint8 [H][W][3], round_half_even(clamp(x * 255, 0, 255))
//                        (reference :477-482 tensor2numpy), 0 for a non-finite value: the frame that is written to disk and that
//                        the harness scores (spei_frame_metrics, metrics.hip).  Optionally a flag, nonzero iff the crop held a
//                        non-finite value, on which the clip API recomputes the window in bf16x3.
//
//   spei_frame_pair_stats — N uint8 [H][W][3] frames (and optionally the frame before them) -> the 64-bin histogram of every frame's
//                        integer luma Y = (77 R + 150 G + 29 B + 128) >> 8 and the sum of |Y_a - Y_b| over every consecutive pair:
//                        the statistics of the clip API's scene-cut rule (video.find_cuts; an extension, the reference has no such
//                        pass).  Integers throughout: the result does not depend on the launch shape or on the order of the sums.
//
// Streaming kernels, one thread per group of 4 pixels of a row: 12 bytes of uint8 read (three dwords when the rows are 4-byte
// aligned), one 16-byte store per plane.  The mirrored indices are computed in the pad band only.  HBM-bound: a 720p frame is
// 2.8 MB in and 11 MB out.
#include "common.h"

namespace {

constexpr int MULT = 20;                                   // two stride-2 stages, then 5x5 windows
constexpr float INV255 = (float)(1.0 / 255.0);             // numpy2tensor's rgb_range / 255 (a Python float) as the float32 scalar
constexpr int BLOCKS_MAX = 8192;

__device__ __forceinline__ int byte_of(const uint32_t (&w)[3], int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xff; }

__global__ __launch_bounds__(256) void frames_u8_in_kernel(const unsigned char* __restrict__ src, int64_t fstride, float* __restrict__ dst,
                                                           float* __restrict__ gray, int H, int W, int Hp, int Wp, int64_t total,
                                                           int aligned) {
    const int gw = Wp >> 2;                                // groups per padded row (Wp % 20 == 0)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / gw;                        // n * Hp + y
        const int x0 = (int)(i - row * gw) * 4;
        const int n = (int)(row / Hp), y = (int)(row - (int64_t)n * Hp);
        if (!dst && y >= H) continue;                      // gray only: the pad rows have nothing to write
        const int sy = y < H ? y : 2 * H - 2 - y;
        const unsigned char* s = src + n * fstride + (int64_t)sy * W * 3;
        float v[3][4];
        if (x0 + 4 <= W) {                                 // interior: 12 consecutive bytes
            uint32_t w[3];
            if (aligned) {
                const uint32_t* p = reinterpret_cast<const uint32_t*>(s + x0 * 3);
                w[0] = p[0]; w[1] = p[1]; w[2] = p[2];
            } else {
                const unsigned char* p = s + x0 * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    w[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][k] = (float)byte_of(w, 3 * k + c);
        } else {                                           // right edge and pad band: column W + j reads column W - 2 - j
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = x0 + k, sx = x < W ? x : 2 * W - 2 - x;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][k] = (float)s[sx * 3 + c];
            }
        }
        if (gray && y < H) {
            float* g = gray + ((int64_t)n * H + y) * W;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < W) g[x0 + k] = spei_gray_px(v[0][k], v[1][k], v[2][k]);
        }
        if (dst) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float4* d = reinterpret_cast<float4*>(dst + (((int64_t)n * 3 + c) * Hp + y) * Wp + x0);
                *d = make_float4(v[c][0] * INV255, v[c][1] * INV255, v[c][2] * INV255, v[c][3] * INV255);
            }
        }
    }
}

__device__ __forceinline__ uint32_t to_u8(float v) {
    const float q = rintf(fminf(fmaxf(v * 255.0f, 0.0f), 255.0f));     // mul(255).clamp(0, 255).round(): half to even, as torch
    return isfinite(v) ? (uint32_t)q : 0u;
}

__global__ __launch_bounds__(256) void frame_u8_out_kernel(const float* __restrict__ src, unsigned char* __restrict__ dst,
                                                           int* __restrict__ nonfinite, int H, int W, int Wp, int64_t plane, int gw,
                                                           int64_t total, int vec_in, int vec_out) {
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / gw), x0 = (int)(i - (int64_t)y * gw) * 4;
        const float* s = src + (int64_t)y * Wp + x0;
        uint32_t q[3][4];
        if (vec_in) {                                      // Wp % 4 == 0: x0 + 4 <= Wp
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 f = *reinterpret_cast<const float4*>(s + c * plane);
                const float e[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    q[c][k] = to_u8(e[k]);
                    bad |= (x0 + k < W && !isfinite(e[k])) ? 1 : 0;     // columns W.. of the group are pad, not part of the crop
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float v = x0 + k < W ? s[c * plane + k] : 0.0f;
                    q[c][k] = to_u8(v);
                    bad |= isfinite(v) ? 0 : 1;
                }
        }
        unsigned char* d = dst + ((int64_t)y * W + x0) * 3;
        if (vec_out && x0 + 4 <= W) {                      // 12 bytes as three dwords
            uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 12; ++j) w[j >> 2] |= q[j % 3][j / 3] << (8 * (j & 3));
            uint32_t* p = reinterpret_cast<uint32_t*>(d);
            p[0] = w[0]; p[1] = w[1]; p[2] = w[2];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < W)
#pragma unroll
                    for (int c = 0; c < 3; ++c) d[k * 3 + c] = (unsigned char)q[c][k];
        }
    }
    if (nonfinite && bad) atomicOr(nonfinite, 1);           // rare: one atomic per thread that met a non-finite value
}

// ---- pair statistics -----------------------------------------------------------------------------------------------------------
// grid (x, n): the blocks of column n stream frame n (member b of its pair: its histogram) beside the frame before it (member a:
// frame n - 1, or `prev` for n = 0, or none), so a frame is read twice at most.  Rows are packed, so a frame is one run of H * W
// pixels: 12-byte groups of 4 pixels as three dwords when both frames start on a 4-byte boundary, bytes otherwise and in the last,
// partial group.  Histogram counts go to one LDS copy per wave; SAD partials are summed per wave, then per block; each block then
// issues one integer atomic per non-empty bin and one 64-bit atomic for its SAD (Guideline 12: integer adds commute exactly).
constexpr int PAIR_BLOCKS = 256;                           // blocks per frame
constexpr int PAIR_BINS = 64;
// A thread adds at most 4 * 255 per group, and a frame holds fewer than 2^31 / 12 groups (the bound of spei_frames_u8_in), so with
// PAIR_BLOCKS blocks of 256 threads even a whole block's SAD fits 32 bits: the partials are widened once, at the global atomic.
static_assert((((1ll << 31) / 12) / (256ll * PAIR_BLOCKS) + 1) * 256 * 4 * 255 < (1ll << 32), "pair SAD: a block's sum must fit 32 bits");

__device__ __forceinline__ void load_group(const unsigned char* __restrict__ p, int valid, bool aligned, uint32_t (&w)[3]) {
    if (valid == 4 && aligned) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        w[0] = q[0]; w[1] = q[1]; w[2] = q[2];
    } else {
        w[0] = w[1] = w[2] = 0u;
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (j < 3 * valid) w[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
    }
}

__device__ __forceinline__ int luma_of(const uint32_t (&w)[3], int k) {
    return (77 * byte_of(w, 3 * k) + 150 * byte_of(w, 3 * k + 1) + 29 * byte_of(w, 3 * k + 2) + 128) >> 8;
}

__global__ __launch_bounds__(256) void frame_pair_stats_kernel(const unsigned char* __restrict__ src, int64_t fstride,
                                                               const unsigned char* __restrict__ prev, int* __restrict__ hist,
                                                               unsigned long long* __restrict__ sad, int64_t pixels) {
    __shared__ unsigned int bins[4][PAIR_BINS];
    __shared__ unsigned int block_sad;
    const int n = blockIdx.y, wave = threadIdx.x >> 6;
    const unsigned char* b = src + n * fstride;
    const unsigned char* a = n > 0 ? b - fstride : prev;   // null: frame 0 of a call without `prev` has no pair
    const bool aligned = (((uintptr_t)b | (uintptr_t)a) & 3) == 0;
    (&bins[0][0])[threadIdx.x] = 0u;
    if (threadIdx.x == 0) block_sad = 0u;
    __syncthreads();
    const int64_t groups = (pixels + 3) >> 2, full = pixels >> 2;
    unsigned int part = 0u;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        const int valid = g < full ? 4 : (int)(pixels - 4 * g);
        uint32_t wb[3], wa[3];
        load_group(b + 12 * g, valid, aligned, wb);
        if (a) load_group(a + 12 * g, valid, aligned, wa);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < valid) {
                const int yb = luma_of(wb, k);
                atomicAdd(&bins[wave][yb >> 2], 1u);
                if (a) part += (unsigned int)abs(luma_of(wa, k) - yb);
            }
        }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) part += __shfl_xor(part, m);
    if (a && (threadIdx.x & 63) == 0) atomicAdd(&block_sad, part);
    __syncthreads();
    if (threadIdx.x < PAIR_BINS) {
        const unsigned int c = bins[0][threadIdx.x] + bins[1][threadIdx.x] + bins[2][threadIdx.x] + bins[3][threadIdx.x];
        if (c) atomicAdd(&hist[n * PAIR_BINS + threadIdx.x], (int)c);
    }
    if (a && threadIdx.x == 0) atomicAdd(&sad[prev ? n : n - 1], (unsigned long long)block_sad);
}

// ---- deep frames (10 and 12 bits in 16-bit words; depth d, D = 2^d - 1; a word above D reads as D) ----------------------------------
// The same three kernels on uint16 samples: a group of 4 pixels is 24 bytes, three 8-byte accesses where base, stride and W allow.
__device__ __forceinline__ int half_of(const uint2 (&w)[3], int j) {
    const uint2 q = w[j >> 2];
    return (((j & 2) ? q.y : q.x) >> (16 * (j & 1))) & 0xffff;
}

__global__ __launch_bounds__(256) void frames_u16_in_kernel(const uint16_t* __restrict__ src, int64_t fstride, float* __restrict__ dst,
                                                            float* __restrict__ gray, int H, int W, int Hp, int Wp, int64_t total,
                                                            int aligned, int D, float inv, float to255) {
    const int gw = Wp >> 2;                                // groups per padded row (Wp % 20 == 0)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / gw;                        // n * Hp + y
        const int x0 = (int)(i - row * gw) * 4;
        const int n = (int)(row / Hp), y = (int)(row - (int64_t)n * Hp);
        if (!dst && y >= H) continue;                      // gray only: the pad rows have nothing to write
        const int sy = y < H ? y : 2 * H - 2 - y;
        const uint16_t* s = src + n * fstride + (int64_t)sy * W * 3;     // fstride in samples
        float v[3][4];
        if (aligned && x0 + 4 <= W) {                      // interior: 24 consecutive bytes
            const uint2* p = reinterpret_cast<const uint2*>(s + x0 * 3);
            const uint2 w[3] = {p[0], p[1], p[2]};
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][k] = (float)min(half_of(w, 3 * k + c), D);
        } else {                                           // unaligned rows, right edge and pad band: column W + j reads W - 2 - j
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = x0 + k, sx = x < W ? x : 2 * W - 2 - x;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][k] = (float)min((int)s[sx * 3 + c], D);
            }
        }
        if (gray && y < H) {                               // the detector's 0..255 scale, the extra bits kept
            float* g = gray + ((int64_t)n * H + y) * W;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < W) g[x0 + k] = spei_gray_px(v[0][k] * to255, v[1][k] * to255, v[2][k] * to255);
        }
        if (dst) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float4* d = reinterpret_cast<float4*>(dst + (((int64_t)n * 3 + c) * Hp + y) * Wp + x0);
                *d = make_float4(v[c][0] * inv, v[c][1] * inv, v[c][2] * inv, v[c][3] * inv);
            }
        }
    }
}

__device__ __forceinline__ uint32_t to_deep(float v, float Df) {
    const float q = rintf(fminf(fmaxf(v * Df, 0.0f), Df));             // mul(D).clamp(0, D).round(): half to even, as torch
    return isfinite(v) ? (uint32_t)q : 0u;
}

__global__ __launch_bounds__(256) void frame_u16_out_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst,
                                                            int* __restrict__ nonfinite, int H, int W, int Wp, int64_t plane, int gw,
                                                            int64_t total, int vec_in, int vec_out, float Df) {
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / gw), x0 = (int)(i - (int64_t)y * gw) * 4;
        const float* s = src + (int64_t)y * Wp + x0;
        uint32_t q[3][4];
        if (vec_in) {                                      // Wp % 4 == 0: x0 + 4 <= Wp
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 f = *reinterpret_cast<const float4*>(s + c * plane);
                const float e[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    q[c][k] = to_deep(e[k], Df);
                    bad |= (x0 + k < W && !isfinite(e[k])) ? 1 : 0;     // columns W.. of the group are pad, not part of the crop
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float v = x0 + k < W ? s[c * plane + k] : 0.0f;
                    q[c][k] = to_deep(v, Df);
                    bad |= isfinite(v) ? 0 : 1;
                }
        }
        uint16_t* d = dst + ((int64_t)y * W + x0) * 3;
        if (vec_out && x0 + 4 <= W) {                      // 24 bytes as three 8-byte stores
            uint32_t w[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 12; ++j) w[j >> 1] |= q[j % 3][j / 3] << (16 * (j & 1));
            uint2* p = reinterpret_cast<uint2*>(d);
            p[0] = make_uint2(w[0], w[1]); p[1] = make_uint2(w[2], w[3]); p[2] = make_uint2(w[4], w[5]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < W)
#pragma unroll
                    for (int c = 0; c < 3; ++c) d[k * 3 + c] = (uint16_t)q[c][k];
        }
    }
    if (nonfinite && bad) atomicOr(nonfinite, 1);           // rare: one atomic per thread that met a non-finite value
}

// A thread adds at most 4 * 4095 per group and holds at most 2732 groups (above), so a wave's SAD fits 32 bits; a block's need not:
// the four wave sums are added in 64 bits by one thread, which issues the block's one global atomic.
static_assert((((1ll << 31) / 12) / (256ll * PAIR_BLOCKS) + 1) * 64 * 4 * 4095 < (1ll << 32), "pair SAD: a wave's sum must fit 32 bits");

__device__ __forceinline__ void load_group(const uint16_t* __restrict__ p, int valid, bool aligned, int D, int (&c)[12]) {
    if (valid == 4 && aligned) {
        const uint2* q = reinterpret_cast<const uint2*>(p);
        const uint2 w[3] = {q[0], q[1], q[2]};
#pragma unroll
        for (int j = 0; j < 12; ++j) c[j] = min(half_of(w, j), D);
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) c[j] = j < 3 * valid ? min((int)p[j], D) : 0;
    }
}

__device__ __forceinline__ int luma_of(const int (&c)[12], int k) {
    return (77 * c[3 * k] + 150 * c[3 * k + 1] + 29 * c[3 * k + 2] + 128) >> 8;
}

__global__ __launch_bounds__(256) void frame_pair_stats_u16_kernel(const uint16_t* __restrict__ src, int64_t fstride,
                                                                   const uint16_t* __restrict__ prev, int* __restrict__ hist,
                                                                   unsigned long long* __restrict__ sad, int64_t pixels, int s) {
    __shared__ unsigned int bins[4][PAIR_BINS];
    __shared__ unsigned int wave_sad[4];
    const int n = blockIdx.y, wave = threadIdx.x >> 6, D = (256 << s) - 1;
    const uint16_t* b = src + n * fstride;                 // fstride in samples
    const uint16_t* a = n > 0 ? b - fstride : prev;        // null: frame 0 of a call without `prev` has no pair
    const bool aligned = (((uintptr_t)b | (uintptr_t)a) & 7) == 0;
    (&bins[0][0])[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t groups = (pixels + 3) >> 2, full = pixels >> 2;
    unsigned int part = 0u;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        const int valid = g < full ? 4 : (int)(pixels - 4 * g);
        int cb[12], ca[12];
        load_group(b + 12 * g, valid, aligned, D, cb);
        if (a) load_group(a + 12 * g, valid, aligned, D, ca);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < valid) {
                const int yb = luma_of(cb, k);
                atomicAdd(&bins[wave][yb >> (2 + s)], 1u);
                if (a) part += (unsigned int)abs(luma_of(ca, k) - yb);
            }
        }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) part += __shfl_xor(part, m);
    if ((threadIdx.x & 63) == 0) wave_sad[wave] = part;
    __syncthreads();
    if (threadIdx.x < PAIR_BINS) {
        const unsigned int c = bins[0][threadIdx.x] + bins[1][threadIdx.x] + bins[2][threadIdx.x] + bins[3][threadIdx.x];
        if (c) atomicAdd(&hist[n * PAIR_BINS + threadIdx.x], (int)c);
    }
    if (a && threadIdx.x == 0)
        atomicAdd(&sad[prev ? n : n - 1], (unsigned long long)wave_sad[0] + wave_sad[1] + wave_sad[2] + wave_sad[3]);
}

inline int grid_for(int64_t total) { return (int)((total + 255) / 256 < BLOCKS_MAX ? (total + 255) / 256 : BLOCKS_MAX); }

}  // namespace

extern "C" int spei_frames_u8_in(const unsigned char* src, int64_t frame_stride, float* dst, float* gray, int N, int H, int W,
                                 spei_stream_t stream) {
    SPEI_REQUIRE(src && (dst || gray), "spei_frames_u8_in: null pointer (src, and dst or gray, are required)");
    SPEI_REQUIRE(N > 0 && H > 0 && W > 0 && (int64_t)H * W * 3 < (1ll << 31), "spei_frames_u8_in: bad frame shape %d x %dx%d", N, H, W);
    SPEI_REQUIRE(N == 1 || frame_stride >= (int64_t)H * W * 3, "spei_frames_u8_in: frame stride %lld < one %dx%d frame",
                 (long long)frame_stride, H, W);
    const int Hp = (H + MULT - 1) / MULT * MULT, Wp = (W + MULT - 1) / MULT * MULT;
    SPEI_REQUIRE(Hp - H < H && Wp - W < W, "spei_frames_u8_in: a %dx%d frame cannot reflect-pad to %dx%d (the pad must be smaller "
                 "than the frame)", H, W, Hp, Wp);
    SPEI_REQUIRE(!dst || ((uintptr_t)dst & 15) == 0, "spei_frames_u8_in: dst must be 16-byte aligned");
    const int aligned = ((uintptr_t)src & 3) == 0 && (N == 1 || (frame_stride & 3) == 0) && (W & 3) == 0;
    const int64_t total = (int64_t)N * Hp * (Wp / 4);
    hipLaunchKernelGGL(frames_u8_in_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, src, frame_stride, dst, gray, H, W,
                       Hp, Wp, total, aligned);
    SPEI_CHECK_LAUNCH("spei_frames_u8_in");
    return 0;
}

extern "C" int spei_frame_u8_out(const float* src, unsigned char* dst, int* nonfinite, int H, int W, int Hp, int Wp,
                                 spei_stream_t stream) {
    SPEI_REQUIRE(src && dst, "spei_frame_u8_out: null pointer");
    SPEI_REQUIRE(H > 0 && W > 0 && Hp >= H && Wp >= W && (int64_t)Hp * Wp < (1ll << 30),
                 "spei_frame_u8_out: bad sizes (crop %dx%d of a %dx%d frame)", H, W, Hp, Wp);
    const int gw = (W + 3) / 4;
    const int vec_in = (Wp & 3) == 0 && ((uintptr_t)src & 15) == 0;
    const int vec_out = (W & 3) == 0 && ((uintptr_t)dst & 3) == 0;
    const int64_t total = (int64_t)H * gw;
    if (nonfinite && hipMemsetAsync(nonfinite, 0, sizeof(int), (hipStream_t)stream) != hipSuccess) {
        spei_set_error("spei_frame_u8_out: clearing the non-finite flag failed");
        return -2;
    }
    hipLaunchKernelGGL(frame_u8_out_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, src, dst, nonfinite, H, W, Wp,
                       (int64_t)Hp * Wp, gw, total, vec_in, vec_out);
    SPEI_CHECK_LAUNCH("spei_frame_u8_out");
    return 0;
}

extern "C" int spei_frame_pair_stats(const unsigned char* src, int64_t frame_stride, const unsigned char* prev, int N, int H, int W,
                                     int* hist, int64_t* sad, spei_stream_t stream) {
    SPEI_REQUIRE(src && hist && sad, "spei_frame_pair_stats: null pointer (src, hist and sad are required)");
    SPEI_REQUIRE(N >= 1 && N <= 65535, "spei_frame_pair_stats: %d frames (1..65535 per call)", N);
    SPEI_REQUIRE(N > 1 || prev, "spei_frame_pair_stats: one frame and no prev make no pair");
    SPEI_REQUIRE(H > 0 && W > 0 && (int64_t)H * W * 3 < (1ll << 31), "spei_frame_pair_stats: bad frame shape %dx%d", H, W);
    SPEI_REQUIRE(N == 1 || frame_stride >= (int64_t)H * W * 3, "spei_frame_pair_stats: frame stride %lld < one %dx%d frame",
                 (long long)frame_stride, H, W);
    const int64_t pixels = (int64_t)H * W, blocks = ((pixels + 3) / 4 + 255) / 256;
    const int pairs = prev ? N : N - 1;
    if (hipMemsetAsync(hist, 0, sizeof(int) * PAIR_BINS * N, (hipStream_t)stream) != hipSuccess ||
        hipMemsetAsync(sad, 0, sizeof(int64_t) * pairs, (hipStream_t)stream) != hipSuccess) {
        spei_set_error("spei_frame_pair_stats: clearing the results failed");
        return -2;
    }
    hipLaunchKernelGGL(frame_pair_stats_kernel, dim3((int)(blocks < PAIR_BLOCKS ? blocks : PAIR_BLOCKS), N), dim3(256), 0,
                       (hipStream_t)stream, src, frame_stride, prev, hist, reinterpret_cast<unsigned long long*>(sad), pixels);
    SPEI_CHECK_LAUNCH("spei_frame_pair_stats");
    return 0;
}

extern "C" int spei_frames_u16_in(const uint16_t* src, int64_t frame_stride, float* dst, float* gray, int N, int H, int W, int depth,
                                  spei_stream_t stream) {
    SPEI_REQUIRE(src && (dst || gray), "spei_frames_u16_in: null pointer (src, and dst or gray, are required)");
    SPEI_REQUIRE(N > 0 && H > 0 && W > 0 && (int64_t)H * W * 3 < (1ll << 31), "spei_frames_u16_in: bad frame shape %d x %dx%d", N, H, W);
    SPEI_REQUIRE(depth == 10 || depth == 12, "spei_frames_u16_in: unknown depth %d (10 or 12)", depth);
    SPEI_REQUIRE(N == 1 || frame_stride >= (int64_t)H * W * 6, "spei_frames_u16_in: frame stride %lld < one %dx%d frame of %lld bytes",
                 (long long)frame_stride, H, W, (long long)H * W * 6);
    SPEI_REQUIRE(N == 1 || (frame_stride & 1) == 0, "spei_frames_u16_in: odd frame stride %lld (bytes, a multiple of 2)",
                 (long long)frame_stride);
    SPEI_REQUIRE(((uintptr_t)src & 1) == 0, "spei_frames_u16_in: src must be 2-byte aligned");
    const int Hp = (H + MULT - 1) / MULT * MULT, Wp = (W + MULT - 1) / MULT * MULT;
    SPEI_REQUIRE(Hp - H < H && Wp - W < W, "spei_frames_u16_in: a %dx%d frame cannot reflect-pad to %dx%d (the pad must be smaller "
                 "than the frame)", H, W, Hp, Wp);
    SPEI_REQUIRE(!dst || ((uintptr_t)dst & 15) == 0, "spei_frames_u16_in: dst must be 16-byte aligned");
    const int aligned = ((uintptr_t)src & 7) == 0 && (N == 1 || (frame_stride & 7) == 0) && (W & 3) == 0;
    const int64_t total = (int64_t)N * Hp * (Wp / 4);
    const int D = (1 << depth) - 1;
    hipLaunchKernelGGL(frames_u16_in_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, src, N == 1 ? 0 : frame_stride / 2,
                       dst, gray, H, W, Hp, Wp, total, aligned, D, (float)(1.0 / D), (float)(255.0 / D));
    SPEI_CHECK_LAUNCH("spei_frames_u16_in");
    return 0;
}

extern "C" int spei_frame_u16_out(const float* src, uint16_t* dst, int* nonfinite, int H, int W, int Hp, int Wp, int depth,
                                  spei_stream_t stream) {
    SPEI_REQUIRE(src && dst, "spei_frame_u16_out: null pointer");
    SPEI_REQUIRE(H > 0 && W > 0 && Hp >= H && Wp >= W && (int64_t)Hp * Wp < (1ll << 30),
                 "spei_frame_u16_out: bad sizes (crop %dx%d of a %dx%d frame)", H, W, Hp, Wp);
    SPEI_REQUIRE(depth == 10 || depth == 12, "spei_frame_u16_out: unknown depth %d (10 or 12)", depth);
    SPEI_REQUIRE(((uintptr_t)dst & 1) == 0, "spei_frame_u16_out: dst must be 2-byte aligned");
    const int gw = (W + 3) / 4;
    const int vec_in = (Wp & 3) == 0 && ((uintptr_t)src & 15) == 0;
    const int vec_out = (W & 3) == 0 && ((uintptr_t)dst & 7) == 0;
    const int64_t total = (int64_t)H * gw;
    if (nonfinite && hipMemsetAsync(nonfinite, 0, sizeof(int), (hipStream_t)stream) != hipSuccess) {
        spei_set_error("spei_frame_u16_out: clearing the non-finite flag failed");
        return -2;
    }
    hipLaunchKernelGGL(frame_u16_out_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, src, dst, nonfinite, H, W, Wp,
                       (int64_t)Hp * Wp, gw, total, vec_in, vec_out, (float)((1 << depth) - 1));
    SPEI_CHECK_LAUNCH("spei_frame_u16_out");
    return 0;
}

extern "C" int spei_frame_pair_stats_u16(const uint16_t* src, int64_t frame_stride, const uint16_t* prev, int N, int H, int W, int depth,
                                         int* hist, int64_t* sad, spei_stream_t stream) {
    SPEI_REQUIRE(src && hist && sad, "spei_frame_pair_stats_u16: null pointer (src, hist and sad are required)");
    SPEI_REQUIRE(N >= 1 && N <= 65535, "spei_frame_pair_stats_u16: %d frames (1..65535 per call)", N);
    SPEI_REQUIRE(N > 1 || prev, "spei_frame_pair_stats_u16: one frame and no prev make no pair");
    SPEI_REQUIRE(H > 0 && W > 0 && (int64_t)H * W * 3 < (1ll << 31), "spei_frame_pair_stats_u16: bad frame shape %dx%d", H, W);
    SPEI_REQUIRE(depth == 10 || depth == 12, "spei_frame_pair_stats_u16: unknown depth %d (10 or 12)", depth);
    SPEI_REQUIRE(N == 1 || frame_stride >= (int64_t)H * W * 6, "spei_frame_pair_stats_u16: frame stride %lld < one %dx%d frame of %lld "
                 "bytes", (long long)frame_stride, H, W, (long long)H * W * 6);
    SPEI_REQUIRE(N == 1 || (frame_stride & 1) == 0, "spei_frame_pair_stats_u16: odd frame stride %lld (bytes, a multiple of 2)",
                 (long long)frame_stride);
    SPEI_REQUIRE((((uintptr_t)src | (uintptr_t)prev) & 1) == 0, "spei_frame_pair_stats_u16: src and prev must be 2-byte aligned");
    const int64_t pixels = (int64_t)H * W, blocks = ((pixels + 3) / 4 + 255) / 256;
    const int pairs = prev ? N : N - 1;
    if (hipMemsetAsync(hist, 0, sizeof(int) * PAIR_BINS * N, (hipStream_t)stream) != hipSuccess ||
        hipMemsetAsync(sad, 0, sizeof(int64_t) * pairs, (hipStream_t)stream) != hipSuccess) {
        spei_set_error("spei_frame_pair_stats_u16: clearing the results failed");
        return -2;
    }
    hipLaunchKernelGGL(frame_pair_stats_u16_kernel, dim3((int)(blocks < PAIR_BLOCKS ? blocks : PAIR_BLOCKS), N), dim3(256), 0,
                       (hipStream_t)stream, src, N == 1 ? 0 : frame_stride / 2, prev, hist, reinterpret_cast<unsigned long long*>(sad),
                       pixels, depth - 8);
    SPEI_CHECK_LAUNCH("spei_frame_pair_stats_u16");
    return 0;
}
