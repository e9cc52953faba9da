// Frame I/O of the clip API (speinet_amd/video.py): uint8 frames of any size in, uint8 frames of the same size out, and the same for
// deep frames (10 and 12 bits in 16-bit words; depth d, D = 2^d - 1; a word above D reads as D).
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
//   spei_frames_u16_in, spei_frame_u16_out, spei_frame_pair_stats_u16 — the same three on uint16 samples of `depth` bits: values
//                        v * (float)(1 / D), the gray plane of v * (float)(255 / D), round_half_even(clamp(x * D, 0, D)), the luma
//                        and its histogram at the depth of the samples (bins of Y >> (depth - 6)).
//
//   spei_frame_requant — a packed frame of in_depth 8, 10 or 12 -> the same frame at out_depth 8, 10 or 12, every sample requant(v) of
//                        pixel_group.h (the value spei_roi_paste_* writes outside its rectangle; a copy at equal depths): the frame
//                        the clip API hands out for a frame it keeps (video.deblur_clip(..., sharp="keep"); an extension, the
//                        reference deblurs every frame).  One flat streaming launch.
//
// One kernel per entry-point pair, templated on the sample type T; the pixel group they stream is in pixel_group.h.  The mirrored
// indices are computed in the pad band only.
#include "pixel_group.h"

namespace {

// T = unsigned char (D = 255, inv = INV255; to255 unused) or uint16_t (D = 2^depth - 1, inv = (float)(1.0 / D), to255 =
// (float)(255.0 / D)); fstride in samples
template <typename T>
__global__ __launch_bounds__(256) void frames_in_kernel(const T* __restrict__ src, int64_t fstride, float* __restrict__ dst,
                                                        float* __restrict__ gray, int H, int W, int Hp, int Wp, int64_t total, int aligned,
                                                        int D, float inv, float to255) {
    const int gw = Wp >> 2;                                // groups per padded row (Wp % 20 == 0)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / gw;                        // n * Hp + y
        const int x0 = (int)(i - row * gw) * 4;
        const int n = (int)(row / Hp), y = (int)(row - (int64_t)n * Hp);
        if (!dst && y >= H) continue;                      // gray only: the pad rows have nothing to write
        const int sy = y < H ? y : 2 * H - 2 - y;
        float v[3][4];
        ingest_group(src + n * fstride + (int64_t)sy * W * 3, x0, W, aligned != 0, D, v);
        if (gray && y < H) {                               // the detector's 0..255 scale, a deep frame's extra bits kept
            float* g = gray + ((int64_t)n * H + y) * W;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < W) {
                    if constexpr (sizeof(T) == 1) g[x0 + k] = spei_gray_px(v[0][k], v[1][k], v[2][k]);
                    else g[x0 + k] = spei_gray_px(v[0][k] * to255, v[1][k] * to255, v[2][k] * to255);
                }
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

// T = unsigned char (Df = 255) or uint16_t (Df = 2^depth - 1)
template <typename T>
__global__ __launch_bounds__(256) void frame_out_kernel(const float* __restrict__ src, T* __restrict__ dst, int* __restrict__ nonfinite,
                                                        int H, int W, int Wp, int64_t plane, int gw, int64_t total, int vec_in,
                                                        int vec_out, float Df) {
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / gw), x0 = (int)(i - (int64_t)y * gw) * 4;
        const float* s = src + (int64_t)y * Wp + x0;
        uint32_t q[3][4];
        if (vec_in) {                                      // Wp % 4 == 0: x0 + 4 <= Wp; columns W.. of the group are pad, not the crop
            bad |= quantise_planes(s, plane, Df, W - x0, q);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float v = x0 + k < W ? s[c * plane + k] : 0.0f;
                    q[c][k] = quantise(v, Df);
                    bad |= isfinite(v) ? 0 : 1;
                }
        }
        store_group(dst + ((int64_t)y * W + x0) * 3, q, vec_out != 0, W - x0);
    }
    if (nonfinite && bad) atomicOr(nonfinite, 1);           // rare: one atomic per thread that met a non-finite value
}

// ---- a frame at another depth --------------------------------------------------------------------------------------------------
// A packed frame is one run of independent samples, so this kernel has no pixel group.  A thread takes a run of samples at a time: the
// side with the wider samples moves as one 16-byte access and the other side as one access of the same samples (16 bytes, or 8 where
// uint8 meets uint16), so a wave reads and writes whole contiguous lines with one instruction each, where two 16-byte stores per
// lane, 32 bytes apart, would fill every line in two halves.  This runs where both bases lie on 16-byte boundaries
// (`vecs` whole runs; 0 otherwise); the samples behind the last whole run go one by one.  The two depths are template arguments:
// `requant` then folds to one constant divisor (a multiply and a shift), or to nothing at equal depths.
template <int DEPTH> struct SampleOf { typedef uint16_t type; };
template <> struct SampleOf<8> { typedef unsigned char type; };
constexpr int requant_run(int in_depth, int out_depth) { return in_depth == 8 && out_depth == 8 ? 16 : 8; }     // samples per thread

template <int N> struct Words { typedef uint4 type; };                         // N dwords as one access
template <> struct Words<2> { typedef uint2 type; };
__device__ __forceinline__ void unpack_words(const uint4& v, uint32_t (&w)[4]) { w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
__device__ __forceinline__ void unpack_words(const uint2& v, uint32_t (&w)[2]) { w[0] = v.x; w[1] = v.y; }
__device__ __forceinline__ uint4 pack_words(const uint32_t (&w)[4]) { return make_uint4(w[0], w[1], w[2], w[3]); }
__device__ __forceinline__ uint2 pack_words(const uint32_t (&w)[2]) { return make_uint2(w[0], w[1]); }

template <int IN, int OUT>
__global__ __launch_bounds__(256) void frame_requant_kernel(const typename SampleOf<IN>::type* __restrict__ src,
                                                            typename SampleOf<OUT>::type* __restrict__ dst, int64_t total, int64_t vecs) {
    typedef typename SampleOf<IN>::type TI;
    typedef typename SampleOf<OUT>::type TO;
    constexpr int Din = (1 << IN) - 1, Dout = (1 << OUT) - 1, RUN = requant_run(IN, OUT);
    constexpr int NI = RUN * (int)sizeof(TI) / 4, NO = RUN * (int)sizeof(TO) / 4, PI = 4 / (int)sizeof(TI), PO = 4 / (int)sizeof(TO);
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    for (int64_t i = t; i < vecs; i += step) {
        uint32_t w[NI], o[NO];
        unpack_words(reinterpret_cast<const typename Words<NI>::type*>(src)[i], w);
#pragma unroll
        for (int k = 0; k < NO; ++k) o[k] = 0u;
#pragma unroll
        for (int j = 0; j < RUN; ++j) {                    // sample j: PI of them per dword read, PO per dword written
            const int v = sample_of((TI)(w[j / PI] >> (32 / PI * (j % PI))), Din);
            o[j / PO] |= requant(v, Din, Dout) << (32 / PO * (j % PO));
        }
        reinterpret_cast<typename Words<NO>::type*>(dst)[i] = pack_words(o);
    }
    for (int64_t j = vecs * RUN + t; j < total; j += step) dst[j] = (TO)requant(sample_of(src[j], Din), Din, Dout);
}

// ---- pair statistics -----------------------------------------------------------------------------------------------------------
// grid (x, n): the blocks of column n stream frame n (member b of its pair: its histogram) beside the frame before it (member a:
// frame n - 1, or `prev` for n = 0, or none), so a frame is read twice at most.  Rows are packed, so a frame is one run of H * W
// pixels: groups of 4 pixels as three words when both frames start on a GROUP_MASK boundary, samples otherwise and in the last,
// partial group.  Histogram counts go to one LDS copy per wave; SAD partials are summed per wave; each block then issues one integer
// atomic per non-empty bin and one 64-bit atomic for its SAD (Guideline 12: integer adds commute exactly).
constexpr int PAIR_BLOCKS = 256;                           // blocks per frame
constexpr int PAIR_BINS = 64;
// A thread adds at most 4 * D per group, and a frame holds fewer than 2^31 / 12 groups (the bound of spei_frames_u8_in), so with
// PAIR_BLOCKS blocks of 256 threads a thread holds at most 2732 groups.  At 8 bits even a whole block's SAD fits 32 bits; at 12 bits
// a wave's does and a block's need not: the four wave sums are added in 64 bits by one thread, which issues the block's one global
// atomic.
static_assert((((1ll << 31) / 12) / (256ll * PAIR_BLOCKS) + 1) * 256 * 4 * 255 < (1ll << 32), "pair SAD: a block's sum must fit 32 bits");
static_assert((((1ll << 31) / 12) / (256ll * PAIR_BLOCKS) + 1) * 64 * 4 * 4095 < (1ll << 32), "pair SAD: a wave's sum must fit 32 bits");

// a group as the kernel holds it: the clamped samples of a deep frame, the three packed dwords of a uint8 frame
template <typename T> struct PairGroup { typedef int type[12]; };
template <> struct PairGroup<unsigned char> { typedef uint32_t type[3]; };

// s = depth - 8: D = 2^(8 + s) - 1, the bins are Y >> (2 + s); fstride in samples
template <typename T>
__global__ __launch_bounds__(256) void frame_pair_stats_kernel(const T* __restrict__ src, int64_t fstride, const T* __restrict__ prev,
                                                               int* __restrict__ hist, unsigned long long* __restrict__ sad,
                                                               int64_t pixels, int s) {
    __shared__ unsigned int bins[4][PAIR_BINS];
    __shared__ unsigned int wave_sad[4];
    const int n = blockIdx.y, wave = threadIdx.x >> 6, D = (256 << s) - 1;
    const T* b = src + n * fstride;
    const T* a = n > 0 ? b - fstride : prev;               // null: frame 0 of a call without `prev` has no pair
    const bool aligned = (((uintptr_t)b | (uintptr_t)a) & GROUP_MASK<T>) == 0;
    (&bins[0][0])[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t groups = (pixels + 3) >> 2, full = pixels >> 2;
    unsigned int part = 0u;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        const int valid = g < full ? 4 : (int)(pixels - 4 * g);
        typename PairGroup<T>::type cb, ca;
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

// the checks that the entry points taking N frames with a byte stride share: the depth, then the stride
template <typename T>
int check_clip(const char* name, int N, int H, int W, int64_t frame_stride, int depth) {
    SPEI_REQUIRE(sizeof(T) == 1 || depth == 10 || depth == 12, "%s: unknown depth %d (10 or 12)", name, depth);
    const int64_t bytes = (int64_t)H * W * 3 * (int64_t)sizeof(T);
    if constexpr (sizeof(T) == 1)
        SPEI_REQUIRE(N == 1 || frame_stride >= bytes, "%s: frame stride %lld < one %dx%d frame", name, (long long)frame_stride, H, W);
    else
        SPEI_REQUIRE(N == 1 || frame_stride >= bytes, "%s: frame stride %lld < one %dx%d frame of %lld bytes", name,
                     (long long)frame_stride, H, W, (long long)bytes);
    SPEI_REQUIRE(N == 1 || (frame_stride & (sizeof(T) - 1)) == 0, "%s: odd frame stride %lld (bytes, a multiple of 2)", name,
                 (long long)frame_stride);
    return 0;
}

template <typename T>
int frames_in(const char* name, const T* src, int64_t frame_stride, float* dst, float* gray, int N, int H, int W, int depth,
              hipStream_t stream) {
    SPEI_REQUIRE(src && (dst || gray), "%s: null pointer (src, and dst or gray, are required)", name);
    SPEI_REQUIRE(N > 0 && H > 0 && W > 0 && (int64_t)H * W * 3 < (1ll << 31), "%s: bad frame shape %d x %dx%d", name, N, H, W);
    if (check_clip<T>(name, N, H, W, frame_stride, depth)) return -1;
    SPEI_REQUIRE(((uintptr_t)src & (sizeof(T) - 1)) == 0, "%s: src must be 2-byte aligned", name);
    const int Hp = (H + MULT - 1) / MULT * MULT, Wp = (W + MULT - 1) / MULT * MULT;
    SPEI_REQUIRE(Hp - H < H && Wp - W < W, "%s: a %dx%d frame cannot reflect-pad to %dx%d (the pad must be smaller than the frame)", name,
                 H, W, Hp, Wp);
    SPEI_REQUIRE(!dst || ((uintptr_t)dst & 15) == 0, "%s: dst must be 16-byte aligned", name);
    const int aligned = ((uintptr_t)src & GROUP_MASK<T>) == 0 && (N == 1 || (frame_stride & GROUP_MASK<T>) == 0) && (W & 3) == 0;
    const int64_t total = (int64_t)N * Hp * (Wp / 4);
    const int D = sizeof(T) == 1 ? 255 : (1 << depth) - 1;
    hipLaunchKernelGGL(frames_in_kernel<T>, dim3(grid_for(total)), dim3(256), 0, stream, src,
                       N == 1 ? 0 : frame_stride / (int64_t)sizeof(T), dst, gray, H, W, Hp, Wp, total, aligned, D,
                       sizeof(T) == 1 ? INV255 : (float)(1.0 / D), (float)(255.0 / D));
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

template <typename T>
int frame_out(const char* name, const float* src, T* dst, int* nonfinite, int H, int W, int Hp, int Wp, int depth, hipStream_t stream) {
    SPEI_REQUIRE(src && dst, "%s: null pointer", name);
    SPEI_REQUIRE(H > 0 && W > 0 && Hp >= H && Wp >= W && (int64_t)Hp * Wp < (1ll << 30), "%s: bad sizes (crop %dx%d of a %dx%d frame)",
                 name, H, W, Hp, Wp);
    SPEI_REQUIRE(sizeof(T) == 1 || depth == 10 || depth == 12, "%s: unknown depth %d (10 or 12)", name, depth);
    SPEI_REQUIRE(((uintptr_t)dst & (sizeof(T) - 1)) == 0, "%s: dst must be 2-byte aligned", name);
    const int gw = (W + 3) / 4;
    const int vec_in = (Wp & 3) == 0 && ((uintptr_t)src & 15) == 0;
    const int vec_out = (W & 3) == 0 && ((uintptr_t)dst & GROUP_MASK<T>) == 0;
    const int64_t total = (int64_t)H * gw;
    if (nonfinite && hipMemsetAsync(nonfinite, 0, sizeof(int), stream) != hipSuccess) {
        spei_set_error("%s: clearing the non-finite flag failed", name);
        return -2;
    }
    hipLaunchKernelGGL(frame_out_kernel<T>, dim3(grid_for(total)), dim3(256), 0, stream, src, dst, nonfinite, H, W, Wp, (int64_t)Hp * Wp,
                       gw, total, vec_in, vec_out, sizeof(T) == 1 ? 255.0f : (float)((1 << depth) - 1));
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

int frame_requant(const char* name, const void* src, int in_depth, void* dst, int out_depth, int H, int W, hipStream_t stream) {
    SPEI_REQUIRE(src && dst, "%s: null pointer", name);
    SPEI_REQUIRE(in_depth == 8 || in_depth == 10 || in_depth == 12, "%s: unknown in_depth %d (8, 10 or 12)", name, in_depth);
    SPEI_REQUIRE(out_depth == 8 || out_depth == 10 || out_depth == 12, "%s: unknown out_depth %d (8, 10 or 12)", name, out_depth);
    SPEI_REQUIRE(H > 0 && W > 0 && (int64_t)H * W * 3 < (1ll << 31), "%s: bad frame shape %dx%d", name, H, W);
    const int in_bytes = in_depth == 8 ? 1 : 2, out_bytes = out_depth == 8 ? 1 : 2;
    SPEI_REQUIRE(((uintptr_t)src & (in_bytes - 1)) == 0 && ((uintptr_t)dst & (out_bytes - 1)) == 0,
                 "%s: misaligned pointer (deep frames are 2-byte aligned)", name);
    const int64_t total = (int64_t)H * W * 3;
    SPEI_REQUIRE(!bytes_overlap(dst, total * out_bytes, src, total * in_bytes), "%s: dst overlaps src", name);
    const int run = requant_run(in_depth, out_depth);
    const int64_t vecs = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0 ? total / run : 0;
    const dim3 grid(grid_for(vecs > total - vecs * run ? vecs : total - vecs * run));
#define SPEI_REQUANT(IN, OUT)                                                                                               \
    case IN * 16 + OUT:                                                                                                     \
        hipLaunchKernelGGL((frame_requant_kernel<IN, OUT>), grid, dim3(256), 0, stream,                                     \
                           static_cast<const SampleOf<IN>::type*>(src), static_cast<SampleOf<OUT>::type*>(dst), total, vecs); \
        break
    switch (in_depth * 16 + out_depth) {
        SPEI_REQUANT(8, 8); SPEI_REQUANT(8, 10); SPEI_REQUANT(8, 12);
        SPEI_REQUANT(10, 8); SPEI_REQUANT(10, 10); SPEI_REQUANT(10, 12);
        SPEI_REQUANT(12, 8); SPEI_REQUANT(12, 10); SPEI_REQUANT(12, 12);
    }
#undef SPEI_REQUANT
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

template <typename T>
int frame_pair_stats(const char* name, const T* src, int64_t frame_stride, const T* prev, int N, int H, int W, int depth, int* hist,
                     int64_t* sad, hipStream_t stream) {
    SPEI_REQUIRE(src && hist && sad, "%s: null pointer (src, hist and sad are required)", name);
    SPEI_REQUIRE(N >= 1 && N <= 65535, "%s: %d frames (1..65535 per call)", name, N);
    SPEI_REQUIRE(N > 1 || prev, "%s: one frame and no prev make no pair", name);
    SPEI_REQUIRE(H > 0 && W > 0 && (int64_t)H * W * 3 < (1ll << 31), "%s: bad frame shape %dx%d", name, H, W);
    if (check_clip<T>(name, N, H, W, frame_stride, depth)) return -1;
    SPEI_REQUIRE((((uintptr_t)src | (uintptr_t)prev) & (sizeof(T) - 1)) == 0, "%s: src and prev must be 2-byte aligned", name);
    const int64_t pixels = (int64_t)H * W, blocks = ((pixels + 3) / 4 + 255) / 256;
    const int pairs = prev ? N : N - 1;
    if (hipMemsetAsync(hist, 0, sizeof(int) * PAIR_BINS * N, stream) != hipSuccess ||
        hipMemsetAsync(sad, 0, sizeof(int64_t) * pairs, stream) != hipSuccess) {
        spei_set_error("%s: clearing the results failed", name);
        return -2;
    }
    hipLaunchKernelGGL(frame_pair_stats_kernel<T>, dim3((int)(blocks < PAIR_BLOCKS ? blocks : PAIR_BLOCKS), N), dim3(256), 0, stream, src,
                       N == 1 ? 0 : frame_stride / (int64_t)sizeof(T), prev, hist, reinterpret_cast<unsigned long long*>(sad), pixels,
                       depth - 8);
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

}  // namespace

extern "C" int spei_frames_u8_in(const unsigned char* src, int64_t frame_stride, float* dst, float* gray, int N, int H, int W,
                                 spei_stream_t stream) {
    return frames_in<unsigned char>("spei_frames_u8_in", src, frame_stride, dst, gray, N, H, W, 8, (hipStream_t)stream);
}

extern "C" int spei_frames_u16_in(const uint16_t* src, int64_t frame_stride, float* dst, float* gray, int N, int H, int W, int depth,
                                  spei_stream_t stream) {
    return frames_in<uint16_t>("spei_frames_u16_in", src, frame_stride, dst, gray, N, H, W, depth, (hipStream_t)stream);
}

extern "C" int spei_frame_u8_out(const float* src, unsigned char* dst, int* nonfinite, int H, int W, int Hp, int Wp,
                                 spei_stream_t stream) {
    return frame_out<unsigned char>("spei_frame_u8_out", src, dst, nonfinite, H, W, Hp, Wp, 8, (hipStream_t)stream);
}

extern "C" int spei_frame_u16_out(const float* src, uint16_t* dst, int* nonfinite, int H, int W, int Hp, int Wp, int depth,
                                  spei_stream_t stream) {
    return frame_out<uint16_t>("spei_frame_u16_out", src, dst, nonfinite, H, W, Hp, Wp, depth, (hipStream_t)stream);
}

extern "C" int spei_frame_requant(const void* src, int in_depth, void* dst, int out_depth, int H, int W, spei_stream_t stream) {
    return frame_requant("spei_frame_requant", src, in_depth, dst, out_depth, H, W, (hipStream_t)stream);
}

extern "C" int spei_frame_pair_stats(const unsigned char* src, int64_t frame_stride, const unsigned char* prev, int N, int H, int W,
                                     int* hist, int64_t* sad, spei_stream_t stream) {
    return frame_pair_stats<unsigned char>("spei_frame_pair_stats", src, frame_stride, prev, N, H, W, 8, hist, sad, (hipStream_t)stream);
}

extern "C" int spei_frame_pair_stats_u16(const uint16_t* src, int64_t frame_stride, const uint16_t* prev, int N, int H, int W, int depth,
                                         int* hist, int64_t* sad, spei_stream_t stream) {
    return frame_pair_stats<uint16_t>("spei_frame_pair_stats_u16", src, frame_stride, prev, N, H, W, depth, hist, sad,
                                      (hipStream_t)stream);
}
