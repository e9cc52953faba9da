// Data-set synthesis (speinet_amd/blurset.py): the reference makes its GoProS-style sets from sharp high-frame-rate footage by
// averaging runs of 1..15 consecutive frames (LD_detector/mix_choice_dataset.py:46-71 _generate_blurry_sequence_, :99-108 the uint8
// frames it writes; sharp_detector_params_estimation_parallel.py:50-76 generate_blurry_sequence).
//
//   spei_window_mean_u8 — T packed uint8 [H][W][3] frames on the device and a table of M runs (start, length), 1 <= length <= 15.
//                         Per run m:  blur[m] = floor(sum_{t < length} frame[start + t] / length) per byte, in integer arithmetic
//                         (== np.mean(window, axis=0) -> float32 -> astype(uint8), :61 and :104: a non-integer quotient with
//                         length <= 15 lies at least 1/15 from an integer, far more than float32 rounding at 255);
//                                     gt[m]   = frame[start + length / 2]  (:62);
//                                     gray[m] = the detector's gray plane of blur[m] (spei_gray_px, as spei_frames_u8_in writes it).
//
// One launch for all runs.  HBM-bound by construction: every source frame of a run is read once (the gt frame a second time, from
// cache) and two frames are written per run, so a clip of T frames in M runs moves (T + 2 M) * H*W*3 bytes plus 4 * M * H*W for the
// gray planes: 720p, T = 480 in M = 80 runs: 1.77 GB + 0.29 GB.  Vector path (H*W a multiple of 16, pointers and frame stride
// 16-byte aligned): one thread per 16 pixels, three 16-byte loads per source frame, three 16-byte stores per output frame, four per
// gray plane.  Otherwise one thread per pixel with byte accesses.  The quotient is a multiply and a shift: with m = ceil(2^16 / n),
// (s * m) >> 16 == s / n for every s <= 15 * 255 and n <= 15 (the error term s * (m n - 2^16) stays below 2^16).
//
//   spei_window_mean_light_u8 — the same launch with the run averaged in LINEAR light (csrc/light.h; an extension beyond the reference):
//                         every source byte is decoded through lin[] (one LDS read), the sums are 32-bit, the quotient is light.h's
//                         multiply-high and the result is encoded by a binary search over thr[] (eight LDS reads per output byte);
//                         gt and the gray plane of the ENCODED bytes as above.  Both kernels are the templates below with LIGHT set: the
//                         tables are staged by the workgroup before its first item, and a run of length 1 copies its bytes
//                         (encode(lin[c]) == c) without touching them.  Same traffic as the code-value launch.
//
//   spei_window_mean_noise_u8 — the light launch with sensor noise between the quotient and the encode (csrc/light.h, NOISE set): the
//                         workgroup also stages the gauss table (4 KB more LDS), a thread makes one Philox call per pixel on the
//                         counter (x, y, run, clip) — x, y from the pixel's index in the frame — and spends a 64-bit multiply-high, an
//                         fp32 square root with two integer corrections and a 64-bit multiply per byte.  A run of length 1 still copies.
#include "common.h"
#include "light.h"
#include "run_checks.h"

namespace {

__device__ __forceinline__ uint32_t quot(uint32_t s, uint32_t magic) { return (s * magic) >> 16; }

template <bool LIGHT>
__device__ __forceinline__ uint32_t mean_of(uint32_t sum, uint32_t magic, const uint32_t* tab) {
    if constexpr (LIGHT) return light_encode(tab + 256, light_quot(sum, magic));
    else return quot(sum, magic);
}

// The per-run constants of a NOISE launch (uniform over the workgroup)
struct RunNoise {
    uint32_t run, clip, A, key0, key1;
    uint64_t B, magic;
    const int32_t* gauss;                                  // in LDS
};

// sums of one pixel's three bytes -> its encoded bytes, with noise; (x, y): the pixel in its frame
__device__ __forceinline__ void noisy_pixel(uint32_t* acc3, uint32_t magic, const uint32_t* tab, const RunNoise& rn, uint32_t x, uint32_t y) {
    uint32_t w[3];
    philox3(x, y, rn.run, rn.clip, rn.key0, rn.key1, w);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        acc3[c] = light_encode(tab + 256, noise_apply(light_quot(acc3[c], magic), gauss_z(rn.gauss, w[c]), rn.A, rn.B, rn.magic));
}

// stage the tables of a run of 2 or more frames (all 256 threads) and read the run's noise record
__device__ __forceinline__ RunNoise run_noise(int32_t* lds, const NoiseArgs& na, int m, int len) {
    if (len > 1) gauss_stage(lds, na.gauss);
    const spei_noise_record r = na.rec[m];
    return RunNoise{r.run, r.clip, r.A, na.key0, na.key1, r.B, len > 1 ? noise_magic(len) : 0ull, lds};
}

template <bool LIGHT, bool NOISE>
__global__ __launch_bounds__(256) void window_mean_vec_kernel(const unsigned char* __restrict__ src, int64_t fstride, const int* __restrict__ runs,
                                                              const uint32_t* __restrict__ tables, unsigned char* __restrict__ blur,
                                                              unsigned char* __restrict__ gt, float* __restrict__ gray, int64_t hw, NoiseArgs na,
                                                              uint32_t W) {
    static_assert(LIGHT || !NOISE, "noise is added in a linear light");
    const int m = blockIdx.y;
    const int start = runs[2 * m], len = runs[2 * m + 1];
    const uint32_t* tab = nullptr;                         // LIGHT: lin[256], thr[256] in LDS
    if constexpr (LIGHT) {
        __shared__ uint32_t lds[LIGHT_WORDS];
        if (len > 1) light_stage(lds, tables);
        tab = lds;
    }
    RunNoise rn;                                           // NOISE: the gauss table in LDS and the run's record
    if constexpr (NOISE) {
        __shared__ int32_t glds[GAUSS_WORDS];
        rn = run_noise(glds, na, m, len);
    }
    const bool copy = LIGHT && len == 1;                   // a run of length 1 returns its bytes; the tables are not staged
    const uint32_t magic = LIGHT ? (copy ? 0u : light_magic(len)) : (65536u + len - 1) / len;
    const int64_t groups = hw >> 4;                        // 16 pixels = 48 bytes per thread
    const int64_t nb = hw * 3;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < groups; i += (int64_t)gridDim.x * 256) {
        uint32_t acc[48];
#pragma unroll
        for (int j = 0; j < 48; ++j) acc[j] = 0u;
        uint4 mid[3];
        for (int t = 0; t < len; ++t) {
            const uint4* p = reinterpret_cast<const uint4*>(src + (start + t) * fstride + i * 48);
            const uint4 q[3] = {p[0], p[1], p[2]};
            if (t == len / 2) { mid[0] = q[0]; mid[1] = q[1]; mid[2] = q[2]; }
            if (copy) break;
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const uint32_t w[4] = {q[v].x, q[v].y, q[v].z, q[v].w};
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
                    if constexpr (LIGHT) acc[16 * v + j] += tab[b];
                    else acc[16 * v + j] += b;
                }
            }
        }
        if (copy) {
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const uint32_t w[4] = {mid[v].x, mid[v].y, mid[v].z, mid[v].w};
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[16 * v + j] = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
            }
        } else {
            if constexpr (NOISE) {
                uint32_t y = (uint32_t)(i * 16) / W, x = (uint32_t)(i * 16) - y * W;       // H * W * 3 < 2^31
#pragma unroll
                for (int px = 0; px < 16; ++px) {
                    noisy_pixel(acc + 3 * px, magic, tab, rn, x, y);
                    if (++x == W) { x = 0u; ++y; }
                }
            } else {
#pragma unroll
                for (int j = 0; j < 48; ++j) acc[j] = mean_of<LIGHT>(acc[j], magic, tab);
            }
        }
        uint4* b = reinterpret_cast<uint4*>(blur + m * nb + i * 48);
        uint4* g = reinterpret_cast<uint4*>(gt + m * nb + i * 48);
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 16; ++j) w[j >> 2] |= acc[16 * v + j] << (8 * (j & 3));
            b[v] = make_uint4(w[0], w[1], w[2], w[3]);
            g[v] = mid[v];
        }
        if (gray) {
            float4* y = reinterpret_cast<float4*>(gray + m * hw + i * 16);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                float e[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int px = 4 * v + j;
                    e[j] = spei_gray_px((float)acc[3 * px], (float)acc[3 * px + 1], (float)acc[3 * px + 2]);
                }
                y[v] = make_float4(e[0], e[1], e[2], e[3]);
            }
        }
    }
}

template <bool LIGHT, bool NOISE>
__global__ __launch_bounds__(256) void window_mean_px_kernel(const unsigned char* __restrict__ src, int64_t fstride, const int* __restrict__ runs,
                                                             const uint32_t* __restrict__ tables, unsigned char* __restrict__ blur,
                                                             unsigned char* __restrict__ gt, float* __restrict__ gray, int64_t hw, NoiseArgs na,
                                                             uint32_t W) {
    static_assert(LIGHT || !NOISE, "noise is added in a linear light");
    const int m = blockIdx.y;
    const int start = runs[2 * m], len = runs[2 * m + 1];
    const uint32_t* tab = nullptr;                         // LIGHT: lin[256], thr[256] in LDS
    if constexpr (LIGHT) {
        __shared__ uint32_t lds[LIGHT_WORDS];
        if (len > 1) light_stage(lds, tables);
        tab = lds;
    }
    RunNoise rn;                                           // NOISE: the gauss table in LDS and the run's record
    if constexpr (NOISE) {
        __shared__ int32_t glds[GAUSS_WORDS];
        rn = run_noise(glds, na, m, len);
    }
    const bool copy = LIGHT && len == 1;                   // a run of length 1 returns its bytes; the tables are not staged
    const uint32_t magic = LIGHT ? (copy ? 0u : light_magic(len)) : (65536u + len - 1) / len;
    const int64_t nb = hw * 3;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
        uint32_t acc[3] = {0u, 0u, 0u};
        for (int t = 0; t < len && !copy; ++t) {
            const unsigned char* p = src + (start + t) * fstride + i * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if constexpr (LIGHT) acc[c] += tab[p[c]];
                else acc[c] += p[c];
            }
        }
        const unsigned char* p = src + (start + len / 2) * fstride + i * 3;
        if constexpr (NOISE)
            if (!copy) noisy_pixel(acc, magic, tab, rn, (uint32_t)i % W, (uint32_t)i / W);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (!NOISE) acc[c] = copy ? (uint32_t)p[c] : mean_of<LIGHT>(acc[c], magic, tab);
            else if (copy) acc[c] = (uint32_t)p[c];
            blur[m * nb + i * 3 + c] = (unsigned char)acc[c];
            gt[m * nb + i * 3 + c] = p[c];
        }
        if (gray) gray[m * hw + i] = spei_gray_px((float)acc[0], (float)acc[1], (float)acc[2]);
    }
}

// The runs are checked on the host copy (run_checks.h; LIGHT: the tables on theirs): the kernels never meet a run that leaves the clip
template <bool LIGHT, bool NOISE = false>
int window_mean(const char* name, const unsigned char* src, int64_t frame_stride, int T, const int* runs, const int* runs_host, int M,
                const uint32_t* tables, const uint32_t* tables_host, unsigned char* blur, unsigned char* gt, float* gray, int H, int W,
                spei_stream_t stream, const int32_t* gauss = nullptr, const int32_t* gauss_host = nullptr,
                const spei_noise_record* noise = nullptr, const spei_noise_record* noise_host = nullptr, uint32_t key0 = 0u,
                uint32_t key1 = 0u) {
    if (window_runs_check(name, src, frame_stride, T, runs, runs_host, M, blur, gt, H, W)) return -1;
    const int64_t hw = (int64_t)H * W;
    if constexpr (LIGHT)
        if (light_check(name, tables, tables_host)) return -1;
    if constexpr (NOISE)
        if (noise_check(name, gauss, gauss_host, noise, noise_host, M)) return -1;
    const NoiseArgs na{gauss, noise, key0, key1};
    const bool vec = (hw & 15) == 0 && (((uintptr_t)src | (uintptr_t)blur | (uintptr_t)gt | (uintptr_t)gray) & 15) == 0 &&
                     (T == 1 || (frame_stride & 15) == 0);
    const int64_t items = vec ? hw >> 4 : hw;
    const int64_t bx = (items + 255) / 256;
    const dim3 grid((unsigned)(bx < 4096 ? bx : 4096), (unsigned)M);
    if (vec)
        hipLaunchKernelGGL((window_mean_vec_kernel<LIGHT, NOISE>), grid, dim3(256), 0, (hipStream_t)stream, src, frame_stride, runs, tables, blur,
                           gt, gray, hw, na, (uint32_t)W);
    else
        hipLaunchKernelGGL((window_mean_px_kernel<LIGHT, NOISE>), grid, dim3(256), 0, (hipStream_t)stream, src, frame_stride, runs, tables, blur,
                           gt, gray, hw, na, (uint32_t)W);
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

}  // namespace

extern "C" int spei_window_mean_u8(const unsigned char* src, int64_t frame_stride, int T, const int* runs, const int* runs_host, int M,
                                   unsigned char* blur, unsigned char* gt, float* gray, int H, int W, spei_stream_t stream) {
    return window_mean<false>("spei_window_mean_u8", src, frame_stride, T, runs, runs_host, M, nullptr, nullptr, blur, gt, gray, H, W, stream);
}

extern "C" int spei_window_mean_light_u8(const unsigned char* src, int64_t frame_stride, int T, const int* runs, const int* runs_host, int M,
                                         const uint32_t* tables, const uint32_t* tables_host, unsigned char* blur, unsigned char* gt,
                                         float* gray, int H, int W, spei_stream_t stream) {
    return window_mean<true>("spei_window_mean_light_u8", src, frame_stride, T, runs, runs_host, M, tables, tables_host, blur, gt, gray, H, W,
                             stream);
}

extern "C" int spei_window_mean_noise_u8(const unsigned char* src, int64_t frame_stride, int T, const int* runs, const int* runs_host, int M,
                                         const uint32_t* tables, const uint32_t* tables_host, const int32_t* gauss, const int32_t* gauss_host,
                                         const spei_noise_record* noise, const spei_noise_record* noise_host, uint32_t key0, uint32_t key1,
                                         unsigned char* blur, unsigned char* gt, float* gray, int H, int W, spei_stream_t stream) {
    return window_mean<true, true>("spei_window_mean_noise_u8", src, frame_stride, T, runs, runs_host, M, tables, tables_host, blur, gt, gray, H,
                                   W, stream, gauss, gauss_host, noise, noise_host, key0, key1);
}
