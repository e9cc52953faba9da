// Camera-shake blur in blur synthesis (include/speinet_hip.h, "camera-shake blur in blur synthesis"; speinet_amd/shake.py makes the
// PSFs): the run's linear mean Lm is correlated with the record's point-spread function before the noise and the encode,
//     Lb(y, x, c) = (sum w[dy][dx] Lm(clamp(y + dy), clamp(x + dx), c) + 2^15) >> 16,     sum w = 65536, radius r <= 16.
//
//   spei_window_mean_shake_u8      — spei_window_mean_noise_u8 / _light_u8 (blurset.hip) with one spei_shake_record per run
//   spei_train_batch_runs_shake_u8 — spei_train_batch_runs_noise_u8 / _light_u8 (train_batch.hip) with one per table record
//
// A launch whose records all have radius 0 IS the noise (or, gauss == NULL, the light) entry's launch: the steady path is the old path.
// Otherwise one launch of the kernels below.  One workgroup of 256 threads makes one 32 x 32 output tile of one record:
//   1. it stages lin / thr (and the gauss table) as light.h does, and packs the PSF's NON-ZERO taps into LDS — a trajectory PSF has a
//      few dozen to a few hundred of its 1089 taps set — one word each: the weight (17 bits) and the tap's offset in the halo tile
//      (13 bits).  Slots are handed out by an LDS atomic, so the order of the list varies; the sum below is exact, so the result does not;
//   2. it forms Lm for the tile plus a halo of r, coordinates clamped to the FRAME, once per workgroup: up to 64 x 64 pixels, one LDS
//      word per channel in three planes of pitch (width | 1) — odd, so that the 4 rows x 8 groups of a 32-lane half of a ds_read_b32
//      fall on 32 different banks;
//   3. thread t makes 4 pixels of tile row t / 8: per tap one broadcast read of the tap word, 12 reads of Lm and 12 64-bit
//      multiply-adds (w < 2^17, Lm < 2^24, the sum below 2^40 + 2^15); then the noise on the OUTPUT pixel's counter, and the encode;
//   4. window mean: the bytes go to blur, the run's middle frame to gt, the gray plane from the encoded bytes (12-byte / 16-byte
//      accesses when W % 4 == 0 and everything is aligned, bytes otherwise).  Train batch: the four packed pixels go into the 32 x 32
//      LDS tile, and the flip / rotate / store phase is train_batch.hip's (train_tile.h).
// A record with radius 0 in a mixed launch stages no halo and runs no tap loop (Lb = Lm); with a run of length 1 it copies its bytes.
// The noise variance V = X - ceil(X q16 / (n 2^16)) without a division: ceil(P / (n 2^16)) = ceil(c / n) with c = ceil(P / 2^16), and
// ceil(c / n) = c - floor(c (n - 1) / n), which is light.h's multiply-high (c <= X < 2^45); n == 1 has ceil(c / 1) = c.
// LDS: 64.7 KB of dynamic LDS per workgroup, two workgroups per CU.  Plain vector stores only.
#include "common.h"
#include "light.h"
#include "run_checks.h"
#include "train_tile.h"

namespace {

constexpr int MAX_R = 16, PSF_SIDE = 2 * MAX_R + 1, PSF_WORDS = PSF_SIDE * PSF_SIDE;
constexpr int HALO = TILE + 2 * MAX_R, PLANE = HALO * (HALO + 1);        // a plane of Lm: up to 64 rows of pitch up to 65
// the workgroup's dynamic LDS, in words
constexpr int LDS_LM = 0, LDS_TAPS = LDS_LM + 3 * PLANE, LDS_COUNT = LDS_TAPS + PSF_WORDS, LDS_LIGHT = LDS_COUNT + 1,
              LDS_GAUSS = LDS_LIGHT + LIGHT_WORDS, LDS_OUT = LDS_GAUSS + GAUSS_WORDS, LDS_TOTAL = LDS_OUT + TILE * PITCH;
constexpr int TAP_SHIFT = 17;                                            // a tap word: weight | offset << 17

// the frames of one run: `len` frames `fstride` bytes apart, rows `pitch` bytes apart, H x W pixels
struct Run {
    const unsigned char* base;
    int64_t fstride;
    int pitch, len, H, W;
};

// 4 pixels 0x00BBGGRR -> 12 bytes
__device__ __forceinline__ void pack12(const uint32_t px[4], uint32_t w[3]) {
    w[0] = px[0] | (px[1] << 24);
    w[1] = (px[1] >> 8) | (px[2] << 16);
    w[2] = (px[2] >> 16) | (px[3] << 8);
}

// L' = clamp(L + ((isqrt(X - ceil(X q16 / (n 2^16))) z + 2048) >> 12), 0, S), X = A L + B; nmagic = noise_magic(n), 0 for n == 1
__device__ __forceinline__ uint32_t shake_noise_apply(uint32_t L, int32_t z, uint32_t A, uint64_t B, uint32_t q16, uint64_t nmagic) {
    const uint64_t X = (uint64_t)A * L + B;
    const uint64_t c = (X * q16 + 65535ull) >> 16;                       // X q16 < 2^61; c <= X as q16 <= 65536
    const uint64_t V = X - c + __umul64hi(c, nmagic);
    const int64_t d = ((int64_t)noise_isqrt(V) * z + 2048) >> 12;
    const int64_t v = (int64_t)L + d;
    return (uint32_t)(v < 0 ? 0 : v > (int64_t)LIGHT_S ? (int64_t)LIGHT_S : v);
}

// Phases 1 and 2, all 256 threads: the tables, the tap list and Lm of frame rows [y0 - r, y0 + nR + r) x columns [x0 - r, x0 + nC + r),
// clamped to the frame, in planes of pitch hp = (nC + 2 r) | 1.  Ends with a barrier; returns the number of taps.
template <bool NOISE>
__device__ __forceinline__ int shake_stage(uint32_t* lds, const Run& run, const uint32_t* __restrict__ tables, const int32_t* __restrict__ gauss,
                                           const uint32_t* __restrict__ psf, int r, int y0, int x0, int nR, int nC) {
    if (threadIdx.x == 0) lds[LDS_COUNT] = 0u;
    light_stage(lds + LDS_LIGHT, tables);
    if constexpr (NOISE) gauss_stage(reinterpret_cast<int32_t*>(lds + LDS_GAUSS), gauss);
    const int hh = nR + 2 * r, hw = nC + 2 * r, hp = hw | 1;
    const int side = 2 * r + 1;
    if (r > 0) {
        for (int i = threadIdx.x; i < side * side; i += 256) {
            const int ty = i / side, tx = i - ty * side;
            const uint32_t w = psf[(MAX_R - r + ty) * PSF_SIDE + MAX_R - r + tx];
            if (w) lds[LDS_TAPS + atomicAdd(&lds[LDS_COUNT], 1u)] = w | ((uint32_t)(ty * hp + tx) << TAP_SHIFT);
        }
    }
    const uint32_t* lin = lds + LDS_LIGHT;
    const uint32_t magic = run.len > 1 ? light_magic(run.len) : 0u;
    uint32_t* lm = lds + LDS_LM;
    for (int i = threadIdx.x; i < hh * hw; i += 256) {
        const int hy = i / hw, hx = i - hy * hw;
        const int y = min(max(y0 - r + hy, 0), run.H - 1), x = min(max(x0 - r + hx, 0), run.W - 1);
        const unsigned char* p = run.base + (int64_t)y * run.pitch + (int64_t)x * 3;
        uint32_t s[3] = {0u, 0u, 0u};
        for (int t = 0; t < run.len; ++t) {
            const unsigned char* q = p + (int64_t)t * run.fstride;
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] += lin[q[c]];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) lm[c * PLANE + hy * hp + hx] = run.len > 1 ? light_quot(s[c], magic) : s[c];
    }
    __syncthreads();
    return (int)lds[LDS_COUNT];
}

// Phase 3: the 4 pixels at (row, g4 .. g4 + 3) of the tile -> 0x00BBGGRR each.  (x, y): the first pixel in its full frame
template <bool NOISE>
__device__ __forceinline__ void shake_pixels(const uint32_t* lds, int ntaps, int r, int hp, int row, int g4, int len,
                                             const spei_shake_record& sr, const spei_noise_record& nr, const NoiseArgs& na, uint32_t x, uint32_t y,
                                             uint32_t px[4]) {
    const uint32_t* b = lds + LDS_LM + row * hp + g4;
    uint32_t L[12];
    if (r == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) L[3 * k + c] = b[c * PLANE + k];
    } else {
        uint64_t acc[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) acc[j] = 1ull << 15;
        for (int i = 0; i < ntaps; ++i) {
            const uint32_t tap = lds[LDS_TAPS + i];
            const uint32_t w = tap & ((1u << TAP_SHIFT) - 1u);
            const uint32_t* t = b + (tap >> TAP_SHIFT);
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[3 * k + c] += (uint64_t)w * t[c * PLANE + k];
        }
#pragma unroll
        for (int j = 0; j < 12; ++j) L[j] = (uint32_t)(acc[j] >> 16);
    }
    const uint32_t* thr = lds + LDS_LIGHT + 256;
    const uint64_t nmagic = NOISE && len > 1 ? noise_magic(len) : 0ull;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t rnd[3] = {0u, 0u, 0u};
        if constexpr (NOISE) philox3(x + k, y, nr.run, nr.clip, na.key0, na.key1, rnd);
        px[k] = 0u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint32_t v = L[3 * k + c];
            if constexpr (NOISE)
                v = shake_noise_apply(v, gauss_z(reinterpret_cast<const int32_t*>(lds + LDS_GAUSS), rnd[c]), nr.A, nr.B, sr.q16, nmagic);
            px[k] |= light_encode(thr, v) << (8 * c);
        }
    }
}

template <bool NOISE>
__global__ __launch_bounds__(256) void window_mean_shake_kernel(const unsigned char* __restrict__ src, int64_t fstride, const int* __restrict__ runs,
                                                                const uint32_t* __restrict__ tables, const uint32_t* __restrict__ psfs,
                                                                const spei_shake_record* __restrict__ shake, unsigned char* __restrict__ blur,
                                                                unsigned char* __restrict__ gt, float* __restrict__ gray, int H, int W,
                                                                int tiles_x, NoiseArgs na, bool wide) {
    extern __shared__ uint32_t lds[];
    const int m = blockIdx.y;
    const int start = runs[2 * m], len = runs[2 * m + 1];
    const spei_shake_record sr = shake[m];
    const int r = (int)sr.radius;
    const int ty0 = (blockIdx.x / tiles_x) * TILE, tx0 = (blockIdx.x % tiles_x) * TILE;
    const int nR = min(TILE, H - ty0), nC = min(TILE, W - tx0);
    const int row = threadIdx.x >> 3, g4 = (threadIdx.x & 7) * 4;
    const bool copy = r == 0 && len == 1;                                // encode(lin[c]) == c
    const Run run{src + (int64_t)start * fstride, fstride, W * 3, len, H, W};
    int ntaps = 0;
    if (!copy) ntaps = shake_stage<NOISE>(lds, run, tables, na.gauss, psfs + (int64_t)(r ? sr.psf : 0u) * PSF_WORDS, r, ty0, tx0, nR, nC);
    if (row >= nR || g4 >= nC) return;
    const int y = ty0 + row, x = tx0 + g4, nk = min(4, nC - g4);         // nk == 4 when `wide`
    const int64_t at = (int64_t)y * W + x;
    const unsigned char* mid = src + (int64_t)(start + len / 2) * fstride + at * 3;
    uint32_t px[4], g[3];
    if (wide) {
        load12(mid, true, g);
    } else {
        g[0] = g[1] = g[2] = 0u;
        for (int j = 0; j < 3 * nk; ++j) g[j >> 2] |= (uint32_t)mid[j] << (8 * (j & 3));
    }
    if (copy) {
        unpack12(g, px);
    } else {
        spei_noise_record nr{};
        if constexpr (NOISE) nr = na.rec[m];
        shake_pixels<NOISE>(lds, ntaps, r, (nC + 2 * r) | 1, row, g4, len, sr, nr, na, (uint32_t)x, (uint32_t)y, px);
    }
    const int64_t nb = (int64_t)H * W * 3;
    unsigned char* bo = blur + m * nb + at * 3;
    unsigned char* go = gt + m * nb + at * 3;
    if (wide) {
        uint32_t w[3];
        pack12(px, w);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            reinterpret_cast<uint32_t*>(bo)[k] = w[k];
            reinterpret_cast<uint32_t*>(go)[k] = g[k];
        }
    } else {
        for (int k = 0; k < nk; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                bo[3 * k + c] = (unsigned char)(px[k] >> (8 * c));
                go[3 * k + c] = (unsigned char)(g[(3 * k + c) >> 2] >> (8 * ((3 * k + c) & 3)));
            }
    }
    if (gray) {
        float e[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            e[k] = spei_gray_px((float)(px[k] & 0xffu), (float)((px[k] >> 8) & 0xffu), (float)((px[k] >> 16) & 0xffu));
        float* yo = gray + (int64_t)m * H * W + at;
        if (wide && ((uintptr_t)gray & 15) == 0) {
            *reinterpret_cast<float4*>(yo) = make_float4(e[0], e[1], e[2], e[3]);
        } else {
            for (int k = 0; k < nk; ++k) yo[k] = e[k];
        }
    }
}

// train_batch.hip's kernel on run records with the load phase replaced by phases 1..3; the store phase is that kernel's
template <bool NOISE>
__global__ __launch_bounds__(256) void train_batch_shake_kernel(const spei_run_record* __restrict__ table, const uint32_t* __restrict__ tables,
                                                                const uint32_t* __restrict__ psfs, const spei_shake_record* __restrict__ shake,
                                                                int n_in, float* __restrict__ input, float* __restrict__ gt, int P, int tiles,
                                                                float scale, NoiseArgs na) {
    extern __shared__ uint32_t lds[];
    uint32_t* out = lds + LDS_OUT;
    const int rr = blockIdx.y;
    const spei_run_record rec = table[rr];
    const spei_shake_record sr = shake[rr];
    const int r = (int)sr.radius;
    const TileGeom g = tile_geom(rec.flags, P, tiles);
    const int row = threadIdx.x >> 3, g4 = (threadIdx.x & 7) * 4;
    const int nR = g.nR, nC = g.nC;
    if (!g.zero) {
        const int len = rec.length;
        const bool copy = r == 0 && len == 1;
        const int fy = rec.y0 + g.cy_lo, fx = rec.x0 + g.cx_lo;          // the tile's corner in its full frame
        const Run run{reinterpret_cast<const unsigned char*>(rec.src), rec.frame_stride, rec.pitch, len, rec.H, rec.W};
        int ntaps = 0;
        if (!copy) ntaps = shake_stage<NOISE>(lds, run, tables, na.gauss, psfs + (int64_t)(r ? sr.psf : 0u) * PSF_WORDS, r, fy, fx, nR, nC);
        if (row < nR && g4 < nC) {
            uint32_t px[4];
            if (copy) {
                const unsigned char* s = run.base + (int64_t)(fy + row) * rec.pitch + (int64_t)(fx + g4) * 3;
                const bool dwords = (((uintptr_t)rec.src + (int64_t)rec.x0 * 3) & 3) == 0 && (rec.pitch & 3) == 0;
                uint32_t w[3];
                load12(s, dwords, w);
                unpack12(w, px);
            } else {
                spei_noise_record nr{};
                if constexpr (NOISE) nr = na.rec[rr];
                shake_pixels<NOISE>(lds, ntaps, r, (nC + 2 * r) | 1, row, g4, len, sr, nr, na, (uint32_t)(fx + g4), (uint32_t)(fy + row), px);
            }
            uint32_t* d = out + row * PITCH + g4;
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = px[k];
        }
        __syncthreads();
    }
    store_tile(out, g, rr, n_in, input, gt, P, scale);
}

// The host copies of the PSF tables and of n shake records, checked before a launch; 0 if valid, else -1 with the text in
// spei_last_error.  *shaken: does any record have a radius above 0?
int shake_check(const char* name, const uint32_t* psfs, const uint32_t* psfs_host, int n_psf, const spei_shake_record* shake,
                const spei_shake_record* shake_host, int n, bool* shaken) {
    SPEI_REQUIRE(shake && shake_host, "%s: null shake records (the device records and their host copy are both required)", name);
    SPEI_REQUIRE(n_psf >= 0 && (n_psf == 0 || (psfs && psfs_host)),
                 "%s: %d PSF tables with a null pointer (the device tables and their host copy are both required)", name, n_psf);
    *shaken = false;
    for (int i = 0; i < n; ++i) {
        const spei_shake_record& c = shake_host[i];
        SPEI_REQUIRE(c.reserved == 0u, "%s: shake record %d: reserved = %u, must be 0", name, i, c.reserved);
        SPEI_REQUIRE(c.radius <= (uint32_t)MAX_R, "%s: shake record %d: radius %u exceeds %d", name, i, c.radius, MAX_R);
        if (c.radius == 0u) {
            SPEI_REQUIRE(c.q16 == 65536u, "%s: shake record %d: radius 0 (the delta) with q16 = %u, must be 65536", name, i, c.q16);
            continue;
        }
        SPEI_REQUIRE(c.psf < (uint32_t)n_psf, "%s: shake record %d: PSF %u of %d tables", name, i, c.psf, n_psf);
        const uint32_t* w = psfs_host + (int64_t)c.psf * PSF_WORDS;
        const int r = (int)c.radius;
        uint64_t sum = 0, sq = 0;
        for (int ty = 0; ty < PSF_SIDE; ++ty)
            for (int tx = 0; tx < PSF_SIDE; ++tx) {
                const uint32_t v = w[ty * PSF_SIDE + tx];
                const bool inside = ty >= MAX_R - r && ty <= MAX_R + r && tx >= MAX_R - r && tx <= MAX_R + r;
                SPEI_REQUIRE(inside || v == 0u, "%s: shake record %d: PSF %u has the weight %u at (dy %d, dx %d), outside its radius %d", name, i,
                             c.psf, v, ty - MAX_R, tx - MAX_R, r);
                SPEI_REQUIRE(v <= 65536u, "%s: shake record %d: PSF %u has the weight %u at (dy %d, dx %d), above 65536", name, i, c.psf, v,
                             ty - MAX_R, tx - MAX_R);
                sum += v;
                sq += (uint64_t)v * v;
            }
        SPEI_REQUIRE(sum == 65536u, "%s: shake record %d: the weights of PSF %u sum to %llu, not 65536", name, i, c.psf, (unsigned long long)sum);
        SPEI_REQUIRE(c.q16 == (uint32_t)(sq >> 16), "%s: shake record %d: q16 = %u, but floor(sum of w^2 / 2^16) of PSF %u is %u", name, i, c.q16,
                     c.psf, (uint32_t)(sq >> 16));
        *shaken = true;
    }
    return 0;
}

}  // namespace

extern "C" int spei_window_mean_shake_u8(const unsigned char* src, int64_t frame_stride, int T, const int* runs, const int* runs_host, int M,
                                         const uint32_t* tables, const uint32_t* tables_host, const int32_t* gauss, const int32_t* gauss_host,
                                         const spei_noise_record* noise, const spei_noise_record* noise_host, uint32_t key0, uint32_t key1,
                                         const uint32_t* psfs, const uint32_t* psfs_host, int n_psf, const spei_shake_record* shake,
                                         const spei_shake_record* shake_host, unsigned char* blur, unsigned char* gt, float* gray, int H, int W,
                                         spei_stream_t stream) {
    const char* name = "spei_window_mean_shake_u8";
    if (window_runs_check(name, src, frame_stride, T, runs, runs_host, M, blur, gt, H, W)) return -1;
    if (light_check(name, tables, tables_host)) return -1;
    if (gauss && noise_check(name, gauss, gauss_host, noise, noise_host, M)) return -1;
    bool shaken = false;
    if (shake_check(name, psfs, psfs_host, n_psf, shake, shake_host, M, &shaken)) return -1;
    if (!shaken)
        return gauss ? spei_window_mean_noise_u8(src, frame_stride, T, runs, runs_host, M, tables, tables_host, gauss, gauss_host, noise,
                                                 noise_host, key0, key1, blur, gt, gray, H, W, stream)
                     : spei_window_mean_light_u8(src, frame_stride, T, runs, runs_host, M, tables, tables_host, blur, gt, gray, H, W, stream);
    const int tiles_x = cdiv(W, TILE), tiles_y = cdiv(H, TILE);
    const bool wide = (W & 3) == 0 && (((uintptr_t)src | (uintptr_t)blur | (uintptr_t)gt) & 3) == 0 && (T == 1 || (frame_stride & 3) == 0);
    const NoiseArgs na{gauss, noise, key0, key1};
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)M);
    const size_t lds = LDS_TOTAL * sizeof(uint32_t);
    if (gauss) {
        ensure_dyn_lds<window_mean_shake_kernel<true>>(lds);
        hipLaunchKernelGGL(window_mean_shake_kernel<true>, grid, dim3(256), lds, (hipStream_t)stream, src, frame_stride, runs, tables, psfs, shake,
                           blur, gt, gray, H, W, tiles_x, na, wide);
    } else {
        ensure_dyn_lds<window_mean_shake_kernel<false>>(lds);
        hipLaunchKernelGGL(window_mean_shake_kernel<false>, grid, dim3(256), lds, (hipStream_t)stream, src, frame_stride, runs, tables, psfs, shake,
                           blur, gt, gray, H, W, tiles_x, na, wide);
    }
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int spei_train_batch_runs_shake_u8(const spei_run_record* table, const spei_run_record* table_host, int n_in, int n_gt,
                                              const uint32_t* tables, const uint32_t* tables_host, const int32_t* gauss,
                                              const int32_t* gauss_host, const spei_noise_record* noise, const spei_noise_record* noise_host,
                                              uint32_t key0, uint32_t key1, const uint32_t* psfs, const uint32_t* psfs_host, int n_psf,
                                              const spei_shake_record* shake, const spei_shake_record* shake_host, float* input, float* gt, int P,
                                              float rgb_range, spei_stream_t stream) {
    const char* name = "spei_train_batch_runs_shake_u8";
    if (batch_table_check(name, table, table_host, n_in, n_gt, input, gt, P, rgb_range)) return -1;
    if (light_check(name, tables, tables_host)) return -1;
    if (gauss && noise_check(name, gauss, gauss_host, noise, noise_host, n_in + n_gt)) return -1;
    bool shaken = false;
    if (shake_check(name, psfs, psfs_host, n_psf, shake, shake_host, n_in + n_gt, &shaken)) return -1;
    if (!shaken)
        return gauss ? spei_train_batch_runs_noise_u8(table, table_host, n_in, n_gt, tables, tables_host, gauss, gauss_host, noise, noise_host, key0,
                                                      key1, input, gt, P, rgb_range, stream)
                     : spei_train_batch_runs_light_u8(table, table_host, n_in, n_gt, tables, tables_host, input, gt, P, rgb_range, stream);
    const int tiles = cdiv(P, TILE);
    const float scale = (float)((double)rgb_range / 255.0);
    const NoiseArgs na{gauss, noise, key0, key1};
    const dim3 grid((unsigned)(tiles * tiles), (unsigned)(n_in + n_gt));
    const size_t lds = LDS_TOTAL * sizeof(uint32_t);
    if (gauss) {
        ensure_dyn_lds<train_batch_shake_kernel<true>>(lds);
        hipLaunchKernelGGL(train_batch_shake_kernel<true>, grid, dim3(256), lds, (hipStream_t)stream, table, tables, psfs, shake, n_in, input, gt, P,
                           tiles, scale, na);
    } else {
        ensure_dyn_lds<train_batch_shake_kernel<false>>(lds);
        hipLaunchKernelGGL(train_batch_shake_kernel<false>, grid, dim3(256), lds, (hipStream_t)stream, table, tables, psfs, shake, n_in, input, gt, P,
                           tiles, scale, na);
    }
    SPEI_CHECK_LAUNCH(name);
    return 0;
}
