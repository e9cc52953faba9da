// The training batch of the dataset loop (speinet_amd/data.py): one launch turns a table of uint8 crop rectangles into the fp32 tensors
// the trainers take — what the reference builds per sample on DataLoader workers (util/utils.py:8-65 get_patch / np2Tensor /
// data_augment, data/videodata_nfs.py:180-207 __getitem__):
//
//   input  fp32 [n_in][3][P][P]   (n_in = B * (n_seq + 2), or B * n_seq without references)
//   gt     fp32 [n_gt][3][P][P]   (n_gt = B: the middle frame's ground truth)
//
// One record per output frame: the address of a uint8 [H][W][3] frame, its row pitch in bytes, the crop origin (y0, x0) and the flags
// {hflip, vflip, rot90, zero}.  Value: (float)u * (float)(rgb_range / 255) (np2Tensor: float64 -> float32, then mul_ by a Python
// scalar in float32), bit-identical to the reference's tensors.  Geometry in the reference's order — crop, [:, ::-1] if hflip,
// [::-1, :] if vflip, np.rot90 (counter-clockwise) if rot90 — which for output pixel (i, j) of the P x P patch reads crop pixel
//     no rot90:  ( vflip ? P-1-i : i ,  hflip ? P-1-j : j )
//     rot90:     ( vflip ? P-1-j : j ,  hflip ? i : P-1-i )
// so a 32 x 32 output tile always reads one 32 x 32 source tile, transposed and / or mirrored.  A workgroup stages that tile through
// LDS: thread t reads 4 pixels (12 bytes: three dwords where the row addresses are 4-byte aligned, bytes otherwise) of source row
// t / 8, so a wave reads 8 source rows of 96 contiguous bytes each; then thread t writes 4 pixels of output row t / 8 as one 16-byte
// store per plane, whatever the flags.  LDS pitch 33 dwords (one packed pixel per dword): a 32-lane half of a ds_write_b32 /
// ds_read_b32 holds 4 rows x 8 groups and touches bank (row + 4 * group + k) % 32 in either orientation — all distinct.
// `zero` records write zeros and read nothing.  Plain vector stores only.
//
// spei_train_batch_runs_u8 (data.SharpTrainLoader: training from sharp footage, the blur synthesised per batch) is the same kernel on
// spei_run_record: the record's frame is the per-byte integer mean of a run of 1..15 consecutive frames, u = floor(sum / length) —
// the bytes of spei_window_mean_u8's blur[m] (csrc/blurset.hip) — formed in the load phase: thread t sums its 12 bytes over the run's
// frames in registers (two bytes per dword, 16 bits each: a sum is at most 15 * 255 = 3825), up to four frames' loads in flight
// before the first add, divides (blurset.hip's multiply and shift) and packs the four pixels into LDS as above.  Everything after
// the barrier is shared.  A ground-truth record is a run of length 1 at the run's middle frame.
//
// spei_train_batch_runs_light_u8 is that kernel with the run averaged in LINEAR light (csrc/light.h) — the bytes of
// spei_window_mean_light_u8's blur[m]: the workgroup stages lin[] and thr[] in LDS, thread t decodes its 12 bytes of every frame (one
// LDS read each) into twelve 32-bit sums — the packed two-sums-per-dword trick does not carry over: a sum reaches 15 (2^24 - 1) —
// divides (light.h's multiply-high), encodes by the binary search over thr[] and packs the four pixels into LDS as above.  A record
// of length 1 (every ground-truth record) is loaded as is.  Everything after the barrier is shared.
//
// spei_train_batch_runs_noise_u8 adds sensor noise between the quotient and the encode (csrc/light.h) — the bytes of
// spei_window_mean_noise_u8's blur[m]: the workgroup also stages the gauss table, and thread t makes one Philox call for each of its
// four pixels on the counter (x, y, run, clip) with (x, y) = (x0 + cx_lo + g4 + k, y0 + cy_lo + row), the pixel in its full frame.
#include "common.h"
#include "light.h"
#include "run_checks.h"
#include "train_tile.h"

namespace {

constexpr int RUN_LOADS = 4;                                             // RUN_LOADS frames' loads are issued before their adds

// 12 bytes of a run of len frames fstride apart averaged in linear light (csrc/light.h), packed as load12 packs them; tab = lin[256],
// thr[256] in LDS, staged iff len > 1.  NOISE: with the noise of record nr under the key of na added to the quotient; gauss = the table
// in LDS (staged iff len > 1), (x, y) = the first of the four pixels in its frame
template <bool NOISE>
__device__ __forceinline__ void run_light12(const unsigned char* s, int64_t fstride, int len, bool dwords, const uint32_t* tab, uint32_t w[3],
                                            const int32_t* gauss, const spei_noise_record& nr, const NoiseArgs& na, uint32_t x, uint32_t y) {
    if (len == 1) {                                                      // encode(lin[c]) == c
        load12(s, dwords, w);
        return;
    }
    uint32_t sum[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) sum[j] = 0u;
    for (int t0 = 0; t0 < len; t0 += RUN_LOADS) {
        uint32_t q[RUN_LOADS][3];
#pragma unroll
        for (int u = 0; u < RUN_LOADS; ++u)
            if (t0 + u < len) load12(s + (int64_t)(t0 + u) * fstride, dwords, q[u]);
#pragma unroll
        for (int u = 0; u < RUN_LOADS; ++u)
            if (t0 + u < len) {
#pragma unroll
                for (int j = 0; j < 12; ++j) sum[j] += tab[(q[u][j >> 2] >> (8 * (j & 3))) & 0xffu];
            }
    }
    const uint32_t magic = light_magic(len);
    w[0] = w[1] = w[2] = 0u;
    if constexpr (NOISE) {
        const uint64_t nmagic = noise_magic(len);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t rnd[3];
            philox3(x + k, y, nr.run, nr.clip, na.key0, na.key1, rnd);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int j = 3 * k + c;
                const uint32_t L = noise_apply(light_quot(sum[j], magic), gauss_z(gauss, rnd[c]), nr.A, nr.B, nmagic);
                w[j >> 2] |= light_encode(tab + 256, L) << (8 * (j & 3));
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) w[j >> 2] |= light_encode(tab + 256, light_quot(sum[j], magic)) << (8 * (j & 3));
    }
}

template <typename Rec, bool LIGHT, bool NOISE>
__global__ __launch_bounds__(256) void train_batch_kernel(const Rec* __restrict__ table, const uint32_t* __restrict__ tables, int n_in,
                                                          float* __restrict__ input, float* __restrict__ gt, int P, int tiles, float scale,
                                                          NoiseArgs na) {
    constexpr bool RUNS = std::is_same<Rec, spei_run_record>::value;
    static_assert(RUNS || !LIGHT, "a light averages runs");
    static_assert(LIGHT || !NOISE, "noise is added in a linear light");
    __shared__ uint32_t lds[TILE * PITCH];
    const int r = blockIdx.y;
    const Rec rec = table[r];
    const TileGeom g = tile_geom(rec.flags, P, tiles);
    const int row = threadIdx.x >> 3, g4 = (threadIdx.x & 7) * 4;
    const int nR = g.nR, nC = g.nC, cy_lo = g.cy_lo, cx_lo = g.cx_lo;
    if (!g.zero) {
        const uint32_t* tab = nullptr;                                   // LIGHT: lin[256], thr[256] in LDS, for a run of 2 or more frames
        if constexpr (LIGHT) {
            __shared__ uint32_t light[LIGHT_WORDS];
            if (rec.length > 1) light_stage(light, tables);
            tab = light;
        }
        const int32_t* gauss = nullptr;                                  // NOISE: the gauss table in LDS, for a run of 2 or more frames
        spei_noise_record nr{};
        if constexpr (NOISE) {
            __shared__ int32_t glds[GAUSS_WORDS];
            if (rec.length > 1) gauss_stage(glds, na.gauss);
            gauss = glds;
            nr = na.rec[r];
        }
        if (row < nR && g4 < nC) {
            const unsigned char* s = reinterpret_cast<const unsigned char*>(rec.src) + (int64_t)(rec.y0 + cy_lo + row) * rec.pitch +
                                     (int64_t)(rec.x0 + cx_lo + g4) * 3;
            bool dwords = (((uintptr_t)rec.src + (int64_t)rec.x0 * 3) & 3) == 0 && (rec.pitch & 3) == 0;      // every row of the crop starts on a dword
            uint32_t w[3];
            if constexpr (RUNS) {
                const int len = rec.length;
                dwords = dwords && (len == 1 || (rec.frame_stride & 3) == 0);                                  // ... in every frame of the run
                if constexpr (LIGHT) {
                    run_light12<NOISE>(s, rec.frame_stride, len, dwords, tab, w, gauss, nr, na, (uint32_t)(rec.x0 + cx_lo + g4),
                                       (uint32_t)(rec.y0 + cy_lo + row));
                } else {
                    // even[k] holds the sums of bytes 0 and 2 of dword k in its two halves, odd[k] those of bytes 1 and 3
                    uint32_t even[3] = {0u, 0u, 0u}, odd[3] = {0u, 0u, 0u};
                    for (int t0 = 0; t0 < len; t0 += RUN_LOADS) {
                        uint32_t q[RUN_LOADS][3];
#pragma unroll
                        for (int u = 0; u < RUN_LOADS; ++u) {
                            q[u][0] = q[u][1] = q[u][2] = 0u;
                            if (t0 + u < len) load12(s + (int64_t)(t0 + u) * rec.frame_stride, dwords, q[u]);
                        }
#pragma unroll
                        for (int u = 0; u < RUN_LOADS; ++u)
#pragma unroll
                            for (int k = 0; k < 3; ++k) {
                                even[k] += q[u][k] & 0x00ff00ffu;
                                odd[k] += (q[u][k] >> 8) & 0x00ff00ffu;
                            }
                    }
                    // (sum * m) >> 16 == sum / len with m = ceil(2^16 / len), for every sum <= 15 * 255 and len <= 15 (csrc/blurset.hip)
                    const uint32_t magic = (65536u + len - 1) / len;
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        w[k] = (((even[k] & 0xffffu) * magic) >> 16) | ((((odd[k] & 0xffffu) * magic) >> 16) << 8) |
                               ((((even[k] >> 16) * magic) >> 16) << 16) | ((((odd[k] >> 16) * magic) >> 16) << 24);
                }
            } else {
                load12(s, dwords, w);
            }
            unpack12(w, lds + row * PITCH + g4);
        }
        __syncthreads();
    }
    store_tile(lds, g, r, n_in, input, gt, P, scale);
}

// Every record is checked on the host copy (run_checks.h): the kernel never meets a record that leaves its frame or its clip
template <typename Rec, bool LIGHT = false, bool NOISE = false>
int train_batch(const char* name, const Rec* table, const Rec* table_host, int n_in, int n_gt, float* input, float* gt, int P, float rgb_range,
                spei_stream_t stream, const uint32_t* tables = nullptr, const uint32_t* tables_host = nullptr, const int32_t* gauss = nullptr,
                const int32_t* gauss_host = nullptr, const spei_noise_record* noise = nullptr, const spei_noise_record* noise_host = nullptr,
                uint32_t key0 = 0u, uint32_t key1 = 0u) {
    if (batch_table_check(name, table, table_host, n_in, n_gt, input, gt, P, rgb_range)) return -1;
    if constexpr (LIGHT)
        if (light_check(name, tables, tables_host)) return -1;
    if constexpr (NOISE)
        if (noise_check(name, gauss, gauss_host, noise, noise_host, n_in + n_gt)) return -1;
    const int tiles = cdiv(P, TILE);
    const float scale = (float)((double)rgb_range / 255.0);
    hipLaunchKernelGGL((train_batch_kernel<Rec, LIGHT, NOISE>), dim3(tiles * tiles, n_in + n_gt), dim3(256), 0, (hipStream_t)stream, table, tables,
                       n_in, input, gt, P, tiles, scale, NoiseArgs{gauss, noise, key0, key1});
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

}  // namespace

extern "C" int spei_train_batch_u8(const spei_crop_record* table, const spei_crop_record* table_host, int n_in, int n_gt, float* input,
                                   float* gt, int P, float rgb_range, spei_stream_t stream) {
    return train_batch("spei_train_batch_u8", table, table_host, n_in, n_gt, input, gt, P, rgb_range, stream);
}

extern "C" int spei_train_batch_runs_u8(const spei_run_record* table, const spei_run_record* table_host, int n_in, int n_gt, float* input,
                                        float* gt, int P, float rgb_range, spei_stream_t stream) {
    return train_batch("spei_train_batch_runs_u8", table, table_host, n_in, n_gt, input, gt, P, rgb_range, stream);
}

extern "C" int spei_train_batch_runs_light_u8(const spei_run_record* table, const spei_run_record* table_host, int n_in, int n_gt,
                                              const uint32_t* tables, const uint32_t* tables_host, float* input, float* gt, int P,
                                              float rgb_range, spei_stream_t stream) {
    return train_batch<spei_run_record, true>("spei_train_batch_runs_light_u8", table, table_host, n_in, n_gt, input, gt, P, rgb_range, stream,
                                              tables, tables_host);
}

extern "C" int spei_train_batch_runs_noise_u8(const spei_run_record* table, const spei_run_record* table_host, int n_in, int n_gt,
                                              const uint32_t* tables, const uint32_t* tables_host, const int32_t* gauss,
                                              const int32_t* gauss_host, const spei_noise_record* noise, const spei_noise_record* noise_host,
                                              uint32_t key0, uint32_t key1, float* input, float* gt, int P, float rgb_range,
                                              spei_stream_t stream) {
    return train_batch<spei_run_record, true, true>("spei_train_batch_runs_noise_u8", table, table_host, n_in, n_gt, input, gt, P, rgb_range,
                                                    stream, tables, tables_host, gauss, gauss_host, noise, noise_host, key0, key1);
}
