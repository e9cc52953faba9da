// Codec artefacts in blur synthesis (include/speinet_hip.h, "codec artefacts in blur synthesis"; speinet_amd/codec.py is the definition):
// a JPEG-style round trip of the synthesis's input frames, in int32, defined bit for bit.
//
//   spei_codec_u8              — in place on N packed uint8 [H][W][3] frames, and their gray planes
//   spei_train_batch_codec_f32 — in place on the fp32 [n_in][3][P][P] input tensor a spei_train_batch_runs_* entry wrote
//
// MCUs are 16 x 16 pixels on a grid with one corner at (-oy, -ox); a sample outside the frame or rectangle is the nearest one inside.
// Colour is BT.601 full range with yuv_io.hip's Q14 constants: Y per pixel, Cb / Cr on the 2 x 2 channel sums (the CENTER rule); on
// the way back chroma is replicated (U16 = 16 Cb[y >> 1][x >> 1]) and yuv_io.hip's inverse applies.  Per 8 x 8 block of s = value - 128,
// with D[u][x] = rint(8192 a(u) cos((2x + 1) u pi / 16)):
//     T[y][u] = (sum_x D[u][x] s[y][x] + 2^9) >> 10        F[v][u] = (sum_y D[v][y] T[y][u] + 2^12) >> 13      (Q3)
//     q = sign(F) ((|F| + 4 Q) / (8 Q))                    G = q Q
//     U[y][u] = (sum_v D[v][y] G[v][u] + 2^9) >> 10        r[y][x] = (sum_u D[u][x] U[y][u] + 2^15) >> 16
//     sample = clip(r + 128, 0, 255)
// The sums stay below 2 965 504, 67 094 528, 24 908 791 and 526 417 325 in magnitude: int32 throughout.
//
// One workgroup of 128 threads makes one MCU of one frame or record:
//   1. thread t loads pixels t and t + 128 of the MCU (coordinates clamped), keeps them packed in LDS and writes Y - 128 into its block;
//   2. thread t makes one chroma sample (Cb for t < 64, Cr above) from the 2 x 2 packed pixels;
//   3. the four matrix passes, three coefficients per thread and pass (6 blocks x 64 = 384 = 3 x 128), 8 integer multiply-adds each,
//      between two LDS buffers with a barrier after each pass; pass 2 also quantises and dequantises.  Block rows have a pitch of 9
//      words: the 8 rows a wave reads in one instruction fall on 8 different banks, and the other lanes read the same words (broadcast);
//   4. thread t converts its two pixels back and stores those that lie inside the frame or rectangle.
// An MCU reads and writes only its own pixels and every read precedes the first barrier, so both entries work in place.  The fp32
// entry maps MCU-local SOURCE coordinates to positions of the stored plane with train_tile.h's rule (a bijection of the P x P square).
// LDS: 5.3 KB per workgroup.  Plain vector stores only.
#include "common.h"
#include "run_checks.h"

namespace {

constexpr int NT = 128, MCU = 16, BP = 9, BLK = 8 * BP, NBLK = 6;
constexpr int F_SKIP = SPEI_CODEC_SKIP;

__constant__ int DCT[64] = {2896, 2896,  2896,  2896,  2896,  2896,  2896,  2896,  4017, 3406,  2276,  799,   -799,  -2276, -3406, -4017,
                            3784, 1567,  -1567, -3784, -3784, -1567, 1567,  3784,  3406, -799,  -4017, -2276, 2276,  4017,  799,   -3406,
                            2896, -2896, -2896, 2896,  2896,  -2896, -2896, 2896,  2276, -4017, 799,   3406,  -3406, -799,  4017,  -2276,
                            1567, -3784, 3784,  -1567, -1567, 3784,  -3784, 1567,  799,  -2276, 3406,  -4017, 4017,  -3406, 2276,  -799};

// yuv_io.hip's `601 full` row
constexpr int YR = 4899, YG = 9617, YB = 1868, UR = -2765, UG = -5427, UB = 8192, VR = 8192, VG = -6860, VB = -1332;
constexpr int CY = 16384, RV = 22970, GU = -5638, GV = -11700, BU = 29032;

__device__ __forceinline__ int clip255(int v) { return min(max(v, 0), 255); }

// N packed uint8 frames and their gray planes
struct SurfU8 {
    unsigned char* frame;
    float* gray;             // the frame's plane, or null
    int W;
    __device__ __forceinline__ uint32_t load(int y, int x) const {
        const unsigned char* p = frame + ((int64_t)y * W + x) * 3;
        return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    }
    __device__ __forceinline__ void store(int y, int x, int r, int g, int b) const {
        unsigned char* p = frame + ((int64_t)y * W + x) * 3;
        p[0] = (unsigned char)r; p[1] = (unsigned char)g; p[2] = (unsigned char)b;
        if (gray) gray[(int64_t)y * W + x] = spei_gray_px((float)r, (float)g, (float)b);
    }
};

// One fp32 [3][P][P] record, stored flipped / rotated as its flags say: (y, x) are SOURCE coordinates of the crop
struct SurfF32 {
    float* plane;
    int P;
    bool hf, vf, rot;
    float s, inv;
    __device__ __forceinline__ int64_t at(int y, int x) const {
        const int a = vf ? P - 1 - y : y;
        const int i = rot ? (hf ? x : P - 1 - x) : a, j = rot ? a : (hf ? P - 1 - x : x);
        return (int64_t)i * P + j;
    }
    __device__ __forceinline__ uint32_t load(int y, int x) const {
        const float* p = plane + at(y, x);
        const int64_t pp = (int64_t)P * P;
        uint32_t px = 0u;
#pragma unroll
        for (int c = 0; c < 3; ++c) px |= (uint32_t)clip255((int)__fadd_rn(__fmul_rn(p[c * pp], inv), 0.5f)) << (8 * c);
        return px;
    }
    __device__ __forceinline__ void store(int y, int x, int r, int g, int b) const {
        float* p = plane + at(y, x);
        const int64_t pp = (int64_t)P * P;
        p[0] = __fmul_rn((float)r, s);
        p[pp] = __fmul_rn((float)g, s);
        p[2 * pp] = __fmul_rn((float)b, s);
    }
};

// The MCU (my, mx) of an H x W surface on the grid with a corner at (-oy, -ox), through the tables qt [2][64]
template <typename Surf>
__device__ __forceinline__ void mcu_round_trip(const Surf& sf, int H, int W, int my, int mx, int oy, int ox, const uint16_t* __restrict__ qt) {
    __shared__ uint32_t pxs[MCU * MCU];
    __shared__ int A[NBLK * BLK], B[NBLK * BLK], qs[128], ds[64];
    const int tid = threadIdx.x;
    const int y0 = my * MCU - oy, x0 = mx * MCU - ox;
    if (y0 >= H || x0 >= W) return;                                      // a grid sized for larger offsets than this record's
    qs[tid] = qt[tid];
    if (tid < 64) ds[tid] = DCT[tid];
#pragma unroll
    for (int p = tid; p < MCU * MCU; p += NT) {
        const int ly = p >> 4, lx = p & 15;
        const uint32_t px = sf.load(min(max(y0 + ly, 0), H - 1), min(max(x0 + lx, 0), W - 1));
        pxs[p] = px;
        const int R = px & 0xff, G = (px >> 8) & 0xff, Bl = (px >> 16) & 0xff;
        A[((ly >> 3) * 2 + (lx >> 3)) * BLK + (ly & 7) * BP + (lx & 7)] = clip255((YR * R + YG * G + YB * Bl + (1 << 13)) >> 14) - 128;
    }
    __syncthreads();
    {
        const int c = tid & 63, cy = c >> 3, cx = c & 7, cr = tid >> 6;
        const uint32_t* q = pxs + (2 * cy) * MCU + 2 * cx;
        int S[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            S[ch] = (int)((q[0] >> (8 * ch)) & 0xff) + (int)((q[1] >> (8 * ch)) & 0xff) + (int)((q[MCU] >> (8 * ch)) & 0xff) +
                    (int)((q[MCU + 1] >> (8 * ch)) & 0xff);
        const int v = cr ? VR * S[0] + VG * S[1] + VB * S[2] : UR * S[0] + UG * S[1] + UB * S[2];
        A[(4 + cr) * BLK + cy * BP + cx] = clip255(((v + (1 << 15)) >> 16) + 128) - 128;
    }
    __syncthreads();
    // forward rows: A = s[y][x] -> B = T[y][u]
#pragma unroll
    for (int i = tid; i < NBLK * 64; i += NT) {
        const int b = i >> 6, y = (i >> 3) & 7, u = i & 7;
        const int* s = A + b * BLK + y * BP;
        int acc = 1 << 9;
#pragma unroll
        for (int x = 0; x < 8; ++x) acc += ds[u * 8 + x] * s[x];
        B[b * BLK + y * BP + u] = acc >> 10;
    }
    __syncthreads();
    // forward columns, quantise, dequantise: B = T[y][u] -> A = G[v][u]
#pragma unroll
    for (int i = tid; i < NBLK * 64; i += NT) {
        const int b = i >> 6, v = (i >> 3) & 7, u = i & 7;
        const int* t = B + b * BLK + u;
        int acc = 1 << 12;
#pragma unroll
        for (int y = 0; y < 8; ++y) acc += ds[v * 8 + y] * t[y * BP];
        const int F = acc >> 13, Q = qs[(b >= 4 ? 64 : 0) + v * 8 + u];
        const int q = (int)((uint32_t)(abs(F) + 4 * Q) / (uint32_t)(8 * Q));
        A[b * BLK + v * BP + u] = (F < 0 ? -q : q) * Q;
    }
    __syncthreads();
    // inverse columns: A = G[v][u] -> B = U[y][u]
#pragma unroll
    for (int i = tid; i < NBLK * 64; i += NT) {
        const int b = i >> 6, y = (i >> 3) & 7, u = i & 7;
        const int* g = A + b * BLK + u;
        int acc = 1 << 9;
#pragma unroll
        for (int v = 0; v < 8; ++v) acc += ds[v * 8 + y] * g[v * BP];
        B[b * BLK + y * BP + u] = acc >> 10;
    }
    __syncthreads();
    // inverse rows: B = U[y][u] -> A = sample[y][x]
#pragma unroll
    for (int i = tid; i < NBLK * 64; i += NT) {
        const int b = i >> 6, y = (i >> 3) & 7, x = i & 7;
        const int* uu = B + b * BLK + y * BP;
        int acc = 1 << 15;
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += ds[u * 8 + x] * uu[u];
        A[b * BLK + y * BP + x] = clip255((acc >> 16) + 128);
    }
    __syncthreads();
#pragma unroll
    for (int p = tid; p < MCU * MCU; p += NT) {
        const int ly = p >> 4, lx = p & 15, y = y0 + ly, x = x0 + lx;
        if (y < 0 || y >= H || x < 0 || x >= W) continue;
        const int Y = A[((ly >> 3) * 2 + (lx >> 3)) * BLK + (ly & 7) * BP + (lx & 7)];
        const int co = (ly >> 1) * BP + (lx >> 1);
        const int yy = CY * 16 * Y, u = 16 * A[4 * BLK + co] - 2048, v = 16 * A[5 * BLK + co] - 2048;
        sf.store(y, x, clip255((yy + RV * v + (1 << 17)) >> 18), clip255((yy + GU * u + GV * v + (1 << 17)) >> 18),
                 clip255((yy + BU * u + (1 << 17)) >> 18));
    }
}

__global__ __launch_bounds__(NT) void codec_u8_kernel(unsigned char* __restrict__ frames, int64_t fstride, int H, int W,
                                                       const spei_codec_record* __restrict__ records, const uint16_t* __restrict__ qtabs,
                                                       float* __restrict__ gray, int mcus_x) {
    const int n = blockIdx.y;
    const spei_codec_record rec = records[n];
    if (rec.flags & F_SKIP) return;
    const SurfU8 sf{frames + (int64_t)n * fstride, gray ? gray + (int64_t)n * H * W : nullptr, W};
    mcu_round_trip(sf, H, W, (int)(blockIdx.x / mcus_x), (int)(blockIdx.x % mcus_x), (int)rec.oy, (int)rec.ox, qtabs + (int64_t)rec.qtab * 128);
}

__global__ __launch_bounds__(NT) void train_batch_codec_kernel(float* __restrict__ input, int P, float s, float inv,
                                                                const spei_codec_record* __restrict__ records,
                                                                const uint16_t* __restrict__ qtabs) {
    const int r = blockIdx.y;
    const spei_codec_record rec = records[r];
    if (rec.flags & (F_SKIP | F_ZERO)) return;
    const int oy = (int)rec.oy, ox = (int)rec.ox;
    const int mcus_x = (P + ox + MCU - 1) / MCU, mcus_y = (P + oy + MCU - 1) / MCU;
    const int my = (int)(blockIdx.x / mcus_x), mx = (int)(blockIdx.x % mcus_x);
    if (my >= mcus_y) return;                                            // the grid is sized for oy = ox = 15
    const SurfF32 sf{input + (int64_t)r * 3 * P * P, P, (rec.flags & F_HFLIP) != 0, (rec.flags & F_VFLIP) != 0, (rec.flags & F_ROT90) != 0, s, inv};
    mcu_round_trip(sf, P, P, my, mx, oy, ox, qtabs + (int64_t)rec.qtab * 128);
}

// The host copies of the n records and the n_qtab tables, checked before a launch; 0 if valid, else -1 with the text in
// spei_last_error.  `known`: the flag bits the entry takes.  *coded: is any record not SKIP / ZERO?
int codec_check(const char* name, const spei_codec_record* records, const spei_codec_record* records_host, int n, const uint16_t* qtabs,
                const uint16_t* qtabs_host, int n_qtab, uint32_t known, bool* coded) {
    SPEI_REQUIRE(records && records_host, "%s: null codec records (the device records and their host copy are both required)", name);
    SPEI_REQUIRE(n_qtab > 0 && qtabs && qtabs_host, "%s: %d quantisation tables (at least one; the device tables and their host copy are both required)",
                 name, n_qtab);
    for (int t = 0; t < n_qtab; ++t)
        for (int k = 0; k < 128; ++k) {
            const int v = qtabs_host[t * 128 + k];
            SPEI_REQUIRE(v >= 1 && v <= 255, "%s: quantisation table %d: entry %d of its %s table is %d (1..255)", name, t, k & 63,
                         k < 64 ? "luminance" : "chrominance", v);
        }
    *coded = false;
    for (int i = 0; i < n; ++i) {
        const spei_codec_record& c = records_host[i];
        SPEI_REQUIRE((c.flags & ~known) == 0u, "%s: codec record %d has unknown flag bits 0x%x", name, i, c.flags & ~known);
        SPEI_REQUIRE(c.qtab < (uint32_t)n_qtab, "%s: codec record %d: table %u of %d tables", name, i, c.qtab, n_qtab);
        SPEI_REQUIRE(c.oy < (uint32_t)MCU && c.ox < (uint32_t)MCU, "%s: codec record %d: grid offset (oy %u, ox %u), each must be below %d", name, i,
                     c.oy, c.ox, MCU);
        if (!(c.flags & (uint32_t)(F_SKIP | F_ZERO))) *coded = true;
    }
    return 0;
}

}  // namespace

extern "C" int spei_codec_u8(unsigned char* frames, int64_t frame_stride, int N, int H, int W, const spei_codec_record* records,
                             const spei_codec_record* records_host, const uint16_t* qtabs, const uint16_t* qtabs_host, int n_qtab, float* gray,
                             spei_stream_t stream) {
    const char* name = "spei_codec_u8";
    SPEI_REQUIRE(frames, "%s: null frames", name);
    SPEI_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && (int64_t)H * W * 3 < (1ll << 31), "%s: bad sizes (%d frames of %dx%d; at most 65535 per launch)",
                 name, N, W, H);
    SPEI_REQUIRE(N == 1 || frame_stride >= (int64_t)H * W * 3, "%s: frame stride %lld < one %dx%d frame", name, (long long)frame_stride, W, H);
    bool coded = false;
    if (codec_check(name, records, records_host, N, qtabs, qtabs_host, n_qtab, (uint32_t)F_SKIP, &coded)) return -1;
    if (!coded) return 0;
    // one grid for all frames: sized for the largest offsets on record, smaller ones leave their last MCUs empty (y0 >= H: nothing stored)
    uint32_t oy = 0, ox = 0;
    for (int i = 0; i < N; ++i)
        if (!(records_host[i].flags & (uint32_t)F_SKIP)) { oy = max(oy, records_host[i].oy); ox = max(ox, records_host[i].ox); }
    const int mcus_x = cdiv(W + (int)ox, MCU), mcus_y = cdiv(H + (int)oy, MCU);
    SPEI_REQUIRE((int64_t)mcus_x * mcus_y < (1ll << 31), "%s: %dx%d frame has too many MCUs", name, W, H);
    hipLaunchKernelGGL(codec_u8_kernel, dim3((unsigned)(mcus_x * mcus_y), (unsigned)N), dim3(NT), 0, (hipStream_t)stream, frames, frame_stride, H, W,
                       records, qtabs, gray, mcus_x);
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int spei_train_batch_codec_f32(float* input, int n_in, int P, float rgb_range, const spei_codec_record* records,
                                          const spei_codec_record* records_host, const uint16_t* qtabs, const uint16_t* qtabs_host, int n_qtab,
                                          spei_stream_t stream) {
    const char* name = "spei_train_batch_codec_f32";
    SPEI_REQUIRE(input, "%s: null input", name);
    SPEI_REQUIRE(n_in > 0 && n_in <= 65535, "%s: bad record count %d (1..65535)", name, n_in);
    SPEI_REQUIRE(P > 0 && P <= 4096, "%s: patch size %d must lie in 1..4096", name, P);
    SPEI_REQUIRE(rgb_range > 0.0f, "%s: rgb_range %g must be positive", name, (double)rgb_range);
    const float s = (float)((double)rgb_range / 255.0), inv = (float)(255.0 / (double)rgb_range);
    for (int u = 0; u < 256; ++u) {
        volatile float v = (float)u * s;
        volatile float t = v * inv;
        const float w = t + 0.5f;
        SPEI_REQUIRE(w >= 0.0f && w < 256.0f && (int)w == u,
                     "%s: rgb_range %g: the byte of the value (float)%d * (float)(rgb_range / 255) is not %d by (int)(v * (float)(255 / rgb_range) + 0.5f)",
                     name, (double)rgb_range, u, u);
    }
    bool coded = false;
    if (codec_check(name, records, records_host, n_in, qtabs, qtabs_host, n_qtab, (uint32_t)(F_HFLIP | F_VFLIP | F_ROT90 | F_ZERO | F_SKIP), &coded))
        return -1;
    if (!coded) return 0;
    const int mcus = cdiv(P + MCU - 1, MCU);
    hipLaunchKernelGGL(train_batch_codec_kernel, dim3((unsigned)(mcus * mcus), (unsigned)n_in), dim3(NT), 0, (hipStream_t)stream, input, P, s, inv,
                       records, qtabs);
    SPEI_CHECK_LAUNCH(name);
    return 0;
}
