// Plane I/O of the clip API's geometric self-ensemble (speinet_amd/ensemble.py, video.deblur_clip(..., ensemble=)): the network runs on
// the flips and transpositions of the padded window input, every output is transformed back and the members are averaged: the
// reference's forward_x8 (util/network_utils.py:308-341), which does this on the host and is never called.  The definition of
// member `op` (bit 0 reverses the columns, bit 1 the rows, bit 2 then transposes) and of the mean is in include/speinet_hip.h.
//
//   spei_planes_d4 — n_planes fp32 planes [H][W] -> T_op of each ([W][H] for op & 4), values copied as bits.  One launch.
//   spei_d4_mean   — K members, each T_op of a packed [C][H][W] (so [C][W][H] for op & 4) -> the float32 mean of their inverse
//                    transforms, summed in table order from the first member, times 2^-log2 K.  One launch.
//
// Both work on 32x32 tiles with one thread per group of 4 floats of a row: 8 lanes cover a tile row (128 bytes), a wave 8 rows.  Where
// H, W and the strides are multiples of 4 and the bases 16-byte aligned (every clip: the padded sizes are multiples of 20) a group is
// one 16-byte access on both sides and a tile's edge falls between groups; otherwise the same code goes element by element with a
// bound per element.  A transposing op stages the tile through LDS, the idiom of train_batch.hip: rows are written as they were
// loaded, columns are read, at a pitch of 33 dwords.  A 32-lane half of a wave holds 4 rows x 8 groups; its ds_write_b32 number k
// touches bank (row + 4 * group + k) % 32 and its ds_read_b32 number k bank (4 * group + k + row) % 32 (with either sign where a
// flip reverses an axis of the tile): 32 distinct banks in both directions under the 32-bank rule that every ds_write and the b32 /
// read2 reads follow.  No wider LDS read is used: at an odd pitch a column is not contiguous and a row not 8-byte aligned.
// The op < 4 members are mirrored copies without LDS: a reversed row is the 16-byte access at the mirrored place, its four dwords
// swapped in registers.  No scratch, no atomics.
#include "common.h"

namespace {

constexpr int TILE = 32, PITCH = 33, SUB = TILE * PITCH;   // one LDS tile in dwords
constexpr int K_MAX = 8;

__device__ __forceinline__ int flip(int p, int n, int on) { return on ? n - 1 - p : p; }
__device__ __forceinline__ int clamp4(int n) { return n < 0 ? 0 : (n > 4 ? 4 : n); }
__device__ __forceinline__ u32x4 rev4(u32x4 v) { return u32x4{v[3], v[2], v[1], v[0]}; }

// dwords base[off .. off + n) of a group of 4; the rest unspecified.  VEC (n = 0 or 4): one 16-byte access, issued by every lane without a
// branch, from base itself where n = 0 (a plane's first group: always there, never used)
template <bool VEC>
__device__ __forceinline__ u32x4 load4(const uint32_t* base, int64_t off, int n) {
    if constexpr (VEC) return *reinterpret_cast<const u32x4*>(base + (n ? off : 0));
    u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (q < n) v[q] = base[off + q];
    return v;
}

template <bool VEC>
__device__ __forceinline__ void store4(uint32_t* p, u32x4 v, int n) {
    if constexpr (VEC) {
        if (n > 0) *reinterpret_cast<u32x4*>(p) = v;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < n) p[q] = v[q];
    }
}

// row[fx ? W - 1 - (x + q) : x + q] = v[q] for q < n
template <bool VEC>
__device__ __forceinline__ void store4_flip(uint32_t* row, int x, int W, u32x4 v, int n, int fx) {
    if (!fx) return store4<VEC>(row + x, v, n);
    if constexpr (VEC) return store4<true>(row + (W - 4 - x), rev4(v), n);
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (q < n) row[W - 1 - x - q] = v[q];
}

// op < 4: a workgroup copies a 64x64 block of one plane, 16 lanes per row (256 bytes), four rows of loads in flight per thread
template <bool VEC>
__global__ __launch_bounds__(256) void planes_flip_kernel(const uint32_t* __restrict__ src, int64_t sstride, uint32_t* __restrict__ dst,
                                                          int64_t dstride, int H, int W, int op) {
    const int bx = blockIdx.x, by = blockIdx.y;
    const int64_t p = blockIdx.z;
    const int fx = op & 1, fy = (op >> 1) & 1;
    const int x = bx * 64 + 4 * (threadIdx.x & 15), y0 = by * 64 + (threadIdx.x >> 4);
    const uint32_t* s = src + p * sstride;
    uint32_t* d = dst + p * dstride;
    const int nx = clamp4(W - x);
    u32x4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int y = y0 + 16 * i, n = y < H ? nx : 0;
        v[i] = load4<VEC>(s, (int64_t)y * W + x, n);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int y = y0 + 16 * i, n = y < H ? nx : 0;
        store4_flip<VEC>(d + (int64_t)(n ? flip(y, H, fy) : 0) * W, x, W, v[i], n, fx);
    }
}

// op >= 4: a workgroup transposes a 64x64 block of one plane as four 32x32 tiles, each through an LDS tile of its own, all four loads
// of a thread in flight before the one barrier.  Tile rows [Y0, Y0 + ny) x columns [X0, X0 + nx) of the source become rows
// [I0, I0 + nx) x columns [J0, J0 + ny) of the [W][H] destination: dst[i][j] = src[fy(j)][fx(i)]
template <bool VEC>
__global__ __launch_bounds__(256) void planes_tr_kernel(const uint32_t* __restrict__ src, int64_t sstride, uint32_t* __restrict__ dst,
                                                        int64_t dstride, int H, int W, int op) {
    __shared__ uint32_t lds[4 * SUB];
    const int bx = blockIdx.x, by = blockIdx.y;
    const int64_t p = blockIdx.z;
    const int fx = op & 1, fy = (op >> 1) & 1;
    const int row = threadIdx.x >> 3, g4 = 4 * (threadIdx.x & 7);
    const uint32_t* s = src + p * sstride;
    uint32_t* d = dst + p * dstride;
    u32x4 v[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int Y0 = by * 64 + (t >> 1) * TILE, X0 = bx * 64 + (t & 1) * TILE;
        const int ny = min(TILE, H - Y0), nx = min(TILE, W - X0);
        const int n = row < ny ? clamp4(nx - g4) : 0;
        v[t] = load4<VEC>(s, (int64_t)(Y0 + row) * W + X0 + g4, n);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) lds[t * SUB + row * PITCH + g4 + q] = v[t][q];
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int Y0 = by * 64 + (t >> 1) * TILE, X0 = bx * 64 + (t & 1) * TILE;
        const int ny = min(TILE, H - Y0), nx = min(TILE, W - X0);
        const int n = row < nx ? clamp4(ny - g4) : 0;      // destination row I0 + row, columns J0 + g4 ..
        const int lc = fx ? nx - 1 - row : row;            // the source column of that row, in the tile
        u32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = lds[t * SUB + (q < n ? (fy ? ny - 1 - (g4 + q) : g4 + q) * PITCH + lc : 0)];
        const int I0 = fx ? W - X0 - nx : X0, J0 = fy ? H - Y0 - ny : Y0;
        store4<VEC>(d + (int64_t)(n ? I0 + row : 0) * H + (n ? J0 + g4 : 0), o, n);
    }
}

struct MeanTab {
    const uint32_t* m[K_MAX];
    int op[K_MAX];
    int slot[K_MAX];                                       // the LDS tile of a transposed member
};

// A workgroup owns one 32x32 tile of one canonical plane.  Member k holds T_op of the result's terms: canon[y][x] is
// m[fy(y)][fx(x)] of an upright member (rows of W) and m[fx(x)][fy(y)] of a transposed one (rows of H), whose tile is loaded by ITS rows
// and turned in LDS.  Every global load of the tile is issued before the first add; the adds run in table order from member 0.
template <int K, bool VEC>
__global__ __launch_bounds__(256) void d4_mean_kernel(MeanTab tab, uint32_t* __restrict__ dst, int H, int W, int n_tr, float scale) {
    extern __shared__ uint32_t lds[];
    const int bx = blockIdx.x, by = blockIdx.y;
    const int64_t plane = (int64_t)blockIdx.z * H * W;
    const int row = threadIdx.x >> 3, g4 = 4 * (threadIdx.x & 7);
    const int Y0 = by * TILE, X0 = bx * TILE;
    const int ny = min(TILE, H - Y0), nx = min(TILE, W - X0);
    const int y = Y0 + row, x = X0 + g4;
    const int n = row < ny ? clamp4(nx - g4) : 0;          // the thread's canonical pixels (y, x .. x + n)
    u32x4 v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int op = tab.op[k], fx = op & 1, fy = (op >> 1) & 1;
        const uint32_t* m = tab.m[k] + plane;
        const bool tr = op & 4;                            // wave-uniform, as fx and fy are: selects, no branches where VEC
        // a transposed member's tile: rows [I0, I0 + nx) x columns [J0, J0 + ny), its row I0 + row to this thread
        const int I0 = fx ? W - X0 - nx : X0, J0 = fy ? H - Y0 - ny : Y0;
        const int nm = row < nx ? clamp4(ny - g4) : 0;
        const int64_t up = (int64_t)flip(y, H, fy) * W;    // an upright member's row of canonical row y
        if constexpr (VEC) {
            const u32x4 t = load4<true>(m, tr ? (int64_t)(I0 + row) * H + J0 + g4 : up + (fx ? W - 4 - x : x), tr ? nm : n);
            v[k] = !tr && fx ? rev4(t) : t;
        } else if (tr) {
            v[k] = load4<false>(m, (int64_t)(I0 + row) * H + J0 + g4, nm);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[k][q] = q < n ? m[up + flip(x + q, W, fx)] : 0u;
        }
    }
    if (n_tr) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (tab.op[k] & 4)
#pragma unroll
                for (int q = 0; q < 4; ++q) lds[tab.slot[k] * SUB + row * PITCH + g4 + q] = v[k][q];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int op = tab.op[k], fx = op & 1, fy = (op >> 1) & 1;
            if (op & 4) {
                const int lj = fy ? ny - 1 - row : row;    // the member's column of canonical row y, in the tile
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    v[k][q] = lds[tab.slot[k] * SUB + (q < n ? (fx ? nx - 1 - (g4 + q) : g4 + q) * PITCH + lj : 0)];
            }
        }
    }
    u32x4 r = v[0];                                        // K = 1: the inverse transform, bits kept
    if constexpr (K > 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float a = __uint_as_float(v[0][q]);
#pragma unroll
            for (int k = 1; k < K; ++k) a = a + __uint_as_float(v[k][q]);
            r[q] = __float_as_uint(a * scale);
        }
    }
    store4<VEC>(dst + plane + (int64_t)(n ? y : 0) * W + x, r, n);
}

inline bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {            // [a, a + na) and [b, b + nb) in floats
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb * 4 && b0 < a0 + (uintptr_t)na * 4;
}

template <int K>
void launch_mean(bool vec, const MeanTab& tab, uint32_t* dst, int H, int W, dim3 grid, int n_tr, hipStream_t stream) {
    const float scale = 1.0f / (float)K;                   // 2^-log2 K: exact
    const size_t lds = (size_t)n_tr * SUB * sizeof(uint32_t);
    if (vec)
        hipLaunchKernelGGL((d4_mean_kernel<K, true>), grid, dim3(256), lds, stream, tab, dst, H, W, n_tr, scale);
    else
        hipLaunchKernelGGL((d4_mean_kernel<K, false>), grid, dim3(256), lds, stream, tab, dst, H, W, n_tr, scale);
}

}  // namespace

extern "C" int spei_planes_d4(const float* src, int64_t src_stride, float* dst, int64_t dst_stride, int64_t n_planes, int H, int W, int op,
                              spei_stream_t stream) {
    const char* name = "spei_planes_d4";
    SPEI_REQUIRE(src && dst, "%s: null pointer", name);
    SPEI_REQUIRE(op >= 0 && op <= 7, "%s: op %d is outside 0..7", name, op);
    SPEI_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W < (1ll << 30), "%s: bad plane shape %dx%d", name, H, W);
    SPEI_REQUIRE(n_planes >= 1, "%s: %lld planes", name, (long long)n_planes);
    const int64_t hw = (int64_t)H * W;
    SPEI_REQUIRE(src_stride >= hw && dst_stride >= hw, "%s: a stride of %lld / %lld floats is smaller than a plane of %dx%d", name,
                 (long long)src_stride, (long long)dst_stride, H, W);
    SPEI_REQUIRE(((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 3) == 0, "%s: src and dst must be 4-byte aligned", name);
    SPEI_REQUIRE(!overlap(src, (n_planes - 1) * src_stride + hw, dst, (n_planes - 1) * dst_stride + hw), "%s: src and dst overlap", name);
    SPEI_REQUIRE(n_planes <= 65535 && cdiv(H, 64) <= 65535, "%s: %lld planes of %dx%d are more than one launch covers", name,
                 (long long)n_planes, H, W);
    const bool vec = (H & 3) == 0 && (W & 3) == 0 && (src_stride & 3) == 0 && (dst_stride & 3) == 0 &&
                     (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(cdiv(W, 64), cdiv(H, 64), (unsigned)n_planes), block(256);
    if (op & 4) {
        if (vec) hipLaunchKernelGGL(planes_tr_kernel<true>, grid, block, 0, st, s, src_stride, d, dst_stride, H, W, op);
        else hipLaunchKernelGGL(planes_tr_kernel<false>, grid, block, 0, st, s, src_stride, d, dst_stride, H, W, op);
    } else {
        if (vec) hipLaunchKernelGGL(planes_flip_kernel<true>, grid, block, 0, st, s, src_stride, d, dst_stride, H, W, op);
        else hipLaunchKernelGGL(planes_flip_kernel<false>, grid, block, 0, st, s, src_stride, d, dst_stride, H, W, op);
    }
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int spei_d4_mean(const float* const* members_host, const int* ops_host, int K, float* dst, int C, int H, int W,
                            spei_stream_t stream) {
    const char* name = "spei_d4_mean";
    SPEI_REQUIRE(members_host && ops_host && dst, "%s: null pointer", name);
    SPEI_REQUIRE(K == 1 || K == 2 || K == 4 || K == 8, "%s: %d members (1, 2, 4 or 8)", name, K);
    SPEI_REQUIRE(C >= 1 && H >= 1 && W >= 1 && (int64_t)H * W < (1ll << 30), "%s: bad shape %dx%dx%d", name, C, H, W);
    SPEI_REQUIRE(((uintptr_t)dst & 3) == 0, "%s: dst must be 4-byte aligned", name);
    const int64_t total = (int64_t)C * H * W;
    MeanTab tab = {};
    int n_tr = 0;
    bool vec = (H & 3) == 0 && (W & 3) == 0 && ((uintptr_t)dst & 15) == 0;
    for (int k = 0; k < K; ++k) {
        SPEI_REQUIRE(ops_host[k] >= 0 && ops_host[k] <= 7, "%s: member %d has op %d, outside 0..7", name, k, ops_host[k]);
        SPEI_REQUIRE(members_host[k] && ((uintptr_t)members_host[k] & 3) == 0, "%s: member %d is a null or misaligned pointer", name, k);
        SPEI_REQUIRE(!overlap(members_host[k], total, dst, total), "%s: dst overlaps member %d", name, k);
        tab.m[k] = reinterpret_cast<const uint32_t*>(members_host[k]);
        tab.op[k] = ops_host[k];
        tab.slot[k] = (ops_host[k] & 4) ? n_tr++ : 0;
        vec = vec && ((uintptr_t)members_host[k] & 15) == 0;
    }
    SPEI_REQUIRE(C <= 65535 && cdiv(H, TILE) <= 65535, "%s: %d planes of %dx%d are more than one launch covers", name, C, H, W);
    const dim3 grid(cdiv(W, TILE), cdiv(H, TILE), C);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    hipStream_t st = (hipStream_t)stream;
    switch (K) {
        case 1: launch_mean<1>(vec, tab, d, H, W, grid, n_tr, st); break;
        case 2: launch_mean<2>(vec, tab, d, H, W, grid, n_tr, st); break;
        case 4: launch_mean<4>(vec, tab, d, H, W, grid, n_tr, st); break;
        default: launch_mean<8>(vec, tab, d, H, W, grid, n_tr, st); break;
    }
    SPEI_CHECK_LAUNCH(name);
    return 0;
}
