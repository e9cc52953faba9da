// The 32 x 32 tile of the training-batch kernels (train_batch.hip, shake.hip): the geometry of a record's flags, the 12-byte row
// segment loads, the packed-pixel LDS tile and the flip / rotate / store phase.  train_batch.hip's header has the reasoning.
#pragma once
#include "common.h"
#include "run_checks.h"

constexpr int TILE = 32, PITCH = TILE + 1;

// 12 bytes = 4 pixels of one source row, as three dwords
__device__ __forceinline__ void load12(const unsigned char* s, bool dwords, uint32_t w[3]) {
    if (dwords) {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(s);
        w[0] = p[0]; w[1] = p[1]; w[2] = p[2];
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            w[k] = (uint32_t)s[4 * k] | ((uint32_t)s[4 * k + 1] << 8) | ((uint32_t)s[4 * k + 2] << 16) | ((uint32_t)s[4 * k + 3] << 24);
    }
}

// 12 bytes = 4 pixels: pixel k is bytes 3k .. 3k+2 -> one dword 0x00BBGGRR each
__device__ __forceinline__ void unpack12(const uint32_t w[3], uint32_t px[4]) {
    const uint64_t lo = (uint64_t)w[0] | ((uint64_t)w[1] << 32), hi = (uint64_t)w[1] | ((uint64_t)w[2] << 32);
    px[0] = (uint32_t)lo & 0xffffffu;
    px[1] = (uint32_t)(lo >> 24) & 0xffffffu;
    px[2] = (uint32_t)(hi >> 16) & 0xffffffu;
    px[3] = (uint32_t)(hi >> 40) & 0xffffffu;
}

// One workgroup's output tile of a P x P patch and the source tile it reads: output rows [oi0, oi0 + nI), columns [oj0, oj0 + nJ)
// (multiples of 4: P % 4 == 0); inside the crop rows [cy_lo, cy_lo + nR), columns [cx_lo, cx_lo + nC), cx_lo % 4 == 0
struct TileGeom {
    int oi0, oj0, nI, nJ, nR, nC, cy_lo, cx_lo;
    bool hf, vf, rot, zero;
};

__device__ __forceinline__ TileGeom tile_geom(int flags, int P, int tiles) {
    TileGeom g;
    g.oi0 = (blockIdx.x / tiles) * TILE;
    g.oj0 = (blockIdx.x % tiles) * TILE;
    g.nI = min(TILE, P - g.oi0);
    g.nJ = min(TILE, P - g.oj0);
    g.hf = flags & F_HFLIP; g.vf = flags & F_VFLIP; g.rot = flags & F_ROT90; g.zero = flags & F_ZERO;
    g.nR = g.rot ? g.nJ : g.nI;
    g.nC = g.rot ? g.nI : g.nJ;
    g.cy_lo = g.rot ? (g.vf ? P - g.oj0 - g.nJ : g.oj0) : (g.vf ? P - g.oi0 - g.nI : g.oi0);
    g.cx_lo = g.rot ? (g.hf ? g.oi0 : P - g.oi0 - g.nI) : (g.hf ? P - g.oj0 - g.nJ : g.oj0);
    return g;
}

// The store phase, after the barrier that follows the load phase: thread (row, g4) writes 4 pixels of output row oi0 + row of record r as
// one 16-byte store per plane, reading the packed source tile `lds` transposed and / or mirrored as the flags say
__device__ __forceinline__ void store_tile(const uint32_t* lds, const TileGeom& g, int r, int n_in, float* __restrict__ input,
                                           float* __restrict__ gt, int P, float scale) {
    const int row = threadIdx.x >> 3, g4 = (threadIdx.x & 7) * 4;
    if (row >= g.nI || g4 >= g.nJ) return;
    const int i = g.oi0 + row;
    float v[3][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = g.oj0 + g4 + k;
        const int cy = g.rot ? (g.vf ? P - 1 - j : j) : (g.vf ? P - 1 - i : i);
        const int cx = g.rot ? (g.hf ? i : P - 1 - i) : (g.hf ? P - 1 - j : j);
        const uint32_t px = g.zero ? 0u : lds[(cy - g.cy_lo) * PITCH + (cx - g.cx_lo)];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][k] = (float)((px >> (8 * c)) & 0xffu) * scale;
    }
    float* base = r < n_in ? input + (int64_t)r * 3 * P * P : gt + (int64_t)(r - n_in) * 3 * P * P;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4*>(base + ((int64_t)c * P + i) * P + g.oj0 + g4) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
}
