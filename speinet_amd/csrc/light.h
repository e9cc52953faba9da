// Averaging in linear light (include/speinet_hip.h, "blur synthesis in linear light"; speinet_amd/light.py makes the tables): what
// spei_window_mean_light_u8 (blurset.hip) and spei_train_batch_runs_light_u8 (train_batch.hip) share.
//
// A workgroup stages the 512 words — lin[256], thr[256] — in LDS once (2 KB; lanes that hit the same word are served by one broadcast,
// so flat content costs nothing).  Decode is one LDS read per source byte, summed in 32 bits (at most 15 S = 251 658 225).  The
// quotient by the run's length n (uniform per workgroup) is a multiply-high: with m = floor((2^32 - 1) / n) + 1 = ceil(2^32 / n) for
// n >= 2 (m <= 2^31 fits a dword) and e = m n - 2^32, 0 <= e < n,
//     (s m) >> 32 = floor(s / n + s e / (n 2^32));     s e / (n 2^32) < 2^28 * 15 / (n 2^32) = 15 / (16 n) < 1 / n,
// and the fraction of s / n is at most (n - 1) / n, so the sum never reaches the next integer: (s m) >> 32 == s / n for every
// s <= 15 S < 2^28 and 2 <= n <= 15.  n == 1 has no such m; a run of length 1 copies its bytes (encode(lin[c]) == c for valid tables).
// Encode is a branch-free binary search over thr: eight LDS reads, thr[0] never among them.
#pragma once
#include "common.h"

constexpr uint32_t LIGHT_S = (1u << 24) - 1;
constexpr int LIGHT_WORDS = 512;

// all 256 threads of the workgroup; ends with a barrier
__device__ __forceinline__ void light_stage(uint32_t* lds, const uint32_t* __restrict__ tables) {
    lds[threadIdx.x] = tables[threadIdx.x];
    lds[threadIdx.x + 256] = tables[threadIdx.x + 256];
    __syncthreads();
}

__device__ __forceinline__ uint32_t light_magic(int len) { return 0xffffffffu / (uint32_t)len + 1u; }      // len >= 2

__device__ __forceinline__ uint32_t light_quot(uint32_t s, uint32_t magic) { return __umulhi(s, magic); }

// #{ c in 1..255 : thr[c] <= L } for strictly increasing thr[1..255]
__device__ __forceinline__ uint32_t light_encode(const uint32_t* thr, uint32_t L) {
    uint32_t c = 0u;
#pragma unroll
    for (uint32_t step = 128u; step; step >>= 1) c += thr[c + step] <= L ? step : 0u;
    return c;
}

// The host copy of the tables, checked before a launch; 0 if valid, else -1 with the text in spei_last_error
static inline int light_check(const char* name, const uint32_t* tables, const uint32_t* tables_host) {
    SPEI_REQUIRE(tables && tables_host, "%s: null light tables (the device tables and their host copy are both required)", name);
    const uint32_t *lin = tables_host, *thr = tables_host + 256;
    SPEI_REQUIRE(lin[0] == 0u, "%s: invalid light tables: lin[0] = %u, must be 0", name, lin[0]);
    SPEI_REQUIRE(lin[255] <= LIGHT_S, "%s: invalid light tables: lin[255] = %u exceeds S = %u", name, lin[255], LIGHT_S);
    for (int c = 1; c < 256; ++c)
        SPEI_REQUIRE(lin[c - 1] < thr[c] && thr[c] <= lin[c],
                     "%s: invalid light tables at code %d: lin[%d] = %u < thr[%d] = %u <= lin[%d] = %u does not hold", name, c, c - 1, lin[c - 1],
                     c, thr[c], c, lin[c]);
    return 0;
}
