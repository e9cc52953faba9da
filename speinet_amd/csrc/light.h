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
//
// Sensor noise (include/speinet_hip.h, "sensor noise in blur synthesis"; the spei_*_noise_u8 entries): between the quotient and the
// encode, L' = clamp(L + d, 0, S) with d drawn per byte from a counter-based generator, so that nothing depends on the launch.
//   Random words: Philox4x32-10 on the counter (x, y, run, clip) — one call per pixel, words 0..2 for R, G, B.
//   Gaussian: the 1025-word table t (Q12 quantiles at i / 1024) staged in LDS beside lin / thr (4100 bytes; two reads of
//     neighbouring words per byte), z = (t[i] (4096 - f) + t[i + 1] f + 2048) >> 12 with i = w >> 22, f = (w >> 10) & 4095:
//     |t| < 2^15, so the sum is below 2^27 + 2^11 in magnitude and fits 32 bits.
//   Variance: V = floor(X (n - 1) / n) with X = A L + B < 2^20 2^24 + 2^42 < 2^45, as ONE 64-bit multiply-high by the workgroup's
//     M = (n - 1) m, m = floor((2^64 - 1) / n) + 1 = ceil(2^64 / n), e = m n - 2^64, 0 <= e < n <= 15.  M < 2^64 (m <= 2^64 / n + 1,
//     so (n - 1) m <= 2^64 - 2^64 / n + n - 1 < 2^64), and
//         X M / 2^64 = X (n - 1) / n + X (n - 1) e / (n 2^64);     X (n - 1) e / (n 2^64) < 2^45 * 14 * 15 / (n 2^64) < 2^-11 / n < 1 / n,
//     while the fraction of X (n - 1) / n is at most (n - 1) / n: the sum never reaches the next integer, so
//     (X M) >> 64 == floor(X (n - 1) / n) for every X < 2^45 and 2 <= n <= 15.
//   sigma = isqrt(V): r = sqrt((float)V) in fp32.  (float)V = V (1 + a), |a| <= 2^-24; a square root good to one ulp returns
//     sqrt(V) (1 + a)^(1/2) (1 + b), |b| <= 2^-23: |r - sqrt(V)| < 2^22.5 (2^-25 + 2^-23 + 2^-47) < 0.89, so s = floor(r) lies in
//     [isqrt(V) - 1, isqrt(V) + 1]: one step down if s s > V, then one step up if (s + 1)^2 <= V, both compared in 64-bit integers.
//   d = (sigma z + 2048) >> 12: sigma < 2^23, |z| < 2^15 — a 64-bit product, arithmetic shift; |d| < 2^26 fits 32 bits.
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

// ---- sensor noise ----

constexpr int GAUSS_WORDS = 1025;

// all 256 threads of the workgroup; ends with a barrier
__device__ __forceinline__ void gauss_stage(int32_t* lds, const int32_t* __restrict__ gauss) {
    for (int k = threadIdx.x; k < GAUSS_WORDS; k += 256) lds[k] = gauss[k];
    __syncthreads();
}

// Philox4x32-10 (Salmon et al., SC'11) of the counter (c0, c1, c2, c3) under the key (k0, k1): output words 0, 1, 2
__device__ __forceinline__ void philox3(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[3]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2;
}

// the Q12 standard normal deviate of a random word: linear interpolation in the table of quantiles
__device__ __forceinline__ int32_t gauss_z(const int32_t* t, uint32_t w) {
    const uint32_t i = w >> 22;
    const int32_t f = (int32_t)((w >> 10) & 4095u);
    return (t[i] * (4096 - f) + t[i + 1] * f + 2048) >> 12;
}

// (n - 1) ceil(2^64 / n), n >= 2: noise_apply's multiplier for floor(X (n - 1) / n)
__device__ __forceinline__ uint64_t noise_magic(int len) { return (uint64_t)(len - 1) * (0xffffffffffffffffull / (uint64_t)len + 1ull); }

__device__ __forceinline__ uint32_t noise_isqrt(uint64_t V) {                  // V < 2^45
    uint32_t s = (uint32_t)__builtin_sqrtf((float)V);
    s -= (uint64_t)s * s > V ? 1u : 0u;
    s += (uint64_t)(s + 1u) * (s + 1u) <= V ? 1u : 0u;
    return s;
}

// L' = clamp(L + ((isqrt(floor((A L + B) (n - 1) / n)) z + 2048) >> 12), 0, S)
__device__ __forceinline__ uint32_t noise_apply(uint32_t L, int32_t z, uint32_t A, uint64_t B, uint64_t magic) {
    const uint64_t V = __umul64hi((uint64_t)A * L + B, magic);
    const int64_t d = ((int64_t)noise_isqrt(V) * z + 2048) >> 12;
    const int64_t v = (int64_t)L + d;
    return (uint32_t)(v < 0 ? 0 : v > (int64_t)LIGHT_S ? (int64_t)LIGHT_S : v);
}

// What a NOISE kernel takes beside the light's tables; one record per run (blurset.hip) or per batch record (train_batch.hip)
struct NoiseArgs {
    const int32_t* gauss;
    const spei_noise_record* rec;
    uint32_t key0, key1;
};

// The host copies of the gauss table and of n noise records, checked before a launch; 0 if valid, else -1 with the text in spei_last_error
static inline int noise_check(const char* name, const int32_t* gauss, const int32_t* gauss_host, const spei_noise_record* noise,
                              const spei_noise_record* noise_host, int n) {
    SPEI_REQUIRE(gauss && gauss_host, "%s: null gauss table (the device table and its host copy are both required)", name);
    SPEI_REQUIRE(noise && noise_host, "%s: null noise records (the device records and their host copy are both required)", name);
    for (int i = 0; i < GAUSS_WORDS; ++i) {
        SPEI_REQUIRE(gauss_host[i] > -32768 && gauss_host[i] < 32768, "%s: invalid gauss table: |t[%d]| = |%d| is not below 2^15", name, i,
                     gauss_host[i]);
        SPEI_REQUIRE(i == 0 || gauss_host[i - 1] < gauss_host[i], "%s: invalid gauss table at word %d: t[%d] = %d < t[%d] = %d does not hold",
                     name, i, i - 1, gauss_host[i - 1], i, gauss_host[i]);
    }
    for (int r = 0; r < n; ++r) {
        const spei_noise_record& c = noise_host[r];
        SPEI_REQUIRE(c.A < (1u << 20), "%s: noise record %d: A = %u is not below 2^20", name, r, c.A);
        SPEI_REQUIRE(c.B < (1ull << 42), "%s: noise record %d: B = %llu is not below 2^42", name, r, (unsigned long long)c.B);
        SPEI_REQUIRE(c.reserved == 0u, "%s: noise record %d: reserved = %u, must be 0", name, r, c.reserved);
    }
    return 0;
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
