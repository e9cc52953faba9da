// The host-side checks of the entries that average runs of frames, shared by blurset.hip, train_batch.hip and shake.hip: every run and
// every record is checked HERE, on the host copy, so a kernel never meets a run that leaves its clip or a record that leaves its frame.
// Each returns 0, or -1 with the text in spei_last_error.
#pragma once
#include "common.h"

#include <type_traits>

constexpr int MAX_RUN = 15;
constexpr int F_HFLIP = 1, F_VFLIP = 2, F_ROT90 = 4, F_ZERO = 8;

// spei_window_mean_*: the pointers, the sizes and the M runs (start, length) of runs_host
static inline int window_runs_check(const char* name, const unsigned char* src, int64_t frame_stride, int T, const int* runs,
                                    const int* runs_host, int M, const unsigned char* blur, const unsigned char* gt, int H, int W) {
    SPEI_REQUIRE(src && runs && runs_host && blur && gt, "%s: null pointer (src, runs, runs_host, blur and gt are required)", name);
    SPEI_REQUIRE(T > 0 && M > 0 && M <= 65535 && H > 0 && W > 0 && (int64_t)H * W * 3 < (1ll << 31),
                 "%s: bad sizes (%d frames of %dx%d, %d runs; at most 65535 runs per launch)", name, T, H, W, M);
    const int64_t hw = (int64_t)H * W;
    SPEI_REQUIRE(T == 1 || frame_stride >= hw * 3, "%s: frame stride %lld < one %dx%d frame", name, (long long)frame_stride, H, W);
    for (int m = 0; m < M; ++m) {
        const int start = runs_host[2 * m], len = runs_host[2 * m + 1];
        SPEI_REQUIRE(len >= 1 && len <= MAX_RUN, "%s: run %d has length %d (1..%d)", name, m, len, MAX_RUN);
        SPEI_REQUIRE(start >= 0 && start <= T - len, "%s: run %d = frames %d..%d leaves the clip of %d frames", name, m, start,
                     start + len - 1, T);
    }
    return 0;
}

// spei_train_batch_*: the destinations, the patch size and the n_in + n_gt records of table_host (spei_crop_record or spei_run_record)
template <typename Rec>
static inline int batch_table_check(const char* name, const Rec* table, const Rec* table_host, int n_in, int n_gt, const float* input,
                                    const float* gt, int P, float rgb_range) {
    SPEI_REQUIRE(table && table_host, "%s: null record table (the device table and its host copy are both required)", name);
    SPEI_REQUIRE(n_in >= 0 && n_gt >= 0 && n_in + n_gt > 0 && n_in + n_gt <= 65535, "%s: bad record counts %d + %d", name, n_in, n_gt);
    SPEI_REQUIRE((n_in == 0 || input) && (n_gt == 0 || gt), "%s: null dst", name);
    SPEI_REQUIRE(((uintptr_t)input & 15) == 0 && ((uintptr_t)gt & 15) == 0, "%s: dst must be 16-byte aligned", name);
    SPEI_REQUIRE(P > 0 && P % 4 == 0 && P <= 4096, "%s: patch size %d must be a positive multiple of 4 (at most 4096)", name, P);
    SPEI_REQUIRE(rgb_range > 0.0f, "%s: rgb_range %g must be positive", name, (double)rgb_range);
    for (int r = 0; r < n_in + n_gt; ++r) {
        const Rec& c = table_host[r];
        SPEI_REQUIRE((c.flags & ~15) == 0, "%s: record %d has unknown flag bits 0x%x", name, r, (unsigned)c.flags);
        if (c.flags & F_ZERO) continue;
        SPEI_REQUIRE(c.src != 0, "%s: record %d has a null frame address", name, r);
        SPEI_REQUIRE(c.H > 0 && c.W > 0 && c.W <= (1 << 24) && c.pitch >= c.W * 3, "%s: record %d: frame %dx%d with a row pitch of %d bytes", name,
                     r, c.W, c.H, c.pitch);
        SPEI_REQUIRE(c.y0 >= 0 && c.x0 >= 0 && (int64_t)c.y0 + P <= c.H && (int64_t)c.x0 + P <= c.W,
                     "%s: record %d: the %dx%d rectangle at (y %d, x %d) leaves its %dx%d frame", name, r, P, P, c.y0, c.x0, c.W, c.H);
        if constexpr (std::is_same<Rec, spei_run_record>::value) {
            SPEI_REQUIRE(c.length >= 1 && c.length <= MAX_RUN, "%s: record %d has a run of length %d (1..%d)", name, r, c.length, MAX_RUN);
            SPEI_REQUIRE(c.length <= c.avail, "%s: record %d: a run of %d frames where %d are left of its clip", name, r, c.length, c.avail);
            SPEI_REQUIRE(c.length == 1 || c.frame_stride >= (int64_t)c.H * c.pitch,
                         "%s: record %d: frame stride %lld < one %dx%d frame with a row pitch of %d bytes", name, r, (long long)c.frame_stride, c.W,
                         c.H, c.pitch);
        }
    }
    return 0;
}
