// The pixel group: the layer under the kernels that move packed [H][W][3] frames in and out of the model's fp32 planes
// (frame_io.hip, tile_io.hip, roi_io.hip).
//
// Streaming kernels, one thread per group of 4 pixels of a row: 12 samples, read or written as three dwords (uint8 samples, 12 bytes)
// or three 8-byte words (uint16 samples, 24 bytes) where the address allows and sample by sample otherwise, beside one 16-byte access
// per fp32 plane.  T is the sample type: unsigned char (D = 255) or uint16_t (10 or 12 bits in 16-bit words: depth d, D = 2^d - 1; a
// word above D reads as D).  HBM-bound: a 720p frame is 2.8 MB packed and 11 MB as planes.
//
// Everything here is written once so that the kernels agree bit for bit by construction: tile ingest with frame ingest, the hard
// stitch, the feathered stitch off its ramps and the ROI paste inside its rectangle with the frame egress.
#pragma once
#include "common.h"

namespace {

constexpr int MULT = 20;                                   // two stride-2 stages, then 5x5 windows
constexpr float INV255 = (float)(1.0 / 255.0);             // numpy2tensor's rgb_range / 255 (a Python float) as the float32 scalar
constexpr int BLOCKS_MAX = 8192;
constexpr int FEATHER_MAX = 200;

inline int grid_for(int64_t total) { return (int)((total + 255) / 256 < BLOCKS_MAX ? (total + 255) / 256 : BLOCKS_MAX); }

// a group is 12 (24) bytes: it can go as three words iff its first sample lies on a 4- (8-) byte boundary
template <typename T>
constexpr uintptr_t GROUP_MASK = sizeof(T) == 1 ? 3 : 7;

__device__ __forceinline__ int byte_of(const uint32_t (&w)[3], int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xff; }
__device__ __forceinline__ int half_of(const uint2 (&w)[3], int j) {
    const uint2 q = w[j >> 2];
    return (((j & 2) ? q.y : q.x) >> (16 * (j & 1))) & 0xffff;
}

// one sample as read: a uint8 is its value, a 16-bit word is clamped to D
template <typename T>
__device__ __forceinline__ int sample_of(T s, int D) {
    if constexpr (sizeof(T) == 1) return (int)s;
    else return min((int)s, D);
}

// the 12 samples of a group of 4 pixels at p, clamped to D; `valid` pixels (1..4) exist, the others read as 0
template <typename T>
__device__ __forceinline__ void load_group(const T* __restrict__ p, int valid, bool aligned, int D, int (&c)[12]) {
    if (valid == 4 && aligned) {
        if constexpr (sizeof(T) == 1) {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
            const uint32_t w[3] = {q[0], q[1], q[2]};
#pragma unroll
            for (int j = 0; j < 12; ++j) c[j] = byte_of(w, j);
        } else {
            const uint2* q = reinterpret_cast<const uint2*>(p);
            const uint2 w[3] = {q[0], q[1], q[2]};
#pragma unroll
            for (int j = 0; j < 12; ++j) c[j] = min(half_of(w, j), D);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) c[j] = j < 3 * valid ? sample_of(p[j], D) : 0;
    }
}

// the same group of uint8 samples kept packed, as its three dwords (the bytes of a missing pixel read as 0): for a kernel that takes
// the samples out where it needs them, which keeps the registers of spei_frame_pair_stats few
__device__ __forceinline__ void load_group(const unsigned char* __restrict__ p, int valid, bool aligned, int, uint32_t (&w)[3]) {
    if (valid == 4 && aligned) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        w[0] = q[0]; w[1] = q[1]; w[2] = q[2];
    } else {
        w[0] = w[1] = w[2] = 0u;
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (j < 3 * valid) w[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
    }
}

// the integer luma Y = (77 R + 150 G + 29 B + 128) >> 8, at the depth of the samples, and that of pixel k of a group
__device__ __forceinline__ int luma(int r, int g, int b) { return (77 * r + 150 * g + 29 * b + 128) >> 8; }
__device__ __forceinline__ int luma_of(const int (&c)[12], int k) { return luma(c[3 * k], c[3 * k + 1], c[3 * k + 2]); }
__device__ __forceinline__ int luma_of(const uint32_t (&w)[3], int k) {
    return luma(byte_of(w, 3 * k), byte_of(w, 3 * k + 1), byte_of(w, 3 * k + 2));
}

// the ingest of one group: pixels x .. x + 3 of the row at s, W pixels long, as floats v[channel][pixel] in 0..D.  The row may be
// shorter than x + 4 (the right edge and the reflect pad of the planes): column W + j reads column W - 2 - j, as torch's F.pad
// mode "reflect".  `aligned`: the row's first sample lies on a GROUP_MASK boundary, so an interior group goes as three words.
template <typename T>
__device__ __forceinline__ void ingest_group(const T* __restrict__ s, int x, int W, bool aligned, int D, float (&v)[3][4]) {
    if (x + 4 <= W) {                                      // interior: 12 consecutive samples, as words or one by one
        int c[12];
        load_group(s + x * 3, 4, aligned, D, c);
#pragma unroll
        for (int j = 0; j < 12; ++j) v[j % 3][j / 3] = (float)c[j];
    } else {                                               // right edge and pad band: the mirrored columns
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xx = x + k, sx = xx < W ? xx : 2 * W - 2 - xx;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][k] = (float)sample_of(s[sx * 3 + c], D);
        }
    }
}

// the input sample at the output depth: v * Dout / Din rounded half up, in integers (at most 4095 * 8190 + 4095 < 2^26); v is a
// sample as read, so at most Din.  The one definition behind spei_frame_requant and the outside of spei_roi_paste_*
__device__ __forceinline__ uint32_t requant(int v, int Din, int Dout) {
    if (Din == Dout) return (uint32_t)v;
    const uint32_t n = (uint32_t)v * 2u * (uint32_t)Dout + (uint32_t)Din;
    return Din == 255 ? n / 510u : Din == 1023 ? n / 2046u : n / 8190u;       // constant divisors: a multiply and a shift each
}

// do the byte ranges [a, a + na) and [b, b + nb) meet (host)
inline bool bytes_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

// mul(D).clamp(0, D).round() of tensor2numpy: half to even, as torch.  `round_sample` is for a value known to be finite;
// `quantise` gives 0 for one that is not (rounded before the test: a select, no branch around the rounding)
__device__ __forceinline__ float rounded(float v, float Df) { return rintf(fminf(fmaxf(v * Df, 0.0f), Df)); }
__device__ __forceinline__ uint32_t round_sample(float v, float Df) { return (uint32_t)rounded(v, Df); }
__device__ __forceinline__ uint32_t quantise(float v, float Df) {
    const float q = rounded(v, Df);
    return isfinite(v) ? (uint32_t)q : 0u;
}

// four pixels of the three planes at s, 16-byte aligned there -> their samples q[channel][pixel]; returns nonzero iff one of the
// first `valid` pixels held a non-finite value (a pixel past them is pad, not part of the frame)
__device__ __forceinline__ int quantise_planes(const float* __restrict__ s, int64_t plane, float Df, int valid, uint32_t (&q)[3][4]) {
    int bad = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float4 f = *reinterpret_cast<const float4*>(s + c * plane);
        const float e[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            q[c][k] = quantise(e[k], Df);
            bad |= (k < valid && !isfinite(e[k])) ? 1 : 0;
        }
    }
    return bad;
}

// the egress of one group: samples q[channel][pixel] to the packed pixels at d.  `vec`: d lies on a GROUP_MASK boundary; then a
// whole group (valid >= 4) goes as three dwords (three 8-byte words).  Otherwise the first `valid` pixels go sample by sample
template <typename T>
__device__ __forceinline__ void store_group(T* __restrict__ d, const uint32_t (&q)[3][4], bool vec, int valid) {
    if (vec && valid >= 4) {
        if constexpr (sizeof(T) == 1) {
            uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 12; ++j) w[j >> 2] |= q[j % 3][j / 3] << (8 * (j & 3));
            uint32_t* p = reinterpret_cast<uint32_t*>(d);
            p[0] = w[0]; p[1] = w[1]; p[2] = w[2];
        } else {
            uint32_t w[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 12; ++j) w[j >> 1] |= q[j % 3][j / 3] << (16 * (j & 1));
            uint2* p = reinterpret_cast<uint2*>(d);
            p[0] = make_uint2(w[0], w[1]); p[1] = make_uint2(w[2], w[3]); p[2] = make_uint2(w[4], w[5]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < valid)
#pragma unroll
                for (int c = 0; c < 3; ++c) d[k * 3 + c] = (T)q[c][k];
    }
}

}  // namespace
