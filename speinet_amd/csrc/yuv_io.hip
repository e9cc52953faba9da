// Planar YUV frames of the clip API (speinet_amd/y4m.py, speinet_amd/video.py): the payload of a YUV4MPEG2 FRAME in, one out.  An
// extension beyond the reference, which reads and writes image files only.
//
//   spei_yuv_to_rgb_u8 — N planar uint8 frames (Y [H][W], then U, then V: [ceil(H/2)][ceil(W/2)] each for 4:2:0, [H][W] each for
//                        4:4:4) -> N packed uint8 [H][W][3] RGB frames, what spei_frames_u8_in and spei_frame_pair_stats take.
//   spei_rgb_u8_to_yuv — one packed uint8 [H][W][3] RGB frame (what spei_frame_u8_out makes) -> one planar frame.
//   spei_planar_to_rgb_u8, spei_rgb_u8_to_planar — the same two for 4:2:2 (U, V: [H][ceil(W/2)] each, co-sited with the even column
//                        of their own row) and mono (the Y plane alone) frames: two more LAYOUT values of the same kernels.
//   spei_yuv_fields_to_rgb_u8, spei_rgb_u8_to_yuv_fields (and _u16) — the same on an INTERLACED frame of any layout (the clip API's
//                        fields="split"): the woven frame whose field p (rows p :: 2) is the conversion of field p's own planar
//                        picture, Y rows p :: 2 and, for 4:2:0, chroma-plane rows p :: 2 (H % 4 == 0), so no chroma of one instant
//                        reaches a row of the other.  The same kernels with a row pitch of 2 and the parity as offset (`fld`).
//
// Integer arithmetic only: the result is defined bit for bit and depends on neither the launch shape nor the access path.  `>>` is
// an arithmetic shift (it floors).  Clipping is to [0,255] for RGB and full range, to [16,235] (Y) and [16,240] (U, V) for limited.
//
// YUV -> RGB.  The chroma of a full-resolution pixel is formed times 16 (U16, V16), neighbour indices clamped to the plane:
//   4:4:4          U16 = 16 U[y][x]
//   4:2:0 rows     j = y >> 1, the other row j - 1 (y even) or j + 1 (y odd), weights 3 : 1 (both sitings)
//   CENTER columns the same rule with i = x >> 1
//   LEFT columns   4 : 0 at even x (co-sited), 2 : 2 of columns i and i + 1 at odd x
//   4:2:2          LEFT's column rule on row y itself: U16 = 16 U[y][i] at even x, 8 (U[y][i] + U[y][i + 1]) at odd x
//   mono           U16 = V16 = 2048: R = G = B
// then, with yy = cy * 16 * (Y - yo), u = U16 - 2048, v = V16 - 2048:
//   R = clip((yy + rv v + 2^17) >> 18)   G = clip((yy + gu u + gv v + 2^17) >> 18)   B = clip((yy + bu u + 2^17) >> 18)
// Every intermediate fits int32 (about 1.5e8 at most).
//
// RGB -> YUV.  Y = clip(((yr R + yg G + yb B + 2^13) >> 14) + yo) per pixel.  Chroma:
//   4:4:4   U = clip(((ur R + ug G + ub B + 2^13) >> 14) + 128) per pixel, V likewise
//   CENTER  the same on S_c, the sum of channel c over rows 2j, 2j + 1 and columns 2i, 2i + 1, with 2^15 and >> 16
//   LEFT    the same on the sum over rows 2j, 2j + 1 of c[2i - 1] + 2 c[2i] + c[2i + 1], with 2^16 and >> 17
//   4:2:2   the same on c[y][2i - 1] + 2 c[y][2i] + c[y][2i + 1] of row y alone, with 2^15 and >> 16 (mono: no chroma)
// indices clamped to the frame.  The 4:2:0 resampling (3 : 1 bilinear up, box or [1 2 1] down) is this project's own definition.
//
// Streaming kernels in the style of frame_io.hip, one thread per group of 4 pixels of a row in a grid-stride loop: dword accesses
// where the rows are 4-byte aligned, bytes otherwise and at the right edge.  In spei_rgb_u8_to_yuv the thread of an even row and an
// even group also makes the (up to) 4 chroma samples of the 2 x 8 pixels below and right of it; the RGB bytes it reads again for
// that are its neighbours' and come from the cache (4:2:2: the even group of every row, for the 8 pixels right of it).  No atomics.
// HBM-bound: a 720p 4:2:0 frame is 1.4 MB on one side and 2.8 MB on the other.
#include "common.h"

namespace {

// 2 blocks per compute unit: a frame is a few MB, so the launch is over before more waves per SIMD would pay
constexpr int BLOCKS_MAX = 512;

// Q14 constants, round(c * 16384).  Each chroma row sums to 0 and each luma row to 16384 (full) or round(16384 * 219 / 255)
// (limited): gray stays gray.
struct Coef {
    int yr, yg, yb, ur, ug, ub, vr, vg, vb, yo, cy, rv, gu, gv, bu;
};
constexpr Coef COEF[2][2] = {
    // [matrix][range]:  yr     yg    yb     ur     ug    ub    vr     vg     vb  yo     cy     rv     gu      gv     bu
    {/* 601 full    */ {4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332, 0, 16384, 22970, -5638, -11700, 29032},
     /* 601 limited */ {4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170, 16, 19077, 26149, -6419, -13320, 33050}},
    {/* 709 full    */ {3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751, 0, 16384, 25802, -3069, -7670, 30402},
     /* 709 limited */ {2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660, 16, 19077, 29372, -3494, -8731, 34610}},
};

__device__ __forceinline__ int clip(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ int byte_at(uint32_t w, int j) { return (w >> (8 * j)) & 0xff; }

// 4 bytes of a plane row from column x0: one dword, or bytes with the column clamped to the row (the lanes past W are not stored)
__device__ __forceinline__ void load4(const unsigned char* __restrict__ row, int x0, int W, bool dword, int (&v)[4]) {
    if (dword) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(row + x0);
#pragma unroll
        for (int p = 0; p < 4; ++p) v[p] = byte_at(w, p);
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p) v[p] = row[min(x0 + p, W - 1)];
    }
}

// 4 bytes of a plane row to column x0: one dword, or the bytes of the columns below W
__device__ __forceinline__ void store4(unsigned char* __restrict__ row, int x0, int W, bool dword, const int (&v)[4]) {
    if (dword) {
        *reinterpret_cast<uint32_t*>(row + x0) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (x0 + p < W) row[x0 + p] = (unsigned char)v[p];
    }
}

// samples of one chroma plane: [H][W] for 4:4:4, [H][ceil(W/2)] for 4:2:2, none for mono, [ceil(H/2)][ceil(W/2)] for 4:2:0
__host__ __device__ __forceinline__ int64_t chroma_size(int H, int W, int layout) {
    if (layout == SPEI_YUV_444) return (int64_t)H * W;
    if (layout == SPEI_YUV_MONO) return 0;
    return (int64_t)(layout == SPEI_YUV_422 ? H : (H + 1) >> 1) * ((W + 1) >> 1);
}

// Rows of a 4:2:0 picture, progressive (fld = 0) or the two woven fields of an interlaced one (fld = 1; H % 4 == 0).  Field p = y & 1
// of frame row y is a planar picture of its own: its Y rows are the frame's rows p :: 2 and its chroma rows the chroma plane's rows
// p :: 2, so a row index of that picture has the pitch 1 << fld and the offset p in the frame's planes.  With fld = 0 every expression
// below is the progressive one.
//   chroma_rows — the chroma rows of the picture that the 3 : 1 row rule clamps to: ceil(H / 2), or H / 4 of a field
//   chroma_row  — the chroma-plane row of chroma row j of the picture that frame row y belongs to
//   next_row    — the frame row below frame row y in its picture, clamped to the picture's last row
__host__ __device__ __forceinline__ int chroma_rows(int H, int fld) { return fld ? H >> 2 : (H + 1) >> 1; }
__device__ __forceinline__ int chroma_row(int j, int y, int fld) { return (j << fld) + (y & fld); }
__device__ __forceinline__ int next_row(int y, int H, int fld) { return y + 1 + fld < H ? y + 1 + fld : y; }

template <int LAYOUT>
__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(const unsigned char* __restrict__ src, int64_t fstride,
                                                         unsigned char* __restrict__ dst, int H, int W, int64_t total, Coef k,
                                                         int aligned, int fld) {
    const int gw = (W + 3) >> 2, Hc = chroma_rows(H, fld), Wc = (W + 1) >> 1;
    const int64_t ysize = (int64_t)H * W, csize = chroma_size(H, W, LAYOUT);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / gw;                        // n * H + y
        const int x0 = (int)(i - row * gw) * 4;
        const int n = (int)(row / H), y = (int)(row - (int64_t)n * H);
        const unsigned char* f = src + n * fstride;
        const unsigned char* up = f + ysize;
        const unsigned char* vp = up + csize;
        const bool dword = aligned && x0 + 4 <= W;
        int Y[4], U16[4], V16[4];
        load4(f + (int64_t)y * W, x0, W, dword, Y);
        if (LAYOUT == SPEI_YUV_444) {
            load4(up + (int64_t)y * W, x0, W, dword, U16);
            load4(vp + (int64_t)y * W, x0, W, dword, V16);
#pragma unroll
            for (int p = 0; p < 4; ++p) { U16[p] *= 16; V16[p] *= 16; }
        } else if (LAYOUT == SPEI_YUV_MONO) {
#pragma unroll
            for (int p = 0; p < 4; ++p) U16[p] = V16[p] = 2048;
        } else if (LAYOUT == SPEI_YUV_422) {
            // chroma columns i0 .. i0 + 2 (clamped) of row y serve the 4 pixels: LEFT's column rule, no row step
            const int i0 = x0 >> 1;
            const int64_t r = (int64_t)y * Wc;
            int u[3], v[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int c = min(i0 + q, Wc - 1);
                u[q] = up[r + c];
                v[q] = vp[r + c];
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int a = p >> 1;                      // column i = x >> 1
                U16[p] = (p & 1) ? 8 * (u[a] + u[a + 1]) : 16 * u[a];
                V16[p] = (p & 1) ? 8 * (v[a] + v[a + 1]) : 16 * v[a];
            }
        } else {
            // chroma columns i0 - 1 .. i0 + 2 (clamped) serve the 4 pixels; rows first: 3 of row j, 1 of the other
            const int fy = y >> fld, j = fy >> 1, jo = clip((fy & 1) ? j + 1 : j - 1, 0, Hc - 1), i0 = x0 >> 1;
            const int64_t rj = (int64_t)chroma_row(j, y, fld) * Wc, ro = (int64_t)chroma_row(jo, y, fld) * Wc;
            int u[4], v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = clip(i0 - 1 + q, 0, Wc - 1);
                u[q] = 3 * up[rj + c] + up[ro + c];
                v[q] = 3 * vp[rj + c] + vp[ro + c];
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int a = 1 + (p >> 1);                // column i = x >> 1
                if (LAYOUT == SPEI_YUV_420_CENTER) {
                    const int b = (p & 1) ? a + 1 : a - 1;
                    U16[p] = 3 * u[a] + u[b];
                    V16[p] = 3 * v[a] + v[b];
                } else {
                    U16[p] = (p & 1) ? 2 * (u[a] + u[a + 1]) : 4 * u[a];
                    V16[p] = (p & 1) ? 2 * (v[a] + v[a + 1]) : 4 * v[a];
                }
            }
        }
        int q[12];                                         // R G B of 4 pixels
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int yy = k.cy * 16 * (Y[p] - k.yo), u = U16[p] - 2048, v = V16[p] - 2048;
            q[3 * p + 0] = clip((yy + k.rv * v + (1 << 17)) >> 18, 0, 255);
            q[3 * p + 1] = clip((yy + k.gu * u + k.gv * v + (1 << 17)) >> 18, 0, 255);
            q[3 * p + 2] = clip((yy + k.bu * u + (1 << 17)) >> 18, 0, 255);
        }
        unsigned char* d = dst + (row * W + x0) * 3;
        if (dword) {                                       // 12 bytes as three dwords
            uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
            for (int t = 0; t < 12; ++t) w[t >> 2] |= (uint32_t)q[t] << (8 * (t & 3));
            uint32_t* o = reinterpret_cast<uint32_t*>(d);
            o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
        } else {
#pragma unroll
            for (int t = 0; t < 12; ++t)
                if (x0 + t / 3 < W) d[t] = (unsigned char)q[t];
        }
    }
}

template <int LAYOUT>
__global__ __launch_bounds__(256) void rgb_to_yuv_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int H,
                                                         int W, int64_t total, Coef k, int limited, int al_src, int al_y, int al_c,
                                                         int fld) {
    const int gw = (W + 3) >> 2, Wc = (W + 1) >> 1;
    const int64_t ysize = (int64_t)H * W, csize = chroma_size(H, W, LAYOUT);
    constexpr bool TWO = LAYOUT != SPEI_YUV_422;           // a chroma sample spans two rows (4:2:0) or one
    const int ylo = limited ? 16 : 0, yhi = limited ? 235 : 255, clo = ylo, chi = limited ? 240 : 255;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / gw), g = (int)(i - (int64_t)y * gw), x0 = g * 4;
        const unsigned char* r0 = src + (int64_t)y * W * 3;
        int c[12];                                         // R G B of 4 pixels
        if (al_src && x0 + 4 <= W) {
            const uint32_t* p = reinterpret_cast<const uint32_t*>(r0 + x0 * 3);
            const uint32_t w[3] = {p[0], p[1], p[2]};
#pragma unroll
            for (int t = 0; t < 12; ++t) c[t] = byte_at(w[t >> 2], t & 3);
        } else {                                           // the lanes past W read column W - 1 and are not stored
#pragma unroll
            for (int t = 0; t < 12; ++t) c[t] = r0[min(x0 + t / 3, W - 1) * 3 + t % 3];
        }
        int Y[4], U[4], V[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int R = c[3 * p], G = c[3 * p + 1], B = c[3 * p + 2];
            Y[p] = clip(((k.yr * R + k.yg * G + k.yb * B + (1 << 13)) >> 14) + k.yo, ylo, yhi);
            if (LAYOUT == SPEI_YUV_444) {
                U[p] = clip(((k.ur * R + k.ug * G + k.ub * B + (1 << 13)) >> 14) + 128, clo, chi);
                V[p] = clip(((k.vr * R + k.vg * G + k.vb * B + (1 << 13)) >> 14) + 128, clo, chi);
            }
        }
        const bool dword = al_y && x0 + 4 <= W;
        store4(dst + (int64_t)y * W, x0, W, dword, Y);
        if (LAYOUT == SPEI_YUV_444) {
            store4(dst + ysize + (int64_t)y * W, x0, W, dword, U);
            store4(dst + 2 * ysize + (int64_t)y * W, x0, W, dword, V);
        } else if (LAYOUT != SPEI_YUV_MONO && (!TWO || !((y >> fld) & 1)) && !(g & 1)) {
            // chroma samples (j, i0 .. i0 + 3) of rows y, y + 1 (4:2:2: of row y alone) and columns x0 .. x0 + 7: s[ch][q] is the sum
            // over those rows of channel ch at column x0 - 1 + q, rows and columns clamped to the frame (q = 0 is the left neighbour
            // of LEFT and 4:2:2)
            const int j = TWO ? chroma_row(y >> fld >> 1, y, fld) : y, i0 = x0 >> 1;
            const unsigned char* r1 = src + (int64_t)next_row(y, H, fld) * W * 3;
            int s[3][9];
            if (al_src && x0 + 8 <= W) {
                const uint32_t* a = reinterpret_cast<const uint32_t*>(r0 + x0 * 3);
                const uint32_t* b = reinterpret_cast<const uint32_t*>(r1 + x0 * 3);
#pragma unroll
                for (int d = 0; d < 6; ++d) {
                    const uint32_t wa = a[d], wb = TWO ? b[d] : 0u;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int t = 4 * d + e;
                        s[t % 3][1 + t / 3] = byte_at(wa, e) + byte_at(wb, e);
                    }
                }
                const int xl = max(x0 - 1, 0) * 3;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) s[ch][0] = LAYOUT == SPEI_YUV_420_CENTER ? 0 : r0[xl + ch] + (TWO ? r1[xl + ch] : 0);
            } else {
#pragma unroll
                for (int q = 0; q < 9; ++q) {
                    const int x = clip(x0 - 1 + q, 0, W - 1) * 3;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) s[ch][q] = r0[x + ch] + (TWO ? r1[x + ch] : 0);
                }
            }
            int Uc[4], Vc[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                int S[3];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    S[ch] = LAYOUT == SPEI_YUV_420_CENTER ? s[ch][1 + 2 * m] + s[ch][2 + 2 * m]
                                                          : s[ch][2 * m] + 2 * s[ch][1 + 2 * m] + s[ch][2 + 2 * m];
                constexpr int SH = LAYOUT == SPEI_YUV_420_LEFT ? 17 : 16;     // Q14 and the sum's 4 (CENTER, 4:2:2) or 8 (LEFT) weights
                Uc[m] = clip(((k.ur * S[0] + k.ug * S[1] + k.ub * S[2] + (1 << (SH - 1))) >> SH) + 128, clo, chi);
                Vc[m] = clip(((k.vr * S[0] + k.vg * S[1] + k.vb * S[2] + (1 << (SH - 1))) >> SH) + 128, clo, chi);
            }
            unsigned char* uo = dst + ysize + (int64_t)j * Wc;
            const bool cdword = al_c && i0 + 4 <= Wc;
            store4(uo, i0, Wc, cdword, Uc);
            store4(uo + csize, i0, Wc, cdword, Vc);
        }
    }
}

// ---- deep samples (10 and 12 bits in little-endian 16-bit words) ------------------------------------------------------------------
// The same two kernels on uint16 samples, depth d = 8 + s, D = 2^d - 1; a word above D reads as D.  Full range uses the rows of
// COEF; limited range has rows of its own per depth (the rule is in include/speinet_hip.h).  One thread per group of 4 pixels as
// above: 8-byte accesses of Y / U / V rows and three of them per 24-byte RGB group where base, stride and W allow, elements
// otherwise and at the right edge.  Every product fits int32; the YUV -> RGB sums are taken in 64 bits (2.3e9 at 12-bit limited).
constexpr Coef COEF_DEEP[2][2] = {
    // [depth 10, 12][matrix], limited range
    {/* 10 601 */ {4195, 8236, 1599, -2421, -4754, 7175, 7175, -6008, -1167, 64, 19133, 26226, -6438, -13359, 33148},
     /* 10 709 */ {2983, 10034, 1013, -1644, -5531, 7175, 7175, -6517, -658, 64, 19133, 29459, -3504, -8757, 34711}},
    {/* 12 601 */ {4192, 8229, 1598, -2420, -4750, 7170, 7170, -6004, -1166, 256, 19147, 26245, -6442, -13369, 33172},
     /* 12 709 */ {2981, 10026, 1012, -1643, -5527, 7170, 7170, -6513, -657, 256, 19147, 29480, -3507, -8763, 34737}},
};

__device__ __forceinline__ int half_at(const uint2& w, int j) { return ((j < 2 ? w.x : w.y) >> (16 * (j & 1))) & 0xffff; }
__device__ __forceinline__ uint2 pack4(int a, int b, int c, int d) {
    return make_uint2((uint32_t)a | ((uint32_t)b << 16), (uint32_t)c | ((uint32_t)d << 16));
}

// 4 samples of a plane row from column x0, each at most D: one 8-byte load, or elements with the column clamped to the row
__device__ __forceinline__ void load4(const uint16_t* __restrict__ row, int x0, int W, bool wide, int D, int (&v)[4]) {
    if (wide) {
        const uint2 w = *reinterpret_cast<const uint2*>(row + x0);
#pragma unroll
        for (int p = 0; p < 4; ++p) v[p] = min(half_at(w, p), D);
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p) v[p] = min((int)row[min(x0 + p, W - 1)], D);
    }
}

__device__ __forceinline__ void store4(uint16_t* __restrict__ row, int x0, int W, bool wide, const int (&v)[4]) {
    if (wide) {
        *reinterpret_cast<uint2*>(row + x0) = pack4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (x0 + p < W) row[x0 + p] = (uint16_t)v[p];
    }
}

// 12 samples (R G B of 4 pixels) from p, each at most D: three 8-byte loads, or elements (pixel x0 + t / 3 clamped to column W - 1)
__device__ __forceinline__ void load_rgb4(const uint16_t* __restrict__ row, int x0, int W, bool wide, int D, int (&c)[12]) {
    if (wide) {
        const uint2* p = reinterpret_cast<const uint2*>(row + x0 * 3);
        const uint2 w[3] = {p[0], p[1], p[2]};
#pragma unroll
        for (int t = 0; t < 12; ++t) c[t] = min(half_at(w[t >> 2], t & 3), D);
    } else {
#pragma unroll
        for (int t = 0; t < 12; ++t) c[t] = min((int)row[min(x0 + t / 3, W - 1) * 3 + t % 3], D);
    }
}

__device__ __forceinline__ int clip_deep(int64_t v, int D) { return (int)min(max(v, (int64_t)0), (int64_t)D); }

template <int LAYOUT>
__global__ __launch_bounds__(256) void yuv_to_rgb_u16_kernel(const uint16_t* __restrict__ src, int64_t fstride,
                                                             uint16_t* __restrict__ dst, int H, int W, int64_t total, Coef k, int s,
                                                             int aligned, int fld) {
    const int gw = (W + 3) >> 2, Hc = chroma_rows(H, fld), Wc = (W + 1) >> 1, D = (256 << s) - 1;
    const int64_t ysize = (int64_t)H * W, csize = chroma_size(H, W, LAYOUT);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / gw;                        // n * H + y
        const int x0 = (int)(i - row * gw) * 4;
        const int n = (int)(row / H), y = (int)(row - (int64_t)n * H);
        const uint16_t* f = src + n * fstride;             // fstride in samples
        const uint16_t* up = f + ysize;
        const uint16_t* vp = up + csize;
        const bool wide = aligned && x0 + 4 <= W;
        int Y[4], U16[4], V16[4];
        load4(f + (int64_t)y * W, x0, W, wide, D, Y);
        if (LAYOUT == SPEI_YUV_444) {
            load4(up + (int64_t)y * W, x0, W, wide, D, U16);
            load4(vp + (int64_t)y * W, x0, W, wide, D, V16);
#pragma unroll
            for (int p = 0; p < 4; ++p) { U16[p] *= 16; V16[p] *= 16; }
        } else if (LAYOUT == SPEI_YUV_MONO) {
#pragma unroll
            for (int p = 0; p < 4; ++p) U16[p] = V16[p] = 2048 << s;
        } else if (LAYOUT == SPEI_YUV_422) {
            const int i0 = x0 >> 1;
            const int64_t r = (int64_t)y * Wc;
            int u[3], v[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int c = min(i0 + q, Wc - 1);
                u[q] = min((int)up[r + c], D);
                v[q] = min((int)vp[r + c], D);
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int a = p >> 1;                      // column i = x >> 1
                U16[p] = (p & 1) ? 8 * (u[a] + u[a + 1]) : 16 * u[a];
                V16[p] = (p & 1) ? 8 * (v[a] + v[a + 1]) : 16 * v[a];
            }
        } else {
            const int fy = y >> fld, j = fy >> 1, jo = clip((fy & 1) ? j + 1 : j - 1, 0, Hc - 1), i0 = x0 >> 1;
            const int64_t rj = (int64_t)chroma_row(j, y, fld) * Wc, ro = (int64_t)chroma_row(jo, y, fld) * Wc;
            int u[4], v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = clip(i0 - 1 + q, 0, Wc - 1);
                u[q] = 3 * min((int)up[rj + c], D) + min((int)up[ro + c], D);
                v[q] = 3 * min((int)vp[rj + c], D) + min((int)vp[ro + c], D);
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int a = 1 + (p >> 1);                // column i = x >> 1
                if (LAYOUT == SPEI_YUV_420_CENTER) {
                    const int b = (p & 1) ? a + 1 : a - 1;
                    U16[p] = 3 * u[a] + u[b];
                    V16[p] = 3 * v[a] + v[b];
                } else {
                    U16[p] = (p & 1) ? 2 * (u[a] + u[a + 1]) : 4 * u[a];
                    V16[p] = (p & 1) ? 2 * (v[a] + v[a + 1]) : 4 * v[a];
                }
            }
        }
        int q[12];                                         // R G B of 4 pixels
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            // int32 products (at most 1.3e9), 64-bit sums
            const int u = U16[p] - (2048 << s), v = V16[p] - (2048 << s);
            const int64_t yy = (int64_t)(k.cy * 16 * (Y[p] - k.yo)) + (1 << 17);
            q[3 * p + 0] = clip_deep((yy + k.rv * v) >> 18, D);
            q[3 * p + 1] = clip_deep((yy + (k.gu * u + k.gv * v)) >> 18, D);
            q[3 * p + 2] = clip_deep((yy + k.bu * u) >> 18, D);
        }
        uint16_t* d = dst + (row * W + x0) * 3;
        if (wide) {                                        // 24 bytes as three 8-byte stores
            uint2* o = reinterpret_cast<uint2*>(d);
            o[0] = pack4(q[0], q[1], q[2], q[3]);
            o[1] = pack4(q[4], q[5], q[6], q[7]);
            o[2] = pack4(q[8], q[9], q[10], q[11]);
        } else {
#pragma unroll
            for (int t = 0; t < 12; ++t)
                if (x0 + t / 3 < W) d[t] = (uint16_t)q[t];
        }
    }
}

template <int LAYOUT>
__global__ __launch_bounds__(256) void rgb_u16_to_yuv_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, int H, int W,
                                                             int64_t total, Coef k, int limited, int s, int al_src, int al_y, int al_c,
                                                             int fld) {
    const int gw = (W + 3) >> 2, Wc = (W + 1) >> 1, D = (256 << s) - 1, mid = 128 << s;
    const int64_t ysize = (int64_t)H * W, csize = chroma_size(H, W, LAYOUT);
    constexpr bool TWO = LAYOUT != SPEI_YUV_422;           // a chroma sample spans two rows (4:2:0) or one
    const int ylo = limited ? 16 << s : 0, yhi = limited ? 235 << s : D, clo = ylo, chi = limited ? 240 << s : D;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / gw), g = (int)(i - (int64_t)y * gw), x0 = g * 4;
        const uint16_t* r0 = src + (int64_t)y * W * 3;
        int c[12];                                         // R G B of 4 pixels
        load_rgb4(r0, x0, W, al_src && x0 + 4 <= W, D, c);
        int Y[4], U[4], V[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int R = c[3 * p], G = c[3 * p + 1], B = c[3 * p + 2];
            Y[p] = clip(((k.yr * R + k.yg * G + k.yb * B + (1 << 13)) >> 14) + k.yo, ylo, yhi);
            if (LAYOUT == SPEI_YUV_444) {
                U[p] = clip(((k.ur * R + k.ug * G + k.ub * B + (1 << 13)) >> 14) + mid, clo, chi);
                V[p] = clip(((k.vr * R + k.vg * G + k.vb * B + (1 << 13)) >> 14) + mid, clo, chi);
            }
        }
        const bool wide = al_y && x0 + 4 <= W;
        store4(dst + (int64_t)y * W, x0, W, wide, Y);
        if (LAYOUT == SPEI_YUV_444) {
            store4(dst + ysize + (int64_t)y * W, x0, W, wide, U);
            store4(dst + 2 * ysize + (int64_t)y * W, x0, W, wide, V);
        } else if (LAYOUT != SPEI_YUV_MONO && (!TWO || !((y >> fld) & 1)) && !(g & 1)) {
            // chroma samples (j, i0 .. i0 + 3) of rows y, y + 1 (4:2:2: of row y alone) and columns x0 .. x0 + 7: sm[ch][q] is the sum
            // over those rows of channel ch at column x0 - 1 + q, rows and columns clamped to the frame (q = 0 is the left neighbour
            // of LEFT and 4:2:2)
            const int j = TWO ? chroma_row(y >> fld >> 1, y, fld) : y, i0 = x0 >> 1;
            const uint16_t* r1 = src + (int64_t)next_row(y, H, fld) * W * 3;
            int sm[3][9];
            if (al_src && x0 + 8 <= W) {
                int a[12], b[12] = {};
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    load_rgb4(r0, x0 + 4 * h, W, true, D, a);
                    if (TWO) load_rgb4(r1, x0 + 4 * h, W, true, D, b);
#pragma unroll
                    for (int t = 0; t < 12; ++t) sm[t % 3][1 + 4 * h + t / 3] = a[t] + b[t];
                }
                const int xl = max(x0 - 1, 0) * 3;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    sm[ch][0] = LAYOUT == SPEI_YUV_420_CENTER ? 0 : min((int)r0[xl + ch], D) + (TWO ? min((int)r1[xl + ch], D) : 0);
            } else {
#pragma unroll
                for (int q = 0; q < 9; ++q) {
                    const int x = clip(x0 - 1 + q, 0, W - 1) * 3;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) sm[ch][q] = min((int)r0[x + ch], D) + (TWO ? min((int)r1[x + ch], D) : 0);
                }
            }
            int Uc[4], Vc[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                int S[3];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    S[ch] = LAYOUT == SPEI_YUV_420_CENTER ? sm[ch][1 + 2 * m] + sm[ch][2 + 2 * m]
                                                          : sm[ch][2 * m] + 2 * sm[ch][1 + 2 * m] + sm[ch][2 + 2 * m];
                constexpr int SH = LAYOUT == SPEI_YUV_420_LEFT ? 17 : 16;     // Q14 and the sum's 4 (CENTER, 4:2:2) or 8 (LEFT) weights
                Uc[m] = clip(((k.ur * S[0] + k.ug * S[1] + k.ub * S[2] + (1 << (SH - 1))) >> SH) + mid, clo, chi);
                Vc[m] = clip(((k.vr * S[0] + k.vg * S[1] + k.vb * S[2] + (1 << (SH - 1))) >> SH) + mid, clo, chi);
            }
            uint16_t* uo = dst + ysize + (int64_t)j * Wc;
            const bool cwide = al_c && i0 + 4 <= Wc;
            store4(uo, i0, Wc, cwide, Uc);
            store4(uo + csize, i0, Wc, cwide, Vc);
        }
    }
}

inline int grid_for(int64_t total) { return (int)((total + 255) / 256 < BLOCKS_MAX ? (total + 255) / 256 : BLOCKS_MAX); }

inline int64_t planar_bytes(int H, int W, int layout) { return (int64_t)H * W + 2 * chroma_size(H, W, layout); }

// spei_yuv_* take the layouts lo .. hi = SPEI_YUV_420_CENTER .. SPEI_YUV_444, spei_planar_* SPEI_YUV_422 .. SPEI_YUV_MONO
inline bool known(int layout, int lo, int hi, int matrix, int range) {
    return layout >= lo && layout <= hi && (matrix == SPEI_YUV_BT601 || matrix == SPEI_YUV_BT709) &&
           (range == SPEI_YUV_FULL || range == SPEI_YUV_LIMITED);
}

// `fields` of a call: 0 converts a progressive frame, 1 the woven fields of an interlaced one.  Only 4:2:0 has rows that depend on one
// another, so only there do the kernels walk fields (fld = 1), and a field must have whole chroma rows: H % 4 == 0.  The other layouts
// convert every row on its own: their fields are their rows, fld = 0
inline int check_fields(const char* name, int fields, int layout, int H) {
    SPEI_REQUIRE(!fields || layout > SPEI_YUV_420_LEFT || (H & 3) == 0, "%s: the fields of a 4:2:0 frame of H = %d rows have no whole "
                 "chroma rows (H must be a multiple of 4: H / 2 rows per field, H / 4 chroma rows)", name, H);
    return 0;
}
inline int field_pitch(int fields, int layout) { return fields && layout <= SPEI_YUV_420_LEFT ? 1 : 0; }

inline Coef deep_coef(int depth, int matrix, int range) {
    return range == SPEI_YUV_FULL ? COEF[matrix][0] : COEF_DEEP[depth == 12][matrix];
}

// one launch of KERNEL<layout> on `grid`, `block` and `stream` of the calling body; the layout is a checked one
#define SPEI_YUV_LAUNCH_AS(KERNEL, L, ...) hipLaunchKernelGGL(KERNEL<L>, grid, block, 0, (hipStream_t)stream, __VA_ARGS__)
#define SPEI_YUV_LAUNCH(KERNEL, layout, ...)                                                 \
    switch (layout) {                                                                       \
        case SPEI_YUV_420_CENTER: SPEI_YUV_LAUNCH_AS(KERNEL, SPEI_YUV_420_CENTER, __VA_ARGS__); break; \
        case SPEI_YUV_420_LEFT: SPEI_YUV_LAUNCH_AS(KERNEL, SPEI_YUV_420_LEFT, __VA_ARGS__); break;     \
        case SPEI_YUV_444: SPEI_YUV_LAUNCH_AS(KERNEL, SPEI_YUV_444, __VA_ARGS__); break;               \
        case SPEI_YUV_422: SPEI_YUV_LAUNCH_AS(KERNEL, SPEI_YUV_422, __VA_ARGS__); break;               \
        default: SPEI_YUV_LAUNCH_AS(KERNEL, SPEI_YUV_MONO, __VA_ARGS__); break;                        \
    }

// The bodies of the entry points: `name` is the entry's, lo .. hi the layouts it takes.
int to_rgb_u8(const char* name, int lo, int hi, const unsigned char* src, int64_t frame_stride, unsigned char* dst, int N, int H, int W,
              int layout, int matrix, int range, int fields, spei_stream_t stream) {
    SPEI_REQUIRE(src && dst, "%s: null pointer", name);
    SPEI_REQUIRE(N >= 1 && H >= 1 && W >= 1 && (int64_t)H * W * 3 < (1ll << 31), "%s: bad frame shape %d x %dx%d", name, N, H, W);
    SPEI_REQUIRE(known(layout, lo, hi, matrix, range), "%s: unknown layout %d, matrix %d or range %d (SPEI_YUV_*)", name, layout, matrix,
                 range);
    if (check_fields(name, fields, layout, H)) return -1;
    const int fld = field_pitch(fields, layout);
    SPEI_REQUIRE(N == 1 || frame_stride >= planar_bytes(H, W, layout), "%s: frame stride %lld < one %dx%d planar frame of %lld bytes", name,
                 (long long)frame_stride, H, W, (long long)planar_bytes(H, W, layout));
    const int aligned = (((uintptr_t)src | (uintptr_t)dst) & 3) == 0 && (N == 1 || (frame_stride & 3) == 0) && (W & 3) == 0;
    const int64_t total = (int64_t)N * H * ((W + 3) / 4);
    const Coef k = COEF[matrix][range];
    const dim3 grid(grid_for(total)), block(256);
    SPEI_YUV_LAUNCH(yuv_to_rgb_kernel, layout, src, frame_stride, dst, H, W, total, k, aligned, fld);
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

int from_rgb_u8(const char* name, int lo, int hi, const unsigned char* src, unsigned char* dst, int H, int W, int layout, int matrix,
                int range, int fields, spei_stream_t stream) {
    SPEI_REQUIRE(src && dst, "%s: null pointer", name);
    SPEI_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W * 3 < (1ll << 31), "%s: bad frame shape %dx%d", name, H, W);
    SPEI_REQUIRE(known(layout, lo, hi, matrix, range), "%s: unknown layout %d, matrix %d or range %d (SPEI_YUV_*)", name, layout, matrix,
                 range);
    if (check_fields(name, fields, layout, H)) return -1;
    const int fld = field_pitch(fields, layout);
    // rows of 3 W, W and ceil(W/2) bytes: 4-byte aligned when W % 4 == 0 (RGB, Y, and the 4:4:4 planes at H W and 2 H W) and, for
    // the 4:2:0 and 4:2:2 chroma planes, when W % 8 == 0
    const int al_src = ((uintptr_t)src & 3) == 0 && (W & 3) == 0;
    const int al_y = ((uintptr_t)dst & 3) == 0 && (W & 3) == 0;
    const int al_c = ((uintptr_t)dst & 3) == 0 && (W & 7) == 0;
    const int64_t total = (int64_t)H * ((W + 3) / 4);
    const Coef k = COEF[matrix][range];
    const int limited = range == SPEI_YUV_LIMITED;
    const dim3 grid(grid_for(total)), block(256);
    SPEI_YUV_LAUNCH(rgb_to_yuv_kernel, layout, src, dst, H, W, total, k, limited, al_src, al_y, al_c, fld);
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

int to_rgb_u16(const char* name, int lo, int hi, const uint16_t* src, int64_t frame_stride, uint16_t* dst, int N, int H, int W, int layout,
               int matrix, int range, int depth, int fields, spei_stream_t stream) {
    SPEI_REQUIRE(src && dst, "%s: null pointer", name);
    SPEI_REQUIRE(N >= 1 && H >= 1 && W >= 1 && (int64_t)H * W * 3 < (1ll << 31), "%s: bad frame shape %d x %dx%d", name, N, H, W);
    SPEI_REQUIRE(known(layout, lo, hi, matrix, range), "%s: unknown layout %d, matrix %d or range %d (SPEI_YUV_*)", name, layout, matrix,
                 range);
    if (check_fields(name, fields, layout, H)) return -1;
    const int fld = field_pitch(fields, layout);
    SPEI_REQUIRE(depth == 10 || depth == 12, "%s: unknown depth %d (10 or 12)", name, depth);
    SPEI_REQUIRE(N == 1 || frame_stride >= 2 * planar_bytes(H, W, layout), "%s: frame stride %lld < one %dx%d planar frame of %lld bytes",
                 name, (long long)frame_stride, H, W, (long long)(2 * planar_bytes(H, W, layout)));
    SPEI_REQUIRE(N == 1 || (frame_stride & 1) == 0, "%s: odd frame stride %lld (bytes, a multiple of 2)", name, (long long)frame_stride);
    SPEI_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 1) == 0, "%s: src and dst must be 2-byte aligned", name);
    const int aligned = (((uintptr_t)src | (uintptr_t)dst) & 7) == 0 && (N == 1 || (frame_stride & 7) == 0) && (W & 3) == 0;
    const int64_t total = (int64_t)N * H * ((W + 3) / 4), fstride = N == 1 ? 0 : frame_stride / 2;
    const Coef k = deep_coef(depth, matrix, range);
    const int s = depth - 8;
    const dim3 grid(grid_for(total)), block(256);
    SPEI_YUV_LAUNCH(yuv_to_rgb_u16_kernel, layout, src, fstride, dst, H, W, total, k, s, aligned, fld);
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

int from_rgb_u16(const char* name, int lo, int hi, const uint16_t* src, uint16_t* dst, int H, int W, int layout, int matrix, int range,
                 int depth, int fields, spei_stream_t stream) {
    SPEI_REQUIRE(src && dst, "%s: null pointer", name);
    SPEI_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W * 3 < (1ll << 31), "%s: bad frame shape %dx%d", name, H, W);
    SPEI_REQUIRE(known(layout, lo, hi, matrix, range), "%s: unknown layout %d, matrix %d or range %d (SPEI_YUV_*)", name, layout, matrix,
                 range);
    if (check_fields(name, fields, layout, H)) return -1;
    const int fld = field_pitch(fields, layout);
    SPEI_REQUIRE(depth == 10 || depth == 12, "%s: unknown depth %d (10 or 12)", name, depth);
    SPEI_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 1) == 0, "%s: src and dst must be 2-byte aligned", name);
    // rows of 6 W, 2 W and 2 ceil(W/2) bytes: 8-byte aligned when W % 4 == 0 (RGB, Y, and the 4:4:4 planes) and, for the 4:2:0 and
    // 4:2:2 chroma planes, when W % 8 == 0
    const int al_src = ((uintptr_t)src & 7) == 0 && (W & 3) == 0;
    const int al_y = ((uintptr_t)dst & 7) == 0 && (W & 3) == 0;
    const int al_c = ((uintptr_t)dst & 7) == 0 && (W & 7) == 0;
    const int64_t total = (int64_t)H * ((W + 3) / 4);
    const Coef k = deep_coef(depth, matrix, range);
    const int limited = range == SPEI_YUV_LIMITED, s = depth - 8;
    const dim3 grid(grid_for(total)), block(256);
    SPEI_YUV_LAUNCH(rgb_u16_to_yuv_kernel, layout, src, dst, H, W, total, k, limited, s, al_src, al_y, al_c, fld);
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

}  // namespace

extern "C" int spei_yuv_to_rgb_u8(const unsigned char* src, int64_t frame_stride, unsigned char* dst, int N, int H, int W, int layout,
                                  int matrix, int range, spei_stream_t stream) {
    return to_rgb_u8("spei_yuv_to_rgb_u8", SPEI_YUV_420_CENTER, SPEI_YUV_444, src, frame_stride, dst, N, H, W, layout, matrix, range, 0, stream);
}

extern "C" int spei_rgb_u8_to_yuv(const unsigned char* src, unsigned char* dst, int H, int W, int layout, int matrix, int range,
                                  spei_stream_t stream) {
    return from_rgb_u8("spei_rgb_u8_to_yuv", SPEI_YUV_420_CENTER, SPEI_YUV_444, src, dst, H, W, layout, matrix, range, 0, stream);
}

extern "C" int spei_yuv_to_rgb_u16(const uint16_t* src, int64_t frame_stride, uint16_t* dst, int N, int H, int W, int layout, int matrix,
                                   int range, int depth, spei_stream_t stream) {
    return to_rgb_u16("spei_yuv_to_rgb_u16", SPEI_YUV_420_CENTER, SPEI_YUV_444, src, frame_stride, dst, N, H, W, layout, matrix, range,
                      depth, 0, stream);
}

extern "C" int spei_rgb_u16_to_yuv(const uint16_t* src, uint16_t* dst, int H, int W, int layout, int matrix, int range, int depth,
                                   spei_stream_t stream) {
    return from_rgb_u16("spei_rgb_u16_to_yuv", SPEI_YUV_420_CENTER, SPEI_YUV_444, src, dst, H, W, layout, matrix, range, depth, 0, stream);
}

// ---- 4:2:2 and mono: the same four bodies on SPEI_YUV_422 and SPEI_YUV_MONO ------------------------------------------------------
extern "C" int spei_planar_to_rgb_u8(const unsigned char* src, int64_t frame_stride, unsigned char* dst, int N, int H, int W, int layout,
                                     int matrix, int range, spei_stream_t stream) {
    return to_rgb_u8("spei_planar_to_rgb_u8", SPEI_YUV_422, SPEI_YUV_MONO, src, frame_stride, dst, N, H, W, layout, matrix, range, 0, stream);
}

extern "C" int spei_rgb_u8_to_planar(const unsigned char* src, unsigned char* dst, int H, int W, int layout, int matrix, int range,
                                     spei_stream_t stream) {
    return from_rgb_u8("spei_rgb_u8_to_planar", SPEI_YUV_422, SPEI_YUV_MONO, src, dst, H, W, layout, matrix, range, 0, stream);
}

extern "C" int spei_planar_to_rgb_u16(const uint16_t* src, int64_t frame_stride, uint16_t* dst, int N, int H, int W, int layout, int matrix,
                                      int range, int depth, spei_stream_t stream) {
    return to_rgb_u16("spei_planar_to_rgb_u16", SPEI_YUV_422, SPEI_YUV_MONO, src, frame_stride, dst, N, H, W, layout, matrix, range, depth,
                      0, stream);
}

extern "C" int spei_rgb_u16_to_planar(const uint16_t* src, uint16_t* dst, int H, int W, int layout, int matrix, int range, int depth,
                                      spei_stream_t stream) {
    return from_rgb_u16("spei_rgb_u16_to_planar", SPEI_YUV_422, SPEI_YUV_MONO, src, dst, H, W, layout, matrix, range, depth, 0, stream);
}

// ---- interlaced frames: the same four bodies on the woven fields, every layout ---------------------------------------------------
// Field p of the result is the conversion above of field p's own planar picture (Y rows p :: 2 and, for 4:2:0, chroma-plane rows
// p :: 2); 4:4:4, 4:2:2 and mono convert row by row, so there the result is the progressive one.
extern "C" int spei_yuv_fields_to_rgb_u8(const unsigned char* src, int64_t frame_stride, unsigned char* dst, int N, int H, int W,
                                         int layout, int matrix, int range, spei_stream_t stream) {
    return to_rgb_u8("spei_yuv_fields_to_rgb_u8", SPEI_YUV_420_CENTER, SPEI_YUV_MONO, src, frame_stride, dst, N, H, W, layout, matrix, range,
                     1, stream);
}

extern "C" int spei_rgb_u8_to_yuv_fields(const unsigned char* src, unsigned char* dst, int H, int W, int layout, int matrix, int range,
                                         spei_stream_t stream) {
    return from_rgb_u8("spei_rgb_u8_to_yuv_fields", SPEI_YUV_420_CENTER, SPEI_YUV_MONO, src, dst, H, W, layout, matrix, range, 1, stream);
}

extern "C" int spei_yuv_fields_to_rgb_u16(const uint16_t* src, int64_t frame_stride, uint16_t* dst, int N, int H, int W, int layout,
                                          int matrix, int range, int depth, spei_stream_t stream) {
    return to_rgb_u16("spei_yuv_fields_to_rgb_u16", SPEI_YUV_420_CENTER, SPEI_YUV_MONO, src, frame_stride, dst, N, H, W, layout, matrix,
                      range, depth, 1, stream);
}

extern "C" int spei_rgb_u16_to_yuv_fields(const uint16_t* src, uint16_t* dst, int H, int W, int layout, int matrix, int range, int depth,
                                          spei_stream_t stream) {
    return from_rgb_u16("spei_rgb_u16_to_yuv_fields", SPEI_YUV_420_CENTER, SPEI_YUV_MONO, src, dst, H, W, layout, matrix, range, depth, 1,
                        stream);
}
