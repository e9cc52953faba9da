// Planar YUV frames of the clip API (speinet_amd/y4m.py, speinet_amd/video.py): the payload of a YUV4MPEG2 FRAME in, one out.  An
// extension beyond the reference, which reads and writes image files only.
//
//   spei_yuv_to_rgb_u8 — N planar uint8 frames (Y [H][W], then U, then V: [ceil(H/2)][ceil(W/2)] each for 4:2:0, [H][W] each for
//                        4:4:4) -> N packed uint8 [H][W][3] RGB frames, what spei_frames_u8_in and spei_frame_pair_stats take.
//   spei_rgb_u8_to_yuv — one packed uint8 [H][W][3] RGB frame (what spei_frame_u8_out makes) -> one planar frame.
//
// Integer arithmetic only: the result is defined bit for bit and depends on neither the launch shape nor the access path.  `>>` is
// an arithmetic shift (it floors).  Clipping is to [0,255] for RGB and full range, to [16,235] (Y) and [16,240] (U, V) for limited.
//
// YUV -> RGB.  The chroma of a full-resolution pixel is formed times 16 (U16, V16), neighbour indices clamped to the plane:
//   4:4:4          U16 = 16 U[y][x]
//   4:2:0 rows     j = y >> 1, the other row j - 1 (y even) or j + 1 (y odd), weights 3 : 1 (both sitings)
//   CENTER columns the same rule with i = x >> 1
//   LEFT columns   4 : 0 at even x (co-sited), 2 : 2 of columns i and i + 1 at odd x
// then, with yy = cy * 16 * (Y - yo), u = U16 - 2048, v = V16 - 2048:
//   R = clip((yy + rv v + 2^17) >> 18)   G = clip((yy + gu u + gv v + 2^17) >> 18)   B = clip((yy + bu u + 2^17) >> 18)
// Every intermediate fits int32 (about 1.5e8 at most).
//
// RGB -> YUV.  Y = clip(((yr R + yg G + yb B + 2^13) >> 14) + yo) per pixel.  Chroma:
//   4:4:4   U = clip(((ur R + ug G + ub B + 2^13) >> 14) + 128) per pixel, V likewise
//   CENTER  the same on S_c, the sum of channel c over rows 2j, 2j + 1 and columns 2i, 2i + 1, with 2^15 and >> 16
//   LEFT    the same on the sum over rows 2j, 2j + 1 of c[2i - 1] + 2 c[2i] + c[2i + 1], with 2^16 and >> 17
// indices clamped to the frame.  The 4:2:0 resampling (3 : 1 bilinear up, box or [1 2 1] down) is this project's own definition.
//
// Streaming kernels in the style of frame_io.hip, one thread per group of 4 pixels of a row in a grid-stride loop: dword accesses
// where the rows are 4-byte aligned, bytes otherwise and at the right edge.  In spei_rgb_u8_to_yuv the thread of an even row and an
// even group also makes the (up to) 4 chroma samples of the 2 x 8 pixels below and right of it; the RGB bytes it reads again for
// that are its neighbours' and come from the cache.  No atomics.  HBM-bound: a 720p 4:2:0 frame is 1.4 MB on one side and 2.8 MB on
// the other.
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

template <int LAYOUT>
__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(const unsigned char* __restrict__ src, int64_t fstride,
                                                         unsigned char* __restrict__ dst, int H, int W, int64_t total, Coef k,
                                                         int aligned) {
    const int gw = (W + 3) >> 2, Hc = (H + 1) >> 1, Wc = (W + 1) >> 1;
    const int64_t ysize = (int64_t)H * W, csize = LAYOUT == SPEI_YUV_444 ? ysize : (int64_t)Hc * Wc;
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
        } else {
            // chroma columns i0 - 1 .. i0 + 2 (clamped) serve the 4 pixels; rows first: 3 of row j, 1 of the other
            const int j = y >> 1, jo = clip((y & 1) ? j + 1 : j - 1, 0, Hc - 1), i0 = x0 >> 1;
            const int64_t rj = (int64_t)j * Wc, ro = (int64_t)jo * Wc;
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
                                                         int W, int64_t total, Coef k, int limited, int al_src, int al_y, int al_c) {
    const int gw = (W + 3) >> 2, Hc = (H + 1) >> 1, Wc = (W + 1) >> 1;
    const int64_t ysize = (int64_t)H * W, csize = LAYOUT == SPEI_YUV_444 ? ysize : (int64_t)Hc * Wc;
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
        } else if (!(y & 1) && !(g & 1)) {
            // chroma samples (j, i0 .. i0 + 3) of rows y, y + 1 and columns x0 .. x0 + 7: s[ch][q] is the sum over the two rows of
            // channel ch at column x0 - 1 + q, rows and columns clamped to the frame (q = 0 is LEFT's left neighbour)
            const int j = y >> 1, i0 = x0 >> 1;
            const unsigned char* r1 = src + (int64_t)min(y + 1, H - 1) * W * 3;
            int s[3][9];
            if (al_src && x0 + 8 <= W) {
                const uint32_t* a = reinterpret_cast<const uint32_t*>(r0 + x0 * 3);
                const uint32_t* b = reinterpret_cast<const uint32_t*>(r1 + x0 * 3);
#pragma unroll
                for (int d = 0; d < 6; ++d) {
                    const uint32_t wa = a[d], wb = b[d];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int t = 4 * d + e;
                        s[t % 3][1 + t / 3] = byte_at(wa, e) + byte_at(wb, e);
                    }
                }
                const int xl = max(x0 - 1, 0) * 3;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) s[ch][0] = LAYOUT == SPEI_YUV_420_LEFT ? r0[xl + ch] + r1[xl + ch] : 0;
            } else {
#pragma unroll
                for (int q = 0; q < 9; ++q) {
                    const int x = clip(x0 - 1 + q, 0, W - 1) * 3;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) s[ch][q] = r0[x + ch] + r1[x + ch];
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
                constexpr int SH = LAYOUT == SPEI_YUV_420_CENTER ? 16 : 17;
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

inline int grid_for(int64_t total) { return (int)((total + 255) / 256 < BLOCKS_MAX ? (total + 255) / 256 : BLOCKS_MAX); }

inline int64_t planar_bytes(int H, int W, int layout) {
    const int64_t c = layout == SPEI_YUV_444 ? (int64_t)H * W : (int64_t)((H + 1) / 2) * ((W + 1) / 2);
    return (int64_t)H * W + 2 * c;
}

inline bool known(int layout, int matrix, int range) {
    return (layout == SPEI_YUV_420_CENTER || layout == SPEI_YUV_420_LEFT || layout == SPEI_YUV_444) &&
           (matrix == SPEI_YUV_BT601 || matrix == SPEI_YUV_BT709) && (range == SPEI_YUV_FULL || range == SPEI_YUV_LIMITED);
}

}  // namespace

extern "C" int spei_yuv_to_rgb_u8(const unsigned char* src, int64_t frame_stride, unsigned char* dst, int N, int H, int W, int layout,
                                  int matrix, int range, spei_stream_t stream) {
    SPEI_REQUIRE(src && dst, "spei_yuv_to_rgb_u8: null pointer");
    SPEI_REQUIRE(N >= 1 && H >= 1 && W >= 1 && (int64_t)H * W * 3 < (1ll << 31), "spei_yuv_to_rgb_u8: bad frame shape %d x %dx%d", N, H, W);
    SPEI_REQUIRE(known(layout, matrix, range), "spei_yuv_to_rgb_u8: unknown layout %d, matrix %d or range %d (SPEI_YUV_*)", layout, matrix,
                 range);
    SPEI_REQUIRE(N == 1 || frame_stride >= planar_bytes(H, W, layout), "spei_yuv_to_rgb_u8: frame stride %lld < one %dx%d planar frame "
                 "of %lld bytes", (long long)frame_stride, H, W, (long long)planar_bytes(H, W, layout));
    const int aligned = (((uintptr_t)src | (uintptr_t)dst) & 3) == 0 && (N == 1 || (frame_stride & 3) == 0) && (W & 3) == 0;
    const int64_t total = (int64_t)N * H * ((W + 3) / 4);
    const Coef k = COEF[matrix][range];
    const dim3 grid(grid_for(total)), block(256);
    if (layout == SPEI_YUV_420_CENTER)
        hipLaunchKernelGGL(yuv_to_rgb_kernel<SPEI_YUV_420_CENTER>, grid, block, 0, (hipStream_t)stream, src, frame_stride, dst, H, W, total,
                           k, aligned);
    else if (layout == SPEI_YUV_420_LEFT)
        hipLaunchKernelGGL(yuv_to_rgb_kernel<SPEI_YUV_420_LEFT>, grid, block, 0, (hipStream_t)stream, src, frame_stride, dst, H, W, total, k,
                           aligned);
    else
        hipLaunchKernelGGL(yuv_to_rgb_kernel<SPEI_YUV_444>, grid, block, 0, (hipStream_t)stream, src, frame_stride, dst, H, W, total, k,
                           aligned);
    SPEI_CHECK_LAUNCH("spei_yuv_to_rgb_u8");
    return 0;
}

extern "C" int spei_rgb_u8_to_yuv(const unsigned char* src, unsigned char* dst, int H, int W, int layout, int matrix, int range,
                                  spei_stream_t stream) {
    SPEI_REQUIRE(src && dst, "spei_rgb_u8_to_yuv: null pointer");
    SPEI_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W * 3 < (1ll << 31), "spei_rgb_u8_to_yuv: bad frame shape %dx%d", H, W);
    SPEI_REQUIRE(known(layout, matrix, range), "spei_rgb_u8_to_yuv: unknown layout %d, matrix %d or range %d (SPEI_YUV_*)", layout, matrix,
                 range);
    // rows of 3 W, W and ceil(W/2) bytes: 4-byte aligned when W % 4 == 0 (RGB, Y, and the 4:4:4 planes at H W and 2 H W) and, for
    // the 4:2:0 chroma planes, when W % 8 == 0
    const int al_src = ((uintptr_t)src & 3) == 0 && (W & 3) == 0;
    const int al_y = ((uintptr_t)dst & 3) == 0 && (W & 3) == 0;
    const int al_c = ((uintptr_t)dst & 3) == 0 && (W & 7) == 0;
    const int64_t total = (int64_t)H * ((W + 3) / 4);
    const Coef k = COEF[matrix][range];
    const int limited = range == SPEI_YUV_LIMITED;
    const dim3 grid(grid_for(total)), block(256);
    if (layout == SPEI_YUV_420_CENTER)
        hipLaunchKernelGGL(rgb_to_yuv_kernel<SPEI_YUV_420_CENTER>, grid, block, 0, (hipStream_t)stream, src, dst, H, W, total, k, limited,
                           al_src, al_y, al_c);
    else if (layout == SPEI_YUV_420_LEFT)
        hipLaunchKernelGGL(rgb_to_yuv_kernel<SPEI_YUV_420_LEFT>, grid, block, 0, (hipStream_t)stream, src, dst, H, W, total, k, limited,
                           al_src, al_y, al_c);
    else
        hipLaunchKernelGGL(rgb_to_yuv_kernel<SPEI_YUV_444>, grid, block, 0, (hipStream_t)stream, src, dst, H, W, total, k, limited, al_src,
                           al_y, al_c);
    SPEI_CHECK_LAUNCH("spei_rgb_u8_to_yuv");
    return 0;
}
