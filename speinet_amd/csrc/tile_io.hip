// Tile I/O of the clip API's large-frame mode (speinet_amd/tiles.py, video.deblur_clip(..., tiles=)): a frame is deblurred as a grid
// of rows x cols overlapping tiles of ONE shape, stitched with hard seams, as the reference's forward_chop does for 2x2
// (inference_SPEINet.py:545-607).
//
//   spei_tiles_u8_in / spei_tiles_u16_in   — one packed [H][W][3] frame -> every tile's fp32 [3][thp][twp] planes, tile k = i * cols + j
//                        at dst + k * tile_stride: bit-identical to spei_frames_u8_in / spei_frames_u16_in (frame_io.hip) on the packed
//                        crop [y0[i], y0[i] + th) x [x0[j], x0[j] + tw), its reflect pad to thp x twp included.  One launch per frame.
//   spei_tiles_u8_out / spei_tiles_u16_out — rows * cols fp32 [3][thp][twp] tiles -> one packed [H][W][3] frame: pixel (y, x) of band
//                        [yb[i], yb[i+1]) x [xb[j], xb[j+1]) comes from tile (i, j) with spei_frame_u8_out / spei_frame_u16_out's
//                        rounding; the flag is set by OWNED pixels only, a tile's margin is never read.  One launch per frame.
//   spei_tiles_u8_blend / spei_tiles_u16_blend — the same with feathered seams (the definition is in include/speinet_hip.h): around
//                        every inner seam a ramp of up to 2 * feather pixels blends the two tiles that computed it, four where a row
//                        and a column ramp cross; every other pixel is the hard stitch's, bit for bit.  One launch per frame.
//
// The tables (at most 8 origins and 9 band bounds per axis, 64 tile pointers) are read from host memory at call time and travel to the
// kernel by value, in its arguments.  Streaming kernels on the pixel group of pixel_group.h, whose ingest, rounding and store they
// share with frame_io.hip.  Tile origins are arbitrary, so the ingest decides per row whether its source is aligned, and the egress
// per group whether its four pixels are one aligned run of one tile.
#include "pixel_group.h"

namespace {

constexpr int GRID_MAX = 8;                                // rows, cols

struct InTab { int y0[GRID_MAX], x0[GRID_MAX]; };
struct OutTab {
    const float* tile[GRID_MAX * GRID_MAX];
    int y0[GRID_MAX], x0[GRID_MAX], yb[GRID_MAX + 1], xb[GRID_MAX + 1];
};

// T = unsigned char (D = 255, inv = INV255) or uint16_t (D = 2^depth - 1, inv = (float)(1.0 / D); a word above D reads as D)
template <typename T>
__global__ __launch_bounds__(256) void tiles_in_kernel(const T* __restrict__ src, int W, float* __restrict__ dst, int64_t tstride,
                                                       InTab tab, int cols, int th, int tw, int thp, int twp, int64_t total, int D,
                                                       float inv) {
    const int gw = twp >> 2;                               // groups per padded row (twp % 20 == 0)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / gw;                        // k * thp + y
        const int x = (int)(i - row * gw) * 4;
        const int k = (int)(row / thp), y = (int)(row - (int64_t)k * thp);
        const int ti = k / cols, tj = k - ti * cols;
        const int sy = y < th ? y : 2 * th - 2 - y;        // padded row th + j reads row th - 2 - j of the tile
        const T* s = src + ((int64_t)(tab.y0[ti] + sy) * W + tab.x0[tj]) * 3;
        float v[3][4];
        ingest_group(s, x, tw, ((uintptr_t)s & GROUP_MASK<T>) == 0, D, v);     // spei_frames_u8_in's values of the tile's row
        float* d = dst + k * tstride + (int64_t)y * twp + x;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            *reinterpret_cast<float4*>(d + (int64_t)c * thp * twp) = make_float4(v[c][0] * inv, v[c][1] * inv, v[c][2] * inv, v[c][3] * inv);
    }
}

// the band of coordinate p: the number of inner bounds b[1 .. n-1] at or below it
__device__ __forceinline__ int band_of(const int (&b)[GRID_MAX + 1], int n, int p) {
    int r = 0;
#pragma unroll
    for (int i = 1; i < GRID_MAX; ++i) r += (i < n && p >= b[i]) ? 1 : 0;
    return r;
}

// the hard stitch of one group: pixels x .. x + 3 of row y, which lies in row band bi and whose first pixel lies in column band bj
// -> their samples q[channel][pixel] from the tiles that own them, spei_frame_u8_out's values; returns nonzero iff one was not finite
__device__ __forceinline__ int hard_stitch(const OutTab& tab, int y, int x, int bi, int bj, int W, int cols, int twp, int64_t plane,
                                           float Df, uint32_t (&q)[3][4]) {
    const int ry = y - tab.y0[bi];
    const float* t = tab.tile[bi * cols + bj];
    const int rx = x - tab.x0[bj];
    if (x + 4 <= W && band_of(tab.xb, cols, x + 3) == bj && (rx & 3) == 0 && ((uintptr_t)t & 15) == 0)
        return quantise_planes(t + (int64_t)ry * twp + rx, plane, Df, 4, q);     // four owned pixels of one tile, 16-byte aligned there
    int bad = 0;                                           // a seam inside the group, an odd tile column or the frame's right edge
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int xx = x + k;
        const int j = band_of(tab.xb, cols, xx);           // xx >= W: the last band, never read
        const float* s = tab.tile[bi * cols + j] + (int64_t)ry * twp + (xx - tab.x0[j]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = xx < W ? s[c * plane] : 0.0f;
            q[c][k] = quantise(v, Df);
            bad |= isfinite(v) ? 0 : 1;
        }
    }
    return bad;
}

// T = unsigned char (Df = 255) or uint16_t (Df = 2^depth - 1)
template <typename T>
__global__ __launch_bounds__(256) void tiles_out_kernel(OutTab tab, T* __restrict__ dst, int* __restrict__ nonfinite, int W, int rows,
                                                        int cols, int twp, int64_t plane, int gw, int64_t total, int vec_out, float Df) {
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / gw), x = (int)(i - (int64_t)y * gw) * 4;
        uint32_t q[3][4];
        bad |= hard_stitch(tab, y, x, band_of(tab.yb, rows, y), band_of(tab.xb, cols, x), W, cols, twp, plane, Df, q);
        store_group(dst + ((int64_t)y * W + x) * 3, q, vec_out != 0, W - x);
    }
    if (nonfinite && bad) atomicOr(nonfinite, 1);           // rare: one atomic per thread that met a non-finite value
}

// ---- feathered seams ------------------------------------------------------------------------------------------------------------------
// OutTab and, per axis, the half-width f[s] of the ramp of inner seam s = 1 .. n-1 (0: a hard seam) and r[s] = (float)(1 / (4 f[s]))
struct BlendTab {
    OutTab t;
    int fy[GRID_MAX], fx[GRID_MAX];
    float ry[GRID_MAX], rx[GRID_MAX];
    // for the one test that sends a group to the ramp code: the ramps' starts b[s] - f[s], and their widths 2 f[s], the columns' plus
    // 3 for the group's own width; a width of 0 (a hard seam, no seam) matches nothing
    int ylo[GRID_MAX], yw[GRID_MAX], xlo[GRID_MAX], xw[GRID_MAX];
};

// does [p, p + ext] meet a ramp?  w[s] = 2 f[s] + ext, or 0.  Seven compares against wave-uniform operands, joined as lane masks
__device__ __forceinline__ bool meets_ramp(const int (&lo)[GRID_MAX], const int (&w)[GRID_MAX], int p_ext) {
    bool r = false;
#pragma unroll
    for (int s = 1; s < GRID_MAX; ++s) r |= (unsigned)(p_ext - lo[s]) < (unsigned)w[s];
    return r;
}

// the seam whose ramp [b[s] - f[s], b[s] + f[s]) holds coordinate p of band i, or 0: the ramps of an axis do not overlap
__device__ __forceinline__ int ramp_of(const int (&b)[GRID_MAX + 1], const int (&f)[GRID_MAX], int n, int i, int p) {
    if (i >= 1 && p < b[i] + f[i]) return i;
    if (i + 1 < n && p >= b[i + 1] - f[i + 1]) return i + 1;
    return 0;
}

// the weight of the high tile at coordinate p of the ramp of seam s: (2 (p - b[s] + f) + 1) / (4 f) with one float32 multiply
__device__ __forceinline__ float ramp_weight(int p, int b, int f, float r) { return (float)(2 * (p - b + f) + 1) * r; }

// tiles_out_kernel with ramps.  A group of four pixels whose row and columns meet no ramp (one test on wave-uniform operands, no table
// lookups: 94 % of the groups at 2160p 2x5) runs hard_stitch, as tiles_out_kernel does, and gives its values.  Of the others, a group
// that lies in one ramp and is aligned in both of its tiles (every ramp group of a plan whose seams and origins are multiples of 4, as
// at 1080p and 2160p) loads 16 bytes per plane from each contributing tile; only a ramp's odd ends go pixel by pixel.  Rows are
// uniform over (nearly) a wave, so a row ramp adds its loads to whole waves and a column ramp only to the groups it crosses.
template <typename T>
__global__ __launch_bounds__(256) void tiles_blend_kernel(BlendTab tab, T* __restrict__ dst, int* __restrict__ nonfinite, int W, int rows,
                                                          int cols, int twp, int64_t plane, int gw, int64_t total, int vec_out, float Df) {
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / gw), x = (int)(i - (int64_t)y * gw) * 4;
        const int bi = band_of(tab.t.yb, rows, y), bj = band_of(tab.t.xb, cols, x);
        uint32_t q[3][4];
        if (!meets_ramp(tab.ylo, tab.yw, y) && !meets_ramp(tab.xlo, tab.xw, x + 3)) {
            // the row in no row ramp, the four pixels in no column ramp: the hard stitch
            bad |= hard_stitch(tab.t, y, x, bi, bj, W, cols, twp, plane, Df, q);
        } else {
            const int sy = ramp_of(tab.t.yb, tab.fy, rows, bi, y);
            const int ilo = sy ? sy - 1 : bi, ihi = sy ? sy : bi;                  // the low and the high tile row (one row outside a ramp)
            const float wy = sy ? ramp_weight(y, tab.t.yb[sy], tab.fy[sy], tab.ry[sy]) : 0.0f;
            const int64_t olo = (int64_t)(y - tab.t.y0[ilo]) * twp, ohi = (int64_t)(y - tab.t.y0[ihi]) * twp;
            // the group as a whole: pixels x and x + 3 in one ramp, or in one band and in no ramp, say the same of the two between them
            // (a ramp is an interval, and a band's ramps are its two ends)
            const int j3 = band_of(tab.t.xb, cols, x + 3);
            const int gx = ramp_of(tab.t.xb, tab.fx, cols, bj, x);
            const int glo = gx ? gx - 1 : bj, ghi = gx ? gx : bj;                      // the low and the high tile column
            const int glc = x - tab.t.x0[glo], ghc = x - tab.t.x0[ghi];
            const float* ga = tab.t.tile[ilo * cols + glo];
            const float* gb = tab.t.tile[ilo * cols + ghi];
            const float* gc = tab.t.tile[ihi * cols + glo];
            const float* gd = tab.t.tile[ihi * cols + ghi];
            if (x + 4 <= W && gx == ramp_of(tab.t.xb, tab.fx, cols, j3, x + 3) && (gx || j3 == bj) && ((glc | ghc) & 3) == 0 &&
                (((uintptr_t)ga | (uintptr_t)gb | (uintptr_t)gc | (uintptr_t)gd) & 15) == 0) {
                // four pixels with the same tiles, 16-byte aligned in each.  No ramp: the hard stitch's loads and values.  A ramp: one
                // 16-byte load per plane and contributing tile, all of a plane's in flight before the first is used
                float wx[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) wx[k] = gx ? ramp_weight(x + k, tab.t.xb[gx], tab.fx[gx], tab.rx[gx]) : 0.0f;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float4 fa = *reinterpret_cast<const float4*>(ga + olo + glc + c * plane);
                    float4 fb = fa, fc = fa, fd = fa;
                    if (gx) fb = *reinterpret_cast<const float4*>(gb + olo + ghc + c * plane);
                    if (sy) {
                        fc = *reinterpret_cast<const float4*>(gc + ohi + glc + c * plane);
                        fd = fc;
                        if (gx) fd = *reinterpret_cast<const float4*>(gd + ohi + ghc + c * plane);
                    }
                    const float ea[4] = {fa.x, fa.y, fa.z, fa.w}, eb[4] = {fb.x, fb.y, fb.z, fb.w};
                    const float ec[4] = {fc.x, fc.y, fc.z, fc.w}, ed[4] = {fd.x, fd.y, fd.z, fd.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float v = ea[k];
                        bool fin = isfinite(v);
                        if (gx) {
                            fin = fin && isfinite(eb[k]);
                            v = fmaf(wx[k], eb[k] - v, v);
                        }
                        if (sy) {
                            float u = ec[k];
                            fin = fin && isfinite(u);
                            if (gx) {
                                fin = fin && isfinite(ed[k]);
                                u = fmaf(wx[k], ed[k] - u, u);
                            }
                            v = fmaf(wy, u - v, v);
                        }
                        q[c][k] = fin ? quantise(v, Df) : 0u;  // 0 if any contributing value is not finite
                        bad |= fin ? 0 : 1;
                    }
                }
            } else {                                       // a ramp's end or a seam inside the group, an odd tile column or the right edge
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int xx = x + k;
                    const int j = band_of(tab.t.xb, cols, xx);                         // xx >= W: the last band, never read
                    const int sx = xx < W ? ramp_of(tab.t.xb, tab.fx, cols, j, xx) : 0;
                    const int jlo = sx ? sx - 1 : j, jhi = sx ? sx : j;
                    const float wx = sx ? ramp_weight(xx, tab.t.xb[sx], tab.fx[sx], tab.rx[sx]) : 0.0f;
                    const int clo = xx - tab.t.x0[jlo], chi = xx - tab.t.x0[jhi];
                    const float* pa = tab.t.tile[ilo * cols + jlo] + olo + clo;    // (low row, low column): the owner outside every ramp
                    const float* pb = tab.t.tile[ilo * cols + jhi] + olo + chi;
                    const float* pc = tab.t.tile[ihi * cols + jlo] + ohi + clo;
                    const float* pd = tab.t.tile[ihi * cols + jhi] + ohi + chi;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        float v = 0.0f;
                        bool fin = true;
                        if (xx < W) {
                            v = pa[c * plane];
                            fin = isfinite(v);
                            if (sx) {
                                const float b = pb[c * plane];
                                fin = fin && isfinite(b);
                                v = fmaf(wx, b - v, v);
                            }
                            if (sy) {
                                float u = pc[c * plane];
                                fin = fin && isfinite(u);
                                if (sx) {
                                    const float d = pd[c * plane];
                                    fin = fin && isfinite(d);
                                    u = fmaf(wx, d - u, u);
                                }
                                v = fmaf(wy, u - v, v);
                            }
                        }
                        q[c][k] = fin ? quantise(v, Df) : 0u;  // 0 if any contributing value is not finite
                        bad |= fin ? 0 : 1;
                    }
                }
            }
        }
        store_group(dst + ((int64_t)y * W + x) * 3, q, vec_out != 0, W - x);
    }
    if (nonfinite && bad) atomicOr(nonfinite, 1);           // rare: one atomic per thread that met a non-finite value
}

// the half-width of inner seam s of an axis of r tiles of real length t (the rule of include/speinet_hip.h)
inline int seam_half(const int* o, const int* b, int r, int t, int s, int feather) {
    int f = feather;
    for (int k = s - 1; k <= s; ++k) {                     // [b - f, b + f) inside the real pixels [o, o + t) of the low and the high tile
        f = f < b[s] - o[k] ? f : b[s] - o[k];
        f = f < o[k] + t - b[s] ? f : o[k] + t - b[s];
    }
    // the two bands next to the seam: half of one with a seam on its other side as well, all of one at the frame's edge
    const int below = s > 1 ? (b[s] - b[s - 1]) / 2 : b[s] - b[s - 1], above = s + 1 < r ? (b[s + 1] - b[s]) / 2 : b[s + 1] - b[s];
    f = f < below ? f : below;
    f = f < above ? f : above;
    return f > 0 ? f : 0;
}

template <typename T>
int tiles_in(const char* name, const T* src, int H, int W, float* dst, int64_t tile_stride, const int* y0, const int* x0, int rows,
             int cols, int th, int tw, int depth, hipStream_t stream) {
    SPEI_REQUIRE(src && dst && y0 && x0, "%s: null pointer", name);
    SPEI_REQUIRE(H > 0 && W > 0 && (int64_t)H * W * 3 < (1ll << 31), "%s: bad frame shape %dx%d", name, H, W);
    SPEI_REQUIRE(rows >= 1 && rows <= GRID_MAX && cols >= 1 && cols <= GRID_MAX, "%s: a grid of %dx%d tiles (1..%d rows and columns)",
                 name, rows, cols, GRID_MAX);
    SPEI_REQUIRE(th > 0 && tw > 0 && th <= H && tw <= W, "%s: a %dx%d tile does not fit a %dx%d frame", name, th, tw, H, W);
    const int thp = (th + MULT - 1) / MULT * MULT, twp = (tw + MULT - 1) / MULT * MULT;
    SPEI_REQUIRE(thp - th < th && twp - tw < tw, "%s: a %dx%d tile cannot reflect-pad to %dx%d (the pad must be smaller than the tile)",
                 name, th, tw, thp, twp);
    SPEI_REQUIRE(sizeof(T) == 1 || depth == 10 || depth == 12, "%s: unknown depth %d (10 or 12)", name, depth);
    SPEI_REQUIRE(((uintptr_t)src & (sizeof(T) - 1)) == 0, "%s: src must be %d-byte aligned", name, (int)sizeof(T));
    SPEI_REQUIRE(((uintptr_t)dst & 15) == 0 && (tile_stride & 3) == 0, "%s: dst must be 16-byte aligned and the tile stride a multiple of "
                 "4 floats", name);
    SPEI_REQUIRE(tile_stride >= (int64_t)3 * thp * twp, "%s: tile stride %lld < one tile of 3x%dx%d floats", name, (long long)tile_stride,
                 thp, twp);
    InTab tab = {};
    for (int i = 0; i < rows; ++i) {
        SPEI_REQUIRE(y0[i] >= 0 && y0[i] <= H - th, "%s: tile row %d at y %d, %d rows, lies outside the %dx%d frame", name, i, y0[i], th, H, W);
        tab.y0[i] = y0[i];
    }
    for (int j = 0; j < cols; ++j) {
        SPEI_REQUIRE(x0[j] >= 0 && x0[j] <= W - tw, "%s: tile column %d at x %d, %d columns, lies outside the %dx%d frame", name, j, x0[j],
                     tw, H, W);
        tab.x0[j] = x0[j];
    }
    const int64_t total = (int64_t)rows * cols * thp * (twp / 4);
    const int D = sizeof(T) == 1 ? 255 : (1 << depth) - 1;
    hipLaunchKernelGGL(tiles_in_kernel<T>, dim3(grid_for(total)), dim3(256), 0, stream, src, W, dst, tile_stride, tab, cols, th, tw, thp,
                       twp, total, D, sizeof(T) == 1 ? INV255 : (float)(1.0 / D));
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

// what the hard and the feathered stitch share on the host: the checks of a call, and its tables as the kernels take them
template <typename T>
int out_table(const char* name, const float* const* tiles, const T* dst, int H, int W, const int* y0, const int* x0, const int* yb,
              const int* xb, int rows, int cols, int thp, int twp, int depth, OutTab& tab) {
    SPEI_REQUIRE(tiles && dst && y0 && x0 && yb && xb, "%s: null pointer", name);
    SPEI_REQUIRE(H > 0 && W > 0 && (int64_t)H * W * 3 < (1ll << 31), "%s: bad frame shape %dx%d", name, H, W);
    SPEI_REQUIRE(rows >= 1 && rows <= GRID_MAX && cols >= 1 && cols <= GRID_MAX, "%s: a grid of %dx%d tiles (1..%d rows and columns)",
                 name, rows, cols, GRID_MAX);
    SPEI_REQUIRE(thp > 0 && twp > 0 && (twp & 3) == 0 && (int64_t)thp * twp < (1ll << 30), "%s: bad tile planes %dx%d (the width a "
                 "multiple of 4)", name, thp, twp);
    SPEI_REQUIRE(sizeof(T) == 1 || depth == 10 || depth == 12, "%s: unknown depth %d (10 or 12)", name, depth);
    SPEI_REQUIRE(((uintptr_t)dst & (sizeof(T) - 1)) == 0, "%s: dst must be %d-byte aligned", name, (int)sizeof(T));
    SPEI_REQUIRE(yb[0] == 0 && yb[rows] == H && xb[0] == 0 && xb[cols] == W, "%s: the bands must span the %dx%d frame (rows %d..%d, "
                 "columns %d..%d)", name, H, W, yb[0], yb[rows], xb[0], xb[cols]);
    for (int i = 0; i < rows; ++i) {
        SPEI_REQUIRE(yb[i] < yb[i + 1], "%s: row band %d is empty or reversed (%d..%d)", name, i, yb[i], yb[i + 1]);
        SPEI_REQUIRE(y0[i] >= 0 && y0[i] < H, "%s: tile row %d at y %d lies outside the %dx%d frame", name, i, y0[i], H, W);
        SPEI_REQUIRE(y0[i] <= yb[i] && yb[i + 1] - y0[i] <= thp, "%s: row band %d (%d..%d) lies outside its tile (%d..%d)", name, i, yb[i],
                     yb[i + 1], y0[i], y0[i] + thp);
        tab.y0[i] = y0[i];
    }
    for (int j = 0; j < cols; ++j) {
        SPEI_REQUIRE(xb[j] < xb[j + 1], "%s: column band %d is empty or reversed (%d..%d)", name, j, xb[j], xb[j + 1]);
        SPEI_REQUIRE(x0[j] >= 0 && x0[j] < W, "%s: tile column %d at x %d lies outside the %dx%d frame", name, j, x0[j], H, W);
        SPEI_REQUIRE(x0[j] <= xb[j] && xb[j + 1] - x0[j] <= twp, "%s: column band %d (%d..%d) lies outside its tile (%d..%d)", name, j,
                     xb[j], xb[j + 1], x0[j], x0[j] + twp);
        tab.x0[j] = x0[j];
    }
    for (int i = 0; i <= rows; ++i) tab.yb[i] = yb[i];
    for (int j = 0; j <= cols; ++j) tab.xb[j] = xb[j];
    for (int k = 0; k < rows * cols; ++k) {
        SPEI_REQUIRE(tiles[k] && ((uintptr_t)tiles[k] & 3) == 0, "%s: tile %d is a null or misaligned pointer", name, k);
        tab.tile[k] = tiles[k];
    }
    return 0;
}

// the one launch of an egress call: tiles_out_kernel on an OutTab or tiles_blend_kernel on a BlendTab
template <typename T, typename Tab>
int launch_out(const char* name, void (*kernel)(Tab, T*, int*, int, int, int, int, int64_t, int, int64_t, int, float), const Tab& tab,
               T* dst, int* nonfinite, int H, int W, int rows, int cols, int thp, int twp, int depth, hipStream_t stream) {
    const int gw = (W + 3) / 4;
    const int vec_out = (W & 3) == 0 && ((uintptr_t)dst & GROUP_MASK<T>) == 0;
    const int64_t total = (int64_t)H * gw;
    if (nonfinite && hipMemsetAsync(nonfinite, 0, sizeof(int), stream) != hipSuccess) {
        spei_set_error("%s: clearing the non-finite flag failed", name);
        return -2;
    }
    hipLaunchKernelGGL(kernel, dim3(grid_for(total)), dim3(256), 0, stream, tab, dst, nonfinite, W, rows, cols, twp, (int64_t)thp * twp, gw,
                       total, vec_out, sizeof(T) == 1 ? 255.0f : (float)((1 << depth) - 1));
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

template <typename T>
int tiles_out(const char* name, const float* const* tiles, T* dst, int* nonfinite, int H, int W, const int* y0, const int* x0,
              const int* yb, const int* xb, int rows, int cols, int thp, int twp, int depth, hipStream_t stream) {
    OutTab tab = {};
    if (out_table(name, tiles, dst, H, W, y0, x0, yb, xb, rows, cols, thp, twp, depth, tab)) return -1;
    return launch_out(name, tiles_out_kernel<T>, tab, dst, nonfinite, H, W, rows, cols, thp, twp, depth, stream);
}

// the hard stitch's call, and with it the real tile size and the feather, which place the ramps
template <typename T>
int tiles_blend(const char* name, const float* const* tiles, T* dst, int* nonfinite, int H, int W, const int* y0, const int* x0,
                const int* yb, const int* xb, int rows, int cols, int thp, int twp, int th, int tw, int feather, int depth,
                hipStream_t stream) {
    BlendTab tab = {};
    if (out_table(name, tiles, dst, H, W, y0, x0, yb, xb, rows, cols, thp, twp, depth, tab.t)) return -1;
    SPEI_REQUIRE(th > 0 && tw > 0 && th <= H && tw <= W, "%s: a %dx%d tile does not fit a %dx%d frame", name, th, tw, H, W);
    SPEI_REQUIRE(thp == (th + MULT - 1) / MULT * MULT && twp == (tw + MULT - 1) / MULT * MULT, "%s: tile planes %dx%d are not the %dx%d "
                 "tile rounded up to multiples of %d", name, thp, twp, th, tw, MULT);
    SPEI_REQUIRE(feather >= 0 && feather <= FEATHER_MAX, "%s: feather %d (0..%d)", name, feather, FEATHER_MAX);
    // every ramp [b - f, b + f) lies in rows (columns) [0, th) ([0, tw)) of both of its tiles by seam_half's clip
    for (int s = 1; s < rows; ++s) {
        tab.fy[s] = seam_half(y0, yb, rows, th, s, feather);
        tab.ry[s] = tab.fy[s] ? (float)(1.0 / (4.0 * tab.fy[s])) : 0.0f;
        tab.ylo[s] = yb[s] - tab.fy[s];
        tab.yw[s] = 2 * tab.fy[s];
    }
    for (int s = 1; s < cols; ++s) {
        tab.fx[s] = seam_half(x0, xb, cols, tw, s, feather);
        tab.rx[s] = tab.fx[s] ? (float)(1.0 / (4.0 * tab.fx[s])) : 0.0f;
        tab.xlo[s] = xb[s] - tab.fx[s];
        tab.xw[s] = tab.fx[s] ? 2 * tab.fx[s] + 3 : 0;     // a group [x, x + 3] meets the ramp iff 0 <= x + 3 - xlo < 2 f + 3
    }
    return launch_out(name, tiles_blend_kernel<T>, tab, dst, nonfinite, H, W, rows, cols, thp, twp, depth, stream);
}

}  // namespace

extern "C" int spei_tiles_u8_blend(const float* const* tiles_host, unsigned char* dst, int* nonfinite, int H, int W, const int* y0_host,
                                   const int* x0_host, const int* yb_host, const int* xb_host, int rows, int cols, int thp, int twp,
                                   int th, int tw, int feather, spei_stream_t stream) {
    return tiles_blend<unsigned char>("spei_tiles_u8_blend", tiles_host, dst, nonfinite, H, W, y0_host, x0_host, yb_host, xb_host, rows,
                                      cols, thp, twp, th, tw, feather, 8, (hipStream_t)stream);
}

extern "C" int spei_tiles_u16_blend(const float* const* tiles_host, uint16_t* dst, int* nonfinite, int H, int W, const int* y0_host,
                                    const int* x0_host, const int* yb_host, const int* xb_host, int rows, int cols, int thp, int twp,
                                    int th, int tw, int feather, int depth, spei_stream_t stream) {
    return tiles_blend<uint16_t>("spei_tiles_u16_blend", tiles_host, dst, nonfinite, H, W, y0_host, x0_host, yb_host, xb_host, rows, cols,
                                 thp, twp, th, tw, feather, depth, (hipStream_t)stream);
}

extern "C" int spei_tiles_u8_in(const unsigned char* src, int H, int W, float* dst, int64_t tile_stride, const int* y0_host,
                                const int* x0_host, int rows, int cols, int th, int tw, spei_stream_t stream) {
    return tiles_in<unsigned char>("spei_tiles_u8_in", src, H, W, dst, tile_stride, y0_host, x0_host, rows, cols, th, tw, 8,
                                   (hipStream_t)stream);
}

extern "C" int spei_tiles_u16_in(const uint16_t* src, int H, int W, float* dst, int64_t tile_stride, const int* y0_host,
                                 const int* x0_host, int rows, int cols, int th, int tw, int depth, spei_stream_t stream) {
    return tiles_in<uint16_t>("spei_tiles_u16_in", src, H, W, dst, tile_stride, y0_host, x0_host, rows, cols, th, tw, depth,
                              (hipStream_t)stream);
}

extern "C" int spei_tiles_u8_out(const float* const* tiles_host, unsigned char* dst, int* nonfinite, int H, int W, const int* y0_host,
                                 const int* x0_host, const int* yb_host, const int* xb_host, int rows, int cols, int thp, int twp,
                                 spei_stream_t stream) {
    return tiles_out<unsigned char>("spei_tiles_u8_out", tiles_host, dst, nonfinite, H, W, y0_host, x0_host, yb_host, xb_host, rows, cols,
                                    thp, twp, 8, (hipStream_t)stream);
}

extern "C" int spei_tiles_u16_out(const float* const* tiles_host, uint16_t* dst, int* nonfinite, int H, int W, const int* y0_host,
                                  const int* x0_host, const int* yb_host, const int* xb_host, int rows, int cols, int thp, int twp,
                                  int depth, spei_stream_t stream) {
    return tiles_out<uint16_t>("spei_tiles_u16_out", tiles_host, dst, nonfinite, H, W, y0_host, x0_host, yb_host, xb_host, rows, cols,
                               thp, twp, depth, (hipStream_t)stream);
}
