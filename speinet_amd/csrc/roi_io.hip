// Region-of-interest I/O of the clip API (video.deblur_clip(..., roi=)): only a rectangle of every frame is deblurred, the rest of the
// frame is the input's.  The rectangle is ingested by spei_tiles_u8_in / spei_tiles_u16_in (tile_io.hip) with a 1x1 table; this file
// holds the way back and the scan that finds the rectangle.
//
//   spei_roi_paste_u8 / spei_roi_paste_u16 — fp32 [3][hp][wp] (the model's output for the rectangle) and the packed input frame
//                        [H][W][3] -> the packed output frame: inside the rectangle spei_frame_u8_out / spei_frame_u16_out's value of
//                        the model's output, outside it the input's sample at the output depth (requant, exact integers), and with
//                        feather > 0 a ramp of that many pixels inside every side of the rectangle that is not a side of the frame,
//                        over which the two are blended (the definition is in include/speinet_hip.h).  One launch writes every sample
//                        once: no copy followed by an overwrite.
//   spei_frame_extent / spei_frame_extent_u16 — N packed frames -> the maximum of the integer luma of spei_frame_pair_stats over every
//                        row and over every column: the input of the clip API's bar rule (video.find_bars).  Integer maxima
//                        commute, so the result is exact whatever the launch shape.
//
// Streaming kernels on the pixel group of pixel_group.h, whose loads, luma, rounding and store they share with frame_io.hip and
// tile_io.hip.  The rectangle's origin is arbitrary, so the paste decides per group whether its four pixels are one aligned run of
// the model's planes; the rectangle and the ramps travel by value and every inside / outside / ramp decision is a compare against them.
#include "pixel_group.h"

namespace {

// the rectangle, and the ramp widths inside its four sides (the feather N, or 0 for a side on the frame's border); r = (float)(1 / (2 N))
struct Rect {
    int y0, x0, h, w;
    int top, bottom, left, right;
    int n;                                                 // the feather: 0 = a hard paste, no group meets a ramp
    float r;
};

// the weight of the model's output at place p of an axis of `len` pixels with ramps of lo / hi pixels at its two ends
__device__ __forceinline__ float axis_weight(int p, int len, int lo, int hi, float r) {
    if (p < lo) return __fmul_rn((float)(2 * p + 1), r);
    if (p >= len - hi) return __fmul_rn((float)(2 * (len - 1 - p) + 1), r);
    return 1.0f;
}

// TI: the input frame's samples (unsigned char: Din = 255; uint16_t: Din = 2^in_depth - 1, a word above it reads as it); TO: the
// output's.  A group wholly outside the rectangle reads the frame only, one wholly inside it and off the ramps the model's planes
// only; a group on a ramp, or across a side of the rectangle, reads both.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void roi_paste_kernel(const float* __restrict__ src, const TI* __restrict__ frame, TO* __restrict__ dst,
                                                        int* __restrict__ nonfinite, int W, Rect rc, int wp, int64_t plane, int gw,
                                                        int64_t total, int vec_src, int vec_frame, int vec_out, int Din, int Dout,
                                                        float inv_in, float Df) {
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / gw), x = (int)(i - (int64_t)y * gw) * 4;
        const int ry = y - rc.y0, rx = x - rc.x0;
        const bool rowin = (unsigned)ry < (unsigned)rc.h;
        const bool allout = !rowin || rx + 3 < 0 || rx >= rc.w;
        const bool allin = rowin && rx >= 0 && rx + 4 <= rc.w;
        // the group meets a ramp: its row lies in a row ramp, or one of its columns in a column ramp
        const bool ramp = !allout && rc.n && (ry < rc.top || ry >= rc.h - rc.bottom || rx < rc.left || rx + 3 >= rc.w - rc.right);
        uint32_t q[3][4];
        int fv[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (!allin || ramp) load_group(frame + ((int64_t)y * W + x) * 3, min(4, W - x), vec_frame != 0, Din, fv);
        if (allout) {
#pragma unroll
            for (int j = 0; j < 12; ++j) q[j % 3][j / 3] = requant(fv[j], Din, Dout);
        } else {
            const float* s = src + (int64_t)ry * wp + rx;
            float m[3][4];
            if (allin && (rx & 3) == 0 && vec_src) {       // four pixels of the rectangle, 16-byte aligned in the planes (wp % 4 == 0)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float4 f = *reinterpret_cast<const float4*>(s + c * plane);
                    m[c][0] = f.x; m[c][1] = f.y; m[c][2] = f.z; m[c][3] = f.w;
                }
            } else {                                       // an odd origin, or a side of the rectangle inside the group
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool in = (unsigned)(rx + k) < (unsigned)rc.w;
#pragma unroll
                    for (int c = 0; c < 3; ++c) m[c][k] = in ? s[c * plane + k] : 0.0f;
                }
            }
            const float wy = ramp ? axis_weight(ry, rc.h, rc.top, rc.bottom, rc.r) : 1.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = (unsigned)(rx + k) < (unsigned)rc.w;
                const float wt = ramp && in ? __fmul_rn(wy, axis_weight(rx + k, rc.w, rc.left, rc.right, rc.r)) : 1.0f;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float mv = m[c][k];
                    float v = mv;
                    if (wt != 1.0f) {                      // the blend with the input's value; wt == 1: the hard paste's bits
                        const float o = __fmul_rn((float)fv[3 * k + c], inv_in);
                        v = fmaf(wt, __fsub_rn(mv, o), o);
                    }
                    const bool fin = isfinite(mv);         // the flag and the 0 follow the model's value, not the blend's
                    bad |= fin ? 0 : 1;
                    q[c][k] = in ? (fin ? round_sample(v, Df) : 0u) : requant(fv[3 * k + c], Din, Dout);
                }
            }
        }
        store_group(dst + ((int64_t)y * W + x) * 3, q, vec_out != 0, W - x);
    }
    if (nonfinite && bad) atomicOr(nonfinite, 1);           // rare: one atomic per thread that met a non-finite value
}

// ---- the extent of the picture ------------------------------------------------------------------------------------------------------
// grid (column tiles of 256 pixels, row blocks, frame groups): a wave streams one row pair of its block's column tile at a time, 4
// pixels per lane, through every frame of its group (frames z, z + gridDim.z, ...), both rows in flight.  The row maxima are kept
// over those frames, reduced over the wave and cost one atomic per row, wave and frame group; the column maxima stay in registers over
// the rows and frames of a wave, meet the block's other waves in LDS and cost one atomic per column and block.  A maximum that does not
// exceed what the table already holds issues no atomic at all (the table only grows, so a stale read can only cost an atomic, never
// lose one).  Guideline 12: integer maxima commute exactly; the frame groups keep the atomics on one address few.
constexpr int EXT_TILE = 256;                              // columns per block: 64 lanes of 4 pixels
constexpr int EXT_ROW_BLOCKS = 32;                         // row blocks per frame at most: each strides over the rows 8 at a time
constexpr int EXT_FRAME_GROUPS = 4;                        // frame groups at most: with more, the atomics of a cold table set the time

template <typename T>
__global__ __launch_bounds__(256) void frame_extent_kernel(const T* __restrict__ src, int64_t fstride, int N, int H, int W, int* rowmax,
                                                           int* colmax, int aligned, int D) {
    __shared__ int cols[EXT_TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * EXT_TILE + lane * 4;
    const int valid = min(4, W - x);                       // <= 0: the lane lies past the row's end
    cols[threadIdx.x] = 0;
    __syncthreads();
    int cm[4] = {0, 0, 0, 0};
    for (int y = blockIdx.y * 8 + wave; y < H; y += gridDim.y * 8) {           // uniform over a wave: every lane runs the reductions
        const int y1 = y + 4;                                                  // the wave's second row of this pass
        int ra = 0, rb = 0;
        for (int n = blockIdx.z; n < N; n += gridDim.z) {
            const T* f = src + n * fstride + (int64_t)x * 3;
            int a[12], b[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) a[j] = b[j] = 0;
            if (valid > 0) {
                load_group(f + (int64_t)y * W * 3, valid, aligned != 0, D, a);
                if (y1 < H) load_group(f + (int64_t)y1 * W * 3, valid, aligned != 0, D, b);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ya = luma_of(a, k), yb = luma_of(b, k);
                const bool px = k < valid;                 // a missing pixel has no luma (its zeros would give 0 anyway)
                ra = max(ra, px ? ya : 0);
                rb = max(rb, px ? yb : 0);
                cm[k] = max(cm[k], px ? max(ya, yb) : 0);
            }
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            ra = max(ra, __shfl_xor(ra, m));
            rb = max(rb, __shfl_xor(rb, m));
        }
        if (lane == 0) {
            if (ra > rowmax[y]) atomicMax(&rowmax[y], ra);
            if (y1 < H && rb > rowmax[y1]) atomicMax(&rowmax[y1], rb);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (cm[k]) atomicMax(&cols[lane * 4 + k], cm[k]);
    __syncthreads();
    const int cx = blockIdx.x * EXT_TILE + threadIdx.x;
    if (cx < W) {
        const int c = cols[threadIdx.x];
        if (c > colmax[cx]) atomicMax(&colmax[cx], c);
    }
}

template <typename TO>
int roi_paste(const char* name, const float* src, const void* frame, int in_depth, TO* dst, int* nonfinite, int H, int W, int y0, int x0,
              int h, int w, int hp, int wp, int feather, int depth, hipStream_t stream) {
    SPEI_REQUIRE(src && frame && dst, "%s: null pointer", name);
    SPEI_REQUIRE(H > 0 && W > 0 && (int64_t)H * W * 3 < (1ll << 31), "%s: bad frame shape %dx%d", name, H, W);
    SPEI_REQUIRE(in_depth == 8 || in_depth == 10 || in_depth == 12, "%s: unknown in_depth %d (8, 10 or 12)", name, in_depth);
    SPEI_REQUIRE(sizeof(TO) == 1 ? depth == 8 : (depth == 10 || depth == 12), "%s: unknown depth %d (%s)", name, depth,
                 sizeof(TO) == 1 ? "8" : "10 or 12");
    SPEI_REQUIRE(h >= 1 && w >= 1 && y0 >= 0 && x0 >= 0 && y0 <= H - h && x0 <= W - w, "%s: the rectangle (%d, %d) %dx%d lies outside the "
                 "%dx%d frame or is empty", name, y0, x0, h, w, H, W);
    SPEI_REQUIRE(hp == (h + MULT - 1) / MULT * MULT && wp == (w + MULT - 1) / MULT * MULT, "%s: planes %dx%d are not the %dx%d rectangle "
                 "rounded up to multiples of %d", name, hp, wp, h, w, MULT);
    const int fmax = FEATHER_MAX < h / 2 ? (FEATHER_MAX < w / 2 ? FEATHER_MAX : w / 2) : (h / 2 < w / 2 ? h / 2 : w / 2);
    SPEI_REQUIRE(feather >= 0 && feather <= fmax, "%s: feather %d (0..%d: at most %d and half of the %dx%d rectangle)", name, feather, fmax,
                 FEATHER_MAX, h, w);
    const int in_bytes = in_depth == 8 ? 1 : 2;
    SPEI_REQUIRE(((uintptr_t)frame & (in_bytes - 1)) == 0 && ((uintptr_t)dst & (sizeof(TO) - 1)) == 0 && ((uintptr_t)src & 3) == 0,
                 "%s: misaligned pointer (src 4-byte, deep frames 2-byte aligned)", name);
    const int64_t samples = (int64_t)H * W * 3;
    SPEI_REQUIRE(!bytes_overlap(dst, samples * sizeof(TO), frame, samples * in_bytes), "%s: dst overlaps frame", name);
    SPEI_REQUIRE(!bytes_overlap(dst, samples * sizeof(TO), src, (int64_t)3 * hp * wp * sizeof(float)), "%s: dst overlaps src", name);
    Rect rc = {y0, x0, h, w, 0, 0, 0, 0, feather, 0.0f};
    if (feather > 0) {                                     // a side on the frame's border has no seam: no ramp
        rc.top = y0 > 0 ? feather : 0;
        rc.bottom = y0 + h < H ? feather : 0;
        rc.left = x0 > 0 ? feather : 0;
        rc.right = x0 + w < W ? feather : 0;
        rc.r = (float)(1.0 / (2.0 * feather));
    }
    const int gw = (W + 3) / 4;
    const int64_t total = (int64_t)H * gw;
    const int vec_src = ((uintptr_t)src & 15) == 0;
    const int vec_frame = (W & 3) == 0 && ((uintptr_t)frame & (in_bytes == 1 ? 3 : 7)) == 0;
    const int vec_out = (W & 3) == 0 && ((uintptr_t)dst & GROUP_MASK<TO>) == 0;
    const int Din = (1 << in_depth) - 1, Dout = (1 << depth) - 1;
    if (nonfinite && hipMemsetAsync(nonfinite, 0, sizeof(int), stream) != hipSuccess) {
        spei_set_error("%s: clearing the non-finite flag failed", name);
        return -2;
    }
    if (in_depth == 8)
        hipLaunchKernelGGL((roi_paste_kernel<unsigned char, TO>), dim3(grid_for(total)), dim3(256), 0, stream, src,
                           static_cast<const unsigned char*>(frame), dst, nonfinite, W, rc, wp, (int64_t)hp * wp, gw, total, vec_src,
                           vec_frame, vec_out, Din, Dout, (float)(1.0 / Din), (float)Dout);
    else
        hipLaunchKernelGGL((roi_paste_kernel<uint16_t, TO>), dim3(grid_for(total)), dim3(256), 0, stream, src,
                           static_cast<const uint16_t*>(frame), dst, nonfinite, W, rc, wp, (int64_t)hp * wp, gw, total, vec_src, vec_frame,
                           vec_out, Din, Dout, (float)(1.0 / Din), (float)Dout);
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

template <typename T>
int frame_extent(const char* name, const T* src, int64_t frame_stride, int N, int H, int W, int depth, int* rowmax, int* colmax,
                 int accumulate, hipStream_t stream) {
    SPEI_REQUIRE(src && rowmax && colmax, "%s: null pointer", name);
    SPEI_REQUIRE(N >= 1 && N <= 65535, "%s: %d frames (1..65535 per call)", name, N);
    SPEI_REQUIRE(H > 0 && W > 0 && (int64_t)H * W * 3 < (1ll << 31), "%s: bad frame shape %dx%d", name, H, W);
    SPEI_REQUIRE(sizeof(T) == 1 || depth == 10 || depth == 12, "%s: unknown depth %d (10 or 12)", name, depth);
    SPEI_REQUIRE(N == 1 || frame_stride >= (int64_t)H * W * 3 * (int64_t)sizeof(T), "%s: frame stride %lld < one %dx%d frame of %lld bytes",
                 name, (long long)frame_stride, H, W, (long long)H * W * 3 * (long long)sizeof(T));
    SPEI_REQUIRE(N == 1 || (frame_stride & (sizeof(T) - 1)) == 0, "%s: odd frame stride %lld (bytes, a multiple of 2)", name,
                 (long long)frame_stride);
    SPEI_REQUIRE(((uintptr_t)src & (sizeof(T) - 1)) == 0, "%s: src must be %d-byte aligned", name, (int)sizeof(T));
    const int aligned = ((uintptr_t)src & GROUP_MASK<T>) == 0 && (N == 1 || (frame_stride & GROUP_MASK<T>) == 0) && (W & 3) == 0;
    if (!accumulate && (hipMemsetAsync(rowmax, 0, sizeof(int) * H, stream) != hipSuccess ||
                        hipMemsetAsync(colmax, 0, sizeof(int) * W, stream) != hipSuccess)) {
        spei_set_error("%s: clearing the maxima failed", name);
        return -2;
    }
    const int row_blocks = (H + 7) / 8 < EXT_ROW_BLOCKS ? (H + 7) / 8 : EXT_ROW_BLOCKS;
    hipLaunchKernelGGL(frame_extent_kernel<T>, dim3((W + EXT_TILE - 1) / EXT_TILE, row_blocks, N < EXT_FRAME_GROUPS ? N : EXT_FRAME_GROUPS),
                       dim3(256), 0, stream, src, N == 1 ? 0 : frame_stride / (int64_t)sizeof(T), N, H, W, rowmax, colmax, aligned,
                       sizeof(T) == 1 ? 255 : (1 << depth) - 1);
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

}  // namespace

extern "C" int spei_roi_paste_u8(const float* src, const void* frame, int in_depth, unsigned char* dst, int* nonfinite, int H, int W,
                                 int y0, int x0, int h, int w, int hp, int wp, int feather, spei_stream_t stream) {
    return roi_paste<unsigned char>("spei_roi_paste_u8", src, frame, in_depth, dst, nonfinite, H, W, y0, x0, h, w, hp, wp, feather, 8,
                                    (hipStream_t)stream);
}

extern "C" int spei_roi_paste_u16(const float* src, const void* frame, int in_depth, uint16_t* dst, int* nonfinite, int H, int W, int y0,
                                  int x0, int h, int w, int hp, int wp, int feather, int depth, spei_stream_t stream) {
    return roi_paste<uint16_t>("spei_roi_paste_u16", src, frame, in_depth, dst, nonfinite, H, W, y0, x0, h, w, hp, wp, feather, depth,
                               (hipStream_t)stream);
}

extern "C" int spei_frame_extent(const unsigned char* src, int64_t frame_stride, int N, int H, int W, int* rowmax, int* colmax,
                                 int accumulate, spei_stream_t stream) {
    return frame_extent<unsigned char>("spei_frame_extent", src, frame_stride, N, H, W, 8, rowmax, colmax, accumulate, (hipStream_t)stream);
}

extern "C" int spei_frame_extent_u16(const uint16_t* src, int64_t frame_stride, int N, int H, int W, int depth, int* rowmax, int* colmax,
                                     int accumulate, spei_stream_t stream) {
    return frame_extent<uint16_t>("spei_frame_extent_u16", src, frame_stride, N, H, W, depth, rowmax, colmax, accumulate,
                                  (hipStream_t)stream);
}
