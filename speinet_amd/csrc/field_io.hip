// Field I/O of the clip API's interlaced mode (video.deblur_clip(..., fields="split"); an extension beyond the reference, which knows
// progressive frames only): a woven frame [H][W][3] of even height is two fields of H / 2 rows, field p (0 = top, 1 = bottom) its rows
// p, p + 2, p + 4, ...  Each parity is deblurred as a clip of its own, so a window runs as two parts of one shape.
//
//   spei_fields_u8_in / spei_fields_u16_in   — one packed [H][W][3] frame -> both fields as fp32 planes [3][hp][wp], field p at
//                        dst + p * field_stride, hp = H / 2 and wp = W rounded up to multiples of 20: field p is bit-identical to
//                        spei_frames_u8_in / spei_frames_u16_in (frame_io.hip) on the packed copy of rows p :: 2, its reflect pad
//                        included.  The pad is the FIELD's: padded field row H / 2 + j reads field row H / 2 - 2 - j, which is frame
//                        row 2 (H / 2 - 2 - j) + p.  One launch per frame.
//   spei_fields_u8_out / spei_fields_u16_out — two fp32 [3][hp][wp] planes -> one packed [H][W][3] frame: row 2 r + p is row r of
//                        spei_frame_u8_out / spei_frame_u16_out's crop of plane p; the flag is set by a non-finite value in either
//                        field's crop.  One launch per frame, every sample written once.
//
// Streaming kernels on the pixel group of pixel_group.h, whose ingest, rounding and store they share with frame_io.hip: one thread per
// group of 4 pixels, adjacent threads on adjacent groups of one row, so the stride-2 row walk changes the row's base only and every
// wave still reads and writes whole contiguous lines.  HBM-bound: the bytes moved are those of the progressive launches.
#include "pixel_group.h"

namespace {

// T = unsigned char (D = 255, inv = INV255) or uint16_t (D = 2^depth - 1, inv = (float)(1.0 / D); a word above D reads as D).
// Hf = H / 2, the rows of a field; fstride in floats
template <typename T>
__global__ __launch_bounds__(256) void fields_in_kernel(const T* __restrict__ src, int W, float* __restrict__ dst, int64_t fstride,
                                                        int Hf, int hp, int wp, int64_t total, int D, float inv) {
    const int gw = wp >> 2;                                // groups per padded row (wp % 20 == 0)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / gw;                        // p * hp + y
        const int x = (int)(i - row * gw) * 4;
        const int p = (int)(row / hp), y = (int)(row - (int64_t)p * hp);
        const int sy = y < Hf ? y : 2 * Hf - 2 - y;        // padded field row Hf + j reads field row Hf - 2 - j
        const T* s = src + (int64_t)(2 * sy + p) * W * 3;  // field row sy of parity p is frame row 2 sy + p
        float v[3][4];
        ingest_group(s, x, W, ((uintptr_t)s & GROUP_MASK<T>) == 0, D, v);      // spei_frames_u8_in's values of the field's row
        float* d = dst + p * fstride + (int64_t)y * wp + x;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            *reinterpret_cast<float4*>(d + (int64_t)c * hp * wp) = make_float4(v[c][0] * inv, v[c][1] * inv, v[c][2] * inv, v[c][3] * inv);
    }
}

// T = unsigned char (Df = 255) or uint16_t (Df = 2^depth - 1); frame row y is row y >> 1 of the plane of parity y & 1
template <typename T>
__global__ __launch_bounds__(256) void fields_out_kernel(const float* __restrict__ top, const float* __restrict__ bottom,
                                                         T* __restrict__ dst, int* __restrict__ nonfinite, int W, int wp, int64_t plane,
                                                         int gw, int64_t total, int vec_in, int vec_out, float Df) {
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / gw), x0 = (int)(i - (int64_t)y * gw) * 4;
        const float* s = ((y & 1) ? bottom : top) + (int64_t)(y >> 1) * wp + x0;
        uint32_t q[3][4];
        if (vec_in) {                                      // wp % 4 == 0: x0 + 4 <= wp; columns W.. of the group are pad, not the crop
            bad |= quantise_planes(s, plane, Df, W - x0, q);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float v = x0 + k < W ? s[c * plane + k] : 0.0f;
                    q[c][k] = quantise(v, Df);
                    bad |= isfinite(v) ? 0 : 1;
                }
        }
        store_group(dst + ((int64_t)y * W + x0) * 3, q, vec_out != 0, W - x0);
    }
    if (nonfinite && bad) atomicOr(nonfinite, 1);           // rare: one atomic per thread that met a non-finite value
}

template <typename T>
int fields_in(const char* name, const T* src, int H, int W, float* dst, int64_t field_stride, int depth, hipStream_t stream) {
    SPEI_REQUIRE(src && dst, "%s: null pointer", name);
    SPEI_REQUIRE(H > 0 && W > 0 && (int64_t)H * W * 3 < (1ll << 31), "%s: bad frame shape %dx%d", name, H, W);
    SPEI_REQUIRE((H & 1) == 0, "%s: a frame of H = %d rows does not split into two fields (H must be even)", name, H);
    const int Hf = H / 2, hp = (Hf + MULT - 1) / MULT * MULT, wp = (W + MULT - 1) / MULT * MULT;
    SPEI_REQUIRE(hp - Hf < Hf && wp - W < W, "%s: a %dx%d field cannot reflect-pad to %dx%d (the pad must be smaller than the field)", name,
                 Hf, W, hp, wp);
    SPEI_REQUIRE(sizeof(T) == 1 || depth == 10 || depth == 12, "%s: unknown depth %d (10 or 12)", name, depth);
    SPEI_REQUIRE(((uintptr_t)src & (sizeof(T) - 1)) == 0, "%s: src must be %d-byte aligned", name, (int)sizeof(T));
    SPEI_REQUIRE(((uintptr_t)dst & 15) == 0 && (field_stride & 3) == 0, "%s: dst must be 16-byte aligned and the field stride a multiple "
                 "of 4 floats", name);
    SPEI_REQUIRE(field_stride >= (int64_t)3 * hp * wp, "%s: field stride %lld < one field of 3x%dx%d floats", name,
                 (long long)field_stride, hp, wp);
    const int64_t total = (int64_t)2 * hp * (wp / 4);
    const int D = sizeof(T) == 1 ? 255 : (1 << depth) - 1;
    hipLaunchKernelGGL(fields_in_kernel<T>, dim3(grid_for(total)), dim3(256), 0, stream, src, W, dst, field_stride, Hf, hp, wp, total, D,
                       sizeof(T) == 1 ? INV255 : (float)(1.0 / D));
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

template <typename T>
int fields_out(const char* name, const float* top, const float* bottom, T* dst, int* nonfinite, int H, int W, int hp, int wp, int depth,
               hipStream_t stream) {
    SPEI_REQUIRE(top && bottom && dst, "%s: null pointer", name);
    SPEI_REQUIRE(H > 0 && W > 0 && (int64_t)H * W * 3 < (1ll << 31), "%s: bad frame shape %dx%d", name, H, W);
    SPEI_REQUIRE((H & 1) == 0, "%s: a frame of H = %d rows is not the weave of two fields (H must be even)", name, H);
    SPEI_REQUIRE(hp >= H / 2 && wp >= W && (int64_t)hp * wp < (1ll << 30), "%s: bad sizes (crop %dx%d of a %dx%d field)", name, H / 2, W, hp,
                 wp);
    SPEI_REQUIRE(sizeof(T) == 1 || depth == 10 || depth == 12, "%s: unknown depth %d (10 or 12)", name, depth);
    SPEI_REQUIRE(((uintptr_t)dst & (sizeof(T) - 1)) == 0, "%s: dst must be 2-byte aligned", name);
    const int gw = (W + 3) / 4;
    const int vec_in = (wp & 3) == 0 && (((uintptr_t)top | (uintptr_t)bottom) & 15) == 0;
    const int vec_out = (W & 3) == 0 && ((uintptr_t)dst & GROUP_MASK<T>) == 0;
    const int64_t total = (int64_t)H * gw;
    if (nonfinite && hipMemsetAsync(nonfinite, 0, sizeof(int), stream) != hipSuccess) {
        spei_set_error("%s: clearing the non-finite flag failed", name);
        return -2;
    }
    hipLaunchKernelGGL(fields_out_kernel<T>, dim3(grid_for(total)), dim3(256), 0, stream, top, bottom, dst, nonfinite, W, wp,
                       (int64_t)hp * wp, gw, total, vec_in, vec_out, sizeof(T) == 1 ? 255.0f : (float)((1 << depth) - 1));
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

}  // namespace

extern "C" int spei_fields_u8_in(const unsigned char* src, int H, int W, float* dst, int64_t field_stride, spei_stream_t stream) {
    return fields_in<unsigned char>("spei_fields_u8_in", src, H, W, dst, field_stride, 8, (hipStream_t)stream);
}

extern "C" int spei_fields_u16_in(const uint16_t* src, int H, int W, float* dst, int64_t field_stride, int depth, spei_stream_t stream) {
    return fields_in<uint16_t>("spei_fields_u16_in", src, H, W, dst, field_stride, depth, (hipStream_t)stream);
}

extern "C" int spei_fields_u8_out(const float* top, const float* bottom, unsigned char* dst, int* nonfinite, int H, int W, int hp, int wp,
                                  spei_stream_t stream) {
    return fields_out<unsigned char>("spei_fields_u8_out", top, bottom, dst, nonfinite, H, W, hp, wp, 8, (hipStream_t)stream);
}

extern "C" int spei_fields_u16_out(const float* top, const float* bottom, uint16_t* dst, int* nonfinite, int H, int W, int hp, int wp,
                                   int depth, spei_stream_t stream) {
    return fields_out<uint16_t>("spei_fields_u16_out", top, bottom, dst, nonfinite, H, W, hp, wp, depth, (hipStream_t)stream);
}
