// Mattes of the clip API (video.deblur_clip(..., matte=)): an 8-bit mask says how much of the deblurred frame every pixel gets, the
// rest is the input's.
//
//   spei_frame_matte_u8 / spei_frame_matte_u16 — the packed input frame [H][W][3], the packed deblurred frame [H][W][3] at the output
//                        depth and the matte [H][W] -> the packed output frame, every sample
//                            (a * (255 - m) + b * m + 127) / 255
//                        with a = requant(input sample) (the kept frame's value), b the deblurred sample (a word above D_out reads as
//                        D_out) and m the matte byte of the pixel (255 - m under `invert`): exact integers, at most 4095 * 255 + 127.
//                        m = 0 gives a, m = 255 gives b, a == b gives a for every m.  dst may be deb itself: the clip loop blends the
//                        frame its egress wrote in place.
//
// A streaming kernel on the pixel group of pixel_group.h: one thread per group of 4 pixels of a row reads its 12 input samples, its 12
// deblurred samples and its 4 matte bytes (one dword where the row length and the base allow, byte by byte otherwise) and then
// writes its 12 samples, so an in-place call reads every group before it is overwritten, by the same thread.
// (Tried and not kept: a thread per 16 consecutive pixels of the packed frame, moved as 16-byte words.  It measured slower on an
// MI355X in three of four cases, 5.5 against 4.1 us at 720p with 12-bit samples: a quarter of the threads, four times the registers.)
#include "pixel_group.h"

namespace {

// TI: the input frame's samples (unsigned char: Din = 255; uint16_t: a word above Din reads as Din); TO: those of deb and dst.  deb
// and dst carry no __restrict__: they may be one buffer.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void frame_matte_kernel(const TI* __restrict__ frame, const TO* deb, const unsigned char* __restrict__ matte,
                                                          TO* dst, int W, int gw, int64_t total, int vec_frame, int vec_deb, int vec_matte,
                                                          int vec_out, int Din, int Dout, int invert) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / gw), x = (int)(i - (int64_t)y * gw) * 4;
        const int valid = min(4, W - x);
        const int64_t at = (int64_t)y * W + x;
        int a[12], b[12], m[4];
        load_group(frame + at * 3, valid, vec_frame != 0, Din, a);
        load_group(deb + at * 3, valid, vec_deb != 0, Dout, b);
        if (vec_matte) {                                   // W % 4 == 0: every group is whole and lies on a dword of the matte
            const uint32_t w = *reinterpret_cast<const uint32_t*>(matte + at);
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] = (w >> (8 * k)) & 0xff;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] = k < valid ? (int)matte[at + k] : 0;
        }
        uint32_t q[3][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t mk = (uint32_t)(invert ? 255 - m[k] : m[k]);
#pragma unroll
            for (int c = 0; c < 3; ++c)
                q[c][k] = (requant(a[3 * k + c], Din, Dout) * (255u - mk) + (uint32_t)b[3 * k + c] * mk + 127u) / 255u;
        }
        store_group(dst + at * 3, q, vec_out != 0, valid);
    }
}

template <typename TO>
int frame_matte(const char* name, const void* frame, int in_depth, const TO* deb, const unsigned char* matte, int invert, TO* dst, int H,
                int W, int depth, hipStream_t stream) {
    SPEI_REQUIRE(frame && deb && matte && dst, "%s: null pointer", name);
    SPEI_REQUIRE(in_depth == 8 || in_depth == 10 || in_depth == 12, "%s: unknown in_depth %d (8, 10 or 12)", name, in_depth);
    SPEI_REQUIRE(sizeof(TO) == 1 ? depth == 8 : (depth == 10 || depth == 12), "%s: unknown depth %d (%s)", name, depth,
                 sizeof(TO) == 1 ? "8" : "10 or 12");
    SPEI_REQUIRE(H > 0 && W > 0 && (int64_t)H * W * 3 < (1ll << 31), "%s: bad frame shape %dx%d", name, H, W);
    const int in_bytes = in_depth == 8 ? 1 : 2;
    SPEI_REQUIRE(((uintptr_t)frame & (in_bytes - 1)) == 0 && (((uintptr_t)deb | (uintptr_t)dst) & (sizeof(TO) - 1)) == 0,
                 "%s: misaligned pointer (deep frames are 2-byte aligned)", name);
    const int64_t pixels = (int64_t)H * W, samples = pixels * 3, out_bytes = samples * (int64_t)sizeof(TO);
    SPEI_REQUIRE((const void*)dst == (const void*)deb || !bytes_overlap(dst, out_bytes, deb, out_bytes),
                 "%s: dst overlaps deb (dst == deb, in place, is the one overlap allowed)", name);
    SPEI_REQUIRE(!bytes_overlap(dst, out_bytes, frame, samples * in_bytes), "%s: dst overlaps frame", name);
    SPEI_REQUIRE(!bytes_overlap(dst, out_bytes, matte, pixels), "%s: dst overlaps matte", name);
    const int gw = (W + 3) / 4;
    const int64_t total = (int64_t)H * gw;
    const int whole = (W & 3) == 0;                        // every group is four pixels of one row
    const int vec_frame = whole && ((uintptr_t)frame & (in_bytes == 1 ? 3 : 7)) == 0;
    const int vec_deb = whole && ((uintptr_t)deb & GROUP_MASK<TO>) == 0;
    const int vec_out = whole && ((uintptr_t)dst & GROUP_MASK<TO>) == 0;
    const int vec_matte = whole && ((uintptr_t)matte & 3) == 0;
    const int Din = (1 << in_depth) - 1, Dout = (1 << depth) - 1;
    if (in_depth == 8)
        hipLaunchKernelGGL((frame_matte_kernel<unsigned char, TO>), dim3(grid_for(total)), dim3(256), 0, stream,
                           static_cast<const unsigned char*>(frame), deb, matte, dst, W, gw, total, vec_frame, vec_deb, vec_matte, vec_out,
                           Din, Dout, invert != 0);
    else
        hipLaunchKernelGGL((frame_matte_kernel<uint16_t, TO>), dim3(grid_for(total)), dim3(256), 0, stream,
                           static_cast<const uint16_t*>(frame), deb, matte, dst, W, gw, total, vec_frame, vec_deb, vec_matte, vec_out, Din,
                           Dout, invert != 0);
    SPEI_CHECK_LAUNCH(name);
    return 0;
}

}  // namespace

extern "C" int spei_frame_matte_u8(const void* frame, int in_depth, const unsigned char* deb, const unsigned char* matte, int invert,
                                   unsigned char* dst, int H, int W, spei_stream_t stream) {
    return frame_matte<unsigned char>("spei_frame_matte_u8", frame, in_depth, deb, matte, invert, dst, H, W, 8, (hipStream_t)stream);
}

extern "C" int spei_frame_matte_u16(const void* frame, int in_depth, const uint16_t* deb, const unsigned char* matte, int invert,
                                    uint16_t* dst, int H, int W, int depth, spei_stream_t stream) {
    return frame_matte<uint16_t>("spei_frame_matte_u16", frame, in_depth, deb, matte, invert, dst, H, W, depth, (hipStream_t)stream);
}
