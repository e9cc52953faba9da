// Weight-stationary 5x5 convolution for the 64-channel level of the encoder / decoder stacks (reference model/block.py:26-47,127-131:
// the two 5x5 convs of a ResBlock at half resolution) on the gfx950 16-bit matrix pipe.
//
// Why: at 64 output channels the slab kernel runs <WM=2, WN=2, TM=2, TN=1>, so a 1 KiB weight fragment from L2 feeds two MFMAs — the
// weight-intake limit that conv32_ws16.hip describes for the 32-channel layers, 41-47 % MFMA busy.  A 64 -> 64 channel
// 5x5 layer has 205 KB of weights = 4 x 51 KB, so the four waves of a workgroup can hold it between them in the same 200 registers per
// wave that conv32_ws_kernel uses:
//     wave w owns output n-tile n = w >> 1 (channels [32n, 32n + 32)) and input-channel half h = w & 1 (k-steps 2h, 2h + 1 of every tap):
//     25 taps x 2 k-steps = 50 fragments, loaded once, MFMA A operands straight from the accumulation registers (mfma_aw).
// One persistent workgroup per CU walks over 6 x 32 pixel tiles of all the launch's maps.  Every wave computes its (n, h) partial sum
// for all 6 tile rows; the two K-halves of an n-tile are then added through LDS (each wave of the pair hands the other the 3 rows the
// other finishes) and each wave of the pair writes 3 rows: bias, ReLU, store.  The next tile's slab (10 x 36 pixels x 64 channels) is
// loaded during the current tile's 300 MFMAs per wave and written to the second slab buffer, as in conv32_ws_kernel.
// LDS: two slabs of 10 * 36 * 144 B + the K-half exchange 4 waves * 3 rows * 4 KiB = 152 832 bytes.
// fp32 accumulation in tap order (dy, dx), then k-step, per half; the result is (h = 0) + (h = 1), then + bias: a fixed order that does
// not depend on the workgroup or the map slot a tile lands in.  Same operand rounding as the slab kernel.
#include "common.h"

namespace {

constexpr int C = 64, KS = 5, PAD = 2, NTAP = KS * KS;
constexpr int TH = 6, TW = 32;                        // output tile
constexpr int IH = TH + KS - 1, IW = TW + KS - 1;     // 10 x 36 slab pixels
constexpr int PITCH = 2 * C + 16;                     // 144 bytes per slab pixel: conflict-free ds_read_b128 of 16 consecutive pixels
constexpr int SLAB = IH * IW * PITCH;                 // 51 840 bytes
constexpr int NTHR = 256;
constexpr int HR = TH / 2;                            // rows each wave of a pair finishes
constexpr int XCH_WAVE = HR * 4 * 64 * 16;            // exchange bytes per wave: 3 rows x 4 channel quadruples x 64 lanes x 16 B
constexpr int LDS_BYTES = 2 * SLAB + 4 * XCH_WAVE;    // 152 832
constexpr int PF = 1;                                 // B fragments are read PF steps ahead of the MFMAs (6 MFMAs = ~200 cycles a step)

struct WsParams {
    const void* a;        // [batch][H*W][64] fp32 or LP
    const void* wfrag;    // fragment order [2][25][4][64][8] LP
    const float* bias;    // [64] or null
    void* out;            // [batch][H*W][64] LP or fp32
    int H, W, batch, act;
    int tiles_x, tiles_y, total;
    long long* stamps;    // tuning build: phase stamps of every workgroup's SECOND tile (steady state), else NULL
};

// MFMA with the resident weight fragment as the A operand read from the accumulation registers (conv32_ws16.hip: left to the compiler
// every use is preceded by v_accvgpr_read copies)
__device__ __forceinline__ void mfma_aw(f32x16& acc, const lpv<_Float16>::x8& w, const lpv<_Float16>::x8& b) {
    asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "a"(w), "v"(b));
}
__device__ __forceinline__ void mfma_aw(f32x16& acc, const lpv<__bf16>::x8& w, const lpv<__bf16>::x8& b) {
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "a"(w), "v"(b));
}
// ... the first of a chain, from 0 (no 96 register moves per tile to clear the accumulators)
__device__ __forceinline__ void mfma_aw0(f32x16& acc, const lpv<_Float16>::x8& w, const lpv<_Float16>::x8& b) {
    asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=v"(acc) : "a"(w), "v"(b));
}
__device__ __forceinline__ void mfma_aw0(f32x16& acc, const lpv<__bf16>::x8& w, const lpv<__bf16>::x8& b) {
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=v"(acc) : "a"(w), "v"(b));
}

// 16-byte chunks of a slab: pixel-major; TA = float: 16 chunks of 4 channels per pixel, TA = LP: 8 chunks of 8 channels
template <typename TA> struct Chunk { static constexpr int CPP = sizeof(TA) == 4 ? 16 : 8; };

template <typename LP, typename TA, typename TO>
__global__ __launch_bounds__(NTHR, 1) void conv64_ws_kernel(const WsParams p) {
    typedef typename lpv<LP>::x8 lp8;
    typedef typename lpv<LP>::x4 lp4;
    constexpr int CPP = Chunk<TA>::CPP;
    constexpr int NCH = IH * IW * CPP;                                  // chunks per slab
    constexpr int NIT = (NCH + NTHR - 1) / NTHR;                        // staging loads per thread: 23 (fp32) / 12 (16-bit)
    // fp32 input: the next slab travels in three parts (8 + 8 + 7 chunks per thread), each requested when the previous one has been
    // written to LDS, at steps 16 and 32 of the MFMA loop: with two parts (conv32_ws_kernel) the 48 staging registers beside the 200
    // weight and 96 accumulator registers spill
    constexpr int NPH = sizeof(TA) == 4 ? 3 : 1;
    constexpr int NITH = (NIT + NPH - 1) / NPH;
    constexpr int PSTEP = 2 * NTAP / NPH;
    static_assert(NPH == 1 || NPH == 3, "the MFMA loop below is cut for one or three staging parts");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, fk = lane >> 5;
    const int nt = wave >> 1, kh = wave & 1;                            // output n-tile, input-channel half

    // ---- this wave's quarter of the layer's weights: 50 fragments, resident for the whole launch ----------------------------------------
    lp8 wreg[NTAP][2];
    {
        const LP* wp = static_cast<const LP*>(p.wfrag) + ((size_t)nt * NTAP * 4 + 2 * kh) * 512 + lane * 8;
#pragma unroll
        for (int t = 0; t < NTAP; ++t)
#pragma unroll
            for (int s = 0; s < 2; ++s) wreg[t][s] = *reinterpret_cast<const lp8*>(wp + (t * 4 + s) * 512);
    }
    float biasv[16];                                                    // accumulator row r <-> output channel 32 nt + 8 (r >> 2) + 4 fk + (r & 3)
#pragma unroll
    for (int r = 0; r < 16; ++r) biasv[r] = p.bias ? p.bias[32 * nt + 8 * (r >> 2) + 4 * fk + (r & 3)] : 0.f;

    typedef u32x4 stage_t;                                              // one 16-byte chunk as it comes from global memory
    stage_t sreg[NITH];
    const size_t map_elems = (size_t)p.H * p.W * C;
    const int per_map = p.tiles_x * p.tiles_y;
    // Tile order: workgroups are dealt to the 8 XCDs round robin, so in each full round of gridDim.x tiles the workgroups of one XCD take
    // a contiguous run of tiles (row-major over the map: vertical and horizontal neighbours, whose slab halos then meet in that XCD's L2).
    // The last, partial round keeps the plain order.  Which tile a workgroup computes never changes what the tile's result is.
    const int G = gridDim.x;
    const int slot = (G & 7) ? (int)blockIdx.x : (int)(blockIdx.x & 7) * (G >> 3) + (int)(blockIdx.x >> 3);
    auto tile_of = [&](int t) {                                         // t: blockIdx.x + round * G
        const int base = t - (int)blockIdx.x;
        return base + G <= p.total ? base + slot : t;
    };
    auto tile_origin = [&](int t, int& b, int& oy0, int& ox0) {
        t = tile_of(t);
        b = t / per_map;
        const int r = t - b * per_map;
        const int ty = r / p.tiles_x;
        oy0 = ty * TH;
        ox0 = (r - ty * p.tiles_x) * TW;
    };
    // chunk c = it * 256 + tid of a slab: slab pixel p0 + it * PPI, 16-byte piece `sub` of it (conv32_ws_kernel)
    constexpr int PPI = NTHR / CPP, E = 16 / (int)sizeof(TA);
    const int p0 = tid / CPP, sub = tid - p0 * CPP;
    const int iy0 = p0 / IW, ix0 = p0 - iy0 * IW;
    const int lds0 = p0 * PITCH + sub * (sizeof(TA) == 4 ? 8 : 16);
    auto advance = [](int& iy, int& ix) {
        ix += PPI % IW;
        iy += PPI / IW;
        if (ix >= IW) { ix -= IW; ++iy; }
    };
    // issue the global loads of tile t's slab, phase ph (clamped coordinates: every load is valid; pixels outside the map become zeros
    // at the write)
    auto load_slab = [&](int t, int ph) {
        int b, oy0, ox0;
        tile_origin(t, b, oy0, ox0);
        const TA* base = static_cast<const TA*>(p.a) + (size_t)b * map_elems + sub * E;
        int iy = iy0, ix = ix0;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (it >= ph * NITH && it < (ph + 1) * NITH) {
                const int iyc = min(iy, IH - 1);                           // (the last iteration runs past the slab for some threads)
                const int gy = min(max(oy0 - PAD + iyc, 0), p.H - 1), gx = min(max(ox0 - PAD + ix, 0), p.W - 1);
                sreg[it - ph * NITH] = *reinterpret_cast<const stage_t*>(base + ((size_t)gy * p.W + gx) * C);
            }
            advance(iy, ix);
        }
    };
    // ... and write chunks [lo, hi) of phase ph (converted to the 16-bit operand format) into slab buffer `buf`
    auto store_slab = [&](int t, int buf, int ph, int lo, int hi) {
        int b, oy0, ox0;
        tile_origin(t, b, oy0, ox0);
        unsigned char* sl = smem + buf * SLAB + lds0;
        int iy = iy0, ix = ix0;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (it >= ph * NITH + lo && it < ph * NITH + hi && it < (ph + 1) * NITH && iy < IH) {
                const int j = it - ph * NITH;
                const bool ok = ((unsigned)(oy0 - PAD + iy) < (unsigned)p.H) & ((unsigned)(ox0 - PAD + ix) < (unsigned)p.W);
                if constexpr (sizeof(TA) == 4) {
                    const f32x4 v = __builtin_bit_cast(f32x4, sreg[j]);
                    lp4 h = to_lp4<LP>(v);
                    if (!ok) h = lp4{(LP)0.f, (LP)0.f, (LP)0.f, (LP)0.f};
                    *reinterpret_cast<lp4*>(sl + it * PPI * PITCH) = h;
                } else {
                    *reinterpret_cast<stage_t*>(sl + it * PPI * PITCH) = ok ? sreg[j] : stage_t{0u, 0u, 0u, 0u};
                }
            }
            advance(iy, ix);
        }
    };

    int t = blockIdx.x;
    if (t >= p.total) return;
#pragma unroll
    for (int ph = 0; ph < NPH; ++ph) {
        load_slab(t, ph);
        store_slab(t, 0, ph, 0, NITH);
    }
    lds_barrier();

    // per-lane slab offsets of the six tile rows (pixel column fr, channel half fk of the wave's k-steps): tap and k-step are immediates.
    // Accumulator i holds tile row (i + 3 kh) mod 6: acc[0..2] are the rows this wave finishes, acc[3..5] the rows it hands its partner,
    // the same registers in both waves of a pair (no selects on kh in the epilogue)
    int boff[TH];
#pragma unroll
    for (int i = 0; i < TH; ++i) boff[i] = (((i + HR * kh) % TH) * IW + fr) * PITCH + kh * 64 + fk * 16;
    unsigned char* const xch = smem + 2 * SLAB;

    int buf = 0;
    for (; t < p.total; t += gridDim.x, buf ^= 1) {
        const int tn = t + gridDim.x;
        const bool more = tn < p.total;
        const int tl = more ? tn : t;                                   // (unconditional loads: a conditional one keeps the old registers alive)
        const bool st_ = t == (int)blockIdx.x + (int)gridDim.x;
        if (st_) SPEI_STAMP(p.stamps, 0);
        load_slab(tl, 0);
        if (st_) SPEI_STAMP(p.stamps, 1);
        __builtin_amdgcn_sched_barrier(0);

        const unsigned char* sl = smem + buf * SLAB;
        f32x16 acc[TH];                                                 // (the first step's MFMAs start them from 0: mfma_aw0)
        // B fragments (pixels) PF steps ahead of the MFMAs that consume them
        lp8 bq[PF + 1][TH];
        auto step_off = [](int step) { const int tap = step >> 1; return ((tap / KS) * IW + (tap % KS)) * PITCH + (step & 1) * 32; };
#pragma unroll
        for (int d = 0; d < PF; ++d)
#pragma unroll
            for (int i = 0; i < TH; ++i) bq[d][i] = *reinterpret_cast<const lp8*>(sl + boff[i] + step_off(d));
        // the MFMA loop in pieces with compile-time step ranges, the fp32 staging parts between them (left inside one loop, the three
        // store / load pairs make the body too large to unroll)
        auto steps = [&](auto lo_c, auto hi_c) {
            constexpr int LO = decltype(lo_c)::value, HI = decltype(hi_c)::value;
#pragma unroll
            for (int step = LO; step < HI; ++step) {
                const int tap = step >> 1, s2 = step & 1;
                if (step + PF < NTAP * 2) {
#pragma unroll
                    for (int i = 0; i < TH; ++i)
                        bq[(step + PF) % (PF + 1)][i] = *reinterpret_cast<const lp8*>(sl + boff[i] + step_off(step + PF));
                }
#pragma unroll
                for (int i = 0; i < TH; ++i) {
                    if (step == 0) mfma_aw0(acc[i], wreg[tap][s2], bq[step % (PF + 1)][i]);
                    else mfma_aw(acc[i], wreg[tap][s2], bq[step % (PF + 1)][i]);
                }
                // 16-bit input: the next slab's 12 chunks go to LDS one per two steps in the second half of the loop
                if (NPH == 1 && step >= NTAP && ((step - NTAP) & 1) == 0 && (step - NTAP) / 2 < NITH)
                    store_slab(tl, buf ^ 1, 0, (step - NTAP) / 2, (step - NTAP) / 2 + 1);
            }
        };
        if constexpr (NPH == 1) {
            steps(std::integral_constant<int, 0>{}, std::integral_constant<int, 2 * NTAP>{});
        } else {                                                        // part k - 1 of the next slab -> LDS, request part k
            steps(std::integral_constant<int, 0>{}, std::integral_constant<int, PSTEP>{});
            store_slab(tl, buf ^ 1, 0, 0, NITH);
            load_slab(tl, 1);
            steps(std::integral_constant<int, PSTEP>{}, std::integral_constant<int, 2 * PSTEP>{});
            store_slab(tl, buf ^ 1, 1, 0, NITH);
            load_slab(tl, 2);
            steps(std::integral_constant<int, 2 * PSTEP>{}, std::integral_constant<int, 2 * NTAP>{});
        }

        // the MFMAs are inline assembly, so the compiler does not pad their result latency: an MFMA's result may be read by another
        // instruction only some wait states after it issues (ISA "required independent instructions": up to 19), and the
        // exchange below reads the accumulators of the last step straight away.  24 wait states, once per tile
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (st_) SPEI_STAMP(p.stamps, 2);
        // ---- K-half exchange: hand the partner wave (same n-tile, other half) the rows it finishes --------------------------------------
        // layout [wave][row j < 3][quadruple g][lane] x 16 B: consecutive lanes, consecutive 16 bytes
        {
            f32x4* x = reinterpret_cast<f32x4*>(xch + wave * XCH_WAVE) + lane;
#pragma unroll
            for (int j = 0; j < HR; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    x[(j * 4 + g) * 64] = f32x4{acc[HR + j][4 * g], acc[HR + j][4 * g + 1], acc[HR + j][4 * g + 2], acc[HR + j][4 * g + 3]};
        }
        lds_barrier();
        if (st_) SPEI_STAMP(p.stamps, 3);
        // ---- epilogue: rows [3h, 3h + 3) of n-tile nt, channel quadruples of one pixel per lane ------------------------------------------
        {
            int b, oy0, ox0;
            tile_origin(t, b, oy0, ox0);
            TO* ob = static_cast<TO*>(p.out) + (size_t)b * map_elems;
            const int ox = ox0 + fr;
            const f32x4* x = reinterpret_cast<const f32x4*>(xch + (wave ^ 1) * XCH_WAVE) + lane;
#pragma unroll
            for (int j = 0; j < HR; ++j) {
                const int oy = oy0 + kh * HR + j;
                if (oy < p.H && ox < p.W) {
                    TO* o = ob + ((size_t)oy * p.W + ox) * C + 32 * nt + 4 * fk;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 q = x[(j * 4 + g) * 64];
                        f32x4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            v[e] = acc[j][4 * g + e] + q[e] + biasv[4 * g + e];       // (one addition: the same either way round)
                            if (p.act == SPEI_ACT_RELU) v[e] = fmaxf(v[e], 0.f);
                        }
                        if constexpr (sizeof(TO) == 4) *reinterpret_cast<f32x4*>(o + 8 * g) = v;
                        else *reinterpret_cast<lp4*>(o + 8 * g) = to_lp4<LP>(v);
                    }
                }
            }
        }
        if (st_) SPEI_STAMP(p.stamps, 4);
        if (NPH > 1) store_slab(tl, buf ^ 1, NPH - 1, 0, NITH);         // (the last tile re-stages itself into the idle buffer: never read)
        else store_slab(tl, buf ^ 1, 0, (NTAP + 1) / 2, NITH);          // whatever the loop's 13 slots did not cover (nothing: 12 chunks)
        lds_barrier();                                                  // the next slab is complete; the exchange has been read
        if (st_) SPEI_STAMP(p.stamps, 5);
    }
}

template <typename LP>
int launch_ws(const WsParams& p, int a16, int o16, hipStream_t st) {
    const size_t lds = LDS_BYTES;
    const int cus = spei_num_cus();
    const dim3 grid(p.total < cus ? p.total : cus);
    if (a16 && o16) {
        ensure_dyn_lds<&conv64_ws_kernel<LP, LP, LP>>(lds);
        hipLaunchKernelGGL((conv64_ws_kernel<LP, LP, LP>), grid, dim3(NTHR), lds, st, p);
    } else if (!a16 && o16) {
        ensure_dyn_lds<&conv64_ws_kernel<LP, float, LP>>(lds);
        hipLaunchKernelGGL((conv64_ws_kernel<LP, float, LP>), grid, dim3(NTHR), lds, st, p);
    } else if (a16 && !o16) {
        ensure_dyn_lds<&conv64_ws_kernel<LP, LP, float>>(lds);
        hipLaunchKernelGGL((conv64_ws_kernel<LP, LP, float>), grid, dim3(NTHR), lds, st, p);
    } else {
        ensure_dyn_lds<&conv64_ws_kernel<LP, float, float>>(lds);
        hipLaunchKernelGGL((conv64_ws_kernel<LP, float, float>), grid, dim3(NTHR), lds, st, p);
    }
    return 0;
}

}  // namespace

extern "C" int spei_conv64_ws16(int fmt, const void* a, int a_fmt, const void* wfrag, const float* bias, void* out, int out_fmt, int batch,
                                int H, int W, int act, spei_stream_t stream) {
    SPEI_REQUIRE(a && wfrag && out, "spei_conv64_ws16: null pointer");
    SPEI_REQUIRE((fmt == SPEI_BF16 || fmt == SPEI_F16) && (a_fmt == SPEI_F32 || a_fmt == fmt) && (out_fmt == SPEI_F32 || out_fmt == fmt),
                 "spei_conv64_ws16: fmt=%d a_fmt=%d out_fmt=%d", fmt, a_fmt, out_fmt);
    SPEI_REQUIRE(batch >= 1 && H > 0 && W > 0 && (int64_t)batch * cdiv(H, TH) * cdiv(W, TW) < (1ll << 30) && (int64_t)H * W < (1ll << 26),
                 "spei_conv64_ws16: batch=%d of %dx%d", batch, H, W);
    SPEI_REQUIRE(act == SPEI_ACT_NONE || act == SPEI_ACT_RELU, "spei_conv64_ws16: act=%d", act);
    SPEI_REQUIRE(((uintptr_t)a | (uintptr_t)wfrag | (uintptr_t)out) % 16 == 0 && a != out, "spei_conv64_ws16: 16-byte alignment, out must not be the input");
    WsParams p;
    p.a = a; p.wfrag = wfrag; p.bias = bias; p.out = out; p.H = H; p.W = W; p.batch = batch; p.act = act;
    p.tiles_x = cdiv(W, TW); p.tiles_y = cdiv(H, TH); p.total = batch * p.tiles_x * p.tiles_y;
    p.stamps = spei_stamp_buffer();
    hipStream_t st = (hipStream_t)stream;
    const int a16 = a_fmt != SPEI_F32, o16 = out_fmt != SPEI_F32;
    const int rc = fmt == SPEI_F16 ? launch_ws<_Float16>(p, a16, o16, st) : launch_ws<__bf16>(p, a16, o16, st);
    if (rc) return rc;
    SPEI_CHECK_LAUNCH("spei_conv64_ws16");
    return 0;
}
