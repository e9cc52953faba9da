// Window attention of the training step in bf16 (speinet_amd/train.py `train_precision = "bf16"`; model/swinir.py:115-149 forward and,
// under loss.backward(), its gradient): the decomposition of swin.hip / swin_bwd.hip — two 256-thread workgroups per 5x5 window, one
// wave per head, 25 tokens padded to 32, one 32 x 32 tile per (window, head) — with every product on v_mfma_f32_32x32x16_bf16 instead of
// v_mfma_f32_32x32x2_f32 (two MFMAs per 32 x 32 x 32 product instead of sixteen).
//
// Arithmetic contract: q, k, v, dO rounded once to bf16 (round to nearest even) while they are staged into LDS; softmax, relative bias,
// shift mask, the row term r_q and dS = P (dP - r_q) in fp32; P and dS rounded to bf16 only where they are an MFMA operand; fp32
// accumulation; the relative-bias gradient (dbias_part) is the fp32 dS.
//
// Operand layout of v_mfma_f32_32x32x16_bf16: lane (i = lane % 32, h = lane / 32) holds A[i][8h .. 8h+7] and B[8h .. 8h+7][i]; the
// accumulator register r of lane (j, h) is C[(r & 3) + 8 (r >> 2) + 4 h][j].  An accumulator used as the next product's A operand
// (the P / dS registers, contracted over their rows) therefore supplies, in step s, element e of lane half h = row key(h, 8 s + e)
// = 16 s + 8 (e >> 2) + 4 h + (e & 3): every row once over the two steps.  The B operand is gathered from LDS with the same row map,
// so each product pairs the right terms (the contraction order is a permutation, the sum is the same one).
#include "common.h"

namespace {

constexpr int WS = 5, NT = 25, HD = 32;
constexpr int HP = HD + 8;                  // bf16 row pitch: 80 bytes, an odd multiple of 16 (conflict-free ds_read_b128)
typedef lpv<__bf16>::x8 bf8;

__device__ __forceinline__ int mask_region(int v, int n, int shift) { return v < n - WS ? 0 : (v < n - shift ? 1 : 2); }
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// token -> pixel of the window (cyclic shift folded in) and its shift-mask region; the first 32 threads
__device__ __forceinline__ void window_tokens(int* tok_pix, int* tok_reg, int H, int W, int shift) {
    const int nwx = W / WS;
    const int win = blockIdx.x >> 1;
    const int wy = win / nwx, wx = win - wy * nwx;
    if (threadIdx.x < 32) {
        int pix = 0, reg = 0;
        if (threadIdx.x < NT) {
            const int ys = wy * WS + threadIdx.x / WS, xs = wx * WS + threadIdx.x % WS;   // shifted-frame coords
            int yo = ys + shift, xo = xs + shift;                                         // roll(-shift)
            if (yo >= H) yo -= H;
            if (xo >= W) xo -= W;
            pix = yo * W + xo;
            reg = shift > 0 ? 3 * mask_region(ys, H, shift) + mask_region(xs, W, shift) : 0;
        }
        tok_pix[threadIdx.x] = pix;
        tok_reg[threadIdx.x] = reg;
    }
}

// 32 rows x 32 fp32 of one head -> bf16 rows of pitch HP (rows >= 25 zero); `ld` floats per pixel row, `col` the head's first column
__device__ __forceinline__ void stage_rows(__bf16 (*dst)[HP], const float* src, int ld, int col, const int* tok_pix, int lane) {
    for (int i = lane; i < 32 * 8; i += 64) {
        const int r = i >> 3, c4 = (i & 7) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (r < NT) v = *reinterpret_cast<const f32x4*>(src + (size_t)tok_pix[r] * ld + col + c4);
        *reinterpret_cast<lpv<__bf16>::x4*>(&dst[r][c4]) = to_lp4<__bf16>(v);
    }
}

// C += A B^T over the 32 head dims: A, B rows from LDS (lane i reads row i)
__device__ __forceinline__ f32x16 rows_product(const __bf16 (*a)[HP], const __bf16 (*b)[HP], int fr, int fk, f32x16 c) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
        c = mfma16(*reinterpret_cast<const bf8*>(&a[fr][16 * s + 8 * fk]), *reinterpret_cast<const bf8*>(&b[fr][16 * s + 8 * fk]), c);
    return c;
}

// C += X M: X given as accumulator registers (lane i = row of C, registers = contraction index), M [32][HP] in LDS (column = lane)
__device__ __forceinline__ f32x16 regs_product(const f32x16 x, const __bf16 (*m)[HP], int fr, int fk, f32x16 c) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        bf8 a, b;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            a[e] = (__bf16)x[8 * s + e];
            b[e] = m[acc_row(8 * s + e, fk)][fr];
        }
        c = mfma16(a, b, c);
    }
    return c;
}

__global__ __launch_bounds__(256) void window_attention16_train_kernel(const float* __restrict__ q, const float* __restrict__ kv,
                                                                       const float* __restrict__ relbias, float* __restrict__ out,
                                                                       int H, int W, int shift) {
    __shared__ __attribute__((aligned(16))) __bf16 sQ[4][32][HP], sK[4][32][HP], sV[4][32][HP];
    __shared__ int tok_pix[32], tok_reg[32];
    {
        const size_t z = (size_t)blockIdx.y * H * W;
        q += z * 256; kv += z * 512; out += z * 256;
    }
    window_tokens(tok_pix, tok_reg, H, W, shift);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int h = (blockIdx.x & 1) * 4 + wave, hl = wave;
    stage_rows(sQ[hl], q, 256, h * HD, tok_pix, lane);
    stage_rows(sK[hl], kv, 512, h * HD, tok_pix, lane);
    stage_rows(sV[hl], kv, 512, 256 + h * HD, tok_pix, lane);
    __syncthreads();
    const int fr = lane & 31, fk = lane >> 5;
    f32x16 st;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
    st = rows_product(sK[hl], sQ[hl], fr, fk, st);           // S^T: lane = query fr, registers = keys
    const int qi = fr < NT ? fr : 0;
    const int qreg = tok_reg[qi];
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int key = acc_row(r, fk);
        float v = -INFINITY;
        if (key < NT) {
            v = st[r] + relbias[(h * NT + qi) * NT + key];
            if (shift > 0 && tok_reg[key] != qreg) v += -100.0f;
        }
        st[r] = v;
        mx = fmaxf(mx, v);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float e = expf(st[r] - mx);
        st[r] = e;
        sum += e;
    }
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] *= inv;               // P (fp32; rounded to bf16 as the operand of O = P V)
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    o = regs_product(st, sV[hl], fr, fk, o);                 // O: column d = fr, rows = queries
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int qq = acc_row(r, fk);
        if (qq < NT) out[(size_t)tok_pix[qq] * 256 + h * HD + fr] = o[r];
    }
}

// Backward: the two passes of swin_bwd.hip.  Pass T (lane = query, registers = keys): S^T, P, dP^T = V dO^T, r_q, dS; dbias_part and
// dQ = dS K.  Pass N (lane = key, registers = queries): S, P from pass T's row statistics, dP = dO V^T, dS; dV = P^T dO, dK = dS^T Q.
__global__ __launch_bounds__(256) void window_attention16_bwd_kernel(const float* __restrict__ q, const float* __restrict__ kv,
                                                                     const float* __restrict__ relbias, const float* __restrict__ dout,
                                                                     float* __restrict__ dq, float* __restrict__ dkv,
                                                                     float* __restrict__ dbias_part, int H, int W, int shift) {
    __shared__ __attribute__((aligned(16))) __bf16 sQ[4][32][HP], sK[4][32][HP], sV[4][32][HP], sD[4][32][HP];
    __shared__ float stat[4][3][32];                          // per head: row max, 1 / row sum, r_q
    __shared__ int tok_pix[32], tok_reg[32];
    {
        const size_t z = (size_t)blockIdx.y * H * W;
        q += z * 256; kv += z * 512; dout += z * 256; dq += z * 256; dkv += z * 512;
        dbias_part += (size_t)blockIdx.y * (H / WS) * (W / WS) * 8 * NT * NT;
    }
    window_tokens(tok_pix, tok_reg, H, W, shift);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int h = (blockIdx.x & 1) * 4 + wave, hl = wave;
    const int win = blockIdx.x >> 1;
    stage_rows(sQ[hl], q, 256, h * HD, tok_pix, lane);
    stage_rows(sK[hl], kv, 512, h * HD, tok_pix, lane);
    stage_rows(sV[hl], kv, 512, 256 + h * HD, tok_pix, lane);
    stage_rows(sD[hl], dout, 256, h * HD, tok_pix, lane);
    __syncthreads();
    const int fr = lane & 31, fk = lane >> 5;
    float* smx = stat[hl][0];
    float* sinv = stat[hl][1];
    float* srq = stat[hl][2];

    // ---- pass T: lane = query fr, register r = key acc_row(r, fk) ----------------------------------------------------------------
    {
        f32x16 st, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { st[r] = 0.f; dp[r] = 0.f; }
        st = rows_product(sK[hl], sQ[hl], fr, fk, st);
        dp = rows_product(sV[hl], sD[hl], fr, fk, dp);
        const int qi = fr < NT ? fr : 0;
        const int qreg = tok_reg[qi];
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = acc_row(r, fk);
            float v = -INFINITY;
            if (key < NT) {
                v = st[r] + relbias[(h * NT + qi) * NT + key];
                if (shift > 0 && tok_reg[key] != qreg) v += -100.0f;
            }
            st[r] = v;
            mx = fmaxf(mx, v);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = expf(st[r] - mx);
            st[r] = e;
            sum += e;
        }
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.0f / sum;
        float rq = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            st[r] *= inv;
            rq += st[r] * dp[r];
        }
        rq += __shfl_xor(rq, 32, 64);
        if (fk == 0) { smx[fr] = mx; sinv[fr] = inv; srq[fr] = rq; }
        float* bp = dbias_part + ((size_t)win * 8 + h) * NT * NT;
        f32x16 ds;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = acc_row(r, fk);
            const bool ok = fr < NT && key < NT;
            ds[r] = ok ? st[r] * (dp[r] - rq) : 0.f;
            if (ok) bp[fr * NT + key] = ds[r];
        }
        f32x16 dqa;
#pragma unroll
        for (int r = 0; r < 16; ++r) dqa[r] = 0.f;
        dqa = regs_product(ds, sK[hl], fr, fk, dqa);           // dQ[query][d] = sum_key dS K
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qq = acc_row(r, fk);
            if (qq < NT) dq[(size_t)tok_pix[qq] * 256 + h * HD + fr] = dqa[r];
        }
    }
    __syncthreads();                                          // pass T's row statistics in LDS

    // ---- pass N: lane = key fr, register r = query acc_row(r, fk) ----------------------------------------------------------------
    {
        f32x16 st, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { st[r] = 0.f; dp[r] = 0.f; }
        st = rows_product(sQ[hl], sK[hl], fr, fk, st);
        dp = rows_product(sD[hl], sV[hl], fr, fk, dp);
        const int key = fr;
        const int kreg = tok_reg[key < NT ? key : 0];
        f32x16 pv, ds;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qq = acc_row(r, fk);
            float p_ = 0.f, d_ = 0.f;
            if (qq < NT && key < NT) {
                float v = st[r] + relbias[(h * NT + qq) * NT + key];
                if (shift > 0 && tok_reg[qq] != kreg) v += -100.0f;
                p_ = expf(v - smx[qq]) * sinv[qq];
                d_ = p_ * (dp[r] - srq[qq]);
            }
            pv[r] = p_;
            ds[r] = d_;
        }
        f32x16 dva, dka;
#pragma unroll
        for (int r = 0; r < 16; ++r) { dva[r] = 0.f; dka[r] = 0.f; }
        dva = regs_product(pv, sD[hl], fr, fk, dva);           // dV[key][d] = sum_query P dO
        dka = regs_product(ds, sQ[hl], fr, fk, dka);           // dK[key][d] = sum_query dS Q
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kk = acc_row(r, fk);
            if (kk < NT) {
                dkv[(size_t)tok_pix[kk] * 512 + h * HD + fr] = dka[r];
                dkv[(size_t)tok_pix[kk] * 512 + 256 + h * HD + fr] = dva[r];
            }
        }
    }
}

}  // namespace

extern "C" int spei_window_attention16_train(const float* q, const float* kv, const float* relbias, float* out, int H, int W, int shift, int batch,
                                             spei_stream_t stream) {
    SPEI_REQUIRE(q && kv && relbias && out, "spei_window_attention16_train: null pointer");
    SPEI_REQUIRE(batch >= 1 && batch <= 65535, "spei_window_attention16_train: batch=%d", batch);
    SPEI_REQUIRE(H > 0 && W > 0 && H % WS == 0 && W % WS == 0, "spei_window_attention16_train: %dx%d is not a multiple of the 5x5 window", H, W);
    SPEI_REQUIRE(shift >= 0 && shift < WS, "spei_window_attention16_train: shift=%d", shift);
    SPEI_REQUIRE((int64_t)H * W * 512 < (1ll << 31), "spei_window_attention16_train: map too large");
    SPEI_REQUIRE(((uintptr_t)q | (uintptr_t)kv) % 16 == 0, "spei_window_attention16_train: q / kv must be 16-byte aligned");
    hipLaunchKernelGGL(window_attention16_train_kernel, dim3(2 * (H / WS) * (W / WS), batch), dim3(256), 0, (hipStream_t)stream, q, kv, relbias, out,
                       H, W, shift);
    SPEI_CHECK_LAUNCH("spei_window_attention16_train");
    return 0;
}

extern "C" int spei_window_attention16_bwd(const float* q, const float* kv, const float* relbias, const float* dout, float* dq, float* dkv,
                                           float* dbias_part, int H, int W, int shift, int batch, spei_stream_t stream) {
    SPEI_REQUIRE(q && kv && relbias && dout && dq && dkv && dbias_part, "spei_window_attention16_bwd: null pointer");
    SPEI_REQUIRE(batch >= 1 && batch <= 65535, "spei_window_attention16_bwd: batch=%d", batch);
    SPEI_REQUIRE(H > 0 && W > 0 && H % WS == 0 && W % WS == 0, "spei_window_attention16_bwd: %dx%d is not a multiple of the 5x5 window", H, W);
    SPEI_REQUIRE(shift >= 0 && shift < WS, "spei_window_attention16_bwd: shift=%d", shift);
    SPEI_REQUIRE((int64_t)H * W * 512 < (1ll << 31), "spei_window_attention16_bwd: map too large");
    SPEI_REQUIRE(((uintptr_t)q | (uintptr_t)kv | (uintptr_t)dout) % 16 == 0, "spei_window_attention16_bwd: q / kv / dout must be 16-byte aligned");
    hipLaunchKernelGGL(window_attention16_bwd_kernel, dim3(2 * (H / WS) * (W / WS), batch), dim3(256), 0, (hipStream_t)stream, q, kv, relbias,
                       dout, dq, dkv, dbias_part, H, W, shift);
    SPEI_CHECK_LAUNCH("spei_window_attention16_bwd");
    return 0;
}
