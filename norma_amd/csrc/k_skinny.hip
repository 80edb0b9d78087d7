// k_skinny.hip -- the decode step's GEMV kernels (gfx950).  HBM-bound: the weights and the tied embedding are streamed once
// per generated token for the whole batch.
//
// Replaces, per decode step of Model::decode (src/models/whisper/model.rs:317-371):
//   skinny_gemm_kernel   candle Linear matmuls of TextDecoder::forward and final_linear for the
//                        newest position only (the reference recomputes the whole prefix: it has
//                        no self-attention KV cache; a cache is mathematically identical)
// Which kernel runs for a shape is skinny_plan (skinny_plan.h); launch_skinny at the end of this file is its switch.
#include <type_traits>

#include "nh_kernels.h"

__device__ __forceinline__ float gelu_tanh_d(float v) { return gelu_tanh_fast(v); }

// ---------------------------------------------------------------------------------------------------
// skinny GEMM: y[R][N] = x[R][K] . W[N][K]^T, R <= 96.  Weights are the MFMA A operand (16 rows per
// tile; each lane streams 16 B of one weight row per k-step, 4 lanes cover a 64 B run), activations
// (L2-resident) the B operand.  Two shapes of the same kernel:
//   KSPLIT = 2 .. 16 : one 16-row tile per workgroup, its KSPLIT waves split K, fp32 partials meet in
//                    LDS (small N: many waves in flight instead of few long ones; the long-K fc2 layer
//                    takes 16 waves so that every wave still has ONE group of <= 10 k-steps in flight);
//   KSPLIT = 1     : every wave owns NT 16-row tiles over the full K, no LDS (the 51866-row logits).
// Up to 8 k-steps of loads are in flight per wave before the first MFMA of a group.
// ---------------------------------------------------------------------------------------------------
#define SK_U 10

// has_pre: bias (and, for SK_RESID_F32, the residual) were fetched at kernel start into pre0, pre1
__device__ __forceinline__ void skinny_store(const SkinnyParams &p, f32x4 v, int r, int n, bool has_pre = false,
                                             f32x4 pre0 = (f32x4){0.f, 0.f, 0.f, 0.f}, f32x4 pre1 = (f32x4){0.f, 0.f, 0.f, 0.f}) {
    if (n >= p.N) return;
    if (has_pre) v += pre0;
    else if (p.bias) {
        if (n + 3 < p.N) v += *reinterpret_cast<const f32x4 *>(p.bias + n);
        else for (int i = 0; i < 4 && n + i < p.N; i++) v[i] += p.bias[n + i];
    }
    if (p.epi == SK_F32) {
        float *dst = reinterpret_cast<float *>(p.out[0]) + (long)r * p.ldo + n;
        if (n + 3 < p.N) *reinterpret_cast<f32x4 *>(dst) = v;
        else for (int i = 0; i < 4 && n + i < p.N; i++) dst[i] = v[i];
        return;
    }
    // the remaining epilogues have N % 4 == 0
    if (p.epi == SK_RESID_F32) {
        float *dst = reinterpret_cast<float *>(p.out[0]) + (long)r * p.ldo + n;
        f32x4 x = has_pre ? pre1 : *reinterpret_cast<const f32x4 *>(dst);
        *reinterpret_cast<f32x4 *>(dst) = x + v;
        return;
    }
    if (p.epi == SK_GELU_F16) { v[0] = gelu_tanh_d(v[0]); v[1] = gelu_tanh_d(v[1]); v[2] = gelu_tanh_d(v[2]); v[3] = gelu_tanh_d(v[3]); }
    half4 hv = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
    if (p.epi == SK_QKV) {
        const int sg = n / p.d, nl = n - sg * p.d;
        const int b = r / p.Tn, i = r - b * p.Tn;
        half_t *dst;
        if (sg == 0) dst = reinterpret_cast<half_t *>(p.out[0]) + (long)r * p.d + nl;
        else {
            const int t0 = p.pos_ptr ? p.pos_ptr[b] : p.t0;  // per-sequence position (decode pool / hipGraph replay)
            // self-attention K/V cache, head-major [b][h][ctx][64]: the keys of one (clip, head) are contiguous for dec_attn_kernel
            dst = reinterpret_cast<half_t *>(sg == 1 ? p.out[1] : p.out[2]) +
                  (((long)b * (p.d >> 6) + (nl >> 6)) * p.ctx + t0 + i) * NH_DH + (nl & 63);
        }
        *reinterpret_cast<half4 *>(dst) = hv;
        return;
    }
    *reinterpret_cast<half4 *>(reinterpret_cast<half_t *>(p.out[0]) + (long)r * p.ldo + n) = hv;
}

// U k-steps of one wave: all loads issued back to back (never guarded: a guarded load makes hipcc drain
// vmcnt(0) per element), then the MFMAs.  The callers cover `steps` with groups of 10, 5, 2 and 1.
template <int U, int NT, int NCB>
__device__ __forceinline__ void skinny_group(const half_t *const (&wp)[NT], int wstep, const half_t *const (&xp)[NCB], int s0,
                                             f32x4 (&acc)[NT][NCB]) {
    half8 a[NT][U], b[NCB][U];
#pragma unroll
    for (int u = 0; u < U; u++) {
#pragma unroll
        for (int t = 0; t < NT; t++) a[t][u] = *reinterpret_cast<const half8 *>(wp[t] + (long)wstep * (s0 + u));
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) b[cb][u] = *reinterpret_cast<const half8 *>(xp[cb] + 32 * (s0 + u));
    }
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int cb = 0; cb < NCB; cb++)
                acc[t][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[t][u], b[cb][u], acc[t][cb], 0, 0, 0);
}

template <int NCB, int KSPLIT, int NT>
__global__ __launch_bounds__(KSPLIT == 1 ? 128 : 64 * KSPLIT) void skinny_gemm_kernel(SkinnyParams p) {
    constexpr int NW = KSPLIT == 1 ? 2 : KSPLIT;  // waves per workgroup
    __shared__ f32x4 red[KSPLIT == 1 ? 1 : KSPLIT][NCB][64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    // tile base row of this wave
    const int n0 = KSPLIT == 1 ? (blockIdx.x * NW + w) * 16 * NT : blockIdx.x * 16;
    // gridDim.y > 1: workgroup y handles activation rows rb .. rb + 16 NCB only (every CU must fetch the activation rows it
    // multiplies, and that fetch -- 35-47 KB/us per CU -- is what these kernels wait for: with few weight tiles it pays to
    // spread the ROWS over more CUs too; per-row arithmetic is unchanged, so results are)
    const int rb = blockIdx.y * 16 * NCB;
    // epilogue operands (bias, residual) of the element this thread will own: fetched now, so their latency
    // hides under the weight stream instead of extending the dependent chain of this latency-bound kernel
    f32x4 pre[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const bool can_pre = KSPLIT != 1 && (p.N & 3) == 0;
    if (can_pre) {
        const int er = rb + (tid >> 2), en = n0 + 4 * (tid & 3);
        if (tid < 64 * NCB && er < p.R && en < p.N) {
            if (p.bias) pre[0] = *reinterpret_cast<const f32x4 *>(p.bias + en);
            if (p.epi == SK_RESID_F32) pre[1] = *reinterpret_cast<const f32x4 *>(reinterpret_cast<const float *>(p.out[0]) + (long)er * p.ldo + en);
        }
    }
    const int kslice = p.K / KSPLIT, kbeg = KSPLIT == 1 ? 0 : w * kslice;
    // weights: row-major [N][K] (a wave instruction = 16 rows x 64 B) or the tile-major repack (1 KiB contiguous)
    const half_t *wp[NT];
    const int wstep = p.Wt ? 512 : 32;
#pragma unroll
    for (int t = 0; t < NT; t++) {
        int wrow = n0 + 16 * t + fr; if (wrow >= p.N) wrow = p.N - 1;
        wp[t] = p.Wt ? p.Wt + ((long)((n0 >> 4) + t) * (p.K >> 5) + (kbeg >> 5)) * 512 + lane * 8
                     : p.W + (long)wrow * p.K + kbeg + 8 * fq;
    }
    const half_t *xp[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) {
        int r = rb + 16 * cb + fr; if (r >= p.R) r = p.R - 1;
        xp[cb] = p.x + (long)r * p.ldx + kbeg + 8 * fq;
    }
    f32x4 acc[NT][NCB];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) acc[t][cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int steps = kslice >> 5;
    {
        int s0 = 0;
        for (; s0 + 10 <= steps; s0 += 10) skinny_group<10, NT, NCB>(wp, wstep, xp, s0, acc);
        if (s0 + 5 <= steps) { skinny_group<5, NT, NCB>(wp, wstep, xp, s0, acc); s0 += 5; }
        for (; s0 + 2 <= steps; s0 += 2) skinny_group<2, NT, NCB>(wp, wstep, xp, s0, acc);
        if (s0 < steps) skinny_group<1, NT, NCB>(wp, wstep, xp, s0, acc);
    }
    if (KSPLIT == 1) {
        // D[n = 4 fq + i][r = 16 cb + fr]: each lane already holds 4 consecutive features of one row
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int cb = 0; cb < NCB; cb++) {
                int r = rb + 16 * cb + fr;
                if (r < p.R) skinny_store(p, acc[t][cb], r, n0 + 16 * t + 4 * fq);
            }
        return;
    }
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) red[w][cb][lane] = acc[0][cb];
    __syncthreads();
    // thread t owns row r = t / 4 and the 4 consecutive features n0 + 4 (t % 4) + i:
    // D[n = 4 fq + i][r = fr] lives in lane 16 fq + fr of column block r / 16
    const int rl = tid >> 2, nq = tid & 3, r = rb + rl;
    const bool owner = (tid < 64 * NCB) && (r < p.R);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (owner) {
        const int src_lane = 16 * nq + (rl & 15), cb = rl >> 4;
        v = red[0][cb][src_lane];
#pragma unroll
        for (int ww = 1; ww < KSPLIT; ww++) v += red[ww][cb][src_lane];
    }
    if (owner) skinny_store(p, v, r, n0 + 4 * nq, can_pre, pre[0], pre[1]);
}

// ---------------------------------------------------------------------------------------------------
// LayerNorm fused into the skinny GEMM (K = 128 STEPS, R <= 32): the 5.4 us LayerNorm launch in front of every
// q|k|v, cross-q and fc1 projection of a decode step is pure latency (160 KB in, 80 KB out), so each workgroup
// normalises the rows itself while its weight tile is in flight.  Wave w owns K-slice w: its lanes already load
// exactly the x elements of their B fragments (row 16 cb + fr, columns kbeg + 32 s + 8 fq .. + 8), as f32 from the
// residual stream; the row statistics meet through LDS (two passes over the register-resident values, the "sliced"
// summation tree of nh_kernels.h), gamma/beta are staged in LDS once per workgroup.
// ---------------------------------------------------------------------------------------------------
template <int STEPS, int NT>
__global__ __launch_bounds__(256) void skinny_ln_kernel(SkinnyParams p) {
    constexpr int K = 128 * STEPS;
    constexpr int NCB = 1;   // one 16-row activation block per workgroup; gridDim.y row blocks (skinny_plan)
    __shared__ f32x4 red[4][NT][NCB][64];
    __shared__ float part[2][4][NCB][16];
    __shared__ __attribute__((aligned(16))) float gb[2][K];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    // A workgroup owns NT consecutive 16-row weight tiles and the activation rows rb .. rb + 16 NCB (gridDim.y row blocks).
    // What it waits for is its own fetch (35-47 KB/us per CU): NT x 41 KB of weights + 16 NCB rows x K f32 of activations,
    // so the launcher shapes (NT, NCB, grid) to keep that sum small while every CU has work.
    const int tiles = (p.N + 15) >> 4, tile0 = blockIdx.x * NT;
    const int rb = blockIdx.y * 16 * NCB;
    const int kbeg = w * 32 * STEPS;
    // weights first: the only HBM stream of the kernel
    const int wstep = p.Wt ? 512 : 32;
    half8 a[NT][STEPS];
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int tile = tile0 + t < tiles ? tile0 + t : tiles - 1;   // a tail workgroup re-reads the last tile; its stores are skipped
        int wrow = tile * 16 + fr; if (wrow >= p.N) wrow = p.N - 1;
        const half_t *wp = p.Wt ? p.Wt + ((long)tile * (K >> 5) + (kbeg >> 5)) * 512 + lane * 8 : p.W + (long)wrow * K + kbeg + 8 * fq;
#pragma unroll
        for (int s = 0; s < STEPS; s++) a[t][s] = *reinterpret_cast<const half8 *>(wp + wstep * s);
    }
    // epilogue operands of the elements this thread will own (see skinny_gemm_kernel)
    f32x4 pre[NT][2];
    const bool can_pre = (p.N & 3) == 0;
#pragma unroll
    for (int t = 0; t < NT; t++) {
        pre[t][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; pre[t][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (can_pre) {
            const int er = rb + (tid >> 2), en = (tile0 + t) * 16 + 4 * (tid & 3);
            if (tid < 64 * NCB && er < p.R && en < p.N) {
                if (p.bias) pre[t][0] = *reinterpret_cast<const f32x4 *>(p.bias + en);
                if (p.epi == SK_RESID_F32) pre[t][1] = *reinterpret_cast<const f32x4 *>(reinterpret_cast<const float *>(p.out[0]) + (long)er * p.ldo + en);
            }
        }
    }
    // the rows, f32
    f32x4 xv[NCB][STEPS][2];
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) {
        int r = rb + 16 * cb + fr; if (r >= p.R) r = p.R - 1;
        const float *xr = p.ln_x + (long)r * K + kbeg + 8 * fq;
#pragma unroll
        for (int s = 0; s < STEPS; s++) {
            xv[cb][s][0] = *reinterpret_cast<const f32x4 *>(xr + 32 * s);
            xv[cb][s][1] = *reinterpret_cast<const f32x4 *>(xr + 32 * s + 4);
        }
    }
    for (int c = tid; c < K / 4; c += 256) {
        reinterpret_cast<f32x4 *>(gb[0])[c] = reinterpret_cast<const f32x4 *>(p.ln_w)[c];
        reinterpret_cast<f32x4 *>(gb[1])[c] = reinterpret_cast<const f32x4 *>(p.ln_b)[c];
    }
    float mean[NCB], inv[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) {
        float s1 = 0.f;
#pragma unroll
        for (int s = 0; s < STEPS; s++) s1 = ln_sum8(s1, xv[cb][s][0], xv[cb][s][1]);
        s1 += __shfl_xor(s1, 16); s1 += __shfl_xor(s1, 32);
        if (fq == 0) part[0][w][cb][fr] = s1;
    }
    __syncthreads();
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) {
        mean[cb] = ln_mean((part[0][0][cb][fr] + part[0][1][cb][fr]) + (part[0][2][cb][fr] + part[0][3][cb][fr]), p.ln_rk);
        float s2 = 0.f;
#pragma unroll
        for (int s = 0; s < STEPS; s++) s2 = ln_sq8(s2, xv[cb][s][0], xv[cb][s][1], mean[cb]);
        s2 += __shfl_xor(s2, 16); s2 += __shfl_xor(s2, 32);
        if (fq == 0) part[1][w][cb][fr] = s2;
    }
    __syncthreads();
    f32x4 acc[NT][NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) {
        inv[cb] = ln_inv((part[1][0][cb][fr] + part[1][1][cb][fr]) + (part[1][2][cb][fr] + part[1][3][cb][fr]), p.ln_rk);
#pragma unroll
        for (int t = 0; t < NT; t++) acc[t][cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int s = 0; s < STEPS; s++) {
        const int k = kbeg + 32 * s + 8 * fq;
        const f32x4 g0 = *reinterpret_cast<const f32x4 *>(&gb[0][k]), g1 = *reinterpret_cast<const f32x4 *>(&gb[0][k + 4]);
        const f32x4 b0 = *reinterpret_cast<const f32x4 *>(&gb[1][k]), b1 = *reinterpret_cast<const f32x4 *>(&gb[1][k + 4]);
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) {
            const f32x4 o0 = ln_apply(xv[cb][s][0], mean[cb], inv[cb], g0, b0);
            const f32x4 o1 = ln_apply(xv[cb][s][1], mean[cb], inv[cb], g1, b1);
            const half8 b = {(half_t)o0[0], (half_t)o0[1], (half_t)o0[2], (half_t)o0[3],
                             (half_t)o1[0], (half_t)o1[1], (half_t)o1[2], (half_t)o1[3]};
#pragma unroll
            for (int t = 0; t < NT; t++) acc[t][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[t][s], b, acc[t][cb], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) red[w][t][cb][lane] = acc[t][cb];
    __syncthreads();
    const int rl = tid >> 2, nq = tid & 3, r = rb + rl;
    if (tid < 64 * NCB && r < p.R) {
        const int src_lane = 16 * nq + (rl & 15), cb = rl >> 4;
#pragma unroll
        for (int t = 0; t < NT; t++) {
            if (tile0 + t >= tiles) break;
            f32x4 v = red[0][t][cb][src_lane];  // same association as skinny_gemm_kernel: the two forms give identical bits
#pragma unroll
            for (int ww = 1; ww < 4; ww++) v += red[ww][t][cb][src_lane];
            skinny_store(p, v, r, (tile0 + t) * 16 + 4 * nq, can_pre, pre[t][0], pre[t][1]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// The same LayerNorm with 16 consecutive lanes per row (lane t = 4 w + fq of the sliced tree): stand-alone kernel and
// the staging pass of the logits kernel.  K = 128 steps, steps <= 10; loads are unconditional and clamped.
// ---------------------------------------------------------------------------------------------------
struct SlicedRow { f32x4 v[LN_MAX_STEPS][2]; float mean, inv; };

__device__ __forceinline__ void sliced_row_stats(SlicedRow &sr, const float *__restrict__ xrow, int K, float rk, int t16) {
    const int steps = K >> 7, w = t16 >> 2, fq = t16 & 3;
    const float *xr = xrow + w * 32 * steps + 8 * fq;
    float s1 = 0.f;
#pragma unroll
    for (int s = 0; s < LN_MAX_STEPS; s++) {
        const int sc = s < steps ? s : steps - 1;
        sr.v[s][0] = *reinterpret_cast<const f32x4 *>(xr + 32 * sc);
        sr.v[s][1] = *reinterpret_cast<const f32x4 *>(xr + 32 * sc + 4);
    }
#pragma unroll
    for (int s = 0; s < LN_MAX_STEPS; s++)
        if (s < steps) s1 = ln_sum8(s1, sr.v[s][0], sr.v[s][1]);
    s1 += __shfl_xor(s1, 1); s1 += __shfl_xor(s1, 2);   // the four lanes of a slice: (l0 + l1) + (l2 + l3)
    s1 += __shfl_xor(s1, 4); s1 += __shfl_xor(s1, 8);   // the four slices: (p0 + p1) + (p2 + p3)
    sr.mean = ln_mean(s1, rk);
    float s2 = 0.f;
#pragma unroll
    for (int s = 0; s < LN_MAX_STEPS; s++)
        if (s < steps) s2 = ln_sq8(s2, sr.v[s][0], sr.v[s][1], sr.mean);
    s2 += __shfl_xor(s2, 1); s2 += __shfl_xor(s2, 2);
    s2 += __shfl_xor(s2, 4); s2 += __shfl_xor(s2, 8);
    sr.inv = ln_inv(s2, rk);
}

__global__ __launch_bounds__(256) void layernorm_sliced_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                               const float *__restrict__ b, half_t *__restrict__ y,
                                                               float *__restrict__ y32, int M, int K, float rk) {
    const int t16 = threadIdx.x & 15;
    int row = blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = row < M;
    if (!live) row = M - 1;  // keep the 16-lane groups whole for the shuffles
    SlicedRow sr;
    sliced_row_stats(sr, x + (long)row * K, K, rk, t16);
    if (!live) return;
    const int steps = K >> 7, k0 = (t16 >> 2) * 32 * steps + 8 * (t16 & 3);
#pragma unroll
    for (int s = 0; s < LN_MAX_STEPS; s++) {
        if (s < steps) {
            const int k = k0 + 32 * s;
            const f32x4 o0 = ln_apply(sr.v[s][0], sr.mean, sr.inv, *reinterpret_cast<const f32x4 *>(w + k), *reinterpret_cast<const f32x4 *>(b + k));
            const f32x4 o1 = ln_apply(sr.v[s][1], sr.mean, sr.inv, *reinterpret_cast<const f32x4 *>(w + k + 4), *reinterpret_cast<const f32x4 *>(b + k + 4));
            const half8 h = {(half_t)o0[0], (half_t)o0[1], (half_t)o0[2], (half_t)o0[3], (half_t)o1[0], (half_t)o1[1], (half_t)o1[2], (half_t)o1[3]};
            *reinterpret_cast<half8 *>(y + (long)row * K + k) = h;
            if (y32) {
                *reinterpret_cast<f32x4 *>(y32 + (long)row * K + k) = o0;
                *reinterpret_cast<f32x4 *>(y32 + (long)row * K + k + 4) = o1;
            }
        }
    }
}

bool launch_layernorm_sliced(const float *x, const float *w, const float *b, half_t *y, float *y32, int M, int K, hipStream_t st) {
    if (K % 128 != 0 || K > 128 * LN_MAX_STEPS || M < 1) return false;
    hipLaunchKernelGGL(layernorm_sliced_kernel, dim3((M + 15) / 16), dim3(256), 0, st, x, w, b, y, y32, M, K, 1.0f / (float)K);
    return true;
}

// ---------------------------------------------------------------------------------------------------
// Large-N variant (the 51866-row tied-embedding logits): the activations are staged ONCE per workgroup
// into LDS as [k-step][row][4 chunks of 16 B] with chunk' = chunk ^ (-(row >> 2) & 3) (conflict-free
// ds_read_b128 B fragments), so the only global traffic of the main loop is the weight stream:
// every wave walks 16-row weight tiles (grid-stride), up to 10 row-segment loads in flight.
// ---------------------------------------------------------------------------------------------------
template <int NCB>
__global__ __launch_bounds__(512) void skinny_lds_kernel(SkinnyParams p) {
    extern __shared__ __attribute__((aligned(16))) char xs[];  // (K / 32) * (16 NCB) * 64 bytes
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int rows = 16 * NCB, steps = p.K >> 5;
    // Work split: every wave of the grid owns a contiguous range of weight rows, 4-row units dealt out evenly (24 or 28 rows
    // at V = 51866 over 2048 waves; whole 16-row tiles per wave left 42 % of the waves with half the work of the others).
    // A tile that sticks out of the range clamps its rows to the last one (cache hits, not HBM) and masks the stores.
    // With the tile-major repack (p.Wt: 1 KiB contiguous per wave instruction, 5.1 vs 3.7 TB/s for this stream) the unit is
    // a whole 16-row tile, dealt out round-robin.
    const int gw = blockIdx.x * 8 + w, nwav = gridDim.x * 8;
    const bool tiled = p.Wt != nullptr;
    const int units = (p.N + 3) >> 2, upw = units / nwav, uex = units % nwav;
    const int ntiles = (p.N + 15) >> 4;
    const int lo = tiled ? 16 * gw : 4 * (gw * upw + (gw < uex ? gw : uex));
    int hi = tiled ? p.N : lo + 4 * (upw + (gw < uex ? 1 : 0)); if (hi > p.N) hi = p.N;
    const int tstride = tiled ? nwav : 1;  // tile t of this wave starts at row lo + 16 t tstride
    const int my_tiles = tiled ? (gw < ntiles ? (ntiles - gw + nwav - 1) / nwav : 0) : ((hi - lo + 15) >> 4);
    const int ngrp = (steps + SK_U - 1) / SK_U;
    const int G = my_tiles * ngrp;  // (tile, k-group) pairs of this wave, k-groups innermost
    // one k-group of weight-row segments: unconditional clamped loads, all in flight together
    auto issue = [&](int g, half8 (&a)[SK_U]) {
        const int tile = g / ngrp, s0 = (g - tile * ngrp) * SK_U;
        const int row0 = lo + 16 * tile * tstride;
        int wrow = row0 + fr; if (wrow > hi - 1) wrow = hi - 1;
        const half_t *wp = tiled ? p.Wt + (long)(row0 >> 4) * steps * 512 + lane * 8 : p.W + (long)wrow * p.K + 8 * fq;
        const int wstep = tiled ? 512 : 32;
#pragma unroll
        for (int u = 0; u < SK_U; u++) {
            const int sc = s0 + u < steps ? s0 + u : steps - 1;
            a[u] = __builtin_nontemporal_load(reinterpret_cast<const half8 *>(wp + (long)wstep * sc));  // 133 MB read once per token
        }
    };
    // the first group is requested BEFORE the activations are staged (and normalised): the weights do not depend on them
    half8 a0[SK_U], a1[SK_U];
    if (G > 0) issue(0, a0);
    if (p.ln_x) {
        // fused final LayerNorm (sliced tree, 16 lanes per row, 32 rows per pass), written as the swizzled fp16 image
        for (int r = tid >> 4; r < rows; r += 32) {
            const int t16 = tid & 15, rr = r < p.R ? r : p.R - 1;
            SlicedRow sr;
            sliced_row_stats(sr, p.ln_x + (long)rr * p.K, p.K, p.ln_rk, t16);
            const int nst = p.K >> 7, k0 = (t16 >> 2) * 32 * nst + 8 * (t16 & 3);
#pragma unroll
            for (int s = 0; s < LN_MAX_STEPS; s++) {
                if (s < nst) {
                    const int k = k0 + 32 * s;
                    const f32x4 o0 = ln_apply(sr.v[s][0], sr.mean, sr.inv, *reinterpret_cast<const f32x4 *>(p.ln_w + k), *reinterpret_cast<const f32x4 *>(p.ln_b + k));
                    const f32x4 o1 = ln_apply(sr.v[s][1], sr.mean, sr.inv, *reinterpret_cast<const f32x4 *>(p.ln_w + k + 4), *reinterpret_cast<const f32x4 *>(p.ln_b + k + 4));
                    const half8 hv = {(half_t)o0[0], (half_t)o0[1], (half_t)o0[2], (half_t)o0[3], (half_t)o1[0], (half_t)o1[1], (half_t)o1[2], (half_t)o1[3]};
                    const int st = k >> 5, q = (k >> 3) & 3;
                    *reinterpret_cast<half8 *>(xs + ((long)st * rows + r) * 64 + ((q ^ ((-(r >> 2)) & 3)) << 4)) = hv;
                }
            }
        }
    } else {
        for (int c = tid; c < steps * rows * 4; c += 512) {
            const int q = c & 3, r = (c >> 2) % rows, st = (c >> 2) / rows;
            const int rr = r < p.R ? r : p.R - 1;
            const u32x4 v = *reinterpret_cast<const u32x4 *>(p.x + (long)rr * p.ldx + 32 * st + 8 * q);
            *reinterpret_cast<u32x4 *>(xs + ((long)st * rows + r) * 64 + ((q ^ ((-(r >> 2)) & 3)) << 4)) = v;
        }
    }
    __syncthreads();
    int boff[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) boff[cb] = (16 * cb + fr) * 64 + ((fq ^ ((-(fr >> 2)) & 3)) << 4);
    f32x4 acc[NCB];
    auto compute = [&](int g, const half8 (&a)[SK_U]) {
        const int tile = g / ngrp, gi = g - tile * ngrp, s0 = gi * SK_U;
        if (gi == 0) {
#pragma unroll
            for (int cb = 0; cb < NCB; cb++) acc[cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < SK_U; u++) {
            if (s0 + u < steps) {
#pragma unroll
                for (int cb = 0; cb < NCB; cb++) {
                    half8 b = *reinterpret_cast<const half8 *>(xs + (long)(s0 + u) * rows * 64 + boff[cb]);
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[u], b, acc[cb], 0, 0, 0);
                }
            }
        }
        if (gi == ngrp - 1) {
            const int n = lo + 16 * tile * tstride + 4 * fq;  // lo and hi are multiples of 4 (hi may be N itself)
            if (n < hi) {
#pragma unroll
                for (int cb = 0; cb < NCB; cb++) {
                    int r = 16 * cb + fr;
                    if (r < p.R) skinny_store(p, acc[cb], r, n);
                }
            }
        }
    };
    // two register sets: the next group is in flight while the current one is multiplied
    for (int g = 0; g < G; g += 2) {
        if (g + 1 < G) issue(g + 1, a1);
        compute(g, a0);
        if (g + 2 < G) issue(g + 2, a0);
        if (g + 1 < G) compute(g + 1, a1);
    }
}

// ---------------------------------------------------------------------------------------------------
// The same logits kernel for 33 .. 96 rows (r03: several encoder batches decoded together, nh_encode_rows): the fp16 image of
// all rows no longer fits the LDS (96 rows x 1280 x 2 B = 240 KB), so K is cut into PHASES of `sp` k-steps; the image of one
// phase is staged, every wave multiplies its (<= 2) weight tiles over that k-range into accumulators it keeps across the
// phases, barrier, next phase.  The weights are still streamed exactly once per token, and every output element is still
// accumulated over k in ascending order in one f32 accumulator: bit-identical to skinny_lds_kernel's result for the same row.
// Activations come as fp16 (LayerNorm as its own launch: the fused form would have to keep every row's statistics).
// Requires the tile-major weights and at most LP_MT tiles per wave.
// ---------------------------------------------------------------------------------------------------
template <int NCB>
__global__ __launch_bounds__(512) void skinny_ldsp_kernel(SkinnyParams p, int sp) {
    extern __shared__ __attribute__((aligned(16))) char xs[];  // sp * (16 NCB) * 64 bytes
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    constexpr int rows = 16 * NCB;
    const int steps = p.K >> 5;
    const int gw = blockIdx.x * 8 + w, nwav = gridDim.x * 8;
    const int ntiles = (p.N + 15) >> 4;
    const int my_tiles = gw < ntiles ? min(LP_MT, (ntiles - gw + nwav - 1) / nwav) : 0;
    int boff[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) boff[cb] = (16 * cb + fr) * 64 + ((fq ^ ((-(fr >> 2)) & 3)) << 4);
    f32x4 acc[LP_MT][NCB];
#pragma unroll
    for (int t = 0; t < LP_MT; t++)
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) acc[t][cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int ph0 = 0; ph0 < steps; ph0 += sp) {
        const int nst = min(sp, steps - ph0);
        const int ngrp = (nst + SK_U - 1) / SK_U;
        const int G = my_tiles * ngrp;                 // (tile, k-group) pairs of this wave in this phase
        auto issue = [&](int g, half8 (&a)[SK_U]) {    // unconditional clamped loads, all in flight together
            const int tile = g / ngrp, s0 = ph0 + (g - tile * ngrp) * SK_U;
            const half_t *wp = p.Wt + (long)(gw + tile * nwav) * steps * 512 + lane * 8;
#pragma unroll
            for (int u = 0; u < SK_U; u++) {
                const int sc = s0 + u < steps ? s0 + u : steps - 1;
                a[u] = __builtin_nontemporal_load(reinterpret_cast<const half8 *>(wp + (long)512 * sc));
            }
        };
        half8 a0[SK_U], a1[SK_U];
        if (G > 0) issue(0, a0);                       // in flight while the image is staged
        __syncthreads();                               // every wave is done with the previous phase's image
        for (int c = tid; c < nst * rows * 4; c += 512) {
            const int q = c & 3, r = (c >> 2) % rows, st = (c >> 2) / rows;
            const int rr = r < p.R ? r : p.R - 1;
            const u32x4 v = *reinterpret_cast<const u32x4 *>(p.x + (long)rr * p.ldx + 32 * (ph0 + st) + 8 * q);
            *reinterpret_cast<u32x4 *>(xs + ((long)st * rows + r) * 64 + ((q ^ ((-(r >> 2)) & 3)) << 4)) = v;
        }
        __syncthreads();
        auto compute = [&](int g, const half8 (&a)[SK_U]) {
            const int tile = g / ngrp, s0 = (g - tile * ngrp) * SK_U;   // phase-local k-step of the group's first step
#pragma unroll
            for (int u = 0; u < SK_U; u++) {
                if (s0 + u < nst) {
#pragma unroll
                    for (int cb = 0; cb < NCB; cb++) {
                        const half8 b = *reinterpret_cast<const half8 *>(xs + (long)(s0 + u) * rows * 64 + boff[cb]);
                        if (tile == 0) acc[0][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[u], b, acc[0][cb], 0, 0, 0);
                        else acc[1][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[u], b, acc[1][cb], 0, 0, 0);
                    }
                }
            }
        };
        for (int g = 0; g < G; g += 2) {
            if (g + 1 < G) issue(g + 1, a1);
            compute(g, a0);
            if (g + 2 < G) issue(g + 2, a0);
            if (g + 1 < G) compute(g + 1, a1);
        }
    }
#pragma unroll
    for (int t = 0; t < LP_MT; t++) {
        if (t < my_tiles) {
            const int n = 16 * (gw + t * nwav) + 4 * fq;
#pragma unroll
            for (int cb = 0; cb < NCB; cb++) {
                const int r = 16 * cb + fr;
                if (r < p.R) skinny_store(p, acc[t][cb], r, n);
            }
        }
    }
}

// tile-major repack of a row-major [N][K] fp16 weight: out[(tile * K/32 + s) * 512 + lane * 8 + j] =
// W[16 tile + (lane & 15)][32 s + 8 (lane >> 4) + j], rows >= N zero: the MFMA A fragment of (tile, k-step s) is 1 KiB contiguous
__global__ __launch_bounds__(256) void repack_tiles_kernel(const half_t *__restrict__ W, half_t *__restrict__ out, int N, int K) {
    const long chunk = blockIdx.x * 256L + threadIdx.x;  // one 16-byte chunk per thread
    const int steps = K >> 5;
    const long total = (long)((N + 15) >> 4) * steps * 64;
    if (chunk >= total) return;
    const int lane = (int)(chunk & 63);
    const long ts = chunk >> 6;
    const int s = (int)(ts % steps);
    const long tile = ts / steps;
    const long row = tile * 16 + (lane & 15);
    u32x4 v = {0u, 0u, 0u, 0u};
    if (row < N) v = *reinterpret_cast<const u32x4 *>(W + row * K + 32 * s + 8 * (lane >> 4));
    *reinterpret_cast<u32x4 *>(out + chunk * 8) = v;
}

void launch_repack_tiles(const half_t *W, half_t *out, int N, int K, hipStream_t st) {
    const long total = (long)((N + 15) >> 4) * (K >> 5) * 64;
    hipLaunchKernelGGL(repack_tiles_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, W, out, N, K);
}

// calls f(std::integral_constant<int, V>) for the V of Vs that equals v: a run-time value of the plan as a template argument
template <int... Vs, class F>
static void with_const(int v, F &&f) {
    (void)((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

bool launch_skinny(const SkinnyParams &p_in, hipStream_t st) {
    const SkinnyPlan pl = skinny_plan(p_in.R, p_in.N, p_in.K, p_in.epi, p_in.Wt != nullptr, p_in.ln_x != nullptr);
    if (pl.kind == SKP_NONE) return false;
    SkinnyParams p = p_in;
    p.ln_rk = 1.0f / (float)p.K;
    const dim3 grid(pl.grid_x, pl.grid_y), block(pl.block);
    switch (pl.kind) {
        case SKP_GEMM:
            with_const<1, 2, 3, 4>(pl.ncb, [&](auto ncb) {
                constexpr int NCB = decltype(ncb)::value;
                if (pl.ksplit == 1) hipLaunchKernelGGL((skinny_gemm_kernel<NCB, 1, 2>), grid, block, 0, st, p);
                else with_const<2, 4, 8, 16>(pl.ksplit, [&](auto ks) {
                    hipLaunchKernelGGL((skinny_gemm_kernel<NCB, decltype(ks)::value, 1>), grid, block, 0, st, p);
                });
            });
            break;
        case SKP_LN:
            with_const<1, 2, 3, 4, 6, 8, 10>(pl.ksplit, [&](auto steps) {
                constexpr int STEPS = decltype(steps)::value;
                if (pl.nt == 1) hipLaunchKernelGGL((skinny_ln_kernel<STEPS, 1>), grid, block, 0, st, p);
                else hipLaunchKernelGGL((skinny_ln_kernel<STEPS, 2>), grid, block, 0, st, p);
            });
            break;
        case SKP_LDS:
            with_const<1, 2>(pl.ncb, [&](auto ncb) {
                launch_lds_exclusive<skinny_lds_kernel<decltype(ncb)::value>>(grid, block, pl.lds_used, st, p);
            });
            break;
        case SKP_LDSP:
            with_const<3, 4, 5, 6>(pl.ncb, [&](auto ncb) {
                launch_lds_exclusive<skinny_ldsp_kernel<decltype(ncb)::value>>(grid, block, pl.lds_used, st, p, pl.sp);
            });
            break;
    }
    return true;
}
