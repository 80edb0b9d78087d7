// k_gemm.hip -- MFMA GEMM for the encoder and the cross-K/V projection (gfx950).
//
//   C[M][N] = A[M][K] . W[N][K]^T (+ bias) with fused epilogues; fp16 operands, fp32 accumulate.
//
// Replaces, on the reference path, candle's Linear/Conv1d matmuls inside AudioEncoder::forward and
// the cross-attention key/value projections (reached through Type::encoder_forward /
// Type::decoder_forward, src/models/whisper/model.rs:455-476).  Conv1d k=3 is expressed as a GEMM
// whose A rows overlap (lda = stride * channels, K = 3 * channels) -- no im2col buffer.
//
// Tile: 128 (M) x 128 (N) x 64 (K) per 256-thread workgroup (4 waves as 2 x 2, 64 x 64 per wave,
// v_mfma_f32_16x16x32_f16).  Both operands are K-contiguous, so each lane's fragment is one 16-byte
// LDS read.  The loop, its LDS image (64 KiB) and its LDS-DMA staging are tile128_mainloop (mfma_tile128.h),
// which transcript scoring (k_score.hip) runs too.
//
// Orientation: by default the weight rows are the MFMA "A" operand, so a lane's 4 accumulator
// registers are 4 consecutive output COLUMNS of one row -> 8-byte fp16 / 16-byte f32 row-major
// stores.  The V^T segment uses the other orientation (4 consecutive rows of one column).
#include <stdlib.h>

#include <atomic>

#include "mfma_tile128.h"

#define BM 128
#define BN 128
#define BK 64

__device__ __forceinline__ float gelu_tanh_f(float v) { return gelu_tanh_fast(v); }

__device__ __forceinline__ const half_t *a_row_ptr(const GemmParams &p, int m) {
    if (m >= p.M) m = p.M - 1;  // clamp: tail rows are loaded but never stored
    int b = nh_div(m, p.a_rpb, p.a_magic), r = m - b * p.a_rpb;
    return p.A + (long)b * p.a_bstride + (long)r * p.lda;
}

// the 128 x 128 x 64 loop of mfma_tile128.h on tile (m0, n0): activation rows through the row map, tail rows clamped
// (a_row_ptr); weight rows n0 .. n0 + 127 as they are (N is a multiple of BN)
template <bool SWAP>
__device__ __forceinline__ void gemm_mainloop(const GemmParams &p, char *smem, int m0, int n0, f32x4 (&acc)[4][4]) {
    tile128_mainloop<SWAP>([&](int row) { return a_row_ptr(p, m0 + row); },
                           [&](int row) { return p.W + (long)(n0 + row) * p.K; }, p.K / BK, smem, acc);
}

__device__ __forceinline__ long out_row(const GemmParams &p, int m) {
    int b = nh_div(m, p.o_rpb, p.o_magic), r = m - b * p.o_rpb;
    return (long)b * p.o_bstride + r + p.o_off;
}

__global__ __launch_bounds__(256, 2) void gemm_f16_kernel(GemmParams p) {
    __shared__ __attribute__((aligned(16))) char smem[T128_LDS];
    // XCD-aware tile order: blocks b and b+8 share an XCD (L2); give each XCD a contiguous run of
    // tiles so the N-tiles of one M-panel (same A rows) are neighbours in one L2.
    const int ntn = p.N / BN, ntm = (p.M + BM - 1) / BM;
    const int bid = xcd_contiguous(blockIdx.x, ntn * ntm);
    const int tm = bid / ntn, tn = bid - tm * ntn;
    const int m0 = tm * BM, n0 = tn * BN;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wm = w >> 1, wn = w & 1;
    const int fr = lane & 15, fq = lane >> 4;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int seg = (p.epi == EPI_F16 || p.epi == EPI_GELU_F16) ? n0 / p.seg_n : 0;
    const bool vt = (p.epi == EPI_F16 && seg == p.vt_seg);
    if (vt) gemm_mainloop<false>(p, smem, m0, n0, acc);
    else gemm_mainloop<true>(p, smem, m0, n0, acc);

    if (vt) {
        // lane holds rows m = mb + 4 fq + r (r = 0..3) of column n = nb + fr
        half_t *dst = reinterpret_cast<half_t *>(seg == 0 ? p.out[0] : seg == 1 ? p.out[1] : p.out[2]);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            int n = n0 + wn * 64 + 16 * i + fr;
            float bv = p.bias ? p.bias[n] : 0.f;
            int nl = n - seg * p.seg_n, h = nl >> 6, dh = nl & 63;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                int m = m0 + wm * 64 + 16 * j + 4 * fq;
                if (m >= p.M) continue;
                int b = nh_div(m, p.S, p.s_magic), s = m - b * p.S;
                half_t *row = dst + ((long)(b * p.H + h) * NH_DH + dh) * NH_SP;
                if (s + 3 < p.S && m + 3 < p.M) {
                    half4 v = {(half_t)(acc[i][j][0] + bv), (half_t)(acc[i][j][1] + bv),
                               (half_t)(acc[i][j][2] + bv), (half_t)(acc[i][j][3] + bv)};
                    *reinterpret_cast<half4 *>(row + s) = v;
                } else {
                    for (int r = 0; r < 4; r++) {
                        int mm = m + r;
                        if (mm >= p.M) break;
                        int bb = nh_div(mm, p.S, p.s_magic), ss = mm - bb * p.S;
                        dst[((long)(bb * p.H + h) * NH_DH + dh) * NH_SP + ss] = (half_t)(acc[i][j][r] + bv);
                    }
                }
            }
        }
        return;
    }
    half_t *obase = reinterpret_cast<half_t *>(seg == 0 ? p.out[0] : seg == 1 ? p.out[1] : p.out[2]);
    // SWAP orientation: lane holds columns n = nb + 4 fq + r (r = 0..3) of row m = mb + fr
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int n = n0 + wn * 64 + 16 * i + 4 * fq;
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (p.bias) bv = *reinterpret_cast<const f32x4 *>(p.bias + n);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int m = m0 + wm * 64 + 16 * j + fr;
            if (m >= p.M) continue;
            f32x4 v = acc[i][j] + bv;
            if (p.epi == EPI_F16 || p.epi == EPI_GELU_F16) {
                if (p.epi == EPI_F16 && seg == 0 && p.seg0_scale != 0.f) v *= p.seg0_scale;
                if (p.epi == EPI_GELU_F16) {
                    v[0] = gelu_tanh_f(v[0]); v[1] = gelu_tanh_f(v[1]);
                    v[2] = gelu_tanh_f(v[2]); v[3] = gelu_tanh_f(v[3]);
                }
                const int nl = n - seg * p.seg_n;
                half_t *dst = p.head_major ? obase + (((long)nh_div(m, p.S, p.s_magic) * p.H + (nl >> 6)) * p.S + (m - nh_div(m, p.S, p.s_magic) * p.S)) * NH_DH + (nl & 63)
                                           : obase + out_row(p, m) * p.ldo + nl;
                half4 hv = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
                *reinterpret_cast<half4 *>(dst) = hv;
            } else if (p.epi == EPI_RESID_F32) {
                float *dst = reinterpret_cast<float *>(p.out[0]) + (long)m * p.ldo + n;
                f32x4 x = *reinterpret_cast<const f32x4 *>(dst);
                *reinterpret_cast<f32x4 *>(dst) = x + v;
            } else {  // EPI_CONV2_F32
                int s = m - nh_div(m, p.S, p.s_magic) * p.S;
                f32x4 pe = *reinterpret_cast<const f32x4 *>(p.pos + (long)s * p.N + n);
                f32x4 o = {gelu_tanh_f(v[0]) + pe[0], gelu_tanh_f(v[1]) + pe[1], gelu_tanh_f(v[2]) + pe[2],
                           gelu_tanh_f(v[3]) + pe[3]};
                *reinterpret_cast<f32x4 *>(reinterpret_cast<float *>(p.out[0]) + (long)m * p.ldo + n) = o;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// 256 x 256 tile kernel for the large encoder shapes (N % 256 == 0, K % 128 == 0, M >= 256): persistent, one
// 512-thread workgroup per CU = 8 waves as 2 (M) x 4 (N), 128 x 64 outputs per wave (128 accumulator VGPRs).
//
// Main loop = the 8-phase "ping-pong" schedule of the CDNA4 playbook (cdna_hip_programming.md, "The 256^2 8-phase
// template"), restated for this kernel's operand layout:
//  * BK = 64 K-tiles in two 64 KiB LDS buffers, each cut into four 16 KiB half-tiles A0 A1 B0 B1.  Half-tile Ah holds,
//    for BOTH wave rows, the h-th 64 rows of the wave's 128 (LDS row l <-> tile row (l >> 6) * 128 + 64 h + (l & 63));
//    Bh the h-th 32 columns of each wave column's 64 (l <-> (l >> 5) * 64 + 32 h + (l & 31)).  The permutation lives
//    in the per-lane SOURCE address of the LDS-DMA (global_load_lds_dwordx4; its LDS destination is lane-linear), and so
//    does the bank swizzle chunk' = chunk ^ ((row >> 1) & 7) that makes the ds_read_b128 fragment reads conflict-free.
//  * a K-tile is four phases = the four 64 x 32 quadrants of the wave's 128 x 64 output, 16 MFMAs each:
//        q0 (m0,n0): reads A0 (8 ds_read_b128) + B0 (4)    q1 (m0,n1): reads B1 (4)
//        q2 (m1,n1): reads A1 (8)                          q3 (m1,n0): no reads (the B0 fragments are kept)
//    so the half-tiles of a buffer die one after the other (A0, B0 after q0; B1 after q1; A1 after q2) and each is
//    re-staged for the K-tile after next two or three phases after its last read, FIVE phases before its first use:
//        q2: A0(t+2)   q3: B0(t+2)   q0: B1(t+1)   q1: A1(t+1)         (one half-tile = 2 LDS-DMA per thread per phase)
//  * the two waves of a SIMD (wave rows wr = 0 / 1) run half a phase apart (one extra s_barrier for wr = 1 up front):
//        phase = [ds_read, LDS-DMA issue, counted vmcnt] s_barrier [lgkmcnt(0), 16 MFMA] s_barrier
//    so in every barrier interval one wave of each SIMD issues MFMAs while the other one reads LDS: the matrix pipe is
//    fed by one of them at all times instead of both reading, then both multiplying.
//  * RAW: the vmcnt that retires a half-tile sits before the FIRST barrier of the phase before its first read (then the
//    lagging group's part has landed too before the leading group reads); WAR: >= 2 phases between last read and re-stage.
//    In steady state four half-tiles stay in flight across every wait: vmcnt(8), never 0 inside the loop.
//
// Persistent tiles: the workgroup walks tiles blockIdx.x, + gridDim.x, ... (XCD-aware order below).  As soon as the
// main loop of a tile ends it issues the six prologue half-tiles of its NEXT tile, then runs the epilogue of the
// finished one: block launch, first-fetch latency and the store drain (14 of 47 us per K = 1280 tile before) hide
// under each other.  The epilogue therefore stays out of the ring: fp16 outputs go through a 2176-byte per-wave
// image (16 rows x 64 columns, 136-byte pitch) behind it, so that every global store writes whole 128-byte rows.
// ---------------------------------------------------------------------------------------------------
#define G2_BM 256
#define G2_BN 256
#define G2_GM 4           // M-panels per group of the tile order (2 and 8 measured: within +-3 %, 4 best overall)
#define PP_BUF 65536
#define PP_HT 16384
#define PP_RING (2 * PP_BUF)
#define PP_EPI_PITCH 136  // bytes per image row (64 fp16 + 8 pad)
#define PP_EPI_WAVE (16 * PP_EPI_PITCH)
#define PP_BIAS (PP_RING + 8 * PP_EPI_WAVE)  // two rows of 256 f32: the bias of this tile's and the next tile's columns
#define PP_LDS (PP_BIAS + 2 * 1024)
#define PP_VT_OOB 0xf0000000u  // V^T epilogue: offset of a row that must not be written; beyond any image launch_gemm admits, and
                               // still so (no wrap) with a column offset added

struct PPSource { unsigned ag[2][2], wg[2][2]; };  // [h][i]: 32-bit element offsets of this lane's eight source rows

// staging map: half-tile slot s = tid + 512 i (i = 0, 1): LDS row l = s >> 3 = (tid >> 3) + 64 i, chunk' = tid & 7,
// source chunk = chunk' ^ ((l >> 1) & 7) (64 i leaves the swizzle unchanged)
__device__ __forceinline__ PPSource pp_source(const GemmParams &p, int m0, int n0) {
    // the lane constants below are recomputed for every tile on purpose: hoisted out of the tile loop they do not fit beside
    // 128 accumulators + 64 fragment registers, get spilled, and their reloads (scratch loads count in vmcnt) make hipcc
    // drain vmcnt(0) in front of the prologue DMAs
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lrow = tid >> 3;
    const int csrc = ((tid & 7) ^ ((lrow >> 1) & 7)) * 8;
    PPSource sg;
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int i = 0; i < 2; i++) {
            // a_row_ptr(p, m) - p.A in 32 bits (launch_gemm sends a map that does not fit to the 128 x 128 kernel): tail rows
            // clamped, the clip index as one multiply-high (a_magic is 0 or exact here)
            const unsigned m = (unsigned)min(m0 + i * 128 + h * 64 + lrow, p.M - 1), b = __umulhi(m, p.a_magic);
            sg.ag[h][i] = b * (unsigned)p.a_bstride + (m - b * (unsigned)p.a_rpb) * (unsigned)p.lda + csrc;
            const int l = lrow + 64 * i;
            sg.wg[h][i] = (unsigned)(n0 + (l >> 5) * 64 + h * 32 + (l & 31)) * (unsigned)p.K + csrc;
        }
    return sg;
}

// which: 0 A0, 1 B0, 2 B1, 3 A1 (the issue order of a K-tile)
__device__ __forceinline__ void pp_stage(const GemmParams &p, char *wbase, const PPSource &sg, int t, int which) {
    const int h = (which >> 1) & 1;
    const bool isB = which == 1 || which == 2;
    char *dst = wbase + (t & 1) * PP_BUF + (isB ? 2 * PP_HT : 0) + h * PP_HT;
    const unsigned ko = (unsigned)t * 64u;
    if (isB) {
        __builtin_amdgcn_global_load_lds((gbl_void *)(p.W + (size_t)(sg.wg[h][0] + ko)), (lds_void *)dst, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gbl_void *)(p.W + (size_t)(sg.wg[h][1] + ko)), (lds_void *)(dst + 8192), 16, 0, 0);
    } else {
        __builtin_amdgcn_global_load_lds((gbl_void *)(p.A + (size_t)(sg.ag[h][0] + ko)), (lds_void *)dst, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gbl_void *)(p.A + (size_t)(sg.ag[h][1] + ko)), (lds_void *)(dst + 8192), 16, 0, 0);
    }
}

// K-tile 0 complete, A0 and B0 of K-tile 1: what phases (-1, 2) and (-1, 3) would have issued
__device__ __forceinline__ void pp_prologue(const GemmParams &p, char *wbase, const PPSource &sg) {
    pp_stage(p, wbase, sg, 0, 0); pp_stage(p, wbase, sg, 0, 1); pp_stage(p, wbase, sg, 0, 2); pp_stage(p, wbase, sg, 0, 3);
    pp_stage(p, wbase, sg, 1, 0); pp_stage(p, wbase, sg, 1, 1);
}

// the main loop proper; the prologue of this tile has been issued (any time) before
template <bool SWAP>
__device__ __forceinline__ void pp_main(const GemmParams &p, char *smem, char *wbase, const PPSource &sg, f32x4 (&acc)[8][4]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wr = w >> 2, wc = w & 3;
    const int fr = lane & 15, fq = lane >> 4;
    const int nt = p.K >> 6;
    // fragment read addresses inside a half-tile: row r, chunk 4 ks + fq, swizzle (r >> 1) & 7 == fr >> 1 for every
    // fragment; the ks = 1 chunk is the ks = 0 address with bit 6 flipped: one per-lane base per k-step, everything
    // else is an immediate offset of the ds_read
    const int offA0 = (wr * 64 + fr) * 128 + ((fq ^ (fr >> 1)) << 4);  // + 2048 i (i = 0..3)
    const int offB0 = (wc * 32 + fr) * 128 + ((fq ^ (fr >> 1)) << 4);  // + 2048 j (j = 0..1)
    const char *const pa[2] = {smem + offA0, smem + (offA0 ^ 64)};
    const char *const pb[2] = {smem + offB0, smem + (offB0 ^ 64)};
    half8 fa[4][2], fb[4][2];  // fa[i][ks]: current m-half; fb[j][ks]: j < 2 n0, j >= 2 n1

    // one phase.  Q: quadrant; BUF: LDS buffer of the K-tile being multiplied; WAIT: vmcnt count (< 0: none);
    // DO_ISSUE: re-stage the half-tile this phase is responsible for, from K-tile ST
#define PP_PHASE(Q, BUF, WAIT, DO_ISSUE, ST)                                                                             \
    {                                                                                                                    \
        constexpr int tb_ = (BUF) * PP_BUF;                                                                              \
        if ((Q) == 0) {                                                                                                  \
            _Pragma("unroll") for (int j = 0; j < 2; j++) _Pragma("unroll") for (int ks = 0; ks < 2; ks++)             \
                fb[j][ks] = *reinterpret_cast<const half8 *>(pb[ks] + (tb_ + 2 * PP_HT + 2048 * j));                    \
            __builtin_amdgcn_sched_barrier(0);                                                                           \
            _Pragma("unroll") for (int i = 0; i < 4; i++) _Pragma("unroll") for (int ks = 0; ks < 2; ks++)             \
                fa[i][ks] = *reinterpret_cast<const half8 *>(pa[ks] + (tb_ + 2048 * i));                               \
        } else if ((Q) == 1) {                                                                                           \
            _Pragma("unroll") for (int j = 0; j < 2; j++) _Pragma("unroll") for (int ks = 0; ks < 2; ks++)             \
                fb[2 + j][ks] = *reinterpret_cast<const half8 *>(pb[ks] + (tb_ + 3 * PP_HT + 2048 * j));                \
        } else if ((Q) == 2) {                                                                                           \
            _Pragma("unroll") for (int i = 0; i < 4; i++) _Pragma("unroll") for (int ks = 0; ks < 2; ks++)             \
                fa[i][ks] = *reinterpret_cast<const half8 *>(pa[ks] + (tb_ + PP_HT + 2048 * i));                       \
        }                                                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                                               \
        if (DO_ISSUE) pp_stage(p, wbase, sg, (ST), (Q) == 2 ? 0 : (Q) == 3 ? 1 : (Q) == 0 ? 2 : 3);                     \
        if ((WAIT) == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");                                                \
        else if ((WAIT) == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");                                           \
        else if ((WAIT) == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");                                           \
        else if ((WAIT) == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                           \
        __builtin_amdgcn_s_barrier();                                                                                    \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                               \
        __builtin_amdgcn_s_setprio(1);                                                                                   \
        {                                                                                                                \
            constexpr int ib_ = ((Q) >= 2) ? 4 : 0, jb_ = ((Q) == 1 || (Q) == 2) ? 2 : 0;                                \
            _Pragma("unroll") for (int ks = 0; ks < 2; ks++) _Pragma("unroll") for (int i = 0; i < 4; i++)             \
                _Pragma("unroll") for (int j = 0; j < 2; j++) {                                                         \
                    if (SWAP) acc[ib_ + i][jb_ + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[jb_ + j][ks], fa[i][ks], acc[ib_ + i][jb_ + j], 0, 0, 0); \
                    else acc[ib_ + i][jb_ + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[i][ks], fb[jb_ + j][ks], acc[ib_ + i][jb_ + j], 0, 0, 0);      \
                }                                                                                                        \
        }                                                                                                                \
        __builtin_amdgcn_s_setprio(0);                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                               \
        __builtin_amdgcn_s_barrier();                                                                                    \
    }

    // everything issued so far (prologue DMAs, the previous tile's stores, the residual tile) has landed
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();        // the stagger: wave row 1 runs half a phase behind
    // steady state: K-tile pairs (t, t + 1) with t + 3 < nt, i.e. every issue below is in range
    int t = 0;
    for (; t + 4 <= nt; t += 2) {
        PP_PHASE(0, 0, 8, true, t + 1)
        PP_PHASE(1, 0, 8, true, t + 1)
        PP_PHASE(2, 0, -1, true, t + 2)
        PP_PHASE(3, 0, 8, true, t + 2)
        PP_PHASE(0, 1, 8, true, t + 2)
        PP_PHASE(1, 1, 8, true, t + 2)
        PP_PHASE(2, 1, -1, true, t + 3)
        PP_PHASE(3, 1, 8, true, t + 3)
    }
    // last pair (nt - 2, nt - 1): nothing left to issue after A1(nt - 1); the waits count down 8 8 . 4 2 0
    PP_PHASE(0, 0, 8, true, t + 1)
    PP_PHASE(1, 0, 8, true, t + 1)
    PP_PHASE(2, 0, -1, false, 0)
    PP_PHASE(3, 0, 4, false, 0)
    PP_PHASE(0, 1, 2, false, 0)
    PP_PHASE(1, 1, 0, false, 0)
    PP_PHASE(2, 1, -1, false, 0)
    PP_PHASE(3, 1, -1, false, 0)
    if (wr == 0) __builtin_amdgcn_s_barrier();        // balance the barrier count of the stagger
#undef PP_PHASE
}

// XCD-aware tile order.  Workgroups b and b + 8 share an XCD (L2): every XCD gets a contiguous run of tiles, walked in
// groups of G2_GM M-panels x all N-tiles, N outer / M inner, so the ~32 tiles an XCD has in flight are 4 M-panels x 8
// N-tiles: the A panels (4 x 256 x K) stay in that XCD's 4 MiB L2 for the whole N sweep and each streamed W tile is
// shared by 4 workgroups (PMC: W was re-fetched once per M-panel from the Infinity Cache with a plain M-major order).
__device__ __forceinline__ void pp_tile(int vb, int ntn, int ntm, int &tm, int &tn) {
    grouped_tile(xcd_contiguous(vb, ntn * ntm), ntn, ntm, G2_GM, tm, tn);
}

// ---- the tile hand-over: next tile's first fetches, then the finished tile's epilogue ----
// Everything a store of the fp16 epilogues needs is decided per launch (launch_gemm: the e_* row map, one form for row-major,
// row-mapped and head-major outputs) or per tile (segment, V^T or not, scaled or not, the sixteen row offsets of a lane), so
// that the 128 outputs of a lane run as one straight line of bias add / scale / GELU / conversion, LDS image and stores.

// The bias of a tile's 256 columns travels with the tile's first fetches: one more LDS-DMA (4 bytes per lane) in front of the
// twelve of the prologue, into one of two 1 KiB rows behind the images (tiles alternate), and the epilogue reads it with
// ds_read.  An ordinary load of the bias in the hand-over makes hipcc wait vmcnt(0) where the value is used -- it does not count
// past LDS-DMAs in flight -- and that is the drain of the next tile's twelve DMAs in front of the epilogue, wherever the load is
// issued.  Being the oldest operation of its batch the extra DMA has retired at every counted wait of the main loop.  The two waves
// of a wave column fetch the same 64 values to the same place.  Without a bias both rows are zero (gemm256_f16_kernel).
__device__ __forceinline__ void pp_bias_stage(const GemmParams &p, char *smem, int w, int n0, int par) {
    if (!p.bias) return;
    int ln = threadIdx.x;
    asm volatile("" : "+v"(ln));
    __builtin_amdgcn_global_load_lds((gbl_void *)(p.bias + n0 + (w & 3) * 64 + (ln & 63)), (lds_void *)(smem + PP_BIAS + par * 1024 + (w & 3) * 256), 4, 0, 0);
}

// starts the fetches of the workgroup's next tile, if it has one (the ring is free: every wave is through its last phase)
__device__ __forceinline__ bool pp_next(const GemmParams &p, char *smem, int w, int par, int &vb, int ntn, int ntm, int &tm, int &tn, PPSource &sg) {
    const int nvb = vb + gridDim.x;
    if (nvb >= ntn * ntm) return false;
    vb = nvb;
    pp_tile(nvb, ntn, ntm, tm, tn);
    pp_bias_stage(p, smem, w, tn * G2_BN, par ^ 1);
    sg = pp_source(p, tm * G2_BM, tn * G2_BN);
    pp_prologue(p, smem + w * 1024, sg);
    return true;
}

// byte offsets of the sixteen 8-row groups a lane stores (rows m0 + wm * 128 + 8 k + (lane >> 3), k = 0 .. 15) from the wave's
// base: row m lies ((m / rpb) * bstride + m % rpb) * e_rs bytes in = ((m / rpb) * e_db + m) * e_rs (plan_gemm256).  A tile whose rows
// are one clip (every tile of a launch whose rows are one batch) has the quotient as a scalar and adds 8 k e_rs per group; a tile
// that holds a clip end or the end of M divides per group.  Rows >= M continue the last clip, so their offsets lie at or beyond
// the last row's and the buffer descriptor (e_bound) drops them: no guard, no exec-masked region around the stores.
__device__ __forceinline__ void pp_row_offsets(const GemmParams &p, int m0, int wm, int ln, unsigned (&off)[16]) {
    const unsigned ml = (unsigned)(m0 + wm * 128 + ((ln >> 3) & 7)), lc = (unsigned)(ln & 7) * 16u;
    const unsigned b0 = __umulhi((unsigned)m0, p.e_magic);
    if (m0 + G2_BM <= p.M && b0 == __umulhi((unsigned)m0 + G2_BM - 1, p.e_magic)) {
        const unsigned base = (b0 * p.e_db + ml) * p.e_rs + lc;
#pragma unroll
        for (int k = 0; k < 16; k++) off[k] = base + (unsigned)(8 * k) * p.e_rs;
    } else {
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const unsigned m = ml + 8 * k;
            off[k] = (__umulhi(m, p.e_magic) * p.e_db + m) * p.e_rs + lc;
        }
    }
}

// bias of the lane's four 4-column pieces (columns wn * 64 + 16 j + 4 fq + r of the tile) from the tile's bias row
__device__ __forceinline__ void pp_bias4(const char *smem, int par, int wn, int ln, f32x4 (&bv)[4]) {
    const char *const src = smem + PP_BIAS + par * 1024 + wn * 256 + ((ln >> 4) & 3) * 16;
#pragma unroll
    for (int j = 0; j < 4; j++) bv[j] = *reinterpret_cast<const f32x4 *>(src + 64 * j);
}

// fp16 / GELU epilogue: lane holds columns n = nb + 4 fq + r of row m = mb + fr: per 16-row block i a [16 m][64 n] fp16 image,
// read back as 128-byte row segments (8 lanes x 16 B; 8 rows per store instruction)
template <bool GELU, bool SCALED>
__device__ __forceinline__ void pp_epi_f16(const f32x4 (&acc)[8][4], const f32x4 (&bv)[4], float scale, char *img, int ln,
                                           __amdgpu_buffer_rsrc_t ors, const unsigned (&off)[16]) {
    char *const wr = img + (ln & 15) * PP_EPI_PITCH + ((ln >> 4) & 3) * 8;
    const char *const rd = img + ((ln >> 3) & 7) * PP_EPI_PITCH + (ln & 7) * 16;
#pragma unroll
    for (int i = 0; i < 8; i++) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            f32x4 v = acc[i][j] + bv[j];
            if (SCALED) v *= scale;
            if (GELU) {
                v[0] = gelu_tanh_f(v[0]); v[1] = gelu_tanh_f(v[1]); v[2] = gelu_tanh_f(v[2]); v[3] = gelu_tanh_f(v[3]);
            }
            half4 hv = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
            *reinterpret_cast<half4 *>(wr + 32 * j) = hv;
        }
#pragma unroll
        for (int it = 0; it < 2; it++) {
            const half4 lo = *reinterpret_cast<const half4 *>(rd + 8 * it * PP_EPI_PITCH);
            const half4 hi = *reinterpret_cast<const half4 *>(rd + 8 * it * PP_EPI_PITCH + 8);
            const half8 o = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), ors, off[2 * i + it], 0, 0);
        }
    }
}

// V^T epilogue: lane holds rows m = mb + 4 fq + r of column n = nb + fr: per 16-column block j and 64-row half a [16 n][64 m]
// image, read back as 16-byte runs of 8 consecutive m.  one_clip (tile-uniform): the tile's 256 rows are one clip b0 and all below
// M, so every run is a whole 16-byte store; otherwise a run that crosses a clip end or M goes out element by element.  One body
// with a scalar branch at each store, not one body per case: hipcc hoists what two bodies have in common above the branch
// between them -- every bias add of the tile, 128 more live registers, and accumulators get spilled.
__device__ __forceinline__ void pp_epi_vt(const GemmParams &p, const f32x4 (&acc)[8][4], const float (&bv)[4], char *img, int ln,
                                          half_t *dst, int m0, int wm, int nl0, bool one_clip, unsigned b0) {
    char *const wr = img + (ln & 15) * PP_EPI_PITCH + ((ln >> 4) & 3) * 8;
    const char *const rd = img + ((ln >> 3) & 7) * PP_EPI_PITCH + (ln & 7) * 16;
    const int nl = nl0 + ((ln >> 3) & 7), ml = m0 + wm * 128 + (ln & 7) * 8;  // + 16 j + 8 it, + 64 hh
    __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc(dst, 0, (int)p.vt_bytes, 0x00020000);
    const unsigned voff = ((b0 * (unsigned)(p.H * NH_DH) + (unsigned)nl) * NH_SP + ((unsigned)ml - b0 * (unsigned)p.S)) * 2u;
    // !one_clip: the lane's two runs (hh = 0, 1) are the same rows for every column: decided once.  whole: the eight rows are one
    // clip and below M; otherwise every row goes to its own offset, or beyond the descriptor when it is >= M (dropped)
    bool whole[2];
    unsigned wo[2];
    if (!one_clip) {
#pragma unroll
        for (int hh = 0; hh < 2; hh++) {
            const int m = ml + 64 * hh;
            const unsigned b = __umulhi((unsigned)m, p.s_magic), ss = (unsigned)m - b * (unsigned)p.S;
            whole[hh] = (int)ss + 7 < p.S && m + 7 < p.M;
            wo[hh] = ((b * (unsigned)(p.H * NH_DH) + (unsigned)nl) * NH_SP + ss) * 2u;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
        for (int hh = 0; hh < 2; hh++) {
#pragma unroll
            for (int ii = 0; ii < 4; ii++) {
                const f32x4 a = acc[4 * hh + ii][j];
                half4 v = {(half_t)(a[0] + bv[j]), (half_t)(a[1] + bv[j]), (half_t)(a[2] + bv[j]), (half_t)(a[3] + bv[j])};
                *reinterpret_cast<half4 *>(wr + 32 * ii) = v;
            }
#pragma unroll
            for (int it = 0; it < 2; it++) {
                const half4 lo = *reinterpret_cast<const half4 *>(rd + 8 * it * PP_EPI_PITCH);
                const half4 hi = *reinterpret_cast<const half4 *>(rd + 8 * it * PP_EPI_PITCH + 8);
                if (one_clip) {
                    const half8 o = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), vrs, voff + (unsigned)(((16 * j + 8 * it) * NH_SP + 64 * hh) * 2), 0, 0);
                } else {
                    const unsigned c = (unsigned)((16 * j + 8 * it) * NH_SP * 2);
                    if (whole[hh]) {
                        const half8 o = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), vrs, wo[hh] + c, 0, 0);
                    } else {
#pragma unroll
                        for (int r = 0; r < 8; r++) {   // recomputed at every run: rare tiles, and sixteen offsets held across the epilogue cost spills
                            const unsigned mm = (unsigned)(ml + 64 * hh + r), bb = __umulhi(mm, p.s_magic);
                            const unsigned eo = (int)mm < p.M ? ((bb * (unsigned)(p.H * NH_DH) + (unsigned)nl) * NH_SP + (mm - bb * (unsigned)p.S)) * 2u : PP_VT_OOB;
                            __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(short, r < 4 ? lo[r] : hi[r - 4]), vrs, eo + c, 0, 0);
                        }
                    }
                }
            }
        }
    }
}

template <int EPI>
__global__ __launch_bounds__(512) void gemm256_f16_kernel(GemmParams p) {
    __shared__ __attribute__((aligned(16))) char smem[PP_LDS];
    const int ntn = p.N / G2_BN, ntm = (p.M + G2_BM - 1) / G2_BM;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // the wave index is a scalar
    const int wm = w >> 2, wn = w & 3;
    const int fr = lane & 15, fq = lane >> 4;
    char *const wbase = smem + w * 1024;  // this wave's 1 KiB run of every 8 KiB DMA group
    char *const img = smem + PP_RING + w * PP_EPI_WAVE;

    int vb = blockIdx.x, tm, tn;
    pp_tile(vb, ntn, ntm, tm, tn);
    if (!p.bias) *reinterpret_cast<float *>(smem + PP_BIAS + threadIdx.x * 4) = 0.f;  // both bias rows; read after pp_main's barriers
    pp_bias_stage(p, smem, w, tn * G2_BN, 0);
    PPSource sg = pp_source(p, tm * G2_BM, tn * G2_BN);
    pp_prologue(p, wbase, sg);
    for (int par = 0;; par ^= 1) {   // par: which bias row this tile's columns use
        const int m0 = tm * G2_BM, n0 = tn * G2_BN;
        f32x4 acc[8][4];
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (EPI == EPI_F16 || EPI == EPI_GELU_F16) {
            // the tile's segment (at most three; seg_n is a multiple of the tile width), its destination and its wave's columns
            const int stn = p.seg_n / G2_BN, seg = (tn >= stn) + (tn >= 2 * stn);
            half_t *const ob = reinterpret_cast<half_t *>(seg == 0 ? p.out[0] : seg == 1 ? p.out[1] : p.out[2]);
            const int nl0 = n0 - seg * p.seg_n + wn * 64;
            if (EPI == EPI_F16 && seg == p.vt_seg) {
                pp_main<false>(p, smem, wbase, sg, acc);
                int ln = threadIdx.x;
                asm volatile("" : "+v"(ln));   // lane constants are recomputed per tile (hoisted, they are spilled: pp_source)
                const unsigned b0 = __umulhi((unsigned)m0, p.s_magic);
                const bool one_clip = m0 + G2_BM <= p.M && b0 == __umulhi((unsigned)m0 + G2_BM - 1, p.s_magic);
                const bool more = pp_next(p, smem, w, par, vb, ntn, ntm, tm, tn, sg);
                asm volatile("" : "+v"(ln));
                float bv[4];   // columns wn * 64 + 16 j + fr of the tile
#pragma unroll
                for (int j = 0; j < 4; j++) bv[j] = *reinterpret_cast<const float *>(smem + PP_BIAS + par * 1024 + wn * 256 + 64 * j + (ln & 15) * 4);
                pp_epi_vt(p, acc, bv, img, ln, ob, m0, wm, nl0, one_clip, b0);
                if (!more) break;
            } else {
                pp_main<true>(p, smem, wbase, sg, acc);
                int ln = threadIdx.x;
                asm volatile("" : "+v"(ln));
                f32x4 bv[4];
                pp_bias4(smem, par, wn, ln, bv);
                // the wave's 64 columns start e_off0 + nl0 * e_cs bytes into the segment (row-major: column nl0 of row o_off;
                // head-major: row 0 of head nl0 / 64); the descriptor ends with the launch's last row, not with the allocation:
                // in a joint decode the next encoder batch's rows follow directly
                const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char *>(ob) + p.e_off0 + (long)nl0 * p.e_cs, 0, (int)p.e_bound, 0x00020000);
                unsigned off[16];
                pp_row_offsets(p, m0, wm, ln, off);
                const bool more = pp_next(p, smem, w, par, vb, ntn, ntm, tm, tn, sg);
                if (EPI == EPI_GELU_F16) pp_epi_f16<true, false>(acc, bv, 0.f, img, ln, ors, off);
                else if (seg == 0 && p.seg0_scale != 0.f) pp_epi_f16<false, true>(acc, bv, p.seg0_scale, img, ln, ors, off);
                else pp_epi_f16<false, false>(acc, bv, 0.f, img, ln, ors, off);
                if (!more) break;
            }
            continue;
        }
        pp_main<true>(p, smem, wbase, sg, acc);

        // EPI_RESID_F32: residual values of four 16-row blocks (64 VGPRs: the fragment registers are dead here), fetched through a
        // buffer descriptor over x[M][ldo]: rows >= M of the last, partial M-panel fall outside it, so their loads return 0 and
        // their stores are dropped by the hardware -- no per-row guard (a guard makes hipcc wrap each row block's stores in an
        // exec-masked region behind s_waitcnt vmcnt(0), and on gfx950 vmcnt counts STORES too: the row blocks would go out one
        // store round trip after the other)
        f32x4 rs[4][4];
        __amdgpu_buffer_rsrc_t xrs;
        unsigned xoff = 0;
        if (EPI == EPI_RESID_F32) {
            xrs = __builtin_amdgcn_make_buffer_rsrc(p.out[0], 0, (int)((long)p.M * p.ldo * 4), 0x00020000);
            int ln = threadIdx.x;
            asm volatile("" : "+v"(ln));   // recomputed per tile (a hoisted lane constant is spilled, and its reload drains vmcnt: pp_source)
            xoff = (unsigned)(((long)(m0 + (ln >> 8) * 128 + (ln & 15)) * p.ldo + n0 + ((ln >> 6) & 3) * 64 + 4 * ((ln >> 4) & 3)) * 4);   // row block i at + 64 i ldo, piece j at + 64 j
#pragma unroll
            for (int ii = 0; ii < 4; ii++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    rs[ii][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, xoff + (unsigned)(64 * ii * p.ldo + 64 * j), 0, 0));
        }
        // every wave is through its last phase: the ring is free.  Start the next tile's first fetches now.
        const bool more = pp_next(p, smem, w, par, vb, ntn, ntm, tm, tn, sg);
        f32x4 bv[4];
        pp_bias4(smem, par, wn, lane, bv);

        // ---- epilogue of tile (m0, n0) ----
        if (EPI == EPI_RESID_F32) {
            // x[m][n] += acc + bias.  r01/r02 took the residual tile as the INITIAL accumulator: 32 loads per lane queued behind the
            // twelve prologue DMAs and waited for before the first MFMA -- 12.8 us of every 57 us out-proj tile with the matrix
            // pipe idle (profiles/r03_gstamps.txt).  Now the tile is fetched here, after the main loop, 16 loads per
            // lane at a time into the registers the fragments no longer need (the first sixteen were issued BEFORE the next tile's
            // prologue DMAs, see above), added in the reference's order x + (A.W + bias), and stored: the residual traffic runs
            // under the next tile's first fetches instead of in front of this tile's first MFMA.
#pragma unroll
            for (int ii = 0; ii < 4; ii++)
#pragma unroll
                for (int j = 0; j < 4; j++)   // the four 64-byte pieces of one 256-byte row segment back to back
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, rs[ii][j] + (acc[ii][j] + bv[j])), xrs, xoff + (unsigned)(64 * ii * p.ldo + 64 * j), 0, 0);
#pragma unroll
            for (int ii = 0; ii < 4; ii++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    rs[ii][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, xoff + (unsigned)(64 * (4 + ii) * p.ldo + 64 * j), 0, 0));
#pragma unroll
            for (int ii = 0; ii < 4; ii++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, rs[ii][j] + (acc[4 + ii][j] + bv[j])), xrs, xoff + (unsigned)(64 * (4 + ii) * p.ldo + 64 * j), 0, 0);
        } else {
            // EPI_CONV2_F32: f32 outputs straight from the accumulators: lane holds columns n = nb + 4 fq + r (16 B) of row m = mb + fr
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int n = n0 + wn * 64 + 16 * j + 4 * fq;
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const int m = m0 + wm * 128 + 16 * i + fr;
                    if (m >= p.M) continue;
                    const f32x4 v = acc[i][j] + bv[j];
                    const int s = m - (int)__umulhi((unsigned)m, p.s_magic) * p.S;
                    const f32x4 pe = *reinterpret_cast<const f32x4 *>(p.pos + (long)s * p.N + n);
                    f32x4 o = {gelu_tanh_f(v[0]) + pe[0], gelu_tanh_f(v[1]) + pe[1], gelu_tanh_f(v[2]) + pe[2],
                               gelu_tanh_f(v[3]) + pe[3]};
                    *reinterpret_cast<f32x4 *>(reinterpret_cast<float *>(p.out[0]) + (long)m * p.ldo + n) = o;
                }
            }
        }
        if (!more) break;
    }
}

// CU count of the CURRENT device, cached per device (one process may drive several GPUs from several threads)
static int device_cu_count() {
    static std::atomic<int> cus[NH_MAX_DEVICES];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= NH_MAX_DEVICES) return 256;
    int n = cus[dev].load(std::memory_order_relaxed);
    if (!n) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

static GemmParams with_magics(const GemmParams &p_in) {
    GemmParams p = p_in;
    const long max_m = (long)p.M - 1;     // the largest row index a kernel divides (tail rows are clamped or skipped first)
    p.a_magic = nh_magic(p.a_rpb, max_m); p.o_magic = nh_magic(p.o_rpb, max_m); p.s_magic = nh_magic(p.S, max_m);
    return p;
}

// What the 256 x 256 kernel assumes beyond its shape: every row division is one multiply-high (no magic of the "divide" class),
// operand and output offsets fit 32 bits for every row of the last, partial M-panel too, and a row-mapped output does not
// overlap itself.  Fills in the fp16 epilogues' row map (GemmParams::e_*).  A launch that does not fit runs the 128 x 128 kernel.
static bool plan_gemm256(GemmParams &p) {
    const bool f16 = p.epi == EPI_F16 || p.epi == EPI_GELU_F16;
    if (p.N % G2_BN != 0 || p.K % 128 != 0 || p.M < G2_BM || (f16 && p.seg_n % G2_BN != 0)) return false;
    const unsigned long long lim = 0xffffffffull;
    const long rows = ((long)p.M + G2_BM - 1) / G2_BM * G2_BM;   // rows the tiles cover
    if (p.a_magic == ~0u || p.s_magic == ~0u) return false;
    if ((unsigned long long)(p.a_magic ? (p.M - 1) / p.a_rpb : 0) * p.a_bstride + (unsigned long long)p.M * p.lda + p.K > lim) return false;
    if (p.s_magic != 0u) {   // the V^T epilogue asks for the clip of a tile's last row, which may lie beyond M
        p.s_magic = nh_magic(p.S, rows - 1);
        if (p.s_magic == ~0u) return false;
    }
    if (!f16) return true;
    const bool hm = p.epi == EPI_F16 && p.head_major;
    const long rpb = hm ? p.S : p.o_rpb, bstride = hm ? (long)p.H * p.S : p.o_bstride;
    p.e_rs = hm ? NH_DH * 2 : (unsigned)(p.ldo * 2);
    p.e_cs = hm ? 2L * p.S : 2L;
    p.e_off0 = hm ? 0L : p.o_off * p.ldo * 2;
    p.e_magic = (rpb <= 0 || rpb >= p.M) ? 0u : nh_magic((int)rpb, rows - 1);
    if (p.e_magic == ~0u || (p.e_magic != 0u && bstride < rpb) || p.ldo * 2 > (long)lim || p.e_rs < 128u) return false;
    p.e_db = p.e_magic ? (unsigned)(bstride - rpb) : 0u;
    const unsigned long long last = ((unsigned long long)(p.e_magic ? (p.M - 1) / rpb : 0) * p.e_db + (unsigned long long)(p.M - 1)) * p.e_rs + 128;
    const unsigned long long far = ((unsigned long long)(p.e_magic ? (rows - 1) / rpb : 0) * p.e_db + (unsigned long long)(rows - 1)) * p.e_rs + 128;
    if (far > lim) return false;
    p.e_bound = (unsigned)last;
    if (p.epi == EPI_F16 && p.vt_seg >= 0) {
        if (p.S <= 0) return false;
        const unsigned long long vb = (unsigned long long)((p.M + p.S - 1) / p.S) * p.H * NH_DH * NH_SP * 2;
        if (vb > PP_VT_OOB) return false;
        p.vt_bytes = (unsigned)vb;
    }
    return true;
}

void launch_gemm(const GemmParams &p_in, hipStream_t st) {
    GemmParams p = with_magics(p_in);
    if (plan_gemm256(p)) {
        const int nwg = (p.N / G2_BN) * ((p.M + G2_BM - 1) / G2_BM);
        int cus = p.cus > 0 ? p.cus : device_cu_count();  // persistent grid: one workgroup per CU the stream can reach
        cus -= cus % 8;  // the tile order assumes workgroups b and b + gridDim.x sit on the same XCD
        const dim3 grid(nwg < cus ? nwg : cus), block(512);
        switch (p.epi) {  // one instantiation per epilogue: a single accumulator-init / store path each (register pressure)
            case EPI_F16: hipLaunchKernelGGL(gemm256_f16_kernel<EPI_F16>, grid, block, 0, st, p); break;
            case EPI_GELU_F16: hipLaunchKernelGGL(gemm256_f16_kernel<EPI_GELU_F16>, grid, block, 0, st, p); break;
            case EPI_RESID_F32: hipLaunchKernelGGL(gemm256_f16_kernel<EPI_RESID_F32>, grid, block, 0, st, p); break;
            default: hipLaunchKernelGGL(gemm256_f16_kernel<EPI_CONV2_F32>, grid, block, 0, st, p); break;
        }
        return;
    }
    launch_gemm_128(p, st);
}

// the 128 x 128 kernel on any supported shape (N % 128 == 0, K % 64 == 0); also the reference of tools/gemm_check
void launch_gemm_128(const GemmParams &p_in, hipStream_t st) {
    const GemmParams p = with_magics(p_in);
    int ntn = p.N / BN, ntm = (p.M + BM - 1) / BM;
    hipLaunchKernelGGL(gemm_f16_kernel, dim3(ntn * ntm), dim3(256), 0, st, p);
}
