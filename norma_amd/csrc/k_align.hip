// k_align.hip -- token-level timestamps (nh_align): cross-attention weights of the alignment heads, their normalisation
// (z-score over the rows, median of 7 along the keys, mean over the heads) and the dynamic-time-warping pass, per clip.
// Contract: include/norma_hip.h (nh_align) and DESIGN.md.  Every clip's arithmetic depends on that clip's rows and keys
// alone: a workgroup never mixes clips, and every reduction has one fixed order, so a clip's results are bit-identical
// whatever the batch around it.
#include <math.h>

#include "nh_kernels.h"

// ---- q capture ------------------------------------------------------------------------------------------------------------
// dq [B][d] (the cross-attention query of one layer at one position) -> q[a][pos][b][64] for the n heads of that layer, with
// ldb rows per position.  Row b goes to its own position, read from device memory when the step is a captured graph or a pool
// step (the launch then bakes in no host position), to the host's `pos` otherwise (nh_align's pass, eager decode steps).
// Rows that are not running (done != 0: finished, no-speech exit, empty) and positions outside [0, npos) write nothing.
__global__ __launch_bounds__(64) void align_qsave_kernel(const half_t *dq, half_t *qlive, AlignLayerHeads lh, int ldb, int d, int pos,
                                                         const int32_t *pos_ptr, const int32_t *done, int npos) {
    const int b = blockIdx.x, i = blockIdx.y;
    if (done && done[b] != 0) return;   // uniform over the workgroup
    const int p = pos_ptr ? pos_ptr[b] : pos;
    if (p < 0 || p >= npos) return;
    const int a = lh.slot[i], h = lh.head[i];
    qlive[(((long)a * npos + p) * ldb + b) * NH_DH + threadIdx.x] = dq[(long)b * d + h * NH_DH + threadIdx.x];
}

void launch_align_qsave(const half_t *dq, half_t *qlive, const AlignLayerHeads &lh, int B, int ldb, int d, int pos, const int32_t *pos_ptr,
                        const int32_t *done, int npos, hipStream_t st) {
    if (lh.n < 1 || B < 1 || B > ldb || npos < 1) return;
    hipLaunchKernelGGL(align_qsave_kernel, dim3(B, lh.n), dim3(64), 0, st, dq, qlive, lh, ldb, d, pos, pos_ptr, done, npos);
}

// ---- weights: W[p][s] = softmax_s(q_p . k_s / 8), s < nk ---------------------------------------------------------------------
// One workgroup (4 waves) per (16 query rows, head, clip).  Both MFMA operands come from registers, loaded straight from
// global memory in fragment order (lane l: row / key l & 15, dims 8 (l >> 4) .. + 7 of each 32-deep k-step), so no LDS feeds
// the matrix pipe ("A neighbour on the CU").  Wave w owns the 16-key tiles w, w + 4, ...; the scores of all its
// tiles (<= 24: nk <= 1536) stay in registers between the maximum, the sum and the division, so the head's K is read once per
// 16 rows (from L2 after the first row block) and W is written once.  row_map moves the two base pointers (query and K) of
// the workgroup to another context row; the fragment loads, the MFMAs and every index of W are the same with and without it.
#define AW_TILES 24
#define AW_MAX_KEYS (AW_TILES * 4 * 16)

__global__ __launch_bounds__(256) void align_weights_kernel(AlignHeadPtrs hp, long q_pos_stride, long q_clip_stride, long k_clip_stride,
                                                            const int32_t *n_rows, const int32_t *n_keys, int max_rows, int S, int clip0,
                                                            float *W, long w_clip_stride, long w_head_stride, long ldw, const int32_t *row_map) {
    __shared__ float red[2][4][16];
    const int g = blockIdx.z, a = blockIdx.y, rb = blockIdx.x * 16, b = clip0 + g;
    const int nr = min(n_rows[b], max_rows), nk = min(n_keys[b], S);
    if (rb >= nr || nk < 1) return;   // uniform over the workgroup
    const int crow = row_map ? row_map[b] : b;   // the context row that holds the clip's queries and cross K
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
    // the query fragment; rows past the clip's last are clamped (computed, never stored)
    const int qrow = min(rb + fr, nr - 1);
    const half_t *qp = hp.q[a] + (long)qrow * q_pos_stride + (long)crow * q_clip_stride + 8 * fq;
    const half8 qa0 = *reinterpret_cast<const half8 *>(qp), qa1 = *reinterpret_cast<const half8 *>(qp + 32);
    const half_t *kb = hp.k[a] + (long)crow * k_clip_stride + 8 * fq;
    const int ntiles = (nk + 15) >> 4;
    const float ninf = -INFINITY;
    f32x4 sc[AW_TILES];
    float mx[4] = {ninf, ninf, ninf, ninf};
#pragma unroll
    for (int t = 0; t < AW_TILES; t++) {
        const int tile = 4 * t + wave;
        sc[t] = f32x4{ninf, ninf, ninf, ninf};
        if (tile < ntiles) {
            const int key = 16 * tile + fr;
            // keys at or beyond nk are never read: the load is clamped to the last valid key and its score masked
            const half_t *kp = kb + (long)min(key, nk - 1) * NH_DH;
            const half8 k0 = *reinterpret_cast<const half8 *>(kp), k1 = *reinterpret_cast<const half8 *>(kp + 32);
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(qa0, k0, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(qa1, k1, c, 0, 0, 0);
            // c[r]: query row rb + 4 fq + r, key 16 tile + fr
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float s = key < nk ? c[r] * 0.125f : ninf;
                sc[t][r] = s;
                mx[r] = fmaxf(mx[r], s);
            }
        }
    }
    // row maximum: the 16 lanes of a row group, then the 4 waves
#pragma unroll
    for (int r = 0; r < 4; r++) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], o));
        if (fr == 0) red[0][wave][4 * fq + r] = mx[r];
    }
    __syncthreads();
    float sum[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = 4 * fq + r;
        mx[r] = fmaxf(fmaxf(red[0][0][row], red[0][1][row]), fmaxf(red[0][2][row], red[0][3][row]));   // finite: key 0 is valid
        sum[r] = 0.f;
    }
#pragma unroll
    for (int t = 0; t < AW_TILES; t++) {
        if (4 * t + wave < ntiles) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float e = __builtin_amdgcn_exp2f((sc[t][r] - mx[r]) * 1.4426950408889634f);   // masked keys: exp2(-inf) = 0
                sc[t][r] = e;
                sum[r] += e;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) sum[r] += __shfl_xor(sum[r], o);
        if (fr == 0) red[1][wave][4 * fq + r] = sum[r];
    }
    __syncthreads();
    float *wp = W + (long)g * w_clip_stride + (long)a * w_head_stride;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = 4 * fq + r;
        sum[r] = ((red[1][0][row] + red[1][1][row]) + red[1][2][row]) + red[1][3][row];
    }
#pragma unroll
    for (int t = 0; t < AW_TILES; t++) {
        const int key = 16 * (4 * t + wave) + fr;
        if (key < nk) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int prow = rb + 4 * fq + r;
                if (prow < nr) wp[(long)prow * ldw + key] = sc[t][r] / sum[r];
            }
        }
    }
}

bool launch_align_weights(const AlignHeadPtrs &hp, int A, long q_pos_stride, long q_clip_stride, long k_clip_stride, const int32_t *n_rows,
                          const int32_t *n_keys, int max_rows, int S, int nclips, int clip0, float *W, long w_clip_stride, long w_head_stride,
                          long ldw, const int32_t *row_map, hipStream_t st) {
    if (A < 1 || A > NH_ALIGN_HEADS || S < 1 || S > AW_MAX_KEYS || ldw < S || max_rows < 1 || nclips < 1) return false;
    hipLaunchKernelGGL(align_weights_kernel, dim3((max_rows + 15) / 16, A, nclips), dim3(256), 0, st, hp, q_pos_stride, q_clip_stride,
                       k_clip_stride, n_rows, n_keys, max_rows, S, clip0, W, w_clip_stride, w_head_stride, ldw, row_map);
    return true;
}

// ---- reduce: column statistics, then z-score -> median of 7 along the keys -> mean over the heads -------------------------------
// mean and population standard deviation of column s of W[a] over the clip's rows: one thread per column, rows in order
__global__ __launch_bounds__(256) void align_stats_kernel(const float *W, long w_clip_stride, long w_head_stride, long ldw, const int32_t *n_rows,
                                                          const int32_t *n_keys, int max_rows, int S, int clip0, float *stats, int A) {
#pragma clang fp contract(off)
    const int g = blockIdx.z, a = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x, b = clip0 + g;
    const int nr = min(n_rows[b], max_rows), nk = min(n_keys[b], S);
    if (s >= nk || nr < 1) return;
    const float *w = W + (long)g * w_clip_stride + (long)a * w_head_stride + s;
    float sum = 0.f;
    for (int p = 0; p < nr; p++) sum += w[(long)p * ldw];
    const float mean = sum / (float)nr;
    float ss = 0.f;
    for (int p = 0; p < nr; p++) {
        const float t = w[(long)p * ldw] - mean;
        ss = __builtin_fmaf(t, t, ss);
    }
    float *st = stats + (((long)g * A + a) * 2) * S;
    st[s] = mean;
    st[S + s] = sqrtf(ss / (float)nr);
}

__device__ __forceinline__ void cswap(float &x, float &y) {
    const float lo = fminf(x, y), hi = fmaxf(x, y);
    x = lo; y = hi;
}

// M[r][s] = mean over the heads of median7_s((W[a][P - 1 + r][.] - mean) / std), reflect padding; nk <= 3: no filter
__global__ __launch_bounds__(256) void align_reduce_kernel(const float *W, long w_clip_stride, long w_head_stride, long ldw, const int32_t *n_rows,
                                                           const int32_t *n_keys, int max_rows, int S, int clip0, const float *stats, int A, int P,
                                                           float *M, long m_clip_stride, long ldm) {
#pragma clang fp contract(off)
    const int g = blockIdx.z, r = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x, b = clip0 + g;
    const int nr = min(n_rows[b], max_rows), nk = min(n_keys[b], S);
    const int p = P - 1 + r;
    if (s >= nk || p >= nr) return;
    float acc = 0.f;
    for (int a = 0; a < A; a++) {
        const float *w = W + (long)g * w_clip_stride + (long)a * w_head_stride + (long)p * ldw;
        const float *st = stats + (((long)g * A + a) * 2) * S;
        float z[7];
#pragma unroll
        for (int i = 0; i < 7; i++) {
            int j = nk > 3 ? s + i - 3 : s;
            if (j < 0) j = -j;
            if (j >= nk) j = 2 * (nk - 1) - j;
            const float sd = st[S + j];
            z[i] = sd == 0.f ? 0.f : (w[j] - st[j]) / sd;
        }
        float med = z[3];
        if (nk > 3) {   // median of 7: a 13-exchange selection network for the middle element
            cswap(z[0], z[5]); cswap(z[0], z[3]); cswap(z[1], z[6]); cswap(z[2], z[4]); cswap(z[0], z[1]); cswap(z[3], z[5]);
            cswap(z[2], z[6]); cswap(z[2], z[3]); cswap(z[3], z[6]); cswap(z[4], z[5]); cswap(z[1], z[4]); cswap(z[1], z[3]);
            cswap(z[3], z[4]);
            med = z[3];
        }
        acc += med;
    }
    M[(long)g * m_clip_stride + (long)r * ldm + s] = acc / (float)A;
}

bool launch_align_reduce(const float *W, long w_clip_stride, long w_head_stride, long ldw, const int32_t *n_rows, const int32_t *n_keys,
                         int max_rows, int S, int nclips, int clip0, int A, int P, float *stats, float *M, long m_clip_stride, long ldm,
                         const int32_t *row_map, hipStream_t st) {
    (void)row_map;   // W, stats and M are the call's own: nothing here is read from a context row
    if (A < 1 || A > NH_ALIGN_HEADS || P < 1 || P > max_rows || S < 1 || ldw < S || ldm < S || nclips < 1) return false;
    hipLaunchKernelGGL(align_stats_kernel, dim3((S + 255) / 256, A, nclips), dim3(256), 0, st, W, w_clip_stride, w_head_stride, ldw, n_rows,
                       n_keys, max_rows, S, clip0, stats, A);
    hipLaunchKernelGGL(align_reduce_kernel, dim3((S + 255) / 256, max_rows - P + 1, nclips), dim3(256), 0, st, W, w_clip_stride, w_head_stride,
                       ldw, n_rows, n_keys, max_rows, S, clip0, stats, A, P, M, m_clip_stride, ldm);
    return true;
}

// ---- dynamic time warping on x = -M ----------------------------------------------------------------------------------------
// One workgroup per clip, thread i - 1 owns row i of the cost matrix; anti-diagonal k = i + j holds the cells that depend on
// diagonals k - 1 and k - 2 only, which live in LDS (three rotating arrays indexed by i).  The trace goes to HBM, one byte
// per cell; thread 0 walks it back from (R, nk).  Every cell is one f32 add of operands the rule defines exactly, so the
// path equals that of a row-by-row evaluation.
#define DTW_THREADS 512

__global__ __launch_bounds__(DTW_THREADS) void align_dtw_kernel(const float *M, long m_clip_stride, long ldm, const int32_t *n_rows,
                                                                const int32_t *n_keys, int P, int max_rows, int S, int clip0, uint8_t *trace,
                                                                long t_clip_stride, int32_t *first, int32_t *last, int ldo) {
#pragma clang fp contract(off)
    __shared__ float diag[3][DTW_THREADS + 1];
    __shared__ int32_t sfirst[DTW_THREADS], slast[DTW_THREADS];
    const int g = blockIdx.x, b = clip0 + g, tid = threadIdx.x;
    int32_t *fo = first + (long)b * ldo, *lo = last + (long)b * ldo;
    for (int i = tid; i < ldo; i += DTW_THREADS) fo[i] = lo[i] = -1;
    const int nr = min(n_rows[b], max_rows), nk = min(n_keys[b], S);
    const int R = nr + 1 - P;
    if (R < 1 || R > DTW_THREADS || nk < 1 || P + R > ldo) return;   // uniform over the workgroup
    const float inf = INFINITY;
    const float *m = M + (long)g * m_clip_stride;
    uint8_t *tr = trace + (long)g * t_clip_stride;
    // diagonal 0 holds cost[0][0] = 0, diagonal 1 the border cells (0, 1) and (1, 0)
    for (int i = tid; i <= R; i += DTW_THREADS) { diag[0][i] = i == 0 ? 0.f : inf; diag[1][i] = inf; diag[2][i] = inf; }
    sfirst[tid] = slast[tid] = -1;
    __syncthreads();
    const int i = tid + 1;
    const float *mrow = m + (long)(i - 1) * ldm;
    uint8_t *trow = tr + (long)(i - 1) * S;
    int d0 = 0, d1 = 1, d2 = 2;
    // x of this thread's cell on the next diagonal, fetched one diagonal ahead of the barrier that needs it
    float xn = (i <= R && 2 - i >= 1 && 2 - i <= nk) ? -mrow[2 - i - 1] : 0.f;
    for (int k = 2; k <= R + nk; k++) {
        const int j = k - i;
        const float x = xn;
        const int jn = j + 1;
        xn = (i <= R && jn >= 1 && jn <= nk) ? -mrow[jn - 1] : 0.f;
        if (i <= R && j >= 1 && j <= nk) {
            const float c0 = diag[d0][i - 1], c1 = diag[d1][i - 1], c2 = diag[d1][i];
            float c; uint8_t t;
            if (c0 < c1 && c0 < c2) { c = c0; t = 0; }
            else if (c1 < c0 && c1 < c2) { c = c1; t = 1; }
            else { c = c2; t = 2; }
            diag[d2][i] = x + c;
            trow[j - 1] = t;
        }
        if (tid == 0) {   // the border cells of this diagonal: (0, k) and, while k <= R, (k, 0)
            diag[d2][0] = inf;
            if (k <= R) diag[d2][k] = inf;
        }
        __syncthreads();
        const int o = d0; d0 = d1; d1 = d2; d2 = o;
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        int bi = R, bj = nk;
        while (bi >= 1 && bj >= 1) {
            if (slast[bi - 1] < 0) slast[bi - 1] = bj - 1;
            sfirst[bi - 1] = bj - 1;
            const uint8_t t = tr[(long)(bi - 1) * S + bj - 1];
            if (t == 0) { bi--; bj--; }
            else if (t == 1) bi--;
            else bj--;
        }
    }
    __syncthreads();
    if (tid < R) { fo[P + tid] = sfirst[tid]; lo[P + tid] = slast[tid]; }
}

bool launch_align_dtw(const float *M, long m_clip_stride, long ldm, const int32_t *n_rows, const int32_t *n_keys, int P, int max_rows, int S,
                      int nclips, int clip0, uint8_t *trace, long t_clip_stride, int32_t *first, int32_t *last, int ldo, const int32_t *row_map,
                      hipStream_t st) {
    (void)row_map;   // M, trace, first and last are the call's own
    if (P < 1 || max_rows < 1 || max_rows + 1 - P > DTW_THREADS || S < 1 || ldm < S || t_clip_stride < (long)(max_rows + 1 - P) * S || nclips < 1 ||
        ldo < max_rows + 1)
        return false;
    hipLaunchKernelGGL(align_dtw_kernel, dim3(nclips), dim3(DTW_THREADS), 0, st, M, m_clip_stride, ldm, n_rows, n_keys, P, max_rows, S, clip0, trace,
                       t_clip_stride, first, last, ldo);
    return true;
}
