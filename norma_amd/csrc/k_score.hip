// k_score.hip -- transcript scoring (nh_score): the log-probability of a GIVEN token at every teacher-forced
// position, without the logits ever reaching memory.
//
//   score_logits_kernel   l[m][v] = xn[m][:] . E[v][:] on 128 (rows) x 128 (vocabulary columns) MFMA tiles, and per row of a
//                         tile, from the accumulator registers: the tile's maximum, its sum of exp(l - maximum), and l[target]
//                         when the row's target column lies in the tile
//   score_merge_kernel    one wave per row: the tiles' (maximum, sum) pairs merged in ascending tile order, then
//                         (double)(l[target] - m) - log((double)se)
//
// The main loop is the 128 x 128 x 64 loop of k_gemm.hip, the same function (tile128_mainloop<true>, mfma_tile128.h: LDS-DMA
// into a swizzled double buffer, every fragment one ds_read_b128, the 32-deep k-steps of an output added in ascending order
// into one accumulator), so a logit has the bits that GEMM would give it and does not depend on M.  What differs is the guard
// on the B side: E holds exactly V rows (51864 .. 51866 are no multiple of 128), so the rows of the last column tile are
// clamped to V - 1 the way the row tail is clamped to the last row, and their columns are kept out of every statistic.
#include "k_device.h"
#include "mfma_tile128.h"

#define SC_BM 128
#define SC_BN 128
#define SC_BK 64
#define SC_LDS T128_LDS                     // two buffers of an A and a B tile; the epilogue's 2 KiB live in the first
#define SC_GM 8                             // row panels whose column tiles are neighbours in the tile order

struct ScoreParams {
    const half_t *xn;        // [M][d] final LayerNorm rows
    const half_t *E;         // [V][d] the embedding as stored
    const int32_t *target;   // [M] target column of every row; < 0: the row is not scored
    int V, d;
    int row0, rows;          // this launch: rows row0 .. row0 + rows - 1 (a panel)
    float *part;             // [rows][ceil(V / 128)][2] of the panel: tile maximum, tile sum
    float *tlogit;           // [M]
};

__global__ __launch_bounds__(256) void score_logits_kernel(ScoreParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int ntn = (p.V + SC_BN - 1) / SC_BN, ntm = (p.rows + SC_BM - 1) / SC_BM, nwg = ntn * ntm;
    // Tile order.  Workgroups b and b + 8 share an XCD (L2): every XCD gets a contiguous run of tiles, walked in groups of
    // SC_GM row panels, column tile outer / row panel inner: the 8 workgroups that follow each other on an XCD read ONE
    // 128-row slab of the embedding (320 KB at d = 1280, 133 MB in all) and 8 row panels that stay in that L2 for the sweep.
    // Nothing below depends on it: any bijection of workgroups onto tiles computes the same.
    int tm, tn;
    grouped_tile(xcd_contiguous(blockIdx.x, nwg), ntn, ntm, SC_GM, tm, tn);
    const int m0 = p.row0 + tm * SC_BM, n0 = tn * SC_BN;
    const int m_end = p.row0 + p.rows;            // rows at or past it are loaded from the last row and never stored
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w >> 1, wn = w & 1;
    const int fr = lane & 15, fq = lane >> 4;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // clamped, not branched around: rows >= M are never read, and neither are embedding rows >= V.  D[row = v][col = m]
    tile128_mainloop<true>([&](int row) { return p.xn + (long)min(m0 + row, m_end - 1) * p.d; },
                           [&](int row) { return p.E + (long)min(n0 + row, p.V - 1) * p.d; }, p.d / SC_BK, smem, acc);

    // ---- epilogue: acc[i][j][r] is column v = n0 + 64 wn + 16 i + 4 fq + r of row m = m0 + 64 wm + 16 j + fr.  A row's 128
    // columns sit in 4 lanes (fq) of each of the 2 waves wn: registers, two shuffles, one exchange through LDS.  Every order
    // below is fixed by the column index alone.  The tiles' LDS is free: every wave is past the loop's last barrier.
    float *smax = reinterpret_cast<float *>(smem), *ssum = smax + 2 * SC_BM;   // [wn][128] each
    const int vb = n0 + wn * 64 + 4 * fq;   // column of acc[0][.][0]
    int tgt[4];
#pragma unroll
    for (int j = 0; j < 4; j++) tgt[j] = p.target[min(m0 + wm * 64 + 16 * j + fr, m_end - 1)];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        float v = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (vb + 16 * i + r < p.V) v = fmaxf(v, acc[i][j][r]);
        v = fmaxf(v, __shfl_xor(v, 16));
        v = fmaxf(v, __shfl_xor(v, 32));
        if (fq == 0) smax[wn * SC_BM + wm * 64 + 16 * j + fr] = v;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int ml = wm * 64 + 16 * j + fr, m = m0 + ml;
        const float mt = fmaxf(smax[ml], smax[SC_BM + ml]);   // finite: column n0 of the tile is < V
        float s = 0.f, tv = 0.f;
        bool hit = false;
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int v = vb + 16 * i + r;
                if (v < p.V) s += __expf(acc[i][j][r] - mt);
                if (v == tgt[j]) { tv = acc[i][j][r]; hit = true; }
            }
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        if (fq == 0) ssum[wn * SC_BM + ml] = s;
        if (hit && m < m_end) p.tlogit[m] = tv;
    }
    __syncthreads();
    if (tid < SC_BM && m0 + tid < m_end) {
        f32x2 o = {fmaxf(smax[tid], smax[SC_BM + tid]), ssum[tid] + ssum[SC_BM + tid]};
        *reinterpret_cast<f32x2 *>(p.part + ((long)(m0 + tid - p.row0) * ntn + tn) * 2) = o;
    }
}

// one wave per row of the panel: lane-strided pass over the row's tiles in ascending order, the xor tree, and the double
// tail.  out[(m / T) * ldo + m % T + off]: row m = b T + p of nh_score is entry p + 1 of clip b.
__global__ __launch_bounds__(256) void score_merge_kernel(const float *__restrict__ part, const float *__restrict__ tlogit,
                                                          const int32_t *__restrict__ target, int row0, int rows, int ntn, int T,
                                                          long ldo, int off, float *__restrict__ out) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int m = row0 + r;
    if (target[m] < 0) return;   // padding and prompt rows: their entries stay 0
    const f32x2 *pp = reinterpret_cast<const f32x2 *>(part) + (long)r * ntn;
    float mx = -INFINITY, se = 0.f;
    for (int t = lane; t < ntn; t += 64) {
        const f32x2 v = pp[t];
        merge_pair(mx, se, v[0], v[1]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) merge_pair(mx, se, __shfl_xor(mx, o), __shfl_xor(se, o));
    if (lane == 0) out[(long)(m / T) * ldo + (m % T) + off] = (float)((double)(tlogit[m] - mx) - log((double)se));
}

int score_panel_rows(int V) {
    const long ntn = (V + SC_BN - 1) / SC_BN;
    return (int)((64l << 20) / (ntn * 8) / SC_BM) * SC_BM;   // >= 16384 for every V <= NH_MAX_VOCAB
}

bool launch_score_rows(const half_t *xn, int M, int d, const half_t *E, int V, const int32_t *target, float *part, float *tlogit,
                       int T, long ldo, int off, float *out, int panel_rows, hipStream_t st) {
    if (M < 1 || V < 1 || V > NH_MAX_VOCAB || d < SC_BK || d % SC_BK != 0 || T < 1) return false;
    if (panel_rows <= 0) panel_rows = score_panel_rows(V);
    if (panel_rows % SC_BM != 0 || panel_rows > score_panel_rows(V)) return false;
    const int ntn = (V + SC_BN - 1) / SC_BN;
    for (int row0 = 0; row0 < M; row0 += panel_rows) {   // the stream orders a panel's merge ahead of the next panel's tiles
        ScoreParams p{};
        p.xn = xn; p.E = E; p.target = target; p.V = V; p.d = d; p.row0 = row0; p.rows = panel_rows < M - row0 ? panel_rows : M - row0;
        p.part = part; p.tlogit = tlogit;
        const int ntm = (p.rows + SC_BM - 1) / SC_BM;
        launch_lds_exclusive<score_logits_kernel>(dim3(ntn * ntm), dim3(256), SC_LDS, st, p);
        hipLaunchKernelGGL(score_merge_kernel, dim3((p.rows + 3) / 4), dim3(256), 0, st, part, tlogit, target, row0, p.rows, ntn, T, ldo,
                           off, out);
    }
    return true;
}
