// k_vad.hip -- long recordings: which frames hold speech, how the speech packs into clips of at most 30 s, and the gather that
// builds those clips' PCM rows (gfx950).  The contract is DESIGN.md 12 (include/norma_hip.h has the same text); it starts from
// the window energies E of k_cut.hip:
//   levels  S = the non-NaN E ascending; Q_lo, Q_hi = S[permille (F' - 1) / 1000]; a = lo_ratio Q_lo, b = hi_ratio Q_hi,
//           r = b < a ? b : a, T = r > abs_floor ? r : abs_floor
//   flags   raw[f] = !(E[f] <= T)
//   shaping (a) runs of raw shorter than min_speech cleared, (b) dilation by pad, (c) inner gaps shorter than min_gap filled
//   pieces  every region, cut by k_cut.hip's rule where it is longer than max_frames; chunks: greedy, in order
// Q_lo and Q_hi are order statistics, found by a radix select over a monotone key: the histograms are integer counts, so the
// result does not depend on how the frames are dealt to workgroups.  The only float arithmetic is the two products and two
// selects of T, in one thread.  Every shaping step is a test on the nearest set frame below and above, which a pair of index
// scans delivers.  All frame indices fit an int (F <= 2^31 / 160).
#include <math.h>

#include "k_device.h"

extern __shared__ int vad_lds[];   // every kernel here that keeps data in LDS across a barrier is launched with its CU's whole LDS

// ---- order statistics ---------------------------------------------------------------------------------------------------
// (the monotone key is f32_ordered / f32_from_ordered of k_device.h)

#define VAD_HIST_LOADS (NH_VAD_HIST_TILE / 256)   // frames per thread, all loaded before the first is counted

// One workgroup per NH_VAD_HIST_TILE frames: byte `shift / 8` of every key under a rank's prefix counts into that rank's
// histogram in LDS; the 256 bins then go to the global histogram, a bin per thread.  While the ranks have not parted only
// histogram 0 is counted.  NaN frames count nowhere.
__global__ __launch_bounds__(256) void vad_hist_kernel(const float *E, long long F, int shift, VadSelect *sel) {
    unsigned *h = reinterpret_cast<unsigned *>(vad_lds);   // [2][256]
    const int tid = threadIdx.x;
    h[tid] = 0u; h[256 + tid] = 0u;
    const unsigned above = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
    const unsigned p0 = sel->prefix[0], p1 = sel->prefix[1];
    const bool parted = sel->parted != 0;
    __syncthreads();
    const long long f0 = (long long)blockIdx.x * NH_VAD_HIST_TILE;
    float v[VAD_HIST_LOADS];
#pragma unroll
    for (int u = 0; u < VAD_HIST_LOADS; u++) {   // unconditional loads (a frame past the end reads frame 0): all in flight together
        const long long f = f0 + tid + 256 * u;
        v[u] = E[f < F ? f : 0];
    }
#pragma unroll
    for (int u = 0; u < VAD_HIST_LOADS; u++) {
        const unsigned k = f32_ordered(v[u]), d = (k >> shift) & 255u;
        const bool in = f0 + tid + 256 * u < F && v[u] == v[u];
        if (in && (k & above) == p0) atomicAdd(&h[d], 1u);
        if (in && parted && (k & above) == p1) atomicAdd(&h[256 + d], 1u);
    }
    __syncthreads();
    if (h[tid]) atomicAdd(&sel->hist[0][tid], h[tid]);
    if (h[256 + tid]) atomicAdd(&sel->hist[1][tid], h[256 + tid]);
}

// ---- index scans ----------------------------------------------------------------------------------------------------------
struct VadMax { __device__ int operator()(int a, int b) const { return a > b ? a : b; } };
struct VadMin { __device__ int operator()(int a, int b) const { return a < b ? a : b; } };
struct VadAdd { __device__ int operator()(int a, int b) const { return a + b; } };

// Exclusive scan of one value per thread over the 256 threads of a workgroup: DIR > 0 over the threads below, DIR < 0 over the
// threads above.  total: over all 256.  lds: 4 ints, free again when the call returns.
template <int DIR, class Op>
__device__ __forceinline__ int vad_block_scan(int v, Op op, int ident, int *lds, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = DIR > 0 ? __shfl_up(inc, off) : __shfl_down(inc, off);
        if (DIR > 0 ? lane >= off : lane + off < 64) inc = op(inc, o);
    }
    int ex = DIR > 0 ? __shfl_up(inc, 1) : __shfl_down(inc, 1);
    if (lane == (DIR > 0 ? 0 : 63)) ex = ident;
    if (lane == (DIR > 0 ? 63 : 0)) lds[wave] = inc;
    __syncthreads();
    int carry = ident;
    total = ident;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const int t = lds[w];
        total = op(total, t);
        if (DIR > 0 ? w < wave : w > wave) carry = op(carry, t);
    }
    __syncthreads();
    return op(carry, ex);
}

// One workgroup, a bin per thread: an exclusive prefix sum over the 256 bins of each rank's histogram; the thread whose bin holds
// the rank owns that rank's digit.  The first pass derives the ranks from F' (the sum of the first histogram), the last one
// turns the keys into the levels.  Every thread reads what it needs of the state before the scans' barriers and writes after
// them; the histograms are cleared for the next pass.
__global__ __launch_bounds__(256) void vad_pick_kernel(VadSelect *sel, int shift, VadLevels lv, float *levels) {
#pragma clang fp contract(off)
    const int t = threadIdx.x;
    const bool parted = sel->parted != 0;
    const int h0 = (int)sel->hist[0][t], h1 = parted ? (int)sel->hist[1][t] : h0;   // at most F < 2^24 frames
    const unsigned p0 = sel->prefix[0], p1 = sel->prefix[1];
    long long r0 = sel->rank[0], r1 = sel->rank[1];
    int n = sel->n_valid, tot;
    const int ex0 = vad_block_scan<1>(h0, VadAdd(), 0, vad_lds, tot);
    const int ex1 = parted ? vad_block_scan<1>(h1, VadAdd(), 0, vad_lds, tot) : ex0;
    if (shift == 24) {   // not parted: tot is the sum of histogram 0
        n = tot;
        r0 = n > 0 ? (long long)lv.lo_permille * (n - 1) / 1000 : 0;
        r1 = n > 0 ? (long long)lv.hi_permille * (n - 1) / 1000 : 0;
    }
    int *digit = vad_lds + 4;   // behind the scans' four words
    if (n > 0 && r0 >= ex0 && r0 < (long long)ex0 + h0) { digit[0] = t; sel->rank[0] = r0 - ex0; }
    if (n > 0 && r1 >= ex1 && r1 < (long long)ex1 + h1) { digit[1] = t; sel->rank[1] = r1 - ex1; }
    sel->hist[0][t] = 0u;
    sel->hist[1][t] = 0u;
    __syncthreads();
    if (t != 0) return;
    const unsigned k0 = n > 0 ? p0 | ((unsigned)digit[0] << shift) : 0u, k1 = n > 0 ? p1 | ((unsigned)digit[1] << shift) : 0u;
    sel->prefix[0] = k0; sel->prefix[1] = k1;
    sel->n_valid = n;
    if (k0 != k1) sel->parted = 1;
    if (shift == 0) {
        const float q_lo = n > 0 ? f32_from_ordered(k0) : 0.0f, q_hi = n > 0 ? f32_from_ordered(k1) : 0.0f;
        const float a = lv.lo_ratio * q_lo;
        const float b = lv.hi_ratio * q_hi;
        const float r = (b < a) ? b : a;
        levels[0] = q_lo; levels[1] = q_hi;
        levels[2] = n <= 0 ? lv.abs_floor : (r > lv.abs_floor) ? r : lv.abs_floor;
    }
}

#define VAD_ITEMS (NH_VAD_TILE / 256)
static_assert(VAD_ITEMS == 8, "a thread's flags are one 8-byte word");

// One workgroup per tile of NH_VAD_TILE frames, thread t holding frames f0 + 8 t .. + 7.
template <int STEP>
__global__ __launch_bounds__(256) void vad_shape_kernel(VadShape p) {
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * NH_VAD_TILE + (long long)tid * VAD_ITEMS;
    const int F = (int)p.F;
    bool x[VAD_ITEMS], y[VAD_ITEMS];
    if (STEP == 0) {
        const float T = p.levels[2];
#pragma unroll
        for (int k = 0; k < VAD_ITEMS; k++) {
            const long long f = base + k;
            const float v = p.E[f < p.F ? f : 0];
            y[k] = f < p.F && v <= T;
        }
    } else {
        const uint2 w = *reinterpret_cast<const uint2 *>(p.in + base);
#pragma unroll
        for (int k = 0; k < VAD_ITEMS; k++) x[k] = (((k < 4 ? w.x : w.y) >> (8 * (k & 3))) & 1u) != 0u;
    }
    if (STEP >= 1 && STEP <= 3) {
        // the nearest set input frame at or below / at or above each of the thread's frames
        int last = -1, first = F;
#pragma unroll
        for (int k = 0; k < VAD_ITEMS; k++)
            if (x[k]) { last = (int)base + k; if (first == F) first = (int)base + k; }
        int tot;
        int l = vad_block_scan<1>(last, VadMax(), -1, vad_lds, tot);
        int r = vad_block_scan<-1>(first, VadMin(), F, vad_lds, tot);
        l = VadMax()(l, p.carry_l[blockIdx.x]);
        r = VadMin()(r, p.carry_r[blockIdx.x]);
        int L[VAD_ITEMS], R[VAD_ITEMS];
#pragma unroll
        for (int k = 0; k < VAD_ITEMS; k++) { if (x[k]) l = (int)base + k; L[k] = l; }
#pragma unroll
        for (int k = VAD_ITEMS - 1; k >= 0; k--) { if (x[k]) r = (int)base + k; R[k] = r; }
#pragma unroll
        for (int k = 0; k < VAD_ITEMS; k++) {
            const int f = (int)base + k;
            bool v;
            if (STEP == 1) v = !x[k] && R[k] - L[k] - 1 >= p.min_speech;                          // x: silence; the run of raw around f
            else if (STEP == 2) v = (L[k] >= 0 && f - L[k] <= p.pad) || (R[k] < F && R[k] - f <= p.pad);   // x: v1
            else v = x[k] || (L[k] >= 0 && R[k] < F && R[k] - L[k] - 1 < p.min_gap);            // x: v2; the gap around f
            y[k] = v && f < F;
        }
    }
    if (STEP <= 3) {
        uint2 w = make_uint2(0u, 0u);
#pragma unroll
        for (int k = 0; k < VAD_ITEMS; k++) (k < 4 ? w.x : w.y) |= (y[k] ? 1u : 0u) << (8 * (k & 3));
        *reinterpret_cast<uint2 *>(p.out + base) = w;
    }
    if (STEP <= 2) {   // what the next step's scan needs of this tile
        int last = -1, first = F;
#pragma unroll
        for (int k = 0; k < VAD_ITEMS; k++)
            if (y[k]) { last = (int)base + k; if (first == F) first = (int)base + k; }
        int tl, tr;
        vad_block_scan<1>(last, VadMax(), -1, vad_lds, tl);
        vad_block_scan<-1>(first, VadMin(), F, vad_lds, tr);
        if (tid == 0) { p.tile_l[blockIdx.x] = tl; p.tile_r[blockIdx.x] = tr; }
    }
    if (STEP >= 4) {   // x: v3.  A region starts at a set frame whose left neighbour is clear, and ends behind one whose right one is
        const bool before = base > 0 && base - 1 < p.F && p.in[base - 1] != 0;   // the neighbours across the thread's 8 frames
        const bool after = base + VAD_ITEMS < p.F && p.in[base + VAD_ITEMS] != 0;
        int n = 0;
        bool start[VAD_ITEMS];
#pragma unroll
        for (int k = 0; k < VAD_ITEMS; k++) { start[k] = x[k] && !(k == 0 ? before : x[k - 1]); n += start[k] ? 1 : 0; }
        int tot;
        int idx = vad_block_scan<1>(n, VadAdd(), 0, vad_lds, tot);
        if (STEP == 4) {
            if (tid == 0) p.tile_l[blockIdx.x] = tot;
        } else {
            idx += p.carry_n[blockIdx.x];
#pragma unroll
            for (int k = 0; k < VAD_ITEMS; k++) {
                if (start[k]) p.regions[2 * (long long)idx++] = base + k;
                // the region that ends here is the last one that started at or below this frame
                if (x[k] && !(k == VAD_ITEMS - 1 ? after : x[k + 1])) p.regions[2 * (long long)(idx - 1) + 1] = base + k + 1;
            }
        }
    }
}

// One workgroup.  Thread t takes the tiles [t per, (t + 1) per): its own totals, an exclusive scan over the 256 threads, then
// the tiles again with the carry.
__global__ __launch_bounds__(256) void vad_carry_kernel(const int *tile_l, const int *tile_r, int *carry_l, int *carry_r, int n_tiles,
                                                        int F, int sum, int *total) {
    const int per = (n_tiles + 255) / 256;
    const int t0 = min(threadIdx.x * per, n_tiles), t1 = min(t0 + per, n_tiles);
    int tot;
    if (sum) {
        int n = 0;
        for (int t = t0; t < t1; t++) n += tile_l[t];
        int c = vad_block_scan<1>(n, VadAdd(), 0, vad_lds, tot);
        for (int t = t0; t < t1; t++) { carry_l[t] = c; c += tile_l[t]; }
        if (threadIdx.x == 0) *total = tot;
        return;
    }
    int last = -1, first = F;
    for (int t = t0; t < t1; t++) { last = max(last, tile_l[t]); first = min(first, tile_r[t]); }
    int l = vad_block_scan<1>(last, VadMax(), -1, vad_lds, tot);
    int r = vad_block_scan<-1>(first, VadMin(), F, vad_lds, tot);
    for (int t = t0; t < t1; t++) { carry_l[t] = l; l = max(l, tile_l[t]); }
    for (int t = t1 - 1; t >= t0; t--) { carry_r[t] = r; r = min(r, tile_r[t]); }
}

// ---- pieces and chunks ----------------------------------------------------------------------------------------------------
// One workgroup walks the regions in order.  A region longer than max_frames is cut like a recording of its own (the same
// search as cut_search_kernel); every piece goes to the open chunk while the chunk's frames stay within max_frames.  All
// threads follow the same walk; thread 0 writes.
__global__ __launch_bounds__(256) void vad_pieces_kernel(VadPieces p) {
    float *w_best = reinterpret_cast<float *>(vad_lds);
    int *w_c = vad_lds + 4;
    const int tid = threadIdx.x;
    const int n_regions = *p.n_regions;
    long long k = 0, n_chunks = 0;
    int held = 0;   // frames of the open chunk; 0: none open
    for (int i = 0; i < n_regions; i++) {
        long long s = p.regions[2 * (long long)i];
        const long long b = p.regions[2 * (long long)i + 1];
        for (bool more = true; more;) {
            more = b - s > (long long)p.max_frames;
            const long long nxt = more ? s + cut_search_range(p.E, s, p.min_frames, p.max_frames, w_best, w_c) : b;
            const int frames = (int)(nxt - s);
            if (held == 0 || held + frames > p.max_frames) {
                if (tid == 0 && n_chunks <= p.cap_chunks) p.chunk_first[n_chunks] = (int32_t)k;
                n_chunks++;
                held = 0;
            }
            held += frames;
            if (tid == 0 && k < p.cap_pieces) {
                p.starts[k] = s * NH_CUT_FRAME;
                const long long len = (long long)frames * NH_CUT_FRAME, left = p.n_samples - s * NH_CUT_FRAME;
                p.lens[k] = (int32_t)(len < left ? len : left);
            }
            k++;
            s = nxt;
        }
    }
    if (tid == 0) {
        if (n_chunks <= p.cap_chunks) p.chunk_first[n_chunks] = (int32_t)k;
        p.counts[0] = (int32_t)k;
        p.counts[1] = (int32_t)n_chunks;
    }
}

// ---- gather ---------------------------------------------------------------------------------------------------------------
#define VAD_GATHER_SPAN 4096   // samples of a row per workgroup

// Workgroup (x, b) writes samples [x SPAN, (x + 1) SPAN) of chunk b's row.  It finds the piece of its first sample by binary
// search over the chunk's cumulative lengths; a thread then walks on from there.  V = 4: 16-byte copies (the launcher has
// checked alignment and that no piece boundary but a row's end falls inside a group of four), V = 1: dwords.
template <int V>
__global__ __launch_bounds__(256) void vad_gather_kernel(VadGather p, int batch) {
    const int b = blockIdx.y;
    const long long *first = p.tab, *src0 = p.tab + batch + 1, *off = src0 + p.n_pieces, *totals = off + p.n_pieces;
    const int j0 = (int)first[b], j1 = (int)first[b + 1];
    const long long total = totals[b], q0 = (long long)blockIdx.x * VAD_GATHER_SPAN;
    if (q0 >= total) return;
    int lo = j0, hi = j1 - 1;   // the last piece that starts at or below q0
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= q0) lo = mid; else hi = mid - 1;
    }
    int j = lo;
    float *dst = p.dst + (long long)b * p.dst_stride;
    for (long long q = q0 + (long long)threadIdx.x * V; q < q0 + VAD_GATHER_SPAN && q < total; q += 256 * V) {
        while (j + 1 < j1 && off[j + 1] <= q) j++;
        const float *s = p.src + src0[j] + (q - off[j]);
        if (V == 4 && q + 4 <= total) {
            *reinterpret_cast<float4 *>(dst + q) = *reinterpret_cast<const float4 *>(s);
        } else {   // dwords; with V = 4 the ragged end of a row, which lies in its last piece
            for (int u = 0; u < V && q + u < total; u++) dst[q + u] = s[u];
        }
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
void launch_vad_hist(const float *E, long long F, int shift, VadSelect *sel, hipStream_t st) {
    const dim3 grid((unsigned)((F + NH_VAD_HIST_TILE - 1) / NH_VAD_HIST_TILE));
    launch_lds_exclusive<vad_hist_kernel>(grid, dim3(256), sizeof(unsigned) * 512, st, E, F, shift, sel);
}

void launch_vad_pick(VadSelect *sel, int shift, const VadLevels &lv, float *levels, hipStream_t st) {
    launch_lds_exclusive<vad_pick_kernel>(dim3(1), dim3(256), sizeof(int) * 6, st, sel, shift, lv, levels);
}

template <int STEP>
static void vad_shape_launch(const VadShape &p, hipStream_t st) {
    const dim3 grid((unsigned)((p.F + NH_VAD_TILE - 1) / NH_VAD_TILE));
    launch_lds_exclusive<vad_shape_kernel<STEP>>(grid, dim3(256), sizeof(int) * 4, st, p);
}

void launch_vad_shape(int step, const VadShape &p, hipStream_t st) {
    switch (step) {
    case 0: vad_shape_launch<0>(p, st); break;
    case 1: vad_shape_launch<1>(p, st); break;
    case 2: vad_shape_launch<2>(p, st); break;
    case 3: vad_shape_launch<3>(p, st); break;
    case 4: vad_shape_launch<4>(p, st); break;
    default: vad_shape_launch<5>(p, st); break;
    }
}

void launch_vad_carry(const int *tile_l, const int *tile_r, int *carry_l, int *carry_r, int n_tiles, long long F, int sum, int *total,
                      hipStream_t st) {
    launch_lds_exclusive<vad_carry_kernel>(dim3(1), dim3(256), sizeof(int) * 4, st, tile_l, tile_r, carry_l, carry_r, n_tiles, (int)F, sum, total);
}

void launch_vad_pieces(const VadPieces &p, hipStream_t st) {
    launch_lds_exclusive<vad_pieces_kernel>(dim3(1), dim3(256), sizeof(int) * 8, st, p);
}

void launch_vad_gather(const VadGather &p, int batch, long long max_total, hipStream_t st) {
    const dim3 grid((unsigned)((max_total + VAD_GATHER_SPAN - 1) / VAD_GATHER_SPAN), (unsigned)batch);
    if (p.vec4) hipLaunchKernelGGL(vad_gather_kernel<4>, grid, dim3(256), 0, st, p, batch);
    else hipLaunchKernelGGL(vad_gather_kernel<1>, grid, dim3(256), 0, st, p, batch);
}
