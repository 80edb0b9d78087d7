// k_cut.hip -- long recordings: where to cut a recording into clips of at most 30 s (gfx950).
//
// The reference walks a recording sequentially and re-seeks to its last timestamp (model.rs:100-146); the batched path decodes
// independent clips instead, and this file chooses their boundaries: the quietest analysis frame near the end of each clip.
// The arithmetic is the contract of DESIGN.md 11 (include/norma_hip.h has the same text), IEEE f32 and unfused:
//   e[f] = ((0 + x0 x0) + x1 x1) + .. + x159 x159      x_j = pcm[160 f + j], 0 at or past the recording's end
//   E[f] = ((0 + e[f - W]) + e[f - W + 1]) + .. + e[f + W]   a frame outside [0, F) adds 0.0f
//   cuts: s_0 = 0; while F - s > max: s <- the LATEST c in [s + min, s + max] with the least E[c], a NaN never chosen
//         (E[c] <= best, ascending, best starting at +inf), s + max when nothing qualifies
// A frame's energy is ONE thread's additions in sample order, so its bits depend neither on the tile, nor on the recording's
// length, nor on where the samples came from.
#include <math.h>

#include "nh_kernels.h"

#define CUT_LOADS 8   // samples per thread in flight while a tile is staged
static_assert((NH_CUT_TILE * NH_CUT_FRAME) % (256 * CUT_LOADS) == 0, "a tile is a whole number of load rounds");

// One workgroup per tile of NH_CUT_TILE frames.  The tile's samples are read coalesced (lane i reads sample i) into LDS rows of
// NH_CUT_ROW floats; thread t < NH_CUT_TILE then sums row t in order.  With the padded stride the 32 lanes of an LDS cycle
// read banks (t + j) mod 32: no conflict.  Launched with the whole LDS of its CU (launch_lds_exclusive, nh_kernels.h).
__global__ __launch_bounds__(256) void cut_energy_kernel(const float *pcm, long long n_valid, float *e, long long n_frames) {
#pragma clang fp contract(off)
    extern __shared__ float cut_rows[];
    const long long f0 = (long long)blockIdx.x * NH_CUT_TILE;
    const long long base = f0 * NH_CUT_FRAME;
    // the loads are unconditional (a sample past the end reads sample 0 and is zeroed afterwards), so nothing orders one
    // sample's load behind another's store
    for (int i0 = threadIdx.x; i0 < NH_CUT_TILE * NH_CUT_FRAME; i0 += 256 * CUT_LOADS) {
        float v[CUT_LOADS];
#pragma unroll
        for (int u = 0; u < CUT_LOADS; u++) {
            const long long g = base + i0 + 256 * u;
            const bool in = g < n_valid;
            const float x = pcm[in ? g : 0];
            v[u] = in ? x : 0.f;
        }
#pragma unroll
        for (int u = 0; u < CUT_LOADS; u++) {
            const int i = i0 + 256 * u, r = i / NH_CUT_FRAME;
            cut_rows[r * NH_CUT_ROW + (i - r * NH_CUT_FRAME)] = v[u];
        }
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= NH_CUT_TILE || f0 + t >= n_frames) return;
    const float *row = cut_rows + t * NH_CUT_ROW;
    float acc = 0.f;
#pragma unroll 16   // the LDS reads of several samples in flight; the additions stay one chain
    for (int j = 0; j < NH_CUT_FRAME; j++) {
        const float x = row[j];
        const float p = x * x;
        acc = acc + p;
    }
    e[f0 + t] = acc;
}

__global__ __launch_bounds__(256) void cut_window_kernel(const float *e, float *E, long long F, int W) {
#pragma clang fp contract(off)
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    float acc = 0.f;
    for (int k = -W; k <= W; k++) {
        const long long g = f + k;
        const bool in = g >= 0 && g < F;
        const float v = e[in ? g : f];
        acc = acc + (in ? v : 0.0f);
    }
    E[f] = acc;
}

// One workgroup walks the chunks; each search is cut_search_range (nh_kernels.h), thread 0 writes the chunk.  Every candidate
// lies below F, because the loop runs only while s + max < F.
__global__ __launch_bounds__(256) void cut_search_kernel(CutSearch p) {
    __shared__ float w_best[4];
    __shared__ int w_c[4];
    const int tid = threadIdx.x;
    long long s = 0, k = 0;
    while (p.F - s > (long long)p.max_frames) {
        const long long nxt = s + cut_search_range(p.E, s, p.min_frames, p.max_frames, w_best, w_c);
        if (tid == 0 && k < p.cap) {
            p.starts[k] = s * NH_CUT_FRAME;
            const long long len = (nxt - s) * NH_CUT_FRAME, left = p.n_samples - s * NH_CUT_FRAME;
            p.lens[k] = (int32_t)(len < left ? len : left);
        }
        s = nxt;
        k++;
    }
    if (tid == 0) {
        if (k < p.cap) {
            p.starts[k] = s * NH_CUT_FRAME;
            p.lens[k] = (int32_t)(p.n_samples - s * NH_CUT_FRAME);
        }
        *p.count = (int32_t)(k + 1);
    }
}

void launch_cut_energy(const float *pcm, long long n_valid, float *e, long long n_frames, hipStream_t st) {
    const dim3 grid((unsigned)((n_frames + NH_CUT_TILE - 1) / NH_CUT_TILE)), block(256);
    launch_lds_exclusive<cut_energy_kernel>(grid, block, cut_lds_bytes(), st, pcm, n_valid, e, n_frames);
}

void launch_cut_window(const float *e, float *E, long long F, int W, hipStream_t st) {
    hipLaunchKernelGGL(cut_window_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, st, e, E, F, W);
}

void launch_cut_search(const CutSearch &p, hipStream_t st) {
    hipLaunchKernelGGL(cut_search_kernel, dim3(1), dim3(256), 0, st, p);
}
