// k_resample.hip -- audio ingest on the device: sample conversion, channel mixdown and polyphase resampling to 16 kHz (gfx950).
//
// Replaces the capture side of the reference (src/lib.rs:172-216): `x.iter().sum() / channels` per frame and dasp's Sinc
// interpolator when the device's rate is not Model::SAMPLE_RATE.  The arithmetic is the contract of DESIGN.md 10, not
// dasp's (which does not lower its cut-off when it downsamples):
//   mono[f] = (s[f][0] + s[f][1] + ...) / (float)channels        f32 additions in channel order, one IEEE division
//   y[n]    = sum over k = -Wc+1 .. Wc of coef[p][k] * mono[i + k]   one f32 accumulator, fmaf, k ascending
//   i = floor((num0 + n M) / L), p = (num0 + n M) mod L               64-bit integers
// One workgroup per (tile of NH_RS_TILE outputs, clip): it loads the native frames its tile's window spans once, mixes
// them down while loading, keeps the mono f32 window in LDS, and every thread then filters its outputs from that window with
// coefficient row p from global memory (the table is at most 4 MB and stays in L2; for L == 1 every output shares one row).
// An output is the work of ONE thread over taps in a fixed order, so its bits do not depend on the tile, the batch or where
// the frames came from.  Launched with the whole LDS of its CU (launch_lds_exclusive, nh_kernels.h): one workgroup, one wave
// per SIMD, so a thread filters several outputs at once to have independent work in flight -- for L > 1 outputs of one phase
// (n, n + L, ...: one coefficient row, windows exactly M frames apart), for L == 1 outputs 256 apart.
#include "nh_kernels.h"

#define RS_PER_THREAD (NH_RS_TILE / 256)
#define RS_GROUP 13     // outputs of one phase a thread filters together: 13 * 160 covers a tile at 44 100 Hz (L = 160)
#define RS_LOADS 4

template <typename T>
__global__ __launch_bounds__(256) void resample_kernel(ResampleParams p) {
#pragma clang fp contract(off)
    extern __shared__ float rs_win[];
    const ResampleClip c = p.clips[blockIdx.y];
    const int n0 = blockIdx.x * NH_RS_TILE;
    if (n0 >= c.n_out) return;
    const int n1 = n0 + NH_RS_TILE < c.n_out ? n0 + NH_RS_TILE : c.n_out;
    const long long L = p.L, M = p.M;
    const int Wc = p.T >> 1, lo = Wc > 0 ? Wc - 1 : 0;
    // the window: frames [f_lo, f_lo + wn) cover taps -Wc+1 .. Wc of outputs n0 .. n1 - 1 (num0 >= 0: / is floor)
    const long long f_lo = (c.num0 + (long long)n0 * M) / L - lo;
    const int wn = (int)((c.num0 + (long long)(n1 - 1) * M) / L + Wc - f_lo) + 1;
    const int ch = p.channels;
    const T *src = reinterpret_cast<const T *>(p.frames) + c.off * ch;
    // RS_LOADS frames per thread in flight: the loads are unconditional (a frame outside the clip reads frame 0 and is
    // zeroed afterwards), so nothing orders one frame's load behind another's store
    for (int w0 = threadIdx.x; w0 < wn; w0 += 256 * RS_LOADS) {
        float m[RS_LOADS];
#pragma unroll
        for (int u = 0; u < RS_LOADS; u++) {
            const long long f = f_lo + w0 + 256 * u;
            const bool in = f >= 0 && f < (long long)c.n_frames;
            const T *s = src + (in ? f : 0) * ch;
            float v = sample_to_f32<T>(s[0]);
            for (int k = 1; k < ch; k++) v += sample_to_f32<T>(s[k]);
            if (ch > 1) v = v / (float)ch;
            m[u] = in ? v : 0.f;
        }
#pragma unroll
        for (int u = 0; u < RS_LOADS; u++)
            if (w0 + 256 * u < wn) rs_win[w0 + 256 * u] = m[u];
    }
    __syncthreads();
    float *out = p.out + (long)blockIdx.y * p.out_stride;
    if (p.L > 1) {
        // Outputs n and n + L share their phase, i.e. their coefficient row, and sit exactly M frames apart.  A thread takes
        // a group of up to RS_GROUP such outputs and walks their taps together: one table read per tap feeds the whole group
        // (lanes read neighbouring rows, and a row is fetched once per group instead of once per output), and the group's
        // accumulators are independent fmaf chains, each k ascending.
        const int tile_n = n1 - n0, Q = p.L * RS_GROUP;
        const int G = ((tile_n + Q - 1) / Q) * p.L;
        for (int g = threadIdx.x; g < G; g += 256) {
            const int q = g / p.L, s0 = q * Q + (g - q * p.L);   // first output of the group, relative to the tile
            if (s0 >= tile_n) continue;
            const long long num = c.num0 + (long long)(n0 + s0) * M;
            const long long i = num / L;
            const float *cf = p.coef + (long)(num - i * L) * p.T;
            const float *w = rs_win + (int)(i - lo - f_lo);
            const int last = (tile_n - 1 - s0) / p.L;             // rows of the group that exist: 0 .. last
            int off[RS_GROUP];
            float acc[RS_GROUP];
#pragma unroll
            for (int r = 0; r < RS_GROUP; r++) { off[r] = (r < last ? r : last) * p.M; acc[r] = 0.f; }   // absent rows repeat the last one, not stored
#pragma unroll 4   // several taps' table and LDS reads in flight; every accumulator still sees its taps in order
            for (int j = 0; j < p.T; j++) {
                const float cj = cf[j];
#pragma unroll
                for (int r = 0; r < RS_GROUP; r++) acc[r] = __builtin_fmaf(cj, w[off[r] + j], acc[r]);
            }
#pragma unroll
            for (int r = 0; r < RS_GROUP; r++)
                if (r <= last) out[n0 + s0 + r * p.L] = acc[r];
        }
        return;
    }
    // L == 1 (every output shares the one row, the coefficient is uniform across the workgroup) and T == 0: a thread owns
    // outputs n0 + tid + 256 r, r = 0 .. RS_PER_THREAD - 1, and walks their taps together, so that with one workgroup on the
    // CU -- one wave per SIMD -- an LDS read is in flight for one output while the others accumulate.
    const float *w[RS_PER_THREAD];
    float acc[RS_PER_THREAD];
#pragma unroll
    for (int r = 0; r < RS_PER_THREAD; r++) {
        const int n = n0 + (int)threadIdx.x + 256 * r;
        const long long num = c.num0 + (long long)(n < n1 ? n : n1 - 1) * M;   // past the tile's end: the last output again, not stored
        w[r] = rs_win + (int)(num / L - lo - f_lo);
        acc[r] = 0.f;
    }
    if (p.T == 0) {
#pragma unroll
        for (int r = 0; r < RS_PER_THREAD; r++) acc[r] = w[r][0];
    } else {
#pragma unroll 8   // the coefficients of several taps arrive in one scalar load, their LDS reads overlap
        for (int j = 0; j < p.T; j++) {
            const float cj = p.coef[j];
#pragma unroll
            for (int r = 0; r < RS_PER_THREAD; r++) acc[r] = __builtin_fmaf(cj, w[r][j], acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < RS_PER_THREAD; r++) {
        const int n = n0 + (int)threadIdx.x + 256 * r;
        if (n < n1) out[n] = acc[r];
    }
}

bool launch_resample(const ResampleParams &p, hipStream_t st) {
    const size_t lds = resample_lds_bytes(p.L, p.M, p.T);
    if (lds > (size_t)NH_LDS_EXCLUSIVE || p.batch < 1 || p.max_out < 1) return false;
    const dim3 grid((unsigned)((p.max_out + NH_RS_TILE - 1) / NH_RS_TILE), (unsigned)p.batch), block(256);
#define RS(T) launch_lds_exclusive<resample_kernel<T>>(grid, block, lds, st, p)
    switch (p.dtype) {
        case 0: RS(float); break;     case 1: RS(double); break;
        case 2: RS(int8_t); break;    case 3: RS(int16_t); break;  case 4: RS(int32_t); break;  case 5: RS(int64_t); break;
        case 6: RS(uint8_t); break;   case 7: RS(uint16_t); break; case 8: RS(uint32_t); break; case 9: RS(uint64_t); break;
        default: return false;
    }
#undef RS
    return true;
}
