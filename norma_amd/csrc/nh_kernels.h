// nh_kernels.h -- internal launch interface between the C-ABI layer (nh_*.hip) and the gfx950
// kernels.  Not part of the public ABI (that is include/norma_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>

#include "skinny_plan.h"

typedef _Float16 half_t;
typedef __attribute__((ext_vector_type(8))) _Float16 half8;
typedef __attribute__((ext_vector_type(4))) _Float16 half4;
typedef __attribute__((ext_vector_type(2))) _Float16 half2v;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

#define NH_MELP 128   // mel channels padded to 128 in the fp16 conv1 input (K = 3*128)
#define NH_SP 1536    // encoder sequence padded to a multiple of 64 for the V^T image
#define NH_DH 64      // head dim of every Whisper size
#define NH_MAX_DEVICES 64  // per-device caches of the launchers (one process may hold contexts on several GPUs)
#define NH_MAX_VOCAB 65536 // launch_logit_step holds a row in registers: LSPLIT (8) workgroups x 256 threads x LMAX (32)

// ---- big MFMA GEMM: C[M][N] = A[M][K] . W[N][K]^T (+bias), fp16 in, fp32 accumulate ------------
enum GemmEpi {
    EPI_F16 = 0,        // fp16 out = acc + bias, up to 3 column segments with own destinations
    EPI_GELU_F16 = 1,   // fp16 out = gelu_tanh(acc + bias)
    EPI_RESID_F32 = 2,  // f32 x[m][n] += acc + bias
    EPI_CONV2_F32 = 3,  // f32 x[m][n] = gelu_tanh(acc + bias) + pos[m % S][n]
};

struct GemmParams {
    const half_t *A; long lda; int a_rpb; long a_bstride;  // row m at A + (m/a_rpb)*a_bstride + (m%a_rpb)*lda
    const half_t *W;    // [N][K]
    const float *bias;  // [N] or nullptr
    int M, N, K;
    int epi;
    void *out[3]; int seg_n; long ldo;          // EPI_F16*: column segment s = n / seg_n goes to out[s]
    int o_rpb; long o_bstride; long o_off;      // output row = (m/o_rpb)*o_bstride + (m%o_rpb) + o_off
    int vt_seg;                                 // segment written as V^T [b][h][64][SP] (or -1)
    int head_major;                             // EPI_F16: every segment is written [b][h][S][64] (clip b = m / S, 64-wide head h)
                                                // instead of [m][seg_n]: the decoder streams cross K/V per (clip, head)
    float seg0_scale;                           // EPI_F16: segment 0 is written as (acc + bias) * seg0_scale (0 = no scaling): the encoder's
                                                // q carries the softmax scale dh^-1/2 * log2(e) into the attention kernel
    int S, H;                                   // rows per clip / heads (V^T and conv2 epilogues)
    const float *pos;                           // conv2: positional embedding [S][N]
    int cus;                                    // workgroups of the persistent grid; 0 = one per CU (tools/cumask runs it on CU-masked streams)
    // filled in by launch_gemm: multipliers for the kernels' integer divisions by a_rpb, o_rpb and S (nh_magic / nh_div below)
    unsigned a_magic, o_magic, s_magic;
    // filled in by launch_gemm for the 256 x 256 kernel's fp16 epilogues: ONE row map for the row-major, row-mapped (conv1) and
    // head-major outputs.  A wave's 64 columns start e_off0 + (first column in the segment) * e_cs bytes into out[seg]; from
    // there row m of batch b = m / rows-per-batch lies (b * e_db + m) * e_rs bytes on (e_magic: the multiplier of that division,
    // 0 when the rows are one batch; e_db = batch stride - rows per batch, in rows), and e_bound is where the launch's last row
    // ends: the buffer descriptor's size, so rows >= M of the last tile are dropped by the hardware.  vt_bytes: size of the V^T image
    unsigned e_magic, e_db, e_rs, e_bound, vt_bytes;
    long e_off0, e_cs;
};
// m / d for 0 <= m <= max_m as one multiply-high: magic = ceil(2^32 / d), exact while m * d < 2^32.  magic == 0 encodes
// "d > every m" (quotient 0: a GEMM whose rows are one batch), magic == ~0u "outside the exact range: divide" (no shape of
// this library: d is rows per clip, <= 3000).  The kernels divide row indices by run-time constants (rows per clip, S);
// hipcc's own expansion computes the reciprocal per lane with v_rcp_iflag and keeps it live across the tile loop, where it
// does not fit beside 128 accumulators + 64 fragment registers: it is spilled, and on gfx950 the reload (a scratch load,
// counted in vmcnt) drains the LDS-DMA pipeline in front of every tile's first fetches.
static inline unsigned nh_magic(int d, long max_m) {
    if (d <= 0 || (long)d > max_m) return 0u;
    if ((unsigned long long)max_m * (unsigned long long)d >= 0x100000000ull) return ~0u;
    return (unsigned)((0x100000000ull + (unsigned)d - 1) / (unsigned)d);
}
#ifdef __HIPCC__
__device__ __forceinline__ int nh_div(int m, int d, unsigned magic) {
    return magic == 0u ? 0 : magic == ~0u ? m / d : (int)__umulhi((unsigned)m, magic);
}
#endif
void launch_gemm(const GemmParams &p, hipStream_t st);
void launch_gemm_128(const GemmParams &p, hipStream_t st);  // always the 128 x 128 kernel

// ---- skinny GEMM for the decoder: y[R][N] = x[R][K] . W[N][K]^T, R <= 96 rows -------------------
// (enum SkinnyEpi, and which kernel serves which shape: skinny_plan.h)
struct SkinnyParams {
    const half_t *x; long ldx;  // [R][K] fp16
    const half_t *W; const float *bias;
    const half_t *Wt;           // optional tile-major repack of W (launch_repack_tiles); the kernels prefer it
    int R, N, K;
    int epi;
    void *out[3]; long ldo;
    // SK_QKV: row r = b*Tn + i  (Tn new positions per sequence); k, v go to the head-major caches [b][h][ctx][64] at t0 + i
    int d, t0, Tn, ctx;
    const int32_t *pos_ptr;  // when set: i32 [B], sequence b writes its K/V at pos_ptr[b] (hipGraph replay of the decode step)
    // LayerNorm fused into the activation load (skinny_ln_supported): x is ignored, the activations are
    // LN(ln_x[r][0..K)) * ln_w + ln_b (eps 1e-5, two-pass f32 statistics), rounded to fp16 like layernorm_kernel does
    const float *ln_x, *ln_w, *ln_b;
    float ln_rk;  // 1.0f / K, filled in by launch_skinny
};
// true when launch_skinny can take its activations through the fused LayerNorm for this shape: a question about (R, N, K)
// alone, whatever the weight layout and the epilogue
inline bool skinny_ln_supported(int R, int N, int K) { return skinny_plan(R, N, K, SK_F32, false, true).kind != SKP_NONE; }

// ---- the decoder's LayerNorm arithmetic ("sliced") ------------------------------------------------
// One fixed summation tree for every LayerNorm of a decode step, whether it runs fused inside a skinny GEMM, in the
// logits kernel's staging pass or as the stand-alone kernel (rows > 32, teacher-forced views): a row of K = 128 STEPS
// values is cut into 4 slices of 32 STEPS; in slice w lane fq sums the 8 values at 32 s + 8 fq (s ascending), the four
// lanes meet as (l0 + l1) + (l2 + l3), the slices as (p0 + p1) + (p2 + p3).  Results are therefore bit-identical across
// batch sizes and across the fused / unfused paths.
#ifdef __HIPCC__
// tanh-GELU (candle's Activation::Gelu is the tanh form): 0.5 v (1 + tanh(u)) == v / (1 + exp(-2u)),
// u = sqrt(2/pi) v (1 + 0.044715 v^2), as 3 full-rate VALU ops + v_exp_f32 + add + v_rcp_f32 + mul.  The IEEE division
// and expf expansions cost ~3x that (the GELU epilogue of a 256^2 GEMM tile is 128 of these per lane with no MFMA to
// hide under), and the library expf carries fast-math flags that let the compiler fold it differently into different
// kernels; this form is explicit, so every kernel gives the same bits.  v_exp_f32 / v_rcp_f32 are 1 ulp; the result is
// then rounded to fp16 (or added to an O(1) positional embedding).  v -> -inf gives v * rcp(inf) = -0, v -> +inf gives v.
// (hipcc's default -ffp-contract=fast lets the backend fuse any mul + add it meets after inlining, differently from
// kernel to kernel; the helpers below switch that off and spell their FMAs out, so they round the same everywhere.)
__device__ __forceinline__ float gelu_tanh_fast(float v) {
#pragma clang fp contract(off)
    const float k0 = -2.0f * 0.7978845608028654f * 1.4426950408889634f;  // -2 sqrt(2/pi) log2(e)
    const float k1 = k0 * 0.044715f;
    const float m = v * __builtin_fmaf(v * v, k1, k0);
    float r = v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(m));
    asm("" : "+v"(r));  // keep the f32 product: no v_fma_mix*_f16 fusion with a following fp16 conversion (see ln_apply)
    return r;
}
__device__ __forceinline__ float ln_sum8(float acc, const f32x4 &a, const f32x4 &b) {
#pragma clang fp contract(off)
    acc += (a[0] + a[1]) + (a[2] + a[3]);
    acc += (b[0] + b[1]) + (b[2] + b[3]);
    return acc;
}
__device__ __forceinline__ float ln_sq8(float acc, const f32x4 &a, const f32x4 &b, float mean) {
#pragma clang fp contract(off)
    const f32x4 t = a - mean, u = b - mean;
    acc += __builtin_fmaf(t[1], t[1], t[0] * t[0]) + __builtin_fmaf(t[3], t[3], t[2] * t[2]);
    acc += __builtin_fmaf(u[1], u[1], u[0] * u[0]) + __builtin_fmaf(u[3], u[3], u[2] * u[2]);
    return acc;
}
// rk = 1.0f / K, computed by the host (or at compile time): hipcc turns a division by a compile-time constant into a
// multiplication by its reciprocal but divides at run time, which rounds differently
__device__ __forceinline__ float ln_mean(float sum, float rk) {
#pragma clang fp contract(off)
    return sum * rk;
}
__device__ __forceinline__ float ln_inv(float sumsq, float rk) {
#pragma clang fp contract(off)
    const float var = sumsq * rk;
    return 1.0f / sqrtf(var + 1e-5f);
}
__device__ __forceinline__ f32x4 ln_apply(const f32x4 &x, float mean, float inv, const f32x4 &g, const f32x4 &b) {
#pragma clang fp contract(off)
    const f32x4 t = (x - mean) * inv;
    f32x4 o = {__builtin_fmaf(t[0], g[0], b[0]), __builtin_fmaf(t[1], g[1], b[1]), __builtin_fmaf(t[2], g[2], b[2]),
               __builtin_fmaf(t[3], g[3], b[3])};
    // the f32 value has to exist: otherwise hipcc folds the FMA and the fp16 conversion that follows into v_fma_mixlo_f16
    // (ONE rounding, to fp16) in some kernels and keeps v_cvt_pk_f16_f32 (two roundings) in others -- different bits at ties
    asm("" : "+v"(o));
    return o;
}
#endif
// stand-alone kernel with that arithmetic (K % 128 == 0, K <= 1280); returns false when the shape is not covered
bool launch_layernorm_sliced(const float *x, const float *w, const float *b, half_t *y, float *y32, int M, int K, hipStream_t st);
// false (and nothing launched) when skinny_plan refuses the shape: R outside 1..96, K % 64 != 0, N % 4 != 0 under an epilogue
// other than SK_F32, or ln_x set where skinny_ln_supported says no
[[nodiscard]] bool launch_skinny(const SkinnyParams &p, hipStream_t st);
// out: ceil(N/16) * 16 * K halfs.  Tile-major: the MFMA A fragment of (16-row tile, 32-deep k-step) is 1 KiB contiguous, so a
// GEMV streams its weights like a memcpy (the row-major form reads 16 x 64 B per wave instruction: 3.7 vs 5.1 TB/s).
void launch_repack_tiles(const half_t *W, half_t *out, int N, int K, hipStream_t st);

// ---- kernels that do not share their CU's LDS: skinny_lds_kernel, skinny_ldsp_kernel (k_skinny.hip: the "two logits kernels
// above" of the finding below, written beside them), xabs_main_kernel (k_xabs.hip) and prefill_attn_kernel (k_prefill.hip) -------
// The two logits kernels above keep their activations in LDS and feed every MFMA from a `ds_read_b128` -- 512 threads, 288-358
// of a SIMD's 512 registers, 40-120 KB of LDS: other kernels' workgroups fit beside them on a CU.  r03 found that they must not:
// the log-mel kernel of ANOTHER context (37 KB of LDS, 4 waves) gave wrong spectra in 1-250 frames of a clip whenever one of these
// workgroups ran beside it (tools/dbg/stress_mel.py: 150-190 wrong clip-mels in 3200 next to 64-row decodes, 6 in 9600 next to
// 32-row ones, none next to 16-row ones or with nothing running; `tools/ldsprobe` shows LDS allocations and barriers of
// co-resident workgroups do stay apart).  Stripping the kernel showed what it takes: the LDS read feeding the MFMA -- without the
// MFMAs (LDS reads into VALU adds), or with the MFMA's B operand taken from registers instead, the neighbour's results are right;
// stores, weight loads and the staging writes do not matter.  No software contract covers that, so these kernels do not share
// their CU's LDS: they ask for all of it, which keeps every LDS-using workgroup off the CU while they run (30 us per token).
#define NH_LDS_EXCLUSIVE (160 * 1024)
#ifdef __HIPCC__
static inline size_t lds_exclusive_bytes(size_t needed) {
#ifdef NH_DBG_SHARE_LDS   // tools/dbg/stress_mel.py's A/B switch, off in every build the Makefiles make: only what the kernel uses
    return needed;
#else
    (void)needed;
    return (size_t)NH_LDS_EXCLUSIVE;
#endif
}
// launches Kernel, which uses lds_used bytes of dynamic LDS, with the whole LDS of its CU
template <auto Kernel, class... Args>
static void launch_lds_exclusive(dim3 grid, dim3 block, size_t lds_used, hipStream_t st, Args... args) {
    // hipFuncSetAttribute acts on the CURRENT device: remember it per device (contexts on several GPUs of one
    // process, each driven by its own host thread)
    static std::atomic<bool> attr_set[NH_MAX_DEVICES];
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= NH_MAX_DEVICES || !attr_set[dev].load(std::memory_order_acquire)) {
        hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, NH_LDS_EXCLUSIVE);
        if (dev >= 0 && dev < NH_MAX_DEVICES) attr_set[dev].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds_exclusive_bytes(lds_used), st, args...);
}
#endif

// ---- elementwise / normalisation -------------------------------------------------------------------
// LayerNorm over rows of f32 x[M][d] -> fp16 y[M][d] (and optionally f32 y32[M][d])
void launch_layernorm(const float *x, const float *w, const float *b, half_t *y, float *y32, int M, int d,
                      hipStream_t st);
// decoder input: x[(b*Tn+i)][:] = E[tokens[b*tok_stride + t0 + i]][:] + P[t0+i][:]
void launch_embed(const int32_t *tokens, int tok_stride, const half_t *E, const half_t *P, float *x, int B,
                  int Tn, int t0, const int32_t *pos_ptr, int d, hipStream_t st);
// the ragged rows of the one-pass forward (PfClip below; n clips, Tmax the longest): x[off_z + i][:] = E[tokens[row_z * tok_stride + i]][:] + P[i][:], i < T_z
struct PfClip;
void launch_embed_ragged(const int32_t *tokens, int tok_stride, const half_t *E, const half_t *P, float *x, const PfClip *clips, int n,
                         int Tmax, int d, hipStream_t st);

// ---- sample conversion (src/dtype.rs / dasp_sample): native capture samples -> f32 PCM -------------------------------
#ifdef __HIPCC__
// dasp_sample's conversions to f32 (the capture side of the reference converts every native sample type to Model::Data with
// Sample::to_sample, src/lib.rs:180,207; the admissible types are src/dtype.rs:37-45).  Signed: s / 2^(bits - 1); unsigned:
// (s - 2^(bits - 1)) / 2^(bits - 1), the subtraction in integers; f64: round to nearest.  Integer -> float conversions
// round to nearest even (v_cvt_f32_i32, and the compiler's i64 sequence), like Rust's `as f32`; the divisions are by
// powers of two, i.e. exact.  resample_kernel is their one user: nh_logmel_samples is a resample at 16 kHz, one channel.
template <typename T> __device__ __forceinline__ float sample_to_f32(T v);
template <> __device__ __forceinline__ float sample_to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float sample_to_f32<double>(double v) { return (float)v; }
template <> __device__ __forceinline__ float sample_to_f32<int8_t>(int8_t v) { return (float)v * (1.0f / 128.0f); }
template <> __device__ __forceinline__ float sample_to_f32<int16_t>(int16_t v) { return (float)v * (1.0f / 32768.0f); }
template <> __device__ __forceinline__ float sample_to_f32<int32_t>(int32_t v) { return (float)v * (1.0f / 2147483648.0f); }
template <> __device__ __forceinline__ float sample_to_f32<int64_t>(int64_t v) { return (float)v * (1.0f / 9223372036854775808.0f); }
template <> __device__ __forceinline__ float sample_to_f32<uint8_t>(uint8_t v) { return (float)((int)v - 128) * (1.0f / 128.0f); }
template <> __device__ __forceinline__ float sample_to_f32<uint16_t>(uint16_t v) { return (float)((int)v - 32768) * (1.0f / 32768.0f); }
template <> __device__ __forceinline__ float sample_to_f32<uint32_t>(uint32_t v) { return (float)(int32_t)(v ^ 0x80000000u) * (1.0f / 2147483648.0f); }
template <> __device__ __forceinline__ float sample_to_f32<uint64_t>(uint64_t v) { return (float)(int64_t)(v ^ 0x8000000000000000ull) * (1.0f / 9223372036854775808.0f); }
#endif

// ---- audio ingest: channel mixdown + polyphase resampling to 16 kHz (k_resample.hip; the contract is DESIGN.md 10) --------
struct ResampleClip {   // one clip of a launch (device memory)
    long long off;      // first frame of the clip's window inside `frames`, in frames
    long long num0;     // source position of output 0 in units of 1/L frame, >= 0
    int n_frames;       // frames the window holds; frames outside [0, n_frames) contribute nothing
    int n_out;          // outputs to write, <= 480000
};
struct ResampleParams {
    const void *frames; // interleaved native samples (device memory)
    int dtype, channels;            // NH_SAMPLE_*, 1 .. 8
    const ResampleClip *clips; int batch;
    const float *coef;  // [L][T]: row p holds f32(h(p/L - k)), k = -T/2 + 1 .. T/2; unused when T == 0
    int L, M, T;        // T == 0 (L == M == 1): the source is at 16 kHz already, y[n] = mono[num0 + n]
    float *out; long out_stride;    // clip b writes out[b * out_stride + n]
    int max_out;        // largest n_out of the launch (sizes the grid)
};
#define NH_RS_TILE 2048   // outputs per workgroup: its window of mono frames is ((TILE - 1) M / L + T + 2) floats of LDS
static inline size_t resample_lds_bytes(int L, int M, int T) {
    return sizeof(float) * (size_t)(((long long)(NH_RS_TILE - 1) * M + L - 1) / L + T + 2);
}
// false (nothing launched): the window does not fit the LDS of a CU, or an unknown sample type
[[nodiscard]] bool launch_resample(const ResampleParams &p, hipStream_t st);

// ---- long recordings: frame energies, window energies and the cut search (k_cut.hip; the contract is DESIGN.md 11) -------
#define NH_CUT_FRAME 160      // == NH_CUT_HOP of the public header
#define NH_CUT_TILE 128       // frames per workgroup of the energy kernel
#define NH_CUT_ROW 161        // LDS row stride in floats: 160 would put the 32 lanes that read one column onto one bank
static inline size_t cut_lds_bytes() { return sizeof(float) * (size_t)NH_CUT_TILE * NH_CUT_ROW; }
// e[f] for f < n_frames: the ordered sum of squares of pcm[160 f .. 160 f + 159] (device memory), samples at or past
// n_valid taken as 0.  1 <= n_valid, n_frames >= 1; pcm[0] must be readable.
void launch_cut_energy(const float *pcm, long long n_valid, float *e, long long n_frames, hipStream_t st);
// E[f] = e[f - W] + .. + e[f + W] in that order, frames outside [0, F) adding 0.0f
void launch_cut_window(const float *e, float *E, long long F, int W, hipStream_t st);
struct CutSearch {
    const float *E; long long F;        // window energies of the F frames
    int min_frames, max_frames;         // 1 <= min_frames <= max_frames
    long long n_samples;                // of the recording: the last chunk runs up to it
    long long *starts; int32_t *lens;   // [cap]: chunk k, for k < cap
    int32_t *count;                     // [1]: the number of chunks, written last, whatever cap is
    long long cap;
};
// one workgroup walks the chunks (the sequential loop of the contract, each search a parallel arg-min)
void launch_cut_search(const CutSearch &p, hipStream_t st);
#ifdef __HIPCC__
// (best, c) of two candidates under "least E, then greatest c"; c < 0: that side has found nothing.  Neither best is ever a
// NaN: `v <= best` is false for one.
__device__ __forceinline__ void cut_merge(float &best, int &c, float ob, int oc) {
    if (oc >= 0 && (c < 0 || ob < best || (ob == best && oc > c))) { best = ob; c = oc; }
}
// One search of the contract's stage 3, by the 256 threads of a workgroup, shared by cut_search_kernel (k_cut.hip) and
// vad_pieces_kernel (k_vad.hip): returns c* - s to every thread.  Thread t looks at candidates s + min + t, + 256, ..
// ascending with the contract's `<=`, which leaves it the latest of its least; the 64 lanes of a wave meet by shuffles, the 4
// waves in w_best[4] / w_c[4] (LDS), which are free again when the call returns.  Candidates are kept relative to s (at most
// 3000: an int); the caller guarantees s + max_frames < F.
__device__ __forceinline__ int cut_search_range(const float *E, long long s, int min_frames, int max_frames, float *w_best, int *w_c) {
    const int tid = threadIdx.x;
    float best = INFINITY;
    int c = -1;
    for (int r = min_frames + tid; r <= max_frames; r += 256) {
        const float v = E[s + r];
        if (v <= best) { best = v; c = r; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oc = __shfl_xor(c, off);
        cut_merge(best, c, ob, oc);
    }
    if ((tid & 63) == 0) { w_best[tid >> 6] = best; w_c[tid >> 6] = c; }
    __syncthreads();
    best = w_best[0]; c = w_c[0];
    for (int w = 1; w < 4; w++) cut_merge(best, c, w_best[w], w_c[w]);
    __syncthreads();   // w_* are next written after this
    return c < 0 ? max_frames : c;
}
#endif

// ---- long recordings: the speech map, its pieces and chunks, and the gather (k_vad.hip; the contract is DESIGN.md 12) -------
#define NH_VAD_HIST_TILE 4096   // frames per workgroup of the select's histogram kernel
#define NH_VAD_TILE 2048        // frames per workgroup of the shaping kernels: 256 threads x 8 consecutive frames
// The state of the radix select over the monotone uint32 key of E: two ranks (Q_lo, Q_hi) walk the key's four bytes from the
// top; they share one histogram while their prefixes agree.  Zeroed before the first pass.
struct VadSelect {
    unsigned hist[2][256];   // counts of the current pass, combined over the workgroups with integer atomics
    unsigned prefix[2];      // the key bytes chosen so far (low bytes 0)
    long long rank[2];       // the rank still to find among the keys under the prefix
    int parted;              // the two prefixes differ: each rank counts into its own histogram
    int n_valid;             // F': the frames whose E is no NaN
};
struct VadLevels {
    int lo_permille, hi_permille;
    float lo_ratio, hi_ratio, abs_floor;
};
// one pass: the histogram of byte `shift / 8` of the keys under each rank's prefix ...
void launch_vad_hist(const float *E, long long F, int shift, VadSelect *sel, hipStream_t st);
// ... and the digit of both ranks; shift == 24 derives the ranks from F', shift == 0 writes levels[3] = Q_lo, Q_hi, T
void launch_vad_pick(VadSelect *sel, int shift, const VadLevels &lv, float *levels, hipStream_t st);
struct VadShape {
    const float *E; const float *levels;   // step 0 reads T = levels[2]
    long long F;
    const uint8_t *in; uint8_t *out;       // flags of whole tiles (the buffers are padded to NH_VAD_TILE; frames past F are 0)
    const int *carry_l, *carry_r;          // per tile: nearest set input frame below / above the tile (-1 / F: none)
    int *tile_l, *tile_r;                  // per tile: last / first set frame of `out` (-1 / F: none); steps 4: tile_l = starts
    int min_speech, pad, min_gap;
    long long *regions; const int *carry_n;   // step 5: a, b pairs, and the regions that start below each tile
};
// step 0: out = (E <= T), the silence flags; 1: out = v1 (in: silence); 2: out = v2 (in: v1); 3: out = v3 (in: v2); 4: region
// starts per tile (in: v3); 5: the region list (in: v3).  Steps 0 - 2 also leave tile_l / tile_r of what they wrote.
void launch_vad_shape(int step, const VadShape &p, hipStream_t st);
// one workgroup: carry_l[t] = max(tile_l[0 .. t)), carry_r[t] = min(tile_r(t .. n)) (sum == 0), or carry_l[t] = the sum of
// tile_l[0 .. t) and *total = the sum of all (sum != 0)
void launch_vad_carry(const int *tile_l, const int *tile_r, int *carry_l, int *carry_r, int n_tiles, long long F, int sum, int *total, hipStream_t st);
struct VadPieces {
    const float *E; const long long *regions; const int *n_regions;
    int min_frames, max_frames;
    long long n_samples;
    long long *starts; int32_t *lens; long long cap_pieces;   // piece k, for k < cap_pieces
    int32_t *chunk_first; long long cap_chunks;                // entries 0 .. cap_chunks
    int32_t *counts;                                           // [2]: pieces and chunks, written last, whatever the caps are
};
// one workgroup walks the regions: pieces (cut_search_range inside regions longer than max_frames) and the greedy chunks
void launch_vad_pieces(const VadPieces &p, hipStream_t st);
struct VadGather {
    const float *src; float *dst; long long dst_stride;   // chunk b's samples go to dst + b * dst_stride
    const long long *tab;   // [batch + 1] first piece of every chunk, then per piece its first sample in src, then per piece the
                            // samples of its chunk before it; the table ends with one more such entry per chunk: its total
    int n_pieces, vec4;     // vec4: src is 16-byte aligned and every piece boundary is a multiple of 4 samples
};
// one launch: PCM row b = the concatenation of chunk b's pieces; max_total: the longest row in samples
void launch_vad_gather(const VadGather &p, int batch, long long max_total, hipStream_t st);

// ---- log-mel -------------------------------------------------------------------------------------------
struct MelTables {     // device pointers, built once on the host with libm (bit-identical twiddles)
    const float *hann;      // [400]
    const float *dft_cos;   // [25][25]  cos(2pi*k*j/25) evaluated as candle's dft() does in f32
    const float *dft_sin;   // [25][25]
    const float *tw_cos;    // radix-2 twiddles for n = 50,100,200,400: offsets 0,25,75,175 (k < n/2)
    const float *tw_sin;
    const float *filters;   // [n_mel][201]
};
// pcm [B][stride] (device), n_samples[B] (device) -> mel32 f32 [B][n_mel][frames] (unnormalised
// log10) and chunk_max[B] (order-preserving uint encoding of the per-clip max, atomicMax).
// grp: [n_mel][2] first / last+1 group-of-4 index with a non-zero filter tap.
void launch_logmel_grp(const float *pcm, const int32_t *n_samples, long stride, const MelTables &t,
                       const int32_t *grp, int n_mel, int frames, float *mel32, unsigned *chunk_max, int B,
                       hipStream_t st);
// normalise=1: v = max(v, max-8)/4+1 in place; always writes the fp16 conv1 image [B][frames+2][128]
void launch_mel_finish_ex(float *mel32, const unsigned *chunk_max, half_t *img, int B, int n_mel, int frames,
                          int normalise, hipStream_t st);

// ---- encoder attention ---------------------------------------------------------------------------------
// q,k: fp16 [B*S][ld] (head h at column h*64), q PRE-SCALED by NH_ENC_Q_SCALE (GemmParams::seg0_scale);
// vt: fp16 [B][H][64][SP]; out: fp16 [B*S][ldo].  The pad columns S..SP-1 of vt are masked (their weights are exactly 0) but still
// multiplied: they must hold finite values.  The V^T epilogue of launch_gemm never writes them; the context zeroes them once.
#define NH_ENC_Q_SCALE (0.125f * 1.4426950408889634f)   // dh^-1/2 * log2(e), dh = 64
void launch_enc_attention(const half_t *q, const half_t *k, long ld, const half_t *vt, half_t *out, long ldo,
                          int B, int S, int H, hipStream_t st);

// ---- decoder attention of a decode step (one query row per (b, h)) ------------------------------------
// q: fp16 [B][d]; kc,vc: fp16 head-major [B][H][ctx][64] (the self-attention cache, or the cross K/V written with
// GemmParams::head_major); out: fp16 [B][d]; keys visible to the row: Tk
// pos_ptr != nullptr: i32 [B]; sequence b attends causally over pos_ptr[b] + 1 keys (device-side positions)
// done: i32 [B] or nullptr; sequences with done[b] != 0 are skipped (their output row is left untouched)
void launch_dec_attention(const half_t *q, const half_t *kc, const half_t *vc, half_t *out, int B, int H, int d, int ctx, int Tk,
                          const int32_t *pos_ptr, hipStream_t st, const int32_t *done);

// ---- attention of the one-pass decoder forward (k_prefill.hip): T query positions per clip at once ---------------------
// q, k, v: fp16 [B*T][ld] as the qkv GEMM leaves them (head h at column 64 h); out fp16 [B*T][ldo].  Query i of a clip sees
// the clip's keys 0 .. i; softmax(q . k / 8) in f32.  Also writes K and V of positions 0 .. T-1 into the head-major self
// cache ck / cv [b][h][C][64].  false (nothing launched): a shape it does not cover (T < 1, T > C).
// The ragged form (clips != nullptr, a device table of B entries): clip z has T_z <= T positions, its q / k / v / out rows
// packed at rows off_z .. off_z + T_z - 1, and its caches -- the self cache written, the cross K/V read -- in context row row_z;
// T is the largest T_z and sizes the grid.  The caller answers for the table: 1 <= T_z <= min(T, C), rows inside the caches,
// offsets that keep the clips' rows apart.  A clip's bits are those of the uniform launch of that clip alone.
struct PfClip { int32_t row, T, off, pad; };
bool launch_prefill_self_attention(const half_t *q, const half_t *k, const half_t *v, long ld, half_t *out, long ldo, half_t *ck,
                                   half_t *cv, int B, int T, int H, int C, hipStream_t st, const PfClip *clips = nullptr);
// q: fp16 [B*T][ldq]; ck, cv: the head-major cross K/V [b][h][S][64]; every query sees the S keys of its clip
bool launch_prefill_cross_attention(const half_t *q, long ldq, const half_t *ck, const half_t *cv, half_t *out, long ldo, int B, int T,
                                    int H, int S, hipStream_t st, const PfClip *clips = nullptr);

// numerics prototype of cross-attention on the encoder output itself (NH_OPT_ABSORBED_XATTN; k_xabs.hip): Wkv = the fused
// [2 d][d] cross K/V projection (K rows first), bkv its bias, xa fp16 [B][S][d], U scratch fp16 [B][H][d]
void launch_xabs_attention(const half_t *q, const half_t *Wkv, const float *bkv, const half_t *xa, half_t *U, half_t *out, int B, int H, int d, int S,
                           const int32_t *done, hipStream_t st);

// the one-pass form (xa streamed once per layer).  U fp16 [B][32][d] with the rows of heads >= H zero, zpart f32 [B][4][H][d],
// mlpart f32 [B][4][32][2]
bool xabs_fast_supported(int d, int H);
void launch_transpose_sq(const half_t *in, half_t *out, int d, hipStream_t st);   // out[c][r] = in[r][c], d x d, d % 32 == 0
void launch_xabs_attention_fast(const half_t *q, const half_t *WkT, const half_t *Wkv, const float *bkv, const half_t *xa, half_t *U, float *zpart, float *mlpart,
                                half_t *out, int B, int H, int d, int S, const int32_t *done, hipStream_t st);

// ---- logit processor: softmax + norma rules + argmax + bookkeeping -----------------------------------
struct DecodeState {        // all device pointers
    int32_t *tokens;        // [B][ctx]
    int32_t *n_tokens;      // [B]
    int32_t *done;          // [B] 0 running, 1 finished, 2 finished by no-speech early exit
    int32_t *have_last;     // [B]
    int32_t *last_ts;       // [B]
    double *sum_logprob;    // [B]
    double *no_speech;      // [B]
    int32_t *n_active;      // [1] running sequences after the last step
    const uint8_t *suppress;  // [V] 1 = suppressed (suppress_tokens U {no_timestamps})
};
struct RuleTokens { int sot, eot, lang, task, no_speech, no_timestamps, zero_sec, one_sec; };
// row stride of every logits buffer [B][ld]: V rounded up to 64 floats.  The pad columns are never read.
inline int nh_logits_ld(int V) { return (V + 63) & ~63; }
// mode 0: no-speech probe at prompt position 0; mode 1: generate a token from logits [B][V]; mode 2 (decode pool): every
// sequence is in the phase its own position pos_ptr[b] says -- 0: no-speech probe, < prompt_len - 1: nothing (the next prompt
// token is given), otherwise generate
// partials: f32 [B][8][8] scratch, tickets: u32 [B] zero-initialised (the kernel re-zeroes them)
// pos_ptr != nullptr: i32 [B], the position of every sequence; the kernel advances those it stepped
// 1 <= V <= NH_MAX_VOCAB (nh_create refuses larger vocabularies)
// handled != nullptr: i32 [B], written by launch_pool_sample_step earlier in the same step; a sequence whose flag is set is left alone
// pfx != nullptr (mode 2 only; nh_pool_prefix): i32 [B], the prefix length n of every row.  Row b probes at pos_ptr[b] == n, is
// inside its prompt while pos_ptr[b] < n + prompt_len - 1 (positions below n consume the prefix: nothing is selected, the
// position moves), and max_new counts from n + prompt_len.  The pointer goes by value, the lengths are read by the kernel.
void launch_logit_step(const float *logits, int V, DecodeState s, RuleTokens tk, int B, int ctx, int cap,
                       int max_new, int prompt_len, int mode, float *partials, unsigned *tickets, int32_t *pos_ptr,
                       hipStream_t st, const int32_t *handled = nullptr, const int32_t *pfx = nullptr);
// decode pool: sequence `row` restarts with the prompt [t0, t1] (P = 2) or [t0, t1, t2] (P = 3), at position 0 when pfx == nullptr;
// detect_flag != nullptr: detect_flag[row] = detect (see PoolDetect)
// pfx != nullptr: pfx[row] = n_prefix, the prompt goes to slots n_prefix .. of the row (ctx >= n_prefix + P; the caller copies
// the n_prefix ids in front of it) and the row starts at position pos0 (0: the steps consume the prefix; n_prefix: one pass does)
void launch_pool_admit(DecodeState s, int32_t *pos, unsigned *tickets, int row, int ctx, int t0, int t1, int t2, int P, hipStream_t st,
                       int32_t *detect_flag = nullptr, int detect = 0, int32_t *pfx = nullptr, int n_prefix = 0, int pos0 = 0);
// decode pool, sampled rows: how each row draws its tokens.  All device pointers, [B]; inv_t == 0: the row is greedy.
struct PoolSampling {
    float *inv_t;
    unsigned long long *seed;
    unsigned *clip, *attempt;
    int32_t *handled;       // written every step by pool_sample_step_kernel: 1 = it generated this row's token
};
// decode pool: sequence `row` decodes its clip again from position 0, sampled at 1 / inv_t; its prompt tokens [0, P) stay
// (a detected language among them: detect_flag[row], when given, is cleared).  pfx != nullptr: from position pfx[row], on the
// self K/V its prefix left in the cache
void launch_pool_retry(DecodeState s, int32_t *pos, unsigned *tickets, PoolSampling ps, int row, int P, float inv_t,
                       unsigned long long seed, unsigned clip, unsigned attempt, hipStream_t st, int32_t *detect_flag = nullptr,
                       const int32_t *pfx = nullptr);
// decode pool: launch_sample_step for the rows that are sampled (inv_t > 0), running and at a generation position
// (pos[b] >= prompt_len - 1); advances pos[b] of those and writes ps.handled[b] for every row.  Runs ahead of
// launch_logit_step(mode 2, handled = ps.handled), which does the probe, the prompt positions and the greedy rows.
// pfx: as launch_logit_step's (row b's prompt_len is pfx[b] + prompt_len).
void launch_pool_sample_step(const float *logits, int V, DecodeState s, RuleTokens tk, int B, int ctx, int cap, int max_new,
                             int prompt_len, PoolSampling ps, int32_t *pos, hipStream_t st, const int32_t *pfx = nullptr);
// t > 0: one SAMPLED token per sequence (model.rs:340-348) under the seeded contract of include/norma_hip.h;
// sequence b draws with clip id clip0 + b, step = its current token count
void launch_sample_step(const float *logits, int V, DecodeState s, RuleTokens tk, int B, int ctx, int cap, int max_new,
                        int prompt_len, float inv_t, unsigned long long seed, unsigned clip0, unsigned attempt, hipStream_t st);
// parity view: rules + one draw on an already soft-maxed probability vector (token -1: everything masked)
void launch_sample_rules(const float *probs_in, int32_t *token_out, const int32_t *tokens, int n_tokens, int last_ts,
                         const uint8_t *suppress, RuleTokens tk, int V, float inv_t, unsigned long long seed, unsigned clip,
                         unsigned attempt, hipStream_t st);
// detect_language: logits [B][ldl] at prompt position 0 -> per-sequence language token (first maximum), optional probs [B][n]
void launch_lang_detect(const float *logits, int V, const int32_t *lang_tokens, int n, float *probs_out, int32_t *lang_out,
                        int B, hipStream_t st);
// decode pool with a language table (nh_pool_detect_languages): a row whose flag is set detects its language in the step it
// takes at position 0 -- launch_lang_detect's arithmetic on that step's logits -- and writes the token into tokens[b][1].
// Goes between the step's logits and launch_logit_step(mode 2), which advances pos.
struct PoolDetect {
    const int32_t *flag;         // i32 [B]: the row was admitted with NH_LANG_DETECT (launch_pool_admit sets, launch_pool_retry clears)
    const int32_t *lang_tokens;  // i32 [n], Language::iter() order
    int n;                       // 1 .. 256; taken by value, so part of the key of the captured step graphs
    int32_t *lang_out;           // i32 [B]
    float *probs;                // f32 [B][256]
};
void launch_pool_lang_detect(const float *logits, int V, DecodeState s, int B, int ctx, const int32_t *pos, PoolDetect det,
                             hipStream_t st);
// ---- repetition guard (k_guard.hip; contract: nh_set_guard in include/norma_hip.h) ----------------------------
#define NH_GUARD_MAX_BIAS 256      // the public header's, token for token (both may be in one translation unit)
#define NH_GUARD_MAX_PERIOD 64     // loop_period at most
#define NH_GUARD_MAX_HISTORY 512   // generated tokens a row can hold: nh_set_guard refuses max_target_positions above it
// nh_guard_params as the kernel takes it, by value (so part of what a captured step bakes in: StepKey::guard_gen)
struct GuardSpec { int ngram; float penalty; int loop_period, loop_repeats, bias; };
struct GuardBufs {
    const int32_t *bias_tok;   // i32 [max_batch][NH_GUARD_MAX_BIAS] per context row; nullptr: no list was ever set
    const float *bias_val;     // f32 [max_batch][NH_GUARD_MAX_BIAS]
    const int32_t *bias_n;     // i32 [max_batch] entries of every row's list
    const int32_t *bias_map;   // i32 [R] the context row whose list row r uses (< 0: none); nullptr: row r uses list r % bias_mod
    int bias_mod;              // the clips of the batch (beam search: hypothesis row j * B + b uses clip b's list)
    int32_t *loop_exit;        // i32 [R] set when the row takes the loop exit, cleared at its first generation position
};
// Goes between the step's logits [R][nh_logits_ld(V)] and the selection kernels.  Edits the rows with done == 0 that stand at
// a generation position (pos == nullptr: all of them; decode pool: pos[r] >= prompt_len - 1); the pad columns, every other
// row and all decode state but loop_exit stay as they are.  max_target_positions <= NH_GUARD_MAX_HISTORY.
// pfx (with pos only; nh_pool_prefix): i32 [R], row r's prompt_len is pfx[r] + prompt_len.
void launch_guard(float *logits, int V, DecodeState s, RuleTokens tk, int R, int ctx, int prompt_len, const int32_t *pos, GuardSpec g,
                  GuardBufs gb, hipStream_t st, const int32_t *pfx = nullptr);
// parity helper: apply rules to one already soft-maxed probability vector
void launch_rules_only(const float *probs_in, float *masked_out, int32_t *argmax_out, const int32_t *tokens,
                       int n_tokens, int last_ts, const uint8_t *suppress, RuleTokens tk, int V, hipStream_t st);

// ---- token-level timestamps (k_align.hip; contract: nh_align in include/norma_hip.h) ----------------------------------------
#define NH_ALIGN_HEADS 32   // == NH_ALIGN_MAX_HEADS of the public header
// q capture: the heads of ONE decoder layer among the alignment heads; slot = the head's index in the caller's list
struct AlignLayerHeads { int32_t slot[NH_ALIGN_HEADS], head[NH_ALIGN_HEADS]; int n; };
// dq fp16 [B][d] (cross-attention query of that layer) -> q fp16 [slot][npos][ldb][64], ldb >= B the buffer's rows.  Every row
// b < B at its OWN position: pos_ptr[b] when pos_ptr != nullptr (captured steps, pools: nothing of the launch depends on a host
// position), the host `pos` otherwise.  Written only for rows with done[b] == 0 (running; done == nullptr: every row) at
// positions in [0, npos): finished and empty rows and positions past the buffer are left alone.
void launch_align_qsave(const half_t *dq, half_t *q, const AlignLayerHeads &lh, int B, int ldb, int d, int pos, const int32_t *pos_ptr,
                        const int32_t *done, int npos, hipStream_t st);
// Per alignment head a: q[a] + p * q_pos_stride + b * q_clip_stride = the 64 halfs of the query of clip b at position p;
// k[a] + b * k_clip_stride + s * 64 = key s of clip b (the head's slab of the head-major cross K cache).  16-byte aligned.
struct AlignHeadPtrs { const half_t *q[NH_ALIGN_HEADS]; const half_t *k[NH_ALIGN_HEADS]; };
// All three launchers work on clips clip0 .. clip0 + nclips - 1 of the batch: n_rows / n_keys (device i32, indexed by the
// clip's index in the BATCH) give the clip's rows n - 1 (clamped to max_rows) and keys (clamped to S); workspaces (W, stats,
// M, trace) are indexed by the clip's index in the GROUP, the outputs first / last by its index in the batch.  They return
// false, and launch nothing, on a shape they do not cover.
// row_map (device i32, indexed like n_rows; nullptr: the identity): the context row whose queries and cross K the clip reads
// -- the `b` of q_clip_stride / k_clip_stride above -- so that a call can work on rows that are no contiguous range (the rows
// of a decode pool).  Everything a launcher writes or sizes stays indexed as described; only the weights read through it.
// W[g][a][p][s] = softmax_s(q . k_s / 8) over s < nk, f32, for p < n_rows; nothing else of W is written.  S <= 1536.
bool launch_align_weights(const AlignHeadPtrs &hp, int A, long q_pos_stride, long q_clip_stride, long k_clip_stride, const int32_t *n_rows,
                          const int32_t *n_keys, int max_rows, int S, int nclips, int clip0, float *W, long w_clip_stride, long w_head_stride,
                          long ldw, const int32_t *row_map, hipStream_t st);
// stats f32 [nclips][A][2][S] scratch (column mean and population std over the clip's rows); M[g][r][s], r < n_rows + 1 - P:
// mean over the heads (in order) of the median of 7 along s (reflect padding, nk <= 3 unfiltered) of (W - mean) / std at
// row P - 1 + r; std == 0 gives 0.  1 <= P <= max_rows.
bool launch_align_reduce(const float *W, long w_clip_stride, long w_head_stride, long ldw, const int32_t *n_rows, const int32_t *n_keys,
                         int max_rows, int S, int nclips, int clip0, int A, int P, float *stats, float *M, long m_clip_stride, long ldm,
                         const int32_t *row_map, hipStream_t st);
// DTW on -M (R = n_rows + 1 - P rows, nk keys; tie rule and trace as nh_align states them): first / last i32 [batch][ldo],
// entries P + r get the first and last key on the path of row r, every other entry -1.  trace: u8 scratch, t_clip_stride
// >= (max_rows + 1 - P) * S per clip.  max_rows + 1 - P <= 512, ldo >= max_rows + 1.
bool launch_align_dtw(const float *M, long m_clip_stride, long ldm, const int32_t *n_rows, const int32_t *n_keys, int P, int max_rows, int S,
                      int nclips, int clip0, uint8_t *trace, long t_clip_stride, int32_t *first, int32_t *last, int ldo, const int32_t *row_map,
                      hipStream_t st);

// ---- beam search (k_beam.hip) ---------------------------------------------------------------------------------
#ifndef NH_MAX_BEAMS
#define NH_MAX_BEAMS 8   // include/norma_hip.h
#endif
// what a beam decode keeps beside DecodeState, all device pointers; rows are beam-major (hypothesis j of clip b: row j * B + b)
struct BeamBufs {
    int32_t *parent;      // [K * B] the row each row's hypothesis came from in the last step; -1: the row is dead
    int32_t *fin_tokens;  // [B][K][ctx] finished hypotheses of every clip, in finishing order, untrimmed
    int32_t *fin_n;       // [B][K]
    double *fin_score;    // [B][K] sum of log-probabilities
    int32_t *fin_count;   // [B]
};
// per live row (done == 0) its K1 <= NH_MAX_BEAMS + 1 best candidates under the logit rules: cand_tok / cand_q
// [R][NH_MAX_BEAMS + 1] (token, masked probability, best first), cand_n [R].  logits f32 [R][nh_logits_ld(V)], V <= NH_MAX_VOCAB.
void launch_beam_select(const float *logits, int V, DecodeState s, RuleTokens tk, int R, int ctx, int K1, int32_t *cand_tok,
                        float *cand_q, int32_t *cand_n, hipStream_t st);
// per clip: merge the candidates of its K rows, write the next hypotheses into rows j * B + b (state moves with its
// hypothesis), the parent map and the finished records.  A live row holds 1 <= n_tokens <= cap - 1 tokens.
void launch_beam_merge(DecodeState s, RuleTokens tk, int V, int B, int K, int ctx, int cap, int max_new, int prompt_len,
                       const int32_t *cand_tok, const float *cand_q, const int32_t *cand_n, BeamBufs bb, hipStream_t st);
// caches: device table of n_caches pointers to head-major self-attention caches fp16 [rows][H][C][64]; row r takes positions
// 0 .. npos-1 of row parent[r] in each (npos <= C; parent[r] < 0 or == r: the row stays).  Any parent map inside a clip.
void launch_beam_reorder(half_t *const *caches, int n_caches, const int32_t *parent, int B, int K, int H, int C, int npos,
                         hipStream_t st);

// ---- transcript scoring (k_score.hip) -------------------------------------------------------------------------
// Rows per launch pair: the partials [rows][ceil(V / 128)][2] f32 of a panel stay within 64 MB (a multiple of 128, >= 16384)
int score_panel_rows(int V);
// For every row m < M with target[m] >= 0: out[(m / T) * ldo + m % T + off] = log softmax(xn[m] . E^T)[target[m]], the
// plain softmax over all V columns -- l[v] = sum_k xn[m][k] E[v][k] (fp16 operands, f32, k-steps ascending into one accumulator),
// mx = max_v l, se = sum_v exp(l[v] - mx) in f32, (float)((double)(l[t] - mx) - log((double)se)).  Rows with target[m] < 0 write
// nothing.  xn fp16 [M][d], E fp16 [V][d] as stored (rows >= M / >= V are never read), target i32 [M] (< V), tlogit f32 [M]
// scratch, part f32 scratch for min(M, panel) rows x ceil(V / 128) x 2; panel_rows 0 = score_panel_rows(V), else a multiple
// of 128 not above it.  No logit reaches memory.  false (nothing launched): d % 64 != 0, V outside 1 .. NH_MAX_VOCAB, M or T < 1.
bool launch_score_rows(const half_t *xn, int M, int d, const half_t *E, int V, const int32_t *target, float *part, float *tlogit,
                       int T, long ldo, int off, float *out, int panel_rows, hipStream_t st);
