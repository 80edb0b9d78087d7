// kref.hip -- test-only C entry points onto the shipped launchers of nh_kernels.h (tests/kref.py, tests/test_gpu_kernel_ref.py).
// Linked against the library's own objects (norma_amd/csrc/build/k_*.o): the kernels under test are the product's, not copies.
// Every entry point takes host buffers (sizes in bytes), allocates device copies, copies every buffer in -- outputs too, so a
// test can see what a kernel must leave alone (done rows, cache positions it does not own) --, launches on a stream of its own,
// synchronises, copies the outputs back and frees.  It returns the hipError_t, or -1 when the launcher refuses the shape.
#include <vector>

#include "../norma_amd/csrc/nh_kernels.h"

namespace {
struct Bufs {
    std::vector<void *> dev;
    hipError_t err = hipSuccess;
    // device copy of `bytes` host bytes (nullptr in, nullptr out)
    template <class T> T *in(const void *host, size_t bytes) {
        if (!host || err != hipSuccess) return nullptr;
        void *d = nullptr;
        if ((err = hipMalloc(&d, bytes ? bytes : 16)) != hipSuccess) return nullptr;
        dev.push_back(d);
        if ((err = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice)) != hipSuccess) return nullptr;
        return static_cast<T *>(d);
    }
    template <class T> T *zeros(size_t bytes) {
        if (err != hipSuccess) return nullptr;
        void *d = nullptr;
        if ((err = hipMalloc(&d, bytes)) != hipSuccess) return nullptr;
        dev.push_back(d);
        if ((err = hipMemset(d, 0, bytes)) == hipSuccess) err = hipDeviceSynchronize();
        return static_cast<T *>(d);
    }
    void out(void *host, const void *d, size_t bytes) {
        if (host && d && err == hipSuccess) err = hipMemcpy(host, d, bytes, hipMemcpyDeviceToHost);
    }
    ~Bufs() {
        for (void *d : dev) (void)hipFree(d);
    }
};
struct Stream {
    hipStream_t s = nullptr;
    // a blocking stream: ordered after the copy-ins and memsets above, which run on the null stream
    Stream() { (void)hipStreamCreate(&s); }
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t finish() {
        hipError_t e = hipGetLastError();
        hipError_t e2 = hipStreamSynchronize(s);
        return e != hipSuccess ? e : e2;
    }
};
}  // namespace

#define KREF_CHECK(b) \
    do {              \
        if ((b).err != hipSuccess) return (int)(b).err; \
    } while (0)

extern "C" {

// launch_skinny (+ launch_repack_tiles when use_wt): x [R][ldx] fp16, W [N][K] fp16, bias f32 [N] or null; out0..2 as the epilogue
// says (SK_QKV: q [R][d], K/V caches [B][H][ctx][64]); pos_ptr i32 [B]; ln_x f32 [R][K], ln_w / ln_b f32 [K]
int kref_skinny(const void *x, long ldx, int R, int N, int K, const void *W, const void *bias, int use_wt, int epi,
                void *out0, size_t out0_bytes, void *out1, void *out2, size_t out12_bytes, long ldo, int d, int t0, int Tn,
                int ctx, const int32_t *pos_ptr, int B, const float *ln_x, const float *ln_w, const float *ln_b) {
    Bufs b;
    Stream st;
    SkinnyParams p{};
    p.x = b.in<half_t>(x, (size_t)R * ldx * 2);
    p.ldx = ldx;
    p.W = b.in<half_t>(W, (size_t)N * K * 2);
    p.bias = b.in<float>(bias, (size_t)N * 4);
    p.R = R; p.N = N; p.K = K; p.epi = epi;
    p.out[0] = b.in<void>(out0, out0_bytes);
    p.out[1] = b.in<void>(out1, out12_bytes);
    p.out[2] = b.in<void>(out2, out12_bytes);
    p.ldo = ldo; p.d = d; p.t0 = t0; p.Tn = Tn; p.ctx = ctx;
    p.pos_ptr = b.in<int32_t>(pos_ptr, (size_t)B * 4);
    p.ln_x = b.in<float>(ln_x, (size_t)R * K * 4);
    p.ln_w = b.in<float>(ln_w, (size_t)K * 4);
    p.ln_b = b.in<float>(ln_b, (size_t)K * 4);
    KREF_CHECK(b);
    if (use_wt) {
        half_t *wt = b.zeros<half_t>((size_t)((N + 15) / 16) * 16 * K * 2);
        KREF_CHECK(b);
        launch_repack_tiles(p.W, wt, N, K, st.s);
        p.Wt = wt;
    }
    if (!launch_skinny(p, st.s)) return -1;
    if (hipError_t e = st.finish()) return (int)e;
    b.out(out0, p.out[0], out0_bytes);
    b.out(out1, p.out[1], out12_bytes);
    b.out(out2, p.out[2], out12_bytes);
    return (int)b.err;
}

int kref_skinny_ln_supported(int R, int N, int K) { return skinny_ln_supported(R, N, K) ? 1 : 0; }

// launch_dec_attention: q [B][d]; kc, vc [B][ctx][d] or head-major [B][H][ctx][64]; out [B][d] (copied in: done rows stay)
int kref_dec_attention(const void *q, const void *kc, const void *vc, void *out, int B, int H, int d, int ctx, int Tk,
                       const int32_t *pos_ptr, int kv_head_major, const int32_t *done) {
    Bufs b;
    Stream st;
    const size_t kv = (size_t)B * ctx * d * 2;
    const half_t *dq = b.in<half_t>(q, (size_t)B * d * 2), *dk = b.in<half_t>(kc, kv), *dv = b.in<half_t>(vc, kv);
    half_t *dout = b.in<half_t>(out, (size_t)B * d * 2);
    const int32_t *dpos = b.in<int32_t>(pos_ptr, (size_t)B * 4), *ddone = b.in<int32_t>(done, (size_t)B * 4);
    KREF_CHECK(b);
    launch_dec_attention(dq, dk, dv, dout, B, 1, H, d, ctx, Tk, dpos, st.s, kv_head_major, ddone);
    if (hipError_t e = st.finish()) return (int)e;
    b.out(out, dout, (size_t)B * d * 2);
    return (int)b.err;
}

// absorbed cross-attention, both forms: Wkv [2d][d] (K rows first), bkv f32 [2d], xa [B][S][d]; fast = 1: the one-pass kernels
// (U scratch [B][32][d] zeroed, so the rows of heads >= H are zero as the launcher requires)
int kref_xabs_attention(const void *q, const void *Wkv, const float *bkv, const void *xa, void *out, int B, int H, int d, int S,
                        const int32_t *done, int fast) {
    Bufs b;
    Stream st;
    const half_t *dq = b.in<half_t>(q, (size_t)B * d * 2), *dw = b.in<half_t>(Wkv, (size_t)2 * d * d * 2);
    const float *dbkv = b.in<float>(bkv, (size_t)2 * d * 4);
    const half_t *dxa = b.in<half_t>(xa, (size_t)B * S * d * 2);
    half_t *dout = b.in<half_t>(out, (size_t)B * d * 2);
    const int32_t *ddone = b.in<int32_t>(done, (size_t)B * 4);
    half_t *U = b.zeros<half_t>((size_t)B * 32 * d * 2);
    KREF_CHECK(b);
    if (!fast) {
        launch_xabs_attention(dq, dw, dbkv, dxa, U, dout, B, H, d, S, ddone, st.s);
    } else {
        if (!xabs_fast_supported(d, H)) return -1;
        half_t *wkt = b.zeros<half_t>((size_t)d * d * 2);
        float *zpart = b.zeros<float>((size_t)B * 4 * H * d * 4), *ml = b.zeros<float>((size_t)B * 4 * 32 * 2 * 4);
        KREF_CHECK(b);
        launch_transpose_sq(dw, wkt, d, st.s);
        launch_xabs_attention_fast(dq, wkt, dw, dbkv, dxa, U, zpart, ml, dout, B, H, d, S, ddone, st.s);
    }
    if (hipError_t e = st.finish()) return (int)e;
    b.out(out, dout, (size_t)B * d * 2);
    return (int)b.err;
}

// launch_enc_attention: q, k [B*S][ld] (q pre-scaled by NH_ENC_Q_SCALE), vt [B][H][64][NH_SP], out [B*S][ldo]
int kref_enc_attention(const void *q, const void *k, long ld, const void *vt, void *out, long ldo, int B, int S, int H) {
    Bufs b;
    Stream st;
    const half_t *dq = b.in<half_t>(q, (size_t)B * S * ld * 2), *dk = b.in<half_t>(k, (size_t)B * S * ld * 2);
    const half_t *dvt = b.in<half_t>(vt, (size_t)B * H * NH_DH * NH_SP * 2);
    half_t *dout = b.in<half_t>(out, (size_t)B * S * ldo * 2);
    KREF_CHECK(b);
    launch_enc_attention(dq, dk, ld, dvt, dout, ldo, B, S, H, st.s);
    if (hipError_t e = st.finish()) return (int)e;
    b.out(out, dout, (size_t)B * S * ldo * 2);
    return (int)b.err;
}

// launch_gemm (kernel128 = 0) or launch_gemm_128: A is a buffer of a_bytes that the row map (a_rpb, a_bstride, lda) reads,
// out0..2 buffers of out_bytes each (copied in and back), pos f32 [S][N] for EPI_CONV2_F32
int kref_gemm(int kernel128, const void *A, size_t a_bytes, long lda, int a_rpb, long a_bstride, const void *W, const float *bias,
              int M, int N, int K, int epi, void *out0, void *out1, void *out2, size_t out_bytes, int seg_n, long ldo, int o_rpb,
              long o_bstride, long o_off, int vt_seg, int head_major, float seg0_scale, int S, int H, const float *pos) {
    Bufs b;
    Stream st;
    GemmParams p{};
    p.A = b.in<half_t>(A, a_bytes);
    p.lda = lda; p.a_rpb = a_rpb; p.a_bstride = a_bstride;
    p.W = b.in<half_t>(W, (size_t)N * K * 2);
    p.bias = b.in<float>(bias, (size_t)N * 4);
    p.M = M; p.N = N; p.K = K; p.epi = epi;
    p.out[0] = b.in<void>(out0, out_bytes);
    p.out[1] = b.in<void>(out1, out_bytes);
    p.out[2] = b.in<void>(out2, out_bytes);
    p.seg_n = seg_n; p.ldo = ldo; p.o_rpb = o_rpb; p.o_bstride = o_bstride; p.o_off = o_off;
    p.vt_seg = vt_seg; p.head_major = head_major; p.seg0_scale = seg0_scale; p.S = S; p.H = H;
    p.pos = b.in<float>(pos, (size_t)S * N * 4);
    KREF_CHECK(b);
    if (kernel128) launch_gemm_128(p, st.s);
    else launch_gemm(p, st.s);
    if (hipError_t e = st.finish()) return (int)e;
    b.out(out0, p.out[0], out_bytes);
    b.out(out1, p.out[1], out_bytes);
    b.out(out2, p.out[2], out_bytes);
    return (int)b.err;
}

// launch_layernorm (sliced = 0) or launch_layernorm_sliced: x f32 [M][K] -> y fp16 [M][K], y32 f32 [M][K] or null
int kref_layernorm(int sliced, const float *x, const float *w, const float *bb, void *y, float *y32, int M, int K) {
    Bufs b;
    Stream st;
    const float *dx = b.in<float>(x, (size_t)M * K * 4), *dw = b.in<float>(w, (size_t)K * 4), *db = b.in<float>(bb, (size_t)K * 4);
    half_t *dy = b.in<half_t>(y, (size_t)M * K * 2);
    float *dy32 = b.in<float>(y32, (size_t)M * K * 4);
    KREF_CHECK(b);
    if (sliced) {
        if (!launch_layernorm_sliced(dx, dw, db, dy, dy32, M, K, st.s)) return -1;
    } else {
        launch_layernorm(dx, dw, db, dy, dy32, M, K, st.s);
    }
    if (hipError_t e = st.finish()) return (int)e;
    b.out(y, dy, (size_t)M * K * 2);
    b.out(y32, dy32, (size_t)M * K * 4);
    return (int)b.err;
}

// launch_embed: tokens i32 [B][tok_stride], E fp16 [V][d], P fp16 [n_pos][d] -> x f32 [B*Tn][d]
int kref_embed(const int32_t *tokens, int tok_stride, const void *E, int V, const void *P, int n_pos, float *x, int B, int Tn,
               int t0, const int32_t *pos_ptr, int d) {
    Bufs b;
    Stream st;
    const int32_t *dt = b.in<int32_t>(tokens, (size_t)B * tok_stride * 4);
    const half_t *dE = b.in<half_t>(E, (size_t)V * d * 2), *dP = b.in<half_t>(P, (size_t)n_pos * d * 2);
    float *dx = b.in<float>(x, (size_t)B * Tn * d * 4);
    const int32_t *dpos = b.in<int32_t>(pos_ptr, (size_t)B * 4);
    KREF_CHECK(b);
    launch_embed(dt, tok_stride, dE, dP, dx, B, Tn, t0, dpos, d, st.s);
    if (hipError_t e = st.finish()) return (int)e;
    b.out(x, dx, (size_t)B * Tn * d * 4);
    return (int)b.err;
}

}  // extern "C"
