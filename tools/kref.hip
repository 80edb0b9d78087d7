// kref.hip -- test-only C entry points onto the shipped launchers of nh_kernels.h (tests/kref.py, tests/test_gpu_kernel_ref.py, tests/test_gpu_mel_ref.py).
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
    const bool launched = launch_skinny(p, st.s);
    if (hipError_t e = st.finish()) return (int)e;
    // copied back after a refusal too: a test can see that a refused launch left the outputs alone
    b.out(out0, p.out[0], out0_bytes);
    b.out(out1, p.out[1], out12_bytes);
    b.out(out2, p.out[2], out12_bytes);
    return launched ? (int)b.err : -1;
}

int kref_skinny_ln_supported(int R, int N, int K) { return skinny_ln_supported(R, N, K) ? 1 : 0; }

// skinny_plan (pure host: no GPU needed): out = {kind, ncb, nt, ksplit, sp, grid.x, grid.y, block, lds_used, lds_exclusive};
// returns 1 when the shape is planned, 0 when it is refused (kind SKP_NONE)
int kref_skinny_plan(int R, int N, int K, int epi, int wt, int ln, int32_t out[10]) {
    const SkinnyPlan pl = skinny_plan(R, N, K, epi, wt != 0, ln != 0);
    const int32_t v[10] = {pl.kind, pl.ncb, pl.nt, pl.ksplit, pl.sp, pl.grid_x, pl.grid_y, pl.block, (int32_t)pl.lds_used, pl.lds_exclusive};
    for (int i = 0; i < 10; i++) out[i] = v[i];
    return pl.kind != SKP_NONE;
}

// launch_dec_attention: q [B][d]; kc, vc head-major [B][H][ctx][64]; out [B][d] (copied in: done rows stay).  head_major must
// be 1: 0 was the row-major [B][ctx][d] layout, which dec_attn_kernel no longer reads (-1, shape refused)
int kref_dec_attention(const void *q, const void *kc, const void *vc, void *out, int B, int H, int d, int ctx, int Tk,
                       const int32_t *pos_ptr, int head_major, const int32_t *done) {
    if (!head_major) return -1;
    Bufs b;
    Stream st;
    const size_t kv = (size_t)B * ctx * d * 2;
    const half_t *dq = b.in<half_t>(q, (size_t)B * d * 2), *dk = b.in<half_t>(kc, kv), *dv = b.in<half_t>(vc, kv);
    half_t *dout = b.in<half_t>(out, (size_t)B * d * 2);
    const int32_t *dpos = b.in<int32_t>(pos_ptr, (size_t)B * 4), *ddone = b.in<int32_t>(done, (size_t)B * 4);
    KREF_CHECK(b);
    launch_dec_attention(dq, dk, dv, dout, B, H, d, ctx, Tk, dpos, st.s, ddone);
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

// launch_prefill_self_attention: q, k, v rows (b, i) at base + (b * T + i) * ld, 64 H halfs each (three buffers, or column
// slices of one q|k|v buffer with ld = 3 * 64 H: each is copied from its own base up to the end of its last row); out
// [B*T][ldo], ck / cv the self cache [B][H][C][64].  out, ck and cv are copied in and back, after a refusal too.
int kref_prefill_self_attention(const void *q, const void *k, const void *v, long ld, void *out, long ldo, void *ck, void *cv, int B,
                                int T, int H, int C) {
    Bufs b;
    Stream st;
    const long rows = (long)(B > 0 ? B : 0) * (T > 0 ? T : 0);
    const size_t in_bytes = rows ? (size_t)((rows - 1) * ld + (long)H * NH_DH) * 2 : 0, out_bytes = (size_t)rows * ldo * 2;
    const size_t cache_bytes = (size_t)B * H * C * NH_DH * 2;
    const half_t *dq = b.in<half_t>(q, in_bytes), *dk = b.in<half_t>(k, in_bytes), *dv = b.in<half_t>(v, in_bytes);
    half_t *dout = b.in<half_t>(out, out_bytes), *dck = b.in<half_t>(ck, cache_bytes), *dcv = b.in<half_t>(cv, cache_bytes);
    KREF_CHECK(b);
    const bool launched = launch_prefill_self_attention(dq, dk, dv, ld, dout, ldo, dck, dcv, B, T, H, C, st.s);
    if (hipError_t e = st.finish()) return (int)e;
    b.out(out, dout, out_bytes);
    b.out(ck, dck, cache_bytes);
    b.out(cv, dcv, cache_bytes);
    return launched ? (int)b.err : -1;
}

// launch_prefill_cross_attention: q rows (b, i) at q + (b * T + i) * ldq; ck, cv head-major cross K/V [B][H][S][64], exactly S
// keys per (clip, head); out [B*T][ldo].  out, ck and cv are copied in and back, after a refusal too.
int kref_prefill_cross_attention(const void *q, long ldq, void *ck, void *cv, void *out, long ldo, int B, int T, int H, int S) {
    Bufs b;
    Stream st;
    const long rows = (long)(B > 0 ? B : 0) * (T > 0 ? T : 0);
    const size_t q_bytes = rows ? (size_t)((rows - 1) * ldq + (long)H * NH_DH) * 2 : 0, out_bytes = (size_t)rows * ldo * 2;
    const size_t kv_bytes = (size_t)B * H * (S > 0 ? S : 0) * NH_DH * 2;
    const half_t *dq = b.in<half_t>(q, q_bytes);
    half_t *dck = b.in<half_t>(ck, kv_bytes), *dcv = b.in<half_t>(cv, kv_bytes), *dout = b.in<half_t>(out, out_bytes);
    KREF_CHECK(b);
    const bool launched = launch_prefill_cross_attention(dq, ldq, dck, dcv, dout, ldo, B, T, H, S, st.s);
    if (hipError_t e = st.finish()) return (int)e;
    b.out(out, dout, out_bytes);
    b.out(ck, dck, kv_bytes);
    b.out(cv, dcv, kv_bytes);
    return launched ? (int)b.err : -1;
}

// The ragged forms of the two launches above.  clips i32 [n][4] = {context row, T, packed offset, 0} per clip; q (k, v) hold
// m_rows packed rows of ld halfs and out m_rows rows of ldo (m_rows >= the rows the table covers: the rest are a test's
// canaries); the caches have cache_rows context rows.  -1, nothing launched: a table that would read or write outside those
// buffers, or whose clips' rows overlap.
static bool kref_clip_table(const int32_t *clips, int n, int m_rows, int cache_rows, int limit, int &Tmax) {
    Tmax = 0;
    if (!clips || n < 1) return false;
    for (int i = 0; i < n; i++) {
        const int32_t *c = clips + 4 * i;
        if (c[0] < 0 || c[0] >= cache_rows || c[1] < 1 || c[1] > limit || c[2] < 0 || (long)c[2] + c[1] > m_rows) return false;
        for (int j = 0; j < i; j++) {
            const int32_t *e = clips + 4 * j;
            if (e[0] == c[0] || (c[2] < e[2] + e[1] && e[2] < c[2] + c[1])) return false;
        }
        Tmax = c[1] > Tmax ? c[1] : Tmax;
    }
    return true;
}

int kref_prefill_self_attention_ragged(const void *q, const void *k, const void *v, long ld, void *out, long ldo, void *ck, void *cv,
                                       const int32_t *clips, int n, int m_rows, int cache_rows, int H, int C) {
    int Tmax = 0;
    if (H < 1 || C < 1 || m_rows < 1 || ld < (long)H * NH_DH || ldo < (long)H * NH_DH || !kref_clip_table(clips, n, m_rows, cache_rows, C, Tmax)) return -1;
    Bufs b;
    Stream st;
    const size_t in_bytes = (size_t)((m_rows - 1) * ld + (long)H * NH_DH) * 2, out_bytes = (size_t)m_rows * ldo * 2;
    const size_t cache_bytes = (size_t)cache_rows * H * C * NH_DH * 2;
    const half_t *dq = b.in<half_t>(q, in_bytes), *dk = b.in<half_t>(k, in_bytes), *dv = b.in<half_t>(v, in_bytes);
    half_t *dout = b.in<half_t>(out, out_bytes), *dck = b.in<half_t>(ck, cache_bytes), *dcv = b.in<half_t>(cv, cache_bytes);
    const PfClip *dtab = b.in<PfClip>(clips, sizeof(PfClip) * n);
    KREF_CHECK(b);
    const bool launched = launch_prefill_self_attention(dq, dk, dv, ld, dout, ldo, dck, dcv, n, Tmax, H, C, st.s, dtab);
    if (hipError_t e = st.finish()) return (int)e;
    b.out(out, dout, out_bytes);
    b.out(ck, dck, cache_bytes);
    b.out(cv, dcv, cache_bytes);
    return launched ? (int)b.err : -1;
}

int kref_prefill_cross_attention_ragged(const void *q, long ldq, void *ck, void *cv, void *out, long ldo, const int32_t *clips, int n,
                                        int m_rows, int cache_rows, int H, int S) {
    int Tmax = 0;
    if (H < 1 || S < 1 || m_rows < 1 || ldq < (long)H * NH_DH || ldo < (long)H * NH_DH || !kref_clip_table(clips, n, m_rows, cache_rows, 1 << 20, Tmax)) return -1;
    Bufs b;
    Stream st;
    const size_t q_bytes = (size_t)((m_rows - 1) * ldq + (long)H * NH_DH) * 2, out_bytes = (size_t)m_rows * ldo * 2;
    const size_t kv_bytes = (size_t)cache_rows * H * S * NH_DH * 2;
    const half_t *dq = b.in<half_t>(q, q_bytes);
    half_t *dck = b.in<half_t>(ck, kv_bytes), *dcv = b.in<half_t>(cv, kv_bytes), *dout = b.in<half_t>(out, out_bytes);
    const PfClip *dtab = b.in<PfClip>(clips, sizeof(PfClip) * n);
    KREF_CHECK(b);
    const bool launched = launch_prefill_cross_attention(dq, ldq, dck, dcv, dout, ldo, n, Tmax, H, S, st.s, dtab);
    if (hipError_t e = st.finish()) return (int)e;
    b.out(out, dout, out_bytes);
    b.out(ck, dck, kv_bytes);
    b.out(cv, dcv, kv_bytes);
    return launched ? (int)b.err : -1;
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

// ---- token selection ------------------------------------------------------------------------------------------------------
namespace {
// device copies of a DecodeState's arrays (host arrays in and out, B rows of ctx tokens); tk: the 8 ints of RuleTokens
struct KrefState {
    DecodeState s{};
    int32_t *tokens, *n_tokens, *done, *have_last, *last_ts;
    double *sum_logprob, *no_speech;
    int B, ctx;
    KrefState(Bufs &b, int B_, int ctx_, int V, const uint8_t *suppress, int32_t *tokens_, int32_t *n_tokens_, int32_t *done_,
              int32_t *have_last_, int32_t *last_ts_, double *sum_logprob_, double *no_speech_)
        : tokens(tokens_), n_tokens(n_tokens_), done(done_), have_last(have_last_), last_ts(last_ts_), sum_logprob(sum_logprob_),
          no_speech(no_speech_), B(B_), ctx(ctx_) {
        s.tokens = b.in<int32_t>(tokens, (size_t)B * ctx * 4);
        s.n_tokens = b.in<int32_t>(n_tokens, (size_t)B * 4);
        s.done = b.in<int32_t>(done, (size_t)B * 4);
        s.have_last = b.in<int32_t>(have_last, (size_t)B * 4);
        s.last_ts = b.in<int32_t>(last_ts, (size_t)B * 4);
        s.sum_logprob = b.in<double>(sum_logprob, (size_t)B * 8);
        s.no_speech = b.in<double>(no_speech, (size_t)B * 8);
        s.n_active = b.zeros<int32_t>(4);
        s.suppress = b.in<uint8_t>(suppress, (size_t)V);
    }
    void out(Bufs &b) {
        b.out(tokens, s.tokens, (size_t)B * ctx * 4);
        b.out(n_tokens, s.n_tokens, (size_t)B * 4);
        b.out(done, s.done, (size_t)B * 4);
        b.out(have_last, s.have_last, (size_t)B * 4);
        b.out(last_ts, s.last_ts, (size_t)B * 4);
        b.out(sum_logprob, s.sum_logprob, (size_t)B * 8);
        b.out(no_speech, s.no_speech, (size_t)B * 8);
    }
};
RuleTokens rule_tokens(const int32_t *t) { return RuleTokens{t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]}; }
}  // namespace

extern "C" {

// K consecutive launch_logit_step on one state, launch k on logits [k][B][ldl] (ldl = V rounded up to 64, as the launcher
// computes it) with mode modes[k] and pos_ptr = pos when use_pos[k] (else null).  admit [n_admit][6] = {before launch k, row,
// t0, t1, t2, P}: launch_pool_admit calls, in order, ahead of launch k (k = K: after the last).  Every state array, pos [B]
// (may be null), tickets [B] and partials [B][LSPLIT][8] are copied in and back.
int kref_logit_step(const float *logits, int K, int V, int B, int ctx, int cap, int max_new, int prompt_len, const int32_t *modes,
                    const int32_t *use_pos, const int32_t *tk, const uint8_t *suppress, int32_t *tokens, int32_t *n_tokens,
                    int32_t *done, int32_t *have_last, int32_t *last_ts, double *sum_logprob, double *no_speech, int32_t *pos,
                    const int32_t *admit, int n_admit, unsigned *tickets, float *partials) {
    // refuse what would write out of bounds: a mode-2 launch or an admission without positions, a row outside [0, B), a
    // live row whose next two writes do not fit below the cap
    if (cap > ctx - 1 || V < 1 || V > NH_MAX_VOCAB) return -1;
    for (int k = 0; k < K; k++) if (modes[k] == 2 && !(use_pos[k] && pos)) return -1;
    for (int a = 0; a < n_admit; a++)
        if (!pos || admit[6 * a + 1] < 0 || admit[6 * a + 1] >= B || (admit[6 * a + 5] != 2 && admit[6 * a + 5] != 3) ||
            admit[6 * a + 5] >= cap || (a && admit[6 * a] < admit[6 * a - 6]))
            return -1;
    for (int r = 0; r < B; r++) if (!done[r] && (n_tokens[r] < 1 || n_tokens[r] >= cap)) return -1;
    Bufs b;
    Stream st;
    const long ldl = nh_logits_ld(V);
    const float *dl = b.in<float>(logits, (size_t)K * B * ldl * 4);
    KrefState ks(b, B, ctx, V, suppress, tokens, n_tokens, done, have_last, last_ts, sum_logprob, no_speech);
    int32_t *dpos = b.in<int32_t>(pos, (size_t)B * 4);
    unsigned *dtick = b.in<unsigned>(tickets, (size_t)B * 4);
    float *dpart = b.in<float>(partials, (size_t)B * 64 * 4);
    KREF_CHECK(b);
    const RuleTokens rt = rule_tokens(tk);
    for (int k = 0, a = 0; k <= K; k++) {
        for (; a < n_admit && admit[6 * a] == k; a++) {
            const int32_t *e = admit + 6 * a;
            launch_pool_admit(ks.s, dpos, dtick, e[1], ctx, e[2], e[3], e[4], e[5], st.s);
        }
        if (k == K) break;
        launch_logit_step(dl + (long)k * B * ldl, V, ks.s, rt, B, ctx, cap, max_new, prompt_len, modes[k], dpart, dtick,
                          use_pos[k] ? dpos : nullptr, st.s);
    }
    if (hipError_t e = st.finish()) return (int)e;
    ks.out(b);
    b.out(pos, dpos, (size_t)B * 4);
    b.out(tickets, dtick, (size_t)B * 4);
    b.out(partials, dpart, (size_t)B * 64 * 4);
    return (int)b.err;
}

// K consecutive launch_sample_step on one state (logits [k][B][ldl] as above); clip0, attempt and seed as the launcher takes them
int kref_sample_step(const float *logits, int K, int V, int B, int ctx, int cap, int max_new, int prompt_len, float inv_t,
                     unsigned long long seed, unsigned clip0, unsigned attempt, const int32_t *tk, const uint8_t *suppress,
                     int32_t *tokens, int32_t *n_tokens, int32_t *done, int32_t *have_last, int32_t *last_ts, double *sum_logprob,
                     double *no_speech) {
    if (cap > ctx - 1 || V < 1) return -1;
    for (int r = 0; r < B; r++) if (!done[r] && (n_tokens[r] < 1 || n_tokens[r] >= cap)) return -1;
    Bufs b;
    Stream st;
    const long ldl = nh_logits_ld(V);
    const float *dl = b.in<float>(logits, (size_t)K * B * ldl * 4);
    KrefState ks(b, B, ctx, V, suppress, tokens, n_tokens, done, have_last, last_ts, sum_logprob, no_speech);
    KREF_CHECK(b);
    const RuleTokens rt = rule_tokens(tk);
    for (int k = 0; k < K; k++)
        launch_sample_step(dl + (long)k * B * ldl, V, ks.s, rt, B, ctx, cap, max_new, prompt_len, inv_t, seed, clip0, attempt, st.s);
    if (hipError_t e = st.finish()) return (int)e;
    ks.out(b);
    return (int)b.err;
}

// launch_lang_detect: logits [B][ldl], lang_tokens [n] (1 <= n <= 256, any order) -> probs [B][n], lang_out [B]
int kref_lang_detect(const float *logits, int V, int B, const int32_t *lang_tokens, int n, float *probs, int32_t *lang_out) {
    Bufs b;
    Stream st;
    if (n < 1 || n > 256) return -1;
    const long ldl = nh_logits_ld(V);
    const float *dl = b.in<float>(logits, (size_t)B * ldl * 4);
    const int32_t *dlt = b.in<int32_t>(lang_tokens, (size_t)n * 4);
    float *dp = b.in<float>(probs, (size_t)B * n * 4);
    int32_t *dout = b.in<int32_t>(lang_out, (size_t)B * 4);
    KREF_CHECK(b);
    launch_lang_detect(dl, V, dlt, n, dp, dout, B, st.s);
    if (hipError_t e = st.finish()) return (int)e;
    b.out(probs, dp, (size_t)B * n * 4);
    b.out(lang_out, dout, (size_t)B * 4);
    return (int)b.err;
}

}  // extern "C"

// ---- token-level timestamps (k_align.hip) ---------------------------------------------------------------------------------
extern "C" {

// launch_align_weights: q fp16 [A][max_rows][B][64] (the capture layout), K fp16 [B][H][S][64] (head-major cross K cache),
// heads i32 [A] = the head of K each list entry reads, n_rows / n_keys i32 [B]; W f32 [B][A][max_rows][S], copied in and back
int kref_align_weights(const void *q, const void *K, const int32_t *heads, int A, int H, int S, int B, const int32_t *n_rows,
                       const int32_t *n_keys, int max_rows, float *W) {
    if (A < 1 || A > NH_ALIGN_HEADS || B < 1 || max_rows < 1 || S < 1) return -1;
    for (int a = 0; a < A; a++) if (heads[a] < 0 || heads[a] >= H) return -1;
    for (int b = 0; b < B; b++) if (n_rows[b] < 0 || n_rows[b] > max_rows || n_keys[b] < 0 || n_keys[b] > S) return -1;
    Bufs b;
    Stream st;
    const half_t *dq = b.in<half_t>(q, (size_t)A * max_rows * B * NH_DH * 2), *dk = b.in<half_t>(K, (size_t)B * H * S * NH_DH * 2);
    const int32_t *dr = b.in<int32_t>(n_rows, (size_t)B * 4), *dn = b.in<int32_t>(n_keys, (size_t)B * 4);
    const size_t wbytes = (size_t)B * A * max_rows * S * 4;
    float *dW = b.in<float>(W, wbytes);
    KREF_CHECK(b);
    AlignHeadPtrs hp{};
    for (int a = 0; a < A; a++) { hp.q[a] = dq + (size_t)a * max_rows * B * NH_DH; hp.k[a] = dk + (size_t)heads[a] * S * NH_DH; }
    const bool launched = launch_align_weights(hp, A, (long)B * NH_DH, NH_DH, (long)H * S * NH_DH, dr, dn, max_rows, S, B, 0, dW,
                                               (long)A * max_rows * S, (long)max_rows * S, S, nullptr, st.s);
    if (hipError_t e = st.finish()) return (int)e;
    b.out(W, dW, wbytes);
    return launched ? (int)b.err : -1;
}

// launch_align_reduce: W f32 [B][A][max_rows][S] -> M f32 [B][max_rows][S] (rows r < n_rows + 1 - P; copied in and back)
int kref_align_reduce(const float *W, int A, int B, int S, int max_rows, const int32_t *n_rows, const int32_t *n_keys, int P, float *M) {
    if (B < 1 || max_rows < 1 || S < 1 || A < 1) return -1;
    for (int b = 0; b < B; b++) if (n_rows[b] < 0 || n_rows[b] > max_rows || n_keys[b] < 0 || n_keys[b] > S) return -1;
    Bufs b;
    Stream st;
    const float *dW = b.in<float>(W, (size_t)B * A * max_rows * S * 4);
    const int32_t *dr = b.in<int32_t>(n_rows, (size_t)B * 4), *dn = b.in<int32_t>(n_keys, (size_t)B * 4);
    const size_t mbytes = (size_t)B * max_rows * S * 4;
    float *dM = b.in<float>(M, mbytes);
    float *stats = b.zeros<float>((size_t)B * A * 2 * S * 4);
    KREF_CHECK(b);
    const bool launched = launch_align_reduce(dW, (long)A * max_rows * S, (long)max_rows * S, S, dr, dn, max_rows, S, B, 0, A, P, stats, dM,
                                              (long)max_rows * S, S, nullptr, st.s);
    if (hipError_t e = st.finish()) return (int)e;
    b.out(M, dM, mbytes);
    return launched ? (int)b.err : -1;
}

// launch_align_dtw: M f32 [B][max_rows][S] -> first, last i32 [B][ldo] (copied in and back), ldo >= max_rows + 1
int kref_align_dtw(const float *M, int B, int S, int max_rows, const int32_t *n_rows, const int32_t *n_keys, int P, int32_t *first,
                   int32_t *last, int ldo) {
    if (B < 1 || max_rows < 1 || S < 1) return -1;
    for (int b = 0; b < B; b++) if (n_rows[b] < 0 || n_rows[b] > max_rows || n_keys[b] < 0 || n_keys[b] > S) return -1;
    Bufs b;
    Stream st;
    const float *dM = b.in<float>(M, (size_t)B * max_rows * S * 4);
    const int32_t *dr = b.in<int32_t>(n_rows, (size_t)B * 4), *dn = b.in<int32_t>(n_keys, (size_t)B * 4);
    int32_t *df = b.in<int32_t>(first, (size_t)B * ldo * 4), *dl = b.in<int32_t>(last, (size_t)B * ldo * 4);
    uint8_t *trace = b.zeros<uint8_t>((size_t)B * max_rows * S);
    KREF_CHECK(b);
    const bool launched = launch_align_dtw(dM, (long)max_rows * S, S, dr, dn, P, max_rows, S, B, 0, trace, (long)max_rows * S, df, dl, ldo, nullptr, st.s);
    if (hipError_t e = st.finish()) return (int)e;
    b.out(first, df, (size_t)B * ldo * 4);
    b.out(last, dl, (size_t)B * ldo * 4);
    return launched ? (int)b.err : -1;
}

}  // extern "C"

// ---- alignment from the decode (k_align.hip: the capture kernel, the row map of the three stage launchers) -------------------
extern "C" {

// launch_align_qsave for the heads `heads` (i32 [n], slots 0 .. n - 1) of one layer: dq fp16 [B][d], qlive fp16
// [n][npos][ldb][64] copied in and back, pos_ptr i32 [B] or null (then `pos`), done i32 [B] or null
int kref_align_qsave_rows(const void *dq, void *qlive, const int32_t *heads, int n, int B, int ldb, int d, int pos, const int32_t *pos_ptr,
                          const int32_t *done, int npos) {
    if (n < 1 || n > NH_ALIGN_HEADS || B < 1 || B > ldb || npos < 1 || d < NH_DH) return -1;
    AlignLayerHeads lh{};
    for (int i = 0; i < n; i++) {
        if (heads[i] < 0 || (heads[i] + 1) * NH_DH > d) return -1;
        lh.slot[i] = i; lh.head[i] = heads[i];
    }
    lh.n = n;
    Bufs b;
    Stream st;
    const size_t qbytes = (size_t)n * npos * ldb * NH_DH * 2;
    const half_t *ddq = b.in<half_t>(dq, (size_t)B * d * 2);
    half_t *dql = b.in<half_t>(qlive, qbytes);
    const int32_t *dp = b.in<int32_t>(pos_ptr, (size_t)B * 4), *dd = b.in<int32_t>(done, (size_t)B * 4);
    KREF_CHECK(b);
    launch_align_qsave(ddq, dql, lh, B, ldb, d, pos, dp, dd, npos, st.s);
    if (hipError_t e = st.finish()) return (int)e;
    b.out(qlive, dql, qbytes);
    return (int)b.err;
}

// The three stage launchers over n clips that read context rows row_map[0 .. n) (i32, every entry in [0, B); null: the
// identity, n <= B).  Layouts as for kref_align_weights / _reduce / _dtw, the outputs [n]-major.
int kref_align_weights_rows(const void *q, const void *K, const int32_t *heads, int A, int H, int S, int B, const int32_t *row_map, int n,
                            const int32_t *n_rows, const int32_t *n_keys, int max_rows, float *W) {
    if (A < 1 || A > NH_ALIGN_HEADS || B < 1 || n < 1 || max_rows < 1 || S < 1 || (!row_map && n > B)) return -1;
    for (int a = 0; a < A; a++) if (heads[a] < 0 || heads[a] >= H) return -1;
    for (int g = 0; g < n; g++)
        if (n_rows[g] < 0 || n_rows[g] > max_rows || n_keys[g] < 0 || n_keys[g] > S || (row_map && (row_map[g] < 0 || row_map[g] >= B))) return -1;
    Bufs b;
    Stream st;
    const half_t *dq = b.in<half_t>(q, (size_t)A * max_rows * B * NH_DH * 2), *dk = b.in<half_t>(K, (size_t)B * H * S * NH_DH * 2);
    const int32_t *dr = b.in<int32_t>(n_rows, (size_t)n * 4), *dn = b.in<int32_t>(n_keys, (size_t)n * 4), *dm = b.in<int32_t>(row_map, (size_t)n * 4);
    const size_t wbytes = (size_t)n * A * max_rows * S * 4;
    float *dW = b.in<float>(W, wbytes);
    KREF_CHECK(b);
    AlignHeadPtrs hp{};
    for (int a = 0; a < A; a++) { hp.q[a] = dq + (size_t)a * max_rows * B * NH_DH; hp.k[a] = dk + (size_t)heads[a] * S * NH_DH; }
    const bool launched = launch_align_weights(hp, A, (long)B * NH_DH, NH_DH, (long)H * S * NH_DH, dr, dn, max_rows, S, n, 0, dW,
                                               (long)A * max_rows * S, (long)max_rows * S, S, dm, st.s);
    if (hipError_t e = st.finish()) return (int)e;
    b.out(W, dW, wbytes);
    return launched ? (int)b.err : -1;
}

int kref_align_reduce_rows(const float *W, int A, int n, int S, int max_rows, const int32_t *row_map, const int32_t *n_rows, const int32_t *n_keys,
                           int P, float *M) {
    if (n < 1 || max_rows < 1 || S < 1 || A < 1) return -1;
    for (int g = 0; g < n; g++) if (n_rows[g] < 0 || n_rows[g] > max_rows || n_keys[g] < 0 || n_keys[g] > S) return -1;
    Bufs b;
    Stream st;
    const float *dW = b.in<float>(W, (size_t)n * A * max_rows * S * 4);
    const int32_t *dr = b.in<int32_t>(n_rows, (size_t)n * 4), *dn = b.in<int32_t>(n_keys, (size_t)n * 4), *dm = b.in<int32_t>(row_map, (size_t)n * 4);
    const size_t mbytes = (size_t)n * max_rows * S * 4;
    float *dM = b.in<float>(M, mbytes);
    float *stats = b.zeros<float>((size_t)n * A * 2 * S * 4);
    KREF_CHECK(b);
    const bool launched = launch_align_reduce(dW, (long)A * max_rows * S, (long)max_rows * S, S, dr, dn, max_rows, S, n, 0, A, P, stats, dM,
                                              (long)max_rows * S, S, dm, st.s);
    if (hipError_t e = st.finish()) return (int)e;
    b.out(M, dM, mbytes);
    return launched ? (int)b.err : -1;
}

int kref_align_dtw_rows(const float *M, int n, int S, int max_rows, const int32_t *row_map, const int32_t *n_rows, const int32_t *n_keys, int P,
                        int32_t *first, int32_t *last, int ldo) {
    if (n < 1 || max_rows < 1 || S < 1) return -1;
    for (int g = 0; g < n; g++) if (n_rows[g] < 0 || n_rows[g] > max_rows || n_keys[g] < 0 || n_keys[g] > S) return -1;
    Bufs b;
    Stream st;
    const float *dM = b.in<float>(M, (size_t)n * max_rows * S * 4);
    const int32_t *dr = b.in<int32_t>(n_rows, (size_t)n * 4), *dn = b.in<int32_t>(n_keys, (size_t)n * 4), *dm = b.in<int32_t>(row_map, (size_t)n * 4);
    int32_t *df = b.in<int32_t>(first, (size_t)n * ldo * 4), *dl = b.in<int32_t>(last, (size_t)n * ldo * 4);
    uint8_t *trace = b.zeros<uint8_t>((size_t)n * max_rows * S);
    KREF_CHECK(b);
    const bool launched = launch_align_dtw(dM, (long)max_rows * S, S, dr, dn, P, max_rows, S, n, 0, trace, (long)max_rows * S, df, dl, ldo, dm, st.s);
    if (hipError_t e = st.finish()) return (int)e;
    b.out(first, df, (size_t)n * ldo * 4);
    b.out(last, dl, (size_t)n * ldo * 4);
    return launched ? (int)b.err : -1;
}

}  // extern "C"

// ---- log-mel (k_mel.hip) ----------------------------------------------------------------------------------------------------
#include "../norma_amd/csrc/mel_host.h"

extern "C" {

// the product's tables (mel_host.h, what nh_model.hip uploads): hann [400], dft_cos / dft_sin [25][25], tw_cos / tw_sin [375].
// Pure host code: no GPU needed.
int kref_mel_tables(float *hann, float *dft_cos, float *dft_sin, float *tw_cos, float *tw_sin) {
    if (!hann || !dft_cos || !dft_sin || !tw_cos || !tw_sin) return -1;
    mel_host_tables(hann, dft_cos, dft_sin, tw_cos, tw_sin);
    return 0;
}

// the group scan of nh_set_mel_filters: filters [n_mel][201] -> grp i32 [n_mel][2].  Pure host code.
int kref_mel_groups(const float *filters, int n_mel, int32_t *grp) {
    if (!filters || !grp || n_mel < 1) return -1;
    mel_host_groups(filters, n_mel, grp);
    return 0;
}

// launch_logmel_grp: pcm f32 [B][stride], n_samples i32 [B] (each in [0, stride]), the five tables, filters [n_mel][201],
// grp [n_mel][2] -> mel32 f32 [B][n_mel][frames] and chunk_max u32 [B].  Both outputs are windows of larger host buffers,
// copied in and back whole: the launch gets mel32 + mel_off of mel_total floats and chunk_max + cm_off of cm_total words, so a
// test sees what lies before and after the window.  `frames` is free (the product passes 1500 or 3000).
int kref_logmel(const float *pcm, long stride, const int32_t *n_samples, int B, const float *hann, const float *dft_cos,
                const float *dft_sin, const float *tw_cos, const float *tw_sin, const float *filters, const int32_t *grp, int n_mel,
                int frames, float *mel32, long mel_off, long mel_total, unsigned *chunk_max, long cm_off, long cm_total) {
    // refuse what would read or write out of bounds
    if (B < 1 || frames < 1 || n_mel < 1 || stride < 1 || !pcm || !n_samples || !filters || !grp || !mel32 || !chunk_max) return -1;
    if (mel_off < 0 || mel_off + (long)B * n_mel * frames > mel_total || cm_off < 0 || cm_off + B > cm_total) return -1;
    for (int b = 0; b < B; b++) if (n_samples[b] < 0 || n_samples[b] > stride) return -1;
    for (int m = 0; m < n_mel; m++) if (grp[2 * m] < 0 || grp[2 * m] > grp[2 * m + 1] || grp[2 * m + 1] > 50) return -1;
    Bufs b;
    Stream st;
    const float *dp = b.in<float>(pcm, (size_t)B * stride * 4);
    const int32_t *dn = b.in<int32_t>(n_samples, (size_t)B * 4), *dg = b.in<int32_t>(grp, (size_t)n_mel * 2 * 4);
    MelTables t{};
    t.hann = b.in<float>(hann, MEL_N_HANN * 4);
    t.dft_cos = b.in<float>(dft_cos, MEL_N_DFT * 4); t.dft_sin = b.in<float>(dft_sin, MEL_N_DFT * 4);
    t.tw_cos = b.in<float>(tw_cos, MEL_N_TW * 4); t.tw_sin = b.in<float>(tw_sin, MEL_N_TW * 4);
    t.filters = b.in<float>(filters, (size_t)n_mel * 201 * 4);
    float *dm = b.in<float>(mel32, (size_t)mel_total * 4);
    unsigned *dc = b.in<unsigned>(chunk_max, (size_t)cm_total * 4);
    KREF_CHECK(b);
    if (!t.hann || !t.dft_cos || !t.dft_sin || !t.tw_cos || !t.tw_sin) return -1;
    launch_logmel_grp(dp, dn, stride, t, dg, n_mel, frames, dm + mel_off, dc + cm_off, B, st.s);
    if (hipError_t e = st.finish()) return (int)e;
    b.out(mel32, dm, (size_t)mel_total * 4);
    b.out(chunk_max, dc, (size_t)cm_total * 4);
    return (int)b.err;
}

// launch_mel_finish_ex: mel32 f32 [B][n_mel][frames] (normalised in place when `normalise`), chunk_max u32 [B] -> img fp16
// [B][frames + 2][NH_MELP].  All three are windows (offset, total, in elements) of host buffers copied in and back whole.
int kref_mel_finish(float *mel32, long mel_off, long mel_total, unsigned *chunk_max, long cm_off, long cm_total, void *img,
                    long img_off, long img_total, int B, int n_mel, int frames, int normalise) {
    if (B < 1 || frames < 1 || n_mel < 1 || n_mel > NH_MELP || !mel32 || !chunk_max || !img) return -1;
    if (mel_off < 0 || mel_off + (long)B * n_mel * frames > mel_total || cm_off < 0 || cm_off + B > cm_total || img_off < 0 ||
        img_off + (long)B * (frames + 2) * NH_MELP > img_total)
        return -1;
    Bufs b;
    Stream st;
    float *dm = b.in<float>(mel32, (size_t)mel_total * 4);
    unsigned *dc = b.in<unsigned>(chunk_max, (size_t)cm_total * 4);
    half_t *di = b.in<half_t>(img, (size_t)img_total * 2);
    KREF_CHECK(b);
    launch_mel_finish_ex(dm + mel_off, dc + cm_off, di + img_off, B, n_mel, frames, normalise, st.s);
    if (hipError_t e = st.finish()) return (int)e;
    b.out(mel32, dm, (size_t)mel_total * 4);
    b.out(chunk_max, dc, (size_t)cm_total * 4);
    b.out(img, di, (size_t)img_total * 2);
    return (int)b.err;
}

}  // extern "C"
