// kref_pool.hip -- test-only C entry points onto what a decode pool's token step launches after the logits (emit_token_step,
// nh_decode.hip) and onto launch_embed_ragged (tests/pool_ref.py, tests/test_gpu_pool_kernel.py).  Linked against the library's
// own objects: the kernels under test are the product's.  Host buffers in, device copies made of every one of them -- outputs
// too, so a test sees what a kernel must leave alone --, the launches on one stream of its own, everything copied back.
// Returns the hipError_t, or -1 -- nothing launched, nothing written -- for what would write out of bounds or what the host
// refuses.
#include <cstring>
#include <vector>

#include "../norma_amd/csrc/nh_kernels.h"

namespace {
struct Dev {
    std::vector<void *> bufs;
    hipError_t err = hipSuccess;
    template <class T> T *in(const void *host, size_t bytes) {
        if (err != hipSuccess) return nullptr;
        void *d = nullptr;
        if ((err = hipMalloc(&d, bytes ? bytes : 16)) != hipSuccess) return nullptr;
        bufs.push_back(d);
        err = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
        return static_cast<T *>(d);
    }
    void out(void *host, const void *d, size_t bytes) {
        if (err == hipSuccess) err = hipMemcpy(host, d, bytes, hipMemcpyDeviceToHost);
    }
    ~Dev() {
        for (void *d : bufs) (void)hipFree(d);
    }
};

// one row of the event table: what happens to `row` ahead of step k
enum { EV_ADMIT = 0, EV_RETRY = 1, EV_INTS = 9 };
// admit: {k, 0, row, t0, t1, t2, detect, n_prefix, pos0}      retry: {k, 1, row, inv_t (f32 bits), seed lo, seed hi, clip, attempt, 0}
}  // namespace

extern "C" {

// K pool steps on one state.  Ahead of step k the events {k, ...} of `events` (i32 [n_events][9], k ascending, k = K: after the
// last step) run in table order: launch_pool_admit / launch_pool_retry.  Step k then launches, on logits [k][B][ldl] (ldl = V
// rounded up to 64), launch_pool_lang_detect (lang_tokens != null), launch_guard(pos, pfx) (use_guard), launch_pool_sample_step
// (sampled[k]) and launch_logit_step(mode 2, handled if sampled[k], pfx if use_pfx).  tk: the 8 ints of RuleTokens.  Every other
// array is copied in and back: logits, the DecodeState arrays ([B][ctx] tokens), pos, pfx, tickets [B], partials [B][64],
// inv_t / seed / clip / attempt / handled [B], detect_flag, lang_out [B], probs [B][256], loop_exit [B].
int kref_pool_steps(float *logits, int K, int V, int B, int ctx, int cap, int max_new, int P, const int32_t *tk, const uint8_t *suppress,
                    int32_t *tokens, int32_t *n_tokens, int32_t *done, int32_t *have_last, int32_t *last_ts, double *sum_logprob,
                    double *no_speech, int32_t *pos, int32_t *pfx, int use_pfx, unsigned *tickets, float *partials, float *inv_t,
                    unsigned long long *seed, unsigned *clip, unsigned *attempt, int32_t *handled, const int32_t *sampled,
                    const int32_t *events, int n_events, const int32_t *lang_tokens, int n_lang, int32_t *detect_flag, int32_t *lang_out,
                    float *probs, int use_guard, int g_ngram, float g_penalty, int g_period, int g_repeats, int32_t *loop_exit) {
    // ---- refusals: everything a kernel would index with is checked here, on the host ----
    if (!logits || !tk || !suppress || !tokens || !n_tokens || !done || !have_last || !last_ts || !sum_logprob || !no_speech || !pos ||
        !pfx || !tickets || !partials || !inv_t || !seed || !clip || !attempt || !handled || !sampled || !detect_flag || !lang_out ||
        !probs || !loop_exit || (n_events > 0 && !events))
        return -1;
    if (K < 1 || B < 1 || V < 1 || V > NH_MAX_VOCAB || (P != 2 && P != 3) || ctx < 4 || cap > ctx - 1 || cap < 2) return -1;
    for (int i = 0; i < 8; i++) if (tk[i] < 0 || tk[i] >= V) return -1;
    if (lang_tokens) {
        if (n_lang < 1 || n_lang > 256) return -1;   // a table size outside 1 .. 256
        for (int i = 0; i < n_lang; i++) if (lang_tokens[i] < 0 || lang_tokens[i] >= V) return -1;
    }
    if (use_guard && (ctx > NH_GUARD_MAX_HISTORY || g_ngram < 0 || g_period < 0 || g_period > NH_GUARD_MAX_PERIOD ||
                      (g_period > 0 && g_repeats < 2) || !(g_penalty > 0.f)))
        return -1;
    for (long i = 0; i < (long)B * ctx; i++) if (tokens[i] < 0 || tokens[i] >= V) return -1;   // the guard indexes logits by them
    std::vector<int> hp(B);   // every row's prefix length as the events move it
    for (int r = 0; r < B; r++) {
        hp[r] = use_pfx ? pfx[r] : 0;
        if (hp[r] < 0 || hp[r] + P >= cap) return -1;
        if (!done[r] && (n_tokens[r] < 1 || n_tokens[r] >= cap)) return -1;   // a live row whose next two writes do not fit
    }
    for (int e = 0; e < n_events; e++) {
        const int32_t *v = events + EV_INTS * e;
        if (v[0] < 0 || v[0] > K || (e && v[0] < v[-EV_INTS]) || v[2] < 0 || v[2] >= B) return -1;   // a row outside [0, B)
        if (v[1] == EV_ADMIT) {
            const int det = v[6], npfx = v[7], pos0 = v[8];
            if (npfx < 0 || (npfx > 0 && !use_pfx) || npfx + P >= cap) return -1;
            if (pos0 != 0 && pos0 != npfx) return -1;
            if (det && npfx > 0) return -1;   // nh_pool_admit refuses detection under a prefix
            if (det != 0 && det != 1) return -1;
            for (int i = 3; i < 6; i++) if (v[i] < 0 || v[i] >= V) return -1;
            hp[v[2]] = npfx;
        } else if (v[1] == EV_RETRY) {
            if (hp[v[2]] + P >= cap) return -1;
        } else {
            return -1;
        }
    }
    // ---- device copies ----
    Dev dv;
    const long ldl = nh_logits_ld(V);
    const size_t lbytes = (size_t)K * B * ldl * 4, tbytes = (size_t)B * ctx * 4, b4 = (size_t)B * 4, b8 = (size_t)B * 8;
    float *dl = dv.in<float>(logits, lbytes);
    DecodeState s{};
    s.tokens = dv.in<int32_t>(tokens, tbytes);
    s.n_tokens = dv.in<int32_t>(n_tokens, b4);
    s.done = dv.in<int32_t>(done, b4);
    s.have_last = dv.in<int32_t>(have_last, b4);
    s.last_ts = dv.in<int32_t>(last_ts, b4);
    s.sum_logprob = dv.in<double>(sum_logprob, b8);
    s.no_speech = dv.in<double>(no_speech, b8);
    const int32_t zero = 0;
    s.n_active = dv.in<int32_t>(&zero, 4);
    s.suppress = dv.in<uint8_t>(suppress, (size_t)V);
    int32_t *dpos = dv.in<int32_t>(pos, b4), *dpfx = dv.in<int32_t>(pfx, b4);
    unsigned *dtick = dv.in<unsigned>(tickets, b4);
    float *dpart = dv.in<float>(partials, (size_t)B * 64 * 4);
    PoolSampling ps{dv.in<float>(inv_t, b4), dv.in<unsigned long long>(seed, b8), dv.in<unsigned>(clip, b4), dv.in<unsigned>(attempt, b4),
                    dv.in<int32_t>(handled, b4)};
    int32_t *dflag = dv.in<int32_t>(detect_flag, b4), *dlout = dv.in<int32_t>(lang_out, b4);
    float *dprobs = dv.in<float>(probs, (size_t)B * 256 * 4);
    const int32_t *dlt = lang_tokens ? dv.in<int32_t>(lang_tokens, (size_t)n_lang * 4) : nullptr;
    int32_t *dexit = dv.in<int32_t>(loop_exit, b4);
    if (dv.err != hipSuccess) return (int)dv.err;
    hipStream_t st = nullptr;
    if (hipError_t e = hipStreamCreate(&st)) return (int)e;   // a blocking stream: ordered after the copies above
    const RuleTokens rt{tk[0], tk[1], tk[2], tk[3], tk[4], tk[5], tk[6], tk[7]};
    const PoolDetect det{dflag, dlt, n_lang, dlout, dprobs};
    const GuardSpec gs{g_ngram, g_penalty, g_period, g_repeats, 0};
    const GuardBufs gb{nullptr, nullptr, nullptr, nullptr, 1, dexit};
    const int32_t *kpfx = use_pfx ? dpfx : nullptr;
    // ---- the steps, in the order of emit_token_step ----
    for (int k = 0, e = 0; k <= K; k++) {
        for (; e < n_events && events[EV_INTS * e] == k; e++) {
            const int32_t *v = events + EV_INTS * e;
            if (v[1] == EV_ADMIT) {
                launch_pool_admit(s, dpos, dtick, v[2], ctx, v[3], v[4], v[5], P, st, dflag, v[6], use_pfx ? dpfx : nullptr, v[7], v[8]);
            } else {
                float it;
                memcpy(&it, v + 3, 4);
                const unsigned long long sd = (unsigned long long)(uint32_t)v[4] | ((unsigned long long)(uint32_t)v[5] << 32);
                launch_pool_retry(s, dpos, dtick, ps, v[2], P, it, sd, (unsigned)v[6], (unsigned)v[7], st, dflag, kpfx);
            }
        }
        if (k == K) break;
        float *lg = dl + (long)k * B * ldl;
        if (dlt) launch_pool_lang_detect(lg, V, s, B, ctx, dpos, det, st);
        if (use_guard) launch_guard(lg, V, s, rt, B, ctx, P, dpos, gs, gb, st, kpfx);
        if (sampled[k]) launch_pool_sample_step(lg, V, s, rt, B, ctx, cap, max_new, P, ps, dpos, st, kpfx);
        launch_logit_step(lg, V, s, rt, B, ctx, cap, max_new, P, 2, dpart, dtick, dpos, st, sampled[k] ? ps.handled : nullptr, kpfx);
    }
    hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    if (e1 != hipSuccess) return (int)e1;
    if (e2 != hipSuccess) return (int)e2;
    dv.out(logits, dl, lbytes);
    dv.out(tokens, s.tokens, tbytes);
    dv.out(n_tokens, s.n_tokens, b4);
    dv.out(done, s.done, b4);
    dv.out(have_last, s.have_last, b4);
    dv.out(last_ts, s.last_ts, b4);
    dv.out(sum_logprob, s.sum_logprob, b8);
    dv.out(no_speech, s.no_speech, b8);
    dv.out(pos, dpos, b4);
    dv.out(pfx, dpfx, b4);
    dv.out(tickets, dtick, b4);
    dv.out(partials, dpart, (size_t)B * 64 * 4);
    dv.out(inv_t, ps.inv_t, b4);
    dv.out(seed, ps.seed, b8);
    dv.out(clip, ps.clip, b4);
    dv.out(attempt, ps.attempt, b4);
    dv.out(handled, ps.handled, b4);
    dv.out(detect_flag, dflag, b4);
    dv.out(lang_out, dlout, b4);
    dv.out(probs, dprobs, (size_t)B * 256 * 4);
    dv.out(loop_exit, dexit, b4);
    return (int)dv.err;
}

// launch_embed_ragged: tokens i32 [tok_rows][tok_stride], E fp16 [V][d], P fp16 [n_pos][d], clips i32 [n][4] = {token row, T,
// packed offset, 0} (PfClip) -> x f32 [m_rows][d], copied in and back (m_rows >= the rows the table covers: the rest are a
// test's canaries).  -1: a table that would read or write outside those buffers, or whose clips share a row or overlap in x.
int kref_embed_ragged(const int32_t *tokens, int tok_stride, int tok_rows, const void *E, int V, const void *P, int n_pos, float *x,
                      int m_rows, const int32_t *clips, int n, int d) {
    if (!tokens || !E || !P || !x || !clips || n < 1 || tok_stride < 1 || tok_rows < 1 || V < 1 || n_pos < 1 || m_rows < 1 || d < 4 || d % 4)
        return -1;
    int Tmax = 0;
    for (int i = 0; i < n; i++) {
        const int32_t *c = clips + 4 * i;
        if (c[0] < 0 || c[0] >= tok_rows || c[1] < 1 || c[1] > tok_stride || c[1] > n_pos || c[2] < 0 || (long)c[2] + c[1] > m_rows) return -1;
        for (int j = 0; j < i; j++) {
            const int32_t *e = clips + 4 * j;
            if (e[0] == c[0] || (c[2] < e[2] + e[1] && e[2] < c[2] + c[1])) return -1;
        }
        for (int t = 0; t < c[1]; t++) {
            const int32_t tok = tokens[(long)c[0] * tok_stride + t];
            if (tok < 0 || tok >= V) return -1;
        }
        Tmax = c[1] > Tmax ? c[1] : Tmax;
    }
    Dev dv;
    const int32_t *dt = dv.in<int32_t>(tokens, (size_t)tok_rows * tok_stride * 4);
    const half_t *dE = dv.in<half_t>(E, (size_t)V * d * 2), *dP = dv.in<half_t>(P, (size_t)n_pos * d * 2);
    float *dx = dv.in<float>(x, (size_t)m_rows * d * 4);
    const PfClip *dc = dv.in<PfClip>(clips, sizeof(PfClip) * n);
    if (dv.err != hipSuccess) return (int)dv.err;
    hipStream_t st = nullptr;
    if (hipError_t e = hipStreamCreate(&st)) return (int)e;
    launch_embed_ragged(dt, tok_stride, dE, dP, dx, dc, n, Tmax, d, st);
    hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    if (e1 != hipSuccess) return (int)e1;
    if (e2 != hipSuccess) return (int)e2;
    dv.out(x, dx, (size_t)m_rows * d * 4);
    return (int)dv.err;
}

}  // extern "C"
