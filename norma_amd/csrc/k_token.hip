// k_token.hip -- token selection of a decode step (gfx950): the rules of Model::decode (src/models/whisper/model.rs:212-277,
// :293-370) on the device, replacing a 207 KB D2H + a fresh [V] mask H2D + three sync scalar reads per token.
//   logit_step_kernel        t = 0: softmax over V, the suppression rules on PROBABILITIES (:212-277, :331-338), greedy argmax
//                            with Iterator::max_by(total_cmp) semantics (:350-356, last maximum wins); the no-speech probe
//                            (:293-315); in a decode pool also the prompt positions
//   sample_step_kernel, pool_sample_step_kernel    t > 0: the same rules, then one seeded draw (:340-348)
//   pool_admit_kernel, pool_retry_kernel           a pool row starts a clip / decodes its clip again, sampled
//   lang_detect_kernel, pool_lang_detect_kernel    Model::detect_language (:194-210), batched / inside a pool step
//   rules_only_kernel, sample_rules_kernel         parity views: the rules (and one draw) on a given probability vector
#include "k_device.h"

// ---------------------------------------------------------------------------------------------------
// logit processor
// ---------------------------------------------------------------------------------------------------
// f32::total_cmp key (Rust std): flip the magnitude bits of negative numbers
__device__ __forceinline__ int total_key(float f) {
    int b = __float_as_int(f);
    return b ^ (int)(((unsigned)(b >> 31)) >> 1);
}

struct BlockRed {   // slots of block_max (fa) and block_sum (fb) of k_device.h, and of block_argmax
    float fa[16], fb[16]; int ia[16], ib[16];
};

// argmax under total_cmp, last maximum wins
__device__ __forceinline__ void block_argmax(int key, int idx, BlockRed &sm, int &okey, int &oidx) {
    for (int o = 32; o > 0; o >>= 1) {
        int k2 = __shfl_xor(key, o), i2 = __shfl_xor(idx, o);
        if (k2 > key || (k2 == key && i2 > idx)) { key = k2; idx = i2; }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sm.ia[threadIdx.x >> 6] = key; sm.ib[threadIdx.x >> 6] = idx; }
    __syncthreads();
    key = sm.ia[0]; idx = sm.ib[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); i++) {
        int k2 = sm.ia[i], i2 = sm.ib[i];
        if (k2 > key || (k2 == key && i2 > idx)) { key = k2; idx = i2; }
    }
    okey = key; oidx = idx;
}

// masked probability of index i: p + (0 | -inf) exactly as the chain of broadcast_adds produces it
__device__ __forceinline__ float masked_value(float p, int i, int rule, const uint8_t *sup, const RuleTokens &tk,
                                              int last_ts) {
    return rule_masks(rule, i, rule != RULE_FIRST && sup[i], tk, last_ts) ? p + (-INFINITY) : p;
}

// which of the four mask chains of model.rs:331-338 / :245-277 applies.  probs(i) gives the soft-maxed probability.
template <typename ProbFn>
__device__ __forceinline__ int rules_decide(ProbFn probs, int V, const int32_t *tokens, int n, int have_last,
                                            const uint8_t *sup, const RuleTokens &tk, BlockRed &sm) {
    const int rule = rule_from_state(have_last, n, tokens[n >= 1 ? n - 1 : 0], tokens[n >= 2 ? n - 2 : 0], tk);
    if (rule != RULE_BY_MASS) return rule;
    float ps = 0.f, pm = -INFINITY;  // model.rs:263-270 on the suppress-masked probabilities
    for (int i = threadIdx.x; i < V; i += blockDim.x) {
        float p = probs(i);
        float pv = sup[i] ? p + (-INFINITY) : p;
        if (i > tk.no_timestamps) ps += pv;
        else if (i < tk.no_timestamps) pm = fmaxf(pm, pv);
    }
    float sum_ts = block_sum(ps, sm.fb);
    float max_text = block_max(pm, sm.fa);
    return (sum_ts >= max_text) ? RULE_NON_TS : RULE_PAST;
}

// thread 0: the books of model.rs:359-370 for `next`, chosen at token count n; the log-prob of :364-365 stays with the caller.
// logit_step_kernel's tail.  The two sampled kernels keep theirs written out, with the all-masked exit of :343-346 in it.
__device__ __forceinline__ void append_token(const DecodeState &s, int b, int32_t *toks, int n, int next, const RuleTokens &tk,
                                             int cap, int max_new, int prompt_len) {
    int nn = n, fin = 0;
    if (next > tk.no_timestamps) { s.last_ts[b] = next; s.have_last[b] = 1; }  // :359-361
    toks[nn++] = next;
    if (nn >= cap) { toks[nn++] = tk.eot; fin = 1; }  // :367-370
    else if (next == tk.eot) fin = 1;                 // :317
    else if (max_new > 0 && nn - prompt_len >= max_new) { toks[nn++] = tk.eot; fin = 1; }  // bench knob
    s.n_tokens[b] = nn;
    if (fin) s.done[b] = 1;
}

// ---- sampled decoding, t > 0 (model.rs:340-348) ------------------------------------------------------------
// The reference draws from rand's WeightedIndex over softmax(q / t), q = the rule-masked PROBABILITIES, with an
// entropy-seeded StdRng, so only its distribution can be matched.  The seeded contract (include/norma_hip.h):
//   w_i = sexp((q_i - max q) * inv_t)        sexp: exp from IEEE f32 operations only, identical in the C oracle
//   u   = (philox4x32-10(key = seed, ctr = {step, clip, attempt, "norm"})[0] >> 8) * 2^-24
//   token = first j whose cumulative weight exceeds u * total, cumulated in f64 over 1024 chunks of ceil(V / 1024)
// One 1024-thread workgroup per sequence; thread c owns chunk c, thread 0 then walks the chunk sums.
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned &o0) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o0 = c0;
}

__device__ __forceinline__ float sexp(float y) {
#pragma clang fp contract(off)
    if (!(y >= -87.0f)) return 0.0f;  // also -inf and NaN: a masked token has weight 0
    const float kf = floorf(__builtin_fmaf(y, 1.44269504088896341f, 0.5f));
    float r = __builtin_fmaf(kf, -0.693359375f, y);
    r = __builtin_fmaf(kf, 2.12194440e-4f, r);
    float p = 1.9875691500e-4f;
    p = __builtin_fmaf(p, r, 1.3981999507e-3f);
    p = __builtin_fmaf(p, r, 8.3334519073e-3f);
    p = __builtin_fmaf(p, r, 4.1665795894e-2f);
    p = __builtin_fmaf(p, r, 1.6666665459e-1f);
    p = __builtin_fmaf(p, r, 5.0000001201e-1f);
    const float z = r * r;
    const float res = __builtin_fmaf(p, z, r) + 1.0f;
    return res * __uint_as_float((unsigned)((int)kf + 127) << 23);
}

struct SampleShared { BlockRed red; double chunk[1024]; int result; float qres; };

// q(i): rule-masked probability.  Returns (all threads) the sampled token or -1 when everything is masked; qout = q(token).
template <typename QFn>
__device__ __forceinline__ int sample_masked(QFn q, int V, float inv_t, unsigned long long seed, unsigned clip, unsigned step,
                                             unsigned attempt, SampleShared &sh, float &qout) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    float mx = -INFINITY;
    for (int i = tid; i < V; i += 1024) mx = fmaxf(mx, q(i));
    const float qmax = block_max(mx, sh.red.fa);
    if (!(qmax > -INFINITY)) { qout = 0.f; return -1; }
    const int CH = (V + 1023) / 1024;
    double sc = 0.0;
    for (int i = tid * CH; i < (tid + 1) * CH && i < V; i++) sc += (double)sexp((q(i) - qmax) * inv_t);
    sh.chunk[tid] = sc;
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int c = 0; c < 1024; c++) total += sh.chunk[c];
        unsigned r0;
        philox4x32_10(step, clip, attempt, 0x6e6f726du, (unsigned)seed, (unsigned)(seed >> 32), r0);
        const float u = (float)(r0 >> 8) * (1.0f / 16777216.0f);
        const double x = (double)u * total;
        double run = 0.0;
        int c = 0;
        for (; c < 1023; c++) { if (run + sh.chunk[c] > x) break; run += sh.chunk[c]; }
        int res = -1, last_pos = -1;
        for (int i = c * CH; i < V; i++) {  // walks on past the chunk only if rounding left x >= the chunk's end
            const float w = sexp((q(i) - qmax) * inv_t);
            if (w > 0.0f) last_pos = i;
            run += (double)w;
            if (run > x) { res = i; break; }
        }
        if (res < 0) res = last_pos;
        sh.result = res; sh.qres = q(res);
    }
    __syncthreads();
    qout = sh.qres;
    return sh.result;
}

// one generated token per sequence at temperature 1 / inv_t: softmax, rules, sampling, the bookkeeping of
// model.rs:359-370.  Same state as logit_step_kernel (which stays the t = 0 path and the no-speech probe).
__global__ __launch_bounds__(1024) void sample_step_kernel(const float *__restrict__ logits, int V, int ldl, DecodeState s,
                                                           RuleTokens tk, int ctx, int cap, int max_new, int prompt_len,
                                                           float inv_t, unsigned long long seed, unsigned clip0, unsigned attempt) {
    __shared__ SampleShared sh;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (s.done[b]) return;
    const float *lg = logits + (long)b * ldl;
    float mx = -INFINITY;
    for (int i = tid; i < V; i += 1024) mx = fmaxf(mx, lg[i]);
    const float m = block_max(mx, sh.red.fa);
    float se = 0.f;
    for (int i = tid; i < V; i += 1024) se += expf(lg[i] - m);
    se = block_sum(se, sh.red.fb);
    auto probs = [&](int i) { return expf(lg[i] - m) / se; };  // model.rs:331
    int32_t *toks = s.tokens + (long)b * ctx;
    const int n = s.n_tokens[b], have_last = s.have_last[b], last_ts = s.last_ts[b];
    const int rule = rules_decide(probs, V, toks, n, have_last, s.suppress, tk, sh.red);
    auto q = [&](int i) { return masked_value(probs(i), i, rule, s.suppress, tk, last_ts); };
    float qv;
    const int next = sample_masked(q, V, inv_t, seed, clip0 + b, (unsigned)n, attempt, sh, qv);
    if (tid != 0) return;
    int nn = n, fin = 0;
    if (next < 0) { toks[nn++] = tk.eot; fin = 1; }                // :343-346 all NaN: push eot, stop (no log-prob)
    else {
        if (next > tk.no_timestamps) { s.last_ts[b] = next; s.have_last[b] = 1; }  // :359-361
        toks[nn++] = next;
        s.sum_logprob[b] += log((double)qv);                       // :364-365
        if (nn >= cap) { toks[nn++] = tk.eot; fin = 1; }           // :367-370
        else if (next == tk.eot) fin = 1;                          // :317
        else if (max_new > 0 && nn - prompt_len >= max_new) { toks[nn++] = tk.eot; fin = 1; }
    }
    s.n_tokens[b] = nn;
    if (fin) s.done[b] = 1;
}

void launch_sample_step(const float *logits, int V, DecodeState s, RuleTokens tk, int B, int ctx, int cap, int max_new,
                        int prompt_len, float inv_t, unsigned long long seed, unsigned clip0, unsigned attempt, hipStream_t st) {
    hipLaunchKernelGGL(sample_step_kernel, dim3(B), dim3(1024), 0, st, logits, V, nh_logits_ld(V), s, tk, ctx, cap, max_new, prompt_len,
                       inv_t, seed, clip0, attempt);
}

// decode pool: sample_step_kernel for the rows of a pool that are sampled.  One workgroup per row; it acts on a row that has
// inv_t > 0, is running and stands at a generation position, draws its token and keeps its books exactly as sample_step_kernel
// does (same device functions, same order: the bits are the lockstep path's), and advances its position.  Every step it also
// tells logit_step_kernel (mode 2, launched next on the same stream) which rows it has dealt with: handled[b].  The two
// kernels never decide that through pos[b], which one of them has moved by then.
__global__ __launch_bounds__(1024) void pool_sample_step_kernel(const float *__restrict__ logits, int V, int ldl, DecodeState s,
                                                                RuleTokens tk, int ctx, int cap, int max_new, int prompt_len,
                                                                PoolSampling ps, int32_t *pos, const int32_t *pfx) {
    __shared__ SampleShared sh;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float inv_t = ps.inv_t[b];
    if (pfx) prompt_len += pfx[b];   // nh_pool_prefix: the row's physical prompt
    const int my_pos = pos[b];  // read by every thread ahead of the first barrier; thread 0 moves it after the last
    const bool mine = inv_t > 0.f && !s.done[b] && my_pos >= prompt_len - 1;
    if (tid == 0) ps.handled[b] = mine ? 1 : 0;
    if (!mine) return;
    const float *lg = logits + (long)b * ldl;
    float mx = -INFINITY;
    for (int i = tid; i < V; i += 1024) mx = fmaxf(mx, lg[i]);
    const float m = block_max(mx, sh.red.fa);
    float se = 0.f;
    for (int i = tid; i < V; i += 1024) se += expf(lg[i] - m);
    se = block_sum(se, sh.red.fb);
    auto probs = [&](int i) { return expf(lg[i] - m) / se; };  // model.rs:331
    int32_t *toks = s.tokens + (long)b * ctx;
    const int n = s.n_tokens[b], have_last = s.have_last[b], last_ts = s.last_ts[b];
    const int rule = rules_decide(probs, V, toks, n, have_last, s.suppress, tk, sh.red);
    auto q = [&](int i) { return masked_value(probs(i), i, rule, s.suppress, tk, last_ts); };
    float qv;
    const int next = sample_masked(q, V, inv_t, ps.seed[b], ps.clip[b], (unsigned)n, ps.attempt[b], sh, qv);
    if (tid != 0) return;
    int nn = n, fin = 0;
    if (next < 0) { toks[nn++] = tk.eot; fin = 1; }                // :343-346 all NaN: push eot, stop (no log-prob)
    else {
        if (next > tk.no_timestamps) { s.last_ts[b] = next; s.have_last[b] = 1; }  // :359-361
        toks[nn++] = next;
        s.sum_logprob[b] += log((double)qv);                       // :364-365
        if (nn >= cap) { toks[nn++] = tk.eot; fin = 1; }           // :367-370
        else if (next == tk.eot) fin = 1;                          // :317
        else if (max_new > 0 && nn - prompt_len >= max_new) { toks[nn++] = tk.eot; fin = 1; }
    }
    s.n_tokens[b] = nn;
    if (fin) s.done[b] = 1;
    pos[b] = my_pos + 1;
}

void launch_pool_sample_step(const float *logits, int V, DecodeState s, RuleTokens tk, int B, int ctx, int cap, int max_new,
                             int prompt_len, PoolSampling ps, int32_t *pos, hipStream_t st, const int32_t *pfx) {
    hipLaunchKernelGGL(pool_sample_step_kernel, dim3(B), dim3(1024), 0, st, logits, V, nh_logits_ld(V), s, tk, ctx, cap, max_new, prompt_len,
                       ps, pos, pfx);
}

// parity view of the sampler: rules + one draw on an already soft-maxed probability vector
__global__ __launch_bounds__(1024) void sample_rules_kernel(const float *__restrict__ probs_in, int32_t *token_out,
                                                            const int32_t *tokens, int n, int last_ts, const uint8_t *sup,
                                                            RuleTokens tk, int V, float inv_t, unsigned long long seed,
                                                            unsigned clip, unsigned attempt) {
    __shared__ SampleShared sh;
    auto probs = [&](int i) { return probs_in[i]; };
    const int rule = rules_decide(probs, V, tokens, n, last_ts >= 0, sup, tk, sh.red);
    auto q = [&](int i) { return masked_value(probs_in[i], i, rule, sup, tk, last_ts); };
    float qv;
    const int next = sample_masked(q, V, inv_t, seed, clip, (unsigned)n, attempt, sh, qv);
    if (threadIdx.x == 0) *token_out = next;
}

void launch_sample_rules(const float *probs_in, int32_t *token_out, const int32_t *tokens, int n_tokens, int last_ts,
                         const uint8_t *suppress, RuleTokens tk, int V, float inv_t, unsigned long long seed, unsigned clip,
                         unsigned attempt, hipStream_t st) {
    hipLaunchKernelGGL(sample_rules_kernel, dim3(1), dim3(1024), 0, st, probs_in, token_out, tokens, n_tokens, last_ts, suppress,
                       tk, V, inv_t, seed, clip, attempt);
}

// ---- the fused decode-step version: ONE sweep over the logits, LSPLIT workgroups per sequence -----------
// softmax is monotonic, so the arg max over an allowed set can be taken on the logits; which set is
// allowed is known before the sweep except for the "last token is text" case, where both candidates
// (best timestamp after last_ts, best allowed text token) are tracked and the choice
// sum_ts >= max_text is made by the last workgroup to arrive.  (Two DISTINCT logits whose f32
// probabilities round to the same value would tie in the reference and resolve to the higher index;
// here the larger logit wins.  That needs a relative gap < 6e-8 and is far below the fp16 noise floor.)
#define LSPLIT 8
constexpr int LMAX = 32;  // logits per thread: ceil(51866 / 8 / 256) = 26 for the largest Whisper vocabulary
static_assert(NH_MAX_VOCAB == LSPLIT * 256 * LMAX, "logit_step_kernel holds exactly NH_MAX_VOCAB logits in registers");

// what logit_step_kernel knows about a sequence BEFORE its sweep: what rule_from_state (k_device.h) says.  The first three
// are the RULE_* of the same name; STEP_TEXT (the last token is text) becomes RULE_NON_TS or RULE_PAST only when the last
// workgroup compares sum_ts with max_text, so RULE_PAST has no counterpart here; STEP_PROBE is mode 0, which selects no token.
enum { STEP_FIRST = RULE_FIRST, STEP_SUP_TS = RULE_SUP_TS, STEP_NON_TS = RULE_NON_TS, STEP_TEXT = RULE_BY_MASS, STEP_PROBE = 5 };

__device__ __forceinline__ void merge_ms(float &m, float &s, float &ts, float m2, float s2, float ts2) {
    float f1, f2;  // the timestamp mass is a sum against the same maxima
    merge_pair(m, s, m2, s2, f1, f2);
    ts = ts * f1 + ts2 * f2;
}

__global__ __launch_bounds__(256) void logit_step_kernel(const float *__restrict__ logits, int V, int ldl,
                                                         DecodeState s, RuleTokens tk, int ctx, int cap, int max_new,
                                                         int prompt_len, int mode, float *partials, unsigned *tickets,
                                                         int32_t *pos_ptr, const int32_t *handled, const int32_t *pfx) {
    __shared__ float sh_f[4][6];
    __shared__ int sh_i[4][2];
    __shared__ int sh_last;
    const int b = blockIdx.y, part = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float *lg = logits + (long)b * ldl;
    const int per = (V + LSPLIT - 1) / LSPLIT, lo = part * per, hi = min(V, lo + per);
    // fetch the whole slice first: the statistics below are a dependent chain, the loads are not
    // (they are issued before the per-sequence state is even looked at -- one memory round trip for both)
    float lv[LMAX]; unsigned char sv[LMAX];
#pragma unroll
    for (int u = 0; u < LMAX; u++) {  // unconditional (clamped) loads: a guarded load makes hipcc wait vmcnt(0) per element
        int i = lo + tid + 256 * u;
        int ic = i < hi ? i : hi - 1;
        lv[u] = lg[ic];
        sv[u] = s.suppress[ic];
    }
    const int32_t *toks = s.tokens + (long)b * ctx;
    const int done = s.done[b];
    const int my_pos = pos_ptr ? pos_ptr[b] : 0;  // this sequence's position; advanced below by whoever finishes its step
    const int n = s.n_tokens[b];
    const int have_last = s.have_last[b], last_ts = s.last_ts[b];
    const double sum_lp_in = s.sum_logprob[b];  // prefetched for the bookkeeping at the end
    const int l1 = toks[n >= 1 ? n - 1 : 0], l2 = toks[n >= 2 ? n - 2 : 0];  // unconditional: one round trip for both
    const float l_nt = lg[tk.no_timestamps];           // no_timestamps is text to supress_past_timestamps only (see below)
    const int sup_nt = s.suppress[tk.no_timestamps];
    const int taken = handled ? handled[b] : 0;  // decode pool: pool_sample_step_kernel generated this sequence's token in this step
    const int npfx = pfx ? pfx[b] : 0;           // decode pool: the row's prefix (nh_pool_prefix); lockstep launches pass no array
    if (done || taken) return;                   // (all LSPLIT workgroups leave before any takes a ticket)
    // mode 2 (decode pool): sequences join a running decode, so each is in its own phase -- the position of sot (0, or behind the
    // row's prefix) is the no-speech probe, the other prompt positions, and those of a prefix that goes through the steps, only
    // feed the caches (their next token is given), then it generates
    if (mode == 2) {
        prompt_len += npfx;
        mode = my_pos == npfx ? 0 : (my_pos < prompt_len - 1 ? 3 : 1);
        if (mode == 3) {  // the position moves only when all LSPLIT workgroups of the sequence have read it: same ticket as below
            if (tid == 0 && __hip_atomic_fetch_add(tickets + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == LSPLIT - 1) {
                __hip_atomic_store(tickets + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                pos_ptr[b] = my_pos + 1;
            }
            return;
        }
    }
    const int NT = tk.no_timestamps;
    // candidate sets: A = allowed non-timestamp tokens (or the first-token window), B = allowed timestamps
    const int kind = mode == 0 ? STEP_PROBE : rule_from_state(have_last, n, l1, l2, tk);
    float m = -INFINITY, se = 0.f, ts = 0.f, tsinf = 0.f, av = -INFINITY, bv = -INFINITY;
    int ai = -1, bi = -1;
    // slice maximum first, then one exp per element against it (the slice lives in registers)
#pragma unroll
    for (int u = 0; u < LMAX; u++) m = fmaxf(m, lv[u]);
    // a thread whose logits are all -inf (the guard's loop exit leaves eot alone, k_guard.hip): exp(-inf - -inf) is NaN,
    // exp(-inf + FLT_MAX) is 0, and its pair (-inf, 0) then merges as nothing.  A finite m is its own maximum with -FLT_MAX.
    // Spelled as a maximum, not as a select on m == -inf: a select lets the compiler fold the merge factors below and drop
    // the fused multiply-add of the first merge, which moves sums by an ulp.
    const float me = fmaxf(m, -3.402823466e+38f);   // -FLT_MAX
#pragma unroll
    for (int u = 0; u < LMAX; u++) {
        const int i = lo + tid + 256 * u;
        if (i >= hi) continue;
        const float l = lv[u];
        const bool is_ts = i > NT;
        const bool sup = sv[u] != 0;
        const float e = __expf(l - me);  // softmax mass, and the timestamp mass of model.rs:263-266
        se += e;
        if (is_ts) { ts += e; if (sup) tsinf = 1.f; }  // p + (-inf) inside the summed slice -> the sum is -inf
        if (kind == STEP_FIRST) { if (i >= tk.zero_sec && i <= tk.one_sec) better(av, ai, l, i); }
        else if (kind == STEP_SUP_TS) { if (!is_ts && !sup) better(av, ai, l, i); }
        else if (kind == STEP_NON_TS) { if (is_ts && i > last_ts && !sup) better(bv, bi, l, i); }
        else if (kind == STEP_TEXT) {  // max_text of model.rs:267-270 runs over i < no_timestamps
            if (i < NT && !sup) better(av, ai, l, i);
            else if (is_ts && i > last_ts && !sup) better(bv, bi, l, i);
        }
    }
    // wave reduction
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        merge_ms(m, se, ts, __shfl_xor(m, o), __shfl_xor(se, o), __shfl_xor(ts, o));
        tsinf = fmaxf(tsinf, __shfl_xor(tsinf, o));
        better(av, ai, __shfl_xor(av, o), __shfl_xor(ai, o));
        better(bv, bi, __shfl_xor(bv, o), __shfl_xor(bi, o));
    }
    if (lane == 0) { sh_f[w][0] = m; sh_f[w][1] = se; sh_f[w][2] = ts; sh_f[w][3] = tsinf; sh_f[w][4] = av; sh_f[w][5] = bv; sh_i[w][0] = ai; sh_i[w][1] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int ww = 1; ww < 4; ww++) {
            merge_ms(m, se, ts, sh_f[ww][0], sh_f[ww][1], sh_f[ww][2]);
            tsinf = fmaxf(tsinf, sh_f[ww][3]);
            better(av, ai, sh_f[ww][4], sh_i[ww][0]);
            better(bv, bi, sh_f[ww][5], sh_i[ww][1]);
        }
        // publish the partial (agent-scope atomics: other workgroups may sit on another XCD/L2), then take a ticket
        float *pp = partials + ((long)b * LSPLIT + part) * 8;
        __hip_atomic_store(pp + 0, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(pp + 1, se, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(pp + 2, ts, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(pp + 3, tsinf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(pp + 4, av, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(pp + 5, bv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(reinterpret_cast<int *>(pp) + 6, ai, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(reinterpret_cast<int *>(pp) + 7, bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // Hand-off to the last arriver.  The payload above went out as agent-scope (sc1, write-through) atomic stores; on gfx950
        // `s_waitcnt vmcnt(0)` returns only when the memory side has acknowledged them, so a relaxed ticket RMW issued after
        // it cannot be observed before them, and the last arriver reads the payload with sc1 loads that bypass its own L2.
        // That is the ISA-level contract this library (gfx950 only) relies on.  The portable spelling -- a RELEASE ticket +
        // an ACQUIRE fence in the last arriver, -DNH_STRICT_MEMORY_MODEL -- makes every arrival write back its whole L2
        // (buffer_wbl2): measured -2 % end-to-end with three batches in flight (5940 vs 6060 audio-s/s), same results.
#if defined(NH_STRICT_MEMORY_MODEL)
        unsigned t = __hip_atomic_fetch_add(tickets + b, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        if (t == LSPLIT - 1) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned t = __hip_atomic_fetch_add(tickets + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
        sh_last = (t == LSPLIT - 1);
    }
    __syncthreads();
    if (!sh_last || w != 0) return;
    // ---- last workgroup of this sequence: combine and do the bookkeeping of model.rs:331-370 ----
    // one L2 round trip: lane 8 q + f fetches field f of partial q, thread 0 then walks them by shuffle
    const unsigned raw = __hip_atomic_load(reinterpret_cast<const unsigned *>(partials) + (long)b * LSPLIT * 8 + lane,
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    m = -INFINITY; se = 0.f; ts = 0.f; tsinf = 0.f; av = -INFINITY; bv = -INFINITY; ai = -1; bi = -1;
#pragma unroll
    for (int q = 0; q < LSPLIT; q++) {
        float m2 = __uint_as_float(__shfl(raw, 8 * q + 0)), s2 = __uint_as_float(__shfl(raw, 8 * q + 1));
        float t2 = __uint_as_float(__shfl(raw, 8 * q + 2)), i2 = __uint_as_float(__shfl(raw, 8 * q + 3));
        float a2 = __uint_as_float(__shfl(raw, 8 * q + 4)), b2 = __uint_as_float(__shfl(raw, 8 * q + 5));
        int ai2 = (int)__shfl(raw, 8 * q + 6), bi2 = (int)__shfl(raw, 8 * q + 7);
        merge_ms(m, se, ts, m2, s2, t2);
        tsinf = fmaxf(tsinf, i2);
        better(av, ai, a2, ai2);
        better(bv, bi, b2, bi2);
    }
    if (tid != 0) return;
    __hip_atomic_store(tickets + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next token
    if (mode == 0) {  // model.rs:293-315
        float p = expf(lg[tk.no_speech] - m) / se;
        s.no_speech[b] = (double)p;
        if ((double)p > 0.6) s.done[b] = 2;
        if (pos_ptr) pos_ptr[b] = my_pos + 1;
        return;
    }
    if (pos_ptr) pos_ptr[b] = my_pos + 1;  // every workgroup of this sequence read it before taking its ticket
    int next = -1; float lnext = 0.f;
    if (kind == STEP_FIRST || kind == STEP_SUP_TS) { next = ai; lnext = av; }
    else if (kind == STEP_NON_TS) { next = bi; lnext = bv; }
    else {
        float sum_ts = tsinf > 0.f ? -INFINITY : ts / se;          // probabilities, as the reference compares them
        float max_text = ai >= 0 ? expf(av - m) / se : -INFINITY;
        if (sum_ts >= max_text) { next = bi; lnext = bv; }          // supress_non_timestamps
        else {                                                      // supress_past_timestamps only
            next = ai; lnext = av; better(lnext, next, bv, bi);
            if (!sup_nt) better(lnext, next, l_nt, NT);             // left unmasked when suppress lacks it
        }
    }
    float pv;
    if (next < 0) { next = V - 1; pv = -INFINITY; }  // every candidate masked: all -inf, last index wins (H3)
    else pv = expf(lnext - m) / se;
    s.sum_logprob[b] = sum_lp_in + log((double)pv);               // :364-365
    append_token(s, b, s.tokens + (long)b * ctx, n, next, tk, cap, max_new, prompt_len);
}

void launch_logit_step(const float *logits, int V, DecodeState s, RuleTokens tk, int B, int ctx, int cap,
                       int max_new, int prompt_len, int mode, float *partials, unsigned *tickets, int32_t *pos_ptr,
                       hipStream_t st, const int32_t *handled, const int32_t *pfx) {
    hipLaunchKernelGGL(logit_step_kernel, dim3(LSPLIT, B), dim3(256), 0, st, logits, V, nh_logits_ld(V), s, tk, ctx, cap, max_new,
                       prompt_len, mode, partials, tickets, pos_ptr, handled, mode == 2 ? pfx : nullptr);
}

// decode pool: what admission and retry both clear -- row `row` stands at position pos0 with its n prefix and P prompt tokens
// and no history
__device__ __forceinline__ void pool_row_reset(const DecodeState &s, int32_t *pos, unsigned *tickets, int row, int P, int n, int pos0) {
    s.n_tokens[row] = n + P; s.done[row] = 0; s.have_last[row] = 0; s.last_ts[row] = 0;
    s.sum_logprob[row] = 0.0; s.no_speech[row] = 0.0;
    pos[row] = pos0; tickets[row] = 0u;
}

// decode pool: sequence `row` starts over with the prompt [t0, t1, (t2)] (model.rs:285-289), at position 0 unless pfx says otherwise.  detect_flag
// (i32 [B] or null): whether the row detects its language in its first step (t1 is a placeholder until then).  pfx (i32 [B] or
// null; nh_pool_prefix): the row's prefix length n_prefix is recorded there, the prompt sits behind the n_prefix ids (which
// the caller copies into the row) and the row starts at pos0: 0, or n_prefix when one pass consumes the prefix.
__global__ void pool_admit_kernel(DecodeState s, int32_t *pos, unsigned *tickets, int row, int ctx, int t0, int t1, int t2, int P,
                                  int32_t *detect_flag, int detect, int32_t *pfx, int n_prefix, int pos0) {
    int32_t *t = s.tokens + (long)row * ctx + n_prefix;
    t[0] = t0; t[1] = t1; if (P == 3) t[2] = t2;
    pool_row_reset(s, pos, tickets, row, P, n_prefix, pos0);
    if (detect_flag) detect_flag[row] = detect;
    if (pfx) pfx[row] = n_prefix;
}
void launch_pool_admit(DecodeState s, int32_t *pos, unsigned *tickets, int row, int ctx, int t0, int t1, int t2, int P, hipStream_t st,
                       int32_t *detect_flag, int detect, int32_t *pfx, int n_prefix, int pos0) {
    if (!pfx) n_prefix = pos0 = 0;
    hipLaunchKernelGGL(pool_admit_kernel, dim3(1), dim3(1), 0, st, s, pos, tickets, row, ctx, t0, t1, t2, P, detect_flag, detect, pfx,
                       n_prefix, pos0);
}

// decode pool: sequence `row` decodes the clip it holds once more, sampled.  The prompt tokens [0, P) are still in place
// (generation writes from P on; the trimming of finish_sequence works on the host copy), so is the clip's cross K/V.
// A language the row detected in its t = 0 attempt is one of those prompt tokens: the retry does not detect again.
// Under a prefix (pfx[row] = n > 0) the row restarts at position n: the self K/V of positions 0 .. n-1 are still in its cache,
// whichever route wrote them, because generation wrote only from n on.
__global__ void pool_retry_kernel(DecodeState s, int32_t *pos, unsigned *tickets, PoolSampling ps, int row, int P, float inv_t,
                                  unsigned long long seed, unsigned clip, unsigned attempt, int32_t *detect_flag, const int32_t *pfx) {
    const int n = pfx ? pfx[row] : 0;
    pool_row_reset(s, pos, tickets, row, P, n, n);
    ps.inv_t[row] = inv_t; ps.seed[row] = seed; ps.clip[row] = clip; ps.attempt[row] = attempt;
    if (detect_flag) detect_flag[row] = 0;
}
void launch_pool_retry(DecodeState s, int32_t *pos, unsigned *tickets, PoolSampling ps, int row, int P, float inv_t,
                       unsigned long long seed, unsigned clip, unsigned attempt, hipStream_t st, int32_t *detect_flag,
                       const int32_t *pfx) {
    hipLaunchKernelGGL(pool_retry_kernel, dim3(1), dim3(1), 0, st, s, pos, tickets, ps, row, P, inv_t, seed, clip, attempt, detect_flag, pfx);
}

// Model::detect_language (model.rs:194-210) on the position-0 logits of a [sot] prompt: softmax over the language
// tokens and the FIRST maximum (the reference sorts descending with a stable sort).  One whole wave per sequence; every
// lane returns the winner's index in lang_tokens.  probs_row: f32 [n] or nullptr.  The one place this arithmetic lives:
// lang_detect_kernel (nh_detect_language) and pool_lang_detect_kernel (the decode pool) both call it.
__device__ __forceinline__ int lang_softmax_wave(const float *__restrict__ lg, const int32_t *__restrict__ lang_tokens, int n,
                                                 float *__restrict__ probs_row, int lane) {
    float v[4]; int idx[4];
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        idx[u] = lane + 64 * u;
        v[u] = idx[u] < n ? lg[lang_tokens[idx[u] < n ? idx[u] : 0]] : -INFINITY;
        mx = fmaxf(mx, v[u]);
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float se = 0.f, e[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { e[u] = idx[u] < n ? expf(v[u] - mx) : 0.f; se += e[u]; }
    for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
    int bk = INT_MIN, bi = 0x7fffffff;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        if (idx[u] < n) {
            float p = e[u] / se;
            if (probs_row) probs_row[idx[u]] = p;
            int key = total_key(p);
            if (key > bk || (key == bk && idx[u] < bi)) { bk = key; bi = idx[u]; }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        int k2 = __shfl_xor(bk, o), i2 = __shfl_xor(bi, o);
        if (k2 > bk || (k2 == bk && i2 < bi)) { bk = k2; bi = i2; }
    }
    return bi;
}

__global__ __launch_bounds__(64) void lang_detect_kernel(const float *__restrict__ logits, int ldl,
                                                         const int32_t *__restrict__ lang_tokens, int n,
                                                         float *__restrict__ probs_out, int32_t *__restrict__ lang_out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int bi = lang_softmax_wave(logits + (long)b * ldl, lang_tokens, n, probs_out ? probs_out + (long)b * n : nullptr, lane);
    if (lane == 0) lang_out[b] = lang_tokens[bi];
}

void launch_lang_detect(const float *logits, int V, const int32_t *lang_tokens, int n, float *probs_out, int32_t *lang_out,
                        int B, hipStream_t st) {
    hipLaunchKernelGGL(lang_detect_kernel, dim3(B), dim3(64), 0, st, logits, nh_logits_ld(V), lang_tokens, n, probs_out, lang_out);
}

// decode pool: a row admitted with NH_LANG_DETECT detects its language in the step it takes at position 0 -- that step IS
// Model::detect_language's forward on [sot].  One wave per row, launched after the step's logits and ahead of
// logit_step_kernel (which moves pos[b]); only the step graphs of a pool that has a language table carry it.  Lane 0 writes
// the token into the row's own prompt; the embedding of position 1, a later kernel on the same stream, is the first to read
// it.  A row that the no-speech probe ends in this very step is detected too: the reference detects before it decodes.
__global__ __launch_bounds__(64) void pool_lang_detect_kernel(const float *__restrict__ logits, int ldl, DecodeState s, int ctx,
                                                              const int32_t *__restrict__ pos, PoolDetect det) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (!det.flag[b] || s.done[b] || pos[b] != 0) return;
    const int bi = lang_softmax_wave(logits + (long)b * ldl, det.lang_tokens, det.n, det.probs + (long)b * 256, lane);
    if (lane == 0) {
        const int32_t lt = det.lang_tokens[bi];
        s.tokens[(long)b * ctx + 1] = lt;
        det.lang_out[b] = lt;
    }
}

void launch_pool_lang_detect(const float *logits, int V, DecodeState s, int B, int ctx, const int32_t *pos, PoolDetect det,
                             hipStream_t st) {
    hipLaunchKernelGGL(pool_lang_detect_kernel, dim3(B), dim3(64), 0, st, logits, nh_logits_ld(V), s, ctx, pos, det);
}

__global__ __launch_bounds__(1024) void rules_only_kernel(const float *__restrict__ probs_in, float *masked_out,
                                                          int32_t *argmax_out, const int32_t *tokens, int n,
                                                          int last_ts, const uint8_t *sup, RuleTokens tk, int V) {
    __shared__ BlockRed sm;
    auto probs = [&](int i) { return probs_in[i]; };
    const int rule = rules_decide(probs, V, tokens, n, last_ts >= 0, sup, tk, sm);
    int bk = INT_MIN, bi = -1;  // the greedy arg max of model.rs:350-356
    for (int i = threadIdx.x; i < V; i += blockDim.x) {
        const float v = masked_value(probs_in[i], i, rule, sup, tk, last_ts);
        masked_out[i] = v;
        const int k = total_key(v);
        if (k > bk || (k == bk && i > bi)) { bk = k; bi = i; }
    }
    int ok, next;
    block_argmax(bk, bi, sm, ok, next);
    if (threadIdx.x == 0) *argmax_out = next;
}

void launch_rules_only(const float *probs_in, float *masked_out, int32_t *argmax_out, const int32_t *tokens,
                       int n_tokens, int last_ts, const uint8_t *suppress, RuleTokens tk, int V, hipStream_t st) {
    hipLaunchKernelGGL(rules_only_kernel, dim3(1), dim3(1024), 0, st, probs_in, masked_out, argmax_out, tokens,
                       n_tokens, last_ts, suppress, tk, V);
}
