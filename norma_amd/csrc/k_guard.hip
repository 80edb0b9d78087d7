// k_guard.hip -- the repetition guard of a decode step (gfx950; contract: nh_set_guard in include/norma_hip.h).
// One kernel between the step's logits and the selection kernels: it edits the f32 logits of every row that is running and
// stands at a generation position, from nothing but the tokens the row has generated.
//   guard_kernel   one 256-thread workgroup per row: the text history h (generated ids < eot) compacted in order into LDS,
//                  then the four stages in the contract's order -- repetition penalty, bias, no-repeat n-gram, loop exit --
//                  with a barrier between them (a later stage may touch a logit an earlier one wrote).
// Every edit is one IEEE f32 operation or an assignment, each logit written by exactly one thread per stage (or by several
// with the same value, -inf): the result does not depend on any order of arrival.
#include "k_device.h"

#define GUARD_THREADS 256
static_assert(GUARD_THREADS == 256 && NH_GUARD_MAX_PERIOD * 4 == GUARD_THREADS, "stage 4 gives every period four threads");

__global__ __launch_bounds__(GUARD_THREADS) void guard_kernel(float *__restrict__ logits, int V, int ldl, DecodeState s, RuleTokens tk,
                                                              int ctx, int prompt_len, const int32_t *__restrict__ pos, GuardSpec g,
                                                              GuardBufs gb, const int32_t *__restrict__ pfx) {
    // h[m .. m + 3] is padding for the 16-byte reads of stage 1
    __shared__ __attribute__((aligned(16))) int32_t h[NH_GUARD_MAX_HISTORY + 4];
    __shared__ int wave_cnt[GUARD_THREADS / 64];
    __shared__ int bad[NH_GUARD_MAX_PERIOD];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // everything up to the first barrier is the same in every thread: whole workgroups leave
    if (s.done[b]) return;
    if (pos && pfx) prompt_len += pfx[b];         // decode pool: the row's prefix (nh_pool_prefix) is part of its physical prompt
    if (pos && pos[b] < prompt_len - 1) return;   // decode pool: the row is at its probe or inside its prompt
    const int n = s.n_tokens[b];
    if (n < prompt_len) return;
    const int32_t *toks = s.tokens + (long)b * ctx;
    float *lg = logits + (long)b * ldl;
    if (tid == 0 && n == prompt_len) gb.loop_exit[b] = 0;   // first generation position: admit, retry and a new decode start clean
    const int glen = min(n - prompt_len, NH_GUARD_MAX_HISTORY);

    // ---- h: the ids < eot of tokens[prompt_len .. n), in order (ballot + prefix counts, no atomic append) ----
    int m = 0;
    for (int base = 0; base < glen; base += GUARD_THREADS) {
        const int i = base + tid;
        const int tok = i < glen ? toks[prompt_len + i] : tk.eot;
        const bool keep = tok < tk.eot;
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wave_cnt[w] = __popcll(mask);
        __syncthreads();
        int off = m, total = 0;
        for (int ww = 0; ww < GUARD_THREADS / 64; ww++) { if (ww < w) off += wave_cnt[ww]; total += wave_cnt[ww]; }
        if (keep) h[off + __popcll(mask & ((1ull << lane) - 1ull))] = tok;
        m += total;
        __syncthreads();
    }
    if (tid < 4) h[m + tid] = -1;
    __syncthreads();

    // ---- 1. repetition penalty: the thread of history position i acts only if no j < i holds the same id ----
    if (g.penalty != 1.0f) {
        for (int i = tid; i < m; i += GUARD_THREADS) {
            const int v = h[i];
            bool dup = false;
            for (int j = 0; j < i; j += 4) {
                const int4 q = *reinterpret_cast<const int4 *>(h + j);
                dup = dup || q.x == v || (j + 1 < i && q.y == v) || (j + 2 < i && q.z == v) || (j + 3 < i && q.w == v);
            }
            if (!dup) {
                const float x = lg[v];
                lg[v] = x < 0.f ? x * g.penalty : __fdiv_rn(x, g.penalty);
            }
        }
        __syncthreads();
    }

    // ---- 2. bias: the list of the row's clip (no id twice: nh_guard_bias refuses duplicates) ----
    if (g.bias && gb.bias_n) {
        const int br = gb.bias_map ? gb.bias_map[b] : b % gb.bias_mod;
        if (br >= 0) {
            const int cnt = gb.bias_n[br];
            for (int k = tid; k < cnt; k += GUARD_THREADS) {
                const int v = gb.bias_tok[(long)br * NH_GUARD_MAX_BIAS + k];
                lg[v] = lg[v] + gb.bias_val[(long)br * NH_GUARD_MAX_BIAS + k];
            }
        }
        __syncthreads();
    }

    // ---- 3. no-repeat n-gram: every earlier occurrence of the last N - 1 text tokens bans the token that followed it ----
    const int N = g.ngram;
    if (N > 0 && m >= N - 1) {
        const int s0 = m - N + 1;
        for (int i = tid; i <= m - N; i += GUARD_THREADS) {
            bool match = true;
            for (int k = 0; k < N - 1; k++) match = match && h[i + k] == h[s0 + k];
            if (match) lg[h[i + N - 1]] = -INFINITY;
        }
        __syncthreads();
    }

    // ---- 4. loop exit: the last p * R text tokens are R copies of one block of p, for some p <= Pmax ----
    if (g.loop_period > 0) {
        const int R = g.loop_repeats;
        if (tid < NH_GUARD_MAX_PERIOD) bad[tid] = 0;
        __syncthreads();
        const int p = (tid >> 2) + 1, q = tid & 3;
        const bool cand = p <= g.loop_period && p * R <= m;
        if (cand) {
            const int len = p * (R - 1);   // m - 1 - i - p >= m - p * R >= 0
            bool mis = false;
            for (int i = q; i < len; i += 4) mis = mis || h[m - 1 - i] != h[m - 1 - i - p];
            if (mis) bad[p - 1] = 1;
        }
        __syncthreads();
        const int hit = __syncthreads_or(cand && q == 0 && !bad[p - 1]);
        // RULE_FIRST and RULE_NON_TS mask eot: the exit waits for the next step, h does not change meanwhile
        const int rule = rule_from_state(s.have_last[b], n, toks[n >= 1 ? n - 1 : 0], toks[n >= 2 ? n - 2 : 0], tk);
        if (hit && (rule == RULE_SUP_TS || rule == RULE_BY_MASS)) {
            // everything but eot's logit becomes -inf: 16-byte stores over the row, scalars around eot and at the tail
            const float4 ninf = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
            float4 *lg4 = reinterpret_cast<float4 *>(lg);   // rows start at multiples of 64 floats
            const int nv4 = V >> 2, e4 = tk.eot >> 2;
            for (int i = tid; i < nv4; i += GUARD_THREADS)
                if (i != e4) lg4[i] = ninf;
            if (tid < 4) {
                const int i = e4 * 4 + tid;
                if (i < V && i != tk.eot) lg[i] = -INFINITY;
            } else if (tid < 8) {
                const int i = nv4 * 4 + (tid - 4);
                if (i < V && (i >> 2) != e4) lg[i] = -INFINITY;
            }
            if (tid == 0) gb.loop_exit[b] = 1;
        }
    }
}

void launch_guard(float *logits, int V, DecodeState s, RuleTokens tk, int R, int ctx, int prompt_len, const int32_t *pos, GuardSpec g,
                  GuardBufs gb, hipStream_t st, const int32_t *pfx) {
    hipLaunchKernelGGL(guard_kernel, dim3(R), dim3(GUARD_THREADS), 0, st, logits, V, nh_logits_ld(V), s, tk, ctx, prompt_len, pos, g, gb, pfx);
}
