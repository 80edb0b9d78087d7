// k_beam.hip -- beam search on the device (gfx950), the work of one step AFTER the logits: DESIGN.md 14.
//   beam_select_kernel   per hypothesis row: f32 softmax statistics, the logit rules of model.rs:212-277 (the rule state is the
//                        row's own), and its K+1 best candidates (token, masked probability q)
//   beam_merge_kernel    per clip: the <= K (K+1) candidates scored s_h + log((double)q), ordered, walked; writes the clip's
//                        next hypotheses (tokens, counts, timestamp state, scores, done flags), the parent map and the
//                        finished records
//   beam_reorder_kernel  self-attention caches of every layer: row r takes positions 0 .. p of row parent[r]
// Rows are beam-major: hypothesis j of clip b is row j * B + b, so a clip's rows are touched by its own workgroup alone.
#include "k_device.h"

constexpr int BSEL_T = 1024;                       // threads of a selection workgroup: one row each
constexpr int BSEL_LT = NH_MAX_VOCAB / BSEL_T;     // logits a thread holds in registers
constexpr int BK1 = NH_MAX_BEAMS + 1;              // candidates kept per row
constexpr int BCAND = NH_MAX_BEAMS * BK1;          // ... and per clip
static_assert(BSEL_LT * BSEL_T == NH_MAX_VOCAB, "beam_select_kernel holds a whole row in registers");

struct BeamRed { float f[BSEL_T / 64]; int i[BSEL_T / 64]; float of; int oi; };

// One workgroup per row.  The row's V logits live in registers (BSEL_LT per thread, clamped unconditional loads: the pad
// columns V .. ldl-1 are never read).  Softmax statistics first; a row whose last token is text learns its rule from them
// (sum_ts >= max_text, model.rs:263-270, on probabilities as logit_step_kernel compares them); then the registers are masked
// to the rule's allowed set and K1 rounds of a block arg max pull the best candidates in order -- softmax is monotonic, so
// the order is taken on the logits (k_token.hip has the caveat), the probability q = expf(l - m) / se only for the winners.
__global__ __launch_bounds__(BSEL_T) void beam_select_kernel(const float *__restrict__ logits, int V, int ldl, DecodeState s,
                                                             RuleTokens tk, int ctx, int K1, int32_t *__restrict__ cand_tok,
                                                             float *__restrict__ cand_q, int32_t *__restrict__ cand_n) {
    __shared__ BeamRed sm;
    const int r = blockIdx.x, tid = threadIdx.x;
    if (s.done[r]) return;   // dead and finished rows: the merge reads nothing of theirs
    const float *lg = logits + (long)r * ldl;
    float lv[BSEL_LT];
#pragma unroll
    for (int u = 0; u < BSEL_LT; u++) {
        const int i = tid + BSEL_T * u;
        lv[u] = lg[i < V ? i : V - 1];
    }
    unsigned long long supbits = 0ull;   // the suppress flags of the thread's tokens, one bit each (a few loads at a time: registers)
#pragma unroll 4
    for (int u = 0; u < BSEL_LT; u++) {
        const int i = tid + BSEL_T * u;
        supbits |= (unsigned long long)(s.suppress[i < V ? i : V - 1] != 0) << u;
    }
    const int32_t *toks = s.tokens + (long)r * ctx;
    const int n = s.n_tokens[r], have_last = s.have_last[r], last_ts = s.last_ts[r];
    const int l1 = toks[n >= 1 ? n - 1 : 0], l2 = toks[n >= 2 ? n - 2 : 0];
    const int NT = tk.no_timestamps;
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < BSEL_LT; u++) if (tid + BSEL_T * u < V) mx = fmaxf(mx, lv[u]);
    const float m = block_max<BSEL_T / 64>(mx, sm.f);
    float se = 0.f, ts = 0.f, tsinf = 0.f, mt = -INFINITY;
#pragma unroll
    for (int u = 0; u < BSEL_LT; u++) {
        const int i = tid + BSEL_T * u;
        if (i >= V) continue;
        const bool sup = (supbits >> u) & 1ull;
        const float e = __expf(lv[u] - m);
        se += e;
        if (i > NT) { ts += e; if (sup) tsinf = 1.f; }   // p + (-inf) inside the summed slice: the sum is -inf
        else if (i < NT && !sup) mt = fmaxf(mt, lv[u]);  // max_text of model.rs:267-270 runs over i < no_timestamps
    }
    se = block_sum<BSEL_T / 64>(se, sm.f);
    int rule = rule_from_state(have_last, n, l1, l2, tk);
    if (rule == RULE_BY_MASS) {                                             // last token is text: decided by the masses
        ts = block_sum<BSEL_T / 64>(ts, sm.f);
        tsinf = block_max<BSEL_T / 64>(tsinf, sm.f);
        mt = block_max<BSEL_T / 64>(mt, sm.f);
        const float sum_ts = tsinf > 0.f ? -INFINITY : ts / se;
        const float max_text = mt > -INFINITY ? expf(mt - m) / se : -INFINITY;
        rule = (sum_ts >= max_text) ? RULE_NON_TS : RULE_PAST;
    }
#pragma unroll
    for (int u = 0; u < BSEL_LT; u++) {
        const int i = tid + BSEL_T * u;
        const bool sup = (supbits >> u) & 1ull;
        if (i >= V || rule_masks(rule, i, sup, tk, last_ts)) lv[u] = -INFINITY;
    }
    // K1 rounds: the best candidate strictly after the one before in (value desc, index desc)
    float pv = INFINITY; int pi = 0x7fffffff, cnt = 0;
    for (int k = 0; k < K1; k++) {
        float bv = -INFINITY; int bi = -1;
#pragma unroll
        for (int u = 0; u < BSEL_LT; u++) {
            const int i = tid + BSEL_T * u;
            const float l = lv[u];
            if (l > -INFINITY && (l < pv || (l == pv && i < pi))) better(bv, bi, l, i);
        }
        for (int o = 32; o > 0; o >>= 1) better(bv, bi, __shfl_xor(bv, o), __shfl_xor(bi, o));
        __syncthreads();
        if ((tid & 63) == 0) { sm.f[tid >> 6] = bv; sm.i[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < BSEL_T / 64; w++) better(bv, bi, sm.f[w], sm.i[w]);
            sm.of = bv; sm.oi = bi;
            if (bi >= 0) { cand_tok[r * BK1 + k] = bi; cand_q[r * BK1 + k] = expf(bv - m) / se; }
        }
        __syncthreads();
        pv = sm.of; pi = sm.oi;
        if (pi < 0) break;   // the allowed set is exhausted (uniform: every thread reads the same slot)
        cnt++;
    }
    if (tid == 0) cand_n[r] = cnt;
}

void launch_beam_select(const float *logits, int V, DecodeState s, RuleTokens tk, int R, int ctx, int K1, int32_t *cand_tok,
                        float *cand_q, int32_t *cand_n, hipStream_t st) {
    hipLaunchKernelGGL(beam_select_kernel, dim3(R), dim3(BSEL_T), 0, st, logits, V, nh_logits_ld(V), s, tk, ctx, K1, cand_tok, cand_q, cand_n);
}

// One wave per clip.  Lane c < K (K+1) owns candidate c = (parent beam c / (K+1), its c % (K+1)-th best); the order is by rank
// counting (every lane counts who sorts before it), lane 0 walks the ordered list and makes the decisions, then all lanes
// move the token histories.  The histories of the clip's K rows are staged in LDS before any row is written: a parent may
// feed several children and a child may land on its parent's sibling.
__global__ __launch_bounds__(64) void beam_merge_kernel(DecodeState s, RuleTokens tk, int V, int B, int K, int ctx, int cap, int max_new,
                                                        int prompt_len, const int32_t *__restrict__ cand_tok,
                                                        const float *__restrict__ cand_q, const int32_t *__restrict__ cand_n,
                                                        BeamBufs bb) {
    extern __shared__ int32_t hist[];                 // [K][ctx]
    __shared__ double sc[BCAND];
    __shared__ int ctok[BCAND], cpar[BCAND], order[BCAND], nvalid;
    __shared__ int pn[NH_MAX_BEAMS], phl[NH_MAX_BEAMS], plts[NH_MAX_BEAMS], plive[NH_MAX_BEAMS];
    // the walk's verdicts: child slot j <- (parent beam, token, forced eot); finished record f <- (parent beam, token, forced)
    __shared__ int ch_par[NH_MAX_BEAMS], ch_tok[NH_MAX_BEAMS], n_child;
    __shared__ int fi_par[NH_MAX_BEAMS], fi_tok[NH_MAX_BEAMS], fi_forced[NH_MAX_BEAMS], fi_slot[NH_MAX_BEAMS], n_fin_new;
    __shared__ double ch_sc[NH_MAX_BEAMS], fi_sc[NH_MAX_BEAMS];
    const int b = blockIdx.x, lane = threadIdx.x, K1 = K + 1, NC = K * K1;
    if (lane < K) {
        const int r = lane * B + b;
        plive[lane] = s.done[r] == 0;
        pn[lane] = s.n_tokens[r]; phl[lane] = s.have_last[r]; plts[lane] = s.last_ts[r];
    }
    __syncthreads();
    bool any = false;
    for (int j = 0; j < K; j++) any = any || plive[j];
    if (!any) {   // a clip that is done (or left by the no-speech exit): nothing moves
        if (lane < K) bb.parent[lane * B + b] = -1;
        return;
    }
    for (int j = 0; j < K; j++) {
        if (!plive[j]) continue;
        const int32_t *t = s.tokens + (long)(j * B + b) * ctx;
        for (int i = lane; i < pn[j] && i < ctx; i += 64) hist[j * ctx + i] = t[i];
    }
    for (int c = lane; c < NC; c += 64) {
        const int j = c / K1, k = c % K1, r = j * B + b;
        const bool ok = plive[j] && k < cand_n[r] && cand_q[r * BK1 + k] > 0.f;   // q == 0: masked, no candidate
        cpar[c] = ok ? j : -1;
        ctok[c] = ok ? cand_tok[r * BK1 + k] : -1;
        sc[c] = ok ? s.sum_logprob[r] + log((double)cand_q[r * BK1 + k]) : 0.0;   // model.rs:364-365
    }
    if (lane == 0) nvalid = 0;
    __syncthreads();
    for (int c = lane; c < NC; c += 64) {
        if (cpar[c] < 0) continue;
        int rank = 0;
        for (int o = 0; o < NC; o++) {
            if (o == c || cpar[o] < 0) continue;
            // o sorts before c: greater score, then lower parent beam, then higher token id
            const bool before = sc[o] > sc[c] || (sc[o] == sc[c] && (cpar[o] < cpar[c] || (cpar[o] == cpar[c] && ctok[o] > ctok[c])));
            rank += before;
        }
        order[rank] = c;
        atomicAdd(&nvalid, 1);
    }
    __syncthreads();
    if (lane == 0) {
        int nf = bb.fin_count[b], nc = 0, nfn = 0;
        for (int q = 0; q < nvalid && nc < K; q++) {
            const int c = order[q], j = cpar[c], tok = ctok[c];
            int forced = 0;
            bool fin = tok == tk.eot;                                           // model.rs:317
            const int nn = pn[j] + 1;                                           // append_token's order (k_token.hip)
            if (nn >= cap) { fin = true; forced = 1; }                          // :367-370
            else if (!fin && max_new > 0 && nn - prompt_len >= max_new) { fin = true; forced = 1; }
            if (fin) {
                if (nf < K) { fi_par[nfn] = j; fi_tok[nfn] = tok; fi_forced[nfn] = forced; fi_sc[nfn] = sc[c]; fi_slot[nfn] = nf; nfn++; nf++; }
            } else { ch_par[nc] = j; ch_tok[nc] = tok; ch_sc[nc] = sc[c]; nc++; }
        }
        if (nf >= K) nc = 0;   // K finished: the clip is done, its live children are not kept
        if (nvalid == 0 && nf == 0) {
            // everything masked in every live row and nothing finished: the clip ends here.  Its best live prefix is left in
            // record 0 with the all-masked convention of the greedy step (last index, log-prob -inf); fin_count stays 0
            int bj = -1;
            for (int j = 0; j < K; j++)
                if (plive[j] && (bj < 0 || s.sum_logprob[j * B + b] > s.sum_logprob[bj * B + b])) bj = j;
            fi_par[0] = bj; fi_tok[0] = V - 1; fi_forced[0] = 0; fi_sc[0] = -INFINITY; fi_slot[0] = 0; nfn = 1;
        }
        n_child = nc; n_fin_new = nfn;
        bb.fin_count[b] = nf;
    }
    __syncthreads();
    // finished records: parent's tokens + token (+ the forced eot)
    for (int f = 0; f < n_fin_new; f++) {
        const int j = fi_par[f], n = pn[j];
        int32_t *ft = bb.fin_tokens + ((long)b * K + fi_slot[f]) * ctx;
        for (int i = lane; i < n; i += 64) ft[i] = hist[j * ctx + i];
        if (lane == 0) {
            int nn = n;
            ft[nn++] = fi_tok[f];
            if (fi_forced[f] && nn < ctx) ft[nn++] = tk.eot;
            bb.fin_n[b * K + fi_slot[f]] = nn;
            bb.fin_score[b * K + fi_slot[f]] = fi_sc[f];
        }
    }
    // the clip's rows: child slots first, the rest dead (their state stays as it is but the flag)
    for (int j = 0; j < K; j++) {
        const int r = j * B + b;
        if (j < n_child) {
            const int pj = ch_par[j], n = pn[pj], tok = ch_tok[j];
            int32_t *t = s.tokens + (long)r * ctx;
            for (int i = lane; i < n; i += 64) t[i] = hist[pj * ctx + i];
            if (lane == 0) {
                t[n] = tok;
                s.n_tokens[r] = n + 1;
                const bool is_ts = tok > tk.no_timestamps;                      // :359-361
                s.have_last[r] = is_ts ? 1 : phl[pj];
                s.last_ts[r] = is_ts ? tok : plts[pj];
                s.sum_logprob[r] = ch_sc[j];
                s.done[r] = 0;
                bb.parent[r] = pj * B + b;
            }
        } else if (lane == 0) {
            s.done[r] = 1;
            bb.parent[r] = -1;
        }
    }
}

void launch_beam_merge(DecodeState s, RuleTokens tk, int V, int B, int K, int ctx, int cap, int max_new, int prompt_len,
                       const int32_t *cand_tok, const float *cand_q, const int32_t *cand_n, BeamBufs bb, hipStream_t st) {
    hipLaunchKernelGGL(beam_merge_kernel, dim3(B), dim3(64), sizeof(int32_t) * (size_t)K * ctx, st, s, tk, V, B, K, ctx, cap, max_new,
                       prompt_len, cand_tok, cand_q, cand_n, bb);
}

// Self-attention caches, head-major [row][h][C][64] fp16.  A thread owns one 16-byte piece (position, eighth of a head row) of
// one (clip, head, layer, K or V) and moves it for all K rows of the clip: every source into registers first, then every
// destination.  No other thread touches that offset of those rows, so any parent map is safe -- swaps, chains, fan-out --
// with no scratch and no barrier.  Rows with parent[r] < 0 (dead) or == r stay; a parent outside the clip's rows is ignored.
__global__ __launch_bounds__(256) void beam_reorder_kernel(half_t *const *__restrict__ caches, const int32_t *__restrict__ parent,
                                                           int B, int K, int H, int C, int npos) {
    const int b = blockIdx.z % B, lk = blockIdx.z / B, h = blockIdx.y;
    const int p = blockIdx.x * 32 + (threadIdx.x >> 3), seg = threadIdx.x & 7;
    if (p >= npos) return;
    typedef unsigned v4u __attribute__((ext_vector_type(4)));   // 16 bytes, a plain vector type: the staging array stays in registers
    v4u *base = reinterpret_cast<v4u *>(caches[lk]);
    const long off = ((long)h * C + p) * 8 + seg;       // in 16-byte units inside a row
    const long row = (long)H * C * 8;
    v4u v[NH_MAX_BEAMS];
    bool mv[NH_MAX_BEAMS];
#pragma unroll
    for (int j = 0; j < NH_MAX_BEAMS; j++) {
        const int r = j * B + b;
        int q = j < K ? parent[r] : -1;
        mv[j] = !(q < 0 || q == r || q % B != b || q / B >= K);
        v[j] = base[(mv[j] ? q : b) * row + off];       // unconditional (row b is the clip's own): the loads go out together
    }
#pragma unroll
    for (int j = 0; j < NH_MAX_BEAMS; j++) if (mv[j]) base[(long)(j * B + b) * row + off] = v[j];
}

// caches: device table of 2 * layers pointers (sk, sv of every layer); npos live positions
void launch_beam_reorder(half_t *const *caches, int n_caches, const int32_t *parent, int B, int K, int H, int C, int npos,
                         hipStream_t st) {
    if (npos < 1) return;
    hipLaunchKernelGGL(beam_reorder_kernel, dim3((npos + 31) / 32, H, B * n_caches), dim3(256), 0, st, caches, parent, B, K, H, C, npos);
}
