// nh_beam.hip -- the C ABI of include/norma_hip.h, part 9: beam search.  nh_decode_beam runs the prompt phase
// of every lockstep decode on the B clip rows, spreads each clip over K rows of the context (beam-major: hypothesis j of clip
// b in row j * B + b) and steps them with the decode step the greedy decode uses, at K * B rows; what follows the logits of
// a step -- candidates, merge, reordering of hypothesis state and self-attention caches -- is k_beam.hip.
#include "nh_ctx.h"

// the beam buffers, made by the first call that needs them
static int ensure_beam_buffers(nh_ctx *ctx) {
    BeamState &bs = ctx->beam;
    if (bs.buf.p) return NH_OK;
    const size_t MB = ctx->B, C = ctx->c.max_target_positions, K1 = NH_MAX_BEAMS + 1, NL = ctx->kv.size();
    Carve cv;
    const size_t o_par = cv.take(MB * 4), o_ft = cv.take(MB * C * 4), o_fn = cv.take(MB * 4), o_fs = cv.take(MB * 8), o_fc = cv.take(MB * 4);
    const size_t o_ct = cv.take(MB * K1 * 4), o_cq = cv.take(MB * K1 * 4), o_cn = cv.take(MB * 4), o_tab = cv.take(2 * NL * sizeof(half_t *));
    if (int rc = bs.buf.reserve(ctx, cv.off, "beam search")) return rc;
    char *p = static_cast<char *>(bs.buf.p);
    bs.bb.parent = reinterpret_cast<int32_t *>(p + o_par);
    bs.bb.fin_tokens = reinterpret_cast<int32_t *>(p + o_ft);
    bs.bb.fin_n = reinterpret_cast<int32_t *>(p + o_fn);
    bs.bb.fin_score = reinterpret_cast<double *>(p + o_fs);
    bs.bb.fin_count = reinterpret_cast<int32_t *>(p + o_fc);
    bs.cand_tok = reinterpret_cast<int32_t *>(p + o_ct);
    bs.cand_q = reinterpret_cast<float *>(p + o_cq);
    bs.cand_n = reinterpret_cast<int32_t *>(p + o_cn);
    bs.caches = reinterpret_cast<half_t **>(p + o_tab);
    std::vector<half_t *> tab;
    for (const KvCache &kv : ctx->kv) { tab.push_back(kv.sk); tab.push_back(kv.sv); }
    HIPCHK(hipMemsetAsync(bs.buf.p, 0, cv.off, ctx->st));
    HIPCHK(hipMemcpyAsync(bs.caches, tab.data(), tab.size() * sizeof(half_t *), hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));   // tab is a local
    return NH_OK;
}

// what follows the logits of a step: candidates per row, the merge per clip (hypothesis state moves here)
static void emit_beam_select_merge(nh_ctx *ctx, int B, int K, int max_new, int prompt_len) {
    const BeamState &bs = ctx->beam;
    const int C = ctx->c.max_target_positions, V = ctx->c.vocab_size;
    launch_beam_select(ctx->logits, V, ctx->ds, ctx->tk, B * K, C, K + 1, bs.cand_tok, bs.cand_q, bs.cand_n, ctx->st);
    launch_beam_merge(ctx->ds, ctx->tk, V, B, K, C, C - 1, max_new, prompt_len, bs.cand_tok, bs.cand_q, bs.cand_n, bs.bb, ctx->st);
}

static void emit_beam_reorder(nh_ctx *ctx, int B, int K, int npos) {
    launch_beam_reorder(ctx->beam.caches, 2 * (int)ctx->kv.size(), ctx->beam.bb.parent, B, K, ctx->c.decoder_attention_heads,
                        ctx->c.max_target_positions, npos, ctx->st);
}

// decoder_step takes its row count from the context's batch: K * B while the beams step, B again whatever way the call ends
struct BatchRows {
    nh_ctx *ctx; int B;
    BatchRows(nh_ctx *c, int rows) : ctx(c), B(c->cur_batch) { c->cur_batch = rows; }
    ~BatchRows() { ctx->cur_batch = B; }
};

extern "C" int nh_decode_beam(nh_ctx *ctx, int beam_size, int32_t *out_tokens, nh_decode_result *results, int max_new_tokens) {
    if (!ctx || !out_tokens || !results) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_decode_beam: bad arguments") : NH_ERR_INVALID;
    if (beam_size < 1 || beam_size > NH_MAX_BEAMS) return ctx->fail(NH_ERR_INVALID, "nh_decode_beam: beam_size must lie in [1, NH_MAX_BEAMS = 8]");
    if (int rc = decode_refusals(ctx)) return rc;
    if (ctx->opt_absorbed) return ctx->fail(NH_ERR_STATE, "nh_decode_beam: the NH_OPT_ABSORBED_XATTN prototype reads the encoder output of the clip rows only");
    const int K = beam_size, B = ctx->cur_batch, R = K * B;
    if (R > ctx->B)
        return ctx->fail(NH_ERR_INVALID, "nh_decode_beam: batch " + std::to_string(B) + " x beam_size " + std::to_string(K) + " = " +
                                             std::to_string(R) + " rows exceed max_batch " + std::to_string(ctx->B));
    hipSetDevice(ctx->dev);
    if (int rc = ensure_beam_buffers(ctx)) return rc;
    BeamState &bs = ctx->beam;
    bs.valid = false;
    DecodePrompt dp{};
    if (int rc = decode_prompt_phase(ctx, max_new_tokens, dp)) return rc;
    const int C = ctx->c.max_target_positions, cap = C - 1, NP = dp.NP, PL = dp.PL;
    int steps = dp.steps;
    // beams 1 .. K-1 of every clip start dead; their cross K/V are the clip's own, copied once (as pool_admit_impl copies them)
    HIPCHK(hipMemsetAsync(bs.bb.fin_count, 0, sizeof(int32_t) * B, ctx->st));
    HIPCHK(hipMemsetAsync(bs.bb.parent, 0xff, sizeof(int32_t) * R, ctx->st));
    if (K > 1) {
        for (int r = B; r < R; r++) ctx->h_done[128 + r] = 1;
        HIPCHK(hipMemcpyAsync(ctx->ds.done + B, ctx->h_done + 128 + B, sizeof(int32_t) * (R - B), hipMemcpyHostToDevice, ctx->st));
        HIPCHK(hipMemsetAsync(ctx->ds.n_tokens + B, 0, sizeof(int32_t) * (R - B), ctx->st));
        HIPCHK(hipMemsetAsync(ctx->ds.have_last + B, 0, sizeof(int32_t) * (R - B), ctx->st));
        HIPCHK(hipMemsetAsync(ctx->ds.last_ts + B, 0, sizeof(int32_t) * (R - B), ctx->st));
        HIPCHK(hipMemsetAsync(ctx->ds.sum_logprob + B, 0, sizeof(double) * (R - B), ctx->st));
        const size_t per = (size_t)ctx->S * ctx->c.d_model * B;   // cross K / V of the B clips in one layer, head-major [row][h][S][64]
        for (KvCache &L : ctx->kv)
            for (int j = 1; j < K; j++) {
                HIPCHK(hipMemcpyAsync(L.ck + per * j, L.ck, per * sizeof(half_t), hipMemcpyDeviceToDevice, ctx->st));
                HIPCHK(hipMemcpyAsync(L.cv + per * j, L.cv, per * sizeof(half_t), hipMemcpyDeviceToDevice, ctx->st));
            }
    }
    {
        BatchRows rows(ctx, R);
        // positions PL-1 .. cap-2, eagerly; the length cap ends every live hypothesis at the last one at the latest.  The host
        // looks at the done flags every 16 steps (and after the last one), as the greedy decode does.
        const int first_pos = PL - 1;
        for (int pos = first_pos; pos <= cap - 2; pos++) {
            decoder_step(ctx, pos, nullptr, false, true, nullptr);
            logits_from_dx(ctx, R);
            if (ctx->guard.on) emit_guard(ctx, R, PL, nullptr, B);   // hypothesis row j * B + b: clip b's bias list
            emit_beam_select_merge(ctx, B, K, max_new_tokens, PL);
            if (K > 1) emit_beam_reorder(ctx, B, K, pos + 1);
            steps++;
            if (((pos + 1 - first_pos) & 15) == 0 || pos == cap - 2) {
                HIPCHK(hipMemcpyAsync(ctx->h_done, ctx->ds.done, R * 4, hipMemcpyDeviceToHost, ctx->st));
                HIPCHK(hipStreamSynchronize(ctx->st));
                bool all = true;
                for (int r = 0; r < R; r++) all = all && ctx->h_done[r] != 0;
                if (all) break;
            }
        }
    }
    HIPCHK(hipEventRecord(ctx->ev[6], ctx->st));
    HIPCHK(hipGetLastError());
    // results: the clip rows' probe and exit, the finished records
    HostDecodeState h;
    bs.fin_tokens.assign((size_t)B * K * C, 0); bs.fin_n.assign((size_t)B * K, 0); bs.fin_score.assign((size_t)B * K, 0.0); bs.fin_count.assign(B, 0);
    if (int rc = queue_decode_state(ctx, nullptr, B, B, h)) return rc;
    HIPCHK(hipMemcpyAsync(bs.fin_tokens.data(), bs.bb.fin_tokens, bs.fin_tokens.size() * 4, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(bs.fin_n.data(), bs.bb.fin_n, bs.fin_n.size() * 4, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(bs.fin_score.data(), bs.bb.fin_score, bs.fin_score.size() * 8, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(bs.fin_count.data(), bs.bb.fin_count, B * 4, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    std::vector<int32_t> win(C);
    for (int b = 0; b < B; b++) {
        if (h.done[b] == 2) {   // the no-speech exit: what the greedy decode returns
            finish_sequence(ctx, h.toks.data() + (size_t)b * C, h.nt[b], 2, h.slp[b], h.nsp[b], out_tokens + (size_t)b * C, results[b], NP);
            continue;
        }
        // the finished hypothesis with the greatest sum_logprob / n (model.rs:373: prompt and eot count, a prefix does not),
        // the earliest on ties; none finished: record 0 holds the clip's dead end (beam_merge_kernel)
        int best = 0;
        for (int f = 1; f < bs.fin_count[b]; f++) {
            const double a = bs.fin_score[b * K + f] / (double)(bs.fin_n[b * K + f] - NP), c = bs.fin_score[b * K + best] / (double)(bs.fin_n[b * K + best] - NP);
            if (a > c) best = f;
        }
        memcpy(win.data(), bs.fin_tokens.data() + ((size_t)b * K + best) * C, sizeof(int32_t) * C);   // the trim works in place
        finish_sequence(ctx, win.data(), bs.fin_n[b * K + best], 1, bs.fin_score[b * K + best], h.nsp[b], out_tokens + (size_t)b * C, results[b], NP);
    }
    bs.valid = true; bs.B = B; bs.K = K; bs.skip = NP;
    ctx->guard.after_beam = true;   // the loop-exit flag does not travel with a hypothesis (nh_guard_report)
    ctx->tm.decode_steps = steps;
    ctx->live.lock_valid = false; ctx->live.P = dp.P;   // the kept queries are not reordered with their hypotheses: nh_align_decoded refuses
    return NH_OK;
}

extern "C" int nh_beam_hypotheses(nh_ctx *ctx, int b, int32_t *tokens, int32_t *n_tokens, double *sum_logprob, int32_t *n_finished) {
    if (!ctx || !tokens || !n_tokens || !sum_logprob || !n_finished) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_beam_hypotheses: bad arguments") : NH_ERR_INVALID;
    const BeamState &bs = ctx->beam;
    if (!bs.valid) return ctx->fail(NH_ERR_STATE, "nh_beam_hypotheses: no beam decode to report on (nh_decode_beam)");
    if (b < 0 || b >= bs.B) return ctx->fail(NH_ERR_INVALID, "nh_beam_hypotheses: clip outside the batch of the last beam decode");
    const int C = ctx->c.max_target_positions, K = bs.K, skip = bs.skip;
    *n_finished = bs.fin_count[b];
    for (int f = 0; f < K; f++) {
        int32_t *t = tokens + (size_t)f * C;
        memset(t, 0, sizeof(int32_t) * C);
        n_tokens[f] = 0; sum_logprob[f] = 0.0;
        if (f >= bs.fin_count[b]) continue;
        const int n = bs.fin_n[b * K + f] - skip;
        memcpy(t, bs.fin_tokens.data() + ((size_t)b * K + f) * C + skip, sizeof(int32_t) * n);
        n_tokens[f] = n; sum_logprob[f] = bs.fin_score[b * K + f];
    }
    return NH_OK;
}

extern "C" int nh_beam_step(nh_ctx *ctx, int beam_size, int batch, const float *logits, int32_t *tokens, int32_t *n_tokens,
                            int32_t *have_last, int32_t *last_ts, int32_t *live, double *score, int max_new_tokens, int prompt_len,
                            int32_t *parent, int32_t *n_finished, int32_t *fin_tokens, int32_t *fin_n, double *fin_score) {
    if (!ctx || !logits || !tokens || !n_tokens || !have_last || !last_ts || !live || !score || !parent || !n_finished || !fin_tokens ||
        !fin_n || !fin_score)
        return ctx ? ctx->fail(NH_ERR_INVALID, "nh_beam_step: bad arguments") : NH_ERR_INVALID;
    const int K = beam_size, B = batch, R = K * B, C = ctx->c.max_target_positions, V = ctx->c.vocab_size;
    if (K < 1 || K > NH_MAX_BEAMS || B < 1 || R > ctx->B) return ctx->fail(NH_ERR_INVALID, "nh_beam_step: beam_size in [1, 8], batch >= 1, batch * beam_size <= max_batch");
    if (!ctx->have_tokens) return ctx->fail(NH_ERR_STATE, "nh_beam_step: call nh_set_tokens first");
    if (ctx->pool.rows > 0) return ctx->fail(NH_ERR_STATE, "nh_beam_step: the context runs a decode pool (nh_pool_begin)");
    for (int r = 0; r < R; r++) {
        if (!live[r]) continue;
        if (n_tokens[r] < 1 || n_tokens[r] > C - 2) return ctx->fail(NH_ERR_INVALID, "nh_beam_step: a live row holds 1 .. max_target_positions - 2 tokens");
        for (int i = 0; i < n_tokens[r]; i++)
            if (tokens[(size_t)r * C + i] < 0 || tokens[(size_t)r * C + i] >= V) return ctx->fail(NH_ERR_INVALID, "nh_beam_step: token id outside the vocabulary");
    }
    for (int b = 0; b < B; b++)
        if (n_finished[b] < 0 || n_finished[b] > K) return ctx->fail(NH_ERR_INVALID, "nh_beam_step: n_finished outside 0 .. beam_size");
    hipSetDevice(ctx->dev);
    if (int rc = ensure_beam_buffers(ctx)) return rc;
    BeamState &bs = ctx->beam;
    bs.valid = false; ctx->live.lock_valid = false;
    std::vector<int32_t> done(R);
    for (int r = 0; r < R; r++) done[r] = live[r] ? 0 : 1;
    // the pad columns V .. ld-1 of every row hold NaN: the selection must never read them
    HIPCHK(hipMemsetAsync(ctx->logits, 0xff, sizeof(float) * (size_t)R * ctx->VP, ctx->st));
    HIPCHK(hipMemcpy2DAsync(ctx->logits, sizeof(float) * ctx->VP, logits, sizeof(float) * V, sizeof(float) * V, R, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(ctx->ds.tokens, tokens, sizeof(int32_t) * (size_t)R * C, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(ctx->ds.n_tokens, n_tokens, 4 * R, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(ctx->ds.have_last, have_last, 4 * R, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(ctx->ds.last_ts, last_ts, 4 * R, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(ctx->ds.done, done.data(), 4 * R, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(ctx->ds.sum_logprob, score, 8 * R, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(bs.bb.fin_count, n_finished, 4 * B, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemsetAsync(bs.bb.fin_tokens, 0, sizeof(int32_t) * (size_t)R * C, ctx->st));
    HIPCHK(hipMemsetAsync(bs.bb.fin_n, 0, 4 * R, ctx->st));
    HIPCHK(hipMemsetAsync(bs.bb.fin_score, 0, 8 * R, ctx->st));
    emit_beam_select_merge(ctx, B, K, max_new_tokens, prompt_len);
    HIPCHK(hipMemcpyAsync(tokens, ctx->ds.tokens, sizeof(int32_t) * (size_t)R * C, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(n_tokens, ctx->ds.n_tokens, 4 * R, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(have_last, ctx->ds.have_last, 4 * R, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(last_ts, ctx->ds.last_ts, 4 * R, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(done.data(), ctx->ds.done, 4 * R, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(score, ctx->ds.sum_logprob, 8 * R, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(parent, bs.bb.parent, 4 * R, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(n_finished, bs.bb.fin_count, 4 * B, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(fin_tokens, bs.bb.fin_tokens, sizeof(int32_t) * (size_t)R * C, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(fin_n, bs.bb.fin_n, 4 * R, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(fin_score, bs.bb.fin_score, 8 * R, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipGetLastError());
    for (int r = 0; r < R; r++) live[r] = done[r] == 0;
    return NH_OK;
}

extern "C" int nh_beam_reorder(nh_ctx *ctx, int beam_size, int batch, const int32_t *parent, int n_pos, int layer, int which, uint16_t *cache) {
    if (!ctx || !parent || !cache) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_beam_reorder: bad arguments") : NH_ERR_INVALID;
    const int K = beam_size, B = batch, R = K * B, C = ctx->c.max_target_positions, d = ctx->c.d_model;
    if (K < 1 || K > NH_MAX_BEAMS || B < 1 || R > ctx->B) return ctx->fail(NH_ERR_INVALID, "nh_beam_reorder: beam_size in [1, 8], batch >= 1, batch * beam_size <= max_batch");
    if (n_pos < 0 || n_pos > C || layer < 0 || layer >= (int)ctx->kv.size() || which < 0 || which > 1) return ctx->fail(NH_ERR_INVALID, "nh_beam_reorder: n_pos, layer or which out of range");
    if (ctx->pool.rows > 0) return ctx->fail(NH_ERR_STATE, "nh_beam_reorder: the context runs a decode pool (nh_pool_begin)");
    hipSetDevice(ctx->dev);
    if (int rc = ensure_beam_buffers(ctx)) return rc;
    ctx->beam.valid = false; ctx->live.lock_valid = false;
    half_t *dst = which ? ctx->kv[layer].sv : ctx->kv[layer].sk;
    const size_t bytes = sizeof(half_t) * (size_t)R * C * d;
    HIPCHK(hipMemcpyAsync(dst, cache, bytes, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(ctx->beam.bb.parent, parent, 4 * R, hipMemcpyHostToDevice, ctx->st));
    emit_beam_reorder(ctx, B, K, n_pos);
    HIPCHK(hipMemcpyAsync(cache, dst, bytes, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipGetLastError());
    return NH_OK;
}
