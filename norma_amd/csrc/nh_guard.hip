// nh_guard.hip -- the C ABI of include/norma_hip.h, part 11: the repetition guard of the decode step.  The
// parameters and the per-row bias lists live here; the edit itself is k_guard.hip, launched by the step (emit_token_step of
// nh_decode.hip, the beam loop of nh_beam.hip) through emit_guard, and by the parity view nh_guard_apply.
#include "nh_ctx.h"

static GuardBufs guard_bufs(const nh_ctx *ctx, const int32_t *bias_map, int clips) {
    const GuardState &g = ctx->guard;
    return GuardBufs{g.bias_tok, g.bias_val, g.bias_n, bias_map, clips > 0 ? clips : 1, g.loop_exit};
}

void emit_guard(nh_ctx *ctx, int R, int prompt_len, const int32_t *pos, int clips) {
    launch_guard(ctx->logits, ctx->c.vocab_size, ctx->ds, ctx->tk, R, ctx->c.max_target_positions, prompt_len, pos, ctx->guard.spec,
                 guard_bufs(ctx, nullptr, clips), ctx->st, pos && ctx->pool.rows > 0 ? ctx->d_pfx : nullptr);
}

// the flags, and with want_bias the bias table: made once, zeroed.  A table that appears is something the captured steps
// took by value as a null pointer: the generation moves.
static int ensure_guard_buffers(nh_ctx *ctx, bool want_bias) {
    GuardState &g = ctx->guard;
    hipSetDevice(ctx->dev);
    if (!g.loop_exit) {
        if (int rc = g.flags.reserve(ctx, sizeof(int32_t) * (size_t)ctx->B, "guard flags", true)) return rc;
        g.loop_exit = g.flags.at<int32_t>();
        g.gen++;
    }
    if (want_bias && !g.bias_tok) {
        const size_t n = (size_t)ctx->B * NH_GUARD_MAX_BIAS;
        Carve cv;
        const size_t o_tok = cv.take(4 * n), o_val = cv.take(4 * n), o_n = cv.take(4 * (size_t)ctx->B), o_map = cv.take(4 * (size_t)ctx->B);
        if (int rc = g.table.reserve(ctx, cv.off, "guard bias table", true)) return rc;   // bias_n starts at zero
        g.bias_tok = g.table.at<int32_t>(o_tok); g.bias_val = g.table.at<float>(o_val);
        g.bias_n = g.table.at<int32_t>(o_n); g.bias_map = g.table.at<int32_t>(o_map);
        g.gen++;
    }
    return NH_OK;
}

extern "C" int nh_set_guard(nh_ctx *ctx, const nh_guard_params *p) {
    if (!ctx) return NH_ERR_INVALID;
    GuardSpec sp{0, 1.0f, 0, 0, 0};
    if (p) {
        if (!(p->repetition_penalty > 0.f) || p->repetition_penalty == INFINITY) return ctx->fail(NH_ERR_INVALID, "nh_set_guard: repetition_penalty must be finite and > 0 (1.0 is off)");
        if (p->no_repeat_ngram < 0 || p->no_repeat_ngram > 16) return ctx->fail(NH_ERR_INVALID, "nh_set_guard: no_repeat_ngram outside 0 .. 16");
        if (p->loop_period < 0 || p->loop_period > NH_GUARD_MAX_PERIOD) return ctx->fail(NH_ERR_INVALID, "nh_set_guard: loop_period outside 0 .. 64");
        if (p->loop_period > 0 && (p->loop_repeats < 2 || p->loop_repeats > 16 || p->loop_period * p->loop_repeats > 448))
            return ctx->fail(NH_ERR_INVALID, "nh_set_guard: loop_repeats outside 2 .. 16, or loop_period * loop_repeats > 448");
        if (p->loop_period == 0 && p->loop_repeats != 0 && (p->loop_repeats < 2 || p->loop_repeats > 16))
            return ctx->fail(NH_ERR_INVALID, "nh_set_guard: loop_repeats outside 2 .. 16");
        sp = GuardSpec{p->no_repeat_ngram, p->repetition_penalty, p->loop_period, p->loop_period > 0 ? p->loop_repeats : 0, p->bias != 0 ? 1 : 0};
    }
    for (const PoolRow &r : ctx->pool.row)
        if (r.busy) return ctx->fail(NH_ERR_STATE, "nh_set_guard: rows are busy (the captured steps carry whether the guard is in them)");
    const bool on = sp.ngram > 0 || sp.penalty != 1.0f || sp.loop_period > 0 || sp.bias != 0;
    if (on) {
        if (ctx->c.max_target_positions > NH_GUARD_MAX_HISTORY) return ctx->fail(NH_ERR_STATE, "nh_set_guard: max_target_positions above 512");
        if (int rc = ensure_guard_buffers(ctx, sp.bias != 0)) return rc;
    }
    GuardState &g = ctx->guard;
    const GuardSpec &o = g.spec;
    if (on != g.on || sp.ngram != o.ngram || sp.penalty != o.penalty || sp.loop_period != o.loop_period || sp.loop_repeats != o.loop_repeats || sp.bias != o.bias) g.gen++;
    g.spec = sp; g.on = on;
    return NH_OK;
}

extern "C" int nh_guard_bias(nh_ctx *ctx, int row, const int32_t *tokens, const float *bias, int n) {
    if (!ctx) return NH_ERR_INVALID;
    if (row < 0 || row >= ctx->B) return ctx->fail(NH_ERR_INVALID, "nh_guard_bias: row outside [0, max_batch)");
    if (n < 0 || n > NH_GUARD_MAX_BIAS) return ctx->fail(NH_ERR_INVALID, "nh_guard_bias: n outside 0 .. NH_GUARD_MAX_BIAS = 256");
    if (n > 0 && (!tokens || !bias)) return ctx->fail(NH_ERR_INVALID, "nh_guard_bias: bad arguments");
    std::vector<int32_t> sorted(tokens, tokens + n);
    std::sort(sorted.begin(), sorted.end());
    for (int i = 0; i < n; i++) {
        if (tokens[i] < 0 || tokens[i] >= ctx->c.vocab_size) return ctx->fail(NH_ERR_INVALID, "nh_guard_bias: token id outside the vocabulary");
        if (i > 0 && sorted[i] == sorted[i - 1]) return ctx->fail(NH_ERR_INVALID, "nh_guard_bias: a token id appears twice");
        if (bias[i] != bias[i] || bias[i] == INFINITY) return ctx->fail(NH_ERR_INVALID, "nh_guard_bias: a bias is NaN or +inf (finite or -inf)");
    }
    GuardState &g = ctx->guard;
    if (n == 0 && !g.bias_tok) return NH_OK;   // nothing to clear, nothing allocated
    // a table that appears moves the graph key; steps captured with the bias enabled already hold it (nh_set_guard made it)
    if (!g.bias_tok)
        if (int rc = ensure_guard_buffers(ctx, true)) return rc;
    hipSetDevice(ctx->dev);
    const int32_t cnt = n;
    if (n > 0) {
        HIPCHK(hipMemcpyAsync(g.bias_tok + (size_t)row * NH_GUARD_MAX_BIAS, tokens, sizeof(int32_t) * n, hipMemcpyHostToDevice, ctx->st));
        HIPCHK(hipMemcpyAsync(g.bias_val + (size_t)row * NH_GUARD_MAX_BIAS, bias, sizeof(float) * n, hipMemcpyHostToDevice, ctx->st));
    }
    HIPCHK(hipMemcpyAsync(g.bias_n + row, &cnt, sizeof(int32_t), hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));   // the caller's buffers and cnt
    return NH_OK;
}

extern "C" int nh_guard_report(nh_ctx *ctx, const int32_t *rows, int n, int32_t *loop_exit) {
    if (!ctx || !loop_exit || n < 1) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_guard_report: bad arguments") : NH_ERR_INVALID;
    const bool pool = ctx->pool.rows > 0;
    const int lim = pool ? ctx->pool.rows : ctx->cur_batch;
    if (!pool && ctx->guard.after_beam) return ctx->fail(NH_ERR_STATE, "nh_guard_report: the last decode was a beam search (the flag does not travel with a hypothesis)");
    if (!rows && n > lim) return ctx->fail(NH_ERR_INVALID, "nh_guard_report: more rows than the batch (or the pool) has");
    for (int i = 0; rows && i < n; i++)
        if (rows[i] < 0 || rows[i] >= lim) return ctx->fail(NH_ERR_INVALID, "nh_guard_report: row outside the batch (or the pool)");
    if (!ctx->guard.loop_exit) {   // no guard was ever on: no row ever took the exit
        for (int i = 0; i < n; i++) loop_exit[i] = 0;
        return NH_OK;
    }
    hipSetDevice(ctx->dev);
    std::vector<int32_t> all(lim);
    HIPCHK(hipMemcpyAsync(all.data(), ctx->guard.loop_exit, sizeof(int32_t) * lim, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    for (int i = 0; i < n; i++) loop_exit[i] = all[rows ? rows[i] : i];
    return NH_OK;
}

extern "C" int nh_guard_apply(nh_ctx *ctx, int rows, const float *logits, const int32_t *tokens, const int32_t *n_tokens, int64_t stride,
                              int prompt_len, const int32_t *active, const int32_t *bias_rows, float *logits_out, int32_t *loop_exit) {
    if (!ctx || !logits || !tokens || !n_tokens || !logits_out || !loop_exit) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_guard_apply: bad arguments") : NH_ERR_INVALID;
    const int C = ctx->c.max_target_positions, V = ctx->c.vocab_size, ld = ctx->VP;
    if (rows < 1 || rows > ctx->B) return ctx->fail(NH_ERR_INVALID, "nh_guard_apply: rows outside 1 .. max_batch");
    if (prompt_len < 1 || stride < 1) return ctx->fail(NH_ERR_INVALID, "nh_guard_apply: prompt_len or stride < 1");
    if (!ctx->have_tokens) return ctx->fail(NH_ERR_STATE, "nh_guard_apply: call nh_set_tokens first");
    if (ctx->pool.rows > 0) return ctx->fail(NH_ERR_STATE, "nh_guard_apply: the context runs a decode pool (nh_pool_begin)");
    if (C > NH_GUARD_MAX_HISTORY) return ctx->fail(NH_ERR_STATE, "nh_guard_apply: max_target_positions above 512");
    std::vector<int32_t> toks((size_t)rows * C, 0), nt(rows), done(rows), hl(rows, 0), map(rows, -1);
    for (int r = 0; r < rows; r++) {
        const int n = n_tokens[r];
        if (n < prompt_len || n > C - 2 || n > stride) return ctx->fail(NH_ERR_INVALID, "nh_guard_apply: n_tokens outside prompt_len .. min(stride, max_target_positions - 2)");
        for (int i = 0; i < n; i++) {
            const int32_t t = tokens[(size_t)r * stride + i];
            if (t < 0 || t >= V) return ctx->fail(NH_ERR_INVALID, "nh_guard_apply: token id outside the vocabulary");
            toks[(size_t)r * C + i] = t;
            if (i >= prompt_len && t > ctx->tk.no_timestamps) hl[r] = 1;   // what a decode's have_last is: a timestamp was generated
        }
        nt[r] = n; done[r] = (active && !active[r]) ? 1 : 0;
        if (bias_rows) {
            if (bias_rows[r] >= ctx->B) return ctx->fail(NH_ERR_INVALID, "nh_guard_apply: bias row outside [0, max_batch)");
            map[r] = bias_rows[r];
        }
    }
    if (int rc = ensure_guard_buffers(ctx, true)) return rc;
    GuardState &g = ctx->guard;
    ctx->live.lock_valid = false; ctx->beam.valid = false;   // the token rows and the logits are the view's now
    // the pad columns V .. ld-1 of every row hold NaN: the edit must neither read nor write them
    HIPCHK(hipMemsetAsync(ctx->logits, 0xff, sizeof(float) * (size_t)rows * ld, ctx->st));
    HIPCHK(hipMemcpy2DAsync(ctx->logits, sizeof(float) * ld, logits, sizeof(float) * V, sizeof(float) * V, rows, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(ctx->ds.tokens, toks.data(), toks.size() * 4, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(ctx->ds.n_tokens, nt.data(), 4 * rows, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(ctx->ds.done, done.data(), 4 * rows, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(ctx->ds.have_last, hl.data(), 4 * rows, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(g.bias_map, map.data(), 4 * rows, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemsetAsync(g.loop_exit, 0, 4 * rows, ctx->st));
    launch_guard(ctx->logits, V, ctx->ds, ctx->tk, rows, C, prompt_len, nullptr, g.spec, guard_bufs(ctx, g.bias_map, 1), ctx->st);
    HIPCHK(hipMemcpyAsync(logits_out, ctx->logits, sizeof(float) * (size_t)rows * ld, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(loop_exit, g.loop_exit, 4 * rows, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipGetLastError());
    return NH_OK;
}
