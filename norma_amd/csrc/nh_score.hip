// nh_score.hip -- the C ABI of include/norma_hip.h, part 10: transcript scoring.  nh_score runs the positions
// of given sequences through the one-pass forward of nh_prefill.hip, keeps the final LayerNorm's fp16 rows on the device and
// hands them to the two kernels of k_score.hip: the vocabulary projection reduced to three numbers per row, and their merge.
#include "nh_ctx.h"

// the score buffers, made by the first call
static int ensure_score_buffers(nh_ctx *ctx) {
    ScoreState &sc = ctx->score;
    if (sc.buf.p) return NH_OK;
    const size_t C = ctx->c.max_target_positions, rows = (size_t)ctx->B * (C - 1), V = ctx->c.vocab_size;
    const size_t panel = std::min(rows, (size_t)score_panel_rows((int)V)), ntn = (V + 127) / 128;
    Carve cv;
    const size_t o_tg = cv.take(rows * 4), o_tl = cv.take(rows * 4), o_out = cv.take((size_t)ctx->B * C * 4), o_part = cv.take(panel * ntn * 8);
    if (int rc = sc.buf.reserve(ctx, cv.off, "transcript scoring")) return rc;
    char *p = static_cast<char *>(sc.buf.p);
    sc.target = reinterpret_cast<int32_t *>(p + o_tg);
    sc.tlogit = reinterpret_cast<float *>(p + o_tl);
    sc.out = reinterpret_cast<float *>(p + o_out);
    sc.part = reinterpret_cast<float *>(p + o_part);
    return NH_OK;
}

extern "C" int nh_score(nh_ctx *ctx, const int32_t *tokens, const int32_t *n_tokens, int prompt_len, float *out_logprob) {
    if (!ctx || !tokens || !n_tokens || !out_logprob) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_score: bad arguments") : NH_ERR_INVALID;
    if (ctx->pool.rows > 0) return ctx->fail(NH_ERR_STATE, "nh_score: the context runs a decode pool (nh_pool_begin)");
    if (!ctx->have_enc) return ctx->fail(NH_ERR_STATE, "nh_score: call nh_encode first");
    if (!prefill_supported(ctx)) return ctx->fail(NH_ERR_STATE, "nh_score: needs d_model % 128 == 0 and NH_OPT_ABSORBED_XATTN == 0");
    const int B = ctx->cur_batch, C = ctx->c.max_target_positions, V = ctx->c.vocab_size, d = ctx->c.d_model;
    if (prompt_len < 1) return ctx->fail(NH_ERR_INVALID, "nh_score: prompt_len < 1");
    int T = 0;   // positions 0 .. T - 1 of every clip go through the forward
    for (int b = 0; b < B; b++) {
        const int n = n_tokens[b];
        if (n <= prompt_len || n > C) return ctx->fail(NH_ERR_INVALID, "nh_score: n_tokens outside (prompt_len, max_target_positions]");
        T = std::max(T, n - 1);
    }
    // what lies past a clip's own tokens never reaches the device: positions n .. hold 0, and rows n - 1 .. have no target
    if (int rc = stage_given_tokens(ctx, "nh_score", tokens, C, 0, n_tokens)) return rc;
    if (int rc = ensure_score_buffers(ctx)) return rc;
    ScoreState &sc = ctx->score;
    std::vector<int32_t> target((size_t)B * T, -1);
    for (int b = 0; b < B; b++)
        for (int i = prompt_len; i < n_tokens[b]; i++) target[(size_t)b * T + i - 1] = tokens[(size_t)b * C + i];   // row i - 1 predicts token i
    HIPCHK(hipMemcpyAsync(sc.target, target.data(), target.size() * 4, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemsetAsync(sc.out, 0, sizeof(float) * (size_t)B * C, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));   // target is a local
    if (int rc = prefill_forward(ctx, T, nullptr, true)) return rc;
    if (!launch_score_rows(ctx->xn, B * T, d, ctx->mdl->tok_emb, V, sc.target, sc.part, sc.tlogit, T, C, 1, sc.out, 0, ctx->st))
        return ctx->fail(NH_ERR_INVALID, "nh_score: shape not covered");
    std::vector<float> out((size_t)B * C);
    HIPCHK(hipMemcpyAsync(out.data(), sc.out, out.size() * 4, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipGetLastError());
    memcpy(out_logprob, out.data(), out.size() * 4);
    return NH_OK;
}
