// nh_align.hip -- the C ABI of include/norma_hip.h, part 4: token-level timestamps -- nh_align (a teacher-forced pass over
// given tokens), nh_align_capture / nh_align_decoded (the queries a decode kept), the views and nh_align_path.  It uses the
// decoder through decoder_step (nh_decode.hip) alone; the kernels are in k_align.hip.
#include "nh_ctx.h"

// ---- token-level timestamps (contract: include/norma_hip.h, nh_align; kernels: k_align.hip) ----------------------------------
static_assert(NH_ALIGN_HEADS == NH_ALIGN_MAX_HEADS, "nh_kernels.h and norma_hip.h disagree");
#define NH_ALIGN_BUDGET ((size_t)256 << 20)   // workspace of a call under NH_OPT_ALIGN_KEEP = 0

// (heads, n_heads) -> hs, once every entry names a head the decoder runs (NH_OPT_DECODER_LAYER_LIMIT counts); hs is written
// only on success.
static int align_head_set(nh_ctx *ctx, const char *who, const nh_align_head *heads, int n_heads, int min_heads, AlignHeadSet &hs) {
    const int A = n_heads, H = ctx->c.decoder_attention_heads, NL = ctx->dec_layer_limit > 0 ? ctx->dec_layer_limit : ctx->c.decoder_layers;
    if (A < min_heads || A > NH_ALIGN_MAX_HEADS)
        return ctx->fail(NH_ERR_INVALID, std::string(who) + ": n_heads outside " + std::to_string(min_heads) + " .. NH_ALIGN_MAX_HEADS");
    for (int a = 0; a < A; a++)
        if (heads[a].layer < 0 || heads[a].layer >= NL || heads[a].head < 0 || heads[a].head >= H)
            return ctx->fail(NH_ERR_INVALID, std::string(who) + ": alignment head " + std::to_string(a) + " names a layer or head the decoder does not run");
    hs.A = A;
    hs.layer.assign(A > 0 ? ctx->c.decoder_layers : 0, AlignLayerHeads{});
    for (int a = 0; a < A; a++) {
        hs.heads[a] = heads[a];
        AlignLayerHeads &lh = hs.layer[heads[a].layer];
        lh.slot[lh.n] = a; lh.head[lh.n] = heads[a].head; lh.n++;
    }
    return NH_OK;
}

// The context's query buffer, grown to hold A heads.  The captured decode steps hold its address by value: a buffer that
// moves makes them stale (StepKey::align_gen), and what a decode kept in the old one is gone.  A failure changes nothing.
static int align_q_buffer(nh_ctx *ctx, const char *who, int A) {
    if (A <= ctx->align_q_heads) return NH_OK;
    // reserve drains the stream first: a finished decode may still be copying into the buffer that goes
    DevBuf q;
    if (int rc = q.reserve(ctx, (size_t)A * (ctx->c.max_target_positions - 1) * ctx->B * NH_DH * sizeof(half_t), who)) return rc;
    ctx->align_q.swap(q);   // ... and the old one goes with q
    ctx->align_q_heads = A;
    ctx->live.gen++; ctx->live.lock_valid = false;
    return NH_OK;
}

// The workspace of a call over n clips with A heads, made again when the shape differs from what is held: the clips of a group
// share it; a group's size is the same for every call of the same heads, and no kernel mixes clips, so grouping never shows in
// the results.  `fixed` counts the query buffer of A heads.
static int align_prepare(nh_ctx *ctx, int A, int n) {
    AlignState &al = ctx->al;
    const size_t C = ctx->c.max_target_positions, NP = C - 1, S = ctx->S, B = ctx->B;
    const size_t fixed = (size_t)A * NP * B * NH_DH * sizeof(half_t) + (size_t)B * (2 * (C + 1) + 2) * sizeof(int32_t);
    const size_t per_clip = ((size_t)A * NP + 2 * A + C) * S * sizeof(float) + (size_t)C * S;
    if (ctx->pool.rows > 0) n = ctx->pool.rows;   // a pool's calls name 1 .. rows rows: sized once for all of them
    int group = n;
    if (!ctx->opt_align_keep) {
        const size_t room = NH_ALIGN_BUDGET > fixed ? NH_ALIGN_BUDGET - fixed : 0;
        group = (int)std::min<size_t>((size_t)n, std::max<size_t>(1, room / per_clip));
    }
    // kept whenever it is large enough: the rows a pool hands back differ from collect to collect.  Another shape carves the
    // buffer again, and only one that needs more than any before costs a stream synchronise and a new allocation.
    if (al.heads == A && al.group >= group && al.S == (int)S) return NH_OK;
    Carve cv;
    const size_t o_rows = cv.take(4 * B), o_keys = cv.take(4 * B), o_map = cv.take(4 * B);
    const size_t o_first = cv.take(4 * B * (C + 1)), o_last = cv.take(4 * B * (C + 1)), zeroed = cv.off;
    const size_t o_W = cv.take(sizeof(float) * group * A * NP * S), o_stats = cv.take(sizeof(float) * group * A * 2 * S);
    const size_t o_M = cv.take(sizeof(float) * group * C * S), o_trace = cv.take((size_t)group * C * S);
    al.heads = al.group = al.S = 0; al.kept = false;   // what the views showed is cut up differently from here on
    if (int rc = al.buf.reserve(ctx, cv.off, "alignment workspace"))
        return rc != NH_ERR_NOMEM ? rc : ctx->fail(rc, "nh_align: the workspace for " + std::to_string(group) + " clips x " + std::to_string(A) +
                                           " heads does not fit (NH_OPT_ALIGN_KEEP = 1 holds the whole batch)");
    HIPCHK(hipMemsetAsync(al.buf.p, 0, zeroed, ctx->st));   // the rows, keys, row map and paths start as zeros
    al.n_rows = al.buf.at<int32_t>(o_rows); al.n_keys = al.buf.at<int32_t>(o_keys); al.row_map = al.buf.at<int32_t>(o_map);
    al.first = al.buf.at<int32_t>(o_first); al.last = al.buf.at<int32_t>(o_last);
    al.W = al.buf.at<float>(o_W); al.stats = al.buf.at<float>(o_stats); al.M = al.buf.at<float>(o_M);
    al.trace = al.buf.at<uint8_t>(o_trace);
    al.heads = A; al.group = group; al.S = (int)S;
    return NH_OK;
}

// Stages 2 - 6 for the n clips whose rows and keys al.n_rows / al.n_keys hold, a group at a time, and the paths back to the
// host.  hp: the heads' queries in the context's buffer and their keys; row_map: device i32 [n] or nullptr.
static int align_stages(nh_ctx *ctx, const char *who, const AlignHeadPtrs &hp, int A, int P, int n, const int32_t *row_map,
                        int32_t *out_first, int32_t *out_last) {
    AlignState &al = ctx->al;
    const int C = ctx->c.max_target_positions, S = ctx->S, H = ctx->c.decoder_attention_heads, NP = C - 1, group = al.group;
    const long wcs = (long)A * NP * S, whs = (long)NP * S, mcs = (long)C * S;
    for (int c0 = 0; c0 < n; c0 += group) {
        const int nc = std::min(group, n - c0);
        bool ok = launch_align_weights(hp, A, (long)ctx->B * NH_DH, NH_DH, (long)H * S * NH_DH, al.n_rows, al.n_keys, NP, S, nc, c0, al.W, wcs, whs, S, row_map, ctx->st);
        ok = ok && launch_align_reduce(al.W, wcs, whs, S, al.n_rows, al.n_keys, NP, S, nc, c0, A, P, al.stats, al.M, mcs, S, row_map, ctx->st);
        ok = ok && launch_align_dtw(al.M, mcs, S, al.n_rows, al.n_keys, P, NP, S, nc, c0, al.trace, mcs, al.first, al.last, C + 1, row_map, ctx->st);
        if (!ok) return ctx->fail(NH_ERR_INVALID, std::string(who) + ": the alignment kernels do not cover this model's shape (S <= 1536, max_target_positions <= 512)");
    }
    std::vector<int32_t> fl((size_t)2 * n * (C + 1));
    HIPCHK(hipMemcpyAsync(fl.data(), al.first, (size_t)n * (C + 1) * 4, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(fl.data() + (size_t)n * (C + 1), al.last, (size_t)n * (C + 1) * 4, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipGetLastError());
    for (int b = 0; b < n; b++) {
        memcpy(out_first + (size_t)b * C, fl.data() + (size_t)b * (C + 1), sizeof(int32_t) * C);
        memcpy(out_last + (size_t)b * C, fl.data() + (size_t)(n + b) * (C + 1), sizeof(int32_t) * C);
    }
    return NH_OK;
}

// What nh_align and nh_align_decoded share once the queries of hs are in the context's buffer: n clips of n_tokens[i] tokens
// (0: nothing to align) over keys[i] keys, clip i in context row row_map[i] (host i32 [n]; nullptr: in row i).
static int align_run(nh_ctx *ctx, const char *who, const AlignHeadSet &hs, int P, int n, const std::vector<int32_t> &n_tokens,
                     const std::vector<int32_t> &keys, const int32_t *row_map, int32_t *out_first, int32_t *out_last) {
    const size_t NP = ctx->c.max_target_positions - 1, S = ctx->S;
    if (int rc = align_prepare(ctx, hs.A, n)) return rc;
    AlignState &al = ctx->al;
    al.kept = false;
    AlignHeadPtrs hp{};
    for (int a = 0; a < hs.A; a++) {
        hp.q[a] = ctx->align_q.at<half_t>() + (size_t)a * NP * ctx->B * NH_DH;
        hp.k[a] = ctx->kv[hs.heads[a].layer].ck + (size_t)hs.heads[a].head * S * NH_DH;
    }
    std::vector<int32_t> rows(n);
    for (int i = 0; i < n; i++) rows[i] = n_tokens[i] > 0 ? n_tokens[i] - 1 : 0;
    HIPCHK(hipMemcpyAsync(al.n_rows, rows.data(), n * 4, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(al.n_keys, keys.data(), n * 4, hipMemcpyHostToDevice, ctx->st));
    if (row_map) HIPCHK(hipMemcpyAsync(al.row_map, row_map, n * 4, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));   // host buffers of this frame and of the caller's
    if (int rc = align_stages(ctx, who, hp, hs.A, P, n, row_map ? al.row_map : nullptr, out_first, out_last)) return rc;
    al.kept = ctx->opt_align_keep; al.P = P; al.A = hs.A;
    al.n_tokens = n_tokens; al.keys = keys;
    return NH_OK;
}

extern "C" int nh_align(nh_ctx *ctx, const int32_t *tokens, const int32_t *n_tokens, int prompt_len, const nh_align_head *heads,
                        int n_heads, const int32_t *n_keys, int32_t *out_first, int32_t *out_last) {
    if (!ctx || !tokens || !n_tokens || !heads || !out_first || !out_last) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_align: bad arguments") : NH_ERR_INVALID;
    if (ctx->pool.rows > 0) return ctx->fail(NH_ERR_STATE, "nh_align: the context runs a decode pool (nh_pool_begin)");
    if (!ctx->have_enc) return ctx->fail(NH_ERR_STATE, "nh_align: call nh_encode first");
    if (ctx->opt_absorbed) return ctx->fail(NH_ERR_STATE, "nh_align: NH_OPT_ABSORBED_XATTN keeps no cross K cache to align against");
    const int B = ctx->cur_batch, C = ctx->c.max_target_positions, S = ctx->S, P = prompt_len;
    AlignHeadSet hs;
    if (int rc = align_head_set(ctx, "nh_align", heads, n_heads, 1, hs)) return rc;
    if (P < 1 || P >= C) return ctx->fail(NH_ERR_INVALID, "nh_align: prompt_len out of range");
    int maxn = 0;
    std::vector<int32_t> keys(B);
    for (int b = 0; b < B; b++) {
        const int n = n_tokens[b], nk = n_keys ? n_keys[b] : S;
        if (n <= P || n > C) return ctx->fail(NH_ERR_INVALID, "nh_align: n_tokens must lie in (prompt_len, max_target_positions]");
        if (nk < 1 || nk > S) return ctx->fail(NH_ERR_INVALID, "nh_align: n_keys must lie in [1, S]");
        keys[b] = nk;
        maxn = std::max(maxn, n);
    }
    // the pass below overwrites the tokens and self K/V the last decode left, and the queries it kept
    if (int rc = stage_given_tokens(ctx, "nh_align", tokens, C, 0, n_tokens)) return rc;
    if (int rc = align_q_buffer(ctx, "nh_align", hs.A)) return rc;
    // stage 1: the teacher-forced pass, every position enqueued back to back
    for (int pos = 0; pos <= maxn - 2; pos++) decoder_step(ctx, pos, nullptr, false, false, &hs);
    return align_run(ctx, "nh_align", hs, P, B, std::vector<int32_t>(n_tokens, n_tokens + B), keys, nullptr, out_first, out_last);
}

// ---- alignment from the decode itself (contract: include/norma_hip.h, nh_align_capture / nh_align_decoded) -------------------
extern "C" int nh_align_capture(nh_ctx *ctx, const nh_align_head *heads, int n_heads) {
    if (!ctx || (n_heads > 0 && !heads)) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_align_capture: bad arguments") : NH_ERR_INVALID;
    AlignHeadSet hs;
    if (int rc = align_head_set(ctx, "nh_align_capture", heads, n_heads, 0, hs)) return rc;
    if (hs.A > 0 && ctx->opt_absorbed) return ctx->fail(NH_ERR_STATE, "nh_align_capture: NH_OPT_ABSORBED_XATTN keeps no cross K cache to align against");
    for (const PoolRow &r : ctx->pool.row)
        if (ctx->pool.rows > 0 && r.busy) return ctx->fail(NH_ERR_STATE, "nh_align_capture: rows are busy (the head list is part of the captured steps)");
    hipSetDevice(ctx->dev);
    if (int rc = align_q_buffer(ctx, "nh_align_capture", hs.A)) return rc;
    // what was kept under the list before is no longer answered for; the step graphs of that list are stale (StepKey)
    ctx->live.hs = std::move(hs);
    ctx->live.gen++; ctx->live.lock_valid = false;
    return NH_OK;
}

extern "C" int nh_align_decoded(nh_ctx *ctx, const int32_t *rows, int n, const int32_t *n_keys, int32_t *out_first, int32_t *out_last) {
    if (!ctx || !out_first || !out_last) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_align_decoded: bad arguments") : NH_ERR_INVALID;
    AlignLive &lv = ctx->live;
    const bool pool = ctx->pool.rows > 0;
    const int C = ctx->c.max_target_positions, S = ctx->S, P = pool ? ctx->pool.prompt : lv.P;
    const int NL = ctx->dec_layer_limit > 0 ? ctx->dec_layer_limit : ctx->c.decoder_layers;
    if (pool && !rows) return ctx->fail(NH_ERR_INVALID, "nh_align_decoded: the context runs a decode pool: name the rows");
    if (!pool && rows) return ctx->fail(NH_ERR_INVALID, "nh_align_decoded: rows are a decode pool's; a lockstep context aligns its whole batch (rows = NULL)");
    if (pool) {
        if (n < 1 || n > ctx->pool.rows) return ctx->fail(NH_ERR_INVALID, "nh_align_decoded: n must lie in [1, rows of the pool]");
        for (int i = 0; i < n; i++)
            if (rows[i] < 0 || rows[i] >= ctx->pool.rows) return ctx->fail(NH_ERR_INVALID, "nh_align_decoded: row outside the pool");
    } else if (lv.lock_valid && n != (int)lv.n.size()) return ctx->fail(NH_ERR_INVALID, "nh_align_decoded: n is not the batch of the last decode");
    if (lv.hs.A < 1) return ctx->fail(NH_ERR_STATE, "nh_align_decoded: no alignment heads are set (nh_align_capture)");
    if (ctx->opt_absorbed) return ctx->fail(NH_ERR_STATE, "nh_align_decoded: NH_OPT_ABSORBED_XATTN keeps no cross K cache to align against");
    for (int a = 0; a < lv.hs.A; a++)
        if (lv.hs.heads[a].layer >= NL) return ctx->fail(NH_ERR_STATE, "nh_align_decoded: NH_OPT_DECODER_LAYER_LIMIT cut an alignment head's layer off");
    if (!pool && !lv.lock_valid) return ctx->fail(NH_ERR_STATE, "nh_align_decoded: no decode under these alignment heads whose state is still in place");
    std::vector<int32_t> keys(n), ntok(n);
    for (int i = 0; i < n; i++) {
        int nt, done;
        if (pool) {
            const PoolRow &r = ctx->pool.row[rows[i]];
            if (r.busy) return ctx->fail(NH_ERR_STATE, "nh_align_decoded: that row is busy (nh_pool_collect hands it back first)");
            if (!r.held) return ctx->fail(NH_ERR_STATE, "nh_align_decoded: no clip was admitted into that row since nh_pool_begin");
            if (r.pfx > 0) return ctx->fail(NH_ERR_STATE, "nh_align_decoded: that row's last decode had a prefix (nh_pool_prefix): the kept queries sit at physical positions");
            if (r.align_gen != lv.gen) return ctx->fail(NH_ERR_STATE, "nh_align_decoded: that row has not been collected since it was admitted or retried under the current alignment heads");
            nt = r.n; done = r.done;
        } else { nt = lv.n[i]; done = lv.done[i]; }
        const int nk = n_keys ? n_keys[i] : S;
        if (nk < 1 || nk > S) return ctx->fail(NH_ERR_INVALID, "nh_align_decoded: n_keys must lie in [1, S]");
        const bool nothing = done == 2 || nt <= P || nt > C;   // the no-speech exit holds the prompt alone
        ntok[i] = nothing ? 0 : nt; keys[i] = nk;
    }
    hipSetDevice(ctx->dev);
    return align_run(ctx, "nh_align_decoded", lv.hs, P, n, ntok, keys, rows, out_first, out_last);
}

// rows x nk floats out of a workspace image with row stride S
static int align_view(nh_ctx *ctx, const float *src, int nrows, int nk, float *out) {
    hipSetDevice(ctx->dev);
    HIPCHK(hipMemcpy2DAsync(out, (size_t)nk * 4, src, (size_t)ctx->al.S * 4, (size_t)nk * 4, nrows, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    return NH_OK;
}

extern "C" int nh_align_weights(nh_ctx *ctx, int b, int a, float *out) {
    if (!ctx || !out) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_align_weights: bad arguments") : NH_ERR_INVALID;
    const AlignState &al = ctx->al;
    if (!al.kept) return ctx->fail(NH_ERR_STATE, "nh_align_weights: no alignment under NH_OPT_ALIGN_KEEP = 1 to look at");
    if (b < 0 || b >= (int)al.n_tokens.size() || a < 0 || a >= al.A) return ctx->fail(NH_ERR_INVALID, "nh_align_weights: clip or head out of range");
    if (al.n_tokens[b] < 1) return ctx->fail(NH_ERR_STATE, "nh_align_weights: that sequence had nothing to align (no-speech exit)");
    const size_t NP = ctx->c.max_target_positions - 1;
    return align_view(ctx, al.W + ((size_t)b * al.A + a) * NP * al.S, al.n_tokens[b] - 1, al.keys[b], out);
}

extern "C" int nh_align_matrix(nh_ctx *ctx, int b, float *out) {
    if (!ctx || !out) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_align_matrix: bad arguments") : NH_ERR_INVALID;
    const AlignState &al = ctx->al;
    if (!al.kept) return ctx->fail(NH_ERR_STATE, "nh_align_matrix: no alignment under NH_OPT_ALIGN_KEEP = 1 to look at");
    if (b < 0 || b >= (int)al.n_tokens.size()) return ctx->fail(NH_ERR_INVALID, "nh_align_matrix: clip out of range");
    if (al.n_tokens[b] < 1) return ctx->fail(NH_ERR_STATE, "nh_align_matrix: that sequence had nothing to align (no-speech exit)");
    return align_view(ctx, al.M + (size_t)b * ctx->c.max_target_positions * al.S, al.n_tokens[b] - al.P, al.keys[b], out);
}

extern "C" int nh_align_path(nh_ctx *ctx, const float *matrix, int R, int nk, int32_t *out_first, int32_t *out_last) {
    if (!ctx || !matrix || !out_first || !out_last) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_align_path: bad arguments") : NH_ERR_INVALID;
    const int Smax = ctx->S > 0 ? ctx->S : ctx->c.max_source_positions;
    if (R < 1 || R > ctx->c.max_target_positions || nk < 1 || nk > Smax) return ctx->fail(NH_ERR_INVALID, "nh_align_path: R or nk out of range");
    hipSetDevice(ctx->dev);
    // a parity view with buffers of its own: the workspace of the last nh_align (and its views) stays as it is
    DevBuf tmp;
    Carve cv;
    const size_t o_M = cv.take(sizeof(float) * (size_t)R * nk), o_trace = cv.take((size_t)R * nk);
    const size_t o_meta = cv.take(4 * (2 + 2 * (size_t)(R + 1)));   // n_rows, n_keys, first [R + 1], last [R + 1]
    if (int rc = tmp.reserve(ctx, cv.off, "nh_align_path", true)) return rc;
    float *M = tmp.at<float>(o_M);
    int32_t *meta = tmp.at<int32_t>(o_meta);
    const int32_t rk[2] = {R, nk};
    std::vector<int32_t> fl(2 * (size_t)(R + 1));
    HIPCHK(hipMemcpyAsync(M, matrix, (size_t)R * nk * 4, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(meta, rk, 8, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    // prompt_len 1 and n - 1 = R rows: row r of the matrix is token 1 + r
    if (!launch_align_dtw(M, (long)R * nk, nk, meta, meta + 1, 1, R, nk, 1, 0, tmp.at<uint8_t>(o_trace), (long)R * nk, meta + 2, meta + 2 + (R + 1), R + 1, nullptr, ctx->st))
        return ctx->fail(NH_ERR_INVALID, "nh_align_path: the DTW kernel covers R <= 512");
    HIPCHK(hipMemcpyAsync(fl.data(), meta + 2, fl.size() * 4, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipGetLastError());
    memcpy(out_first, fl.data() + 1, sizeof(int32_t) * R);
    memcpy(out_last, fl.data() + (R + 1) + 1, sizeof(int32_t) * R);
    return NH_OK;
}
