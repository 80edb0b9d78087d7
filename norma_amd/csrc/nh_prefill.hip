// nh_prefill.hip -- the C ABI of include/norma_hip.h, part 3b: decoder prompts (nh_set_prompts) and the one-pass teacher-forced
// decoder forward that consumes them (prefill_forward; nh_decoder_forward_onepass is its parity view).
//
// A decode step streams the decoder weights and every row's cross K/V once per position.  T given positions need neither
// T times: rows (clip, position), M = B * T, go through the encoder's MFMA GEMM (k_gemm.hip) for every projection, and
// through the two attention kernels of k_prefill.hip.  Scratch: the encoder's workspaces, which are idle while the
// context decodes (one stream per context; M <= B * max_target_positions < B * 1500 rows, the encoder's own row count),
// so nothing is allocated and the rows need no grouping:
//   x   f32 residual stream      xn   LayerNorm output        q    self q, then the cross q
//   k   self k                   hid  self v, then the MLP's hidden rows (v is dead by then)
//   att attention output         (hid once more, as f32: the final LayerNorm's f32 rows of the parity view)
// All of these the encoder writes before it reads; h1, mel_img and vt keep zero rows / columns between calls and stay untouched.
// Where the roundings sit: every GEMM takes fp16 rows and accumulates in f32; LayerNorm (the sliced tree of
// the decode step where the width allows) reads the f32 residual stream and rounds once to fp16; q, k, v and the cross q are
// rounded once to fp16 by their GEMM's epilogue (bias added in f32); attention as k_prefill.hip states; GELU in f32,
// rounded once; the residual adds are f32.  A row's arithmetic never looks at another clip's rows and no reduction's order
// depends on M: both GEMM kernels add the 32-deep k-steps of an output in ascending order into one accumulator.
// The ragged form (a decode pool's prefixes, nh_pool_prefix): a list of clips (context row r_i, T_i), rows packed (clip,
// position), M = sum T_i.  The GEMMs and LayerNorms see M rows as before; the embedding and the two attention launches read
// the clip table, which goes up in one copy.  It writes the self caches of the listed rows and reads their cross K/V and
// token rows; of everything else it touches only the scratch above, none of which a staged clip waits in (mel_img, the cross
// K/V of the staging rows) -- and every context has that scratch, a decoding one that never encodes too (build_context).
#include "nh_ctx.h"

bool prefill_supported(const nh_ctx *ctx) { return ctx->c.d_model % 128 == 0 && !ctx->opt_absorbed; }

static void pf_gemm(nh_ctx *ctx, const half_t *A, long lda, const LinW &W, int M, int N, int K, int epi, void *o0, void *o1, void *o2,
                    long ldo, int seg_n) {
    GemmParams p{};
    p.A = A; p.lda = lda; p.a_rpb = M; p.a_bstride = 0; p.W = W.w; p.bias = W.b; p.M = M; p.N = N; p.K = K; p.epi = epi;
    p.out[0] = o0; p.out[1] = o1; p.out[2] = o2; p.seg_n = seg_n; p.ldo = ldo; p.o_rpb = M; p.o_bstride = 0; p.o_off = 0;
    p.vt_seg = -1; p.S = M; p.H = ctx->c.decoder_attention_heads;
    launch_gemm(p, ctx->st);
}

int prefill_forward(nh_ctx *ctx, int T, float *hidden, bool keep_rows, PfClip *clips, int n) {
    const nh_model &m = *ctx->mdl;
    const int d = ctx->c.d_model, B = clips ? n : ctx->cur_batch, H = ctx->c.decoder_attention_heads, C = ctx->c.max_target_positions, S = ctx->S;
    if (!prefill_supported(ctx)) return ctx->fail(NH_ERR_STATE, "the one-pass decoder forward needs d_model % 128 == 0 and NH_OPT_ABSORBED_XATTN == 0");
    int M = B * T;
    const PfClip *tab = nullptr;   // device side of clips
    if (clips) {
        if (hidden || keep_rows || n < 1 || n > ctx->B || !ctx->pfx_host) return ctx->fail(NH_ERR_INVALID, "one-pass decoder forward: bad clip list");
        M = 0; T = 0;
        for (int i = 0; i < n; i++) {
            if (clips[i].row < 0 || clips[i].row >= ctx->B || clips[i].T < 1 || clips[i].T > C) return ctx->fail(NH_ERR_INVALID, "one-pass decoder forward: clip outside the context");
            clips[i].off = M; clips[i].pad = 0;
            M += clips[i].T; T = std::max(T, clips[i].T);
        }
        if ((long)M > (long)ctx->B * 1500) return ctx->fail(NH_ERR_INVALID, "one-pass decoder forward: more rows than the workspaces hold");
        PfClip *h = reinterpret_cast<PfClip *>(ctx->pfx_host + (size_t)ctx->B * (C / 2));
        memcpy(h, clips, sizeof(PfClip) * n);
        HIPCHK(hipMemcpyAsync(ctx->d_pfclips, h, sizeof(PfClip) * n, hipMemcpyHostToDevice, ctx->st));
        tab = ctx->d_pfclips;
    }
    if (B < 1 || T < 1 || T > C || S < 1) return ctx->fail(NH_ERR_INVALID, "one-pass decoder forward: T out of range");
    float *x = ctx->x;
    half_t *xn = ctx->xn, *q = ctx->q, *k = ctx->k, *v = ctx->hid, *att = ctx->att, *hid = ctx->hid;
    const bool full = hidden != nullptr || keep_rows;
    int layers = (int)m.dec.size();
    if (ctx->dec_layer_limit > 0 && ctx->dec_layer_limit < layers) layers = ctx->dec_layer_limit;   // depth profile of the parity tests
    if (tab) launch_embed_ragged(ctx->ds.tokens, C, m.tok_emb, m.dec_pos, x, tab, B, T, d, ctx->st);
    else launch_embed(ctx->ds.tokens, C, m.tok_emb, m.dec_pos, x, B, T, 0, nullptr, d, ctx->st);
    for (int l = 0; l < layers; l++) {
        const DecLayer &L = m.dec[l];
        const KvCache &kv = ctx->kv[l];
        dec_layernorm(ctx, L.ln1, x, xn, nullptr, M, d);
        pf_gemm(ctx, xn, d, L.qkv, M, 3 * d, d, EPI_F16, q, k, v, d, d);
        if (!launch_prefill_self_attention(q, k, v, d, att, d, kv.sk, kv.sv, B, T, H, C, ctx->st, tab))
            return ctx->fail(NH_ERR_INVALID, "one-pass decoder forward: self-attention shape not covered");
        if (!full && l == layers - 1) break;   // a decode needs the prefix rows' K/V only: nothing below feeds a later position
        pf_gemm(ctx, att, d, L.o, M, d, d, EPI_RESID_F32, x, nullptr, nullptr, d, d);
        dec_layernorm(ctx, L.ln2, x, xn, nullptr, M, d);
        pf_gemm(ctx, xn, d, L.cq, M, d, d, EPI_F16, q, nullptr, nullptr, d, d);
        if (!launch_prefill_cross_attention(q, d, kv.ck, kv.cv, att, d, B, T, H, S, ctx->st, tab))
            return ctx->fail(NH_ERR_INVALID, "one-pass decoder forward: cross-attention shape not covered");
        pf_gemm(ctx, att, d, L.co, M, d, d, EPI_RESID_F32, x, nullptr, nullptr, d, d);
        dec_layernorm(ctx, L.ln3, x, xn, nullptr, M, d);
        pf_gemm(ctx, xn, d, L.fc1, M, 4 * d, d, EPI_GELU_F16, hid, nullptr, nullptr, 4 * d, 4 * d);
        pf_gemm(ctx, hid, 4 * d, L.fc2, M, d, 4 * d, EPI_RESID_F32, x, nullptr, nullptr, d, d);
    }
    if (keep_rows && !hidden) {
        dec_layernorm(ctx, m.dec_ln, x, xn, nullptr, M, d);
    } else if (full) {
        float *y32 = reinterpret_cast<float *>(ctx->hid);   // B * 1500 * 4 d halfs: room for 2 * B * 1500 * d floats
        dec_layernorm(ctx, m.dec_ln, x, xn, y32, M, d);
        HIPCHK(hipMemcpyAsync(hidden, y32, sizeof(float) * (size_t)M * d, hipMemcpyDeviceToHost, ctx->st));
        HIPCHK(hipStreamSynchronize(ctx->st));
    }
    HIPCHK(hipGetLastError());
    return NH_OK;
}

extern "C" int nh_decoder_forward_onepass(nh_ctx *ctx, const int32_t *tokens, int T, float *hidden_out) {
    if (!ctx || !tokens || !hidden_out) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_decoder_forward_onepass: bad arguments") : NH_ERR_INVALID;
    if (ctx->pool.rows > 0) return ctx->fail(NH_ERR_STATE, "nh_decoder_forward_onepass: the context runs a decode pool (nh_pool_begin)");
    if (!ctx->have_enc) return ctx->fail(NH_ERR_STATE, "nh_decoder_forward_onepass: call nh_encode first");
    if (T < 1 || T > ctx->c.max_target_positions) return ctx->fail(NH_ERR_INVALID, "nh_decoder_forward_onepass: T out of range");
    if (!prefill_supported(ctx)) return ctx->fail(NH_ERR_STATE, "nh_decoder_forward_onepass: needs d_model % 128 == 0 and NH_OPT_ABSORBED_XATTN == 0");
    if (int rc = stage_given_tokens(ctx, "nh_decoder_forward_onepass", tokens, T, T)) return rc;
    return prefill_forward(ctx, T, hidden_out);
}

// The ids of a pool row's next clip (contract: include/norma_hip_pool.h).  Nothing is launched: the ids wait in the context's pinned
// host buffer until the admission copies them into the row.
extern "C" int nh_pool_prefix(nh_ctx *ctx, int row, const int32_t *tokens, int n_prefix) {
    if (!ctx) return NH_ERR_INVALID;
    Pool &pl = ctx->pool;
    if (pl.rows < 1) return ctx->fail(NH_ERR_STATE, "nh_pool_prefix: no decode pool (nh_pool_begin)");
    if (row < 0 || row >= pl.rows || pl.row[row].busy) return ctx->fail(NH_ERR_INVALID, "nh_pool_prefix: row is not a free row of the pool");
    const int half = ctx->c.max_target_positions / 2;
    if (n_prefix < 0 || n_prefix > half - 1) return ctx->fail(NH_ERR_INVALID, "nh_pool_prefix: n_prefix outside [0, max_target_positions / 2 - 1]");
    if (!tokens || n_prefix == 0) { if (!pl.pending.empty()) pl.pending[row] = 0; return NH_OK; }
    for (int i = 0; i < n_prefix; i++)
        if (tokens[i] < 0 || tokens[i] >= ctx->c.vocab_size) return ctx->fail(NH_ERR_INVALID, "nh_pool_prefix: token id outside the vocabulary");
    if (!ctx->pfx_host) {
        hipSetDevice(ctx->dev);
        const size_t bytes = sizeof(int32_t) * (size_t)ctx->B * half + sizeof(PfClip) * (size_t)ctx->B;
        if (hipHostMalloc(reinterpret_cast<void **>(&ctx->pfx_host), bytes, 0) != hipSuccess) {
            ctx->pfx_host = nullptr; (void)hipGetLastError();
            return ctx->fail(NH_ERR_NOMEM, "nh_pool_prefix: hipHostMalloc failed");
        }
    }
    if (pl.pending.empty()) pl.pending.assign(ctx->B, 0);
    // the row is free: nh_pool_collect drained the stream behind the copy of the ids it held before
    memcpy(ctx->pfx_host + (size_t)row * half, tokens, sizeof(int32_t) * n_prefix);
    pl.pending[row] = n_prefix;
    return NH_OK;
}

extern "C" int nh_set_prompts(nh_ctx *ctx, const int32_t *tokens, int n_prefix, int64_t stride, int batch) {
    if (!ctx) return NH_ERR_INVALID;
    if (ctx->pool.rows > 0) return ctx->fail(NH_ERR_STATE, "nh_set_prompts: the context runs a decode pool (pool rows take no prefix)");
    if (batch != ctx->cur_batch || batch < 1) return ctx->fail(NH_ERR_INVALID, "nh_set_prompts: batch is not the context's current batch");
    if (!tokens || n_prefix == 0) { clear_prompt(ctx); return NH_OK; }
    if (n_prefix < 0 || n_prefix > ctx->c.max_target_positions / 2 - 1)
        return ctx->fail(NH_ERR_INVALID, "nh_set_prompts: n_prefix outside [0, max_target_positions / 2 - 1]");
    if (stride < n_prefix) return ctx->fail(NH_ERR_INVALID, "nh_set_prompts: stride < n_prefix");
    for (int b = 0; b < batch; b++)
        for (int i = 0; i < n_prefix; i++) {
            const int32_t t = tokens[(size_t)b * stride + i];
            if (t < 0 || t >= ctx->c.vocab_size) return ctx->fail(NH_ERR_INVALID, "nh_set_prompts: token id outside the vocabulary");
        }
    ctx->prompt.resize((size_t)batch * n_prefix);
    for (int b = 0; b < batch; b++) memcpy(ctx->prompt.data() + (size_t)b * n_prefix, tokens + (size_t)b * stride, sizeof(int32_t) * n_prefix);
    ctx->n_prefix = n_prefix; ctx->prompt_batch = batch;
    return NH_OK;
}
