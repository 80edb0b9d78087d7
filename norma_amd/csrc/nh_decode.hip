// nh_decode.hip -- the C ABI of include/norma_hip.h, part 3: the decoder step and what sequences it -- the lockstep decode,
// the decode pool, language detection and the parity views.  Token-level timestamps (nh_align.hip) come here for decoder_step.
#include "nh_ctx.h"

// ---- decoder ---------------------------------------------------------------------------------------------
#define NH_GRAPH_STEPS 8

// whoever changes something the captured steps bake in (StepKey, the options) drops the graphs, the next decode captures
// again.  first = 1 keeps the greedy pair.
void drop_graphs(nh_ctx *ctx, int first) {
    for (int s = first; s < 2; s++) {
        StepGraphs &g = ctx->graphs[s];
        if (g.one) hipGraphExecDestroy(g.one);
        if (g.multi) hipGraphExecDestroy(g.multi);
        g = StepGraphs{};
    }
}

static void skinny(nh_ctx *ctx, const half_t *x, long ldx, const LinW &W, int R, int N, int K, int epi, void *o0, void *o1,
                   void *o2, long ldo, int t0, int ctxlen, const int32_t *pos_ptr = nullptr, const float *ln_x = nullptr,
                   const float *ln_w = nullptr, const float *ln_b = nullptr) {
    SkinnyParams p{};
    p.pos_ptr = pos_ptr; p.ln_x = ln_x; p.ln_w = ln_w; p.ln_b = ln_b;
    p.x = x; p.ldx = ldx; p.W = W.w; p.Wt = W.wt; p.bias = W.b; p.R = R; p.N = N; p.K = K; p.epi = epi;
    p.out[0] = o0; p.out[1] = o1; p.out[2] = o2; p.ldo = ldo; p.d = ctx->c.d_model; p.t0 = t0; p.Tn = 1; p.ctx = ctxlen;
    // every caller checks skinny_ln_supported before it passes ln_x, R <= max_batch <= 96, and every K and N of the model is a
    // multiple of 64 but the vocabulary (SK_F32): a refusal is a broken invariant, and going on would leave the output as it was
    if (!launch_skinny(p, ctx->st)) {
        fprintf(stderr, "norma_hip: launch_skinny refused R=%d N=%d K=%d (ln_x %s)\n", R, N, K, ln_x ? "set" : "unset");
        abort();
    }
}

// every decoder LayerNorm uses the "sliced" summation tree (nh_kernels.h) when the width allows, so that the fused and
// the stand-alone forms, and every batch size, give bit-identical rows
void dec_layernorm(nh_ctx *ctx, const LnW &ln, const float *x, half_t *y, float *y32, int R, int K) {
    if (!launch_layernorm_sliced(x, ln.w, ln.b, y, y32, R, K, ctx->st)) launch_layernorm(x, ln.w, ln.b, y, y32, R, K, ctx->st);
}

// LayerNorm + projection of one decode step: fused into the skinny GEMM when the shape allows (the separate
// LayerNorm launch is pure latency at B rows), otherwise LayerNorm into dxn first
static void ln_skinny(nh_ctx *ctx, const LnW &ln, const LinW &W, int R, int N, int K, int epi, void *o0, void *o1, void *o2,
                      long ldo, int t0, int ctxlen, const int32_t *pos_ptr) {
    if (ctx->opt_fuse_ln && skinny_ln_supported(R, N, K)) {
        skinny(ctx, nullptr, K, W, R, N, K, epi, o0, o1, o2, ldo, t0, ctxlen, pos_ptr, ctx->dx, ln.w, ln.b);
    } else {
        dec_layernorm(ctx, ln, ctx->dx, ctx->dxn, nullptr, R, K);
        skinny(ctx, ctx->dxn, K, W, R, N, K, epi, o0, o1, o2, ldo, t0, ctxlen, pos_ptr);
    }
}

// one decoder position for the whole batch: consumes tokens[b][pos], leaves the residual stream in dx.
// final_ln: also LN(dx) -> dxn (fp16) / dy32 (f32) (the teacher-forced view; the step path fuses it into the logits).
// pos_ptr != nullptr: the position comes from device memory (the step is being captured into a hipGraph).
// skip_done: finished sequences skip their attention (only inside decode_impl, where ds.done is live).
// keep (nh_align's pass; a decode under nh_align_capture): the layers that hold alignment heads copy those heads' cross-attention
// query to ctx->align_q[head][pos][row][64] right after the projection, every row at the position and under the done flag the
// step itself goes by; nullptr (every other caller, and a decode with no heads set): nothing is added to the step.
void decoder_step(nh_ctx *ctx, int pos, const int32_t *pos_ptr, bool final_ln, bool skip_done, const AlignHeadSet *keep) {
    const int32_t *done = skip_done ? ctx->ds.done : nullptr;
    const nh_model &m = *ctx->mdl;
    const int d = ctx->c.d_model, B = ctx->pool.rows > 0 ? ctx->pool.rows : ctx->cur_batch, H = ctx->c.decoder_attention_heads, C = ctx->c.max_target_positions;
    launch_embed(ctx->ds.tokens, C, m.tok_emb, m.dec_pos, ctx->dx, B, 1, pos, pos_ptr, d, ctx->st);
    for (size_t l = 0; l < m.dec.size(); l++) {
        if (ctx->dec_layer_limit > 0 && (int)l >= ctx->dec_layer_limit) break;  // depth profile of the parity tests
        const DecLayer &L = m.dec[l];
        const KvCache &kv = ctx->kv[l];
        ln_skinny(ctx, L.ln1, L.qkv, B, 3 * d, d, SK_QKV, ctx->dq, kv.sk, kv.sv, d, pos, C, pos_ptr);
        launch_dec_attention(ctx->dq, kv.sk, kv.sv, ctx->datt, B, H, d, C, pos + 1, pos_ptr, ctx->st, done);  // head-major cache
        skinny(ctx, ctx->datt, d, L.o, B, d, d, SK_RESID_F32, ctx->dx, nullptr, nullptr, d, 0, C);
        ln_skinny(ctx, L.ln2, L.cq, B, d, d, SK_F16, ctx->dq, nullptr, nullptr, d, 0, C, nullptr);
        if (keep && keep->layer[l].n) launch_align_qsave(ctx->dq, ctx->align_q.at<half_t>(), keep->layer[l], B, ctx->B, d, pos, pos_ptr, done, C - 1, ctx->st);
        if (ctx->opt_absorbed == 2) launch_xabs_attention_fast(ctx->dq, L.ckv.wt, L.ckv.w, L.ckv.b, ctx->xa16, ctx->xabs.u.at<half_t>(), ctx->xabs.z, ctx->xabs.ml, ctx->datt, B, H, d, ctx->S, done, ctx->st);
        else if (ctx->opt_absorbed) launch_xabs_attention(ctx->dq, L.ckv.w, L.ckv.b, ctx->xa16, ctx->xabs.u.at<half_t>(), ctx->datt, B, H, d, ctx->S, done, ctx->st);
        else launch_dec_attention(ctx->dq, kv.ck, kv.cv, ctx->datt, B, H, d, ctx->S, ctx->S, nullptr, ctx->st, done);  // head-major cross K/V
        skinny(ctx, ctx->datt, d, L.co, B, d, d, SK_RESID_F32, ctx->dx, nullptr, nullptr, d, 0, C);
        ln_skinny(ctx, L.ln3, L.fc1, B, 4 * d, d, SK_GELU_F16, ctx->dhid, nullptr, nullptr, 4 * d, 0, C, nullptr);
        skinny(ctx, ctx->dhid, 4 * d, L.fc2, B, d, 4 * d, SK_RESID_F32, ctx->dx, nullptr, nullptr, d, 0, C);
    }
    if (final_ln) dec_layernorm(ctx, m.dec_ln, ctx->dx, ctx->dxn, ctx->dy32, B, d);
}

// TextDecoder::final_linear on LN(dx) of the R rows of the last decoder_step(..., final_ln = false)
static LinW tied_embedding(nh_ctx *ctx) { return LinW{ctx->mdl->tok_emb, nullptr, ctx->mdl->tok_emb_t}; }  // no bias (final_linear)
void logits_from_dx(nh_ctx *ctx, int R) {
    const int d = ctx->c.d_model;
    ln_skinny(ctx, ctx->mdl->dec_ln, tied_embedding(ctx), R, ctx->c.vocab_size, d, SK_F32, ctx->logits, nullptr, nullptr, ctx->VP, 0, 0, nullptr);
}

static void logits_from_dxn(nh_ctx *ctx, int R) {
    skinny(ctx, ctx->dxn, ctx->c.d_model, tied_embedding(ctx), R, ctx->c.vocab_size, ctx->c.d_model, SK_F32, ctx->logits, nullptr, nullptr,
           ctx->VP, 0, 0);
}

// what Model::decode returns for one sequence from the state its loop left behind (model.rs:308-315, 373-381)
// skip: the prefix of a prompted decode (nh_set_prompts), which is not part of what comes back: tokens, their count and the
// divisor of avg_logprob are those of the sequence from sot on
void finish_sequence(nh_ctx *ctx, int32_t *t, int n, int done, double slp, double nsp, int32_t *out_tokens, nh_decode_result &r, int skip) {
    const int C = ctx->c.max_target_positions;
    t += skip; n -= skip;
    r.no_speech_prob = nsp;
    r.no_speech_exit = (done == 2);
    if (done == 2) { r.avg_logprob = 0.0; }  // model.rs:308-315
    else {
        r.avg_logprob = slp / (double)n;  // model.rs:373 (prompt and eot count)
        while (n >= 2 && t[n - 2] > ctx->tk.no_timestamps) { t[n - 2] = t[n - 1]; n--; }  // :375-381
    }
    r.n_tokens = n;
    memcpy(out_tokens, t, sizeof(int32_t) * (C - skip));
    for (int i = n; i < C; i++) out_tokens[i] = 0;
}

int queue_decode_state(nh_ctx *ctx, const int32_t *rows, int n, int B, HostDecodeState &h) {
    const int C = ctx->c.max_target_positions;
    h.toks.resize((size_t)n * C); h.nt.resize(B); h.done.resize(B); h.slp.resize(B); h.nsp.resize(B);
    if (!rows) HIPCHK(hipMemcpyAsync(h.toks.data(), ctx->ds.tokens, h.toks.size() * 4, hipMemcpyDeviceToHost, ctx->st));
    else
        for (int i = 0; i < n; i++)
            HIPCHK(hipMemcpyAsync(h.toks.data() + (size_t)i * C, ctx->ds.tokens + (size_t)rows[i] * C, sizeof(int32_t) * C, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(h.nt.data(), ctx->ds.n_tokens, B * 4, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(h.done.data(), ctx->ds.done, B * 4, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(h.slp.data(), ctx->ds.sum_logprob, B * 8, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(h.nsp.data(), ctx->ds.no_speech, B * 8, hipMemcpyDeviceToHost, ctx->st));
    return NH_OK;
}

// device state -> results of the sequences in rows[0 .. n) (rows == nullptr: rows 0 .. n - 1); only those token rows cross
static int read_results(nh_ctx *ctx, const int32_t *rows, int n, int32_t *out_tokens, nh_decode_result *results, int skip = 0) {
    const int C = ctx->c.max_target_positions;
    HostDecodeState h;
    if (int rc = queue_decode_state(ctx, rows, n, rows ? ctx->pool.rows : n, h)) return rc;
    HIPCHK(hipStreamSynchronize(ctx->st));
    for (int i = 0; i < n; i++)
        if (rows && h.done[rows[i]] != 1 && h.done[rows[i]] != 2) return ctx->fail(NH_ERR_STATE, "nh_pool_collect: that row has not finished (see nh_pool_step's done flags)");
    if (!rows) { ctx->live.n.assign(n, 0); ctx->live.done.assign(n, 0); }
    for (int i = 0; i < n; i++) {
        const int b = rows ? rows[i] : i;
        // a pool row's skip is its own prefix (nh_pool_prefix)
        finish_sequence(ctx, h.toks.data() + (size_t)i * C, h.nt[b], h.done[b], h.slp[b], h.nsp[b], out_tokens + (size_t)i * C, results[i],
                        rows ? ctx->pool.row[b].pfx : skip);
        // what nh_align_decoded aligns: the sequence as returned
        if (rows) { PoolRow &r = ctx->pool.row[b]; r.n = results[i].n_tokens; r.done = h.done[b]; }
        else { ctx->live.n[i] = results[i].n_tokens; ctx->live.done[i] = h.done[b]; }
    }
    return NH_OK;
}

// One generated token for every sequence: the decoder at the sequences' positions, the logits, and the kernels that pick the
// token and advance the state.  Issued eagerly or into a stream capture (ensure_step_graphs): the same calls either way.
struct StepSpec {
    int B, max_new, P;
    int mode;                  // launch_logit_step's: 1 lockstep batch, 2 pool (a position per row)
    bool sampled;              // lockstep: every sequence samples with the arguments below; pool: some busy row is on a retry (psamp)
    int pos;                   // the batch's position, when pos_ptr == nullptr
    int32_t *pos_ptr;          // device-side positions, read and advanced by the step (pools, captured steps)
    float inv_t; unsigned long long seed; unsigned clip0, attempt;   // lockstep sampling (nh_decode_sampled)
};
// the heads whose queries the context's decodes keep (nh_align_capture); nullptr: none
static const AlignHeadSet *kept_heads(const nh_ctx *ctx) { return ctx->live.hs.A > 0 ? &ctx->live.hs : nullptr; }

static void emit_token_step(nh_ctx *ctx, const StepSpec &s) {
    const int C = ctx->c.max_target_positions, cap = C - 1, V = ctx->c.vocab_size;
    const bool pool = s.mode == 2;
    decoder_step(ctx, s.pos, s.pos_ptr, false, true, kept_heads(ctx));
    logits_from_dx(ctx, s.B);
    if (pool && ctx->pool.lang_n > 0)
        launch_pool_lang_detect(ctx->logits, V, ctx->ds, s.B, C, s.pos_ptr, PoolDetect{ctx->d_lang_flag, ctx->d_lang_tokens, ctx->pool.lang_n, ctx->d_lang_out, ctx->d_lang_probs}, ctx->st);
    const int32_t *pfx = pool ? ctx->d_pfx : nullptr;   // a pool's per-row prefix lengths: the pointer, so a prefix never recaptures
    if (ctx->guard.on) emit_guard(ctx, s.B, s.P, pool ? s.pos_ptr : nullptr, s.B);   // nh_set_guard; off: nothing is launched
    if (s.sampled && !pool) {  // lockstep sampled: every sequence draws its token
        launch_sample_step(ctx->logits, V, ctx->ds, ctx->tk, s.B, C, cap, s.max_new, s.P, s.inv_t, s.seed, s.clip0, s.attempt, ctx->st);
        return;
    }
    // greedy.  In a pool with a row on a sampled retry, the kernel of those rows goes first and tells the greedy one which it took.
    if (s.sampled) launch_pool_sample_step(ctx->logits, V, ctx->ds, ctx->tk, s.B, C, cap, s.max_new, s.P, ctx->psamp, s.pos_ptr, ctx->st, pfx);
    launch_logit_step(ctx->logits, V, ctx->ds, ctx->tk, s.B, C, cap, s.max_new, s.P, s.mode, ctx->lpart, ctx->ltick, s.pos_ptr, ctx->st,
                      s.sampled ? ctx->psamp.handled : nullptr, pfx);
}

// The graphs of `key`, captured unless the slot holds them already.  A key that the greedy slot does not hold drops both
// pairs (whatever changed, the sampled pair is stale too); one that only the sampled slot does not hold drops that pair.
static int ensure_step_graphs(nh_ctx *ctx, const StepKey &key) {
    StepGraphs &g = ctx->graphs[key.sampled];
    if (g.key == key) return NH_OK;
    drop_graphs(ctx, key.sampled);
    std::lock_guard<std::mutex> lk(ctx->mdl->capture_mu);
    const StepSpec spec{key.B, key.max_new, key.P, key.pool ? 2 : 1, key.sampled, 0, ctx->d_pos, 0.f, 0, 0, 0};
    for (int which = 0; which < 2; which++) {
        hipGraph_t graph = nullptr;
        hipError_t ge = hipStreamBeginCapture(ctx->st, hipStreamCaptureModeThreadLocal);
        if (ge != hipSuccess) return ctx->fail(NH_ERR_HIP, std::string("hipStreamBeginCapture: ") + hipGetErrorString(ge));
        for (int i = 0; i < (which ? NH_GRAPH_STEPS : 1); i++) emit_token_step(ctx, spec);  // every step reads and advances the device-side positions
        // the stream must leave capture mode whatever happened in between; a failed capture leaves no graph behind
        ge = hipStreamEndCapture(ctx->st, &graph);
        if (ge == hipSuccess && !graph) ge = hipErrorStreamCaptureInvalidated;
        if (ge == hipSuccess) {
            ge = hipGraphInstantiate(which ? &g.multi : &g.one, graph, nullptr, nullptr, 0);
            if (ge != hipSuccess) (which ? g.multi : g.one) = nullptr;
        }
        if (graph) hipGraphDestroy(graph);
        if (ge != hipSuccess) {
            (void)hipGetLastError();
            drop_graphs(ctx, key.sampled);
            return ctx->fail(NH_ERR_HIP, std::string("decode-step graph capture: ") + hipGetErrorString(ge));
        }
    }
    g.key = key;
    return NH_OK;
}

// What a decode of the lockstep batch refuses before it touches anything (nh_decode_greedy, nh_decode_sampled, nh_decode_beam)
int decode_refusals(nh_ctx *ctx) {
    if (!ctx->have_enc) return ctx->fail(NH_ERR_STATE, "nh_decode: call nh_encode first");
    if (!ctx->have_tokens) return ctx->fail(NH_ERR_STATE, "nh_decode: call nh_set_tokens first");
    if (ctx->pool.rows > 0) return ctx->fail(NH_ERR_STATE, "nh_decode: the context runs a decode pool (nh_pool_begin); a batch submitted with row0 = 0 ends it");
    if (ctx->n_prefix > 0 && ctx->prompt_batch != ctx->cur_batch) return ctx->fail(NH_ERR_STATE, "nh_decode: the prefix was set for another batch (rows joined since nh_set_prompts)");
    return NH_OK;
}

// How every decode of the lockstep batch begins (model.rs:285-305): the state of the B clip rows starts over, the prompt
// [prefix.., sot, lang?, task] is written and consumed up to its last token, the no-speech probe reads sot's logits.  On
// return the rows stand before their first generation step at position dp.PL - 1, the stream not yet drained.
int decode_prompt_phase(nh_ctx *ctx, int max_new_tokens, DecodePrompt &dp) {
    const int NP = ctx->n_prefix;   // nh_set_prompts: tokens in front of the prompt; 0: none, and everything below is the plain decode
    hipSetDevice(ctx->dev);
    if (int rc = ensure_decoder_repack(ctx)) return rc;
    ctx->live.lock_valid = false;
    const int B = ctx->cur_batch, C = ctx->c.max_target_positions, cap = C - 1, V = ctx->c.vocab_size;
    // model.rs:285-289: prompt = [sot, lang?, task]
    const bool per_seq = (int)ctx->seq_lang.size() == B;
    const int P = (per_seq || ctx->tk.lang >= 0) ? 3 : 2;  // 2 or 3, so position 0 is never a generation step
    const int PL = NP + P;   // the physical prompt: what the rules, the forced first timestamp and max_new_tokens count from
    std::vector<int32_t> toks((size_t)B * C, 0), nt(B, PL);
    for (int b = 0; b < B; b++) {
        int32_t *t = toks.data() + (size_t)b * C;
        int i = NP;
        if (NP > 0) memcpy(t, ctx->prompt.data() + (size_t)b * NP, sizeof(int32_t) * NP);
        t[i++] = ctx->tk.sot;
        if (P == 3) t[i++] = per_seq ? ctx->seq_lang[b] : ctx->tk.lang;
        t[i++] = ctx->tk.task;
    }
    // the encoder and cross K/V ran on this same stream: the wait orders nothing new (the cross-context one in pool_admit_impl
    // does) and stays as part of the stream's order of operations
    HIPCHK(hipStreamWaitEvent(ctx->st, ctx->enc_done, 0));
    HIPCHK(hipMemcpyAsync(ctx->ds.tokens, toks.data(), toks.size() * 4, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(ctx->ds.n_tokens, nt.data(), B * 4, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemsetAsync(ctx->ds.done, 0, B * 4, ctx->st));
    HIPCHK(hipMemsetAsync(ctx->ltick, 0, B * 4, ctx->st));
    HIPCHK(hipMemsetAsync(ctx->ds.have_last, 0, B * 4, ctx->st));
    HIPCHK(hipMemsetAsync(ctx->ds.last_ts, 0, B * 4, ctx->st));
    HIPCHK(hipMemsetAsync(ctx->ds.sum_logprob, 0, B * 8, ctx->st));
    HIPCHK(hipMemsetAsync(ctx->ds.no_speech, 0, B * 8, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));  // toks/nt are stack-owned host buffers
    HIPCHK(hipEventRecord(ctx->ev[5], ctx->st));
    int steps = 0;
    // Prompt phase (eager): position pos consumes tokens[pos]; pos 0 also yields no_speech_prob
    // (model.rs:293-305: logits at position 0 of the flush = true pass).
    // Under a prefix, positions 0 .. NP-1 consume it first: in one pass over all of them (nh_prefill.hip: the caches of those
    // positions are all the later ones need), or through the step one by one (NH_OPT_PROMPT_STEPWISE, prefixes too short for
    // the one pass to pay, widths and options it does not cover); sot then sits at position NP, and the probe reads ITS logits.
    if (NP > 0) {
        if (!ctx->opt_prompt_stepwise && NP >= NH_PREFILL_MIN_PREFIX && prefill_supported(ctx)) {
            if (int rc = prefill_forward(ctx, NP, nullptr)) return rc;
        } else {
            for (int pos = 0; pos < NP; pos++) decoder_step(ctx, pos, nullptr, false, true, kept_heads(ctx));
        }
        steps += NP;
    }
    for (int pos = NP; pos < PL - 1; pos++) {
        decoder_step(ctx, pos, nullptr, true, true, kept_heads(ctx));
        steps++;
        if (pos == NP) {
            logits_from_dxn(ctx, B);
            launch_logit_step(ctx->logits, V, ctx->ds, ctx->tk, B, C, cap, max_new_tokens, PL, 0, ctx->lpart, ctx->ltick, nullptr, ctx->st);
        }
    }
    dp = DecodePrompt{B, NP, P, PL, steps};
    return NH_OK;
}

// Model::decode (model.rs:279-389) for the whole batch.  inv_t == 0: t = 0, greedy (hipGraph replay); inv_t > 0: every
// token is sampled at temperature 1 / inv_t under the seeded contract (eager launches: the fallback path is rare).
static int decode_impl(nh_ctx *ctx, int32_t *out_tokens, nh_decode_result *results, int max_new_tokens, float inv_t,
                       unsigned long long seed, unsigned clip0, unsigned attempt) {
    if (!ctx || !out_tokens || !results) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_decode: bad arguments") : NH_ERR_INVALID;
    if (int rc = decode_refusals(ctx)) return rc;
    DecodePrompt dp{};
    if (int rc = decode_prompt_phase(ctx, max_new_tokens, dp)) return rc;
    const int B = dp.B, NP = dp.NP, P = dp.P, PL = dp.PL, cap = ctx->c.max_target_positions - 1;
    int steps = dp.steps;
    // Generation phase: one token per step from pos = P-1 on.  The length cap (model.rs:367) forces eot once
    // pos + 2 >= cap, so pos never exceeds cap - 2.  The ~20-launch step is captured (once, and 8 steps back to back) into hipGraphs that
    // reads the position from device memory (the eager loop is host-launch-bound at ~5 us per tiny kernel).
    const bool no_graph = !ctx->opt_graphs || inv_t > 0.f;
    if (!no_graph)
        if (int rc = ensure_step_graphs(ctx, StepKey{B, ctx->S, max_new_tokens, PL, ctx->token_gen, 0, false, false, ctx->live.gen, ctx->guard.gen})) return rc;
    const int32_t first_pos = PL - 1;
    for (int b = 0; b < B; b++) ctx->h_done[128 + b] = first_pos;  // every sequence of a batch starts generating at the same position
    HIPCHK(hipMemcpyAsync(ctx->d_pos, ctx->h_done + 128, sizeof(int32_t) * B, hipMemcpyHostToDevice, ctx->st));
    // positions first_pos .. cap - 2; the host looks at the done flags every 16 steps (and after the last one)
    for (int pos = first_pos; pos <= cap - 2;) {
        int n = 1;
        if (no_graph) {
            emit_token_step(ctx, StepSpec{B, max_new_tokens, PL, 1, inv_t > 0.f, pos, nullptr, inv_t, seed, clip0, attempt});
        } else if (pos + NH_GRAPH_STEPS - 1 <= cap - 2) {
            HIPCHK(hipGraphLaunch(ctx->graphs[0].multi, ctx->st));
            n = NH_GRAPH_STEPS;
        } else {
            HIPCHK(hipGraphLaunch(ctx->graphs[0].one, ctx->st));
        }
        steps += n;
        const int before = pos - first_pos;
        pos += n;
        if ((before >> 4) != ((pos - first_pos) >> 4) || pos > cap - 2) {
            HIPCHK(hipMemcpyAsync(ctx->h_done, ctx->ds.done, B * 4, hipMemcpyDeviceToHost, ctx->st));
            HIPCHK(hipStreamSynchronize(ctx->st));
            bool all = true;
            for (int b = 0; b < B; b++) all = all && ctx->h_done[b] != 0;
            if (all) break;
        }
    }
    HIPCHK(hipEventRecord(ctx->ev[6], ctx->st));
    HIPCHK(hipGetLastError());
    if (int rc = read_results(ctx, nullptr, B, out_tokens, results, NP)) return rc;
    ctx->tm.decode_steps = steps;
    ctx->guard.after_beam = false;
    // after a prompted decode the kept queries sit at physical positions, which nh_align_decoded does not map: it refuses
    ctx->live.lock_valid = kept_heads(ctx) != nullptr && NP == 0; ctx->live.P = P;
    return NH_OK;
}

extern "C" int nh_decode_greedy(nh_ctx *ctx, int32_t *out_tokens, nh_decode_result *results, int max_new_tokens) {
    return decode_impl(ctx, out_tokens, results, max_new_tokens, 0.f, 0, 0, 0);
}

extern "C" int nh_decode_sampled(nh_ctx *ctx, int32_t *out_tokens, nh_decode_result *results, int max_new_tokens,
                                 float temperature, uint64_t seed, uint32_t clip0, uint32_t attempt) {
    if (ctx && !(temperature > 0.f)) return ctx->fail(NH_ERR_INVALID, "nh_decode_sampled: temperature must be > 0 (use nh_decode_greedy for t = 0)");
    return decode_impl(ctx, out_tokens, results, max_new_tokens, 1.0f / temperature, seed, clip0, attempt);
}

// ---- decode pool -------------------------------------------------------------------------------------------
// The reference's loop ends per sequence at eot (model.rs:317), so the sequences of a batch do not finish together.
// Rows [0, rows) of the context decode, every row at its own position; a finished row is handed back (nh_pool_collect)
// and refilled (nh_pool_admit) from the encoder staging rows [rows, max_batch) while the others go on.  Every row's
// arithmetic is what it is in nh_decode_greedy -- the step kernels are the same, only the position is per row.
extern "C" int nh_pool_begin(nh_ctx *ctx, int rows, int max_new_tokens, int per_clip_language) {
    if (!ctx) return NH_ERR_INVALID;
    if (rows < 1 || rows >= ctx->B) return ctx->fail(NH_ERR_INVALID, "nh_pool_begin: rows must lie in [1, max_batch - 1] (the rows above are encoder staging)");
    if (!ctx->have_tokens) return ctx->fail(NH_ERR_STATE, "nh_pool_begin: call nh_set_tokens first");
    hipSetDevice(ctx->dev);
    if (int rc = ensure_decoder_repack(ctx)) return rc;
    if (ctx->opt_absorbed) return ctx->fail(NH_ERR_STATE, "nh_pool_begin: the NH_OPT_ABSORBED_XATTN prototype covers lockstep decodes only");
    bool was_sampled = false;   // read off the rows of the pool before, which the fresh Pool replaces
    for (const PoolRow &r : ctx->pool.row) was_sampled = was_sampled || r.inv_t_set;
    const int prompt = (per_clip_language || ctx->tk.lang >= 0) ? 3 : 2;
    ctx->pool = Pool{rows, max_new_tokens, prompt, 0, per_clip_language != 0, std::vector<PoolRow>(rows)};   // no language table, fresh rows
    ctx->cur_batch = rows; ctx->frames = -1; ctx->S = 0; ctx->have_mel = false; ctx->have_enc = false;
    ctx->live.lock_valid = false;
    ctx->seq_lang.clear();
    clear_prompt(ctx);
    for (int b = 0; b < rows; b++) ctx->h_done[128 + b] = 3;  // 3: empty row (skipped like a finished one)
    HIPCHK(hipMemcpyAsync(ctx->ds.done, ctx->h_done + 128, sizeof(int32_t) * rows, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemsetAsync(ctx->d_pos, 0, sizeof(int32_t) * rows, ctx->st));
    HIPCHK(hipMemsetAsync(ctx->d_pfx, 0, sizeof(int32_t) * ctx->B, ctx->st));   // no row has a prefix, none is pending (the fresh Pool)
    HIPCHK(hipMemsetAsync(ctx->ltick, 0, sizeof(unsigned) * rows, ctx->st));
    if (was_sampled) HIPCHK(hipMemsetAsync(ctx->psamp.inv_t, 0, sizeof(float) * ctx->B, ctx->st));  // rows an earlier pool left on a retry: greedy again
    HIPCHK(hipStreamSynchronize(ctx->st));
    return NH_OK;
}

// A row that is admitted again or handed back leaves the list of the next ragged prefill: the list never holds a row twice,
// so it never outgrows the pool
static void drop_pending_prefill(Pool &pl, int row) {
    pl.todo.erase(std::remove_if(pl.todo.begin(), pl.todo.end(), [row](const PfClip &c) { return c.row == row; }), pl.todo.end());
}

static int pool_admit_impl(nh_ctx *ctx, nh_ctx *src, int src_row, int dst_row, int32_t lang) {
    if (dst_row < 0 || dst_row >= ctx->pool.rows || ctx->pool.row[dst_row].busy) return ctx->fail(NH_ERR_INVALID, "nh_pool_admit: dst_row is not a free row of the pool");
    PoolRow &row = ctx->pool.row[dst_row];
    const int P = ctx->pool.prompt;
    const bool detect = lang == NH_LANG_DETECT;
    if (!ctx->pool.per_clip_language && (lang >= 0 || detect)) return ctx->fail(NH_ERR_INVALID, "nh_pool_admit: the pool was begun without per-clip languages");
    if (detect && ctx->pool.lang_n < 1) return ctx->fail(NH_ERR_STATE, "nh_pool_admit: NH_LANG_DETECT needs the pool's language table (nh_pool_detect_languages)");
    // a detecting row holds sot in slot 1 until its first step has written the language there; nothing reads the slot before
    int32_t lg = detect ? ctx->tk.sot : lang >= 0 ? lang : ctx->tk.lang;
    if (P == 3 && (lg < 0 || lg >= ctx->c.vocab_size)) return ctx->fail(NH_ERR_INVALID, "nh_pool_admit: language token outside the vocabulary");
    // nh_pool_prefix: the ids this admission consumes.  Every refusal above and this one leave them pending.
    const int NP = ctx->pool.pending.empty() ? 0 : ctx->pool.pending[dst_row];
    if (NP > 0 && detect) return ctx->fail(NH_ERR_INVALID, "nh_pool_admit: NH_LANG_DETECT into a row with a pending prefix (the probe step behind a prefix is not nh_detect_language's forward)");
    // the route: one ragged pass at the head of the next nh_pool_step, or the pool's own steps from position 0
    const bool onepass = NP >= NH_PREFILL_MIN_PREFIX && !ctx->opt_prompt_stepwise && prefill_supported(ctx);
    hipSetDevice(ctx->dev);
    const size_t per = (size_t)ctx->S * ctx->c.d_model;  // cross K / V of one clip and layer, head-major [h][S][64]
    if (src != ctx) HIPCHK(hipStreamWaitEvent(ctx->st, src->enc_done, 0));   // the other context's encoder ran on its own stream
    for (size_t l = 0; l < ctx->kv.size(); l++) {
        auto &L = ctx->kv[l]; auto &Ls = src->kv[l];
        HIPCHK(hipMemcpyAsync(L.ck + per * dst_row, Ls.ck + per * src_row, per * sizeof(half_t), hipMemcpyDeviceToDevice, ctx->st));
        HIPCHK(hipMemcpyAsync(L.cv + per * dst_row, Ls.cv + per * src_row, per * sizeof(half_t), hipMemcpyDeviceToDevice, ctx->st));
    }
    if (src != ctx) {   // src's next encoder submission waits for these copies
        HIPCHK(hipEventRecord(ctx->kv_copied->e, ctx->st));
        std::lock_guard<std::mutex> lk(src->readers_mu);
        if (std::find(src->kv_readers.begin(), src->kv_readers.end(), ctx->kv_copied) == src->kv_readers.end()) src->kv_readers.push_back(ctx->kv_copied);
    }
    // model.rs:285-289: prompt = [sot, lang?, task]
    const int C = ctx->c.max_target_positions;
    if (NP > 0)   // the ids, verbatim, in front of the prompt: one copy out of the context's pinned buffer
        HIPCHK(hipMemcpyAsync(ctx->ds.tokens + (size_t)dst_row * C, ctx->pfx_host + (size_t)dst_row * (C / 2), sizeof(int32_t) * NP, hipMemcpyHostToDevice, ctx->st));
    launch_pool_admit(ctx->ds, ctx->d_pos, ctx->ltick, dst_row, C, ctx->tk.sot, P == 3 ? lg : ctx->tk.task,
                      ctx->tk.task, P, ctx->st, ctx->d_lang_flag, detect ? 1 : 0, ctx->d_pfx, NP, onepass ? NP : 0);
    HIPCHK(hipGetLastError());
    if (NP > 0) ctx->pool.pending[dst_row] = 0;   // one-shot
    drop_pending_prefill(ctx->pool, dst_row);   // the row names at most one clip of the next ragged pass: this one
    if (onepass) ctx->pool.todo.push_back(PfClip{dst_row, NP, 0, 0});
    row.pfx = NP;
    row.detect = detect; row.detected = false;
    if (row.inv_t_set) {  // an admitted row is greedy (a pool that never retried launches nothing here)
        HIPCHK(hipMemsetAsync(ctx->psamp.inv_t + dst_row, 0, sizeof(float), ctx->st));
        row.inv_t_set = false;
    }
    row.busy = true; row.held = true; row.sampled = false; row.align_gen = -1;
    return NH_OK;
}

// The clip in `row` once more, sampled (the fallback of decode_with_fallback, model.rs:164-191, for one row of a pool): the row
// restarts at position 0 on the cross K/V and the prompt it still holds -- nothing is copied, where an admission copies the
// clip's cross K/V of every layer.  A row with a prefix of n ids restarts at position n, on the self K/V of positions 0 .. n-1
// that its first decode left in the cache: nothing is computed again either.
extern "C" int nh_pool_retry(nh_ctx *ctx, int row, float temperature, uint64_t seed, uint32_t clip, uint32_t attempt) {
    if (!ctx) return NH_ERR_INVALID;
    if (ctx->pool.rows < 1) return ctx->fail(NH_ERR_STATE, "nh_pool_retry: no decode pool (nh_pool_begin)");
    if (row < 0 || row >= ctx->pool.rows) return ctx->fail(NH_ERR_INVALID, "nh_pool_retry: row outside the pool");
    PoolRow &r = ctx->pool.row[row];
    if (r.busy) return ctx->fail(NH_ERR_STATE, "nh_pool_retry: that row is busy (nh_pool_collect hands it back first)");
    if (!r.held) return ctx->fail(NH_ERR_STATE, "nh_pool_retry: no clip was admitted into that row since nh_pool_begin");
    if (!(temperature > 0.f && temperature < INFINITY)) return ctx->fail(NH_ERR_INVALID, "nh_pool_retry: temperature must be > 0 and finite (an admitted row decodes at t = 0)");
    hipSetDevice(ctx->dev);
    launch_pool_retry(ctx->ds, ctx->d_pos, ctx->ltick, ctx->psamp, row, ctx->pool.prompt, 1.0f / temperature, seed, clip, attempt, ctx->st,
                      ctx->d_lang_flag, ctx->d_pfx);
    HIPCHK(hipGetLastError());
    r.busy = true; r.sampled = true; r.inv_t_set = true; r.align_gen = -1;
    return NH_OK;
}

extern "C" int nh_pool_admit(nh_ctx *ctx, int src_row, int dst_row, int32_t lang) {
    if (!ctx) return NH_ERR_INVALID;
    if (ctx->pool.rows < 1) return ctx->fail(NH_ERR_STATE, "nh_pool_admit: no decode pool (nh_pool_begin)");
    if (!ctx->have_enc || src_row < ctx->pool.rows || src_row >= ctx->cur_batch) return ctx->fail(NH_ERR_STATE, "nh_pool_admit: src_row is not an encoded staging row (nh_encode_rows)");
    return pool_admit_impl(ctx, ctx, src_row, dst_row, lang);
}

extern "C" int nh_pool_admit_from(nh_ctx *ctx, nh_ctx *enc, int src_row, int dst_row, int32_t lang) {
    if (!ctx || !enc) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_pool_admit_from: bad arguments") : NH_ERR_INVALID;
    if (enc == ctx) return nh_pool_admit(ctx, src_row, dst_row, lang);
    if (ctx->pool.rows < 1) return ctx->fail(NH_ERR_STATE, "nh_pool_admit_from: no decode pool (nh_pool_begin)");
    if (enc->mdl != ctx->mdl || enc->dev != ctx->dev) return ctx->fail(NH_ERR_INVALID, "nh_pool_admit_from: the encoder context must share this context's weights (nh_create_shared)");
    if (enc->pool.rows > 0) return ctx->fail(NH_ERR_INVALID, "nh_pool_admit_from: the encoder context runs a pool of its own");
    if (!enc->have_enc || src_row < 0 || src_row >= enc->cur_batch) return ctx->fail(NH_ERR_STATE, "nh_pool_admit_from: src_row is not an encoded row of the encoder context (nh_encode / nh_encode_rows)");
    if (ctx->frames < 0) { ctx->frames = enc->frames; ctx->S = enc->S; }   // the pool's clip length is its first clip's
    else if (enc->frames != ctx->frames) return ctx->fail(NH_ERR_INVALID, "all clips of one decode pool must produce the same number of mel frames");
    return pool_admit_impl(ctx, enc, src_row, dst_row, lang);
}

extern "C" int nh_pool_step(nh_ctx *ctx, int n_steps, int32_t *done_out) {
    if (!ctx || !done_out) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_pool_step: bad arguments") : NH_ERR_INVALID;
    if (ctx->pool.rows < 1) return ctx->fail(NH_ERR_STATE, "nh_pool_step: no decode pool (nh_pool_begin)");
    if (n_steps < 0) return ctx->fail(NH_ERR_INVALID, "nh_pool_step: n_steps < 0");
    Pool &pl = ctx->pool;
    const int B = pl.rows;
    hipSetDevice(ctx->dev);
    bool any = false, sampled = false;  // sampled: a busy row is on a retry -- the steps carry pool_sample_step_kernel
    for (const PoolRow &r : pl.row) { any = any || r.busy; sampled = sampled || (r.busy && r.sampled); }
    if (any && n_steps > 0) {
        if (ctx->S < 1) return ctx->fail(NH_ERR_STATE, "nh_pool_step: rows are busy but nothing was ever encoded");
        // the prefixes of the rows admitted since the last one, in ONE ragged pass: eager, ahead of the graph launches, and on
        // this stream behind the admissions' copies of cross K/V and ids.  Those rows stand at their sot already.
        if (!pl.todo.empty()) {
            std::vector<PfClip> todo;
            todo.swap(pl.todo);
            if (int rc = prefill_forward(ctx, 0, nullptr, false, todo.data(), (int)todo.size())) {
                pl.todo.swap(todo);   // refused before anything ran: the prefixes are still owed
                return rc;
            }
        }
        const StepGraphs &g = ctx->graphs[sampled];
        for (int s = 0; ctx->opt_graphs && s <= (int)sampled; s++)   // the greedy pair also when this call replays the sampled one
            if (int rc = ensure_step_graphs(ctx, StepKey{B, ctx->S, pl.max_new, pl.prompt, ctx->token_gen, pl.lang_n, true, s == 1, ctx->live.gen, ctx->guard.gen})) return rc;
        for (int left = n_steps; left > 0;) {
            if (!ctx->opt_graphs) {
                emit_token_step(ctx, StepSpec{B, pl.max_new, pl.prompt, 2, sampled, 0, ctx->d_pos, 0.f, 0, 0, 0});
                left--;
            } else if (left >= NH_GRAPH_STEPS) { HIPCHK(hipGraphLaunch(g.multi, ctx->st)); left -= NH_GRAPH_STEPS; }
            else { HIPCHK(hipGraphLaunch(g.one, ctx->st)); left--; }
        }
        ctx->tm.decode_steps += n_steps;
        for (PoolRow &r : pl.row) if (r.busy && r.detect) r.detected = true;  // its first step is behind it
    }
    HIPCHK(hipMemcpyAsync(ctx->h_done, ctx->ds.done, B * 4, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipGetLastError());
    for (int b = 0; b < B; b++) done_out[b] = pl.row[b].busy ? ctx->h_done[b] : 3;
    return NH_OK;
}

extern "C" int nh_pool_collect(nh_ctx *ctx, const int32_t *rows, int n, int32_t *out_tokens, nh_decode_result *results) {
    if (!ctx || !rows || !out_tokens || !results || n < 1) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_pool_collect: bad arguments") : NH_ERR_INVALID;
    if (ctx->pool.rows < 1) return ctx->fail(NH_ERR_STATE, "nh_pool_collect: no decode pool (nh_pool_begin)");
    for (int i = 0; i < n; i++)
        if (rows[i] < 0 || rows[i] >= ctx->pool.rows || !ctx->pool.row[rows[i]].busy) return ctx->fail(NH_ERR_INVALID, "nh_pool_collect: not a busy row of the pool");
    hipSetDevice(ctx->dev);
    if (int rc = read_results(ctx, rows, n, out_tokens, results)) return rc;
    // heads cannot change while a row is busy (nh_align_capture refuses), so the whole decode ran under the current list
    for (int i = 0; i < n; i++) drop_pending_prefill(ctx->pool, rows[i]);
    for (int i = 0; i < n; i++) { PoolRow &r = ctx->pool.row[rows[i]]; r.busy = false; r.sampled = false; r.align_gen = kept_heads(ctx) ? ctx->live.gen : -1; }
    return NH_OK;
}

// The pool's language table.  The step graphs bake the table's size in (PoolDetect::n goes by value) and whether the
// detection kernel is part of a step at all, so the table changes only while no row is busy, and its size is in the graph key.
extern "C" int nh_pool_detect_languages(nh_ctx *ctx, const int32_t *lang_tokens, int n) {
    if (!ctx) return NH_ERR_INVALID;
    if (ctx->pool.rows < 1) return ctx->fail(NH_ERR_STATE, "nh_pool_detect_languages: no decode pool (nh_pool_begin)");
    if (!ctx->pool.per_clip_language) return ctx->fail(NH_ERR_INVALID, "nh_pool_detect_languages: the pool was begun without per-clip languages");
    if (!lang_tokens || n < 1 || n > 256) return ctx->fail(NH_ERR_INVALID, "nh_pool_detect_languages: bad arguments (1 <= n <= 256)");
    for (int i = 0; i < n; i++)
        if (lang_tokens[i] < 0 || lang_tokens[i] >= ctx->c.vocab_size) return ctx->fail(NH_ERR_INVALID, "nh_pool_detect_languages: token id outside the vocabulary");
    for (const PoolRow &r : ctx->pool.row)
        if (r.busy) return ctx->fail(NH_ERR_STATE, "nh_pool_detect_languages: rows are busy (the table is part of the captured steps)");
    hipSetDevice(ctx->dev);
    HIPCHK(hipMemcpyAsync(ctx->d_lang_tokens, lang_tokens, n * 4, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));  // lang_tokens is the caller's
    ctx->pool.lang_n = n;
    // languages detected under another table are no longer answered for (nh_pool_languages)
    for (PoolRow &r : ctx->pool.row) r.detect = r.detected = false;
    return NH_OK;
}

extern "C" int nh_pool_languages(nh_ctx *ctx, const int32_t *rows, int n_rows, int32_t *out_lang, float *out_probs) {
    if (!ctx || !rows || !out_lang || n_rows < 1) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_pool_languages: bad arguments") : NH_ERR_INVALID;
    if (ctx->pool.rows < 1) return ctx->fail(NH_ERR_STATE, "nh_pool_languages: no decode pool (nh_pool_begin)");
    for (int i = 0; i < n_rows; i++) {
        if (rows[i] < 0 || rows[i] >= ctx->pool.rows) return ctx->fail(NH_ERR_INVALID, "nh_pool_languages: row outside the pool");
        if (!ctx->pool.row[rows[i]].detect) return ctx->fail(NH_ERR_STATE, "nh_pool_languages: that row's clip was not admitted with NH_LANG_DETECT");
        if (!ctx->pool.row[rows[i]].detected) return ctx->fail(NH_ERR_STATE, "nh_pool_languages: that row has not taken a step since it was admitted (nh_pool_step)");
    }
    hipSetDevice(ctx->dev);
    const int n = ctx->pool.lang_n;
    std::vector<int32_t> lang(ctx->pool.rows);
    HIPCHK(hipMemcpyAsync(lang.data(), ctx->d_lang_out, sizeof(int32_t) * ctx->pool.rows, hipMemcpyDeviceToHost, ctx->st));
    if (out_probs)
        for (int i = 0; i < n_rows; i++)
            HIPCHK(hipMemcpyAsync(out_probs + (size_t)i * n, ctx->d_lang_probs + (size_t)rows[i] * 256, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    for (int i = 0; i < n_rows; i++) out_lang[i] = lang[rows[i]];
    return NH_OK;
}

extern "C" int nh_sample_rules(nh_ctx *ctx, const float *probs, const int32_t *tokens, int n_tokens, int last_timestamp,
                               float temperature, uint64_t seed, uint32_t clip, uint32_t attempt, int32_t *token_out) {
    if (!ctx || !probs || !tokens || !token_out || n_tokens < 1 || !(temperature > 0.f))
        return ctx ? ctx->fail(NH_ERR_INVALID, "nh_sample_rules: bad arguments") : NH_ERR_INVALID;
    if (!ctx->have_tokens) return ctx->fail(NH_ERR_STATE, "nh_sample_rules: call nh_set_tokens first");
    hipSetDevice(ctx->dev);
    const int V = ctx->c.vocab_size;
    HIPCHK(hipMemcpyAsync(ctx->logits, probs, sizeof(float) * V, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(ctx->ds.tokens, tokens, sizeof(int32_t) * n_tokens, hipMemcpyHostToDevice, ctx->st));
    launch_sample_rules(ctx->logits, ctx->ds.n_active, ctx->ds.tokens, n_tokens, last_timestamp, ctx->suppress, ctx->tk, V,
                        1.0f / temperature, seed, clip, attempt, ctx->st);
    HIPCHK(hipMemcpyAsync(token_out, ctx->ds.n_active, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipGetLastError());
    return NH_OK;
}

extern "C" int nh_set_languages(nh_ctx *ctx, const int32_t *langs) {
    if (!ctx) return NH_ERR_INVALID;
    ctx->seq_lang.clear();
    if (langs) {
        for (int b = 0; b < ctx->cur_batch; b++) {
            if (langs[b] < 0 || langs[b] >= ctx->c.vocab_size) { ctx->seq_lang.clear(); return ctx->fail(NH_ERR_INVALID, "nh_set_languages: token id outside the vocabulary"); }
            ctx->seq_lang.push_back(langs[b]);
        }
    }
    return NH_OK;
}

extern "C" int nh_detect_language(nh_ctx *ctx, const int32_t *lang_tokens, int n, int32_t *out_lang, float *out_probs) {
    if (!ctx || !lang_tokens || !out_lang || n < 1 || n > 256) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_detect_language: bad arguments (1 <= n <= 256)") : NH_ERR_INVALID;
    // the probe overwrites tokens and self-K/V of rows [0, cur_batch): the busy rows of a pool would decode on from that
    // (a pool detects languages on its encoder contexts: nh_pool_admit_from takes the language per row)
    if (ctx->pool.rows > 0) return ctx->fail(NH_ERR_STATE, "nh_detect_language: the context runs a decode pool (nh_pool_begin)");
    if (!ctx->have_enc) return ctx->fail(NH_ERR_STATE, "nh_detect_language: call nh_encode first");
    if (!ctx->have_tokens) return ctx->fail(NH_ERR_STATE, "nh_detect_language: call nh_set_tokens first");
    const int B = ctx->cur_batch, V = ctx->c.vocab_size;
    for (int i = 0; i < n; i++) if (lang_tokens[i] < 0 || lang_tokens[i] >= V) return ctx->fail(NH_ERR_INVALID, "nh_detect_language: token id outside the vocabulary");
    // tokens = [[sot]], model.rs:195: every clip the same one token
    if (int rc = stage_given_tokens(ctx, "nh_detect_language", &ctx->tk.sot, 0, 1)) return rc;
    HIPCHK(hipMemcpyAsync(ctx->d_lang_tokens, lang_tokens, n * 4, hipMemcpyHostToDevice, ctx->st));   // the caller's, read before the drain below
    decoder_step(ctx, 0);
    logits_from_dxn(ctx, B);
    launch_lang_detect(ctx->logits, V, ctx->d_lang_tokens, n, out_probs ? ctx->d_lang_probs : nullptr, ctx->d_lang_out, B, ctx->st);
    HIPCHK(hipMemcpyAsync(out_lang, ctx->d_lang_out, B * 4, hipMemcpyDeviceToHost, ctx->st));
    if (out_probs) HIPCHK(hipMemcpyAsync(out_probs, ctx->d_lang_probs, (size_t)B * n * 4, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipGetLastError());
    ctx->seq_lang.assign(out_lang, out_lang + B);
    return NH_OK;
}

extern "C" int nh_transcribe_batch(nh_ctx *ctx, const float *pcm_dev, const int32_t *n_samples, int64_t stride, int batch,
                                   int32_t *out_tokens, nh_decode_result *results, int max_new_tokens) {
    int rc = nh_logmel_device(ctx, pcm_dev, n_samples, stride, batch);
    if (rc) return rc;
    if ((rc = nh_encode(ctx))) return rc;
    return nh_decode_greedy(ctx, out_tokens, results, max_new_tokens);
}

int stage_given_tokens(nh_ctx *ctx, const char *who, const int32_t *tokens, size_t stride, int n_all, const int32_t *n_each) {
    const int B = ctx->cur_batch, C = ctx->c.max_target_positions, V = ctx->c.vocab_size;
    std::vector<int32_t> toks((size_t)B * C, 0);
    for (int b = 0; b < B; b++) {
        const int n = n_each ? n_each[b] : n_all;
        for (int i = 0; i < n; i++) {
            const int32_t t = tokens[(size_t)b * stride + i];
            if (t < 0 || t >= V) return ctx->fail(NH_ERR_INVALID, std::string(who) + ": token id outside the vocabulary");
            toks[(size_t)b * C + i] = t;
        }
    }
    hipSetDevice(ctx->dev);
    if (int rc = ensure_decoder_repack(ctx)) return rc;
    HIPCHK(hipStreamWaitEvent(ctx->st, ctx->enc_done, 0));
    ctx->live.lock_valid = false;   // the tokens, and the self K/V the caller's pass writes next, replace what the last decode left
    HIPCHK(hipMemcpyAsync(ctx->ds.tokens, toks.data(), toks.size() * 4, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));   // toks is a local
    return NH_OK;
}

extern "C" int nh_decoder_forward(nh_ctx *ctx, const int32_t *tokens, int T, float *hidden_out) {
    if (!ctx || !tokens || !hidden_out) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_decoder_forward: bad arguments") : NH_ERR_INVALID;
    if (ctx->pool.rows > 0) return ctx->fail(NH_ERR_STATE, "nh_decoder_forward: the context runs a decode pool (nh_pool_begin)");
    if (!ctx->have_enc) return ctx->fail(NH_ERR_STATE, "nh_decoder_forward: call nh_encode first");
    const int B = ctx->cur_batch, C = ctx->c.max_target_positions, d = ctx->c.d_model;
    if (T < 1 || T > C) return ctx->fail(NH_ERR_INVALID, "nh_decoder_forward: T out of range");
    if (int rc = stage_given_tokens(ctx, "nh_decoder_forward", tokens, T, T)) return rc;
    std::vector<float> row((size_t)B * d);
    for (int pos = 0; pos < T; pos++) {
        decoder_step(ctx, pos);
        HIPCHK(hipMemcpyAsync(row.data(), ctx->dy32, row.size() * 4, hipMemcpyDeviceToHost, ctx->st));
        HIPCHK(hipStreamSynchronize(ctx->st));
        for (int b = 0; b < B; b++) memcpy(hidden_out + ((size_t)b * T + pos) * d, row.data() + (size_t)b * d, sizeof(float) * d);
    }
    HIPCHK(hipGetLastError());
    return NH_OK;
}

extern "C" int nh_final_linear(nh_ctx *ctx, const float *x, int rows, float *logits_out) {
    if (!ctx || !x || !logits_out) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_final_linear: bad arguments") : NH_ERR_INVALID;
    if (rows < 1) return ctx->fail(NH_ERR_INVALID, "nh_final_linear: rows must be >= 1");
    hipSetDevice(ctx->dev);
    if (int rc = ensure_decoder_repack(ctx)) return rc;
    const int d = ctx->c.d_model, V = ctx->c.vocab_size;
    std::vector<_Float16> h((size_t)ctx->B * d);
    for (int r0 = 0; r0 < rows; r0 += ctx->B) {  // the workspace holds max_batch rows at a time
        const int nr = rows - r0 < ctx->B ? rows - r0 : ctx->B;
        for (size_t i = 0; i < (size_t)nr * d; i++) h[i] = (_Float16)x[(size_t)r0 * d + i];
        HIPCHK(hipMemcpyAsync(ctx->dxn, h.data(), (size_t)nr * d * 2, hipMemcpyHostToDevice, ctx->st));
        HIPCHK(hipStreamSynchronize(ctx->st));
        logits_from_dxn(ctx, nr);
        for (int r = 0; r < nr; r++)
            HIPCHK(hipMemcpyAsync(logits_out + (size_t)(r0 + r) * V, ctx->logits + (size_t)r * ctx->VP, sizeof(float) * V,
                                  hipMemcpyDeviceToHost, ctx->st));
        HIPCHK(hipStreamSynchronize(ctx->st));
    }
    HIPCHK(hipGetLastError());
    return NH_OK;
}

extern "C" int nh_apply_rules(nh_ctx *ctx, const float *probs, const int32_t *tokens, int n_tokens, int last_timestamp,
                              float *masked_out, int32_t *argmax_out) {
    if (!ctx || !probs || !tokens || !masked_out || !argmax_out || n_tokens < 1)
        return ctx ? ctx->fail(NH_ERR_INVALID, "nh_apply_rules: bad arguments") : NH_ERR_INVALID;
    if (!ctx->have_tokens) return ctx->fail(NH_ERR_STATE, "nh_apply_rules: call nh_set_tokens first");
    hipSetDevice(ctx->dev);
    const int V = ctx->c.vocab_size;
    float *d_in = ctx->logits, *d_out = ctx->logits + ctx->VP * (ctx->B > 1 ? 1 : 0);
    DevBuf tmp_out;   // a max_batch 1 context has no second row of logits
    if (ctx->B == 1) {
        if (int rc = tmp_out.reserve(ctx, sizeof(float) * V, "masked row")) return rc;
        d_out = tmp_out.at<float>();
    }
    int32_t *d_tok = ctx->ds.tokens;
    HIPCHK(hipMemcpyAsync(d_in, probs, sizeof(float) * V, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(d_tok, tokens, sizeof(int32_t) * n_tokens, hipMemcpyHostToDevice, ctx->st));
    launch_rules_only(d_in, d_out, ctx->ds.n_active, d_tok, n_tokens, last_timestamp, ctx->suppress, ctx->tk, V, ctx->st);
    HIPCHK(hipMemcpyAsync(masked_out, d_out, sizeof(float) * V, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(argmax_out, ctx->ds.n_active, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipGetLastError());
    return NH_OK;
}
