// nh_encode.hip -- the C ABI of include/norma_hip.h, part 2: log-mel and encoder, sequenced on the context's stream.
#include "nh_ctx.h"

static long mel_frames_for(long n) {  // candle pcm_to_mel frame count (SURVEY.md 3.3[A]-2)
    long n_len = n / 160, pad = 1500;
    if (n_len % pad != 0) n_len = (n_len / pad + 1) * pad;
    return n_len + pad;
}

// the zero rows framing each clip in the conv inputs move with the frame count
static int reframe(nh_ctx *ctx) {
    if (ctx->frames == ctx->last_frames) return NH_OK;
    HIPCHK(hipMemsetAsync(ctx->mel_img, 0, sizeof(half_t) * (size_t)ctx->B * (NH_N_FRAMES + 2) * NH_MELP, ctx->st));
    HIPCHK(hipMemsetAsync(ctx->h1, 0, sizeof(half_t) * (size_t)ctx->B * (NH_N_FRAMES + 2) * ctx->c.d_model, ctx->st));
    ctx->last_frames = ctx->frames;
    return NH_OK;
}

// ---- log-mel -------------------------------------------------------------------------------------------
static int clip_mel_frames(int n_samples) {   // narrow(2, 0, min(3000, frames)), model.rs:88
    const long f = mel_frames_for(n_samples);
    return f > NH_N_FRAMES ? NH_N_FRAMES : (int)f;
}

// row0 > 0: the clips join the rows already filled (several encoder batches of one joint decode, nh_logmel_device_rows)
int check_batch(nh_ctx *ctx, const int32_t *n_samples, int batch, int row0) {
    if (batch < 1 || row0 < 0 || row0 + batch > ctx->B) return ctx->fail(NH_ERR_INVALID, "rows [row0, row0 + batch) must lie in [0, max_batch]");
    for (int b = 0; b < batch; b++) {
        if (n_samples[b] < 1 || n_samples[b] > NH_N_SAMPLES)
            return ctx->fail(NH_ERR_INVALID, "clip length must be in [1, 480000] samples");
        if (clip_mel_frames(n_samples[b]) != clip_mel_frames(n_samples[0]))
            return ctx->fail(NH_ERR_INVALID, "clips of one batch must produce the same number of mel frames");
    }
    const int fr = clip_mel_frames(n_samples[0]);
    if (ctx->pool.rows > 0 && row0 >= ctx->pool.rows) {  // decode pool: encoder staging rows above the decoding ones
        if (ctx->frames >= 0 && fr != ctx->frames) return ctx->fail(NH_ERR_INVALID, "all clips of one decode pool must produce the same number of mel frames");
    } else if (row0 > 0) {
        if (row0 > ctx->cur_batch) return ctx->fail(NH_ERR_STATE, "row0 leaves a gap after the rows filled so far");
        if (fr != ctx->frames) return ctx->fail(NH_ERR_INVALID, "all rows of one joint decode must produce the same number of mel frames");
    }
    return NH_OK;
}

// an accepted batch (check_batch) becomes the context's
static int commit_batch(nh_ctx *ctx, const int32_t *n_samples, int batch, int row0) {
    const int fr = clip_mel_frames(n_samples[0]);
    ctx->live.lock_valid = false;   // a lockstep decode's captured sequences (nh_align_decoded) end with the batch they belong to
    ctx->have_enc = false;
    if (row0 > 0) {   // pool staging rows or the next rows of a joint decode
        if (row0 + batch > ctx->cur_batch) ctx->cur_batch = row0 + batch;
        if (ctx->frames >= 0) return NH_OK;
        ctx->frames = fr; ctx->S = (fr + 2 - 3) / 2 + 1;   // the first clips of a pool set its frame count
        return reframe(ctx);
    }
    ctx->cur_batch = batch; ctx->frames = fr; ctx->S = (fr + 2 - 3) / 2 + 1;
    ctx->have_mel = false;
    ctx->pool.rows = 0;  // a fresh batch ends a decode pool
    ctx->seq_lang.clear();
    clear_prompt(ctx);   // a prefix belongs to the batch it was set for (nh_set_prompts)
    return reframe(ctx);
}

int run_logmel(nh_ctx *ctx, const float *pcm_dev, const int32_t *n_samples, int64_t stride, int batch, int row0) {
    if (int rc = commit_batch(ctx, n_samples, batch, row0)) return rc;
    const int nm = ctx->c.num_mel_bins;
    int32_t *nsamp = ctx->nsamp + row0;
    unsigned *cmax = ctx->chunk_max + row0;
    float *mel32 = ctx->mel32 + (size_t)row0 * nm * ctx->frames;
    half_t *img = ctx->mel_img + (size_t)row0 * (ctx->frames + 2) * NH_MELP;
    HIPCHK(hipMemcpyAsync(nsamp, n_samples, sizeof(int32_t) * batch, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->st));
    HIPCHK(hipMemsetAsync(cmax, 0, sizeof(unsigned) * batch, ctx->st));
    launch_logmel_grp(pcm_dev, nsamp, stride, ctx->mdl->mt, ctx->mdl->mel_grp, nm, ctx->frames, mel32, cmax, batch, ctx->st);
    launch_mel_finish_ex(mel32, cmax, img, batch, nm, ctx->frames, 1, ctx->st);
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->st));
    HIPCHK(hipGetLastError());
    ctx->have_mel = true;
    return NH_OK;
}

// nh_logmel, nh_logmel_rows and their _device forms after the pointer checks: every refusal, then (host PCM) the copies
// into the PCM rows, then the log-mel
static int logmel_rows(nh_ctx *ctx, const float *pcm, bool on_device, const int32_t *n_samples, int64_t stride, int batch, int row0) {
    hipSetDevice(ctx->dev);
    if (!ctx->mdl->have_filters) return ctx->fail(NH_ERR_STATE, "nh_logmel: mel filters not set");
    if (int rc = check_batch(ctx, n_samples, batch, row0)) return rc;
    if (on_device) return run_logmel(ctx, pcm, n_samples, stride, batch, row0);
    float *dst = ctx->pcm + (size_t)row0 * NH_N_SAMPLES;
    for (int b = 0; b < batch; b++)
        HIPCHK(hipMemcpyAsync(dst + (size_t)b * NH_N_SAMPLES, pcm + (size_t)b * stride, sizeof(float) * n_samples[b],
                              hipMemcpyHostToDevice, ctx->st));
    return run_logmel(ctx, dst, n_samples, NH_N_SAMPLES, batch, row0);
}

extern "C" int nh_logmel_device_rows(nh_ctx *ctx, const float *pcm_dev, const int32_t *n_samples, int64_t stride, int batch, int row0) {
    if (!ctx || !pcm_dev || !n_samples) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_logmel_device_rows: bad arguments") : NH_ERR_INVALID;
    return logmel_rows(ctx, pcm_dev, true, n_samples, stride, batch, row0);
}

extern "C" int nh_logmel_device(nh_ctx *ctx, const float *pcm_dev, const int32_t *n_samples, int64_t stride, int batch) {
    if (!ctx || !pcm_dev || !n_samples) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_logmel_device: bad arguments") : NH_ERR_INVALID;
    return logmel_rows(ctx, pcm_dev, true, n_samples, stride, batch, 0);
}

extern "C" int nh_logmel(nh_ctx *ctx, const float *pcm, const int32_t *n_samples, int64_t stride, int batch) {
    if (!ctx || !pcm || !n_samples) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_logmel: bad arguments") : NH_ERR_INVALID;
    return logmel_rows(ctx, pcm, false, n_samples, stride, batch, 0);
}

extern "C" int nh_logmel_rows(nh_ctx *ctx, const float *pcm, const int32_t *n_samples, int64_t stride, int batch, int row0) {
    if (!ctx || !pcm || !n_samples) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_logmel_rows: bad arguments") : NH_ERR_INVALID;
    return logmel_rows(ctx, pcm, false, n_samples, stride, batch, row0);
}

extern "C" int nh_get_mel(nh_ctx *ctx, int b, float *out) {
    if (!ctx || !out) return NH_ERR_INVALID;
    if (!ctx->have_mel || b < 0 || b >= ctx->cur_batch) return ctx->fail(NH_ERR_STATE, "nh_get_mel: no mel for that clip");
    hipSetDevice(ctx->dev);
    size_t per = (size_t)ctx->c.num_mel_bins * ctx->frames;
    HIPCHK(hipMemcpyAsync(out, ctx->mel32 + per * b, per * 4, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    return NH_OK;
}

extern "C" int nh_set_mel(nh_ctx *ctx, const float *mel, int batch) {
    if (!ctx || !mel) return NH_ERR_INVALID;
    hipSetDevice(ctx->dev);
    std::vector<int32_t> ns(batch > 0 ? batch : 1, NH_N_SAMPLES);
    if (int rc = check_batch(ctx, ns.data(), batch)) return rc;
    if (int rc = commit_batch(ctx, ns.data(), batch, 0)) return rc;
    size_t per = (size_t)ctx->c.num_mel_bins * NH_N_FRAMES;
    HIPCHK(hipMemcpyAsync(ctx->mel32, mel, per * batch * 4, hipMemcpyHostToDevice, ctx->st));
    launch_mel_finish_ex(ctx->mel32, ctx->chunk_max, ctx->mel_img, batch, ctx->c.num_mel_bins, ctx->frames, 0, ctx->st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->st));
    ctx->have_mel = true;
    return NH_OK;
}

// ---- encoder ---------------------------------------------------------------------------------------------
static void gemm_prof_begin(nh_ctx *ctx) {
    if (!ctx->profile_gemm) return;
    if (ctx->gemm_ev_used + 2 > ctx->gemm_ev.size()) {
        for (int i = 0; i < 64; i++) { hipEvent_t e; hipEventCreate(&e); ctx->gemm_ev.push_back(e); }
    }
    hipEventRecord(ctx->gemm_ev[ctx->gemm_ev_used], ctx->st);
}
static void gemm_prof_end(nh_ctx *ctx, const GemmParams &p) {
    if (!ctx->profile_gemm) return;
    hipEventRecord(ctx->gemm_ev[ctx->gemm_ev_used + 1], ctx->st);
    ctx->gemm_ev_used += 2;
    ctx->gemm_flops_acc += 2.0 * (double)p.M * (double)p.N * (double)p.K;
}

static void gemm_plain(nh_ctx *ctx, const half_t *A, long lda, const LinW &W, int M, int N, int K, int epi, void *o0,
                       void *o1, void *o2, int seg_n, long ldo, int vt_seg, int head_major = 0, float seg0_scale = 0.f) {
    GemmParams p{};
    p.head_major = head_major; p.seg0_scale = seg0_scale;
    p.A = A; p.lda = lda; p.a_rpb = M; p.a_bstride = 0; p.W = W.w; p.bias = W.b; p.M = M; p.N = N; p.K = K; p.epi = epi;
    p.out[0] = o0; p.out[1] = o1; p.out[2] = o2; p.seg_n = seg_n; p.ldo = ldo; p.o_rpb = M; p.o_bstride = 0; p.o_off = 0;
    p.vt_seg = vt_seg; p.S = ctx->S; p.H = ctx->c.encoder_attention_heads; p.pos = nullptr;
    gemm_prof_begin(ctx);
    launch_gemm(p, ctx->st);
    gemm_prof_end(ctx, p);
}

// Type::encoder_forward + the cross K/V of every decoder layer for the clips in rows [row0, row0 + B) of the context
static int encode_rows(nh_ctx *ctx, int row0, int B) {
    if (!ctx->have_mel) return ctx->fail(NH_ERR_STATE, "nh_encode: call nh_logmel first");
    if (nh_missing_tensors(ctx) != 0) return ctx->fail(NH_ERR_STATE, "nh_encode: " + std::to_string(nh_missing_tensors(ctx)) + " tensors not loaded");
    if (row0 < 0 || B < 1 || row0 + B > ctx->cur_batch) return ctx->fail(NH_ERR_INVALID, "nh_encode_rows: rows outside the clips given to nh_logmel");
    hipSetDevice(ctx->dev);
    ctx->live.lock_valid = false;
    const nh_model &m = *ctx->mdl;
    const int d = ctx->c.d_model, F = ctx->frames, S = ctx->S, H = ctx->c.encoder_attention_heads;
    const int M = B * S;
    const size_t r0 = (size_t)row0;
    // this group's slices of the per-clip workspaces
    half_t *const mel_img = ctx->mel_img + r0 * (F + 2) * NH_MELP, *const h1 = ctx->h1 + r0 * (F + 2) * d;
    float *const x = ctx->x + r0 * S * d, *const xa32 = ctx->xa32 + r0 * S * d;
    half_t *const xn = ctx->xn + r0 * S * d, *const q = ctx->q + r0 * S * d, *const k = ctx->k + r0 * S * d, *const att = ctx->att + r0 * S * d;
    half_t *const vt = ctx->vt + r0 * d * NH_SP, *const hid = ctx->hid + r0 * S * 4 * d, *const xa16 = ctx->xa16 + r0 * S * d;
    ctx->gemm_ev_used = 0; ctx->gemm_flops_acc = 0.0;
    {   // decode pools of other contexts that are still copying K/V out of these rows (nh_pool_admit_from) go first
        std::lock_guard<std::mutex> lk(ctx->readers_mu), cap(ctx->mdl->capture_mu);
        for (auto &e : ctx->kv_readers) HIPCHK(hipStreamWaitEvent(ctx->st, e->e, 0));
        ctx->kv_readers.clear();
    }
    HIPCHK(hipEventRecord(ctx->ev[2], ctx->st));
    {   // conv1 + GELU: A rows overlap (lda = 128, K = 3 * 128) inside the zero-framed mel image
        GemmParams p{};
        p.A = mel_img; p.lda = NH_MELP; p.a_rpb = F; p.a_bstride = (long)(F + 2) * NH_MELP;
        p.W = m.conv1.w; p.bias = m.conv1.b; p.M = B * F; p.N = d; p.K = 3 * NH_MELP; p.epi = EPI_GELU_F16;
        p.out[0] = h1; p.seg_n = d; p.ldo = d; p.o_rpb = F; p.o_bstride = F + 2; p.o_off = 1; p.vt_seg = -1;
        p.S = S; p.H = H;
        gemm_prof_begin(ctx); launch_gemm(p, ctx->st); gemm_prof_end(ctx, p);
    }
    {   // conv2 (stride 2) + GELU + transpose + sinusoid positions -> f32 residual stream
        GemmParams p{};
        p.A = h1; p.lda = 2L * d; p.a_rpb = S; p.a_bstride = (long)(F + 2) * d;
        p.W = m.conv2.w; p.bias = m.conv2.b; p.M = M; p.N = d; p.K = 3 * d; p.epi = EPI_CONV2_F32;
        p.out[0] = x; p.seg_n = d; p.ldo = d; p.o_rpb = M; p.o_bstride = 0; p.o_off = 0; p.vt_seg = -1;
        p.S = S; p.H = H; p.pos = m.enc_pos;
        gemm_prof_begin(ctx); launch_gemm(p, ctx->st); gemm_prof_end(ctx, p);
    }
    for (auto &L : m.enc) {
        launch_layernorm(x, L.ln1.w, L.ln1.b, xn, nullptr, M, d, ctx->st);
        // q leaves the GEMM as (x W_q + b_q) * dh^-1/2 * log2(e): candle's q * dh^-1/4 and k * dh^-1/4 and the
        // exp -> exp2 change of base, applied once in f32 before the one rounding to fp16 (k_attn_enc.hip)
        gemm_plain(ctx, xn, d, L.qkv, M, 3 * d, d, EPI_F16, q, k, vt, d, d, 2, 0, NH_ENC_Q_SCALE);
        launch_enc_attention(q, k, d, vt, att, d, B, S, H, ctx->st);
        gemm_plain(ctx, att, d, L.o, M, d, d, EPI_RESID_F32, x, nullptr, nullptr, d, d, -1);
        launch_layernorm(x, L.ln2.w, L.ln2.b, xn, nullptr, M, d, ctx->st);
        gemm_plain(ctx, xn, d, L.fc1, M, 4 * d, d, EPI_GELU_F16, hid, nullptr, nullptr, 4 * d, 4 * d, -1);
        gemm_plain(ctx, hid, 4 * d, L.fc2, M, d, 4 * d, EPI_RESID_F32, x, nullptr, nullptr, d, d, -1);
    }
    launch_layernorm(x, m.ln_post.w, m.ln_post.b, xa16, xa32, M, d, ctx->st);
    HIPCHK(hipEventRecord(ctx->ev[3], ctx->st));
    // cross-attention K/V of every decoder layer (the flush = true work of MultiHeadAttention::forward), head-major
    // [b][h][S][64]: clip row0 starts at row0 * S * d
    for (size_t l = 0; l < m.dec.size(); l++)
        gemm_plain(ctx, xa16, d, m.dec[l].ckv, M, 2 * d, d, EPI_F16, ctx->kv[l].ck + r0 * S * d, ctx->kv[l].cv + r0 * S * d, nullptr, d, d, -1, 1);
    HIPCHK(hipEventRecord(ctx->ev[4], ctx->st));
    HIPCHK(hipEventRecord(ctx->enc_done, ctx->st));
    HIPCHK(hipGetLastError());
    ctx->have_enc = true;
    return NH_OK;
}

extern "C" int nh_encode(nh_ctx *ctx) {
    if (!ctx) return NH_ERR_INVALID;
    return encode_rows(ctx, 0, ctx->cur_batch);
}

extern "C" int nh_encode_rows(nh_ctx *ctx, int row0, int batch) {
    if (!ctx) return NH_ERR_INVALID;
    return encode_rows(ctx, row0, batch);
}

extern "C" int nh_encoder_output(nh_ctx *ctx, int b, float *out) {
    if (!ctx || !out) return NH_ERR_INVALID;
    if (!ctx->have_enc || b < 0 || b >= ctx->cur_batch) return ctx->fail(NH_ERR_STATE, "nh_encoder_output: no encoder output for that clip");
    hipSetDevice(ctx->dev);
    size_t per = (size_t)ctx->S * ctx->c.d_model;
    HIPCHK(hipMemcpyAsync(out, ctx->xa32 + per * b, per * 4, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    return NH_OK;
}
