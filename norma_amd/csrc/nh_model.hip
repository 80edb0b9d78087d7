// nh_model.hip -- the C ABI of include/norma_hip.h, part 1: the device state of one Whisper model on one MI355X (weights in fp16,
// f32 LayerNorm/bias parameters) and of its contexts (workspaces for `max_batch` 30-second clips); tokens, options, timings.
#include "nh_ctx.h"
#include "mel_host.h"

// message of the last failed nh_create on THIS thread (contexts are created from one thread per GPU)
static thread_local std::string g_create_error;

// ---- expected tensor names (the set candle reads) ---------------------------------
static void add_lin(std::set<std::string> &s, const std::string &p, bool bias = true) {
    s.insert(p + ".weight");
    if (bias) s.insert(p + ".bias");
}
static void add_attn(std::set<std::string> &s, const std::string &p) {
    add_lin(s, p + ".q_proj"); add_lin(s, p + ".k_proj", false); add_lin(s, p + ".v_proj"); add_lin(s, p + ".out_proj");
}
static void build_expected(nh_model *m) {
    auto &s = m->expected;
    add_lin(s, "model.encoder.conv1"); add_lin(s, "model.encoder.conv2");
    for (int i = 0; i < m->c.encoder_layers; i++) {
        std::string p = "model.encoder.layers." + std::to_string(i);
        add_attn(s, p + ".self_attn"); add_lin(s, p + ".self_attn_layer_norm");
        add_lin(s, p + ".fc1"); add_lin(s, p + ".fc2"); add_lin(s, p + ".final_layer_norm");
    }
    add_lin(s, "model.encoder.layer_norm");
    s.insert("model.decoder.embed_tokens.weight"); s.insert("model.decoder.embed_positions.weight");
    for (int i = 0; i < m->c.decoder_layers; i++) {
        std::string p = "model.decoder.layers." + std::to_string(i);
        add_attn(s, p + ".self_attn"); add_lin(s, p + ".self_attn_layer_norm");
        add_attn(s, p + ".encoder_attn"); add_lin(s, p + ".encoder_attn_layer_norm");
        add_lin(s, p + ".fc1"); add_lin(s, p + ".fc2"); add_lin(s, p + ".final_layer_norm");
    }
    add_lin(s, "model.decoder.layer_norm");
}

extern "C" int nh_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" const char *nh_last_error(const nh_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

nh_ctx::~nh_ctx() {
    hipSetDevice(dev);
    if (st) hipStreamSynchronize(st);
    drop_graphs(this);
    for (auto &e : ev) if (e) hipEventDestroy(e);
    for (auto &e : gemm_ev) hipEventDestroy(e);
    if (enc_done) hipEventDestroy(enc_done);
    if (h_done) hipHostFree(h_done);
    if (pfx_host) hipHostFree(pfx_host);
    if (st) hipStreamDestroy(st);
}   // ... then the arena and every DevBuf free themselves, and the last context of a model frees its weights (~nh_model)

extern "C" void nh_destroy(nh_ctx *ctx) { delete ctx; }

static bool build_mel_tables(nh_model *m, std::string &err) {
    // host tables with libm, the same f32 expressions candle evaluates (mel_host.h, see k_mel.hip)
    std::vector<float> hann(MEL_N_HANN), dc(MEL_N_DFT), dsn(MEL_N_DFT), twc(MEL_N_TW), tws(MEL_N_TW);
    mel_host_tables(hann.data(), dc.data(), dsn.data(), twc.data(), tws.data());
    float *d_h = m->allocs.dalloc_into<float>(400), *d_dc = m->allocs.dalloc_into<float>(625), *d_ds = m->allocs.dalloc_into<float>(625);
    float *d_tc = m->allocs.dalloc_into<float>(375), *d_ts = m->allocs.dalloc_into<float>(375);
    if (!d_h || !d_dc || !d_ds || !d_tc || !d_ts) { err = "hipMalloc(mel tables)"; return false; }
    if (hipMemcpy(d_h, hann.data(), 400 * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_dc, dc.data(), 625 * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_ds, dsn.data(), 625 * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_tc, twc.data(), 375 * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_ts, tws.data(), 375 * 4, hipMemcpyHostToDevice) != hipSuccess) { err = "hipMemcpy(mel tables)"; return false; }
    m->mt.hann = d_h; m->mt.dft_cos = d_dc; m->mt.dft_sin = d_ds; m->mt.tw_cos = d_tc; m->mt.tw_sin = d_ts;
    return true;
}

// the weight tables of one model on one device (zero-filled until nh_load_tensor fills them)
static std::shared_ptr<nh_model> build_model(int device_ordinal, const nh_config *cfg, std::string &err, int &code) {
    auto m = std::make_shared<nh_model>();
    m->dev = device_ordinal; m->c = *cfg;
    const int d = cfg->d_model, V = cfg->vocab_size, nm = cfg->num_mel_bins, ctxlen = cfg->max_target_positions;
    build_expected(m.get());
    bool ok = true;
#define MA(field, T, n) ok = ok && ((m->field = m->allocs.dalloc_into<T>((size_t)(n))) != nullptr)
#define ML(f, T, n) ok = ok && ((L.f = m->allocs.dalloc_into<T>((size_t)(n))) != nullptr)
    MA(conv1.w, half_t, (long)d * 3 * NH_MELP); MA(conv1.b, float, d);
    MA(conv2.w, half_t, (long)d * 3 * d); MA(conv2.b, float, d);
    MA(enc_pos, float, 1500L * d);
    m->enc.resize(cfg->encoder_layers);
    for (auto &L : m->enc) {
        ML(ln1.w, float, d); ML(ln1.b, float, d); ML(ln2.w, float, d); ML(ln2.b, float, d);
        ML(qkv.w, half_t, 3L * d * d); ML(qkv.b, float, 3 * d); ML(o.w, half_t, (long)d * d); ML(o.b, float, d);
        ML(fc1.w, half_t, 4L * d * d); ML(fc1.b, float, 4 * d); ML(fc2.w, half_t, 4L * d * d); ML(fc2.b, float, d);
    }
    MA(ln_post.w, float, d); MA(ln_post.b, float, d); MA(dec_ln.w, float, d); MA(dec_ln.b, float, d);
    MA(tok_emb, half_t, (long)V * d); MA(dec_pos, half_t, (long)ctxlen * d);
    m->dec.resize(cfg->decoder_layers);
    for (auto &L : m->dec) {
        ML(ln1.w, float, d); ML(ln1.b, float, d); ML(ln2.w, float, d); ML(ln2.b, float, d); ML(ln3.w, float, d); ML(ln3.b, float, d);
        ML(qkv.w, half_t, 3L * d * d); ML(qkv.b, float, 3 * d); ML(o.w, half_t, (long)d * d); ML(o.b, float, d);
        ML(cq.w, half_t, (long)d * d); ML(cq.b, float, d); ML(ckv.w, half_t, 2L * d * d); ML(ckv.b, float, 2 * d);
        ML(co.w, half_t, (long)d * d); ML(co.b, float, d);
        ML(fc1.w, half_t, 4L * d * d); ML(fc1.b, float, 4 * d); ML(fc2.w, half_t, 4L * d * d); ML(fc2.b, float, d);
    }
    MA(mel_grp, int32_t, 2 * nm);
#undef ML
#undef MA
    if (!ok) { err = "hipMalloc failed while sizing the model (out of device memory?)"; code = NH_ERR_NOMEM; return nullptr; }
    {   // encoder sinusoids, recomputed in f32 exactly as candle's sinusoids()
        std::vector<float> pos(1500L * d);
        int half = d / 2;
        float inc = logf(10000.0f) / (float)(half - 1);
        for (int p = 0; p < 1500; p++)
            for (int i = 0; i < half; i++) {
                float st = (float)p * expf((float)i * (-inc));
                pos[(long)p * d + i] = sinf(st);
                pos[(long)p * d + half + i] = cosf(st);
            }
        if (hipMemcpy(m->enc_pos, pos.data(), pos.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
            err = "hipMemcpy(enc_pos) failed"; code = NH_ERR_HIP; return nullptr;
        }
    }
    if (!build_mel_tables(m.get(), err)) { code = NH_ERR_NOMEM; return nullptr; }
    return m;
}

// stream, workspaces and caches of one context over an existing model
static int build_context(std::shared_ptr<nh_model> mdl, int max_batch, nh_ctx **out) {
    const nh_config *cfg = &mdl->c;
    const int d = cfg->d_model;
    nh_ctx *ctx = new nh_ctx();
    ctx->dev = mdl->dev; ctx->c = *cfg; ctx->B = max_batch; ctx->mdl = mdl;
    auto bail = [&](int code) { g_create_error = ctx->err; delete ctx; return code; };
    if (hipSetDevice(ctx->dev) != hipSuccess) { ctx->err = "hipSetDevice failed"; return bail(NH_ERR_HIP); }
    // ONE stream per context.  r02 gave the decode loop a stream of its own at the highest priority; r03
    // measured what that costs: the runtime backs every stream with an HSA queue, the queues are spread over the command
    // processor's pipes in CREATION ORDER, and when the decode streams of two contexts land on one pipe their kernel chains
    // take turns instead of overlapping -- three batches in flight ran at 4810 audio-s/s instead of 6330 after a harmless
    // reordering of nh_create (weights allocated before the streams), with no other change (profiles/r03_stream_order.txt:
    // two streams per context in r02's order 6332, without priorities 6332, one or two throw-away streams in front 6338 /
    // 6326, three 4782, decode stream created first 4785, ONE stream per context 6358).  Encoder and decode of one
    // context are sequential anyway; with one queue per context three contexts plus the null stream fit the four pipes.
    if (hipStreamCreateWithFlags(&ctx->st, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->enc_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&(ctx->kv_copied = std::make_shared<nh_ctx::EventBox>())->e, hipEventDisableTiming) != hipSuccess) {
        ctx->err = "hipStreamCreateWithFlags failed"; return bail(NH_ERR_HIP);
    }
    for (auto &e : ctx->ev) hipEventCreate(&e);
    const int B = max_batch, V = cfg->vocab_size, nm = cfg->num_mel_bins, ctxlen = cfg->max_target_positions;
    const long M = (long)B * 1500;
    ctx->VP = nh_logits_ld(V);
    bool ok = true;
#define DA(field, T, n) ok = ok && ((ctx->field = ctx->allocs.dalloc_into<T>((size_t)(n))) != nullptr)
    // this context's K/V caches: cross K/V of the current batch, self-attention cache
    ctx->kv.resize(cfg->decoder_layers);
    for (auto &L : ctx->kv) {
#define DL(f, T, n) ok = ok && ((L.f = ctx->allocs.dalloc_into<T>((size_t)(n))) != nullptr)
        DL(ck, half_t, M * d); DL(cv, half_t, M * d);
        DL(sk, half_t, (long)B * ctxlen * d); DL(sv, half_t, (long)B * ctxlen * d);
#undef DL
    }
    // mel
    DA(pcm, float, (long)B * NH_N_SAMPLES); DA(nsamp, int32_t, B); DA(mel32, float, (long)B * nm * NH_N_FRAMES);
    DA(chunk_max, unsigned, B); DA(mel_img, half_t, (long)B * (NH_N_FRAMES + 2) * NH_MELP);
    // encoder
    DA(h1, half_t, (long)B * (NH_N_FRAMES + 2) * d); DA(x, float, M * d); DA(xn, half_t, M * d);
    DA(q, half_t, M * d); DA(k, half_t, M * d); DA(vt, half_t, (long)B * d * NH_SP); DA(att, half_t, M * d);
    DA(hid, half_t, M * 4 * d); DA(xa16, half_t, M * d); DA(xa32, float, M * d);
    // decoder
    DA(dx, float, (long)B * d); DA(dy32, float, (long)B * d); DA(logits, float, (long)B * ctx->VP);
    DA(dxn, half_t, (long)B * d); DA(dq, half_t, (long)B * d); DA(datt, half_t, (long)B * d); DA(dhid, half_t, (long)B * 4 * d);
    DA(ds.tokens, int32_t, (long)B * ctxlen); DA(ds.n_tokens, int32_t, B); DA(ds.done, int32_t, B);
    DA(ds.have_last, int32_t, B); DA(ds.last_ts, int32_t, B); DA(ds.sum_logprob, double, B); DA(ds.no_speech, double, B);
    DA(ds.n_active, int32_t, 1); DA(suppress, uint8_t, V); DA(lpart, float, (long)B * 64); DA(ltick, unsigned, B); DA(d_pos, int32_t, B);
    DA(psamp.inv_t, float, B); DA(psamp.seed, unsigned long long, B); DA(psamp.clip, unsigned, B); DA(psamp.attempt, unsigned, B); DA(psamp.handled, int32_t, B);
    DA(d_lang_tokens, int32_t, 256); DA(d_lang_out, int32_t, B); DA(d_lang_flag, int32_t, B); DA(d_lang_probs, float, (long)B * 256);
    DA(d_pfx, int32_t, B); DA(d_pfclips, PfClip, B);
#undef DA
    if (!ok) { ctx->err = "hipMalloc failed while sizing the context (out of device memory?)"; return bail(NH_ERR_NOMEM); }
    ctx->ds.suppress = ctx->suppress;
    if (hipHostMalloc(reinterpret_cast<void **>(&ctx->h_done), sizeof(int32_t) * 256, 0) != hipSuccess) {
        ctx->err = "hipHostMalloc failed"; return bail(NH_ERR_NOMEM);
    }
    *out = ctx;
    return NH_OK;
}

extern "C" int nh_create(int device_ordinal, const nh_config *cfg, int max_batch, nh_ctx **out) {
    if (!cfg || !out || max_batch < 1) { g_create_error = "nh_create: bad arguments"; return NH_ERR_INVALID; }
    const int d = cfg->d_model;
    if (d % 128 != 0 || d > 1280 || d / cfg->encoder_attention_heads != NH_DH ||
        d / cfg->decoder_attention_heads != NH_DH || cfg->max_source_positions != 1500 ||
        (cfg->num_mel_bins != 80 && cfg->num_mel_bins != 128) || max_batch > NH_MAX_BATCH) {
        g_create_error = "nh_create: unsupported config (need d_model % 128 == 0, d_model <= 1280, head dim 64, "
                         "max_source_positions 1500, num_mel_bins 80|128, max_batch <= 96)";
        return NH_ERR_INVALID;
    }
    if (cfg->vocab_size < 1 || cfg->vocab_size > NH_MAX_VOCAB) {
        g_create_error = "nh_create: unsupported vocab_size " + std::to_string(cfg->vocab_size) + " (the vocabulary must hold 1 to " +
                         std::to_string(NH_MAX_VOCAB) + " tokens: the decode step keeps a row of logits in registers)";
        return NH_ERR_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_ordinal < 0 || device_ordinal >= ndev) {
        g_create_error = "nh_create: no HIP device with ordinal " + std::to_string(device_ordinal) +
                         " (SelectedDevice::Rocm needs a visible MI355X; there is no CPU fallback)";
        return NH_ERR_HIP;
    }
    if (hipSetDevice(device_ordinal) != hipSuccess) { g_create_error = "hipSetDevice failed"; return NH_ERR_HIP; }
    std::string err; int code = NH_ERR_HIP;
    std::shared_ptr<nh_model> mdl = build_model(device_ordinal, cfg, err, code);
    if (!mdl) { g_create_error = err; return code; }
    return build_context(mdl, max_batch, out);
}

// A second (third ...) context on the SAME device over the SAME weights: own stream, workspaces, K/V caches, tokens and
// decode state; the model tables are shared and reference counted (freed with the last context).
extern "C" int nh_create_shared(nh_ctx *parent, int max_batch, nh_ctx **out) {
    if (!parent || !out || max_batch < 1 || max_batch > NH_MAX_BATCH) { g_create_error = "nh_create_shared: bad arguments (1 <= max_batch <= 96)"; return NH_ERR_INVALID; }
    return build_context(parent->mdl, max_batch, out);
}

// ---- weight loading ----------------------------------------------------------------------------------
static float host_elem(const void *data, int dtype, size_t i) {
    return dtype == NH_DTYPE_F32 ? reinterpret_cast<const float *>(data)[i]
                                 : (float)reinterpret_cast<const _Float16 *>(data)[i];
}
static int up_f16(nh_ctx *ctx, half_t *dst, const void *data, int dtype, size_t n) {
    if (dtype == NH_DTYPE_F16) { HIPCHK(hipMemcpy(dst, data, n * 2, hipMemcpyHostToDevice)); return NH_OK; }
    std::vector<_Float16> tmp(n);
    const float *s = reinterpret_cast<const float *>(data);
    for (size_t i = 0; i < n; i++) tmp[i] = (_Float16)s[i];
    HIPCHK(hipMemcpy(dst, tmp.data(), n * 2, hipMemcpyHostToDevice));
    return NH_OK;
}
static int up_f32(nh_ctx *ctx, float *dst, const void *data, int dtype, size_t n) {
    if (dtype == NH_DTYPE_F32) { HIPCHK(hipMemcpy(dst, data, n * 4, hipMemcpyHostToDevice)); return NH_OK; }
    std::vector<float> tmp(n);
    for (size_t i = 0; i < n; i++) tmp[i] = host_elem(data, dtype, i);
    HIPCHK(hipMemcpy(dst, tmp.data(), n * 4, hipMemcpyHostToDevice));
    return NH_OK;
}
// conv weight [co][ci][3] -> [co][kk * cpad + ci] fp16 (zero padded channels)
static int up_conv(nh_ctx *ctx, half_t *dst, const void *data, int dtype, int co, int ci, int cpad) {
    std::vector<_Float16> tmp((size_t)co * 3 * cpad, (_Float16)0.f);
    for (int o = 0; o < co; o++)
        for (int c = 0; c < ci; c++)
            for (int kk = 0; kk < 3; kk++)
                tmp[((size_t)o * 3 + kk) * cpad + c] = (_Float16)host_elem(data, dtype, ((size_t)o * ci + c) * 3 + kk);
    HIPCHK(hipMemcpy(dst, tmp.data(), tmp.size() * 2, hipMemcpyHostToDevice));
    return NH_OK;
}

static bool starts(const std::string &s, const char *p, std::string &rest) {
    size_t n = strlen(p);
    if (s.compare(0, n, p) != 0) return false;
    rest = s.substr(n);
    return true;
}

extern "C" int nh_load_tensor(nh_ctx *ctx, const char *name_c, int dtype, const int64_t *shape, int ndim,
                              const void *data) {
    if (!ctx || !name_c || !data || !shape || (dtype != NH_DTYPE_F32 && dtype != NH_DTYPE_F16))
        return ctx ? ctx->fail(NH_ERR_INVALID, "nh_load_tensor: bad arguments") : NH_ERR_INVALID;
    hipSetDevice(ctx->dev);
    const std::string name(name_c);
    if (name == "model.encoder.embed_positions.weight" || name == "proj_out.weight") return NH_OK;  // not read by candle
    nh_model &m = *ctx->mdl;
    if (!m.expected.count(name)) return ctx->fail(NH_ERR_INVALID, "nh_load_tensor: unknown tensor name " + name);
    size_t n = 1;
    for (int i = 0; i < ndim; i++) n *= (size_t)shape[i];
    const int d = ctx->c.d_model;
    auto want = [&](size_t expect) -> int {
        if (n != expect)
            return ctx->fail(NH_ERR_INVALID, "nh_load_tensor: " + name + " has " + std::to_string(n) +
                                                 " elements, expected " + std::to_string(expect));
        return NH_OK;
    };
    int rc = NH_OK;
    std::string rest;
    auto lin = [&](LinW &L, const std::string &leaf, size_t n_out, size_t n_in, size_t row_off) -> int {
        if (leaf == "weight") { if ((rc = want(n_out * n_in))) return rc; return up_f16(ctx, L.w + row_off * n_in, data, dtype, n); }
        if (leaf == "bias") { if ((rc = want(n_out))) return rc; return up_f32(ctx, L.b + row_off, data, dtype, n); }
        return ctx->fail(NH_ERR_INVALID, "nh_load_tensor: unknown leaf in " + name);
    };
    auto ln = [&](LnW &L, const std::string &leaf) -> int {
        if ((rc = want(d))) return rc;
        if (leaf == "weight") return up_f32(ctx, L.w, data, dtype, n);
        if (leaf == "bias") return up_f32(ctx, L.b, data, dtype, n);
        return ctx->fail(NH_ERR_INVALID, "nh_load_tensor: unknown leaf in " + name);
    };
    // the eight tensors that an encoder and a decoder layer share; fin: the layer's final_layer_norm
    auto layer = [&](auto &L, LnW &fin, const std::string &sub) -> bool {
        std::string leaf;
        if (starts(sub, "self_attn.q_proj.", leaf)) rc = lin(L.qkv, leaf, d, d, 0);
        else if (starts(sub, "self_attn.k_proj.", leaf)) rc = lin(L.qkv, leaf, d, d, d);
        else if (starts(sub, "self_attn.v_proj.", leaf)) rc = lin(L.qkv, leaf, d, d, 2 * d);
        else if (starts(sub, "self_attn.out_proj.", leaf)) rc = lin(L.o, leaf, d, d, 0);
        else if (starts(sub, "self_attn_layer_norm.", leaf)) rc = ln(L.ln1, leaf);
        else if (starts(sub, "fc1.", leaf)) rc = lin(L.fc1, leaf, 4 * d, d, 0);
        else if (starts(sub, "fc2.", leaf)) rc = lin(L.fc2, leaf, d, 4 * d, 0);
        else if (starts(sub, "final_layer_norm.", leaf)) rc = ln(fin, leaf);
        else return false;
        return true;
    };
    if (name == "model.encoder.conv1.weight") { if (!(rc = want((size_t)d * ctx->c.num_mel_bins * 3))) rc = up_conv(ctx, m.conv1.w, data, dtype, d, ctx->c.num_mel_bins, NH_MELP); }
    else if (name == "model.encoder.conv1.bias") { if (!(rc = want(d))) rc = up_f32(ctx, m.conv1.b, data, dtype, n); }
    else if (name == "model.encoder.conv2.weight") { if (!(rc = want((size_t)d * d * 3))) rc = up_conv(ctx, m.conv2.w, data, dtype, d, d, d); }
    else if (name == "model.encoder.conv2.bias") { if (!(rc = want(d))) rc = up_f32(ctx, m.conv2.b, data, dtype, n); }
    else if (starts(name, "model.encoder.layer_norm.", rest)) rc = ln(m.ln_post, rest);
    else if (starts(name, "model.decoder.layer_norm.", rest)) rc = ln(m.dec_ln, rest);
    else if (name == "model.decoder.embed_tokens.weight") { if (!(rc = want((size_t)ctx->c.vocab_size * d))) rc = up_f16(ctx, m.tok_emb, data, dtype, n); }
    else if (name == "model.decoder.embed_positions.weight") { if (!(rc = want((size_t)ctx->c.max_target_positions * d))) rc = up_f16(ctx, m.dec_pos, data, dtype, n); }
    else {
        bool is_enc = starts(name, "model.encoder.layers.", rest);
        bool is_dec = !is_enc && starts(name, "model.decoder.layers.", rest);
        if (!is_enc && !is_dec) return ctx->fail(NH_ERR_INVALID, "nh_load_tensor: unhandled tensor " + name);
        size_t dot = rest.find('.');
        int idx = atoi(rest.substr(0, dot).c_str());
        std::string sub = rest.substr(dot + 1), leaf;
        bool known;
        if (is_enc) known = layer(m.enc[idx], m.enc[idx].ln2, sub);
        else {
            DecLayer &L = m.dec[idx];
            if (!(known = layer(L, L.ln3, sub))) {
                known = true;
                if (starts(sub, "encoder_attn.q_proj.", leaf)) rc = lin(L.cq, leaf, d, d, 0);
                else if (starts(sub, "encoder_attn.k_proj.", leaf)) rc = lin(L.ckv, leaf, d, d, 0);
                else if (starts(sub, "encoder_attn.v_proj.", leaf)) rc = lin(L.ckv, leaf, d, d, d);
                else if (starts(sub, "encoder_attn.out_proj.", leaf)) rc = lin(L.co, leaf, d, d, 0);
                else if (starts(sub, "encoder_attn_layer_norm.", leaf)) rc = ln(L.ln2, leaf);
                else known = false;
            }
        }
        if (!known) return ctx->fail(NH_ERR_INVALID, "nh_load_tensor: unhandled tensor " + name);
    }
    if (rc == NH_OK) {
        std::lock_guard<std::mutex> lk(m.mu);
        m.loaded.insert(name); m.dec_tiled_valid = false;
    }
    return rc;
}

// The decoder's GEMVs stream every weight once per token: repack them tile-major (launch_repack_tiles) so that a wave
// instruction reads 1 KiB contiguous instead of 16 row pieces of 64 B.  Done lazily before the first decoder use and
// again after any nh_load_tensor; the row-major originals stay (embedding lookup, cross-K/V GEMM, re-loading).
//
// Contexts read the model's tables in place (ctx->mdl->...), with no lock on the hot path.  That is sound because
//  - every pointer in nh_model is set once and never moved: the tables by build_model, before any context exists; the `wt`
//    repacks and tok_emb_t below, on the first repack, under `mu`; a repack after a reload rewrites the same buffers;
//  - every decode entry point comes through here first, and this function takes `mu` and synchronises: a context that
//    goes on to read a `wt` pointer has either set it itself or acquired the lock after the context that did;
//  - mt.filters, the one pointer nh_set_mel_filters replaces, has always been read straight from the model.
int ensure_decoder_repack(nh_ctx *ctx) {
    nh_model &m = *ctx->mdl;
    {
        std::lock_guard<std::mutex> lk(m.mu);   // contexts that share the model may get here together: one of them repacks
        if (!m.dec_tiled_valid) {
            const int d = ctx->c.d_model, V = ctx->c.vocab_size;
            auto one = [&](half_t *&dst, const half_t *src, int N, int K) -> bool {
                if (!dst) { dst = m.allocs.dalloc_into<half_t>((size_t)((N + 15) / 16) * 16 * K, false); }
                if (!dst) return false;
                launch_repack_tiles(src, dst, N, K, ctx->st);
                return true;
            };
            bool ok = one(m.tok_emb_t, m.tok_emb, V, d);
            for (auto &L : m.dec) {
                ok = ok && one(L.qkv.wt, L.qkv.w, 3 * d, d) && one(L.o.wt, L.o.w, d, d) && one(L.cq.wt, L.cq.w, d, d) &&
                     one(L.co.wt, L.co.w, d, d) && one(L.fc1.wt, L.fc1.w, 4 * d, d) && one(L.fc2.wt, L.fc2.w, d, 4 * d);
                // the cross K projection transposed ([feature][head dim]; NH_OPT_ABSORBED_XATTN reads Wk_h^T q from it)
                if (ok && !L.ckv.wt) L.ckv.wt = m.allocs.dalloc_into<half_t>((size_t)d * d, false);
                ok = ok && L.ckv.wt;
                if (ok) launch_transpose_sq(L.ckv.w, L.ckv.wt, d, ctx->st);
            }
            if (!ok) return ctx->fail(NH_ERR_NOMEM, "hipMalloc(tile-major decoder weights)");
            HIPCHK(hipStreamSynchronize(ctx->st));
            HIPCHK(hipGetLastError());
            m.dec_tiled_valid = true;
        }
    }
    return NH_OK;
}

extern "C" int nh_missing_tensors(const nh_ctx *ctx) {
    if (!ctx) return -1;
    std::lock_guard<std::mutex> lk(ctx->mdl->mu);
    return (int)(ctx->mdl->expected.size() - ctx->mdl->loaded.size());
}

extern "C" int nh_set_mel_filters(nh_ctx *ctx, const float *filters, int n_mel) {
    if (!ctx || !filters) return NH_ERR_INVALID;
    if (n_mel != ctx->c.num_mel_bins) return ctx->fail(NH_ERR_INVALID, "Unexpected number of mel bins (num_mel_bins), got: " + std::to_string(n_mel));
    hipSetDevice(ctx->dev);
    nh_model &m = *ctx->mdl;
    std::lock_guard<std::mutex> lk(m.mu);
    float *df = m.allocs.dalloc_into<float>((size_t)n_mel * 201);
    if (!df) return ctx->fail(NH_ERR_NOMEM, "hipMalloc(mel filters)");
    HIPCHK(hipMemcpy(df, filters, (size_t)n_mel * 201 * 4, hipMemcpyHostToDevice));
    std::vector<int32_t> grp(2 * n_mel);
    mel_host_groups(filters, n_mel, grp.data());
    HIPCHK(hipMemcpy(m.mel_grp, grp.data(), grp.size() * 4, hipMemcpyHostToDevice));
    m.mt.filters = df;
    m.have_filters = true;
    return NH_OK;
}

extern "C" int nh_set_tokens(nh_ctx *ctx, const nh_tokens *tk, const int32_t *suppress_tokens, int n_suppress) {
    if (!ctx || !tk || (n_suppress > 0 && !suppress_tokens)) return NH_ERR_INVALID;
    const int V = ctx->c.vocab_size;
    auto inr = [&](int t) { return t >= 0 && t < V; };
    if (!inr(tk->sot) || !inr(tk->eot) || !inr(tk->task) || !inr(tk->no_speech) || !inr(tk->no_timestamps) ||
        !inr(tk->zero_sec) || !inr(tk->one_sec) || (tk->lang >= V))
        return ctx->fail(NH_ERR_INVALID, "nh_set_tokens: token id outside the vocabulary");
    hipSetDevice(ctx->dev);
    // monolingual.rs:386-395: suppress_tokens = config list U {no_timestamps}
    std::vector<uint8_t> sup(V, 0);
    for (int i = 0; i < n_suppress; i++) if (inr(suppress_tokens[i])) sup[suppress_tokens[i]] = 1;
    sup[tk->no_timestamps] = 1;
    HIPCHK(hipMemcpy(ctx->suppress, sup.data(), V, hipMemcpyHostToDevice));
    ctx->tk = RuleTokens{tk->sot, tk->eot, tk->lang, tk->task, tk->no_speech, tk->no_timestamps, tk->zero_sec, tk->one_sec};
    ctx->have_tokens = true;
    ctx->token_gen++;  // the captured step graphs carry the old ids by value (logit_step_kernel): re-capture
    drop_graphs(ctx);
    return NH_OK;
}

extern "C" int nh_reset(nh_ctx *ctx) {  // Type::reset_kv_cache (model.rs:485-490)
    if (!ctx) return NH_ERR_INVALID;
    ctx->have_enc = false;
    clear_prompt(ctx);
    return NH_OK;
}

extern "C" int nh_synchronize(nh_ctx *ctx) {
    if (!ctx) return NH_ERR_INVALID;
    hipSetDevice(ctx->dev);
    HIPCHK(hipStreamSynchronize(ctx->st));
    return NH_OK;
}

// ---- instrumentation -------------------------------------------------------------------------------------
extern "C" int nh_set_profile_gemm(nh_ctx *ctx, int enable) {
    if (!ctx) return NH_ERR_INVALID;
    ctx->profile_gemm = enable != 0;
    return NH_OK;
}

extern "C" int nh_set_option(nh_ctx *ctx, int option, int value) {
    if (!ctx) return NH_ERR_INVALID;
    if (option == NH_OPT_DECODE_GRAPHS) ctx->opt_graphs = value != 0;
    else if (option == NH_OPT_FUSE_DECODE_LAYERNORM) { ctx->opt_fuse_ln = value != 0; drop_graphs(ctx); }
    else if (option == NH_OPT_DECODER_LAYER_LIMIT) {
        if (value < 0 || value > ctx->c.decoder_layers) return ctx->fail(NH_ERR_INVALID, "nh_set_option: layer limit outside [0, decoder_layers]");
        ctx->dec_layer_limit = value; drop_graphs(ctx);
        ctx->live.gen++; ctx->live.lock_valid = false;   // queries kept under another depth are not answered for (nh_align_decoded)
    }
    else if (option == NH_OPT_ABSORBED_XATTN) {
        if (value < 0 || value > 2) return ctx->fail(NH_ERR_INVALID, "nh_set_option: NH_OPT_ABSORBED_XATTN takes 0, 1 or 2");
        // pool steps would read xa16 rows that admission never fills (it copies the cross K/V only); nh_pool_begin refuses the reverse order
        if (value && ctx->pool.rows > 0) return ctx->fail(NH_ERR_STATE, "nh_set_option: NH_OPT_ABSORBED_XATTN covers lockstep decodes only, and the context runs a decode pool");
        if (value == 2 && !xabs_fast_supported(ctx->c.d_model, ctx->c.decoder_attention_heads)) value = 1;   // widths the one-pass kernel is not built for
        hipSetDevice(ctx->dev);
        AbsorbedState &xs = ctx->xabs;
        // the launcher needs u's rows of heads >= H to be zero, and xabs_u_fast_kernel writes only the heads it has
        if (value)
            if (int rc = xs.u.reserve(ctx, sizeof(half_t) * (size_t)ctx->B * 32 * ctx->c.d_model, "absorbed attention scratch", true)) return rc;
        if (value == 2) {
            Carve cv;
            const size_t o_z = cv.take(sizeof(float) * (size_t)ctx->B * 4 * ctx->c.decoder_attention_heads * ctx->c.d_model);
            const size_t o_ml = cv.take(sizeof(float) * (size_t)ctx->B * 4 * 32 * 2);
            if (int rc = xs.parts.reserve(ctx, cv.off, "absorbed attention partials", true)) return rc;
            xs.z = xs.parts.at<float>(o_z); xs.ml = xs.parts.at<float>(o_ml);
        }
        ctx->opt_absorbed = value; drop_graphs(ctx);
        ctx->live.gen++; ctx->live.lock_valid = false;
    }
    else if (option == NH_OPT_ALIGN_KEEP) ctx->opt_align_keep = value != 0;
    else if (option == NH_OPT_PROMPT_STEPWISE) ctx->opt_prompt_stepwise = value != 0;
    else return ctx->fail(NH_ERR_INVALID, "nh_set_option: unknown option " + std::to_string(option));
    return NH_OK;
}

extern "C" int nh_get_timings(nh_ctx *ctx, nh_timings *out) {
    if (!ctx || !out) return NH_ERR_INVALID;
    hipSetDevice(ctx->dev);
    HIPCHK(hipStreamSynchronize(ctx->st));
    nh_timings t = ctx->tm;
    hipEventElapsedTime(&t.mel_ms, ctx->ev[0], ctx->ev[1]);
    hipEventElapsedTime(&t.encoder_ms, ctx->ev[2], ctx->ev[3]);
    hipEventElapsedTime(&t.cross_kv_ms, ctx->ev[3], ctx->ev[4]);
    hipEventElapsedTime(&t.decode_ms, ctx->ev[5], ctx->ev[6]);
    (void)hipGetLastError();  // a phase that has not run yet (a decode pool records no decode interval) leaves its time at 0, not an error behind
    t.gemm_ms = 0.f; t.gemm_launches = 0; t.gemm_flops = ctx->gemm_flops_acc;
    for (size_t i = 0; i + 1 < ctx->gemm_ev_used; i += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->gemm_ev[i], ctx->gemm_ev[i + 1]) == hipSuccess) { t.gemm_ms += ms; t.gemm_launches++; }
    }
    *out = t;
    return NH_OK;
}
