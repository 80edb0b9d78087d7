// nh_ctx.h -- the state behind the C ABI of include/norma_hip.h, shared by the files that implement it: nh_model.hip
// (create / destroy, weights, tokens, options, timings), nh_encode.hip (log-mel, encoder), nh_decode.hip (decoder step,
// lockstep decode, decode pool, parity views), nh_prefill.hip (decoder prompts, the one-pass forward), nh_score.hip (transcript scoring), nh_align.hip (token-level timestamps), nh_resample.hip (audio ingest),
// nh_cut.hip (cutting long recordings), nh_vad.hip (their speech map).  Device memory has two owners and no third: an
// Arena for what is made once and kept until its owner dies (the model's tables, the workspaces build_context makes), and
// DevBuf for everything made lazily, grown, replaced or living for one call -- a feature's lazy buffers are ONE DevBuf cut
// with Carve, so a group is there or not there.  Both release themselves: ~nh_ctx names neither.  Also here: the batch check
// (check_batch) that runs before anything is queued.  No torch, no candle, no CPU fallback: an entry point runs the HIP
// path or fails.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <algorithm>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../../include/norma_hip_pool.h"   // ... which includes norma_hip.h
#include "nh_kernels.h"

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            return ctx->fail(NH_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
        }                                                                                     \
    } while (0)

// Device buffers made once and kept until their owner dies: they never move and are never replaced.
struct Arena {
    std::vector<void *> ptrs;
    Arena() = default;
    Arena(const Arena &) = delete;
    Arena &operator=(const Arena &) = delete;
    ~Arena() { for (void *p : ptrs) hipFree(p); }   // the owner's destructor has made the device current
    template <typename T>
    T *dalloc_into(size_t n, bool zero = true) {
        void *p = nullptr;
        if (n == 0) n = 1;
        if (hipMalloc(&p, n * sizeof(T)) != hipSuccess) return nullptr;
        if (zero) hipMemset(p, 0, n * sizeof(T));
        ptrs.push_back(p);
        return reinterpret_cast<T *>(p);
    }
};

struct LinW { half_t *w = nullptr; float *b = nullptr; half_t *wt = nullptr; /* tile-major repack (decoder GEMVs) */ };
struct LnW { float *w = nullptr, *b = nullptr; };
struct EncLayer { LnW ln1, ln2; LinW qkv, o, fc1, fc2; };
struct DecLayer { LnW ln1, ln2, ln3; LinW qkv, o, cq, ckv, co, fc1, fc2; };
// one decoder layer's caches of one context: cross K/V of the current batch, self-attention K/V
struct KvCache { half_t *ck = nullptr, *cv = nullptr, *sk = nullptr, *sv = nullptr; };

// The read-only half of a context: everything nh_load_tensor / nh_set_mel_filters fill in.  Owned through a shared_ptr, so
// that several contexts on one device (nh_create_shared) run on ONE copy of the weights: bench.py keeps three batches in
// flight per GPU, and three private copies meant 3 x 1.5 GB of HBM and three different address ranges for the 225 MB of
// decoder weights + embedding every in-flight decode streams per token.  The contexts read these tables in place: no
// pointer in here moves once it is set (see ensure_decoder_repack).
struct nh_model {
    int dev = 0;
    nh_config c{};
    Arena allocs;                    // the tables below; lazy additions (repacks, resample and mel filter tables) under mu
    LinW conv1, conv2;
    float *enc_pos = nullptr;
    std::vector<EncLayer> enc;
    LnW ln_post, dec_ln;
    half_t *tok_emb = nullptr, *dec_pos = nullptr;
    half_t *tok_emb_t = nullptr;     // tile-major repack of the tied embedding (logits GEMV)
    std::vector<DecLayer> dec;
    bool dec_tiled_valid = false;    // the repacks mirror the row-major decoder weights loaded so far
    std::set<std::string> expected, loaded;
    MelTables mt{};
    int32_t *mel_grp = nullptr;
    bool have_filters = false;
    // nh_resample's filters, one per source rate seen so far (coef: device f32 [L][T], in allocs); built under mu on first use
    struct ResampleTable { int src_hz, L, M, T; float *coef; };
    std::vector<ResampleTable> rs_tables;
    std::mutex mu;                   // guards loaded / dec_tiled_valid and the lazy repack
    // hipStreamWaitEvent fails ("dependency created on uncaptured work in another stream") on an event whose stream is capturing
    // at that moment, even one recorded before: a step capture and the encoders' waits on kv_readers exclude each other
    std::mutex capture_mu;
    ~nh_model() { hipSetDevice(dev); }   // ... and allocs frees the tables
};

struct PoolRow {   // one row of a decode pool, as the host knows it
    bool busy = false;
    bool held = false;       // the row holds a clip: admitted since nh_pool_begin (nh_pool_retry decodes that clip again)
    bool sampled = false;    // the row is busy on a sampled retry (nh_pool_retry); cleared by nh_pool_collect and by an admit
    bool inv_t_set = false;  // the row's device-side inv_t is > 0 (its last decode was a retry): the next admit zeroes it
    bool detect = false;     // the row's clip was admitted with NH_LANG_DETECT; an admit sets or clears it
    bool detected = false;   // ... and has taken a step since: d_lang_out / d_lang_probs hold its language
    int pfx = 0;             // prefix length of the clip the row holds (nh_pool_prefix; the device side is nh_ctx::d_pfx)
    // what nh_pool_collect last read off the row (nh_align_decoded): tokens after finish_sequence's trim, the done flag, and
    // the alignment generation its queries were kept under (-1: none; an admit or a retry clears it)
    int n = 0, done = 0, align_gen = -1;
};
// Decode pool (nh_pool_*): rows [0, rows) decode, each at its own position; rows above are encoder staging.  rows == 0: no pool.
struct Pool {
    int rows = 0, max_new = 0, prompt = 0;
    int lang_n = 0;          // entries of the pool's language table in d_lang_tokens (nh_pool_detect_languages); 0: none
    bool per_clip_language = false;
    std::vector<PoolRow> row;
    // nh_pool_prefix: pending[r] ids wait in pfx_host row r for the next admission into row r (0: none); todo: the rows admitted
    // on the one-pass route since the last ragged prefill, which the head of the next nh_pool_step that runs steps issues
    std::vector<int> pending;
    std::vector<PfClip> todo;
};

// Everything a captured decode step takes by value (batch, encoder length, max_new_tokens, prompt length, the rule token ids,
// the size of a pool's language table) and which kernels it holds.  A step under another key captures again.
struct StepKey {
    int B = -1, S = -1, max_new = -1, P = -1, token_gen = -1, lang_n = -1;
    bool pool = false, sampled = false;
    int align_gen = 0;   // the alignment heads whose queries the steps keep go by value too (nh_align_capture)
    int guard_gen = 0;   // ... and so do the guard's parameters, its tables, and whether its kernel is in the step (nh_set_guard)
    bool operator==(const StepKey &o) const {
        return B == o.B && S == o.S && max_new == o.max_new && P == o.P && token_gen == o.token_gen && lang_n == o.lang_n &&
               pool == o.pool && sampled == o.sampled && align_gen == o.align_gen && guard_gen == o.guard_gen;
    }
};
struct StepGraphs {
    StepKey key;                    // B == -1: nothing captured
    hipGraphExec_t one = nullptr;   // one decode step
    hipGraphExec_t multi = nullptr; // NH_GRAPH_STEPS consecutive steps (one launch gap instead of NH_GRAPH_STEPS)
};

// A device buffer that grows on demand: empty until the first call that needs it (a context that never stages, plans or
// aligns holds nothing), released with whatever it is a member or a local of.
struct nh_ctx;
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) hipFree(p); }   // ~nh_ctx has made the device current and drained the stream
    // room for `need` bytes (contents are not kept; zero: a buffer made here starts as zeros, in stream order); on failure the
    // buffer is empty and NH_ERR_NOMEM names `what`
    int reserve(nh_ctx *ctx, size_t need, const char *what, bool zero = false);
    void swap(DevBuf &o) { std::swap(p, o.p); std::swap(bytes, o.bytes); }
    template <typename T>
    T *at(size_t off = 0) const { return reinterpret_cast<T *>(static_cast<char *>(p) + off); }
};
// One DevBuf carved into 16-byte aligned pieces: take(bytes) is the piece's offset, `off` ends as the bytes to reserve
static inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }
struct Carve {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += up16(bytes); return o; }
};

// The workspace of stages 2 - 6 (nh_align, nh_align_decoded): allocated by the first alignment (contexts that never align pay
// nothing).  The last call's shape is kept for the views (nh_align_weights / nh_align_matrix).
struct AlignState {
    DevBuf buf;                      // everything below, carved again when the shape changes; it only grows
    int32_t *n_rows = nullptr, *n_keys = nullptr;   // [max_batch]
    int32_t *row_map = nullptr;                     // [max_batch] context row of every clip of a call (nh_align_decoded on a pool)
    int32_t *first = nullptr, *last = nullptr;      // [max_batch][C + 1]
    float *W = nullptr, *stats = nullptr, *M = nullptr;   // per clip of a group: [heads][C - 1][S], [heads][2][S], [C][S]
    uint8_t *trace = nullptr;        // [C][S] per clip of a group
    int heads = 0, group = 0, S = 0; // the shape the workspace was made for
    // the last nh_align / nh_align_decoded, for the views (n_tokens 0: that clip had nothing to align)
    bool kept = false;
    int P = 0, A = 0;
    std::vector<int32_t> n_tokens, keys;
};

// A validated list of alignment heads and its per-layer table (align_head_set, nh_align.hip)
struct AlignHeadSet {
    int A = 0;
    nh_align_head heads[NH_ALIGN_HEADS];
    std::vector<AlignLayerHeads> layer;   // [decoder_layers] while A > 0; n == 0: no head there
};

// nh_align_capture: the alignment heads whose cross-attention queries every decode of the context keeps, and what the
// context remembers of the last lockstep decode for nh_align_decoded.  hs.A == 0 (the default): the decode step launches
// nothing for it.
struct AlignLive {
    AlignHeadSet hs;
    int gen = 0;   // in StepKey; bumped by nh_align_capture, by options that change what a step computes, and when align_q moves
    // the last lockstep decode, while nothing has overwritten what it left: per clip the tokens after the trim and the done flag
    bool lock_valid = false;
    int P = 0;
    std::vector<int32_t> n, done;
};

// nh_cut_plan: everything it owns.  Two (e, E) workspaces: a plan computes into the one that is not the view of nh_cut_energy
// and becomes the view only when it succeeds, so a refused call -- cap too small is known only after the search -- leaves the
// view of the plan before as it was.
struct CutState {
    DevBuf ws[2];                // e[F] then E[F] of the plan computed there
    int view = -1;               // the workspace of the last successful plan; -1: none yet
    long long F = 0;             // its frames
    DevBuf out;                  // the search's outputs: starts[cap] (64-bit), lens[cap], the count; cut again by every plan
};

// nh_vad_plan: everything it owns, beside and apart from CutState (the view of nh_cut_energy is not its to change).  Two view
// workspaces for the same reason as there: the counts are known only after the walk, and a refused plan shows nothing.
struct VadState {
    DevBuf ws[2];                // of the plan computed there: regions (a, b pairs, 64-bit), levels[3] + the region count, E[F], v3[F]
    int view = -1;               // the workspace of the last successful plan; -1: none yet
    long long F = 0;             // its frames
    DevBuf tmp;                  // e[F], the select's state, the per-tile scan records, two flag buffers
    DevBuf out;                  // piece starts (64-bit), piece lengths, chunk_first, the two counts
    DevBuf tab;                  // nh_logmel_pieces_rows: the piece table of a batch of device PCM
    std::vector<long long> h_tab;   // ... and its host side, alive until the next call's copy
};

// nh_decode_beam: everything it owns.  One allocation made by the first beam decode (or beam view), sized by max_batch
// alone (K * B rows never exceed it); a context that never searches holds nothing.  The host side keeps the finished lists
// of the last beam decode for nh_beam_hypotheses.
struct BeamState {
    DevBuf buf;
    BeamBufs bb{};
    int32_t *cand_tok = nullptr, *cand_n = nullptr;   // [max_batch][NH_MAX_BEAMS + 1], [max_batch]
    float *cand_q = nullptr;
    half_t **caches = nullptr;                        // [2 * decoder_layers] sk, sv of every layer
    bool valid = false;                               // the vectors below are the last beam decode's
    int B = 0, K = 0, skip = 0;
    std::vector<int32_t> fin_tokens, fin_n, fin_count;
    std::vector<double> fin_score;
};

// nh_score: everything it owns.  One allocation made by the first call, sized by max_batch alone; a context that never scores
// holds nothing.
struct ScoreState {
    DevBuf buf;
    int32_t *target = nullptr;   // [max_batch * (C - 1)] target column of every row (clip, position); -1: not scored
    float *tlogit = nullptr;     // [max_batch * (C - 1)] the target's logit
    float *out = nullptr;        // [max_batch][C] device side of out_logprob
    float *part = nullptr;       // the tile partials of one row panel (launch_score_rows)
};

// nh_set_guard / nh_guard_bias: the repetition guard of the context's decode steps.  on == false (the default): a step launches
// nothing for it.  The flags are made by the first nh_set_guard that switches something on, the bias table by the first
// nh_guard_bias (or by enabling the bias): a context that never calls them holds nothing.
struct GuardState {
    GuardSpec spec{0, 1.0f, 0, 0, 0};
    bool on = false;
    int gen = 0;                    // in StepKey; bumped whenever spec changes or a table is made
    DevBuf flags, table;            // loop_exit; the four pieces of the bias table.  Both start as zeros.
    int32_t *loop_exit = nullptr;   // [max_batch]
    int32_t *bias_tok = nullptr, *bias_n = nullptr, *bias_map = nullptr;   // [max_batch][NH_GUARD_MAX_BIAS], [max_batch], [max_batch] (nh_guard_apply)
    float *bias_val = nullptr;
    bool after_beam = false;        // the last lockstep decode was a beam search: nh_guard_report refuses
};

// NH_OPT_ABSORBED_XATTN: the scratch of the absorbed cross-attention, made by the first nh_set_option that switches it on
struct AbsorbedState {
    DevBuf u;                    // fp16 [max_batch][32][d] (heads padded to 32; made as zeros, and the pad rows stay zero)
    DevBuf parts;                // the key-range partials of the one-pass form (value 2): z, then ml
    float *z = nullptr, *ml = nullptr;
};

struct nh_ctx {
    int dev = 0;
    std::shared_ptr<nh_model> mdl;
    hipStream_t st = nullptr;   // the context's one stream: log-mel, encoder, cross K/V, decode loop (see build_context)
    hipEvent_t enc_done = nullptr;
    // nh_pool_admit_from: decode pools of OTHER contexts copy cross K/V out of this context's rows on THEIR streams; the next
    // encoder submission here must not overwrite those rows before the copies have run
    struct EventBox { hipEvent_t e = nullptr; ~EventBox() { if (e) hipEventDestroy(e); } };
    std::shared_ptr<EventBox> kv_copied;       // recorded on this context's stream after it copied K/V out of another context
    std::mutex readers_mu;
    std::vector<std::shared_ptr<EventBox>> kv_readers;   // kv_copied of the pools that read this context's K/V since its last encode (kept alive here)
    nh_config c{};
    int B = 1;
    std::string err;
    Arena allocs;               // the workspaces and caches below: build_context makes them all, nothing joins them later
    std::vector<KvCache> kv;    // [decoder_layers]; the weights are read from mdl
    // mel
    float *pcm = nullptr;
    // The one staging of host audio on its way to the PCM rows or the cut energies (nh_logmel_samples, nh_resample*,
    // nh_cut_plan): at most NH_STAGE_BYTES, except a single resample clip that alone needs more.  Every use is a copy on the
    // context's stream with the kernel that reads it queued right behind, so the stream orders the next copy, whoever
    // makes it, behind the kernel that read the bytes before.
    DevBuf stage;
    DevBuf rs_clips;            // ResampleClip [max_batch]: per-clip records of a resample call, made by the first one
    CutState cut;               // nh_cut_plan, nh_cut_energy
    VadState vad;               // nh_vad_plan, nh_vad_view, nh_logmel_pieces_rows
    int32_t *nsamp = nullptr;
    float *mel32 = nullptr;
    unsigned *chunk_max = nullptr;
    half_t *mel_img = nullptr;
    // encoder workspaces
    half_t *h1 = nullptr, *xn = nullptr, *q = nullptr, *k = nullptr, *vt = nullptr, *att = nullptr, *hid = nullptr,
           *xa16 = nullptr;
    float *x = nullptr, *xa32 = nullptr;
    // decoder workspaces
    float *dx = nullptr, *dy32 = nullptr, *logits = nullptr;
    half_t *dxn = nullptr, *dq = nullptr, *datt = nullptr, *dhid = nullptr;
    DecodeState ds{};
    uint8_t *suppress = nullptr;
    float *lpart = nullptr;
    unsigned *ltick = nullptr;
    int32_t *d_pos = nullptr;  // [max_batch] device-side decode position of every sequence (hipGraph replays read and advance it)
    Pool pool;                       // decode pool (nh_pool_*)
    PoolSampling psamp{};            // [max_batch] each: per-row temperature, seed, clip, attempt, and the step's handled flags
    int32_t *d_lang_flag = nullptr;  // [max_batch] device side of PoolRow::detect, cleared by a retry (the token is in the prompt by then)
    // nh_pool_prefix.  d_pfx: [max_batch] device side of PoolRow::pfx, which the pool-mode selection kernels and the guard read
    // through the pointer (zero at creation and at nh_pool_begin; the admit kernel writes a row's).  d_pfclips: [max_batch] the
    // clip table of a ragged one-pass forward.  pfx_host: pinned, [max_batch][max_target_positions / 2] pending ids, then
    // max_batch PfClip: the host side of the two async copies (ids at an admission, the table at a prefill); a row's ids are
    // rewritten only while the row is free and the table only by nh_pool_step, both behind a drained stream.  Made by the
    // first nh_pool_prefix: a context that never takes a prefix holds no host buffer.
    int32_t *d_pfx = nullptr;
    PfClip *d_pfclips = nullptr;
    int32_t *pfx_host = nullptr;
    // [0]: greedy steps, lockstep or pool; [1]: pool steps with at least one sampled row busy (pool_sample_step_kernel ahead of
    // logit_step_kernel).  Kept side by side, so a pool that goes back and forth between the two states captures each once.
    StepGraphs graphs[2];
    int token_gen = 0;  // bumped by nh_set_tokens; part of the graph key
    bool opt_graphs = true, opt_fuse_ln = true;  // nh_set_option
    int opt_absorbed = 0;        // NH_OPT_ABSORBED_XATTN: 1 = numerics prototype, 2 = one-pass kernels
    AbsorbedState xabs;
    bool opt_align_keep = false; // NH_OPT_ALIGN_KEEP
    AlignState al;               // nh_align, nh_align_decoded
    AlignLive live;              // nh_align_capture
    BeamState beam;              // nh_decode_beam
    ScoreState score;            // nh_score
    GuardState guard;            // nh_set_guard, nh_guard_bias, nh_guard_report, nh_guard_apply
    // The context's one query buffer, fp16 [align_q_heads][C - 1][max_batch][64]: nh_align's teacher-forced pass and the decodes
    // under nh_align_capture both write it, stages 2 - 6 read it.  Grown by align_q_buffer alone.
    DevBuf align_q;
    int align_q_heads = 0;
    int dec_layer_limit = 0;    // parity view (NH_OPT_DECODER_LAYER_LIMIT): run only the first n decoder blocks; 0 = all
    std::vector<int32_t> seq_lang;  // per-sequence language tokens (LanguageState::Detect), empty = tk.lang for all
    // nh_set_prompts: what the next decodes of the current lockstep batch put in front of [sot, lang?, task]: n_prefix ids per
    // clip, [prompt_batch][n_prefix].  Bound to the batch like seq_lang (clear_prompt); n_prefix == 0: none.
    std::vector<int32_t> prompt;
    int n_prefix = 0, prompt_batch = 0;
    bool opt_prompt_stepwise = false;   // NH_OPT_PROMPT_STEPWISE
    int32_t *d_lang_tokens = nullptr, *d_lang_out = nullptr;
    float *d_lang_probs = nullptr;
    RuleTokens tk{};
    bool have_tokens = false;
    int VP = 0;
    // pinned host staging
    int32_t *h_done = nullptr;
    // state
    int cur_batch = 0, frames = 0, S = 0, last_frames = -1;
    bool have_mel = false, have_enc = false;
    // timings
    hipEvent_t ev[7]{};
    nh_timings tm{};
    bool profile_gemm = false;
    std::vector<hipEvent_t> gemm_ev;
    size_t gemm_ev_used = 0;
    double gemm_flops_acc = 0.0;

    int fail(int code, const std::string &msg) { err = msg; return code; }
    // Device current, stream drained, step graphs, events, h_done, stream (nh_model.hip); the members -- the arena, every
    // DevBuf, then the model -- release themselves after that.  A context whose stream or events were never made destructs too.
    ~nh_ctx();
};

#define NH_STAGE_BYTES (256ull << 20)   // ctx->stage per group of clips or frames (the alignment workspace's figure)

inline int DevBuf::reserve(nh_ctx *ctx, size_t need, const char *what, bool zero) {
    if (bytes >= need) return NH_OK;
    HIPCHK(hipStreamSynchronize(ctx->st));   // nothing may still read what goes away
    if (p) hipFree(p);
    p = nullptr; bytes = 0;
    if (hipMalloc(&p, need) != hipSuccess) {
        p = nullptr; (void)hipGetLastError();
        return ctx->fail(NH_ERR_NOMEM, std::string("hipMalloc(") + what + ")");
    }
    bytes = need;
    if (zero) HIPCHK(hipMemsetAsync(p, 0, need, ctx->st));
    return NH_OK;
}

void drop_graphs(nh_ctx *ctx, int first = 0);   // nh_decode.hip
void decoder_step(nh_ctx *ctx, int pos, const int32_t *pos_ptr = nullptr, bool final_ln = true, bool skip_done = false,
                  const AlignHeadSet *keep = nullptr);   // nh_decode.hip
int ensure_decoder_repack(nh_ctx *ctx);         // nh_model.hip
// nh_decode.hip, shared with nh_beam.hip: the refusals and the prompt phase every lockstep decode begins with, the logits of
// the R rows of the last decoder_step(..., final_ln = false), and what Model::decode returns for one sequence
struct DecodePrompt { int B, NP, P, PL, steps; };   // batch, prefix length, prompt length (2 | 3), NP + P, decoder steps so far
int decode_refusals(nh_ctx *ctx);
int decode_prompt_phase(nh_ctx *ctx, int max_new_tokens, DecodePrompt &dp);
void logits_from_dx(nh_ctx *ctx, int R);
// nh_guard.hip: the guard's launch on the R rows whose logits the step just wrote, ahead of the selection kernels.  Callers
// check ctx->guard.on first: with the guard off a step emits nothing.  pos: a pool's per-row positions, nullptr otherwise;
// clips: the batch's clips (row r uses the bias list of context row r % clips).
void emit_guard(nh_ctx *ctx, int R, int prompt_len, const int32_t *pos, int clips);
// LayerNorm of R rows of f32 x[R][K]: the sliced summation tree of the decode step where the width allows, so that the fused
// and the stand-alone forms, every batch size and the one-pass forward give bit-identical rows
void dec_layernorm(nh_ctx *ctx, const LnW &ln, const float *x, half_t *y, float *y32, int R, int K);
// Given tokens onto the device: the zero-padded [cur_batch][max_target_positions] image of ds.tokens.  Clip b brings
// tokens[b * stride + i], i < n_each[b] (n_each == nullptr: i < n_all for every clip).  Every id is checked against the
// vocabulary (`who` names the caller in the refusal) before anything is touched; then the decoder repack, the wait for the
// encoder, the copy, and the stream drained.  What the last decode left for nh_align_decoded is gone after it.
int stage_given_tokens(nh_ctx *ctx, const char *who, const int32_t *tokens, size_t stride, int n_all, const int32_t *n_each = nullptr);
// The decode state of rows 0 .. B-1 on its way to the host, queued on the context's stream (the caller drains it).  Token rows:
// rows[0 .. n) of the context (rows == nullptr: rows 0 .. n-1), packed.
struct HostDecodeState { std::vector<int32_t> toks, nt, done; std::vector<double> slp, nsp; };
int queue_decode_state(nh_ctx *ctx, const int32_t *rows, int n, int B, HostDecodeState &h);
void finish_sequence(nh_ctx *ctx, int32_t *t, int n, int done, double slp, double nsp, int32_t *out_tokens, nh_decode_result &r, int skip = 0);
// nh_prefill.hip: TextDecoder::forward over positions 0 .. T-1 of ds.tokens for the rows of the lockstep batch in one pass:
// self K/V of those positions land in the caches.  hidden == nullptr (a decode's prefix): the last block stops once its K/V
// are written; otherwise everything, the final LayerNorm included, and the B * T rows are copied to `hidden` (host f32).
// keep_rows (with hidden == nullptr; nh_score): everything as well, but the final LayerNorm's fp16 rows [B * T][d] stay in
// ctx->xn, nothing is copied to the host and the stream is not waited for.
bool prefill_supported(const nh_ctx *ctx);
// Shortest prefix the default route sends through the one pass.  Its fifteen-odd launches on a handful of rows cost 0.64 - 0.76 ms
// at distil-large-v3's shape with 32 clips whatever the length, a decode step 0.18 ms: measured 0.64 / 0.67 / 0.71 ms against
// 0.17 / 0.36 / 0.73 ms stepwise at 1 / 2 / 4 tokens (tools/dbg/prompt_cost.py, profiles/prompt_cost.json): the crossover
// lies between 2 and 4.
#define NH_PREFILL_MIN_PREFIX 4
// The ragged form (clips != nullptr: n host entries, rows and lengths; the offsets are filled in here): the given context rows,
// clip i over its own positions 0 .. T_i - 1, packed; T is ignored, hidden and keep_rows are not offered.  The table goes up
// in one copy from pfx_host.  A decode pool's prefixes (nh_pool_step).
int prefill_forward(nh_ctx *ctx, int T, float *hidden, bool keep_rows = false, PfClip *clips = nullptr, int n = 0);
inline void clear_prompt(nh_ctx *ctx) { ctx->prompt.clear(); ctx->n_prefix = 0; ctx->prompt_batch = 0; }
// nh_encode.hip: may `batch` clips of these lengths become rows row0 .. of the context's mel batch?  Row range, clip lengths,
// equal mel frames, the pool and row-gap rules.  Changes nothing in the context: every entry point that fills PCM rows
// calls it before its first copy or launch.
int check_batch(nh_ctx *ctx, const int32_t *n_samples, int batch, int row0 = 0);
// ... and what follows an accepted check: the batch becomes the context's, then the log-mel of the clips of device PCM
int run_logmel(nh_ctx *ctx, const float *pcm_dev, const int32_t *n_samples, int64_t stride, int batch, int row0 = 0);
// nh_cut.hip: e[F] and E[F] of a recording in host (staged in groups) or device memory, queued on the context's stream
int cut_energies(nh_ctx *ctx, const float *pcm, int on_device, long long N, float *e, float *E, long long F, int half_window);
