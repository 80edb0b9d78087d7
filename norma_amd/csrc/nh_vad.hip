// nh_vad.hip -- the C ABI of include/norma_hip.h, part 7: long recordings without their silence.  nh_vad_plan maps the speech of
// a recording and packs it into clips of at most 30 s (k_vad.hip, on the energies of k_cut.hip), nh_vad_view is its parity view,
// nh_logmel_pieces_rows gathers the planned clips into the PCM rows and feeds them to the log-mel.  The contract is in the
// header and in DESIGN.md 12.
#include "nh_ctx.h"

// A view workspace of F frames: regions (a, b pairs, 64-bit; F frames hold at most F / 2 + 1 runs), levels[3] + the region
// count, E[F], v3 (whole tiles)
struct VadLayout { long long max_regions; size_t levels, E, v3, bytes; };
static VadLayout vad_layout(long long F) {
    VadLayout l{};
    l.max_regions = F / 2 + 1;
    l.levels = 2 * sizeof(long long) * (size_t)l.max_regions;
    l.E = l.levels + 16;
    l.v3 = l.E + up16(sizeof(float) * (size_t)F);
    l.bytes = l.v3 + (size_t)((F + NH_VAD_TILE - 1) / NH_VAD_TILE) * NH_VAD_TILE;
    return l;
}

static bool vad_float_ok(float v) { return v >= 0.0f && !std::isinf(v); }   // false for a NaN

extern "C" int nh_vad_plan(nh_ctx *ctx, const float *pcm, int on_device, int64_t n_samples, const nh_vad_params *p,
                           int64_t *piece_starts, int32_t *piece_lens, int cap_pieces, int32_t *n_pieces,
                           int32_t *chunk_first, int cap_chunks, int32_t *n_chunks) {
    if (!ctx || !pcm || !piece_starts || !piece_lens || !n_pieces || !chunk_first || !n_chunks)
        return ctx ? ctx->fail(NH_ERR_INVALID, "nh_vad_plan: bad arguments") : NH_ERR_INVALID;
    const nh_vad_params q = p ? *p : nh_vad_params{NH_N_FRAMES, 2000, 15, 100, 900, 4.0f, 0.01f, 0.0f, 10, 20, 100};
    if (n_samples < 1 || n_samples > (int64_t)INT32_MAX) return ctx->fail(NH_ERR_INVALID, "nh_vad_plan: n_samples must be in [1, 2^31 - 1]");
    if (q.max_frames < 1 || q.max_frames > NH_N_FRAMES) return ctx->fail(NH_ERR_INVALID, "nh_vad_plan: max_frames must be in [1, 3000]");
    if (q.min_frames < 1 || q.min_frames > q.max_frames) return ctx->fail(NH_ERR_INVALID, "nh_vad_plan: min_frames must be in [1, max_frames]");
    if (q.half_window < 0 || q.half_window > 100) return ctx->fail(NH_ERR_INVALID, "nh_vad_plan: half_window must be in [0, 100]");
    if (q.lo_permille < 0 || q.hi_permille > 1000 || q.lo_permille > q.hi_permille)
        return ctx->fail(NH_ERR_INVALID, "nh_vad_plan: 0 <= lo_permille <= hi_permille <= 1000");
    if (!vad_float_ok(q.lo_ratio) || !vad_float_ok(q.hi_ratio) || !vad_float_ok(q.abs_floor))
        return ctx->fail(NH_ERR_INVALID, "nh_vad_plan: lo_ratio, hi_ratio and abs_floor must be finite and >= 0");
    if (q.min_speech_frames < 1 || q.min_speech_frames > NH_N_FRAMES) return ctx->fail(NH_ERR_INVALID, "nh_vad_plan: min_speech_frames must be in [1, 3000]");
    if (q.pad_frames < 0 || q.pad_frames > NH_N_FRAMES) return ctx->fail(NH_ERR_INVALID, "nh_vad_plan: pad_frames must be in [0, 3000]");
    if (q.min_gap_frames < 1 || q.min_gap_frames > NH_N_FRAMES) return ctx->fail(NH_ERR_INVALID, "nh_vad_plan: min_gap_frames must be in [1, 3000]");
    if (cap_pieces < 0 || cap_chunks < 0) return ctx->fail(NH_ERR_INVALID, "nh_vad_plan: negative cap");
    hipSetDevice(ctx->dev);
    VadState &vs = ctx->vad;
    const long long N = n_samples, F = (N + NH_CUT_HOP - 1) / NH_CUT_HOP;
    const long long n_tiles = (F + NH_VAD_TILE - 1) / NH_VAD_TILE, Fp = n_tiles * NH_VAD_TILE;
    const VadLayout lay = vad_layout(F);
    const long long max_regions = lay.max_regions;
    const int into = vs.view == 0 ? 1 : 0;     // the view's workspace is never the one that grows
    if (int rc = vs.ws[into].reserve(ctx, lay.bytes, "speech map")) return rc;
    char *const ws = static_cast<char *>(vs.ws[into].p);
    long long *const regions = reinterpret_cast<long long *>(ws);
    float *const levels = reinterpret_cast<float *>(ws + lay.levels);
    int *const n_regions = reinterpret_cast<int *>(ws + lay.levels) + 3;
    float *const E = reinterpret_cast<float *>(ws + lay.E);
    uint8_t *const v3 = reinterpret_cast<uint8_t *>(ws + lay.v3);
    // scratch: e, the select's state, four per-tile records, two flag buffers (whole tiles)
    const size_t o_sel = up16(sizeof(float) * (size_t)F), o_tiles = o_sel + up16(sizeof(VadSelect));
    const size_t o_flags = o_tiles + up16(4 * sizeof(int) * (size_t)n_tiles);
    if (int rc = vs.tmp.reserve(ctx, o_flags + 2 * (size_t)Fp, "speech map scratch")) return rc;
    char *const tmp = static_cast<char *>(vs.tmp.p);
    float *const e = reinterpret_cast<float *>(tmp);
    VadSelect *const sel = reinterpret_cast<VadSelect *>(tmp + o_sel);
    int *const tile_l = reinterpret_cast<int *>(tmp + o_tiles), *const tile_r = tile_l + n_tiles, *const carry_l = tile_r + n_tiles,
        *const carry_r = carry_l + n_tiles;
    uint8_t *const flags0 = reinterpret_cast<uint8_t *>(tmp + o_flags), *const flags1 = flags0 + Fp;
    // every region holds a piece, every further piece at least min_frames frames; the device records at most what the caller can take
    const long long kp = std::min(max_regions + F / q.min_frames + 1, (long long)std::max(cap_pieces, 1));
    const long long kc = std::min(max_regions + F / q.min_frames + 1, (long long)std::max(cap_chunks, 1));
    const size_t o_lens = sizeof(long long) * (size_t)kp, o_first = o_lens + sizeof(int32_t) * (size_t)kp,
                 o_counts = o_first + sizeof(int32_t) * (size_t)(kc + 1);
    if (int rc = vs.out.reserve(ctx, o_counts + 2 * sizeof(int32_t), "piece records")) return rc;
    char *const out = static_cast<char *>(vs.out.p);
    long long *const d_starts = reinterpret_cast<long long *>(out);
    int32_t *const d_lens = reinterpret_cast<int32_t *>(out + o_lens), *const d_first = reinterpret_cast<int32_t *>(out + o_first),
            *const d_counts = reinterpret_cast<int32_t *>(out + o_counts);

    HIPCHK(hipMemsetAsync(sel, 0, sizeof(VadSelect), ctx->st));
    if (int rc = cut_energies(ctx, pcm, on_device, N, e, E, F, q.half_window)) return rc;
    const VadLevels lv{q.lo_permille, q.hi_permille, q.lo_ratio, q.hi_ratio, q.abs_floor};
    for (int shift = 24; shift >= 0; shift -= 8) {
        launch_vad_hist(E, F, shift, sel, ctx->st);
        launch_vad_pick(sel, shift, lv, levels, ctx->st);
    }
    VadShape sh{};
    sh.E = E; sh.levels = levels; sh.F = F; sh.carry_l = carry_l; sh.carry_r = carry_r; sh.tile_l = tile_l; sh.tile_r = tile_r;
    sh.min_speech = q.min_speech_frames; sh.pad = q.pad_frames; sh.min_gap = q.min_gap_frames;
    sh.regions = regions; sh.carry_n = carry_l;
    const uint8_t *const ins[6] = {nullptr, flags0, flags1, flags0, v3, v3};
    uint8_t *const outs[6] = {flags0, flags1, flags0, v3, nullptr, nullptr};
    for (int step = 0; step < 6; step++) {
        sh.in = ins[step]; sh.out = outs[step];
        launch_vad_shape(step, sh, ctx->st);
        if (step <= 2) launch_vad_carry(tile_l, tile_r, carry_l, carry_r, (int)n_tiles, F, 0, nullptr, ctx->st);
        if (step == 4) launch_vad_carry(tile_l, tile_r, carry_l, carry_r, (int)n_tiles, F, 1, n_regions, ctx->st);
    }
    VadPieces pc{};
    pc.E = E; pc.regions = regions; pc.n_regions = n_regions; pc.min_frames = q.min_frames; pc.max_frames = q.max_frames;
    pc.n_samples = N; pc.starts = d_starts; pc.lens = d_lens; pc.cap_pieces = kp; pc.chunk_first = d_first; pc.cap_chunks = kc;
    pc.counts = d_counts;
    launch_vad_pieces(pc, ctx->st);
    HIPCHK(hipGetLastError());
    int32_t n[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(n, d_counts, sizeof(n), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    if (n[0] > cap_pieces || n[1] > cap_chunks) {
        *n_pieces = n[0]; *n_chunks = n[1];
        return ctx->fail(NH_ERR_INVALID, "nh_vad_plan: the plan has " + std::to_string(n[0]) + " pieces in " + std::to_string(n[1]) +
                                             " chunks, the caps are " + std::to_string(cap_pieces) + " and " + std::to_string(cap_chunks));
    }
    HIPCHK(hipMemcpyAsync(piece_starts, d_starts, sizeof(int64_t) * (size_t)n[0], hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(piece_lens, d_lens, sizeof(int32_t) * (size_t)n[0], hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(chunk_first, d_first, sizeof(int32_t) * (size_t)(n[1] + 1), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    *n_pieces = n[0]; *n_chunks = n[1];
    vs.view = into;
    vs.F = F;
    return NH_OK;
}

extern "C" int nh_vad_view(nh_ctx *ctx, float *E, uint8_t *speech, int64_t cap_frames, float levels[3], int64_t *regions, int cap_regions,
                           int32_t *n_regions) {
    if (!ctx) return NH_ERR_INVALID;
    const VadState &vs = ctx->vad;
    if (vs.view < 0) return ctx->fail(NH_ERR_STATE, "nh_vad_view: no plan yet");
    if ((E || speech) && cap_frames < vs.F) return ctx->fail(NH_ERR_INVALID, "nh_vad_view: the last plan has " + std::to_string(vs.F) + " frames");
    hipSetDevice(ctx->dev);
    const char *ws = static_cast<const char *>(vs.ws[vs.view].p);
    const VadLayout lay = vad_layout(vs.F);
    struct { float levels[3]; int32_t n_regions; } lv;
    HIPCHK(hipMemcpyAsync(&lv, ws + lay.levels, sizeof(lv), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    if (n_regions) *n_regions = lv.n_regions;
    if (regions && cap_regions < lv.n_regions)
        return ctx->fail(NH_ERR_INVALID, "nh_vad_view: the last plan has " + std::to_string(lv.n_regions) + " regions");
    if (levels) memcpy(levels, lv.levels, sizeof(lv.levels));
    if (E) HIPCHK(hipMemcpyAsync(E, ws + lay.E, sizeof(float) * (size_t)vs.F, hipMemcpyDeviceToHost, ctx->st));
    if (speech) HIPCHK(hipMemcpyAsync(speech, ws + lay.v3, (size_t)vs.F, hipMemcpyDeviceToHost, ctx->st));
    if (regions) HIPCHK(hipMemcpyAsync(regions, ws, 2 * sizeof(int64_t) * (size_t)lv.n_regions, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    return NH_OK;
}

// The piece table of a batch, checked: nullptr and totals[b] = the samples of chunk b, or what is wrong with it.  The only
// host code here that indexes by what the caller passed.
static const char *vad_check_pieces(const int64_t *piece_starts, const int32_t *piece_lens, const int32_t *chunk_first, int batch,
                                    std::vector<int32_t> &totals) {
    if (chunk_first[0] < 0) return "nh_logmel_pieces_rows: chunk_first must ascend from 0 or above";
    totals.assign((size_t)batch, 0);
    for (int b = 0; b < batch; b++) {
        if (chunk_first[b + 1] < chunk_first[b]) return "nh_logmel_pieces_rows: chunk_first must ascend";
        if (chunk_first[b + 1] == chunk_first[b]) return "nh_logmel_pieces_rows: a chunk without a piece";
        long long total = 0;
        for (int32_t j = chunk_first[b]; j < chunk_first[b + 1]; j++) {
            if (piece_lens[j] < 1) return "nh_logmel_pieces_rows: piece length below 1";
            if (piece_starts[j] < 0) return "nh_logmel_pieces_rows: negative start";
            total += piece_lens[j];
            if (total > NH_N_SAMPLES) return "nh_logmel_pieces_rows: a chunk's pieces must total at most 480000 samples";
        }
        totals[(size_t)b] = (int32_t)total;
    }
    return nullptr;
}

extern "C" int nh_logmel_pieces_rows(nh_ctx *ctx, const float *pcm, int on_device, const int64_t *piece_starts, const int32_t *piece_lens,
                                     const int32_t *chunk_first, int batch, int row0) {
    if (!ctx || !pcm || !piece_starts || !piece_lens || !chunk_first)
        return ctx ? ctx->fail(NH_ERR_INVALID, "nh_logmel_pieces_rows: bad arguments") : NH_ERR_INVALID;
    hipSetDevice(ctx->dev);
    if (!ctx->mdl->have_filters) return ctx->fail(NH_ERR_STATE, "nh_logmel_pieces_rows: mel filters not set");
    if (batch < 1 || batch > ctx->B) return ctx->fail(NH_ERR_INVALID, "rows [row0, row0 + batch) must lie in [0, max_batch]");
    std::vector<int32_t> totals;
    if (const char *why = vad_check_pieces(piece_starts, piece_lens, chunk_first, batch, totals)) return ctx->fail(NH_ERR_INVALID, why);
    if (int rc = check_batch(ctx, totals.data(), batch, row0)) return rc;
    float *dst = ctx->pcm + (size_t)row0 * NH_N_SAMPLES;
    const int32_t j0 = chunk_first[0], n_pieces = chunk_first[batch] - j0;
    if (!on_device) {
        for (int b = 0; b < batch; b++) {
            size_t at = 0;
            for (int32_t j = chunk_first[b]; j < chunk_first[b + 1]; at += (size_t)piece_lens[j], j++)
                HIPCHK(hipMemcpyAsync(dst + (size_t)b * NH_N_SAMPLES + at, pcm + piece_starts[j], sizeof(float) * (size_t)piece_lens[j],
                                      hipMemcpyHostToDevice, ctx->st));
        }
        return run_logmel(ctx, dst, totals.data(), NH_N_SAMPLES, batch, row0);
    }
    // device PCM: one table, one copy, one launch.  [batch + 1] first piece of every chunk (from 0), [n] first sample, [n] samples
    // of the chunk before the piece, [batch] totals
    VadState &vs = ctx->vad;
    std::vector<long long> &tab = vs.h_tab;
    tab.assign((size_t)(batch + 1) + 2 * (size_t)n_pieces + (size_t)batch, 0);
    long long *const first = tab.data(), *const src0 = first + batch + 1, *const off = src0 + n_pieces, *const tot = off + n_pieces;
    bool vec4 = reinterpret_cast<uintptr_t>(pcm) % 16 == 0;
    long long max_total = 0;
    for (int b = 0; b < batch; b++) {
        first[b] = chunk_first[b] - j0;
        long long at = 0;
        for (int32_t j = chunk_first[b]; j < chunk_first[b + 1]; j++) {
            src0[j - j0] = piece_starts[j];
            off[j - j0] = at;
            at += piece_lens[j];
            // a group of four samples must not straddle two pieces, nor start off a 16-byte boundary
            if (piece_starts[j] % 4 != 0 || (j + 1 < chunk_first[b + 1] && piece_lens[j] % 4 != 0)) vec4 = false;
        }
        tot[b] = at;
        max_total = std::max(max_total, at);
    }
    first[batch] = n_pieces;
    if (int rc = vs.tab.reserve(ctx, sizeof(long long) * tab.size(), "piece table")) return rc;
    HIPCHK(hipMemcpyAsync(vs.tab.p, tab.data(), sizeof(long long) * tab.size(), hipMemcpyHostToDevice, ctx->st));
    VadGather g{};
    g.src = pcm; g.dst = dst; g.dst_stride = NH_N_SAMPLES; g.tab = static_cast<const long long *>(vs.tab.p);
    g.n_pieces = n_pieces; g.vec4 = vec4 ? 1 : 0;
    launch_vad_gather(g, batch, max_total, ctx->st);
    HIPCHK(hipGetLastError());
    return run_logmel(ctx, dst, totals.data(), NH_N_SAMPLES, batch, row0);
}
