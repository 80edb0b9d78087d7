// nh_cut.hip -- the C ABI of include/norma_hip.h, part 6: long recordings.  nh_cut_plan cuts a recording into clips of at most
// 30 s at the quietest frame near each clip's end (k_cut.hip), nh_cut_energy is its parity view, nh_logmel_chunks_rows feeds
// the planned clips to the log-mel.  The contract is in the header and in DESIGN.md 11.
#include "nh_ctx.h"

#define CUT_STAGE_FRAMES ((long long)(NH_STAGE_BYTES / (sizeof(float) * NH_CUT_HOP)))
static_assert(NH_CUT_HOP == NH_CUT_FRAME, "the public hop is the kernels' frame");

// Stages 1 and 2 of the contract, queued on the context's stream: e[F] and E[F] (device) of a recording of N samples.  Host PCM
// goes through the context's one staging in groups of whole frames, one energy launch per group.  nh_vad_plan starts here too.
int cut_energies(nh_ctx *ctx, const float *pcm, int on_device, long long N, float *e, float *E, long long F, int half_window) {
    if (on_device) {
        launch_cut_energy(pcm, N, e, F, ctx->st);
    } else {
        if (int rc = ctx->stage.reserve(ctx, sizeof(float) * (size_t)std::min(N, CUT_STAGE_FRAMES * NH_CUT_HOP), "PCM staging")) return rc;
        float *const stage = static_cast<float *>(ctx->stage.p);
        for (long long f0 = 0; f0 < F; f0 += CUT_STAGE_FRAMES) {
            const long long nf = std::min(CUT_STAGE_FRAMES, F - f0), ns = std::min(nf * NH_CUT_HOP, N - f0 * NH_CUT_HOP);
            HIPCHK(hipMemcpyAsync(stage, pcm + f0 * NH_CUT_HOP, sizeof(float) * (size_t)ns, hipMemcpyHostToDevice, ctx->st));
            launch_cut_energy(stage, ns, e + f0, nf, ctx->st);
        }
    }
    launch_cut_window(e, E, F, half_window, ctx->st);
    return NH_OK;
}

extern "C" int nh_cut_plan(nh_ctx *ctx, const float *pcm, int on_device, int64_t n_samples, const nh_cut_params *p,
                           int64_t *starts, int32_t *lens, int cap, int32_t *n_chunks) {
    if (!ctx || !pcm || !starts || !lens || !n_chunks) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_cut_plan: bad arguments") : NH_ERR_INVALID;
    const nh_cut_params q = p ? *p : nh_cut_params{NH_N_FRAMES, 2000, 15};
    if (n_samples < 1 || n_samples > (int64_t)INT32_MAX) return ctx->fail(NH_ERR_INVALID, "nh_cut_plan: n_samples must be in [1, 2^31 - 1]");
    if (q.max_frames < 1 || q.max_frames > NH_N_FRAMES) return ctx->fail(NH_ERR_INVALID, "nh_cut_plan: max_frames must be in [1, 3000]");
    if (q.min_frames < 1 || q.min_frames > q.max_frames) return ctx->fail(NH_ERR_INVALID, "nh_cut_plan: min_frames must be in [1, max_frames]");
    if (q.half_window < 0 || q.half_window > 100) return ctx->fail(NH_ERR_INVALID, "nh_cut_plan: half_window must be in [0, 100]");
    hipSetDevice(ctx->dev);
    CutState &cs = ctx->cut;
    const long long N = n_samples, F = (N + NH_CUT_HOP - 1) / NH_CUT_HOP;
    const int into = cs.view == 0 ? 1 : 0;   // the view's workspace is never the one that grows
    if (int rc = cs.ws[into].reserve(ctx, sizeof(float) * 2 * (size_t)F, "frame energies")) return rc;
    float *const e = static_cast<float *>(cs.ws[into].p), *const E = e + F;
    // a chunk that is not the last holds at least min_frames frames; the device records at most what the caller can take
    const long long bound = F / q.min_frames + 1;
    const long long kcap = std::min(bound, (long long)std::max(cap, 1));
    Carve cv;
    const size_t o_starts = cv.take(sizeof(long long) * (size_t)kcap), o_lens = cv.take(sizeof(int32_t) * (size_t)kcap), o_count = cv.take(sizeof(int32_t));
    if (int rc = cs.out.reserve(ctx, cv.off, "chunk records")) return rc;
    long long *const d_starts = cs.out.at<long long>(o_starts);
    int32_t *const d_lens = cs.out.at<int32_t>(o_lens), *const d_count = cs.out.at<int32_t>(o_count);
    if (int rc = cut_energies(ctx, pcm, on_device, N, e, E, F, q.half_window)) return rc;
    CutSearch s{};
    s.E = E; s.F = F; s.min_frames = q.min_frames; s.max_frames = q.max_frames; s.n_samples = N;
    s.starts = d_starts; s.lens = d_lens; s.count = d_count; s.cap = kcap;
    launch_cut_search(s, ctx->st);
    HIPCHK(hipGetLastError());
    int32_t n = 0;
    HIPCHK(hipMemcpyAsync(&n, d_count, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    *n_chunks = n;
    if (n > cap) return ctx->fail(NH_ERR_INVALID, "nh_cut_plan: the plan has " + std::to_string(n) + " chunks, cap is " + std::to_string(cap));
    HIPCHK(hipMemcpyAsync(starts, d_starts, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(lens, d_lens, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    cs.view = into;
    cs.F = F;
    return NH_OK;
}

extern "C" int nh_cut_energy(nh_ctx *ctx, float *e, float *E, int64_t cap_frames) {
    if (!ctx) return NH_ERR_INVALID;
    const CutState &cs = ctx->cut;
    if (cs.view < 0) return ctx->fail(NH_ERR_STATE, "nh_cut_energy: no plan yet");
    if (cap_frames < cs.F) return ctx->fail(NH_ERR_INVALID, "nh_cut_energy: the last plan has " + std::to_string(cs.F) + " frames");
    hipSetDevice(ctx->dev);
    const float *w = static_cast<const float *>(cs.ws[cs.view].p);   // e[F] then E[F]
    if (e) HIPCHK(hipMemcpyAsync(e, w, sizeof(float) * (size_t)cs.F, hipMemcpyDeviceToHost, ctx->st));
    if (E) HIPCHK(hipMemcpyAsync(E, w + cs.F, sizeof(float) * (size_t)cs.F, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    return NH_OK;
}

extern "C" int nh_logmel_chunks_rows(nh_ctx *ctx, const float *pcm, int on_device, const int64_t *starts, const int32_t *n_samples,
                                     int batch, int row0) {
    if (!ctx || !pcm || !starts || !n_samples) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_logmel_chunks_rows: bad arguments") : NH_ERR_INVALID;
    hipSetDevice(ctx->dev);
    if (!ctx->mdl->have_filters) return ctx->fail(NH_ERR_STATE, "nh_logmel_chunks_rows: mel filters not set");
    if (int rc = check_batch(ctx, n_samples, batch, row0)) return rc;
    for (int b = 0; b < batch; b++)
        if (starts[b] < 0) return ctx->fail(NH_ERR_INVALID, "nh_logmel_chunks_rows: negative start");
    float *dst = ctx->pcm + (size_t)row0 * NH_N_SAMPLES;
    for (int b = 0; b < batch; b++)
        HIPCHK(hipMemcpyAsync(dst + (size_t)b * NH_N_SAMPLES, pcm + starts[b], sizeof(float) * (size_t)n_samples[b],
                              on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->st));
    return run_logmel(ctx, dst, n_samples, NH_N_SAMPLES, batch, row0);
}
