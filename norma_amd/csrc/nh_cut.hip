// nh_cut.hip -- the C ABI of include/norma_hip.h, part 6: long recordings.  nh_cut_plan cuts a recording into clips of at most
// 30 s at the quietest frame near each clip's end (k_cut.hip), nh_cut_energy is its parity view, nh_logmel_chunks_rows feeds
// the planned clips to the log-mel.  The contract is in the header and in DESIGN.md 11.
#include "nh_ctx.h"

#define CUT_STAGE_BYTES (256ull << 20)    // staging of host PCM per group of frames (nh_resample's figure)
#define CUT_STAGE_FRAMES ((long long)(CUT_STAGE_BYTES / (sizeof(float) * NH_CUT_HOP)))
static_assert(NH_CUT_HOP == NH_CUT_FRAME, "the public hop is the kernels' frame");

// room for F frames in workspace w; the view's workspace is never the one that grows
static int cut_workspace(nh_ctx *ctx, CutState::Ws &w, long long F) {
    if (w.frames >= F) return NH_OK;
    HIPCHK(hipStreamSynchronize(ctx->st));   // nothing may still read what goes away
    if (w.e) hipFree(w.e);
    if (w.E) hipFree(w.E);
    w.e = w.E = nullptr; w.frames = 0;
    if (hipMalloc(reinterpret_cast<void **>(&w.e), sizeof(float) * (size_t)F) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&w.E), sizeof(float) * (size_t)F) != hipSuccess) {
        if (w.e) hipFree(w.e);
        w.e = w.E = nullptr;
        return ctx->fail(NH_ERR_NOMEM, "hipMalloc(frame energies)");
    }
    w.frames = F;
    return NH_OK;
}

static int cut_outputs(nh_ctx *ctx, long long cap) {
    CutState &cs = ctx->cut;
    if (!cs.count && hipMalloc(reinterpret_cast<void **>(&cs.count), sizeof(int32_t)) != hipSuccess)
        return ctx->fail(NH_ERR_NOMEM, "hipMalloc(chunk count)");
    if (cs.out_cap >= cap) return NH_OK;
    HIPCHK(hipStreamSynchronize(ctx->st));
    if (cs.starts) hipFree(cs.starts);
    if (cs.lens) hipFree(cs.lens);
    cs.starts = nullptr; cs.lens = nullptr; cs.out_cap = 0;
    if (hipMalloc(reinterpret_cast<void **>(&cs.starts), sizeof(long long) * (size_t)cap) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&cs.lens), sizeof(int32_t) * (size_t)cap) != hipSuccess) {
        if (cs.starts) hipFree(cs.starts);
        cs.starts = nullptr;
        return ctx->fail(NH_ERR_NOMEM, "hipMalloc(chunk records)");
    }
    cs.out_cap = cap;
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
    CutState::Ws &w = cs.ws[cs.view == 0 ? 1 : 0];
    if (int rc = cut_workspace(ctx, w, F)) return rc;
    // a chunk that is not the last holds at least min_frames frames; the device records at most what the caller can take
    const long long bound = F / q.min_frames + 1;
    const long long kcap = std::min(bound, (long long)std::max(cap, 1));
    if (int rc = cut_outputs(ctx, kcap)) return rc;
    if (on_device) {
        launch_cut_energy(pcm, N, w.e, F, ctx->st);
    } else {
        const size_t need = sizeof(float) * (size_t)std::min(N, CUT_STAGE_FRAMES * NH_CUT_HOP);
        if (cs.stage_bytes < need) {
            HIPCHK(hipStreamSynchronize(ctx->st));
            if (cs.stage) hipFree(cs.stage);
            cs.stage = nullptr; cs.stage_bytes = 0;
            if (hipMalloc(reinterpret_cast<void **>(&cs.stage), need) != hipSuccess) return ctx->fail(NH_ERR_NOMEM, "hipMalloc(PCM staging)");
            cs.stage_bytes = need;
        }
        for (long long f0 = 0; f0 < F; f0 += CUT_STAGE_FRAMES) {   // the stream orders a group's copy behind the kernel that read the one before
            const long long nf = std::min(CUT_STAGE_FRAMES, F - f0), ns = std::min(nf * NH_CUT_HOP, N - f0 * NH_CUT_HOP);
            HIPCHK(hipMemcpyAsync(cs.stage, pcm + f0 * NH_CUT_HOP, sizeof(float) * (size_t)ns, hipMemcpyHostToDevice, ctx->st));
            launch_cut_energy(cs.stage, ns, w.e + f0, nf, ctx->st);
        }
    }
    launch_cut_window(w.e, w.E, F, q.half_window, ctx->st);
    CutSearch s{};
    s.E = w.E; s.F = F; s.min_frames = q.min_frames; s.max_frames = q.max_frames; s.n_samples = N;
    s.starts = cs.starts; s.lens = cs.lens; s.count = cs.count; s.cap = kcap;
    launch_cut_search(s, ctx->st);
    HIPCHK(hipGetLastError());
    int32_t n = 0;
    HIPCHK(hipMemcpyAsync(&n, cs.count, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    *n_chunks = n;
    if (n > cap) return ctx->fail(NH_ERR_INVALID, "nh_cut_plan: the plan has " + std::to_string(n) + " chunks, cap is " + std::to_string(cap));
    HIPCHK(hipMemcpyAsync(starts, cs.starts, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(lens, cs.lens, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    cs.view = (int)(&w - cs.ws);
    cs.F = F;
    return NH_OK;
}

extern "C" int nh_cut_energy(nh_ctx *ctx, float *e, float *E, int64_t cap_frames) {
    if (!ctx) return NH_ERR_INVALID;
    const CutState &cs = ctx->cut;
    if (cs.view < 0) return ctx->fail(NH_ERR_STATE, "nh_cut_energy: no plan yet");
    if (cap_frames < cs.F) return ctx->fail(NH_ERR_INVALID, "nh_cut_energy: the last plan has " + std::to_string(cs.F) + " frames");
    hipSetDevice(ctx->dev);
    const CutState::Ws &w = cs.ws[cs.view];
    if (e) HIPCHK(hipMemcpyAsync(e, w.e, sizeof(float) * (size_t)cs.F, hipMemcpyDeviceToHost, ctx->st));
    if (E) HIPCHK(hipMemcpyAsync(E, w.E, sizeof(float) * (size_t)cs.F, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    return NH_OK;
}

extern "C" int nh_logmel_chunks_rows(nh_ctx *ctx, const float *pcm, int on_device, const int64_t *starts, const int32_t *n_samples,
                                     int batch, int row0) {
    if (!ctx || !pcm || !starts || !n_samples) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_logmel_chunks_rows: bad arguments") : NH_ERR_INVALID;
    hipSetDevice(ctx->dev);
    if (!ctx->mdl->have_filters) return ctx->fail(NH_ERR_STATE, "nh_logmel_chunks_rows: mel filters not set");
    if (batch < 1 || row0 < 0 || row0 + batch > ctx->B) return ctx->fail(NH_ERR_INVALID, "rows [row0, row0 + batch) must lie in [0, max_batch]");
    for (int b = 0; b < batch; b++) {
        if (starts[b] < 0) return ctx->fail(NH_ERR_INVALID, "nh_logmel_chunks_rows: negative start");
        if (n_samples[b] < 1 || n_samples[b] > NH_N_SAMPLES) return ctx->fail(NH_ERR_INVALID, "clip length must be in [1, 480000] samples");
    }
    float *dst = ctx->pcm + (size_t)row0 * NH_N_SAMPLES;
    for (int b = 0; b < batch; b++)
        HIPCHK(hipMemcpyAsync(dst + (size_t)b * NH_N_SAMPLES, pcm + starts[b], sizeof(float) * (size_t)n_samples[b],
                              on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->st));
    return run_logmel(ctx, dst, n_samples, NH_N_SAMPLES, batch, row0);
}
