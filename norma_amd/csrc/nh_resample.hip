// nh_resample.hip -- the C ABI of include/norma_hip.h, part 5: audio ingest.  Sample conversion, channel mixdown and resampling
// to 16 kHz on the device (k_resample.hip), in front of the log-mel: the filter design and its per-rate tables, the staging of
// host frames, nh_resample, nh_logmel_resampled_rows and nh_logmel_samples.  The contract is in the header and in DESIGN.md 10.
#include "nh_ctx.h"

#define RS_TARGET_HZ 16000
#define RS_ZERO_CROSSINGS 32.0
#define RS_ROLLOFF 0.92
#define RS_BETA 8.6
#define RS_MAX_TABLE (1 << 20)            // entries: a 4 MB table

struct RsDesign { int L = 0, M = 0, T = 0; double c = 0, W = 0; };

// L, M, T of a source rate; false where the contract refuses it
static bool resample_design(int src_hz, RsDesign &d) {
    if (src_hz < 8000 || src_hz > 192000) return false;
    int a = RS_TARGET_HZ, b = src_hz;
    while (b) { const int t = a % b; a = b; b = t; }
    d.L = RS_TARGET_HZ / a; d.M = src_hz / a;
    if (src_hz == RS_TARGET_HZ) { d.T = 0; d.c = 1.0; d.W = 0.0; return true; }
    d.c = RS_ROLLOFF * (d.L < d.M ? (double)d.L / (double)d.M : 1.0);
    d.W = RS_ZERO_CROSSINGS / d.c;
    d.T = 2 * (int)ceil(d.W);
    return (long long)d.L * d.T <= RS_MAX_TABLE;
}

static double bessel_i0(double x) {   // sum over k of ((x/2)^k / k!)^2
    double sum = 1.0, term = 1.0;
    const double q = 0.25 * x * x;
    for (int k = 1; k < 500; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

static double resample_h(const RsDesign &d, double u) {
    if (!(fabs(u) < d.W)) return 0.0;
    const double x = M_PI * d.c * u, r = u / d.W;
    const double sinc = x == 0.0 ? 1.0 : sin(x) / x;
    return d.c * sinc * bessel_i0(RS_BETA * sqrt(1.0 - r * r)) / bessel_i0(RS_BETA);
}

// the device table of src_hz (design already accepted), built on first use and kept with the model's shared tables
static int resample_table(nh_ctx *ctx, int src_hz, const RsDesign &d, const float **coef) {
    nh_model &m = *ctx->mdl;
    std::lock_guard<std::mutex> lk(m.mu);
    for (const auto &t : m.rs_tables)
        if (t.src_hz == src_hz) { *coef = t.coef; return NH_OK; }
    float *dev = nullptr;
    if (d.T > 0) {
        const int Wc = d.T / 2;
        std::vector<float> h((size_t)d.L * d.T);
        for (int p = 0; p < d.L; p++)
            for (int j = 0; j < d.T; j++) h[(size_t)p * d.T + j] = (float)resample_h(d, (double)p / (double)d.L - (double)(j - Wc + 1));
        dev = m.allocs.dalloc_into<float>(h.size(), false);
        if (!dev) return ctx->fail(NH_ERR_NOMEM, "hipMalloc(resampling filter)");
        HIPCHK(hipMemcpy(dev, h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice));
    }
    m.rs_tables.push_back({src_hz, d.L, d.M, d.T, dev});
    *coef = dev;
    return NH_OK;
}

static long long whole_clip_outputs(const RsDesign &d, long long n_frames) { return (n_frames * d.L + d.M - 1) / d.M; }

extern "C" int nh_resample_len(int src_hz, int64_t n_frames) {
    RsDesign d;
    if (!resample_design(src_hz, d) || n_frames < 1 || n_frames > (int64_t)INT32_MAX) return -1;
    const long long n = whole_clip_outputs(d, n_frames);
    return n >= 1 && n <= NH_N_SAMPLES ? (int)n : -1;
}

extern "C" int nh_resample_table(nh_ctx *ctx, int src_hz, float *coef, int32_t *L, int32_t *M, int32_t *T) {
    if (!ctx && coef) return NH_ERR_INVALID;   // the sizes alone need no context
    RsDesign d;
    if (!resample_design(src_hz, d))
        return ctx ? ctx->fail(NH_ERR_INVALID, "nh_resample_table: src_hz outside 8000 .. 192000, or a filter of more than 2^20 entries") : NH_ERR_INVALID;
    if (L) *L = d.L;
    if (M) *M = d.M;
    if (T) *T = d.T;
    if (!coef || d.T == 0) return NH_OK;
    hipSetDevice(ctx->dev);
    const float *dev = nullptr;
    if (int rc = resample_table(ctx, src_hz, d, &dev)) return rc;
    HIPCHK(hipMemcpy(coef, dev, sizeof(float) * (size_t)d.L * d.T, hipMemcpyDeviceToHost));
    return NH_OK;
}

extern "C" int nh_sample_size(int dt) {
    switch (dt) {
        case NH_SAMPLE_F32: case NH_SAMPLE_I32: case NH_SAMPLE_U32: return 4;
        case NH_SAMPLE_F64: case NH_SAMPLE_I64: case NH_SAMPLE_U64: return 8;
        case NH_SAMPLE_I16: case NH_SAMPLE_U16: return 2;
        case NH_SAMPLE_I8: case NH_SAMPLE_U8: return 1;
        default: return 0;
    }
}

// what a call says of its frames, whatever its clips: sample type, channels, rate (-> d), stride
static int resample_format(nh_ctx *ctx, const char *who, int dt, int channels, int src_hz, int64_t stride_frames, RsDesign &d) {
    const std::string w(who);
    if (!nh_sample_size(dt)) return ctx->fail(NH_ERR_INVALID, w + ": unknown sample type " + std::to_string(dt));
    if (channels < 1 || channels > 8) return ctx->fail(NH_ERR_INVALID, w + ": channels must be in [1, 8]");
    if (src_hz < 8000 || src_hz > 192000) return ctx->fail(NH_ERR_INVALID, w + ": src_hz must be in [8000, 192000]");
    if (!resample_design(src_hz, d)) return ctx->fail(NH_ERR_INVALID, w + ": the filter of this rate has more than 2^20 entries");
    if (stride_frames < 0) return ctx->fail(NH_ERR_INVALID, w + ": negative stride");
    if (resample_lds_bytes(d.L, d.M, d.T) > (size_t)NH_LDS_EXCLUSIVE) return ctx->fail(NH_ERR_INVALID, w + ": the window of one tile does not fit the LDS");
    return NH_OK;
}

// The clips' own checks, then the launches: clips -> PCM rows row0 .. of the context, after resample_format and with rows the
// caller has checked (check_batch, or nh_resample's range test).  n_final[batch], when given, receives the outputs written per
// clip.  Nothing is launched or allocated before every clip has passed.
static int resample_rows(nh_ctx *ctx, const char *who, const RsDesign &d, const void *frames, int on_device, int dt, int channels,
                         int src_hz, const int32_t *n_frames, int64_t stride_frames, int batch, const int64_t *num0,
                         const int32_t *n_out, int row0, int32_t *n_final) {
    const std::string w(who);
    std::vector<ResampleClip> clips((size_t)batch);
    int max_out = 0;
    for (int b = 0; b < batch; b++) {
        if (n_frames[b] < 1) return ctx->fail(NH_ERR_INVALID, w + ": a clip needs at least one frame");
        const long long no = n_out ? (long long)n_out[b] : whole_clip_outputs(d, n_frames[b]);
        if (no < 1 || no > NH_N_SAMPLES) return ctx->fail(NH_ERR_INVALID, w + ": a clip must yield 1 .. 480000 samples");
        const long long z = num0 ? (long long)num0[b] : 0;
        if (z < 0) return ctx->fail(NH_ERR_INVALID, w + ": num0 must not be negative");
        clips[b] = ResampleClip{(long long)b * stride_frames, z, n_frames[b], (int)no};
        if (n_final) n_final[b] = (int32_t)no;
        if ((int)no > max_out) max_out = (int)no;
    }
    const float *coef = nullptr;
    if (int rc = resample_table(ctx, src_hz, d, &coef)) return rc;
    if (int rc = ctx->rs_clips.reserve(ctx, sizeof(ResampleClip) * (size_t)ctx->B, "resample clip records")) return rc;
    ResampleClip *const d_clips = ctx->rs_clips.at<ResampleClip>();
    ResampleParams p{};
    p.dtype = dt; p.channels = channels; p.coef = coef; p.L = d.L; p.M = d.M; p.T = d.T; p.out_stride = NH_N_SAMPLES;
    const size_t fb = (size_t)nh_sample_size(dt) * (size_t)channels;   // bytes per frame
    if (on_device) {
        HIPCHK(hipMemcpyAsync(d_clips, clips.data(), sizeof(ResampleClip) * (size_t)batch, hipMemcpyHostToDevice, ctx->st));
        p.frames = frames; p.clips = d_clips; p.batch = batch; p.max_out = max_out;
        p.out = ctx->pcm + (size_t)row0 * NH_N_SAMPLES;
        if (!launch_resample(p, ctx->st)) return ctx->fail(NH_ERR_INVALID, w + ": launch refused");
        HIPCHK(hipGetLastError());
        return NH_OK;
    }
    // host frames: groups of clips packed back to back in the staging, one launch per group
    std::vector<std::pair<int, int>> groups;   // [first, last); a clip larger than the cap is staged alone
    size_t need = 0, run = 0;
    int g0 = 0;
    for (int b = 0; b < batch; b++) {
        const size_t bytes = (size_t)n_frames[b] * fb;
        if (b > g0 && run + bytes > NH_STAGE_BYTES) { groups.emplace_back(g0, b); g0 = b; run = 0; }
        run += bytes;
        need = std::max(need, run);
    }
    groups.emplace_back(g0, batch);
    if (int rc = ctx->stage.reserve(ctx, need, "native frame staging")) return rc;
    for (const auto &g : groups) {   // a clip's frames start where the previous clip of its group ends
        long long off = 0;
        for (int b = g.first; b < g.second; b++) { clips[b].off = off; off += n_frames[b]; }
    }
    HIPCHK(hipMemcpyAsync(d_clips, clips.data(), sizeof(ResampleClip) * (size_t)batch, hipMemcpyHostToDevice, ctx->st));
    for (const auto &g : groups) {
        int gmax = 0;
        for (int b = g.first; b < g.second; b++) {
            HIPCHK(hipMemcpyAsync(reinterpret_cast<char *>(ctx->stage.p) + (size_t)clips[b].off * fb,
                                  reinterpret_cast<const char *>(frames) + (size_t)b * (size_t)stride_frames * fb,
                                  (size_t)n_frames[b] * fb, hipMemcpyHostToDevice, ctx->st));
            gmax = std::max(gmax, clips[b].n_out);
        }
        p.frames = ctx->stage.p; p.clips = d_clips + g.first; p.batch = g.second - g.first; p.max_out = gmax;
        p.out = ctx->pcm + (size_t)(row0 + g.first) * NH_N_SAMPLES;
        if (!launch_resample(p, ctx->st)) return ctx->fail(NH_ERR_INVALID, w + ": launch refused");
    }
    HIPCHK(hipGetLastError());
    return NH_OK;
}

extern "C" int nh_resample(nh_ctx *ctx, const void *frames, int on_device, int sample_dtype, int channels, int src_hz,
                           const int32_t *n_frames, int64_t stride_frames, int batch, const int64_t *num0, const int32_t *n_out,
                           float *out_host, int64_t out_stride) {
    if (!ctx || !frames || !n_frames) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_resample: bad arguments") : NH_ERR_INVALID;
    hipSetDevice(ctx->dev);
    RsDesign d;
    if (int rc = resample_format(ctx, "nh_resample", sample_dtype, channels, src_hz, stride_frames, d)) return rc;
    if (batch < 1 || batch > ctx->B) return ctx->fail(NH_ERR_INVALID, "nh_resample: rows [row0, row0 + batch) must lie in [0, max_batch]");
    std::vector<int32_t> n((size_t)batch);
    if (int rc = resample_rows(ctx, "nh_resample", d, frames, on_device, sample_dtype, channels, src_hz, n_frames, stride_frames, batch,
                               num0, n_out, 0, n.data()))
        return rc;
    if (!out_host) return NH_OK;
    for (int b = 0; b < batch; b++)
        HIPCHK(hipMemcpyAsync(out_host + (size_t)b * (size_t)out_stride, ctx->pcm + (size_t)b * NH_N_SAMPLES, sizeof(float) * (size_t)n[b],
                              hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    return NH_OK;
}

extern "C" int nh_logmel_resampled_rows(nh_ctx *ctx, const void *frames, int on_device, int sample_dtype, int channels, int src_hz,
                                        const int32_t *n_frames, int64_t stride_frames, int batch, int row0) {
    if (!ctx || !frames || !n_frames) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_logmel_resampled_rows: bad arguments") : NH_ERR_INVALID;
    hipSetDevice(ctx->dev);
    if (!ctx->mdl->have_filters) return ctx->fail(NH_ERR_STATE, "nh_logmel_resampled_rows: mel filters not set");
    RsDesign d;
    if (int rc = resample_format(ctx, "nh_logmel_resampled_rows", sample_dtype, channels, src_hz, stride_frames, d)) return rc;
    std::vector<int32_t> n(batch > 0 ? (size_t)batch : 0);
    for (size_t b = 0; b < n.size(); b++) n[b] = nh_resample_len(src_hz, n_frames[b]);   // -1: no frames, or more than a row holds
    if (int rc = check_batch(ctx, n.data(), batch, row0)) return rc;
    if (int rc = resample_rows(ctx, "nh_logmel_resampled_rows", d, frames, on_device, sample_dtype, channels, src_hz, n_frames,
                               stride_frames, batch, nullptr, nullptr, row0, nullptr))
        return rc;
    return run_logmel(ctx, ctx->pcm + (size_t)row0 * NH_N_SAMPLES, n.data(), NH_N_SAMPLES, batch, row0);
}

// src/dtype.rs + dasp_sample's Sample::to_sample::<f32> (src/lib.rs:180,207), on the device: the native samples cross PCIe
// as they are and become Model::Data (f32) in HBM.  At 16 kHz and one channel the resample kernel takes no division and no
// tap: y[n] = sample_to_f32(s[n]).
extern "C" int nh_logmel_samples(nh_ctx *ctx, const void *pcm, int sample_dtype, const int32_t *n_samples, int64_t stride, int batch) {
    if (!ctx || !pcm || !n_samples) return ctx ? ctx->fail(NH_ERR_INVALID, "nh_logmel_samples: bad arguments") : NH_ERR_INVALID;
    if (!nh_sample_size(sample_dtype)) return ctx->fail(NH_ERR_INVALID, "nh_logmel_samples: unknown sample type " + std::to_string(sample_dtype));
    if (sample_dtype == NH_SAMPLE_F32) return nh_logmel(ctx, reinterpret_cast<const float *>(pcm), n_samples, stride, batch);
    hipSetDevice(ctx->dev);
    if (!ctx->mdl->have_filters) return ctx->fail(NH_ERR_STATE, "nh_logmel: mel filters not set");
    RsDesign d;
    if (int rc = resample_format(ctx, "nh_logmel_samples", sample_dtype, 1, RS_TARGET_HZ, stride, d)) return rc;
    if (int rc = check_batch(ctx, n_samples, batch)) return rc;
    if (int rc = resample_rows(ctx, "nh_logmel_samples", d, pcm, 0, sample_dtype, 1, RS_TARGET_HZ, n_samples, stride, batch, nullptr,
                               nullptr, 0, nullptr))
        return rc;
    return run_logmel(ctx, ctx->pcm, n_samples, NH_N_SAMPLES, batch);
}
