/*
 * norma_hip.h -- C ABI of libnorma_hip.so: the MI355X (gfx950) Whisper hot path for norma.
 *
 * This is the drop-in boundary a `norma-hip-sys` FFI crate binds.  Plain
 * pointers and sizes only; no C++ or torch types.  Every function returns an int status
 * (NH_OK == 0) and never throws or aborts; nh_last_error() gives the message for the last
 * failure on that context.  A context is owned by one host thread (the reference's `Model` is
 * `Send`, not `Sync`: src/models/mod.rs:24, src/lib.rs:377,462-464).  One process may hold any number of contexts, on one
 * device or several, each driven by its own thread; they share nothing mutable.  Several contexts on ONE device are how the
 * latency-bound decode of one batch is overlapped with the encoder of the next (bench.py keeps three batches in flight).
 *
 * All citations are relative to the reference repository MikeIvanichev/norma @ 2024_10_08.
 *
 * What each entry point replaces:
 *   nh_create / nh_destroy        SelectedDevice -> device (src/models/mod.rs:47-55) and
 *                                 Whisper::load (src/models/whisper/monolingual.rs:371-373)
 *   nh_create_shared              (no counterpart: the reference is single-stream) further contexts over one weight set
 *   nh_load_tensor                VarBuilder::from_mmaped_safetensors tensor reads by HF name
 *                                 (monolingual.rs:237-239)
 *   nh_set_mel_filters            the include_bytes! filterbank (monolingual.rs:351-362)
 *   nh_set_tokens                 special-token ids + the four vocab masks (monolingual.rs:376-430)
 *   nh_logmel                     audio::pcm_to_mel + Tensor::from_vec + narrow
 *                                 (src/models/whisper/model.rs:74-88)
 *   nh_resample, nh_logmel_resampled_rows
 *                                 the capture side's channel mixdown and Sinc resampler (src/lib.rs:172-216)
 *   nh_cut_plan, nh_logmel_chunks_rows
 *                                 (no counterpart: the reference re-seeks sequentially, model.rs:100-146) the clips of a long
 *                                 recording for the batched path, cut in pauses
 *   nh_vad_plan, nh_logmel_pieces_rows
 *                                 (no counterpart) the same clips without the recording's silence: a speech map over the
 *                                 cut planner's energies, packed into clips of at most 30 s
 *   nh_encode                     Type::encoder_forward (model.rs:168, :455-464)
 *   nh_decode_greedy              Model::decode at t = 0 (model.rs:279-389) including the logit
 *                                 rules (model.rs:212-277), batched, on device
 *   nh_encoder_output, nh_decoder_forward, nh_final_linear, nh_apply_rules
 *                                 fine-grained views of the same state for layer-level parity:
 *                                 Type::decoder_forward / decoder_final_linear (model.rs:466-483)
 *   nh_decode_sampled             Model::decode at t > 0 (model.rs:340-348) under the seeded sampling contract below
 *   nh_detect_language            Model::detect_language (model.rs:194-210)
 *   nh_pool_detect_languages, nh_pool_languages
 *                                 the same for the clips of a decode pool, each in its own first decode step
 *   nh_reset                      Type::reset_kv_cache (model.rs:485-490)
 *   nh_set_prompts, nh_decoder_forward_onepass
 *                                 (no counterpart: every reference decode starts from [sot, lang?, task], model.rs:285-289)
 *                                 tokens in front of the prompt, consumed in one pass
 *   nh_pool_prefix                the same per row of a decode pool, every row its own length, one ragged pass: declared in
 *                                 norma_hip_pool.h
 */
#ifndef NORMA_HIP_H
#define NORMA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NH_OK 0
#define NH_ERR_INVALID 1   /* bad argument / unknown tensor name / wrong shape */
#define NH_ERR_HIP 2       /* a HIP runtime call failed (message has the hipError string) */
#define NH_ERR_STATE 3     /* call sequence error (e.g. decode before encode) */
#define NH_ERR_NOMEM 4

#define NH_DTYPE_F32 0
#define NH_DTYPE_F16 1

#define NH_MAX_BATCH 96     /* rows (clips) one context decodes together */
#define NH_N_SAMPLES 480000 /* candle m::N_SAMPLES (model.rs:69)  */
#define NH_N_FRAMES 3000    /* candle m::N_FRAMES  (model.rs:88)  */

typedef struct nh_ctx nh_ctx; /* opaque; owns all device memory and one HIP stream */

/* candle `Config` fields read from HF config.json (monolingual.rs:347). */
typedef struct nh_config {
    int32_t num_mel_bins;
    int32_t max_source_positions; /* 1500 */
    int32_t d_model;
    int32_t encoder_attention_heads;
    int32_t encoder_layers;
    int32_t vocab_size;
    int32_t max_target_positions; /* 448 */
    int32_t decoder_attention_heads;
    int32_t decoder_layers;
} nh_config;

/* norma `Model` token fields (model.rs:37-41) + ids used for first_token_supress. */
typedef struct nh_tokens {
    int32_t sot, eot;
    int32_t lang;  /* language token pushed after sot (model.rs:286-288); < 0: none */
    int32_t task;  /* transcribe / translate */
    int32_t no_speech, no_timestamps;
    int32_t zero_sec, one_sec; /* <|0.00|>, <|1.00|> */
} nh_tokens;

/* Result of one greedy decode (model.rs:494-499 DecodingResult, compression_ratio is always NaN). */
typedef struct nh_decode_result {
    int32_t n_tokens;       /* tokens written for this sequence, prompt and eot included (a prefix of nh_set_prompts is not) */
    int32_t no_speech_exit; /* 1: early return of model.rs:308-315 */
    double avg_logprob;
    double no_speech_prob;
} nh_decode_result;

/* ---- lifetime -------------------------------------------------------------------------------- */
/* device_ordinal: SelectedDevice::Rocm(ord).  max_batch: chunks processed per call (>= 1). */
int nh_create(int device_ordinal, const nh_config *cfg, int max_batch, nh_ctx **out);
/* Another context on the same device over the SAME weights as `parent` (the reference runs one stream per model,
 * src/lib.rs:462-464; a chunk-parallel caller keeps several batches in flight per GPU and must not pay 1.5 - 3.1 GB of HBM and a
 * separate weight stream per batch).  The new context has its own streams, workspaces, K/V caches, tokens (nh_set_tokens) and
 * decode state; everything nh_load_tensor / nh_set_mel_filters fill in is shared and reference counted: it is freed when the
 * last context of the family is destroyed, in any order.  Loading through ANY context of a family is seen by all of them and
 * must not overlap with a running call on another one (load once, then run); the run-time calls of different contexts may
 * overlap freely, one host thread per context. */
int nh_create_shared(nh_ctx *parent, int max_batch, nh_ctx **out);
void nh_destroy(nh_ctx *ctx);
const char *nh_last_error(const nh_ctx *ctx); /* ctx may be NULL: error of a failed nh_create */
/* 1 when built for and running on a gfx950 device visible to HIP, else 0 (no side effects). */
int nh_device_count(void);

/* ---- model state ----------------------------------------------------------------------------- */
/* name: HF tensor name, e.g. "model.encoder.layers.3.self_attn.q_proj.weight".  data: host
 * pointer, row-major, dtype NH_DTYPE_*.  Tensors candle does not read
 * ("model.encoder.embed_positions.weight", "proj_out.weight") are accepted and ignored. */
int nh_load_tensor(nh_ctx *ctx, const char *name, int dtype, const int64_t *shape, int ndim,
                   const void *data);
/* filters: f32 [num_mel_bins][201] */
int nh_set_mel_filters(nh_ctx *ctx, const float *filters, int n_mel);
int nh_set_tokens(nh_ctx *ctx, const nh_tokens *tk, const int32_t *suppress_tokens, int n_suppress);
/* Number of tensors still missing before the model can run (0 = complete). */
int nh_missing_tensors(const nh_ctx *ctx);

/* ---- the hot path ---------------------------------------------------------------------------- */
/* pcm: host f32 mono 16 kHz, `batch` clips back to back with stride `stride` samples, clip b has
 * n_samples[b] <= 480000 valid samples (the rest is treated as absent, exactly as pcm_to_mel pads
 * with zeros).  Computes the log-mel of every clip on device. */
int nh_logmel(nh_ctx *ctx, const float *pcm, const int32_t *n_samples, int64_t stride, int batch);
/* The sample types norma's `DType` trait admits (src/dtype.rs:37-45): the capture side hands the transcriber samples of the
 * device's native type and converts them with dasp_sample (`Sample::to_sample::<T::Data>`, src/lib.rs:180,207) to the model's
 * Data type -- f32 for Whisper (model.rs:49).  nh_logmel_samples takes the native samples (host memory) and does that
 * conversion on the GPU, so a 16-bit microphone stream crosses PCIe at 2 bytes per sample.  Conversions are dasp_sample's:
 *   i8/i16/i32/i64 -> f32:  (s as f32) / 2^(bits-1)          u8/u16/u32/u64 -> f32: the same after subtracting 2^(bits-1)
 *   f64 -> f32: s as f32 (round to nearest even)             f32: unchanged
 * (integer -> f32 conversions round to nearest even, as Rust's `as` does). */
#define NH_SAMPLE_F32 0
#define NH_SAMPLE_F64 1
#define NH_SAMPLE_I8 2
#define NH_SAMPLE_I16 3
#define NH_SAMPLE_I32 4
#define NH_SAMPLE_I64 5
#define NH_SAMPLE_U8 6
#define NH_SAMPLE_U16 7
#define NH_SAMPLE_U32 8
#define NH_SAMPLE_U64 9
/* Bytes per sample of an NH_SAMPLE_* type (0: unknown). */
int nh_sample_size(int sample_dtype);
/* Like nh_logmel, with `pcm` holding samples of type `sample_dtype` (host memory, `stride` SAMPLES between clips).  The
 * samples are staged and converted as nh_resample's host frames are, at 16 kHz and one channel (f32 goes to nh_logmel). */
int nh_logmel_samples(nh_ctx *ctx, const void *pcm, int sample_dtype, const int32_t *n_samples, int64_t stride, int batch);
/* ---- audio ingest: channel mixdown and resampling to 16 kHz on the device --------------------------------
 * The capture side of the reference mixes the device's channels down to mono and, when the device's rate is not
 * Model::SAMPLE_RATE, runs a sinc resampler before Model::transcribe sees a sample (src/lib.rs:172-216).  Here a clip is
 * n_frames frames of `channels` interleaved samples of one NH_SAMPLE_* type at src_hz, and
 *   1 every sample becomes f32 by the formulas above (nh_logmel_samples)
 *   2 mono[j] = (s[j][0] + s[j][1] + ...) / (float)channels: f32 additions in channel order, one IEEE division (the
 *     reference's `x.iter().sum() / channels`; integer input is summed in f32, not in the native type, and cannot overflow)
 *   3 g = gcd(16000, src_hz), L = 16000 / g, M = src_hz / g.  Output n sits at source position (num0 + n M) / L frames
 *     (num0: caller-supplied, in units of 1/L frame; 0 for a whole clip): i = floor of it, p = (num0 + n M) mod L, in 64-bit
 *     integers, and
 *       y[n] = sum over k = -Wc+1 .. Wc of coef[p][k] * mono[i + k]       one f32 accumulator, fmaf, k ascending
 *       coef[p][k] = (float)h(p/L - k),  h(u) = c sinc(c u) I0(8.6 sqrt(1 - (u/W)^2)) / I0(8.6) for |u| < W, else 0
 *       c = 0.92 min(1, L/M), W = 32 / c, Wc = ceil(W), T = 2 Wc taps;  sinc(x) = sin(pi x) / (pi x)
 *     (a Kaiser-windowed sinc with 32 zero crossings whose cut-off follows the lower of the two rates: stop band at or
 *     below -87 dB from the target Nyquist frequency on, -3 dB at 7.24 kHz when downsampling); evaluated on the host in
 *     double, once per src_hz and weight set.  Frames outside [0, n_frames) contribute nothing.
 *     src_hz == 16000: no filter, y[n] = mono[num0 + n] (T = 0), as the reference skips its resampler at equal rates.
 * A whole clip yields ceil(n_frames L / M) samples.  A clip's outputs are bit-identical alone or in a batch and from host or
 * device memory; outputs computed from a window of the clip's frames (num0 shifted accordingly) equal the whole clip's as
 * long as the window holds every in-range frame within Wc of their positions.
 * Refused with NH_ERR_INVALID, nothing launched, outputs untouched: unknown sample type; channels outside 1 .. 8; src_hz
 * outside 8000 .. 192000; L * T > 2^20 (the standard rates need at most 44 800 entries); n_frames < 1; n_out outside
 * 1 .. 480000; num0 < 0; batch or rows outside the context. */
/* samples a whole clip of n_frames frames at src_hz yields, or -1 where nh_resample would refuse it */
int nh_resample_len(int src_hz, int64_t n_frames);
/* The filter of src_hz as the device holds it (a view for tests): *L, *M, *T and, unless coef == NULL (sizes only, no device
 * work, ctx may be NULL), coef f32 [L][T] with coef[p][k + T/2 - 1] = (float)h(p/L - k).  src_hz == 16000: L = M = 1, T = 0. */
int nh_resample_table(nh_ctx *ctx, int src_hz, float *coef, int32_t *L, int32_t *M, int32_t *T);
/* frames: `batch` clips, clip b at frame b * stride_frames (host memory, or device memory when on_device != 0) with
 * n_frames[b] frames.  num0: host i64 [batch] or NULL (0); n_out: host i32 [batch] or NULL (the whole clip).  The result
 * lands in the context's PCM rows -- row b at b * 480000 floats, where nh_logmel puts host PCM -- and, when out_host is
 * given, is copied there (clip b at b * out_stride floats) and the stream synchronised.  Host frames are staged in groups
 * of clips that keep the native staging at or under 256 MiB (a clip that needs more on its own is staged alone).  The
 * context has ONE staging, shared by nh_resample*, nh_logmel_samples and nh_cut_plan, allocated by the first call that
 * needs it and grown on demand.  One launch per group; device frames: one launch. */
int nh_resample(nh_ctx *ctx, const void *frames, int on_device, int sample_dtype, int channels, int src_hz,
                const int32_t *n_frames, int64_t stride_frames, int batch, const int64_t *num0, const int32_t *n_out,
                float *out_host, int64_t out_stride);
/* Whole clips through nh_resample into the PCM rows row0 .., then exactly what nh_logmel_device_rows does on them (same row
 * rules; row0 = 0 is the plain batch).  No copy back, no synchronisation. */
int nh_logmel_resampled_rows(nh_ctx *ctx, const void *frames, int on_device, int sample_dtype, int channels, int src_hz,
                             const int32_t *n_frames, int64_t stride_frames, int batch, int row0);
/* ---- long recordings: cut chunks at the quietest frame, on the device --------------------------------------
 * The reference walks a recording sequentially and re-seeks to its last timestamp (model.rs:100-146); the batched path
 * decodes independent clips of at most 30 s.  nh_cut_plan chooses their boundaries in pauses instead of every 480 000
 * samples.  A recording is N >= 1 f32 mono samples at 16 kHz, in host or device memory; F = ceil(N / 160) analysis frames
 * (160 samples: the log-mel hop, half a timestamp unit), W = half_window.  All arithmetic is IEEE f32, unfused:
 *   1 e[f]: acc = 0; for j = 0 .. 159 ascending: x = pcm[160 f + j] (0 at or past N), p = x * x, acc = acc + p.  One
 *     accumulator in that order: a frame's bits do not depend on tiling, on N or on where the samples live.
 *   2 E[f]: acc = 0; for k = -W .. W ascending: acc = acc + e[f + k], a frame outside [0, F) adding 0.0f.
 *   3 s_0 = 0; while F - s_k > max_frames: best = +inf, c* = s_k + max_frames; for c = s_k + min_frames .. s_k + max_frames
 *     ascending: if E[c] <= best then best = E[c], c* = c; s_{k+1} = c*.  So a cut is the LATEST minimum of its range, a
 *     NaN is never chosen, and an all-NaN range cuts at s_k + max_frames.  Chunk k starts at starts[k] = 160 s_k and is
 *     lens[k] = min(160 (s_{k+1} - s_k), N - starts[k]) samples long; the last chunk runs to N.
 *   4 stages 1 - 3 run on the context's stream without returning to the host between cuts; only starts, lens and the count
 *     come back, and the call returns when they are on the host.
 * Refused with NH_ERR_INVALID, nothing launched, starts / lens and the view of nh_cut_energy untouched: n_samples < 1 or
 * > 2^31 - 1; max_frames outside 1 .. 3000; min_frames outside 1 .. max_frames; half_window outside 0 .. 100.  cap smaller
 * than the number of chunks is refused the same way as far as the caller can see -- starts, lens and the view of the plan
 * before stay as they were -- but *n_chunks is set to the number needed, so the caller can retry (the number is known only
 * once the search has run: it runs in a second workspace that becomes the view when the call succeeds).
 * Host PCM is staged in groups of whole frames that keep the staging at or under 256 MiB (the context's one staging, see
 * nh_resample).  Staging and workspaces are allocated by the first call that needs them and grow on demand.  The call touches nothing else in the context and is
 * legal in any state (before the tensors are loaded, beside a running decode pool).
 * Results for samples whose squares are subnormal are unspecified up to a flush to zero. */
#define NH_CUT_HOP 160                       /* samples per analysis frame: the log-mel hop, half a timestamp unit */
typedef struct nh_cut_params { int32_t max_frames, min_frames, half_window; } nh_cut_params;
/* p == NULL: the defaults {3000, 2000, 15}: chunks of at most 30 s, the cut searched in their last 10 s, a 0.31 s window.
 * starts: host i64 [cap], lens: host i32 [cap], n_chunks: host i32 [1]. */
int nh_cut_plan(nh_ctx *ctx, const float *pcm, int on_device, int64_t n_samples, const nh_cut_params *p,
                int64_t *starts, int32_t *lens, int cap, int32_t *n_chunks);
/* Parity view of the LAST successful plan: e and E, F floats each (host; either may be NULL).  NH_ERR_STATE before any
 * plan, NH_ERR_INVALID if cap_frames < F. */
int nh_cut_energy(nh_ctx *ctx, float *e, float *E, int64_t cap_frames);
/* Clip b = pcm[starts[b] .. starts[b] + n_samples[b]) of a recording in host or device (on_device != 0) memory goes to the
 * context's PCM row row0 + b; then exactly what nh_logmel_device_rows does on those rows (same row rules, the bits of a
 * log-mel of a copy of those samples).  No copy back, no synchronisation.  starts[b] >= 0, 1 <= n_samples[b] <= 480000.
 * A clip of fewer than 160 samples produces 1500 mel frames, not 3000, and is refused beside longer clips like in every
 * nh_logmel*; of a plan only the final chunk can be that short. */
int nh_logmel_chunks_rows(nh_ctx *ctx, const float *pcm, int on_device, const int64_t *starts,
                          const int32_t *n_samples, int batch, int row0);
/* ---- long recordings: keep the speech, drop the silence, on the device -------------------------------------
 * nh_cut_plan sends every sample of a recording through the encoder and the decode loop.  nh_vad_plan keeps the speech only:
 * a speech map over the same energies, packed into clips of at most 30 s, each clip a concatenation of pieces of the
 * recording.  A recording is N >= 1 f32 mono samples at 16 kHz, in host or device memory; F = ceil(N / 160) analysis frames;
 * e[f] and E[f] are EXACTLY stages 1 and 2 of nh_cut_plan (W = half_window): same arithmetic, same bits.  All float steps
 * are single IEEE f32 operations, everything else is integer, so numpy reproduces every bit.
 *   1 Levels.  S = the non-NaN values of E sorted ascending, F' = |S|.  Q_lo = S[lo_permille (F' - 1) / 1000], Q_hi =
 *     S[hi_permille (F' - 1) / 1000] (integer division in int64).  a = lo_ratio * Q_lo; b = hi_ratio * Q_hi; r = (b < a) ? b : a;
 *     T = (r > abs_floor) ? r : abs_floor.  F' = 0: T = abs_floor (and the view shows Q_lo = Q_hi = 0).  The two ratios are a
 *     floor taken from the quiet end and a ceiling taken from the loud end, and the smaller wins: a recording that is speech
 *     throughout loses only what lies 20 dB below its loud level, one whose noise is within 20 dB of its speech loses
 *     nothing.  The rule errs toward keeping audio.
 *   2 Raw flags.  raw[f] = !(E[f] <= T).  A NaN frame is speech: what cannot be judged is kept.
 *   3 Shaping, in this order, on frame indices.  (a) a maximal run of raw shorter than min_speech_frames is cleared: v1.
 *     (b) v2[f] is true if any v1[g] with |g - f| <= pad_frames and 0 <= g < F is true.  (c) a maximal run of !v2 that lies
 *     strictly between two speech runs and is shorter than min_gap_frames becomes speech: v3.  Leading and trailing silence
 *     are never filled.  Regions are the maximal runs [a, b) of v3, ascending.
 *   4 Pieces.  For each region in order: s = a; while b - s > max_frames: c* by stage 3 of nh_cut_plan over c = s + min_frames
 *     .. s + max_frames (the latest least E[c], a NaN never chosen, s + max_frames if nothing qualifies), emit [s, c*), s = c*;
 *     emit [s, b).  Piece j starts at sample 160 s_j and is min(160 len_j, N - 160 s_j) samples long.
 *   5 Chunks.  Greedy, in order: a chunk takes the next piece while it is empty or while its frame total plus that piece
 *     stays <= max_frames.  chunk_first[k] is the index of chunk k's first piece, chunk_first[n_chunks] = n_pieces.  A
 *     recording with no speech has 0 pieces and 0 chunks (chunk_first[0] = 0); that is not an error.
 *   6 No host round trip between the stages; only the piece and chunk records and the two counts come back, and the call
 *     returns when they are on the host.
 *   7 Refusals and subnormals as for nh_cut_plan.  NH_ERR_INVALID, nothing launched, outputs and the view untouched:
 *     n_samples outside 1 .. 2^31 - 1; max_frames, min_frames, half_window outside nh_cut_plan's ranges; lo_permille or
 *     hi_permille outside 0 .. 1000 or lo > hi; a ratio or abs_floor that is negative or not finite; min_speech_frames or
 *     min_gap_frames outside 1 .. 3000; pad_frames outside 0 .. 3000; a negative cap.  A cap smaller than its count looks the
 *     same to the caller, but BOTH *n_pieces and *n_chunks are set to what is needed (the plan ran in a second workspace that
 *     becomes the view only when the call succeeds).  Results for samples whose squares are subnormal are unspecified up to
 *     a flush to zero.
 * The defaults -- the quiet decile x 4, the loud decile - 20 dB, 0.1 s of speech, 0.2 s of padding, gaps of 1 s -- are design
 * choices that have not been tuned on real speech; what is tested is this arithmetic, not recognition accuracy.
 * The call owns its state (allocated by the first call, grown on demand), leaves the view of nh_cut_energy as it found it,
 * touches nothing else in the context and is legal in any state, like nh_cut_plan; host PCM goes through the context's one
 * staging in the same groups. */
typedef struct nh_vad_params {
    int32_t max_frames, min_frames, half_window;            /* as nh_cut_params, same ranges */
    int32_t lo_permille, hi_permille;                       /* 0..1000, lo <= hi */
    float   lo_ratio, hi_ratio, abs_floor;                  /* finite, >= 0 */
    int32_t min_speech_frames, pad_frames, min_gap_frames;  /* 1..3000, 0..3000, 1..3000 */
} nh_vad_params;                                            /* 44 bytes */
/* p == NULL: the defaults {3000, 2000, 15, 100, 900, 4.0f, 0.01f, 0.0f, 10, 20, 100}.  piece_starts: host i64 [cap_pieces],
 * piece_lens: host i32 [cap_pieces], chunk_first: host i32 [cap_chunks + 1], n_pieces / n_chunks: host i32 [1]. */
int nh_vad_plan(nh_ctx *ctx, const float *pcm, int on_device, int64_t n_samples, const nh_vad_params *p,
                int64_t *piece_starts, int32_t *piece_lens, int cap_pieces, int32_t *n_pieces,
                int32_t *chunk_first /* cap_chunks + 1 */, int cap_chunks, int32_t *n_chunks);
/* Parity view of the LAST successful plan; any pointer may be NULL.  E: F floats, speech: v3, F bytes of 0 / 1 (cap_frames >=
 * F when either is given), levels: Q_lo, Q_hi, T, regions: a, b pairs in frames, *n_regions: their number (set whenever the
 * pointer is given).  NH_ERR_STATE before any plan; NH_ERR_INVALID, nothing else written, for too little room. */
int nh_vad_view(nh_ctx *ctx, float *E, uint8_t *speech /* v3 */, int64_t cap_frames, float levels[3] /* Q_lo, Q_hi, T */,
                int64_t *regions /* a, b pairs */, int cap_regions, int32_t *n_regions);
/* PCM row row0 + b = the concatenation of chunk b's pieces pcm[piece_starts[j] .. + piece_lens[j]), j = chunk_first[b] ..
 * chunk_first[b + 1] - 1, of a recording in host or device (on_device != 0) memory; then exactly what nh_logmel_device_rows
 * does on those rows with n_samples[b] = the chunk's total: the bits of a log-mel of the concatenation.  No copy back, no
 * synchronisation.  Device PCM: the piece table goes up in one copy and one launch gathers the whole batch (16-byte copies
 * when pcm is 16-byte aligned and no piece boundary inside a row falls off a multiple of 4 samples -- every plan's pieces
 * start at multiples of 160 samples, and only a recording's final piece, last in its row, has a ragged length --, dwords
 * otherwise); host PCM: one copy per piece.  Refused before anything is queued: a chunk_first that does not ascend, a chunk
 * with no piece, a piece length below 1, a negative start, a chunk total above 480 000, and what every nh_logmel*_rows
 * refuses (row range, a chunk below 160 samples beside longer ones). */
int nh_logmel_pieces_rows(nh_ctx *ctx, const float *pcm, int on_device, const int64_t *piece_starts,
                          const int32_t *piece_lens, const int32_t *chunk_first /* batch + 1 */, int batch, int row0);
/* Same, but pcm is a DEVICE pointer (already resident in HBM; no copy). */
int nh_logmel_device(nh_ctx *ctx, const float *pcm_dev, const int32_t *n_samples, int64_t stride, int batch);
/* Encoder forward over the mel of the last nh_logmel call (flush = true semantics: the cross
 * K/V of every decoder layer is recomputed). */
int nh_encode(nh_ctx *ctx);
/* Several encoder batches, ONE decode (r03).  The decode step streams the decoder weights and the tied embedding once per
 * token for all rows of the context, so decoding 64 or 96 clips together reads 15 - 20 % fewer bytes per clip than two or
 * three 32-clip decodes -- while the ENCODER side can still be fed 32 clips at a time as they arrive:
 *   nh_logmel_rows(ctx, pcm, n, stride, 32, 0);  nh_encode_rows(ctx, 0, 32);      first 32 clips -> rows 0 .. 31
 *   nh_logmel_rows(ctx, pcm2, n2, stride, 32, 32); nh_encode_rows(ctx, 32, 32);   next 32 clips  -> rows 32 .. 63
 *   nh_decode_greedy(ctx, ...)                                                          all rows filled so far, in lockstep
 * row0 = 0 starts a new set of rows; row0 > 0 must continue where the previous call ended (no gaps) with clips of the same
 * mel length; every row's arithmetic is what it is in a batch of its own (bit-identical results).  The reference decodes one
 * stream at a time (src/lib.rs:462-464): no counterpart. */
int nh_logmel_rows(nh_ctx *ctx, const float *pcm, const int32_t *n_samples, int64_t stride, int batch, int row0);        /* host PCM */
int nh_logmel_device_rows(nh_ctx *ctx, const float *pcm_dev, const int32_t *n_samples, int64_t stride, int batch, int row0); /* PCM in HBM */
int nh_encode_rows(nh_ctx *ctx, int row0, int batch);
/* Greedy decode of all `batch` sequences.  out_tokens: host i32 [batch][max_target_positions],
 * results: [batch].  max_new_tokens <= 0: reference behaviour (cap at max_target_positions - 1). */
int nh_decode_greedy(nh_ctx *ctx, int32_t *out_tokens, nh_decode_result *results, int max_new_tokens);
/* Decode pool (r03): sequences that join and leave a running decode.  The reference's loop ends per sequence at eot
 * (model.rs:317); decoded as one lockstep batch the short sequences wait for the longest.  Here rows [0, rows) of the context
 * decode, every row at its own position, and the rows above them are encoder staging:
 *   nh_pool_begin(ctx, 64, 0, 0);
 *   nh_logmel_rows(ctx, pcm, n, stride, 32, 64);  nh_encode_rows(ctx, 64, 32);      32 clips -> staging rows 64 .. 95
 *   nh_pool_admit(ctx, 64 + i, free_row, -1);                                      clip i joins the decode at position 0
 *   nh_pool_step(ctx, 16, done);                                                   16 tokens for every busy row
 *   nh_pool_collect(ctx, rows_done, k, tokens, results);                           finished rows out, their slots are free again
 * A row's prompt ([sot, lang?, task], model.rs:285-289), no-speech probe and exit (:293-315), rules, length cap (:367) and
 * result (:373-381) are those of nh_decode_greedy, and so are its bits: the same step kernels run, only the position is read
 * per row.  All clips of a pool must produce the same number of mel frames.  nh_logmel* with row0 = 0 ends the pool.
 * per_clip_language != 0: the prompt carries a language token given per clip at nh_pool_admit (LanguageState::Detect);
 * otherwise nh_tokens.lang decides, as in nh_decode_greedy, and `lang` must be -1.
 * lang == NH_LANG_DETECT (per_clip_language pools with a language table, nh_pool_detect_languages): the row detects its
 * language itself.  Its prompt is [sot, <detected>, task]; slot 1 holds sot until the row's first step has written the
 * language there, and nothing reads the slot before.  Refused: NH_ERR_INVALID in a pool begun without per-clip languages,
 * NH_ERR_STATE while the pool has no table. */
#define NH_LANG_DETECT (-2)
int nh_pool_begin(nh_ctx *ctx, int rows, int max_new_tokens, int per_clip_language);
/* The clip encoded at staging row src_row (>= rows) starts decoding in the free row dst_row (< rows): its cross K/V move
 * (device-to-device, 4 * S * d_model bytes per decoder layer), its decode state starts over.  Asynchronous. */
int nh_pool_admit(nh_ctx *ctx, int src_row, int dst_row, int32_t lang);
/* The same, the clip coming from row src_row of ANOTHER context of the same weight set (nh_create_shared) that ran
 * nh_logmel* + nh_encode / nh_encode_rows on it: one context decodes without ever stalling for an encoder submission while others
 * encode.  Ordered on the device (the copy waits for that encoder, that context's next encoder submission waits for the copy); on
 * the host the caller keeps this call apart from calls ON `enc` that change its rows (nh_logmel*, nh_encode*). */
int nh_pool_admit_from(nh_ctx *ctx, nh_ctx *enc, int src_row, int dst_row, int32_t lang);
/* n_steps decode steps (one token per busy, unfinished row each), then done_out[rows]: 0 running, 1 finished, 2 finished by
 * the no-speech exit, 3 empty.  Returns when the steps have run. */
int nh_pool_step(nh_ctx *ctx, int n_steps, int32_t *done_out);
/* Results of the n finished rows `rows[]`: out_tokens host i32 [n][max_target_positions], results [n]; the rows are free
 * for nh_pool_admit afterwards. */
int nh_pool_collect(nh_ctx *ctx, const int32_t *rows, int n, int32_t *out_tokens, nh_decode_result *results);
/* The clip that last decoded in `row` decodes again from position 0, every generated token SAMPLED at `temperature` (> 0)
 * under the seeded contract of nh_decode_sampled (step = tokens so far, clip, attempt as given).  Valid on a row that
 * nh_pool_collect has handed back and that no nh_pool_admit* has refilled since: its cross K/V and its prompt are still in
 * place, nothing is copied.  The row is busy again afterwards; asynchronous.  This is the retry of decode_with_fallback
 * (model.rs:164-191) for one row: the caller walks TEMPERATURES (norma_amd/pool.py does, fallback=True), an admitted row is
 * always the t = 0 attempt.  The row's bits are those of nh_decode_sampled on a batch that holds the clip at index
 * clip - clip0, whatever the other rows of the pool do meanwhile.  Refused (NH_ERR_INVALID / NH_ERR_STATE, nothing is
 * launched): no pool, row out of range, row busy, row never admitted since nh_pool_begin, temperature <= 0 or not finite. */
int nh_pool_retry(nh_ctx *ctx, int row, float temperature, uint64_t seed, uint32_t clip, uint32_t attempt);
/* A prompt prefix per pool row, every row its own length (nh_pool_prefix): include/norma_hip_pool.h, which includes this header. */
/* Language detection inside the pool.  Model::detect_language (model.rs:194-210) is one decoder forward on [sot] and a softmax
 * over the language-token logits; the first step of a pooled row is that forward (position 0 consumes sot against the clip's
 * cross K/V), and the language token is first consumed one step later.  So a row admitted with lang = NH_LANG_DETECT detects
 * in its first step and writes the token into its own prompt: no extra decoder step, no second context, no host round trip.
 * Token and probabilities are, bit for bit, those of nh_detect_language on a batch that holds the clip (the same device
 * function on the same logits).  A row that the no-speech probe ends in that step has a language too (the reference detects
 * before it decodes); nh_pool_retry keeps the detected token, it is part of the prompt by then.
 * nh_pool_detect_languages sets the pool's table: lang_tokens in `Language::iter()` order, 1 <= n <= 256, as for
 * nh_detect_language.  Call it after nh_pool_begin, which clears the table.  Refused, nothing launched: no pool
 * (NH_ERR_STATE); pool begun without per-clip languages, n out of range, a token id outside the vocabulary (NH_ERR_INVALID);
 * any row busy (NH_ERR_STATE: the captured step graphs carry the table's size, and whether they detect at all).  A new table
 * forgets what was detected under the one before (nh_pool_languages refuses those rows). */
int nh_pool_detect_languages(nh_ctx *ctx, const int32_t *lang_tokens, int n);
/* Detected token (out_lang: host i32 [n_rows]) and probabilities over the table (out_probs: host f32 [n_rows][n] or NULL) of
 * rows[]: rows admitted with NH_LANG_DETECT that have taken at least one nh_pool_step step since and have not been refilled --
 * while they run, and after nh_pool_collect (the lifetime nh_pool_retry relies on).  The token is also tokens[1] of the
 * row's nh_pool_collect result.  Refused: NH_ERR_INVALID for a row outside the pool, NH_ERR_STATE for any other row. */
int nh_pool_languages(nh_ctx *ctx, const int32_t *rows, int n_rows, int32_t *out_lang, float *out_probs);
/* Model::decode at t > 0 (model.rs:340-348): every token is SAMPLED from softmax(q / t), q = the rule-masked
 * probabilities.  The reference draws with rand::WeightedIndex from an entropy-seeded StdRng (model.rs:30), so only its
 * distribution can be reproduced; this build fixes a seeded SAMPLING CONTRACT (the C oracle implements the same, bit for bit):
 *   weights  w_i = sexp((q_i - max q) * (1.0f / t)), sexp = exp from IEEE f32 operations only (Cephes polynomial),
 *            masked entries (-inf) weigh 0; this is softmax(q / t) up to the normalisation WeightedIndex ignores;
 *   uniform  u = (philox4x32-10(key = {seed lo, seed hi}, counter = {step, clip, attempt, 0x6e6f726d})[0] >> 8) * 2^-24,
 *            step = tokens in the sequence so far, clip = clip0 + index in the batch, attempt = index into
 *            TEMPERATURES (decode_with_fallback, model.rs:175);
 *   choice   the first token whose cumulative weight exceeds u * total (WeightedIndex::sample's partition_point),
 *            cumulated in f64 over 1024 chunks of ceil(V / 1024) consecutive tokens, then inside the chunk;
 *   all masked: eot is pushed and the sequence stops (model.rs:343-346).  Log-prob bookkeeping as for t = 0.
 * Under a prefix (nh_set_prompts) `step` is the PHYSICAL token count, the prefix included. */
int nh_decode_sampled(nh_ctx *ctx, int32_t *out_tokens, nh_decode_result *results, int max_new_tokens,
                      float temperature, uint64_t seed, uint32_t clip0, uint32_t attempt);
/* ---- beam search ---------------------------------------------------------------------------------------------
 * Model::decode at t = 0 with K = beam_size hypotheses per clip instead of one, chosen on the device.  Acts on the current
 * lockstep batch of B clips after nh_encode*; out_tokens / results have nh_decode_greedy's shape and hold the best hypothesis
 * of every clip.  At K = 1 it is nh_decode_greedy's search (tokens identical, avg_logprob within 1e-5: the selection kernel
 * sums the softmax in another order than logit_step_kernel).
 *   rows     hypothesis j of clip b lives in context row j * B + b (beam-major).  Beam 0 is the clip's own row; the cross K/V
 *            of rows j >= 1 are device-to-device copies of row b, made once per decode.  Afterwards the context is a lockstep
 *            batch of B clips again, rows 0 .. B-1 hold their cross K/V: a following nh_decode_greedy, nh_decode_sampled,
 *            nh_align or nh_detect_language behaves as after a greedy decode.  nh_align_decoded refuses (kept queries are not
 *            reordered with their hypotheses).
 *   prompt   exactly the greedy decode's, on the B clip rows: no-speech probe and exit, per-clip languages, a prefix from
 *            nh_set_prompts.  Generation starts with beam 0 live at score 0.0, beams 1 .. K-1 dead.
 *   step     per live hypothesis h: q = its rule-masked probabilities (the rules, rule state and f32 softmax of the greedy
 *            step, the row's own n_tokens / last timestamp / last two tokens); its K + 1 best tokens by q (equal q: the
 *            higher id first; q == 0 is no candidate) are candidates with score s_h + log((double)q).  Per clip the <= K (K+1)
 *            candidates are ordered by score descending, then lower parent beam, then higher token id, and walked until K
 *            live children are chosen: an eot candidate becomes a finished hypothesis if the clip holds fewer than K (else
 *            it is dropped); any other becomes the next live hypothesis with the greedy step's bookkeeping -- a forced eot at
 *            the length cap (model.rs:367) or at max_new_tokens adds no log-probability and finishes it under the same
 *            room-for-K rule.  Hypothesis state and self-attention caches move with the hypothesis.
 *   end      a clip is done with K finished hypotheses or no live one.  Its result is the finished hypothesis with the
 *            greatest sum_logprob / n (n counts prompt and eot, model.rs:373, not a prefix), the earliest on ties, through
 *            the greedy decode's trailing-timestamp trim.  A no-speech exit returns what greedy returns.  A clip in which
 *            everything was masked before anything finished returns its best prefix + the last vocabulary index with
 *            avg_logprob -inf (the greedy step's all-masked convention), and ends there.
 * Refused, nothing launched, state untouched.  NH_ERR_INVALID: beam_size outside 1 .. NH_MAX_BEAMS; batch * beam_size >
 * max_batch; NULL outputs.  NH_ERR_STATE: no encoder output; no tokens; a running decode pool; NH_OPT_ABSORBED_XATTN != 0; a
 * prefix set for another batch.  The beam buffers are allocated by the first call; other decodes allocate and launch nothing new. */
#define NH_MAX_BEAMS 8
int nh_decode_beam(nh_ctx *ctx, int beam_size, int32_t *out_tokens, nh_decode_result *results, int max_new_tokens);
/* The finished hypotheses of clip b from the last nh_decode_beam, in finishing order, untrimmed, from sot on (a prefix is not
 * part of them): tokens host i32 [beam_size][max_target_positions] (zero-filled past each end), n_tokens i32 [beam_size],
 * sum_logprob f64 [beam_size], *n_finished how many there are.  beam_size is that of the decode reported on, not an argument:
 * every one of its rows is written, so buffers of NH_MAX_BEAMS rows always suffice.  NH_ERR_STATE without a beam decode to
 * report on. */
int nh_beam_hypotheses(nh_ctx *ctx, int b, int32_t *tokens, int32_t *n_tokens, double *sum_logprob, int32_t *n_finished);
/* ---- repetition guard ----------------------------------------------------------------------------------------
 * Four edits of a row's f32 logits between the step's logits and the selection kernels, from nothing but the tokens the row
 * has generated; one kernel, in every decode mode (greedy, sampled, pool, beam).  With every component off (the default) a
 * step launches nothing for it and every result keeps its bits.
 * For a row that is running (done == 0) and stands at a generation position: PL = the physical prompt length of the step
 * (prefix + [sot, lang?, task]), n = its token count, g = tokens[PL .. n), h = the entries of g with id < eot in order (text
 * only: timestamps and specials are dropped, so a loop whose copies carry different timestamps is a loop), m = len(h).  In
 * this order:
 *   1 repetition_penalty r (r > 0, 1.0f off): for every DISTINCT v in h, once: x = logits[v]; logits[v] = x < 0 ? x * r : x / r
 *     (one IEEE f32 multiply, or one correctly rounded divide).
 *   2 bias (bias != 0): for every entry (v, beta) of the row's list (nh_guard_bias): logits[v] += beta in f32.
 *   3 no_repeat_ngram N (1 .. 16, 0 off): if m >= N - 1, s = h[m-N+1 .. m); for every i in [0, m-N] with h[i .. i+N-1) == s:
 *     logits[h[i+N-1]] = -inf.  N = 1 bans every token of h.
 *   4 loop exit (loop_period Pmax 1 .. 64, 0 off; loop_repeats R 2 .. 16; Pmax * R <= 448): if some p <= Pmax has p * R <= m and
 *     h[m-1-i] == h[m-1-i-p] for all 0 <= i < p * (R - 1), and the row's own rule state is "last token a timestamp, the one
 *     before it no text" (text only) or "last token text" -- the two states in which the rules leave eot unmasked; in the
 *     others (first generated token; a timestamp right after text, which a timestamp must follow) the exit waits for the
 *     next step, h unchanged -- every logit except
 *     eot's becomes -inf and the row's loop-exit flag is set.  The selection kernels then pick eot by themselves with
 *     log-probability log 1 = 0.  The flag is cleared when the row stands at its first generation position (n == PL).
 * Never edited: rows in their prompt phase or at the no-speech probe, finished rows, the pad columns, and anything in
 * nh_detect_language, nh_score, nh_align and the nh_decoder_forward* views.  avg_logprob is the log of the softmax over the
 * EDITED logits. */
typedef struct nh_guard_params { int32_t no_repeat_ngram; float repetition_penalty; int32_t loop_period, loop_repeats; int32_t bias; } nh_guard_params;
/* The context's guard (its own per context, nh_create_shared children included), kept until changed; NULL: off.  Refused, state
 * untouched: NH_ERR_INVALID for a NaN, infinite or non-positive penalty or sizes out of range (with loop_period == 0,
 * loop_repeats must be 0 or 2 .. 16 and is not used), NH_ERR_STATE while any pool row is busy (the captured step graphs carry
 * whether the kernel is in them) and on a model with max_target_positions > 512 (the kernel holds a row's history in LDS).  A change takes effect in the next decode, under
 * NH_OPT_DECODE_GRAPHS too. */
int nh_set_guard(nh_ctx *ctx, const nh_guard_params *p);
#define NH_GUARD_MAX_BIAS 256
/* The bias list of context row `row` (host arrays of n entries; n == 0: clear), kept until replaced or cleared and applied
 * while nh_guard_params.bias != 0; in a pool the caller sets it before nh_pool_admit of that row.  Under nh_decode_beam
 * hypothesis row j * B + b uses clip b's list.  The device table is made by the first use.  Ordered on the context's stream;
 * returns when the caller's buffers are no longer needed.  Refused (NH_ERR_INVALID), lists untouched: a row outside
 * [0, max_batch), n outside 0 .. NH_GUARD_MAX_BIAS, an id twice, an id outside [0, V), a bias NaN or +inf (-inf is allowed). */
int nh_guard_bias(nh_ctx *ctx, int row, const int32_t *tokens, const float *bias, int n);
/* The loop-exit flags (host i32 [n]) of rows[0 .. n) (rows == NULL: rows 0 .. n-1): of the lockstep batch after a greedy or
 * sampled decode; of pool rows while they run and after nh_pool_collect until the row is refilled.  NH_ERR_STATE after
 * nh_decode_beam: the exit ends hypotheses there too, but the flag does not travel with a hypothesis. */
int nh_guard_report(nh_ctx *ctx, const int32_t *rows, int n, int32_t *loop_exit);
/* Parity view: the edit alone, by the kernel of the step, under the context's nh_set_guard parameters.  logits host f32
 * [rows][V]; row r holds tokens[r * stride .. + n_tokens[r]) (prompt_len <= n_tokens[r] <= max_target_positions - 2), is edited
 * only if active == NULL or active[r] != 0, and uses the bias list of context row bias_rows[r] (NULL or < 0: none).  Whether a
 * timestamp has been generated is read off the tokens.  logits_out host f32 [rows][ld], ld = V rounded up to 64: the device
 * rows whole, pad columns (uploaded as all-ones bit patterns) included; loop_exit host i32 [rows].  Overwrites the context's
 * token rows and logits like nh_beam_step. */
int nh_guard_apply(nh_ctx *ctx, int rows, const float *logits, const int32_t *tokens, const int32_t *n_tokens, int64_t stride,
                   int prompt_len, const int32_t *active, const int32_t *bias_rows, float *logits_out, int32_t *loop_exit);
/* Model::detect_language (model.rs:194-210) for every clip of the batch: one decoder step on [sot], softmax over the
 * n language-token logits (lang_tokens in `Language::iter()` order, multilingual.rs:395-398), first maximum.
 * out_lang: host i32 [batch]; out_probs: host f32 [batch][n] or NULL.  The detected tokens become the per-sequence
 * language tokens of the next nh_decode_greedy (LanguageState::set_language_token). */
int nh_detect_language(nh_ctx *ctx, const int32_t *lang_tokens, int n, int32_t *out_lang, float *out_probs);
/* Per-sequence language tokens for the next decode (host i32 [batch]); NULL: back to nh_tokens.lang for all. */
int nh_set_languages(nh_ctx *ctx, const int32_t *langs);
/* ---- decoder prompts ---------------------------------------------------------------------------------------
 * Tokens in front of [sot, lang?, task] for the next nh_decode_greedy / nh_decode_sampled of the current lockstep batch: an
 * initial prompt (vocabulary, style), or the previous window's text when a stream is transcribed in sequence.  ONE prefix
 * length per batch, the contents per clip.
 * tokens: host i32, clip b's prefix at tokens + b * stride, n_prefix entries, taken verbatim (the caller puts
 * <|startofprev|> first if it wants Whisper's convention).  n_prefix == 0 or tokens == NULL: none.
 * What a prefix means: decoder positions 0 .. n_prefix - 1 consume it; [sot, lang?, task] sit at n_prefix ..; the no-speech
 * probe (model.rs:293-305) reads the logits at sot's position, n_prefix; generation starts at n_prefix + P - 1; the rules,
 * the forced first timestamp and max_new_tokens see prompt_len = n_prefix + P; the length cap (model.rs:367) applies to the
 * physical sequence, prefix included.  What comes back is the sequence from sot on: out_tokens and n_tokens exclude the
 * prefix, avg_logprob is divided by that n_tokens (so n_prefix == 0 gives the bits of a decode that never saw a prompt, and a
 * prefix does not dilute the fallback test), no_speech_exit as ever.  nh_detect_language ignores the prefix (the reference
 * detects on [sot] alone).
 * The prefix positions go through the one-pass forward (nh_decoder_forward_onepass's arithmetic; the last decoder block stops
 * once its K/V are cached), or -- under NH_OPT_PROMPT_STEPWISE = 1, for prefixes of fewer than 4 tokens (measured: the one
 * pass does not pay below that), at widths the one pass does not cover (d_model % 128 != 0) and under NH_OPT_ABSORBED_XATTN --
 * through the decode step position by position; the positions from sot on are decode steps
 * either way.
 * Lifetime: bound to the batch, like nh_set_languages: cleared by nh_logmel* with row0 == 0, nh_set_mel, nh_reset and
 * nh_pool_begin; a decode whose batch differs from the one the prefix was set for (rows joined since) is NH_ERR_STATE.
 * After a prompted decode nh_align_decoded refuses (NH_ERR_STATE): the kept queries sit at physical positions.
 * Refused, nothing launched, state unchanged.  NH_ERR_INVALID: batch != the current batch; n_prefix outside
 * 0 .. max_target_positions / 2 - 1; a token id outside the vocabulary; stride < n_prefix.  NH_ERR_STATE: a running pool. */
int nh_set_prompts(nh_ctx *ctx, const int32_t *tokens, int n_prefix, int64_t stride, int batch);
/* Device-resident log-mel -> encoder -> decode without intermediate host syncs (bench path). */
int nh_transcribe_batch(nh_ctx *ctx, const float *pcm_dev, const int32_t *n_samples, int64_t stride,
                        int batch, int32_t *out_tokens, nh_decode_result *results, int max_new_tokens);
int nh_reset(nh_ctx *ctx);
int nh_synchronize(nh_ctx *ctx);

/* ---- fine-grained views for layer-level parity tests ------------------------------------------- */
/* mel of clip b in candle layout: f32 [num_mel_bins][3000] */
int nh_get_mel(nh_ctx *ctx, int b, float *out);
/* Upload a mel directly (f32 [batch][num_mel_bins][3000]) instead of nh_logmel. */
int nh_set_mel(nh_ctx *ctx, const float *mel, int batch);
/* encoder output of clip b: f32 [1500][d_model] */
int nh_encoder_output(nh_ctx *ctx, int b, float *out);
/* TextDecoder::forward for every clip over a teacher-forced prefix: tokens i32 [batch][T] ->
 * hidden f32 [batch][T][d_model] (after the final LayerNorm). */
int nh_decoder_forward(nh_ctx *ctx, const int32_t *tokens, int T, float *hidden_out);
/* nh_decoder_forward's contract (same arguments, same state afterwards: self K/V of positions 0 .. T-1 and the device-side
 * tokens overwritten), computed in one pass over the T positions: rows (clip, position) through the MFMA GEMM, a causal
 * self-attention and a cross-attention kernel over all positions of a clip (DESIGN.md 13 has the roundings, which are not
 * the decode step's: the two agree within tolerances, not bit for bit).  A clip's rows are bit-identical whatever the batch.
 * NH_ERR_STATE also for d_model % 128 != 0 and under NH_OPT_ABSORBED_XATTN. */
int nh_decoder_forward_onepass(nh_ctx *ctx, const int32_t *tokens, int T, float *hidden_out);
/* TextDecoder::final_linear on host-provided rows: x f32 [rows][d_model] -> logits f32 [rows][V] */
int nh_final_linear(nh_ctx *ctx, const float *x, int rows, float *logits_out);
/* The logit rules on device: probs f32 [V] (already soft-maxed), tokens so far, last timestamp
 * (< 0: first generated token).  Returns the masked probabilities (model.rs:333-338). */
int nh_apply_rules(nh_ctx *ctx, const float *probs, const int32_t *tokens, int n_tokens,
                   int last_timestamp, float *masked_out, int32_t *argmax_out);

/* The sampler alone: rules + one draw on a soft-maxed probability vector (token_out = -1: everything masked). */
int nh_sample_rules(nh_ctx *ctx, const float *probs, const int32_t *tokens, int n_tokens, int last_timestamp,
                    float temperature, uint64_t seed, uint32_t clip, uint32_t attempt, int32_t *token_out);

/* One beam step on host-provided logits and hypothesis state: exactly the selection and merge kernels of nh_decode_beam (the
 * hypothesis state moves in the merge).  K = beam_size, B = batch, rows beam-major (j * B + b), K * B <= max_batch.
 * logits f32 [K*B][V] (uploaded with NaN in the device buffer's pad columns).  In and out, per row: tokens i32
 * [K*B][max_target_positions], n_tokens, have_last (0 | 1), last_ts, live (0 | 1; a live row holds 1 .. max_target_positions - 2
 * tokens), score f64.  max_new_tokens and prompt_len as in a decode.  Out: parent i32 [K*B] (the row each live row's
 * hypothesis came from, -1 for a dead row; a row that stays dead keeps its state), n_finished i32 [B] (in: finished
 * hypotheses the clip already holds; out: after the step), and the records of the newly finished in slots n_finished_in ..
 * n_finished_out - 1 of fin_tokens i32 [B][K][max_target_positions], fin_n i32 [B][K], fin_score f64 [B][K]. */
int nh_beam_step(nh_ctx *ctx, int beam_size, int batch, const float *logits, int32_t *tokens, int32_t *n_tokens,
                 int32_t *have_last, int32_t *last_ts, int32_t *live, double *score, int max_new_tokens, int prompt_len,
                 int32_t *parent, int32_t *n_finished, int32_t *fin_tokens, int32_t *fin_n, double *fin_score);
/* The cache reorder of a beam step alone: `cache` (host fp16 bits [K*B][heads][max_target_positions][64]) is uploaded into
 * the self-attention K (which = 0) or V (1) cache of decoder layer `layer`, row r takes positions 0 .. n_pos-1 of row
 * parent[r] in every layer's caches (parent[r] < 0, == r or outside the clip's rows: the row stays), and that cache comes back. */
int nh_beam_reorder(nh_ctx *ctx, int beam_size, int batch, const int32_t *parent, int n_pos, int layer, int which, uint16_t *cache);

/* ---- token-level timestamps ------------------------------------------------------------------------ */
/* The decoder yields one timestamp token per segment boundary; nh_align gives every token a time, the way Whisper runtimes
 * do: cross-attention weights of a few "alignment heads" over a teacher-forced pass, normalised, median-filtered, averaged,
 * and a dynamic-time-warping (DTW) path through the result.  All of it runs on the device (DESIGN.md 9 has the stages and
 * their exact arithmetic).  It aligns the sequence as decoded -- timestamp tokens included --: what the caller holds. */
#define NH_ALIGN_MAX_HEADS 32
typedef struct nh_align_head { int32_t layer, head; } nh_align_head;   /* decoder layer, head in that layer */
/* For every clip of the current lockstep batch (after nh_encode / nh_encode_rows; a decode may or may not have run):
 * tokens      host i32 [batch][max_target_positions], the sequences as nh_decode_* returned them (prompt .. eot)
 * n_tokens    host i32 [batch], prompt_len < n_tokens[b] <= max_target_positions
 * prompt_len  tokens [0, prompt_len) are the prompt ([sot, lang?, task]); they get no time.  >= 1
 * n_keys      host i32 [batch] or NULL (= S): encoder frames that hold audio, 1 <= n_keys[b] <= S
 * out_first / out_last  host i32 [batch][max_target_positions]: first and last encoder frame (20 ms each) on the
 *                       DTW path of token i; -1 for i < prompt_len and i >= n_tokens[b]
 * Stages, for clip b with n = n_tokens[b], nk = n_keys[b], P = prompt_len:
 *   1 positions p = 0 .. n - 2 consume tokens[b][p] through the decoder step of nh_decoder_forward (no logits, no host
 *     round trip between positions)
 *   2 W[a][p][s] = softmax over s < nk of q . k_s / 8 for head a = (l, h): q the fp16 cross-attention query of layer l at
 *     position p, k_s the fp16 cross K cache row; f32 accumulation, f32 result.  Row p belongs to token p + 1.
 *   3 per (a, s): z = (W - mean) / std over the n - 1 rows (population std); std == 0 gives z = 0
 *   4 median of 7 along s inside [0, nk), reflect padding without repeating the edge; nk <= 3 is left unfiltered
 *   5 M[r][s] = mean over the heads, in list order, of the filtered z at row P - 1 + r, r = 0 .. n - P - 1 (token P + r)
 *   6 DTW on x = -M in f32: cost[0][0] = 0, the other border cells +inf, cost[i][j] = x[i-1][j-1] + c with c the least of
 *     c0 = cost[i-1][j-1], c1 = cost[i-1][j], c2 = cost[i][j-1]: c0 (trace 0) if c0 < c1 and c0 < c2, else c1 (trace 1) if
 *     c1 < c0 and c1 < c2, else c2 (trace 2); backtrace from (R, nk): trace 0 i--, j--; 1 i--; 2 j--.  out_first[P + r]
 *     and out_last[P + r] are the least and greatest j - 1 visited with i - 1 == r.
 * Refused, nothing launched (NH_ERR_STATE): no encoder output, a decode pool, NH_OPT_ABSORBED_XATTN != 0 (no K cache);
 * (NH_ERR_INVALID): n_heads outside 1 .. NH_ALIGN_MAX_HEADS, a layer or head out of range (or at or beyond
 * NH_OPT_DECODER_LAYER_LIMIT), a token id outside the vocabulary, n_tokens, prompt_len or n_keys out of range.
 * Afterwards the context is in the state nh_decoder_forward leaves: self K/V and the device-side tokens are overwritten,
 * cross K/V and the encoder output untouched.  A clip's outputs are bit-identical whatever the batch around it. */
int nh_align(nh_ctx *ctx, const int32_t *tokens, const int32_t *n_tokens, int prompt_len,
             const nh_align_head *heads, int n_heads, const int32_t *n_keys,
             int32_t *out_first, int32_t *out_last);
/* Alignment from the decode itself.  The only thing nh_align's teacher-forced pass produces that the decode did not already
 * hold is the 64 fp16 query values per alignment head and position; a context told the heads beforehand keeps them while it
 * decodes, and stages 2 - 6 then run on what is kept: no second decoder pass, and the rows of a decode pool can be aligned.
 *
 * nh_align_capture: the alignment heads whose cross-attention queries every following decode of this context keeps
 * (nh_decode_greedy, nh_decode_sampled, every step of a pool row): one 64-thread-per-(row, head) launch per decoder layer
 * that holds a head, writing the running rows at their own positions.  n_heads == 0: off (the default; the decode step is
 * launched as without this function).  Tokens, log-probs and no-speech probabilities are the same bits either way.
 * Refused, nothing changed: n_heads outside 0 .. NH_ALIGN_MAX_HEADS, a layer or head out of range or at or beyond
 * NH_OPT_DECODER_LAYER_LIMIT (NH_ERR_INVALID); NH_OPT_ABSORBED_XATTN != 0, any pool row busy -- the captured step graphs
 * carry the list -- (NH_ERR_STATE).  A new list forgets what was kept under the one before. */
int nh_align_capture(nh_ctx *ctx, const nh_align_head *heads, int n_heads);
/* Token times of sequences this context has just decoded, from the kept queries: stages 2 - 6 of nh_align, no decoder pass.
 * rows == NULL: the n == batch clips of the last lockstep decode.  rows != NULL: n pool rows that nh_pool_collect has
 * handed back and that no admit / retry has touched since (the lifetime nh_pool_retry and nh_pool_languages rely on); a
 * retried row is aligned on its retry, once that has been collected.
 * The sequence aligned is the one the decode / collect returned (n_tokens after the trailing-timestamp trim; the context
 * remembers it -- the trim only drops trailing timestamp tokens and moves eot up, so query rows 0 .. n - 2 consumed exactly
 * the returned tokens 0 .. n - 2), prompt_len is the decode's own.  n_keys: host i32 [n] or NULL (= S).
 * out_first / out_last: host i32 [n][max_target_positions], as for nh_align, and equal to nh_align's on the returned tokens.
 * A sequence ended by the no-speech exit has nothing to align: all -1.
 * A lockstep context's sequences stay valid until nh_logmel* / nh_encode* / another decode / nh_align / nh_decoder_forward /
 * nh_detect_language; a pool row's until an admit or retry of that row.
 * Refused, nothing launched, outputs untouched.  NH_ERR_STATE: no heads set; no valid captured sequence (lockstep); a pool
 * row that is busy, was never admitted, was decoded before the current head list was set, or was refilled or retried and not
 * collected since.  NH_ERR_INVALID: a row outside the pool; rows == NULL on a pool context, or rows on a lockstep one; n
 * that does not match the batch (pool: outside [1, rows of the pool]); n_keys outside [1, S]. */
int nh_align_decoded(nh_ctx *ctx, const int32_t *rows, int n, const int32_t *n_keys, int32_t *out_first, int32_t *out_last);
/* parity views of the LAST alignment (nh_align or nh_align_decoded; b = the index within that call), valid only under
 * NH_OPT_ALIGN_KEEP = 1 (otherwise NH_ERR_STATE) */
int nh_align_weights(nh_ctx *ctx, int b, int a, float *out);   /* f32 [n_tokens[b]-1][n_keys[b]] probabilities of heads[a] */
int nh_align_matrix(nh_ctx *ctx, int b, float *out);           /* f32 [n_tokens[b]-prompt_len][n_keys[b]] the DTW input */
/* the DTW alone on a host matrix f32 [R][nk] (cost = -matrix): parity view, R <= max_target_positions, nk <= S
 * (S = max_source_positions when nothing is encoded yet); out_first / out_last host i32 [R] */
int nh_align_path(nh_ctx *ctx, const float *matrix, int R, int nk, int32_t *out_first, int32_t *out_last);

/* ---- transcript scoring ---------------------------------------------------------------------------- */
/* How probable is every token of a GIVEN transcript under the model: what a word confidence, the score of a corrected
 * transcript, re-ranking another model's hypotheses and a fallback test on the weakest span are built from.  All positions of
 * all clips go through the decoder in one pass (nh_decoder_forward_onepass's arithmetic) and through one projection onto the
 * vocabulary that is reduced on the fly: no logit reaches memory.
 * For every clip of the current lockstep batch (after nh_encode / nh_encode_rows; a decode may or may not have run):
 * tokens       host i32 [batch][max_target_positions]: the sequences as a decode returned them, or any others
 * n_tokens     host i32 [batch], prompt_len < n_tokens[b] <= max_target_positions
 * prompt_len   tokens [0, prompt_len) are given, not scored.  >= 1.  A prefix that stood in front of sot during the decode
 *              (nh_set_prompts) is scored by passing it as part of `tokens`, with prompt_len = n_prefix + P; nh_score itself
 *              ignores nh_set_prompts
 * out_logprob  host f32 [batch][max_target_positions]: for prompt_len <= i < n_tokens[b], entry i is the natural log of the
 *              probability of tokens[b][i] under the PLAIN softmax (no logit rules) over all V logits of position i - 1 -- the
 *              quantity a decode adds to its sum of log-probabilities for the token it picks (its expf(l - m) / se is not
 *              renormalised by the rules).  Every other entry is written as 0.0f
 * Arithmetic, for clip b with n = n_tokens[b]:
 *   1 positions 0 .. max_b(n) - 2 of all clips go through the one-pass forward up to the final LayerNorm's fp16 rows xn.
 *     Positions past a clip's own n - 2 are padding: the self-attention is causal, so they reach no scored position, and
 *     what the caller holds in tokens[b][n:] is never looked at
 *   2 l[v] = sum_k xn[k] E[v][k]: fp16 operands, f32 accumulation, the k-steps added in ascending order into one
 *     accumulator (the statement the GEMMs make: a logit does not depend on the number of rows)
 *   3 m = max_v l and se = sum_v expf(l[v] - m) in f32, in an order fixed by v alone
 *   4 out = (float)((double)(l[t] - m) - log((double)se)), which stays finite where expf(l[t] - m) underflows
 * A clip's outputs are bit-identical whatever the batch around it and whatever sits in tokens[b][n_tokens[b]:].
 * Afterwards the context is in the state nh_decoder_forward_onepass leaves: self K/V and the device-side tokens are
 * overwritten, cross K/V and the encoder output untouched; nh_align_decoded refuses until the next decode.
 * Refused, nothing launched, outputs untouched.  NH_ERR_STATE: no encoder output, a decode pool, d_model % 128 != 0,
 * NH_OPT_ABSORBED_XATTN != 0.  NH_ERR_INVALID: NULL arguments, prompt_len < 1, n_tokens[b] outside
 * (prompt_len, max_target_positions], a token id outside the vocabulary among the first n_tokens[b].
 * Its buffers are one allocation made by the first call and freed with the context: a context that never scores allocates
 * and launches nothing for it. */
int nh_score(nh_ctx *ctx, const int32_t *tokens, const int32_t *n_tokens, int prompt_len, float *out_logprob);

/* ---- instrumentation --------------------------------------------------------------------------- */
/* Milliseconds (HIP events on the context's stream) spent in the phases of the last
 * nh_transcribe_batch / nh_logmel+nh_encode+nh_decode_greedy sequence. */
typedef struct nh_timings {
    float mel_ms, encoder_ms, cross_kv_ms, decode_ms;
    int32_t decode_steps;
    float gemm_ms;      /* summed duration of the dominant encoder GEMM kernel launches */
    int32_t gemm_launches;
    double gemm_flops;  /* algorithmic FLOPs of those launches */
} nh_timings;
int nh_get_timings(nh_ctx *ctx, nh_timings *out);
/* 1: bracket every encoder GEMM launch with a pair of HIP event records on its stream (no synchronisation; bench roofline). */
int nh_set_profile_gemm(nh_ctx *ctx, int enable);

/* A/B switches for the bit-exactness screens in tests/ (the defaults are the product configuration; options 0 and 1 change
 * only how the decode step is launched, never its results). */
#define NH_OPT_DECODE_GRAPHS 0          /* 1 (default): replay the captured decode step; 0: launch every kernel eagerly */
#define NH_OPT_FUSE_DECODE_LAYERNORM 1  /* 1 (default): LayerNorm inside the consuming GEMV; 0: stand-alone LayerNorm kernel */
/* Parity view, the one option that DOES change results: n > 0 runs only the first n decoder blocks of TextDecoder::forward
 * (model.rs:466-476) before the final LayerNorm, so a test can compare the hidden state against an oracle built with n decoder
 * layers and see how the fp16 error grows with depth; 0 (default) = all of them. */
#define NH_OPT_DECODER_LAYER_LIMIT 2
/* Cross-attention computed on the encoder output itself (u = Wk^T q, z = p^T xa, o = Wv z + bv), lockstep
 * decodes only.  1: slow prototype kernels that place the fp16 roundings where the one-pass kernel does (the numerics experiment);
 * 2: the one-pass kernels (xa streamed once per decoder layer; d_model 512 / 768 / 1024 / 1280, other widths fall back to 1).
 * 0 (default): K and V as the reference computes them. */
#define NH_OPT_ABSORBED_XATTN 3
/* The workspace of nh_align / nh_align_decoded.
 * 1: keep every clip's weights and matrix for the views nh_align_weights / nh_align_matrix (the whole
 * batch is held: NH_ERR_NOMEM when that does not fit); 0 (default): clips are processed in groups that keep the workspace at
 * or under 256 MiB, and the views refuse. */
#define NH_OPT_ALIGN_KEEP 4
/* Decoder prompts.  1: the prefix goes through the decode step position by position (the A/B screen); 0 (default): one pass */
#define NH_OPT_PROMPT_STEPWISE 5
int nh_set_option(nh_ctx *ctx, int option, int value);

#ifdef __cplusplus
}
#endif
#endif /* NORMA_HIP_H */
