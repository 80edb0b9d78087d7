/*
 * norma_host.h -- C shim over the C++ host layer (norma_amd/csrc/norma_host.hpp), which mirrors norma's
 * Whisper plugin interface (ModelDefinition / Model::transcribe, src/models/mod.rs:13-34,
 * src/models/whisper/model.rs:55-191) on top of the kernel-level C ABI of norma_hip.h.
 * It exists so that the host layer can be driven from tests (ctypes) exactly like the Rust crate would
 * drive it; a Rust integration binds norma_hip.h directly and keeps this policy in Rust.
 */
#ifndef NORMA_HOST_H
#define NORMA_HOST_H
#include <stddef.h>
#include <stdint.h>

#include "norma_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SelectedDevice kinds (src/models/mod.rs:36-43 + the new Rocm variant) */
#define NM_DEVICE_CPU 0
#define NM_DEVICE_CUDA 1
#define NM_DEVICE_METAL 2
#define NM_DEVICE_ROCM 3

/* monolingual::ModelType (monolingual.rs:32-46): the fp16 checkpoints first, then the quantised ones, then multilingual::ModelType */
#define NM_MODEL_TINY_EN 0
#define NM_MODEL_BASE_EN 1
#define NM_MODEL_SMALL_EN 2
#define NM_MODEL_MEDIUM_EN 3
#define NM_MODEL_DISTIL_MEDIUM_EN 4
#define NM_MODEL_DISTIL_LARGE_EN_V2 5
#define NM_MODEL_DISTIL_LARGE_EN_V3 6
/* the q8_0 GGUF checkpoints of lmz/candle-whisper (monolingual QuantizedTinyEn, multilingual QuantizedTiny): loaded from
 * config-{ext}.json / tokenizer-{ext}.json / model-{ext}-q80.gguf, ext = "tiny-en" / "tiny"; weights are dequantised at load */
#define NM_MODEL_QUANTIZED_TINY_EN 7
#define NM_MODEL_QUANTIZED_TINY 8
/* multilingual::ModelType (multilingual.rs:47-57): load with language = NULL / "" (detected) or a fixed "<|xx|>" (MultiAsMono) */
#define NM_MODEL_TINY 9
#define NM_MODEL_BASE 10
#define NM_MODEL_SMALL 11
#define NM_MODEL_MEDIUM 12
#define NM_MODEL_LARGE 13
#define NM_MODEL_LARGE_V2 14
#define NM_MODEL_LARGE_V3 15

typedef struct nm_definition nm_definition; /* whisper::monolingual::Definition */
typedef struct nm_model nm_model;           /* whisper::Model */
typedef struct nm_tensors nm_tensors;       /* the tensors a checkpoint provides (caller-owned memory) */

nm_definition *nm_definition_new(int model_type, int device_kind, size_t ordinal); /* Definition::new */
void nm_definition_free(nm_definition *d);
int nm_definition_set_responsiveness(nm_definition *d, uint64_t period_ms); /* 0 ok, 1 = Error::Respnsivness */
size_t nm_definition_max_chunk_len(const nm_definition *d);                 /* common_params().max_chunk_len() */
size_t nm_definition_data_buffer_size(const nm_definition *d);
void nm_definition_set_data_buffer_size(nm_definition *d, size_t n);

nm_tensors *nm_tensors_new(void);
void nm_tensors_add(nm_tensors *t, const char *name, int dtype, const int64_t *shape, int ndim, const void *data);
void nm_tensors_free(nm_tensors *t);

/* ModelDefinition::blocking_try_to_model; NULL on failure with the message in err */
nm_model *nm_definition_blocking_try_to_model(const nm_definition *d, const nh_config *cfg, const nh_tokens *tk,
                                              const int32_t *suppress, int n_suppress, const float *mel_filters,
                                              int n_mel, const nm_tensors *tensors, char *err, int err_len);
/* The same from a local directory with config.json, tokenizer.json, model.safetensors (monolingual.rs:323-373 after
 * its hf-hub download); installs the byte-level BPE detokeniser so transcribe also produces text (model.rs:147). */
nm_model *nm_definition_blocking_try_to_model_from_dir(const nm_definition *d, const char *dir, const float *mel_filters,
                                                       int n_mel, const char *language, int translate, char *err,
                                                       int err_len);
/* multilingual models: LanguageState::Detect (model.rs:393-440).  lang_tokens in Language::iter() order
 * (languages.rs:7-107); the language is inferred on the first slice and cleared on final_chunk.
 * (nm_definition_blocking_try_to_model_from_dir enables it itself when `language` is NULL or "".) */
void nm_model_enable_language_detection(nm_model *m, const int32_t *lang_tokens, int n);
/* GGUF reader check (no GPU needed): writes one line per tensor "name type d0xd1.. sum_of_dequantised_values\n" into buf,
 * returns the number of tensors or -1 (message in buf). */
int nm_gguf_list(const char *path, char *buf, int cap);
/* i-th language code in Language::iter() order (languages.rs:7-107, used at model.rs:204 and multilingual.rs:395-398);
 * NULL past the 99th.  The language token is "<|code|>". */
const char *nm_language_code(int i);
/* The asset readers alone (no GPU): tokenizer.json (Tokenizer::from_file, token_to_id, decode -- monolingual.rs:349,
 * mod.rs:86-90, model.rs:147) and safetensors (VarBuilder::from_mmaped_safetensors, monolingual.rs:237-239). */
typedef struct nm_tokenizer nm_tokenizer;
nm_tokenizer *nm_tokenizer_open(const char *path, char *err, int err_len);
void nm_tokenizer_free(nm_tokenizer *t);
int nm_tokenizer_token_to_id(const nm_tokenizer *t, const char *token); /* -1 = whisper::Error::TokenId */
/* writes the UTF-8 text (NUL-terminated, truncated to cap - 1) and returns its full length in bytes */
int nm_tokenizer_decode(const nm_tokenizer *t, const uint32_t *ids, size_t n, int skip_special_tokens, char *buf, int cap);
/* one line per tensor "name dtype d0xd1.. sum sum_abs\n" (f64 sums of the values widened to f32); returns the number of
 * tensors or -1 with the message in buf.  F32, F16 and BF16 are read. */
int nm_safetensors_list(const char *path, char *buf, int cap);
int nm_model_language_token(const nm_model *m); /* current language token, -1 = not detected yet */
/* decode_with_fallback's sampled attempts at t = 0.2 .. 1.0 (model.rs:175-188).  ON by default with an entropy seed, as in the
 * reference (StdRng::from_entropy): a slice whose every attempt has avg_logprob < -1 is dropped.  enable = 1 with a seed
 * fixes the draws (seeded sampling contract of norma_hip.h; the reference's draws cannot be reproduced, only their
 * distribution); enable = 0 returns the t = 0 result and nm_model_last_result reports needed_fallback. */
void nm_model_set_temperature_fallback(nm_model *m, int enable, uint64_t seed);
/* Beam search for the t = 0 attempt of decode_with_fallback (nh_decode_beam, norma_hip.h): k hypotheses, 1 <= k <= 8.  k = 1
 * (the default) is the greedy decode of the reference and changes nothing; the sampled attempts are never beams.  A slice
 * decoded by the beam carries no token times.  Returns 0, or 1 (k out of range, no device memory for a context of k rows). */
int nm_model_set_beam_size(nm_model *m, int k);
/* text of the last nm_model_transcribe call (empty without a tokenizer); returns its length */
int nm_model_last_text(const nm_model *m, char *buf, int cap);
void nm_model_free(nm_model *m);

/* Model::transcribe(&mut data, final_chunk).  out_tokens receives the token ids of every emitted segment
 * (what the reference hands to tokenizer.decode, model.rs:147), segments separated by -1; *n_out = ints
 * written; *buffered = samples the model keeps for the next call.  Returns 0, or 1 on a backend error. */
int nm_model_transcribe(nm_model *m, const float *data, size_t n, int final_chunk, int32_t *out_tokens, int cap,
                        int *n_out, size_t *buffered, char *err, int err_len);
/* ---- audio ingest (src/lib.rs:172-216: the capture callback's channel mixdown and resampler; nh_resample of norma_hip.h) --- */
/* The format of the frames nm_model_transcribe_frames takes; the default is 16 000 Hz mono, what nm_model_transcribe takes.
 * Set on a definition it applies to the models made from it afterwards. */
void nm_definition_set_input_format(nm_definition *d, uint32_t src_hz, int channels);
void nm_model_set_input_format(nm_model *m, uint32_t src_hz, int channels);
/* Model::transcribe on native frames: n frames of `channels` interleaved samples of type sample_dtype (NH_SAMPLE_*) at the
 * model's input rate go through the model's streaming resampler; the 16 kHz samples that became computable are appended to
 * the buffer nm_model_transcribe uses and its loop runs unchanged.  final_chunk also flushes and resets the resampler.
 * Outputs as for nm_model_transcribe. */
int nm_model_transcribe_frames(nm_model *m, const void *frames, int sample_dtype, size_t n, int final_chunk, int32_t *out_tokens,
                               int cap, int *n_out, size_t *buffered, char *err, int err_len);
/* The streaming resampler's bookkeeping as a pure function (no GPU).  A stream has `received` frames and `emitted` outputs so
 * far and keeps the frames from first_kept on.  With L, M, T of nh_resample_table and Wc = T / 2, output n is ready when
 * floor(n M / L) + Wc <= received - 1; on the final push everything below ceil(received L / M) is (zeros beyond the end).
 * *n_ready: outputs emitted .. emitted + n_ready - 1 are ready; *f0, *num0: first frame of the window and start position to
 * give nh_resample for output `emitted`: f0 = max(first_kept, floor(emitted M / L) - Wc + 1), num0 = emitted M - f0 L;
 * *drop_before: first frame still needed once they are out (= received on the final push).  Returns 0, or 1 for a rate
 * nh_resample refuses or inconsistent counts. */
int nm_resample_plan(int src_hz, int64_t received, int64_t emitted, int64_t first_kept, int final_push, int64_t *n_ready,
                     int64_t *f0, int64_t *num0, int64_t *drop_before);
/* norma::Resampler: the streaming form of nh_resample on the model's context.  push returns how many 16 kHz samples became
 * computable (-1: refused, message in err; the stream is reset), read copies them out (returns how many there are); the
 * total over a stream equals nh_resample on the whole of it, however it was cut.  final_push flushes and resets. */
typedef struct nm_resampler nm_resampler;
nm_resampler *nm_resampler_new(nm_model *m, int src_hz, int channels, int sample_dtype);
void nm_resampler_free(nm_resampler *r);
int64_t nm_resampler_push(nm_resampler *r, const void *frames, size_t n, int final_push, char *err, int err_len);
int64_t nm_resampler_read(const nm_resampler *r, float *out, int64_t cap);
void nm_resampler_state(const nm_resampler *r, int64_t *received, int64_t *emitted, int64_t *kept);
/* Token-level timestamps (nh_align of norma_hip.h).  heads: n [layer, head] pairs, n = 0 switches them off (the default).
 * When on, every slice's accepted decode is aligned over the frames that hold audio.  Returns 0, or 1 when n is out of range. */
int nm_model_set_alignment_heads(nm_model *m, const int32_t *layer_head_pairs, int n);
/* alignment_heads of the checkpoint's generation_config.json (nm_definition_blocking_try_to_model_from_dir): writes up to cap
 * pairs, returns how many the checkpoint lists (0 without that file).  Not enabled by itself. */
int nm_model_checkpoint_alignment_heads(const nm_model *m, int32_t *layer_head_pairs, int cap);
/* (start, end) in seconds from the start of its slice for every token the last nm_model_transcribe wrote to out_tokens, in that
 * order (the -1 separators have no entry).  Writes up to cap pairs, returns how many there are: 0 with alignment off. */
int nm_model_last_token_times(const nm_model *m, float *start, float *end, int cap);
/* Decoder prompts (nh_set_prompts of norma_hip.h; no counterpart in the reference).  set_prompt_tokens: an initial prompt --
 * n token ids (the tokenizer here only decodes), n = 0: none -- for every slice.  set_condition_on_previous: inside
 * nm_model_transcribe the text tokens of the emitted segments are kept as history, and a slice decodes under
 * [<|startofprev|>] + (initial prompt + history) cut to its last max_target_positions / 2 - 2 ids, the same for every
 * temperature of decode_with_fallback; the history is dropped on final_chunk and after a slice accepted at a temperature
 * above 0.5.  Both off (the default): the calls and the bits of a model without them.  <|startofprev|> is looked up by
 * nm_definition_blocking_try_to_model_from_dir (token_to_id); a model made from tensors is told it with
 * nm_model_set_startofprev_token.  Slices decoded under a prefix get no token times (nm_model_set_alignment_heads).
 * nm_model_prompt_prefix: the prefix the NEXT slice would decode under (up to cap ids are written; returns its length). */
void nm_model_set_prompt_tokens(nm_model *m, const int32_t *ids, int n);
void nm_model_set_condition_on_previous(nm_model *m, int enable);
void nm_model_set_startofprev_token(nm_model *m, int32_t id);
int nm_model_prompt_prefix(const nm_model *m, int32_t *ids, int cap);
/* The repetition guard of every decode of the model (nh_set_guard of norma_hip.h; no counterpart in the reference):
 * no-repeat n-gram, repetition penalty, loop exit (period, repeats) and whether the token bias applies.  (0, 1.0, 0, 0, 0), the
 * default, is off: the calls and the bits of a model without it.  set_token_bias: n (id, bias) pairs for the model's single
 * row, finite or -inf, applied while the guard's bias != 0; n = 0 clears.  Both return 0, or 1 when nh_set_guard /
 * nh_guard_bias refuse (nothing changes).  last_loop_exit: 1 when the last decoded slice left by the loop exit (never under a
 * beam: the flag does not travel with a hypothesis). */
int nm_model_set_repetition_guard(nm_model *m, int no_repeat_ngram, float repetition_penalty, int loop_period, int loop_repeats, int bias);
int nm_model_set_token_bias(nm_model *m, const int32_t *ids, const float *bias, int n);
int nm_model_last_loop_exit(const nm_model *m);
/* DecodingResult of the last decoded slice + whether the reference would have entered its sampled fallback */
void nm_model_last_result(const nm_model *m, double *avg_logprob, double *no_speech_prob, int *needed_fallback,
                          int *n_tokens);

#ifdef __cplusplus
}
#endif
#endif
