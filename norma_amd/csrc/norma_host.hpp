// norma_host.hpp -- C++ host layer above the C ABI (include/norma_hip.h) that mirrors norma's plugin
// interface for the Whisper path: same names, argument meaning and error behaviour as the Rust items
// it stands in for (the reference is compiled Rust; no Rust toolchain exists in this environment, so
// the host side is written in C++; the Rust binding itself is in INTEGRATION.md).
//
//   reference (MikeIvanichev/norma @ 2024_10_08)                 here
//   ------------------------------------------------------------ ---------------------------------
//   models::SelectedDevice              src/models/mod.rs:36-55   norma::SelectedDevice (+ Rocm(ord))
//   models::CommonModelParams           src/models/mod.rs:58-117  norma::CommonModelParams
//   models::ModelDefinition / Model     src/models/mod.rs:13-34   norma::whisper::Definition / Model
//   whisper::Error                      whisper/mod.rs:64-84      norma::whisper::Error
//   whisper::monolingual::ModelType     monolingual.rs:32-111     norma::whisper::ModelType
//   whisper::Model::transcribe          model.rs:55-159           Model::transcribe
//   Model::decode_with_fallback (t=0)   model.rs:164-191          Model::decode_with_fallback
//   SliceExt::inclusive_boxed_by        src/utils.rs:22-76        norma::inclusive_boxed_by
//   capture callback: mixdown + Sinc    src/lib.rs:172-216        norma::Resampler, Model::transcribe_frames
//
// Text decoding needs a tokenizer (`tokenizers` crate in the reference, model.rs:147); none is
// available offline, so transcribe() returns the token ids of each segment and, when a detokenizer
// callback is installed, the text as well.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <memory>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../../include/norma_hip.h"
#include "norma_assets.hpp"

namespace norma {

// ---- src/utils.rs:22-76 ----------------------------------------------------------------------------
// Consecutive sub-slices that start AND end (inclusive) on an element matching pred.
template <typename T, typename P>
std::vector<std::pair<size_t, size_t>> inclusive_boxed_by(const std::vector<T> &v, P pred) {
    std::vector<std::pair<size_t, size_t>> out;  // [begin, end)
    size_t base = 0;
    while (base < v.size()) {
        size_t s = base;
        while (s < v.size() && !pred(v[s])) s++;
        if (s >= v.size()) break;
        size_t e = s + 1;
        while (e < v.size() && !pred(v[e])) e++;
        if (e >= v.size()) break;
        out.emplace_back(s, e + 1);
        base = e + 1;
    }
    return out;
}

// ---- src/models/mod.rs:36-55 ------------------------------------------------------------------------
struct SelectedDevice {
    enum Kind { Cpu, Cuda, Metal, Rocm } kind = Cpu;  // Default = Cpu
    size_t ordinal = 0;
    static SelectedDevice cpu() { return {}; }
    static SelectedDevice cuda(size_t n) { return {Cuda, n}; }
    static SelectedDevice metal() { return {Metal, 0}; }
    static SelectedDevice rocm(size_t n) { return {Rocm, n}; }  // NEW: MI355X ordinal, selects the HIP backend
};

// ---- src/models/mod.rs:58-117 -----------------------------------------------------------------------
class CommonModelParams {
    static constexpr size_t MIN_CHUNK_LEN = 100, MIN_STRING_BUF_SIZE = 1;
    size_t max_chunk_len_, data_buffer_size_, string_buffer_size_;
  public:
    CommonModelParams(size_t max_chunk_len, size_t data_buffer_size, size_t string_buffer_size)
        : max_chunk_len_(std::max(max_chunk_len, MIN_CHUNK_LEN)), data_buffer_size_(data_buffer_size + 2),
          string_buffer_size_(std::max(string_buffer_size, MIN_STRING_BUF_SIZE)) {}
    size_t max_chunk_len() const { return std::max(max_chunk_len_, MIN_CHUNK_LEN); }
    size_t data_buffer_size() const { return data_buffer_size_; }
    size_t string_buffer_size() const { return string_buffer_size_; }
    void set_max_chunk_len(size_t v) { max_chunk_len_ = std::max(v, MIN_CHUNK_LEN); }
    void set_data_buffer_size(size_t v) { data_buffer_size_ = v + 2; }
    void set_string_buffer_size(size_t v) { string_buffer_size_ = std::max(v, MIN_STRING_BUF_SIZE); }
};

namespace whisper {

constexpr uint32_t SAMPLE_RATE = 16000;       // Model::SAMPLE_RATE (model.rs:52)
constexpr size_t N_SAMPLES = NH_N_SAMPLES;    // candle m::N_SAMPLES
constexpr double NO_SPEECH_THRESHOLD = 0.6, LOGPROB_THRESHOLD = -1.0;
constexpr int N_TEMPERATURES = 6;
constexpr float TEMPERATURES[N_TEMPERATURES] = {0.0f, 0.2f, 0.4f, 0.6f, 0.8f, 1.0f};  // candle m::TEMPERATURES (model.rs:175)

// whisper/mod.rs:64-84 (variants that can occur on this path) + the run-time error of model.rs:44-46
struct Error {
    enum Kind { None, TokenId, Backend /* TranscriberError */, MelBins, Respnsivness, UnsupportedDevice } kind = None;
    std::string message;
    explicit operator bool() const { return kind != None; }
};

enum class VocabVersion { V1, V2, EnV1, EnV2 };  // whisper/mod.rs:57-62

// monolingual.rs:32-46 (ids/revisions are download metadata, out of scope offline)
// monolingual::ModelType (monolingual.rs:32-46) followed by multilingual::ModelType (multilingual.rs:47-57); one Definition
// class serves both families here (language fixed = monolingual / MultiAsMono, language detected = multilingual)
enum class ModelType { TinyEn, BaseEn, SmallEn, MediumEn, DistilMediumEn, DistilLargeEnV2, DistilLargeEnV3,
                       QuantizedTinyEn, QuantizedTiny,   // the q8_0 GGUF checkpoints
                       Tiny, Base, Small, Medium, Large, LargeV2, LargeV3 };
inline VocabVersion vocab_version(ModelType m) {  // monolingual.rs:99-110, multilingual.rs:73-84
    switch (m) {
        case ModelType::TinyEn: case ModelType::BaseEn: case ModelType::SmallEn: case ModelType::MediumEn:
        case ModelType::QuantizedTinyEn: return VocabVersion::EnV1;
        case ModelType::DistilLargeEnV3: case ModelType::LargeV3: return VocabVersion::V2;
        default: return VocabVersion::V1;
    }
}
// multilingual.rs:87-92 / the monolingual twin: file-name infix of the quantised checkpoints, nullptr for the others
inline const char *quantized_ext(ModelType m) {
    return m == ModelType::QuantizedTiny ? "tiny" : m == ModelType::QuantizedTinyEn ? "tiny-en" : nullptr;
}

// whisper::Language (languages.rs:7-107): the 99 languages in `Language::iter()` order; token = "<|code|>" (:119-222)
static const char *const LANGUAGE_CODES[99] = {
    "en", "zh", "de", "es", "ru", "ko", "fr", "ja", "pt", "tr", "pl", "ca", "nl", "ar", "sv", "it", "id", "hi", "fi", "vi",
    "he", "uk", "el", "ms", "cs", "ro", "da", "hu", "ta", "no", "th", "ur", "hr", "bg", "lt", "la", "mi", "ml", "cy", "sk",
    "te", "fa", "lv", "bn", "sr", "az", "sl", "kn", "et", "mk", "br", "eu", "is", "hy", "ne", "mn", "bs", "kk", "sq", "sw",
    "gl", "mr", "pa", "si", "km", "sn", "yo", "so", "af", "oc", "ka", "be", "tg", "sd", "gu", "am", "yi", "lo", "uz", "fo",
    "ht", "ps", "tk", "nn", "mt", "sa", "lb", "my", "bo", "tl", "mg", "as", "tt", "haw", "ln", "ha", "ba", "jw", "su"};

// crate::dtype::DType (src/dtype.rs:10-45): the sample types a capture stream may deliver.  `valid` marks the four that are
// candle DTypes in the reference (u8, u32, f32, f64: "These are valid DTypes"); the others "can (will) be converted".  Here
// every one of them maps to an NH_SAMPLE_* code of the C ABI, whose nh_logmel_samples does dasp_sample's conversion to
// Model::Data (f32) on the GPU.
template <typename T> struct DType;
#define NORMA_DTYPE(T, CODE, VALID) template <> struct DType<T> { static constexpr int sample = CODE; static constexpr bool valid = VALID; }
NORMA_DTYPE(uint8_t, NH_SAMPLE_U8, true);   NORMA_DTYPE(uint32_t, NH_SAMPLE_U32, true);
NORMA_DTYPE(float, NH_SAMPLE_F32, true);    NORMA_DTYPE(double, NH_SAMPLE_F64, true);
NORMA_DTYPE(int8_t, NH_SAMPLE_I8, false);   NORMA_DTYPE(int16_t, NH_SAMPLE_I16, false);
NORMA_DTYPE(int32_t, NH_SAMPLE_I32, false); NORMA_DTYPE(int64_t, NH_SAMPLE_I64, false);
NORMA_DTYPE(uint16_t, NH_SAMPLE_U16, false); NORMA_DTYPE(uint64_t, NH_SAMPLE_U64, false);
#undef NORMA_DTYPE


// ---- audio ingest (src/lib.rs:172-216): native frames at the device's rate -> Model::Data at SAMPLE_RATE ------------------
// The streaming bookkeeping of Resampler as a pure function (nm_resample_plan of norma_host.h; no GPU): a stream has
// `received` frames so far, `emitted` outputs so far, and still keeps the frames from `first_kept` on.  With L, M, Wc of
// nh_resample (Wc = T / 2): output n is ready when floor(n M / L) + Wc <= received - 1, or, on the final push, when
// n < ceil(received L / M) (frames past the end are zeros).  n_ready: outputs emitted .. emitted + n_ready - 1 are ready now;
// f0, num0: the window [f0, ..) and start position nh_resample takes for output `emitted`; drop_before: the first frame
// still needed once they are out (everything received, on the final push).
struct ResamplePlan { long long n_ready = 0, f0 = 0, num0 = 0, drop_before = 0; };
inline bool resample_plan(int src_hz, long long received, long long emitted, long long first_kept, bool final_push, ResamplePlan &pl) {
    int32_t L = 0, M = 0, T = 0;
    if (nh_resample_table(nullptr, src_hz, nullptr, &L, &M, &T) || received < 0 || emitted < 0 || first_kept < 0 || first_kept > received) return false;
    const long long Wc = T / 2, lo = Wc > 0 ? Wc - 1 : 0;
    const long long usable = final_push ? received : received - Wc;              // outputs below ceil(usable L / M) are ready
    const long long total = usable > 0 ? (usable * L + M - 1) / M : 0;
    pl.n_ready = std::max(0LL, total - emitted);
    pl.f0 = std::max(first_kept, emitted * M / L - lo);
    pl.num0 = emitted * M - pl.f0 * L;
    pl.drop_before = final_push ? received : std::min(received, std::max(first_kept, (emitted + pl.n_ready) * M / L - lo));
    return true;
}

// The streaming form of nh_resample: push(frames, n, final) returns the 16 kHz samples that have become computable.  It keeps
// the frames it still needs and the counts of frames received and outputs emitted; every push calls nh_resample on the kept
// window, in pieces of at most 480000 outputs.  The samples are those of nh_resample on the whole stream, whatever the pieces.
// (The reference's ring buffer restarts at every capture callback, src/lib.rs:198-202; this one does not.)
class Resampler {
  public:
    Resampler(nh_ctx *ctx, int src_hz, int channels, int sample_dtype)
        : ctx_(ctx), src_hz_(src_hz), channels_(channels), dtype_(sample_dtype), frame_bytes_((size_t)nh_sample_size(sample_dtype) * (size_t)std::max(channels, 0)) {}
    int src_hz() const { return src_hz_; }
    int channels() const { return channels_; }
    int sample_dtype() const { return dtype_; }
    long long received() const { return received_; }
    long long emitted() const { return emitted_; }
    size_t kept_frames() const { return frame_bytes_ ? kept_.size() / frame_bytes_ : 0; }
    const char *last_error() const { return nh_last_error(ctx_); }
    // the stream lives on the host (kept frames, counters); the context only lends its device buffers, so a stream goes on
    // across a change of context (Model::set_beam_size replaces the model's)
    void rebind(nh_ctx *ctx) { ctx_ = ctx; }
    // frames: n frames of `channels` interleaved samples of the resampler's type.  Appends to `out`.  false: the backend
    // refused (nh_last_error has the message); the stream is reset.
    bool push(const void *frames, size_t n, bool final_push, std::vector<float> &out) {
        int32_t L = 0, M = 0, T = 0;
        if (!frame_bytes_ || nh_resample_table(ctx_, src_hz_, nullptr, &L, &M, &T)) { reset(); return refuse(); }
        const long long Wc = T / 2;
        const char *src = static_cast<const char *>(frames);
        kept_.insert(kept_.end(), src, src + n * frame_bytes_);
        received_ += (long long)n;
        ResamplePlan pl;
        if (!resample_plan(src_hz_, received_, emitted_, first_kept_, final_push, pl)) { reset(); return refuse(); }
        const long long drop_before = pl.drop_before;
        for (long long left = pl.n_ready; left > 0;) {
            const int32_t piece = (int32_t)std::min<long long>(left, NH_N_SAMPLES);
            resample_plan(src_hz_, received_, emitted_, first_kept_, final_push, pl);   // f0, num0 of this piece
            const long long hi = std::min(received_, (emitted_ + piece - 1) * M / L + Wc + 1);
            const int32_t nf = (int32_t)(hi - pl.f0);
            const int64_t num0 = pl.num0;
            const size_t at = out.size();
            out.resize(at + (size_t)piece);
            if (nh_resample(ctx_, kept_.data() + (size_t)(pl.f0 - first_kept_) * frame_bytes_, 0, dtype_, channels_, src_hz_, &nf, nf, 1,
                            &num0, &piece, out.data() + at, piece)) { out.resize(at); reset(); return false; }
            emitted_ += piece; left -= piece;
        }
        if (final_push) reset();
        else {
            kept_.erase(kept_.begin(), kept_.begin() + (long)((size_t)(drop_before - first_kept_) * frame_bytes_));
            first_kept_ = drop_before;
        }
        return true;
    }
    void reset() { kept_.clear(); received_ = emitted_ = first_kept_ = 0; }

  private:
    bool refuse() {   // leaves the refusal's message in the context: a whole-clip call with the same format is refused the same way
        const int32_t one = 1; const float z = 0.f;
        nh_resample(ctx_, &z, 0, dtype_, channels_, src_hz_, &one, 1, 1, nullptr, nullptr, nullptr, 0);
        return false;
    }
    nh_ctx *ctx_;
    int src_hz_, channels_, dtype_;
    size_t frame_bytes_;
    std::vector<char> kept_;
    long long received_ = 0, emitted_ = 0, first_kept_ = 0;
};

enum class Task { Transcribe, Translate };  // multilingual.rs:19-25

struct DecodingResult {  // model.rs:494-499
    std::vector<uint32_t> tokens;
    double avg_logprob = 0, no_speech_prob = 0, compression_ratio = 0;
    // with alignment heads set (Model::set_alignment_heads): first and last 20 ms encoder frame of every token, -1 for the
    // prompt; empty otherwise (no counterpart in the reference, whose timing stops at the segment)
    std::vector<int32_t> first_frame, last_frame;
    bool loop_exit = false;   // the decode left by the repetition guard's loop exit (Model::set_repetition_guard; never under a beam)
};

// one `<ts> text <ts|eot>` span, model.rs:100-149.  token_start / token_end: seconds from the start of the slice the segment was
// decoded from, one pair per entry of `tokens`, when alignment heads are set; empty otherwise
struct Segment { std::vector<uint32_t> tokens; std::string text; std::vector<float> token_start, token_end; };

// The loaded model: owns one nh_ctx (batch 1, like the reference) and the carried-over PCM buffer.
class Model {
  public:
    typedef float Data;                               // Model::Data = f32 (model.rs:49)
    Model(nh_ctx *ctx, nh_config cfg, nh_tokens tk) : ctx_(ctx), cfg_(cfg), tk_(tk) {}
    Model(Model &&) = delete;   // the nh_ctx * is raw, and nothing moves a Model
    Model(const Model &) = delete;
    ~Model() { if (ctx_) nh_destroy(ctx_); }

    void set_detokenizer(std::function<std::string(const uint32_t *, size_t)> f) { detok_ = std::move(f); }
    // LanguageState::Detect (model.rs:393-440): the language is inferred on the first slice of a transcription and
    // cleared on final_chunk; `language_tokens` in Language::iter() order (multilingual.rs:395-398)
    void enable_language_detection(std::vector<int32_t> language_tokens) { detect_ = true; lang_tokens_ = std::move(language_tokens); lang_token_ = -1; }
    int32_t language_token() const { return detect_ ? lang_token_ : tk_.lang; }
    size_t buffered_samples() const { return buf_.size(); }
    // Token-level timestamps: with a non-empty list, every decode keeps those heads' cross-attention queries
    // (nh_align_capture) and decode_with_fallback aligns the attempt it accepts from them (nh_align_decoded over the
    // audio-bearing frames of the slice: no second decoder pass); transcribe fills Segment::token_start / token_end.  Empty
    // (the default): off, nothing runs and nothing changes.  The list reaches the context with the next slice.
    void set_alignment_heads(std::vector<nh_align_head> heads) { align_heads_ = std::move(heads); capture_stale_ = true; }
    // what the checkpoint's generation_config.json lists as alignment_heads ([layer, head] pairs; empty without one).
    // Remembered, not enabled: hand it to set_alignment_heads to turn the timestamps on.
    const std::vector<nh_align_head> &checkpoint_alignment_heads() const { return checkpoint_heads_; }
    void set_checkpoint_alignment_heads(std::vector<nh_align_head> heads) { checkpoint_heads_ = std::move(heads); }

    // Decoder prompts (nh_set_prompts; no counterpart in the reference, whose every decode starts from [sot, lang?, task]).
    // set_prompt_tokens: an initial prompt -- token ids, the tokenizer here only decodes -- for every slice.
    // set_condition_on_previous: inside transcribe the text tokens of the segments it emits are kept as history, and a slice
    // decodes under [<|startofprev|>] + (initial prompt + history) cut to its last max_target_positions / 2 - 2 ids; every
    // temperature of decode_with_fallback uses that same prefix.  The history is dropped on final_chunk and after a slice
    // that was accepted at a temperature above 0.5 (what it says is not to be trusted as context).  Both off (the default):
    // the calls and the bits of a model without them.  Under a prefix a slice's tokens get no times (set_alignment_heads):
    // nh_align_decoded does not cover prompted decodes.
    void set_prompt_tokens(std::vector<int32_t> ids) { prompt_tokens_ = std::move(ids); }
    void set_condition_on_previous(bool on) { condition_ = on; if (!on) history_.clear(); }
    void set_startofprev_token(int32_t id) { sop_token_ = id; }   // <|startofprev|> (token_to_id at load; -1: unknown)
    // what the next slice decodes under; empty: no prefix
    std::vector<int32_t> prompt_prefix() const {
        std::vector<int32_t> body(prompt_tokens_);
        if (condition_) body.insert(body.end(), history_.begin(), history_.end());
        std::vector<int32_t> out;
        if (body.empty()) return out;
        const size_t room = (size_t)std::max(0, cfg_.max_target_positions / 2 - 2);
        const size_t from = body.size() > room ? body.size() - room : 0;
        out.push_back(sop_token_);
        out.insert(out.end(), body.begin() + (long)from, body.end());
        return out;
    }

    // The format of the frames transcribe_frames takes: the capture device's rate and channel count (src/lib.rs:172-216 reads
    // them from the stream's config).  The default, 16 000 Hz mono, is what transcribe takes.  A new format starts a new stream.
    void set_input_format(uint32_t src_hz, int channels) { src_hz_ = src_hz; channels_ = channels; resampler_.reset(); }
    uint32_t input_rate() const { return src_hz_; }
    int input_channels() const { return channels_; }
    nh_ctx *context() const { return ctx_; }
    // Native frames in, as the capture callback hands them over (n frames of input_channels() interleaved samples of one
    // NH_SAMPLE_* type): they go through the model's Resampler (mixdown and resampling on the device), the 16 kHz samples that
    // became computable are appended to the buffer transcribe uses, and transcribe's loop runs on it unchanged.  final_chunk
    // also flushes the resampler (the tail of the stream, zeros beyond its end) and resets it.
    Error transcribe_frames(const void *frames, int sample_dtype, size_t n, bool final_chunk, std::vector<Segment> &out, std::string *text = nullptr) {
        if (!resampler_ || resampler_->sample_dtype() != sample_dtype)
            resampler_.reset(new Resampler(ctx_, (int)src_hz_, channels_, sample_dtype));
        std::vector<float> pcm;
        if (!resampler_->push(frames, n, final_chunk, pcm)) return backend_error();
        return transcribe(pcm, final_chunk, out, text);
    }
    template <typename T>
    Error transcribe_frames(const T *frames, size_t n, bool final_chunk, std::vector<Segment> &out, std::string *text = nullptr) {
        return transcribe_frames(static_cast<const void *>(frames), DType<T>::sample, n, final_chunk, out, text);
    }

    // Model::transcribe (model.rs:55-159).  `data` is consumed (swapped/appended into the model's buffer).
    // Returns an Error with kind != None on a backend failure (the reference's TranscriberError, which
    // ends the transcriber thread: src/lib.rs:466-477).
    Error transcribe(std::vector<float> &data, bool final_chunk, std::vector<Segment> &out, std::string *text = nullptr) {
        if (buf_.empty()) std::swap(buf_, data);                      // :60-64
        else { buf_.insert(buf_.end(), data.begin(), data.end()); data.clear(); }
        bool stop = false;
        while (!buf_.empty() && !stop) {                              // 'new_chunk, :68
            const size_t slice_len = std::min(buf_.size(), N_SAMPLES);
            DecodingResult dr;
            bool have = false;
            Error e = decode_with_fallback(buf_.data(), slice_len, dr, have);
            if (e) return e;
            if (!have) { drain(slice_len); continue; }                // :90-93
            const size_t first_new = out.size();                      // the segments this slice appends are the history's
            if (dr.no_speech_prob > NO_SPEECH_THRESHOLD && dr.avg_logprob < LOGPROB_THRESHOLD) { drain(slice_len); continue; }  // :95-98
            bool drained = false;
            for (auto seg : inclusive_boxed_by(dr.tokens, [&](uint32_t t) { return t > (uint32_t)tk_.no_timestamps || t == (uint32_t)tk_.eot; })) {
                const uint32_t *tok = dr.tokens.data() + seg.first;
                const size_t n = seg.second - seg.first;
                const uint32_t s_timestamp = tok[0] - (uint32_t)tk_.no_timestamps - 1;  // :103
                const uint32_t e_tok = tok[n - 1];
                if (e_tok == (uint32_t)tk_.eot) {
                    if (s_timestamp == 0 || final_chunk) {
                        if (slice_len == N_SAMPLES || final_chunk) { drain(slice_len); drained = true; }  // :109-115
                        else { stop = true; break; }                                                     // :116-123
                    } else {
                        const size_t pre = buf_.size();
                        drain(std::min((size_t)s_timestamp * 320, slice_len));                           // :125-127
                        drained = true;
                        if (pre > slice_len) break;                                                       // :129-136
                        stop = true; break;                                                               // :138-143
                    }
                }
                Segment sg;
                sg.tokens.assign(tok + 1, tok + n - 1);                                                   // tokens[1..len-1], :147
                if (!dr.first_frame.empty())
                    for (size_t i = seg.first + 1; i + 1 < seg.second; i++) {   // 20 ms per encoder frame
                        sg.token_start.push_back(0.02f * (float)dr.first_frame[i]);
                        sg.token_end.push_back(0.02f * (float)(dr.last_frame[i] + 1));
                    }
                if (detok_) { sg.text = detok_(sg.tokens.data(), sg.tokens.size()); if (text) *text += sg.text; }
                out.push_back(std::move(sg));
            }
            // H1: a result without any drained segment (e.g. the no-speech early return, whose
            // tokens hold no timestamp, or segments that all close on a timestamp) leaves `buf` untouched in the
            // reference, which then spins forever on the same slice.  Deviation: drain the slice and go on.
            if (!stop && !drained) drain(slice_len);
            if (condition_) {
                if (TEMPERATURES[accepted_] > 0.5f) history_.clear();
                else for (size_t i = first_new; i < out.size(); i++) history_.insert(history_.end(), out[i].tokens.begin(), out[i].tokens.end());
            }
        }
        if (final_chunk) {                                            // :153-156
            if (detect_) lang_token_ = -1;                            // self.lang.clear()
            history_.clear();
            int rc = nh_reset(ctx_);
            if (rc) return backend_error();
        }
        return Error{};
    }

    // decode_with_fallback (model.rs:164-191).  The t = 0 pass is deterministic.  The sampled attempts (t = 0.2 .. 1.0)
    // draw from an entropy-seeded RNG in the reference (monolingual.rs:433-439) and cannot be reproduced draw for draw;
    // here they follow the seeded sampling contract of include/norma_hip.h (same distribution).  Default = the
    // reference's behaviour: the loop is ON and the seed comes from std::random_device (StdRng::from_entropy), so a
    // hopeless slice is dropped exactly when the reference would drop it.  set_temperature_fallback(true, seed) fixes the
    // seed (reproducible tests); set_temperature_fallback(false, _) returns the t = 0 result even when the reference would
    // have gone on, and last_needed_fallback() says so.
    void set_temperature_fallback(bool enable, uint64_t seed) { fallback_ = enable; seed_ = seed; slices_ = 0; }
    // Beam search for the t = 0 attempt (nh_decode_beam; the reference decodes greedily, Whisper runtimes default to 5 beams).
    // k = 1, the default, is the greedy decode and changes nothing; at k > 1 attempt 0 of the TEMPERATURES loop keeps k
    // hypotheses and returns the best, the sampled attempts stay as they are.  The context a model is made with decodes one
    // row; the first k beyond its rows replaces it by one of k rows on the same weights (nh_create_shared), told the same
    // tokens: a model whose suppress list was never recorded (set_suppress_tokens; the loaders call it) is refused there, not
    // told an empty one.  A stream of transcribe_frames goes on across the change: its resampler is handed the new context.
    // A slice decoded by the beam gets no token times (the kept queries are not reordered with the hypotheses).
    Error set_beam_size(int k) {
        if (k < 1 || k > NH_MAX_BEAMS) return Error{Error::Backend, "set_beam_size: 1 .. " + std::to_string(NH_MAX_BEAMS)};
        if (k > ctx_rows_) {
            if (!suppress_known_)
                return Error{Error::Backend, "set_beam_size: the suppress list this model's context was told is not recorded (set_suppress_tokens)"};
            nh_ctx *c = nullptr;
            if (nh_create_shared(ctx_, k, &c)) return backend_error();
            if (nh_set_tokens(c, &tk_, suppress_.data(), (int)suppress_.size())) { Error e{Error::Backend, nh_last_error(c)}; nh_destroy(c); return e; }
            // ... and the same guard and bias list
            if (nh_set_guard(c, &guard_) || nh_guard_bias(c, 0, bias_tok_.data(), bias_val_.data(), (int)bias_tok_.size())) { Error e{Error::Backend, nh_last_error(c)}; nh_destroy(c); return e; }
            nh_destroy(ctx_);
            ctx_ = c; ctx_rows_ = k;
            if (resampler_) resampler_->rebind(c);
            capture_stale_ = !align_heads_.empty();
        }
        beam_size_ = k;
        return Error{};
    }
    // The repetition guard of every decode of this model (nh_set_guard, include/norma_hip.h; no counterpart in the reference):
    // no-repeat n-gram, repetition penalty, loop exit, and whether the token bias below applies.  {0, 1.0, 0, 0, 0} (the
    // default) is off: the calls and the bits of a model without it.  A refused value leaves the guard as it was.
    Error set_repetition_guard(const nh_guard_params &p) {
        if (nh_set_guard(ctx_, &p)) return backend_error();
        guard_ = p;
        return Error{};
    }
    // {token: beta} for the model's single row (nh_guard_bias), applied while the guard has bias != 0; n = 0 clears it
    Error set_token_bias(const int32_t *ids, const float *beta, int n) {
        if (nh_guard_bias(ctx_, 0, ids, beta, n)) return backend_error();
        bias_tok_.assign(ids, ids + (n > 0 ? n : 0)); bias_val_.assign(beta, beta + (n > 0 ? n : 0));
        return Error{};
    }
    void set_suppress_tokens(std::vector<int32_t> ids) { suppress_ = std::move(ids); suppress_known_ = true; }   // what the context was told (the loaders call it)
    Error decode_with_fallback(const float *pcm, size_t n, DecodingResult &dr, bool &have) {
        int32_t ns = (int32_t)n;
        if (nh_logmel(ctx_, pcm, &ns, (int64_t)n, 1)) return backend_error();   // audio::pcm_to_mel + narrow, :74-88
        if (nh_encode(ctx_)) return backend_error();                            // encoder_forward(mel, true), :168
        if (detect_) {                                                          // :170-173
            if (lang_token_ < 0) {
                if (nh_detect_language(ctx_, lang_tokens_.data(), (int)lang_tokens_.size(), &lang_token_, nullptr)) return backend_error();
            } else if (nh_set_languages(ctx_, &lang_token_)) return backend_error();
        }
        if (capture_stale_) {                                                   // the decodes below keep the heads' queries
            if (nh_align_capture(ctx_, align_heads_.data(), (int)align_heads_.size())) return backend_error();
            capture_stale_ = false;
        }
        // the prefix of this slice (nh_logmel above cleared the one before); the same for every temperature below
        const std::vector<int32_t> prefix = prompt_prefix();
        if (!prefix.empty()) {
            if (sop_token_ < 0) return Error{Error::Backend, "a decoder prompt needs the <|startofprev|> token (set_startofprev_token)"};
            if (nh_set_prompts(ctx_, prefix.data(), (int)prefix.size(), (int64_t)prefix.size(), 1)) return backend_error();
        }
        std::vector<int32_t> toks(cfg_.max_target_positions);
        have = false;
        const uint32_t clip = slices_++;
        for (int a = 0; a < N_TEMPERATURES && !have; a++) {                      // for &t in m::TEMPERATURES, :175
            nh_decode_result r{};
            const bool beam = a == 0 && beam_size_ > 1;
            if (beam) { if (nh_decode_beam(ctx_, beam_size_, toks.data(), &r, 0)) return backend_error(); }
            else if (a == 0) { if (nh_decode_greedy(ctx_, toks.data(), &r, 0)) return backend_error(); }   // decode(.., 0.0), :176
            else if (nh_decode_sampled(ctx_, toks.data(), &r, 0, TEMPERATURES[a], seed_, clip, (uint32_t)a)) return backend_error();
            dr.tokens.assign(toks.begin(), toks.begin() + r.n_tokens);
            dr.avg_logprob = r.avg_logprob; dr.no_speech_prob = r.no_speech_prob;
            dr.compression_ratio = 0.0 / 0.0;                                    // f64::NAN, :387
            dr.loop_exit = false;
            if (guard_.loop_period > 0 && !beam) {                               // the flag does not travel with a beam hypothesis
                int32_t le = 0;
                if (nh_guard_report(ctx_, nullptr, 1, &le)) return backend_error();
                dr.loop_exit = le != 0;
            }
            // :177-187 -- accept unless avg_logprob < -1 (compression_ratio is NaN, so that test is always false)
            const bool needs_fallback = dr.avg_logprob < LOGPROB_THRESHOLD;
            if (a == 0) needs_fallback_ = needs_fallback && !(dr.no_speech_prob > NO_SPEECH_THRESHOLD);
            if (!needs_fallback || dr.no_speech_prob > NO_SPEECH_THRESHOLD || !fallback_) { have = true; accepted_ = a; }
            dr.first_frame.clear(); dr.last_frame.clear();
            const int P = (detect_ || tk_.lang >= 0) ? 3 : 2;                    // [sot, lang?, task], model.rs:285-289
            if (have && !beam && !align_heads_.empty() && r.n_tokens > P && prefix.empty()) {               // the accepted attempt; a no-speech exit holds the prompt alone
                const int32_t nt = r.n_tokens;
                const int32_t nk = (int32_t)std::min<size_t>((size_t)cfg_.max_source_positions, (n + 319) / 320);   // frames that hold audio
                std::vector<int32_t> first(cfg_.max_target_positions), last(cfg_.max_target_positions);
                if (nh_align_decoded(ctx_, nullptr, 1, &nk, first.data(), last.data())) return backend_error();   // of the decode just above
                dr.first_frame.assign(first.begin(), first.begin() + nt);
                dr.last_frame.assign(last.begin(), last.begin() + nt);
            }
        }
        last_ = dr;
        return Error{};                                                          // have == false: Ok(None), :189-190
    }
    const DecodingResult &last_result() const { return last_; }
    bool has_detokenizer() const { return (bool)detok_; }
    bool last_needed_fallback() const { return needs_fallback_; }

  private:
    static uint64_t entropy_seed() { std::random_device rd; return ((uint64_t)rd() << 32) ^ (uint64_t)rd(); }  // StdRng::from_entropy, monolingual.rs:433
    void drain(size_t n) { buf_.erase(buf_.begin(), buf_.begin() + (long)std::min(n, buf_.size())); }
    Error backend_error() const { return Error{Error::Backend, nh_last_error(ctx_)}; }
    nh_ctx *ctx_;
    nh_config cfg_;
    nh_tokens tk_;
    std::vector<float> buf_;
    std::function<std::string(const uint32_t *, size_t)> detok_;
    DecodingResult last_;
    bool needs_fallback_ = false;
    bool fallback_ = true;
    uint64_t seed_ = entropy_seed();
    uint32_t slices_ = 0;
    bool detect_ = false;
    std::vector<nh_align_head> align_heads_, checkpoint_heads_;
    bool capture_stale_ = false;   // align_heads_ changed since the context was last told (nh_align_capture)
    std::vector<int32_t> lang_tokens_;
    int32_t lang_token_ = -1;
    uint32_t src_hz_ = SAMPLE_RATE;
    int channels_ = 1;
    std::unique_ptr<Resampler> resampler_;   // made by the first transcribe_frames
    std::vector<int32_t> prompt_tokens_, history_;   // the initial prompt; the text tokens emitted since the last final_chunk
    bool condition_ = false;
    int32_t sop_token_ = -1;
    int accepted_ = 0;                       // index into TEMPERATURES of the attempt the last decode_with_fallback accepted
    std::vector<int32_t> suppress_;          // the suppress list the context was told (a beam context is told again)
    bool suppress_known_ = false;            // set_suppress_tokens was called: an empty list is then a list, not an omission
    int beam_size_ = 1, ctx_rows_ = 1;       // set_beam_size; rows the context decodes (its max_batch)
    nh_guard_params guard_{0, 1.0f, 0, 0, 0};   // set_repetition_guard; what the context was told (a beam context is told again)
    std::vector<int32_t> bias_tok_;          // set_token_bias
    std::vector<float> bias_val_;
};

// One tensor handed to the loader (HF name, f32 or f16 data) -- stands in for the safetensors mmap of
// monolingual.rs:237-239; the caller decides where the bytes come from.
struct TensorView { std::string name; int dtype; std::vector<int64_t> shape; const void *data; };

// monolingual::Definition (monolingual.rs:113-174, 176-452).  The hf-hub download is out of scope (no
// network); the loaded pieces (config, special-token ids, suppress list, mel filters, tensors) are passed in.
class Definition {
  public:
    Definition(ModelType model, SelectedDevice device)  // Definition::new, monolingual.rs:124-130
        : model_(model), device_(device), common_params_(SAMPLE_RATE * 25, 3, 3) {}
    const CommonModelParams &common_params() const { return common_params_; }
    Error set_responsiveness(uint64_t period_ms) {      // monolingual.rs:147-156
        if (period_ms >= 1000 && period_ms <= 30000) { common_params_.set_max_chunk_len((size_t)SAMPLE_RATE * period_ms / 1000); return Error{}; }
        return Error{Error::Respnsivness, "The respnsivness must be over 1 second and under 30"};
    }
    void set_data_buffer_size(size_t n) { common_params_.set_data_buffer_size(n); }
    void set_string_buffer_size(size_t n) { common_params_.set_string_buffer_size(n); }
    ModelType model() const { return model_; }
    // what the capture device delivers (Model::transcribe_frames); the default is Model::SAMPLE_RATE, mono
    void set_input_format(uint32_t src_hz, int channels) { src_hz_ = src_hz; channels_ = channels; }

    // blocking_try_to_model (monolingual.rs:320-451) for SelectedDevice::Rocm.
    Error blocking_try_to_model(const nh_config &cfg, const nh_tokens &tk, const std::vector<int32_t> &suppress,
                                const float *mel_filters, int n_mel, const std::vector<TensorView> &tensors,
                                Model **out) const {
        if (device_.kind != SelectedDevice::Rocm)
            return Error{Error::UnsupportedDevice, "this build only implements SelectedDevice::Rocm(ord)"};
        if (n_mel != 80 && n_mel != 128)   // whisper::Error::MelBins, monolingual.rs:351-355
            return Error{Error::MelBins, "Unexpected number of mel bins (num_mel_bins), got: " + std::to_string(n_mel)};
        nh_ctx *ctx = nullptr;
        if (nh_create((int)device_.ordinal, &cfg, 1, &ctx)) return Error{Error::Backend, nh_last_error(nullptr)};
        auto fail = [&]() { Error e{Error::Backend, nh_last_error(ctx)}; nh_destroy(ctx); return e; };
        for (const auto &t : tensors)
            if (nh_load_tensor(ctx, t.name.c_str(), t.dtype, t.shape.data(), (int)t.shape.size(), t.data)) return fail();
        if (nh_missing_tensors(ctx) != 0) { nh_destroy(ctx); return Error{Error::Backend, "checkpoint is missing tensors"}; }
        if (nh_set_mel_filters(ctx, mel_filters, n_mel)) return fail();
        if (nh_set_tokens(ctx, &tk, suppress.data(), (int)suppress.size())) return fail();
        *out = new Model(ctx, cfg, tk);
        (*out)->set_suppress_tokens(suppress);
        (*out)->set_input_format(src_hz_, channels_);
        return Error{};
    }

    // The same from a local checkpoint directory holding config.json, tokenizer.json and model.safetensors
    // (what monolingual.rs:323-373 reads after the hf-hub download).  `language` is the `<|xx|>` token of
    // ModelType::language() (monolingual.rs:85-97, :384); translate selects <|translate|> (multilingual.rs:383-386).
    Error blocking_try_to_model_from_dir(const std::string &dir, const float *mel_filters, int n_mel, Model **out,
                                         const std::string &language = "<|en|>", bool translate = false,
                                         bool detect_language = false) const {
        std::string err;
        // quantised models: config-{ext}.json / tokenizer-{ext}.json / model-{ext}-q80.gguf (multilingual.rs:195-199)
        const char *qext = quantized_ext(model_);
        const std::string sfx = qext ? std::string("-") + qext : std::string();
        assets::ConfigJson cj;
        if (!cj.load(dir + "/config" + sfx + ".json", err)) return Error{Error::Backend, err};
        auto tok = std::make_shared<assets::TokenizerJson>();
        if (!tok->load(dir + "/tokenizer" + sfx + ".json", err)) return Error{Error::Backend, err};
        auto id = [&](const char *t, int &dst) { dst = tok->token_to_id(t); return dst >= 0; };
        nh_tokens tk{};
        // candle constants m::SOT_TOKEN, EOT_TOKEN, TRANSCRIBE_TOKEN, TRANSLATE_TOKEN, NO_TIMESTAMPS_TOKEN, NO_SPEECH_TOKENS
        if (!id("<|startoftranscript|>", tk.sot)) return Error{Error::TokenId, "Failed to get token ID for: <|startoftranscript|>"};
        if (!id("<|endoftext|>", tk.eot)) return Error{Error::TokenId, "Failed to get token ID for: <|endoftext|>"};
        if (!id(translate ? "<|translate|>" : "<|transcribe|>", tk.task)) return Error{Error::TokenId, "Failed to get token ID for the task token"};
        if (!id("<|nocaptions|>", tk.no_speech) && !id("<|nospeech|>", tk.no_speech)) return Error{Error::TokenId, "Failed to get token ID for: <|nocaptions|> nor <|nospeech|>"};
        if (!id("<|notimestamps|>", tk.no_timestamps)) return Error{Error::TokenId, "Failed to get token ID for: <|notimestamps|>"};
        std::vector<int32_t> lang_tokens;
        if (detect_language) {  // multilingual::Definition: LanguageState::Detect (multilingual.rs:395-398, :463-466)
            tk.lang = -1;
            for (const char *code : LANGUAGE_CODES) {
                int t = tok->token_to_id(std::string("<|") + code + "|>");
                if (t < 0) return Error{Error::TokenId, std::string("Failed to get token ID for: <|") + code + "|>"};
                lang_tokens.push_back(t);
            }
        } else if (!id(language.c_str(), tk.lang)) return Error{Error::TokenId, "Failed to get token ID for: " + language};
        if (!id("<|0.00|>", tk.zero_sec)) return Error{Error::TokenId, "Failed to get token ID for: <|0.00|>"};
        if (!id("<|1.00|>", tk.one_sec)) return Error{Error::TokenId, "Failed to get token ID for: <|1.00|>"};
        assets::SafeTensors st;
        assets::GgufFile gg;
        std::vector<std::vector<float>> deq;   // dequantised GGUF tensors (kept alive until the upload below)
        std::vector<TensorView> tv;
        std::vector<std::pair<size_t, size_t>> bf16_fix;
        if (qext) {
            if (!gg.open(dir + "/model-" + qext + "-q80.gguf", err)) return Error{Error::Backend, err};
            deq.resize(gg.tensors.size());
            for (size_t i = 0; i < gg.tensors.size(); i++) {
                assets::GgufFile::to_f32(gg.tensors[i], deq[i]);
                tv.push_back(TensorView{gg.tensors[i].name, NH_DTYPE_F32, gg.tensors[i].shape, deq[i].data()});
            }
        } else {
            if (!st.open(dir + "/model.safetensors", err)) return Error{Error::Backend, err};
            for (const auto &t : st.tensors) {
                if (t.dtype == "F16") tv.push_back(TensorView{t.name, NH_DTYPE_F16, t.shape, t.data});
                else if (t.dtype == "F32") tv.push_back(TensorView{t.name, NH_DTYPE_F32, t.shape, t.data});
                else if (t.dtype == "BF16") {   // widened on the host (exact); candle casts every dtype to m::DTYPE the same way
                    deq.emplace_back();
                    assets::st_to_f32(t, deq.back());
                    tv.push_back(TensorView{t.name, NH_DTYPE_F32, t.shape, nullptr});
                    bf16_fix.push_back({tv.size() - 1, deq.size() - 1});
                } else return Error{Error::Backend, "model.safetensors: unsupported dtype " + t.dtype + " for " + t.name};
            }
            for (auto &f : bf16_fix) tv[f.first].data = deq[f.second].data();   // deq may have reallocated while growing
        }
        nh_config cfg{cj.num_mel_bins, cj.max_source_positions, cj.d_model, cj.encoder_attention_heads, cj.encoder_layers,
                      cj.vocab_size, cj.max_target_positions, cj.decoder_attention_heads, cj.decoder_layers};
        Error e = blocking_try_to_model(cfg, tk, cj.suppress_tokens, mel_filters, n_mel, tv, out);
        if (e) return e;
        (*out)->set_detokenizer([tok](const uint32_t *ids, size_t n) { return tok->decode(ids, n); });  // model.rs:147
        if (detect_language) (*out)->enable_language_detection(std::move(lang_tokens));
        (*out)->set_startofprev_token(tok->token_to_id("<|startofprev|>"));   // -1 where the vocabulary has none: prompts are refused
        // generation_config.json, when the checkpoint has one: alignment_heads = [[layer, head], ...] (remembered, not enabled)
        {
            assets::MappedFile gf;
            std::string gerr;
            if (gf.open(dir + "/generation_config" + sfx + ".json", gerr)) {
                assets::Json gj; assets::JsonParser gp(gf.data(), gf.size());
                std::vector<nh_align_head> heads;
                if (gp.parse(gj) && gj.type == assets::Json::Obj)
                    if (const assets::Json *ah = gj.get("alignment_heads"))
                        for (const auto &pr : ah->arr)
                            if (pr.type == assets::Json::Arr && pr.arr.size() == 2 && pr.arr[0].type == assets::Json::Num && pr.arr[1].type == assets::Json::Num)
                                heads.push_back(nh_align_head{(int32_t)pr.arr[0].num, (int32_t)pr.arr[1].num});
                (*out)->set_checkpoint_alignment_heads(std::move(heads));
            }
        }
        return Error{};
    }

  private:
    ModelType model_;
    SelectedDevice device_;
    CommonModelParams common_params_;
    uint32_t src_hz_ = SAMPLE_RATE;
    int channels_ = 1;
};

}  // namespace whisper
}  // namespace norma
