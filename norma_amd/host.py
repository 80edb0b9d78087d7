"""Python face of the C++ host layer (norma_amd/csrc/norma_host.hpp through include/norma_host.h).

Names and behaviour follow the reference's plugin API so that tests read like the reference's own
usage (README.md:16-52, src/models/mod.rs:13-56, src/models/whisper/monolingual.rs:113-174):

    definition = monolingual.Definition(ModelType.DistilLargeEnV3, SelectedDevice.Rocm(0))
    model = definition.blocking_try_to_model(...)      # ModelDefinition::blocking_try_to_model
    segments = model.transcribe(pcm, final_chunk=True)  # Model::transcribe

The transcribe policy (buffering, 30 s windows, seek by timestamps, final_chunk) runs in C++ on top of
the C ABI; nothing here computes anything.
"""
import ctypes as C
import enum
import os
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import assets_io, cabi, hip
from .config import Config


HEADER_PATH = os.path.join(os.path.dirname(hip.HEADER_PATH), "norma_host.h")
_K = cabi.read(HEADER_PATH).constants   # NM_DEVICE_*, NM_MODEL_*


@dataclass(frozen=True)
class SelectedDevice:
    """`enum SelectedDevice { Cpu, Cuda(usize), Metal }` (src/models/mod.rs:36-43) + `Rocm(usize)`; kind is an NM_DEVICE_*."""
    kind: int = _K["NM_DEVICE_CPU"]
    ordinal: int = 0

    @staticmethod
    def Cpu():
        return SelectedDevice(_K["NM_DEVICE_CPU"], 0)

    @staticmethod
    def Cuda(n: int):
        return SelectedDevice(_K["NM_DEVICE_CUDA"], n)

    @staticmethod
    def Metal():
        return SelectedDevice(_K["NM_DEVICE_METAL"], 0)

    @staticmethod
    def Rocm(n: int):
        return SelectedDevice(_K["NM_DEVICE_ROCM"], n)


# monolingual::ModelType (monolingual.rs:32-46), its q8_0 GGUF checkpoints (Quantized*), then multilingual::ModelType
# (multilingual.rs:47-57: language=None detects the language, a fixed "<|xx|>" is MultiAsMono).  The members are the header's
# NM_MODEL_* under the reference's names: NM_MODEL_DISTIL_LARGE_EN_V3 is ModelType.DistilLargeEnV3.
ModelType = enum.IntEnum("ModelType", {"".join(w.capitalize() for w in n[len("NM_MODEL_"):].split("_")): v
                                       for n, v in _K.items() if n.startswith("NM_MODEL_")}, module=__name__)


QUANTIZED_EXT = {ModelType.QuantizedTinyEn: "tiny-en", ModelType.QuantizedTiny: "tiny"}


class WhisperError(RuntimeError):
    """whisper::Error / TranscriberError (src/models/whisper/mod.rs:64-84, model.rs:44-46)."""


_bound = False


def _lib():
    """the library with every function of include/norma_host.h bound (its nh_config / nh_tokens are hip's classes: the header
    includes norma_hip.h)"""
    global _bound
    L = hip.load_library()
    if not _bound:
        cabi.bind(L, HEADER_PATH)
        _bound = True
    return L


def resample_plan(src_hz: int, received: int, emitted: int, first_kept: int, final: bool):
    """nm_resample_plan, the streaming resampler's bookkeeping (pure, no GPU): (n_ready, f0, num0, drop_before), or None
    where it refuses."""
    v = [C.c_int64(0) for _ in range(4)]
    if _lib().nm_resample_plan(int(src_hz), int(received), int(emitted), int(first_kept), int(final), *[C.byref(x) for x in v]):
        return None
    return tuple(int(x.value) for x in v)


def _native_frames(frames: np.ndarray, channels: int) -> np.ndarray:
    """[frames][channels] (or [frames] for mono) of a native capture type, contiguous"""
    a = np.ascontiguousarray(frames)
    assert a.dtype in hip.SAMPLE_DTYPES and a.ndim in (1, 2) and (a.shape[1] if a.ndim == 2 else 1) == channels, \
        f"expected [frames][{channels}] of a capture sample type"
    return a


class Model:
    """whisper::Model: `Data = f32`, `SAMPLE_RATE = 16000` (model.rs:48-52)."""
    SAMPLE_RATE = 16000

    def __init__(self, handle, ctx_len: int):
        self._h = handle
        self._ctx_len = ctx_len
        self.buffered_samples = 0

    def close(self):
        if self._h:
            _lib().nm_model_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def transcribe(self, data: np.ndarray, final_chunk: bool) -> List[List[int]]:
        """Model::transcribe (model.rs:55-159): returns the token ids of each emitted segment."""
        data = np.ascontiguousarray(data, dtype=np.float32)
        cap = 64 * (self._ctx_len + 2)
        out = np.zeros(cap, dtype=np.int32)
        n_out, buffered = C.c_int(0), C.c_size_t(0)
        err = C.create_string_buffer(512)
        rc = _lib().nm_model_transcribe(self._h, data.ctypes.data_as(C.POINTER(C.c_float)), len(data), int(final_chunk),
                                        out.ctypes.data_as(C.POINTER(C.c_int32)), cap, C.byref(n_out), C.byref(buffered),
                                        err, 512)
        self.buffered_samples = int(buffered.value)
        if rc:
            raise WhisperError(err.value.decode())
        return self._segments(out, n_out.value)

    def _segments(self, out, n_out):
        segs, cur = [], []
        for t in out[:n_out].tolist():
            if t == -1:
                segs.append(cur)
                cur = []
            else:
                cur.append(t)
        self._last_segments = segs
        return segs

    def set_input_format(self, src_hz: int, channels: int):
        """The capture device's rate and channel count, for transcribe_frames (default: 16 000 Hz mono)."""
        _lib().nm_model_set_input_format(self._h, int(src_hz), int(channels))
        self._channels = int(channels)

    def transcribe_frames(self, frames: np.ndarray, final_chunk: bool) -> List[List[int]]:
        """Model::transcribe on native frames ([frames][channels], or [frames] for mono, of a capture sample type at the
        rate given to set_input_format): mixed down and resampled on the device by the model's streaming Resampler, then
        transcribe's own loop.  final_chunk also flushes and resets the resampler."""
        a = _native_frames(frames, getattr(self, "_channels", 1))
        cap = 64 * (self._ctx_len + 2)
        out = np.zeros(cap, dtype=np.int32)
        n_out, buffered = C.c_int(0), C.c_size_t(0)
        err = C.create_string_buffer(512)
        rc = _lib().nm_model_transcribe_frames(self._h, a.ctypes.data_as(C.c_void_p), hip.SAMPLE_DTYPES[a.dtype], a.shape[0],
                                               int(final_chunk), out.ctypes.data_as(C.POINTER(C.c_int32)), cap, C.byref(n_out),
                                               C.byref(buffered), err, 512)
        self.buffered_samples = int(buffered.value)
        if rc:
            raise WhisperError(err.value.decode())
        return self._segments(out, n_out.value)

    def enable_language_detection(self, lang_tokens: Sequence[int]):
        """multilingual LanguageState::Detect: tokens of `Language::iter()` (languages.rs:7-107) in order."""
        a = np.ascontiguousarray(lang_tokens, dtype=np.int32)
        _lib().nm_model_enable_language_detection(self._h, a.ctypes.data_as(C.POINTER(C.c_int32)), len(a))

    def set_temperature_fallback(self, enable: bool, seed: int = 0):
        """decode_with_fallback's sampled attempts (model.rs:175-188) on/off; draws follow the seeded sampling contract."""
        _lib().nm_model_set_temperature_fallback(self._h, int(enable), int(seed))

    def set_beam_size(self, k: int):
        """Beam search with k hypotheses for the t = 0 attempt (HipWhisper.decode_beam); k = 1, the default, is the greedy
        decode.  The sampled fallback attempts are unchanged."""
        if _lib().nm_model_set_beam_size(self._h, int(k)):
            raise WhisperError(f"set_beam_size: 1 .. 8 hypotheses (and device memory for a context of that many rows), got {k}")

    def set_repetition_guard(self, no_repeat_ngram: int = 0, repetition_penalty: float = 1.0, loop_period: int = 0,
                             loop_repeats: int = 0, bias: bool = False):
        """The repetition guard of every decode (HipWhisper.set_guard); no arguments: off, the default."""
        if _lib().nm_model_set_repetition_guard(self._h, int(no_repeat_ngram), float(repetition_penalty), int(loop_period),
                                                int(loop_repeats), int(bool(bias))):
            raise WhisperError("set_repetition_guard: refused (penalty > 0 and finite, n-gram 0 .. 16, period 0 .. 64, repeats 2 .. 16, period * repeats <= 448)")

    def set_token_bias(self, bias: Optional[dict]):
        """{token: beta} added to the logits of every decode while set_repetition_guard(bias=True); None or {}: none."""
        items = sorted((bias or {}).items())
        ids = np.array([k for k, _ in items], dtype=np.int32)
        bv = np.array([v for _, v in items], dtype=np.float32)
        if _lib().nm_model_set_token_bias(self._h, ids.ctypes.data_as(C.POINTER(C.c_int32)), bv.ctypes.data_as(C.POINTER(C.c_float)), len(ids)):
            raise WhisperError("set_token_bias: refused (at most 256 distinct ids inside the vocabulary, each bias finite or -inf)")

    def set_prompt_tokens(self, ids: Sequence[int]):
        """An initial prompt (token ids; the tokenizer only decodes) every slice decodes under, behind <|startofprev|>; [] = none."""
        a = np.ascontiguousarray(ids, dtype=np.int32)
        _lib().nm_model_set_prompt_tokens(self._h, a.ctypes.data_as(C.POINTER(C.c_int32)), len(a))

    def set_condition_on_previous(self, enable: bool):
        """Carry the text of the segments transcribe emits into the following slices' prompt (dropped on final_chunk and
        after a slice accepted at a temperature above 0.5)."""
        _lib().nm_model_set_condition_on_previous(self._h, int(enable))

    def set_startofprev_token(self, token: int):
        """<|startofprev|> for a model made from tensors (a checkpoint directory's tokenizer is asked by the loader)"""
        _lib().nm_model_set_startofprev_token(self._h, int(token))

    def prompt_prefix(self) -> List[int]:
        """the prefix the next slice would decode under ([] = none)"""
        a = np.zeros(self._ctx_len, dtype=np.int32)
        n = _lib().nm_model_prompt_prefix(self._h, a.ctypes.data_as(C.POINTER(C.c_int32)), len(a))
        return a[:n].tolist()

    def set_alignment_heads(self, heads: Sequence[Tuple[int, int]]):
        """Token-level timestamps: [(decoder layer, head)] switches them on for every slice transcribe decodes, an empty
        list (the default) off.  last_token_times() then holds one (start, end) per token transcribe returned."""
        a = np.ascontiguousarray(heads, dtype=np.int32).reshape(-1, 2)
        if _lib().nm_model_set_alignment_heads(self._h, a.ctypes.data_as(C.POINTER(C.c_int32)), len(a)):
            raise WhisperError(f"set_alignment_heads: 0 .. {hip.NH_ALIGN_MAX_HEADS} heads")

    def checkpoint_alignment_heads(self) -> List[Tuple[int, int]]:
        """alignment_heads of the checkpoint's generation_config.json ([] without one); not enabled by itself"""
        a = np.zeros((hip.NH_ALIGN_MAX_HEADS * 8, 2), dtype=np.int32)
        n = _lib().nm_model_checkpoint_alignment_heads(self._h, a.ctypes.data_as(C.POINTER(C.c_int32)), len(a))
        return [(int(l), int(h)) for l, h in a[:min(n, len(a))]]

    def last_token_times(self) -> List[List[Tuple[float, float]]]:
        """(start, end) in seconds from the start of its slice for every token of the last transcribe call, grouped like
        its segments; [] with alignment off"""
        cap = 64 * (self._ctx_len + 2)
        s, e = np.zeros(cap, dtype=np.float32), np.zeros(cap, dtype=np.float32)
        fp = C.POINTER(C.c_float)
        n = _lib().nm_model_last_token_times(self._h, s.ctypes.data_as(fp), e.ctypes.data_as(fp), cap)
        if n == 0:
            return []
        out, i = [], 0
        for seg in self._last_segments:
            out.append([(float(s[i + k]), float(e[i + k])) for k in range(len(seg))])
            i += len(seg)
        return out

    @property
    def language_token(self) -> int:
        return int(_lib().nm_model_language_token(self._h))

    def last_text(self) -> str:
        """Concatenated text of the last transcribe call (needs a model loaded with a tokenizer)."""
        n = _lib().nm_model_last_text(self._h, None, 0)
        buf = C.create_string_buffer(n + 1)
        _lib().nm_model_last_text(self._h, buf, n + 1)
        return buf.value.decode("utf-8", errors="replace")

    def last_result(self) -> dict:
        a, n, f, k = C.c_double(0), C.c_double(0), C.c_int(0), C.c_int(0)
        _lib().nm_model_last_result(self._h, C.byref(a), C.byref(n), C.byref(f), C.byref(k))
        return dict(avg_logprob=a.value, no_speech_prob=n.value, needed_fallback=bool(f.value), n_tokens=k.value,
                    loop_exit=bool(_lib().nm_model_last_loop_exit(self._h)))


class Resampler:
    """norma::Resampler on a model's context: the streaming form of HipWhisper.resample.  push(frames, final) returns the
    16 kHz samples that have become computable; over a stream they are those of one resample of the whole of it."""

    def __init__(self, model: Model, src_hz: int, channels: int, dtype):
        self._channels, self._dtype = int(channels), np.dtype(dtype)
        self._model = model   # the resampler runs on the model's context: keep it alive
        self._h = _lib().nm_resampler_new(model._h, int(src_hz), int(channels), hip.SAMPLE_DTYPES[self._dtype])
        if not self._h:
            raise WhisperError("nm_resampler_new failed")

    def close(self):
        if self._h:
            _lib().nm_resampler_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def push(self, frames: np.ndarray, final: bool = False) -> np.ndarray:
        a = _native_frames(np.asarray(frames, dtype=self._dtype), self._channels)
        err = C.create_string_buffer(512)
        n = _lib().nm_resampler_push(self._h, a.ctypes.data_as(C.c_void_p), a.shape[0], int(final), err, 512)
        if n < 0:
            raise WhisperError(err.value.decode())
        out = np.zeros(n, dtype=np.float32)
        _lib().nm_resampler_read(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), n)
        return out

    def state(self) -> dict:
        v = [C.c_int64(0) for _ in range(3)]
        _lib().nm_resampler_state(self._h, *[C.byref(x) for x in v])
        return dict(received=int(v[0].value), emitted=int(v[1].value), kept=int(v[2].value))


def gguf_list(path: str):
    """Tensors of a GGUF file as the C++ reader sees them: [(name, ggml_type, shape, sum of dequantised values)]."""
    _lib()
    buf = C.create_string_buffer(1 << 20)
    n = _lib().nm_gguf_list(path.encode(), buf, len(buf))
    if n < 0:
        raise WhisperError(buf.value.decode())
    out = []
    for line in buf.value.decode().splitlines():
        name, ty, shape, s = line.split(" ")
        out.append((name, int(ty), tuple(int(x) for x in shape.split("x")), float(s)))
    return out


class Definition:
    """whisper::monolingual::Definition (monolingual.rs:113-174)."""

    def __init__(self, model: ModelType, device: SelectedDevice):
        self.model, self.device = model, device
        self._h = _lib().nm_definition_new(int(model), device.kind, device.ordinal)

    def __del__(self):
        try:
            if self._h:
                _lib().nm_definition_free(self._h)
                self._h = None
        except Exception:
            pass

    def _model(self, h, ctx_len: int) -> Model:
        m = Model(C.c_void_p(h), ctx_len)
        m._channels = getattr(self, "_channels", 1)
        return m

    def set_responsiveness(self, period_ms: int):
        if _lib().nm_definition_set_responsiveness(self._h, period_ms):
            raise WhisperError("The respnsivness must be over 1 second and under 30")

    def set_data_buffer_size(self, n: int):
        _lib().nm_definition_set_data_buffer_size(self._h, n)

    def set_input_format(self, src_hz: int, channels: int):
        """what the capture device delivers to Model.transcribe_frames (default 16 000 Hz mono); applies to the models made
        from this definition afterwards"""
        _lib().nm_definition_set_input_format(self._h, int(src_hz), int(channels))
        self._channels = int(channels)

    @property
    def max_chunk_len(self) -> int:
        return int(_lib().nm_definition_max_chunk_len(self._h))

    @property
    def data_buffer_size(self) -> int:
        return int(_lib().nm_definition_data_buffer_size(self._h))

    def blocking_try_to_model_from_dir(self, path: str, language: Optional[str] = "<|en|>", translate: bool = False,
                                       ctx_len: int = 448) -> Model:
        """Load config.json / tokenizer.json / model.safetensors from a local directory (the files the reference
        fetches through hf-hub, monolingual.rs:323-345).  language=None: multilingual Definition, the language is
        detected (multilingual.rs:463-466)."""
        import json
        ext = QUANTIZED_EXT.get(self.model)   # quantised checkpoints: config-{ext}.json, tokenizer-{ext}.json, model-{ext}-q80.gguf
        with open(os.path.join(path, f"config-{ext}.json" if ext else "config.json")) as f:
            n_mel = json.load(f)["num_mel_bins"]
        filt = np.ascontiguousarray(assets_io.mel_filters(n_mel), dtype=np.float32)
        err = C.create_string_buffer(512)
        h = _lib().nm_definition_blocking_try_to_model_from_dir(self._h, path.encode(), filt.ctypes.data_as(C.POINTER(C.c_float)),
                                                                filt.shape[0], (language or "").encode(), int(translate), err, 512)
        if not h:
            raise WhisperError(err.value.decode())
        return self._model(h, ctx_len)

    def blocking_try_to_model(self, cfg: Config, tokens, lang: int, task: int,
                              weights: Iterable[Tuple[str, np.ndarray]], mel_filters: Optional[np.ndarray] = None) -> Model:
        """ModelDefinition::blocking_try_to_model (monolingual.rs:320-451) with local pieces instead of hf-hub."""
        L = _lib()
        c = hip.NhConfig(cfg.num_mel_bins, cfg.max_source_positions, cfg.d_model, cfg.encoder_attention_heads,
                         cfg.encoder_layers, cfg.vocab_size, cfg.max_target_positions, cfg.decoder_attention_heads,
                         cfg.decoder_layers)
        tk = hip.NhTokens(tokens.sot, tokens.eot, lang, task, tokens.no_speech, tokens.no_timestamps, tokens.zero_sec,
                          tokens.one_sec)
        sup = np.asarray(cfg.suppress_tokens, dtype=np.int32)
        filt = np.ascontiguousarray(assets_io.mel_filters(cfg.num_mel_bins) if mel_filters is None else mel_filters,
                                    dtype=np.float32)
        tl = L.nm_tensors_new()
        keep = []
        try:
            for name, arr in weights:
                arr = np.ascontiguousarray(arr)
                dt = hip.NH_DTYPE_F16 if arr.dtype == np.float16 else hip.NH_DTYPE_F32
                if dt == hip.NH_DTYPE_F32:
                    arr = np.ascontiguousarray(arr, dtype=np.float32)
                keep.append(arr)
                shape = (C.c_int64 * arr.ndim)(*arr.shape)
                L.nm_tensors_add(tl, name.encode(), dt, shape, arr.ndim, arr.ctypes.data_as(C.c_void_p))
            err = C.create_string_buffer(512)
            h = L.nm_definition_blocking_try_to_model(self._h, C.byref(c), C.byref(tk),
                                                      sup.ctypes.data_as(C.POINTER(C.c_int32)), len(sup),
                                                      filt.ctypes.data_as(C.POINTER(C.c_float)), filt.shape[0], tl, err, 512)
            if not h:
                raise WhisperError(err.value.decode())
            return self._model(h, cfg.max_target_positions)
        finally:
            L.nm_tensors_free(tl)
