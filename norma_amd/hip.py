"""ctypes binding of libnorma_hip.so (include/norma_hip.h) -- the only way Python reaches the HIP path.

There is deliberately no CPU fallback here: if the shared library is missing or no MI355X is
visible, construction fails loudly (the reference's `SelectedDevice::Cuda(n)` fails the same way
when candle cannot open the device, `src/models/mod.rs:47-55`).
"""
import ctypes as C
import os
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import cabi
from .config import Config

_HERE = os.path.dirname(os.path.abspath(__file__))
# NORMA_HIP_LIB selects another BUILD of the same HIP library (libnorma_hip_strict.so: -DNH_STRICT_MEMORY_MODEL); there is no
# other implementation to select
LIB_PATH = os.environ.get("NORMA_HIP_LIB") or os.path.join(_HERE, "libnorma_hip.so")
STRICT_LIB_PATH = os.path.join(_HERE, "libnorma_hip_strict.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "norma_hip.h")
# the decode pool's extensions to that ABI (nh_pool_prefix): a header of its own that includes the first, same library (the
# first header's prototype list is pinned by tests/test_cabi_cpu.py; why, in full: the top of norma_hip_pool.h)
POOL_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "norma_hip_pool.h")

_H = cabi.read(HEADER_PATH)
# every integer #define of the header under its own name: NH_OPT_*, NH_DTYPE_*, NH_SAMPLE_*, NH_ERR_*, NH_LANG_DETECT, NH_CUT_HOP, ...
globals().update(_H.constants)
N_SAMPLES, N_FRAMES = NH_N_SAMPLES, NH_N_FRAMES
# the NH_SAMPLE_* code of each numpy dtype (the types of src/dtype.rs)
SAMPLE_DTYPES = {np.dtype(t): _H.constants["NH_SAMPLE_" + s] for s, t in (
    ("F32", np.float32), ("F64", np.float64), ("I8", np.int8), ("I16", np.int16), ("I32", np.int32), ("I64", np.int64),
    ("U8", np.uint8), ("U16", np.uint16), ("U32", np.uint32), ("U64", np.uint64))}


class HipError(RuntimeError):
    """A non-zero status from the C ABI (message = nh_last_error)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"norma_hip status {code}: {msg}")
        self.code = code


# the header's structs, fields in the header's names and order
NhConfig, NhTokens, NhDecodeResult, NhAlignHead = (_H.structs[n] for n in ("nh_config", "nh_tokens", "nh_decode_result", "nh_align_head"))
# nh_cut_params: analysis frames of 160 samples (nh_cut_plan), defaults {3000, 2000, 15}; nh_vad_params (nh_vad_plan): the same,
# then the levels' ranks and ratios, then the shaping in frames, defaults {3000, 2000, 15, 100, 900, 4.0, 0.01, 0.0, 10, 20, 100};
# nh_guard_params (nh_set_guard): {0, 1.0, 0, 0, 0} is off
NhCutParams, NhVadParams, NhGuardParams, NhTimings = (_H.structs[n] for n in ("nh_cut_params", "nh_vad_params", "nh_guard_params", "nh_timings"))


def _vad_params_of(cls, params):
    """an NhVadParams as is, or a tuple in field order"""
    if isinstance(params, cls):
        return params
    return cls(*[(float if t is C.c_float else int)(x) for x, (_, t) in zip(params, cls._fields_)])


NhVadParams.of = classmethod(_vad_params_of)

# PCM the header types `const float *` that may live in device memory: callers hand these over as bare addresses (c_void_p).
# The one list kept by hand beside the header: a new entry point that takes host-or-device PCM needs its line here, and says
# so itself if it is forgotten -- its first call with a c_void_p raises ctypes.ArgumentError, nothing is passed wrongly.
_ADDRESSES = {"nh_logmel_device": ("pcm_dev",), "nh_logmel_device_rows": ("pcm_dev",), "nh_transcribe_batch": ("pcm_dev",),
              "nh_cut_plan": ("pcm",), "nh_logmel_chunks_rows": ("pcm",), "nh_vad_plan": ("pcm",), "nh_logmel_pieces_rows": ("pcm",)}


def declared_symbols() -> List[str]:
    """Every function include/norma_hip.h declares (used by the CPU-side ABI test)."""
    return sorted(_H.prototypes)


def pool_declared_symbols() -> List[str]:
    """Every function include/norma_hip_pool.h declares on top of those"""
    return sorted(cabi.read(POOL_HEADER_PATH).prototypes)


_lib = None


def load_library() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  norma_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    cabi.bind(L, HEADER_PATH, _ADDRESSES)
    cabi.bind(L, POOL_HEADER_PATH)
    _lib = L
    return L


def device_count() -> int:
    return int(load_library().nh_device_count())


class DeviceBuffer:
    """The bytes of a numpy array in HBM, for the entry points that take a device pointer (logmel_device, resample, ...):
    hipMalloc + hipMemcpy of the HIP runtime libnorma_hip.so itself is linked to.  `.ptr` is the device address; free() or the
    garbage collector releases it."""

    _rt = None

    @classmethod
    def runtime(cls) -> C.CDLL:
        if cls._rt is None:
            load_library()
            path = "libamdhip64.so"
            with open("/proc/self/maps") as f:   # the copy already in this process, not whichever the search path finds
                for line in f:
                    if "libamdhip64" in line:
                        path = line.split()[-1]
                        break
            rt = C.CDLL(path)
            rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            rt.hipFree.argtypes = [C.c_void_p]
            cls._rt = rt
        return cls._rt

    def __init__(self, arr: np.ndarray):
        rt = self.runtime()
        a = np.ascontiguousarray(arr)
        p = C.c_void_p()
        if rt.hipMalloc(C.byref(p), max(1, a.nbytes)) != 0:
            raise HipError(NH_ERR_NOMEM, f"hipMalloc({a.nbytes})")
        self.ptr, self.nbytes = int(p.value), a.nbytes
        if rt.hipMemcpy(C.c_void_p(self.ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, 1) != 0:   # hipMemcpyHostToDevice
            self.free()
            raise HipError(NH_ERR_HIP, "hipMemcpy to the device failed")

    def free(self):
        if getattr(self, "ptr", 0):
            self._rt.hipFree(C.c_void_p(self.ptr))
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


class HipWhisper:
    """One Whisper model resident on one MI355X (one `nh_ctx`).  Not thread-safe, like the
    reference's `Model: Send` (one transcriber thread calls it, `src/lib.rs:462-464`)."""

    def __init__(self, cfg: Config, device: int = 0, max_batch: int = 1, share_with: "Optional[HipWhisper]" = None):
        """share_with: another HipWhisper on the same device whose WEIGHTS (and mel filters) this context uses
        (nh_create_shared); tokens, streams, workspaces and K/V caches are its own."""
        self.L = load_library()
        self.cfg = cfg
        self.max_batch = max_batch
        h = C.c_void_p()
        if share_with is not None:
            rc = self.L.nh_create_shared(share_with._h, max_batch, C.byref(h))
        else:
            c = NhConfig(cfg.num_mel_bins, cfg.max_source_positions, cfg.d_model, cfg.encoder_attention_heads,
                         cfg.encoder_layers, cfg.vocab_size, cfg.max_target_positions,
                         cfg.decoder_attention_heads, cfg.decoder_layers)
            rc = self.L.nh_create(device, C.byref(c), max_batch, C.byref(h))
        if rc != 0:
            raise HipError(rc, self.L.nh_last_error(None).decode())
        self._h = h
        self.batch = 0
        self._decoded, self._decoded_rows, self._task, self._eot = [], {}, -1, -1   # what the last decode / collects returned (align_decoded)
        self._experiment_switches()

    # -- lifetime ------------------------------------------------------------------------------
    def _experiment_switches(self):
        """NORMA_HIP_ABSORBED_XATTN=1: every context runs the NH_OPT_ABSORBED_XATTN numerics prototype (lets the whole parity suite
        be run against it: DESIGN.md 8 item 1)."""
        if os.environ.get("NORMA_HIP_ABSORBED_XATTN"):
            self.set_option(NH_OPT_ABSORBED_XATTN, int(os.environ["NORMA_HIP_ABSORBED_XATTN"]))

    def close(self):
        if getattr(self, "_h", None):
            self.L.nh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int):
        if rc != 0:
            raise HipError(rc, self.L.nh_last_error(self._h).decode())

    # -- model state ---------------------------------------------------------------------------
    def load_tensor(self, name: str, arr: np.ndarray):
        if arr.dtype == np.float16:
            dt = NH_DTYPE_F16
        else:
            arr = np.ascontiguousarray(arr, dtype=np.float32)
            dt = NH_DTYPE_F32
        arr = np.ascontiguousarray(arr)
        shape = (C.c_int64 * arr.ndim)(*arr.shape)
        self._chk(self.L.nh_load_tensor(self._h, name.encode(), dt, shape, arr.ndim, arr.ctypes.data_as(C.c_void_p)))

    def load_weights(self, weights: Iterable[Tuple[str, np.ndarray]]):
        for name, arr in weights:
            self.load_tensor(name, arr)
        missing = self.L.nh_missing_tensors(self._h)
        if missing:
            raise HipError(NH_ERR_STATE, f"{missing} tensors missing after load_weights")

    def set_mel_filters(self, filters: np.ndarray):
        f = np.ascontiguousarray(filters, dtype=np.float32)
        self._chk(self.L.nh_set_mel_filters(self._h, _fp(f), f.shape[0]))

    def set_tokens(self, tokens, lang: int, task: int, suppress: Optional[Sequence[int]] = None):
        tk = NhTokens(tokens.sot, tokens.eot, lang, task, tokens.no_speech, tokens.no_timestamps,
                      tokens.zero_sec, tokens.one_sec)
        sup = np.asarray(self.cfg.suppress_tokens if suppress is None else suppress, dtype=np.int32)
        self._chk(self.L.nh_set_tokens(self._h, C.byref(tk), _ip(sup), len(sup)))
        self._task, self._eot = int(task), int(tokens.eot)

    # -- hot path ------------------------------------------------------------------------------
    def logmel(self, clips: Sequence[np.ndarray]):
        """clips: list of f32 PCM arrays (each <= 480000 samples)."""
        B = len(clips)
        ns = np.array([len(c) for c in clips], dtype=np.int32)
        stride = int(max(ns.max(), 1))
        buf = np.zeros((B, stride), dtype=np.float32)
        for b, c in enumerate(clips):
            buf[b, :len(c)] = c
        self._chk(self.L.nh_logmel(self._h, _fp(buf), _ip(ns), stride, B))
        self.batch = B

    def _filled(self, row0: int, n: int):
        """what an accepted nh_logmel*_rows call leaves as the context's batch (commit_batch of nh_encode.hip): row 0 starts a
        batch, higher rows join one -- and refilling rows in its middle does not shorten it"""
        self.batch = max(self.batch, row0 + n) if row0 > 0 else n

    @staticmethod
    def _lens(given: Optional[Sequence[int]], n: int, whole: int) -> np.ndarray:
        """i32 [n]: the clips' lengths as given, or `whole` for each"""
        return np.full(n, whole, dtype=np.int32) if given is None else np.ascontiguousarray(given, dtype=np.int32)

    def logmel_array(self, pcm: np.ndarray, n_samples: Optional[Sequence[int]] = None):
        """pcm: contiguous f32 [batch][stride] in HOST memory, handed to nh_logmel as is (no staging copy here)."""
        assert pcm.dtype == np.float32 and pcm.ndim == 2 and pcm.flags.c_contiguous
        B, stride = pcm.shape
        ns = self._lens(n_samples, B, stride)
        self._chk(self.L.nh_logmel(self._h, _fp(pcm), _ip(ns), stride, B))
        self.batch = B

    def logmel_samples(self, pcm: np.ndarray, n_samples: Optional[Sequence[int]] = None):
        """pcm: contiguous [batch][stride] array of a native capture type (src/dtype.rs: u8 .. f64); converted to f32 on the
        GPU with dasp_sample's formulas (nh_logmel_samples)."""
        assert pcm.ndim == 2 and pcm.flags.c_contiguous and pcm.dtype in SAMPLE_DTYPES
        B, stride = pcm.shape
        ns = self._lens(n_samples, B, stride)
        self._chk(self.L.nh_logmel_samples(self._h, pcm.ctypes.data_as(C.c_void_p), SAMPLE_DTYPES[pcm.dtype], _ip(ns), stride, B))
        self.batch = B

    # -- audio ingest (include/norma_hip.h: nh_resample*): native interleaved frames at any rate -> 16 kHz mono on the device
    def _frames(self, frames, n_frames, stride_frames, dtype, channels):
        """(pointer, on_device, NH_SAMPLE_*, channels, n_frames i32 [B], stride in frames, keep-alive) of either a numpy
        array [B][frames][channels] / [B][frames] (mono), or a device pointer with dtype, channels, n_frames and stride given"""
        if isinstance(frames, np.ndarray):
            assert frames.ndim in (2, 3) and frames.dtype in SAMPLE_DTYPES
            a = np.ascontiguousarray(frames)
            ch = 1 if a.ndim == 2 else a.shape[2]
            nf = self._lens(n_frames, a.shape[0], a.shape[1])
            assert len(nf) == a.shape[0]
            return a.ctypes.data_as(C.c_void_p), 0, SAMPLE_DTYPES[a.dtype], ch, nf, a.shape[1], a
        nf = np.ascontiguousarray(n_frames, dtype=np.int32)
        return C.c_void_p(int(frames)), 1, SAMPLE_DTYPES[np.dtype(dtype)], int(channels), nf, int(stride_frames), None

    def resample_table(self, src_hz: int):
        """(coef f32 [L][T], L, M, T): the filter of src_hz as the device holds it (nh_resample_table)"""
        L_, M_, T_ = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._chk(self.L.nh_resample_table(self._h, int(src_hz), None, C.byref(L_), C.byref(M_), C.byref(T_)))
        coef = np.zeros((L_.value, T_.value), dtype=np.float32)
        if coef.size:
            self._chk(self.L.nh_resample_table(self._h, int(src_hz), _fp(coef), C.byref(L_), C.byref(M_), C.byref(T_)))
        return coef, L_.value, M_.value, T_.value

    def resample(self, frames, src_hz: int, n_frames: Optional[Sequence[int]] = None, num0: Optional[Sequence[int]] = None,
                 n_out: Optional[Sequence[int]] = None, stride_frames: int = 0, dtype=None, channels: int = 1) -> List[np.ndarray]:
        """nh_resample: the clips of `frames` (see _frames) mixed down and resampled to 16 kHz; returns one f32 array per clip.
        num0 / n_out: per-clip start position (units of 1/L frame) and output count, None = whole clips."""
        ptr, dev, dt, ch, nf, stride, keep = self._frames(frames, n_frames, stride_frames, dtype, channels)
        B = len(nf)
        z = None if num0 is None else np.ascontiguousarray(num0, dtype=np.int64)
        no = None if n_out is None else np.ascontiguousarray(n_out, dtype=np.int32)
        lens = [int(x) if 1 <= int(x) <= N_SAMPLES else 0 for x in no] if no is not None else \
               [max(0, self.L.nh_resample_len(int(src_hz), int(x))) for x in nf]
        out = np.zeros((B, max(1, max(lens, default=1))), dtype=np.float32)
        self._chk(self.L.nh_resample(self._h, ptr, dev, dt, ch, int(src_hz), _ip(nf), stride, B,
                                     None if z is None else z.ctypes.data_as(C.POINTER(C.c_int64)), None if no is None else _ip(no),
                                     _fp(out), out.shape[1]))
        return [out[b, :lens[b]].copy() for b in range(B)]

    def logmel_resampled_rows(self, frames, src_hz: int, row0: int, n_frames: Optional[Sequence[int]] = None,
                              stride_frames: int = 0, dtype=None, channels: int = 1):
        """nh_logmel_resampled_rows: whole clips of native frames -> 16 kHz mono -> log-mel of rows [row0, row0 + B)"""
        ptr, dev, dt, ch, nf, stride, keep = self._frames(frames, n_frames, stride_frames, dtype, channels)
        self._chk(self.L.nh_logmel_resampled_rows(self._h, ptr, dev, dt, ch, int(src_hz), _ip(nf), stride, len(nf), int(row0)))
        self._filled(row0, len(nf))

    def logmel_resampled(self, frames, src_hz: int, n_frames: Optional[Sequence[int]] = None, stride_frames: int = 0,
                         dtype=None, channels: int = 1):
        """the plain batch: logmel_resampled_rows with row0 = 0"""
        self.logmel_resampled_rows(frames, src_hz, 0, n_frames, stride_frames, dtype, channels)

    # -- long recordings (include/norma_hip.h: nh_cut_plan, nh_logmel_chunks_rows): cut at the quietest frame, on the device
    @staticmethod
    def _recording(pcm, n_samples):
        """(pointer, on_device, samples, keep-alive) of a host f32 array or of a device pointer with n_samples given"""
        if isinstance(pcm, np.ndarray):
            a = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1)
            return a.ctypes.data_as(C.c_void_p), 0, len(a) if n_samples is None else int(n_samples), a
        return C.c_void_p(int(pcm)), 1, int(n_samples), None

    def cut_plan(self, pcm, n_samples: Optional[int] = None, params=None):
        """nh_cut_plan: (starts i64 [n], lens i32 [n]) of the chunks of a 16 kHz mono recording -- a host f32 array, or a
        device pointer with n_samples.  params: None (the defaults {3000, 2000, 15}), an NhCutParams, or a tuple
        (max_frames, min_frames, half_window)."""
        ptr, dev, n, keep = self._recording(pcm, n_samples)
        q = None if params is None else params if isinstance(params, NhCutParams) else NhCutParams(*[int(v) for v in params])
        cap = self._plan_cap(n, q)
        while True:
            starts, lens, cnt = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int32), C.c_int32(0)
            rc = self.L.nh_cut_plan(self._h, ptr, dev, n, None if q is None else C.byref(q),
                                    starts.ctypes.data_as(C.POINTER(C.c_int64)), _ip(lens), cap, C.byref(cnt))
            if rc != 0 and cnt.value > cap:   # refused for cap alone: the call says how many there are
                cap = int(cnt.value)
                continue
            self._chk(rc)
            self._cut_frames = -(-n // NH_CUT_HOP)
            return starts[:cnt.value].copy(), lens[:cnt.value].copy()

    @staticmethod
    def _plan_cap(n: int, q) -> int:
        """room for the records of a plan over n samples that is right unless the cuts fall early: two per max_frames
        (q: the plan's parameters or None, the defaults); a plan that needs more says so and runs again (cut_plan, vad_plan)"""
        return max(4, 2 * (n // (NH_CUT_HOP * (q.max_frames if q is not None and q.max_frames > 0 else N_FRAMES))) + 2)

    def cut_energy(self):
        """(e, E) f32 [F] of the last cut_plan: frame and window energies (nh_cut_energy)"""
        F = getattr(self, "_cut_frames", 0)
        e, E = np.zeros(F, dtype=np.float32), np.zeros(F, dtype=np.float32)
        self._chk(self.L.nh_cut_energy(self._h, _fp(e), _fp(E), F))
        return e, E

    def logmel_chunks_rows(self, pcm, starts: Sequence[int], lens: Sequence[int], row0: int = 0):
        """nh_logmel_chunks_rows: clips pcm[starts[b] : starts[b] + lens[b]] of a recording (host f32 array or device
        pointer) -> log-mel of rows [row0, row0 + len(starts))"""
        ptr, dev, _, keep = self._recording(pcm, 0)
        st = np.ascontiguousarray(starts, dtype=np.int64)
        ns = np.ascontiguousarray(lens, dtype=np.int32)
        assert len(st) == len(ns)
        if keep is not None and len(st):
            assert int(st.min()) >= 0 and int((st + ns).max()) <= len(keep), "a clip leaves the recording"
        self._chk(self.L.nh_logmel_chunks_rows(self._h, ptr, dev, st.ctypes.data_as(C.POINTER(C.c_int64)), _ip(ns), len(ns), int(row0)))
        self._filled(row0, len(ns))

    # -- long recordings without their silence (include/norma_hip.h: nh_vad_plan, nh_logmel_pieces_rows)
    def vad_plan(self, pcm, n_samples: Optional[int] = None, params=None):
        """nh_vad_plan: (piece_starts i64 [n_pieces], piece_lens i32 [n_pieces], chunk_first i32 [n_chunks + 1]) of the speech
        of a 16 kHz mono recording -- a host f32 array, or a device pointer with n_samples.  params: None (the defaults), an
        NhVadParams, or a tuple in its field order."""
        ptr, dev, n, keep = self._recording(pcm, n_samples)
        q = None if params is None else NhVadParams.of(params)
        cap_p = cap_c = self._plan_cap(n, q)
        while True:
            starts, lens, first = np.zeros(cap_p, dtype=np.int64), np.zeros(cap_p, dtype=np.int32), np.zeros(cap_c + 1, dtype=np.int32)
            n_p, n_c = C.c_int32(0), C.c_int32(0)
            rc = self.L.nh_vad_plan(self._h, ptr, dev, n, None if q is None else C.byref(q), starts.ctypes.data_as(C.POINTER(C.c_int64)),
                                    _ip(lens), cap_p, C.byref(n_p), _ip(first), cap_c, C.byref(n_c))
            if rc != 0 and (n_p.value > cap_p or n_c.value > cap_c):   # refused for the caps alone: the call says what it needs
                cap_p, cap_c = max(cap_p, int(n_p.value)), max(cap_c, int(n_c.value))
                continue
            self._chk(rc)
            self._vad_frames = -(-n // NH_CUT_HOP)
            return starts[:n_p.value].copy(), lens[:n_p.value].copy(), first[:n_c.value + 1].copy()

    def vad_view(self):
        """(E f32 [F], speech u8 [F], levels f32 [3] = Q_lo, Q_hi, T, regions i64 [n][2]) of the last vad_plan (nh_vad_view)"""
        F = getattr(self, "_vad_frames", 0)
        E, speech, levels, cnt = np.zeros(F, dtype=np.float32), np.zeros(F, dtype=np.uint8), np.zeros(3, dtype=np.float32), C.c_int32(0)
        self._chk(self.L.nh_vad_view(self._h, _fp(E), speech.ctypes.data_as(C.POINTER(C.c_uint8)), F, _fp(levels), None, 0, C.byref(cnt)))
        regions = np.zeros((cnt.value, 2), dtype=np.int64)
        self._chk(self.L.nh_vad_view(self._h, None, None, 0, None, regions.ctypes.data_as(C.POINTER(C.c_int64)), cnt.value, None))
        return E, speech, levels, regions

    def logmel_pieces_rows(self, pcm, piece_starts: Sequence[int], piece_lens: Sequence[int], chunk_first: Sequence[int], row0: int = 0):
        """nh_logmel_pieces_rows: row row0 + b = the concatenation of the pieces chunk_first[b] .. chunk_first[b + 1] - 1 of a
        recording (host f32 array or device pointer) -> log-mel of rows [row0, row0 + len(chunk_first) - 1).  chunk_first may be
        a slice of a plan's: the pieces it names are rebased here."""
        ptr, dev, _, keep = self._recording(pcm, 0)
        cf = np.ascontiguousarray(chunk_first, dtype=np.int32)
        assert len(cf) >= 2, "chunk_first holds batch + 1 entries"
        j0, j1 = int(cf[0]), int(cf[-1])
        st = np.ascontiguousarray(np.asarray(piece_starts, dtype=np.int64)[j0:j1])
        ns = np.ascontiguousarray(np.asarray(piece_lens, dtype=np.int32)[j0:j1])
        cf = cf - np.int32(j0)
        assert len(st) == len(ns) == j1 - j0, "chunk_first names pieces that are not there"
        if keep is not None and len(st):
            assert int(st.min()) >= 0 and int((st + ns).max()) <= len(keep), "a piece leaves the recording"
        self._chk(self.L.nh_logmel_pieces_rows(self._h, ptr, dev, st.ctypes.data_as(C.POINTER(C.c_int64)), _ip(ns), _ip(cf), len(cf) - 1, int(row0)))
        self._filled(row0, len(cf) - 1)

    def logmel_device(self, pcm_dev_ptr: int, n_samples: Sequence[int], stride: int):
        """PCM already resident in HBM (device pointer, f32 [batch][stride])."""
        ns = np.asarray(n_samples, dtype=np.int32)
        self._chk(self.L.nh_logmel_device(self._h, C.c_void_p(pcm_dev_ptr), _ip(ns), stride, len(ns)))
        self.batch = len(ns)

    def logmel_device_rows(self, pcm_dev_ptr: int, n_samples: Sequence[int], stride: int, row0: int):
        """Clips for rows [row0, row0 + len(n_samples)) of the context (several encoder batches, one joint decode)."""
        ns = np.asarray(n_samples, dtype=np.int32)
        self._chk(self.L.nh_logmel_device_rows(self._h, C.c_void_p(pcm_dev_ptr), _ip(ns), stride, len(ns), row0))
        self._filled(row0, len(ns))

    def logmel_array_rows(self, pcm: np.ndarray, row0: int):
        """pcm: contiguous f32 [batch][stride] in HOST memory -> rows [row0, row0 + batch)."""
        assert pcm.dtype == np.float32 and pcm.ndim == 2 and pcm.flags.c_contiguous
        B, stride = pcm.shape
        self._chk(self.L.nh_logmel_rows(self._h, _fp(pcm), _ip(self._lens(None, B, stride)), stride, B, row0))
        self._filled(row0, B)

    def encode_rows(self, row0: int, batch: int):
        self._chk(self.L.nh_encode_rows(self._h, row0, batch))

    # ---- decode pool (include/norma_hip.h: nh_pool_*): rows [0, rows) decode at their own positions, the rows above stage
    # encoder output; norma_amd/pool.py holds the refill policy
    def pool_begin(self, rows: int, max_new_tokens: int = 0, per_clip_language: bool = False):
        self._chk(self.L.nh_pool_begin(self._h, rows, max_new_tokens, int(per_clip_language)))
        self.pool_rows = self.batch = rows   # nh_pool_begin: the rows filled so far are the pool's; staging rows join above them
        self._decoded_rows = {}

    def pool_admit(self, src_row: int, dst_row: int, lang: int = -1):
        self._chk(self.L.nh_pool_admit(self._h, src_row, dst_row, lang))

    def pool_admit_from(self, enc: "HipWhisper", src_row: int, dst_row: int, lang: int = -1):
        """the clip encoded in row src_row of ANOTHER context of the same weight set joins this context's pool"""
        self._chk(self.L.nh_pool_admit_from(self._h, enc._h, src_row, dst_row, lang))

    def pool_step(self, n_steps: int) -> np.ndarray:
        """n_steps tokens for every busy row; returns the rows' flags (0 running, 1 finished, 2 no-speech exit, 3 empty)."""
        done = np.zeros(self.pool_rows, dtype=np.int32)
        self._chk(self.L.nh_pool_step(self._h, n_steps, _ip(done)))
        return done

    def pool_collect(self, rows: Sequence[int]) -> List[dict]:
        rows = np.asarray(rows, dtype=np.int32)
        toks, res = self._decode_out(len(rows))
        self._chk(self.L.nh_pool_collect(self._h, _ip(rows), len(rows), _ip(toks), res))
        seqs, out = self._sequences(toks, res)
        self._decoded_rows.update(zip(rows.tolist(), seqs))
        return out

    def pool_retry(self, row: int, temperature: float, seed: int, clip: int, attempt: int):
        """the clip that row `row` last decoded (collected, not refilled since) decodes again, sampled at `temperature` under
        the seeded contract of decode_sampled with this clip id and attempt; the row is busy again"""
        self._chk(self.L.nh_pool_retry(self._h, int(row), float(temperature), int(seed), int(clip), int(attempt)))

    def pool_prefix(self, row: int, ids: Optional[Sequence[int]]):
        """nh_pool_prefix (include/norma_hip_pool.h): the token ids (taken verbatim) that the next admission into the free row `row` puts in front of
        [sot, lang?, task]; one-shot; None or an empty list clears the row's pending prefix.  The row's result excludes them."""
        a = np.ascontiguousarray(ids if ids is not None else [], dtype=np.int32).reshape(-1)
        self._chk(self.L.nh_pool_prefix(self._h, int(row), _ip(a) if len(a) else None, len(a)))

    def pool_detect_languages(self, lang_tokens: Sequence[int]):
        """the pool's language table (Language::iter() order), after pool_begin(per_clip_language=True) and while no row is
        busy: clips admitted with lang = NH_LANG_DETECT detect their language in their own first decode step"""
        lt = np.ascontiguousarray(lang_tokens, dtype=np.int32)
        self._chk(self.L.nh_pool_detect_languages(self._h, _ip(lt), len(lt)))
        self.pool_lang_n = len(lt)

    def pool_languages(self, rows: Sequence[int], want_probs: bool = True):
        """(tokens, probs [len(rows)][n] or None) of rows admitted with NH_LANG_DETECT that have stepped since"""
        rows = np.asarray(rows, dtype=np.int32)
        out = np.zeros(len(rows), dtype=np.int32)
        probs = np.zeros((len(rows), getattr(self, "pool_lang_n", 0)), dtype=np.float32) if want_probs else None
        self._chk(self.L.nh_pool_languages(self._h, _ip(rows), len(rows), _ip(out), _fp(probs) if want_probs else None))
        return out.tolist(), probs

    def get_mel(self, b: int, frames: int = N_FRAMES) -> np.ndarray:
        out = np.zeros((self.cfg.num_mel_bins, frames), dtype=np.float32)
        self._chk(self.L.nh_get_mel(self._h, b, _fp(out)))
        return out

    def set_mel(self, mel: np.ndarray):
        mel = np.ascontiguousarray(mel, dtype=np.float32)
        assert mel.ndim == 3 and mel.shape[1:] == (self.cfg.num_mel_bins, N_FRAMES)
        self._chk(self.L.nh_set_mel(self._h, _fp(mel), mel.shape[0]))
        self.batch = mel.shape[0]

    def encode(self):
        self._chk(self.L.nh_encode(self._h))

    def encoder_output(self, b: int, S: int = 1500) -> np.ndarray:
        out = np.zeros((S, self.cfg.d_model), dtype=np.float32)
        self._chk(self.L.nh_encoder_output(self._h, b, _fp(out)))
        return out

    def _decode_out(self, n: int):
        """(tokens i32 [n][max_target_positions], nh_decode_result [n]) for a decode or a collect of n rows to fill"""
        return np.zeros((n, self.cfg.max_target_positions), dtype=np.int32), (NhDecodeResult * n)()

    @staticmethod
    def _sequences(toks: np.ndarray, res):
        """per row of a filled _decode_out: (n_tokens, no-speech exit, tokens[1]), what align_decoded aligns afterwards, and the
        dict the decodes and pool_collect return"""
        seqs = [(int(r.n_tokens), bool(r.no_speech_exit), int(t[1])) for t, r in zip(toks, res)]
        return seqs, [dict(tokens=t[:r.n_tokens].tolist(), avg_logprob=r.avg_logprob, no_speech_prob=r.no_speech_prob,
                           no_speech_exit=bool(r.no_speech_exit)) for t, r in zip(toks, res)]

    def _results(self, toks: np.ndarray, res) -> List[dict]:
        """the dicts of a lockstep decode, whose sequences align_decoded aligns from now on"""
        self._decoded, out = self._sequences(toks, res)
        return out

    def _decode(self, fn, *args) -> List[dict]:
        """fn(ctx, out_tokens, results, *args) on the lockstep batch"""
        toks, res = self._decode_out(self.batch)
        self._chk(fn(self._h, _ip(toks), res, *args))
        return self._results(toks, res)

    def decode_greedy(self, max_new_tokens: int = 0) -> List[dict]:
        return self._decode(self.L.nh_decode_greedy, max_new_tokens)

    def decode_sampled(self, temperature: float, seed: int, clip0: int = 0, attempt: int = 1,
                       max_new_tokens: int = 0) -> List[dict]:
        """Model::decode at t > 0 (model.rs:340-348) under the seeded sampling contract of include/norma_hip.h."""
        return self._decode(self.L.nh_decode_sampled, max_new_tokens, float(temperature), int(seed), int(clip0), int(attempt))

    def decode_beam(self, beam_size: int, max_new_tokens: int = 0) -> List[dict]:
        """Beam search at t = 0 (include/norma_hip.h): decode_greedy's dicts for the best hypothesis of every
        clip, plus `hypotheses`: the clip's finished list [(tokens, sum_logprob)] in finishing order, untrimmed."""
        toks, res = self._decode_out(self.batch)
        self._chk(self.L.nh_decode_beam(self._h, int(beam_size), _ip(toks), res, max_new_tokens))
        out = self._results(toks, res)
        for b, o in enumerate(out):
            o["hypotheses"] = self.beam_hypotheses(b)
        return out

    def beam_hypotheses(self, b: int) -> List[Tuple[List[int], float]]:
        """The finished list of clip b from the last beam decode (nh_beam_hypotheses).  The library writes one row per beam of
        that decode, so the arrays hold NH_MAX_BEAMS rows whatever its beam size was."""
        Cn = self.cfg.max_target_positions
        ft = np.zeros((NH_MAX_BEAMS, Cn), dtype=np.int32)
        fn = np.zeros(NH_MAX_BEAMS, dtype=np.int32)
        fs = np.zeros(NH_MAX_BEAMS, dtype=np.float64)
        nf = C.c_int32(0)
        self._chk(self.L.nh_beam_hypotheses(self._h, int(b), _ip(ft), _ip(fn), fs.ctypes.data_as(C.POINTER(C.c_double)), C.byref(nf)))
        return [(ft[f, :fn[f]].tolist(), float(fs[f])) for f in range(nf.value)]

    def beam_step(self, beam_size: int, batch: int, logits: np.ndarray, state: dict, n_finished: Sequence[int],
                  max_new_tokens: int = 0, prompt_len: int = 3) -> dict:
        """One beam step on given logits f32 [K*B][V] and hypothesis state (parity view nh_beam_step).  state: tokens
        [K*B][C], n_tokens, have_last, last_ts, live, score per row.  Returns the new state, parent, n_finished and the
        newly finished records per clip [(tokens, sum_logprob)]."""
        K, B, Cn = int(beam_size), int(batch), self.cfg.max_target_positions
        R = K * B
        lg = np.ascontiguousarray(logits, dtype=np.float32).reshape(R, self.cfg.vocab_size)
        i32 = lambda k: np.ascontiguousarray(np.array(state[k], dtype=np.int32).reshape(R, -1))
        toks = np.ascontiguousarray(np.array(state["tokens"], dtype=np.int32).reshape(R, Cn))
        nt, hl, lt, lv = i32("n_tokens"), i32("have_last"), i32("last_ts"), i32("live")
        sc = np.ascontiguousarray(np.array(state["score"], dtype=np.float64).reshape(R))
        nf_in = np.array(n_finished, dtype=np.int32).reshape(B)
        nf = nf_in.copy()
        par = np.zeros(R, dtype=np.int32)
        ft = np.zeros((B, K, Cn), dtype=np.int32)
        fn = np.zeros((B, K), dtype=np.int32)
        fs = np.zeros((B, K), dtype=np.float64)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        self._chk(self.L.nh_beam_step(self._h, K, B, _fp(lg), _ip(toks), _ip(nt), _ip(hl), _ip(lt), _ip(lv), dp(sc), int(max_new_tokens),
                                      int(prompt_len), _ip(par), _ip(nf), _ip(ft), _ip(fn), dp(fs)))
        fin = [[(ft[b, f, :fn[b, f]].tolist(), float(fs[b, f])) for f in range(int(nf_in[b]), int(nf[b]))] for b in range(B)]
        return dict(tokens=toks, n_tokens=nt.reshape(R), have_last=hl.reshape(R), last_ts=lt.reshape(R), live=lv.reshape(R),
                    score=sc, parent=par, n_finished=nf, finished=fin, fin_raw=(ft, fn, fs))

    def beam_reorder(self, beam_size: int, batch: int, parent: Sequence[int], n_pos: int, layer: int, which: int,
                     cache: np.ndarray) -> np.ndarray:
        """The self-attention cache reorder of a beam step alone (nh_beam_reorder): cache fp16 [K*B][heads][C][64]."""
        R = int(beam_size) * int(batch)
        c = np.ascontiguousarray(cache, dtype=np.float16).reshape(R, self.cfg.decoder_attention_heads, self.cfg.max_target_positions, 64).copy()
        par = np.array(parent, dtype=np.int32).reshape(R)
        self._chk(self.L.nh_beam_reorder(self._h, int(beam_size), int(batch), _ip(par), int(n_pos), int(layer), int(which),
                                         c.view(np.uint16).ctypes.data_as(C.POINTER(C.c_uint16))))
        return c

    # ---- repetition guard (include/norma_hip.h: nh_set_guard ...) ----
    def set_guard(self, no_repeat_ngram: int = 0, repetition_penalty: float = 1.0, loop_period: int = 0, loop_repeats: int = 0,
                  bias: bool = False):
        """The guard of this context's decode steps, kept until changed; set_guard(None) or no arguments: off."""
        if no_repeat_ngram is None:
            self._chk(self.L.nh_set_guard(self._h, None))
            return
        p = NhGuardParams(int(no_repeat_ngram), float(repetition_penalty), int(loop_period), int(loop_repeats), int(bool(bias)))
        self._chk(self.L.nh_set_guard(self._h, C.byref(p)))

    def guard_bias(self, row: int, bias: Optional[dict]):
        """{token: beta} for context row `row` (applied while set_guard(bias=True)); None or {}: clear"""
        items = sorted((bias or {}).items())
        tk = np.array([k for k, _ in items], dtype=np.int32)
        bv = np.array([v for _, v in items], dtype=np.float32)
        self._chk(self.L.nh_guard_bias(self._h, int(row), _ip(tk) if len(tk) else None, _fp(bv) if len(tk) else None, len(tk)))

    def guard_report(self, rows: Optional[Sequence[int]] = None) -> List[int]:
        """loop-exit flags of the given rows (pool rows are named; None: every clip of the lockstep batch)"""
        if rows is None:
            out = np.zeros(self.batch, dtype=np.int32)
            self._chk(self.L.nh_guard_report(self._h, None, self.batch, _ip(out)))
        else:
            r = np.ascontiguousarray(rows, dtype=np.int32)
            out = np.zeros(len(r), dtype=np.int32)
            self._chk(self.L.nh_guard_report(self._h, _ip(r), len(r), _ip(out)))
        return out.tolist()

    def guard_apply(self, logits: np.ndarray, tokens: Sequence[Sequence[int]], prompt_len: int = 3,
                    active: Optional[Sequence[int]] = None, bias_rows: Optional[Sequence[int]] = None):
        """The guard's edit alone on logits f32 [rows][V] and one token list per row (parity view nh_guard_apply).  Returns
        (device rows f32 [rows][ld] with the pad columns, loop_exit [rows])."""
        lg = np.ascontiguousarray(logits, dtype=np.float32).reshape(len(tokens), self.cfg.vocab_size)
        R = lg.shape[0]
        stride = max(max(len(t) for t in tokens), 1)
        toks = np.zeros((R, stride), dtype=np.int32)
        nt = np.zeros(R, dtype=np.int32)
        for r, t in enumerate(tokens):
            toks[r, :len(t)] = t
            nt[r] = len(t)
        act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
        br = None if bias_rows is None else np.ascontiguousarray(bias_rows, dtype=np.int32)
        ld = (self.cfg.vocab_size + 63) & ~63
        out = np.zeros((R, ld), dtype=np.float32)
        le = np.zeros(R, dtype=np.int32)
        self._chk(self.L.nh_guard_apply(self._h, R, _fp(lg), _ip(toks), _ip(nt), stride, int(prompt_len),
                                        None if act is None else _ip(act), None if br is None else _ip(br), _fp(out), _ip(le)))
        return out, le

    def transcribe_batch_device(self, pcm_dev_ptr: int, n_samples: Sequence[int], stride: int,
                                max_new_tokens: int = 0) -> List[dict]:
        """pcm already resident in HBM (device pointer, f32 [batch][stride])."""
        ns = np.asarray(n_samples, dtype=np.int32)
        toks, res = self._decode_out(len(ns))
        self._chk(self.L.nh_transcribe_batch(self._h, C.c_void_p(pcm_dev_ptr), _ip(ns), stride, len(ns), _ip(toks), res,
                                             max_new_tokens))
        self.batch = len(ns)
        return self._results(toks, res)

    def detect_language(self, lang_tokens: Sequence[int], want_probs: bool = True):
        """Model::detect_language for every clip; the result also becomes the decode prompt's language token."""
        lt = np.ascontiguousarray(lang_tokens, dtype=np.int32)
        out = np.zeros(self.batch, dtype=np.int32)
        probs = np.zeros((self.batch, len(lt)), dtype=np.float32) if want_probs else None
        self._chk(self.L.nh_detect_language(self._h, _ip(lt), len(lt), _ip(out), _fp(probs) if want_probs else None))
        return out.tolist(), probs

    def set_languages(self, langs: Optional[Sequence[int]]):
        if langs is None:
            self._chk(self.L.nh_set_languages(self._h, None))
        else:
            a = np.ascontiguousarray(langs, dtype=np.int32)
            self._chk(self.L.nh_set_languages(self._h, _ip(a)))

    def set_prompts(self, prompts: Optional[Sequence[Sequence[int]]]):
        """nh_set_prompts: one list of token ids per clip of the batch, all of ONE length, put in front of [sot, lang?, task]
        by the next decode_greedy / decode_sampled (taken verbatim: <|startofprev|> first is the caller's to add); None or
        empty lists: no prefix.  The results exclude the prefix."""
        if prompts is None:
            self._chk(self.L.nh_set_prompts(self._h, None, 0, 0, self.batch))
            return
        n = len(prompts[0]) if len(prompts) else 0
        if any(len(p) != n for p in prompts):
            raise ValueError("set_prompts: one prefix length per batch (ragged prefixes are not supported)")
        a = np.ascontiguousarray(np.asarray(prompts, dtype=np.int32).reshape(len(prompts), n))
        self._chk(self.L.nh_set_prompts(self._h, _ip(a) if n else None, n, n, len(prompts)))

    def reset(self):
        self._chk(self.L.nh_reset(self._h))

    def synchronize(self):
        self._chk(self.L.nh_synchronize(self._h))

    # -- fine-grained parity views ---------------------------------------------------------------
    def _decoder_forward(self, fn, tokens: np.ndarray) -> np.ndarray:
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        B, T = tokens.shape
        assert B == self.batch
        out = np.zeros((B, T, self.cfg.d_model), dtype=np.float32)
        self._chk(fn(self._h, _ip(tokens), T, _fp(out)))
        return out

    def decoder_forward(self, tokens: np.ndarray) -> np.ndarray:
        return self._decoder_forward(self.L.nh_decoder_forward, tokens)

    def decoder_forward_onepass(self, tokens: np.ndarray) -> np.ndarray:
        """decoder_forward's contract computed in one pass over the T positions (nh_decoder_forward_onepass)"""
        return self._decoder_forward(self.L.nh_decoder_forward_onepass, tokens)

    def final_linear(self, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, self.cfg.d_model)
        out = np.zeros((x.shape[0], self.cfg.vocab_size), dtype=np.float32)
        self._chk(self.L.nh_final_linear(self._h, _fp(x), x.shape[0], _fp(out)))
        return out

    def apply_rules(self, probs: np.ndarray, tokens: Sequence[int], last_timestamp: int):
        p = np.ascontiguousarray(probs, dtype=np.float32)
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.zeros_like(p)
        am = C.c_int32(0)
        self._chk(self.L.nh_apply_rules(self._h, _fp(p), _ip(t), len(t), last_timestamp, _fp(out), C.byref(am)))
        return out, int(am.value)

    def sample_rules(self, probs: np.ndarray, tokens: Sequence[int], last_timestamp: int, temperature: float, seed: int,
                     clip: int = 0, attempt: int = 1) -> int:
        """The sampler alone: rules + one seeded draw on a soft-maxed probability vector (-1: everything masked)."""
        p = np.ascontiguousarray(probs, dtype=np.float32)
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        tok = C.c_int32(0)
        self._chk(self.L.nh_sample_rules(self._h, _fp(p), _ip(t), len(t), last_timestamp, float(temperature), int(seed),
                                         int(clip), int(attempt), C.byref(tok)))
        return int(tok.value)

    # -- token-level timestamps -------------------------------------------------------------------
    def _token_rows(self, tokens, n_tokens: Optional[Sequence[int]], whole: bool):
        """(tokens i32 [batch][max_target_positions], n_tokens i32 [batch]) of one token list per clip of the batch, or of an
        array of that shape with n_tokens.  whole: such an array goes in as given, what lies past n_tokens included; otherwise
        the rows are zero past n_tokens."""
        B, Cn = self.batch, self.cfg.max_target_positions
        if n_tokens is None:
            n_tokens = [len(t) for t in tokens]
        nt = np.ascontiguousarray(n_tokens, dtype=np.int32)
        assert len(nt) == B and len(tokens) == B
        if whole and isinstance(tokens, np.ndarray) and tokens.shape == (B, Cn):
            return np.ascontiguousarray(tokens, dtype=np.int32), nt
        toks = np.zeros((B, Cn), dtype=np.int32)
        for b in range(B):
            n = max(0, min(int(nt[b]), Cn))
            toks[b, :n] = np.asarray(tokens[b], dtype=np.int32)[:n]
        return toks, nt

    @staticmethod
    def _heads(heads: Sequence[Tuple[int, int]]):
        """nh_align_head [len(heads)] (one entry at least, so that an empty list is still a pointer)"""
        return (NhAlignHead * max(1, len(heads)))(*[NhAlignHead(int(l), int(h)) for l, h in heads])

    def align(self, tokens: Sequence[Sequence[int]], n_tokens: Optional[Sequence[int]] = None, prompt_len: int = 3,
              heads: Sequence[Tuple[int, int]] = (), n_keys: Optional[Sequence[int]] = None):
        """nh_align for every clip of the batch: tokens = the sequences as decode_* returned them (lists, or an i32 array
        [batch][max_target_positions] with n_tokens), heads = [(decoder layer, head)], n_keys = encoder frames that hold audio
        (None: all).  Returns (first, last): i32 [batch][max_target_positions], the first and last 20 ms encoder frame of every
        token, -1 for the prompt and past the end."""
        B, Cn = self.batch, self.cfg.max_target_positions
        toks, nt = self._token_rows(tokens, n_tokens, whole=False)
        hs = self._heads(heads)
        nk = None if n_keys is None else np.ascontiguousarray(n_keys, dtype=np.int32)
        assert nk is None or len(nk) == B
        first = np.full((B, Cn), -2, dtype=np.int32)
        last = np.full((B, Cn), -2, dtype=np.int32)
        self._align_out = (first, last)   # a refused call leaves them as they are (the tests look)
        self._chk(self.L.nh_align(self._h, _ip(toks), _ip(nt), int(prompt_len), hs, len(heads), None if nk is None else _ip(nk),
                                  _ip(first), _ip(last)))
        self._align_shape = (nt.copy(), int(prompt_len), np.full(B, self.cfg.max_source_positions, np.int32) if nk is None else nk.copy())
        return first, last

    # -- transcript scoring --------------------------------------------------------------------------
    def score(self, tokens: Sequence[Sequence[int]], n_tokens: Optional[Sequence[int]] = None, prompt_len: int = 3,
              out: Optional[np.ndarray] = None) -> np.ndarray:
        """nh_score for every clip of the batch: tokens = the sequences as decode_* returned them, or any others (lists, or an
        i32 array [batch][max_target_positions] with n_tokens).  Returns f32 [batch][max_target_positions]: entry i of clip b,
        prompt_len <= i < n_tokens[b], is ln p(tokens[b][i]) under the plain softmax of position i - 1; every other entry 0.
        A prefix that stood in front of sot goes in front of `tokens`, with prompt_len = len(prefix) + 2 or 3.
        out: the array to write (a refused call leaves it as it is)."""
        B, Cn = self.batch, self.cfg.max_target_positions
        toks, nt = self._token_rows(tokens, n_tokens, whole=True)
        if out is None:
            out = np.zeros((B, Cn), dtype=np.float32)
        assert out.dtype == np.float32 and out.shape == (B, Cn) and out.flags.c_contiguous
        self._chk(self.L.nh_score(self._h, _ip(toks), _ip(nt), int(prompt_len), _fp(out)))
        return out

    def align_capture(self, heads: Sequence[Tuple[int, int]]):
        """nh_align_capture: every following decode of this context (decode_greedy, decode_sampled, the rows of a pool) keeps
        the cross-attention queries of `heads` = [(decoder layer, head)] for align_decoded; [] turns it off (the default)."""
        self._chk(self.L.nh_align_capture(self._h, self._heads(heads), len(heads)))

    def align_decoded(self, rows: Optional[Sequence[int]] = None, n_keys: Optional[Sequence[int]] = None):
        """nh_align_decoded: (first, last) i32 [n][max_target_positions] of the sequences this context has just decoded, from
        the queries kept while decoding (align_capture) -- no decoder pass.  rows=None: the clips of the last lockstep decode;
        rows=[...]: pool rows that pool_collect has handed back and nothing has refilled or retried since.  The sequences are
        the ones the decode / collect returned; first / last are -1 for the prompt, past the end, and for a no-speech exit."""
        Cn = self.cfg.max_target_positions
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        n = self.batch if r is None else len(r)
        nk = None if n_keys is None else np.ascontiguousarray(n_keys, dtype=np.int32)
        assert nk is None or len(nk) == n
        first = np.full((n, Cn), -1, dtype=np.int32)
        last = np.full((n, Cn), -1, dtype=np.int32)
        self._chk(self.L.nh_align_decoded(self._h, None if r is None else _ip(r), n, None if nk is None else _ip(nk), _ip(first), _ip(last)))
        # the views' shape, from what the decode / collect returned: the prompt is [sot, task] or [sot, language, task]
        seqs = self._decoded if r is None else [self._decoded_rows[int(x)] for x in r]
        nt = np.array([0 if exit_ else n_ for n_, exit_, _ in seqs], dtype=np.int32)
        P = 2 if seqs and seqs[0][2] == self._task else 3
        self._align_shape = (nt, P, np.full(n, self.cfg.max_source_positions, np.int32) if nk is None else nk.copy())
        return first, last

    def align_weights(self, b: int, a: int) -> np.ndarray:
        """f32 [n_tokens[b] - 1][n_keys[b]]: the softmax of heads[a] of the last align (NH_OPT_ALIGN_KEEP = 1)"""
        nt, _, nk = self._align_shape
        out = np.zeros((int(nt[b]) - 1, int(nk[b])), dtype=np.float32)
        self._chk(self.L.nh_align_weights(self._h, int(b), int(a), _fp(out)))
        return out

    def align_matrix(self, b: int) -> np.ndarray:
        """f32 [n_tokens[b] - prompt_len][n_keys[b]]: the DTW input of the last align (NH_OPT_ALIGN_KEEP = 1)"""
        nt, P, nk = self._align_shape
        out = np.zeros((int(nt[b]) - P, int(nk[b])), dtype=np.float32)
        self._chk(self.L.nh_align_matrix(self._h, int(b), _fp(out)))
        return out

    def align_path(self, matrix: np.ndarray):
        """the DTW alone on a host matrix f32 [R][nk] (cost = -matrix): (first, last) i32 [R]"""
        m = np.ascontiguousarray(matrix, dtype=np.float32)
        R, nk = m.shape
        first, last = np.full(R, -2, np.int32), np.full(R, -2, np.int32)
        self._chk(self.L.nh_align_path(self._h, _fp(m), R, nk, _ip(first), _ip(last)))
        return first, last

    # -- instrumentation ---------------------------------------------------------------------------
    def set_profile_gemm(self, enable: bool):
        self._chk(self.L.nh_set_profile_gemm(self._h, int(enable)))

    def set_option(self, option: int, value: int):
        """A/B switches of include/norma_hip.h (NH_OPT_*): how the decode step is launched, never what it computes."""
        self._chk(self.L.nh_set_option(self._h, int(option), int(value)))

    def timings(self) -> dict:
        t = NhTimings()
        self._chk(self.L.nh_get_timings(self._h, C.byref(t)))
        return {n: getattr(t, n) for n, _ in NhTimings._fields_}
