"""CPU: the header reader (norma_amd/cabi.py) and the bindings it makes for include/norma_hip.h and include/norma_host.h.
The expected types, sizes and values are written out here literally: they are what the two headers say today, read by eye, so
that a reader that drifts from C's rules shows up as a failing line and not as a shifted argument.  No device is touched."""
import ctypes as C
import re
from ctypes import POINTER, c_char_p, c_int, c_int64, c_size_t, c_uint16, c_void_p

import numpy as np
import pytest

from norma_amd import cabi, hip, host


def _parameter_count(text: str, name: str) -> int:
    """the commas of `name`'s parameter list in the raw header text, counted without the reader: comments stripped, the text
    between the name's parenthesis and the next `)` (no prototype of the two headers nests parentheses)"""
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    params = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, code).group(1).strip()
    return 0 if params in ("", "void") else params.count(",") + 1


@pytest.mark.parametrize("path, lib, n", [(hip.HEADER_PATH, hip.load_library, 69), (host.HEADER_PATH, host._lib, 45)])
def test_every_prototype_is_bound_with_its_parameter_count(path, lib, n):
    L = lib()
    H = cabi.read(path)
    assert len(H.prototypes) == n
    with open(path) as f:
        text = f.read()
    for name, (restype, argtypes, names) in H.prototypes.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(argtypes) == len(names) == _parameter_count(text, name), name
        assert fn.restype is restype, name
        assert all(names), name   # every parameter of the two headers is named
    assert sorted(cabi.bind(C.CDLL(hip.LIB_PATH), path)) == sorted(H.prototypes)


def test_declared_symbols_are_the_names_the_header_mentions_before_a_parenthesis():
    """the comments of norma_hip.h name no function that the header does not declare, so the prototype names are what the
    earlier regex over the raw text gave"""
    with open(hip.HEADER_PATH) as f:
        text = f.read()
    assert hip.declared_symbols() == sorted(set(re.findall(r"\b(nh_[a-z_0-9]+)\s*\(", text)))
    assert len(hip.declared_symbols()) == 69


def test_spot_checks_of_the_generated_types():
    L = host._lib()
    a = L.nh_resample.argtypes
    assert len(a) == 13 and a[1] is c_void_p and a[9] is POINTER(c_int64) and a[12] is c_int64
    assert L.nh_create.argtypes[-1] is POINTER(c_void_p)
    assert L.nh_last_error.restype is c_char_p
    assert L.nh_destroy.restype is None
    assert L.nh_beam_reorder.argtypes[-1] is POINTER(c_uint16)
    assert L.nm_definition_max_chunk_len.restype is c_size_t
    assert L.nm_language_code.restype is c_char_p
    assert L.nm_resampler_push.restype is c_int64
    # further corners of the mapping: an opaque pointer, an array parameter, a typed struct pointer, char * out-buffers
    assert L.nh_destroy.argtypes == [c_void_p] and L.nm_definition_new.restype is c_void_p
    assert L.nh_vad_view.argtypes[4] is POINTER(C.c_float) and L.nh_vad_view.argtypes[2] is POINTER(C.c_uint8)
    assert L.nh_get_timings.argtypes[1] is POINTER(hip.NhTimings) and L.nh_set_guard.argtypes[1] is POINTER(hip.NhGuardParams)
    assert L.nm_model_transcribe.argtypes[2] is c_size_t and L.nm_model_transcribe.argtypes[8] is c_char_p
    assert L.nm_model_transcribe.argtypes[6] is POINTER(c_int) and L.nm_model_transcribe.argtypes[7] is POINTER(c_size_t)
    assert L.nh_device_count.argtypes == [] and L.nh_device_count.restype is c_int
    assert L.nh_pool_retry.argtypes[2:] == [C.c_float, C.c_uint64, C.c_uint32, C.c_uint32]


def test_device_or_host_pcm_is_bound_as_a_bare_address():
    """the seven `const float *` parameters that may hold a device address take what the callers hand them, a c_void_p; every
    entry names a real pointer parameter (bind refuses one that does not)"""
    L = hip.load_library()
    H = cabi.read(hip.HEADER_PATH)
    assert len(hip._ADDRESSES) == 7
    for fn, (param,) in hip._ADDRESSES.items():
        i = H.prototypes[fn][2].index(param)
        assert i == 1 and H.prototypes[fn][1][i] is POINTER(C.c_float) and getattr(L, fn).argtypes[i] is c_void_p, fn
    for bad in ({"nh_cut_plan": ("pcmx",)}, {"nh_cut_planx": ("pcm",)}, {"nh_cut_plan": ("on_device",)}, {"nh_resample": ("frames",)}):
        with pytest.raises(cabi.HeaderError):
            cabi.bind(C.CDLL(hip.LIB_PATH), hip.HEADER_PATH, bad)


def test_host_header_uses_the_first_headers_struct_classes():
    H, N = cabi.read(hip.HEADER_PATH), cabi.read(host.HEADER_PATH)
    assert N.structs["nh_config"] is H.structs["nh_config"] is hip.NhConfig
    a = host._lib().nm_definition_blocking_try_to_model.argtypes
    assert a[1] is POINTER(hip.NhConfig) and a[2] is POINTER(hip.NhTokens)
    assert not any(n.startswith("nh_") for n in N.prototypes) and not any(n.startswith("NH_") for n in N.constants)


def test_struct_sizes_and_the_offsets_padding_decides():
    r = hip.NhDecodeResult
    assert C.sizeof(r) == 24 and r.avg_logprob.offset == 8 and r.no_speech_prob.offset == 16
    t = hip.NhTimings
    assert C.sizeof(t) == 40 and t.gemm_flops.offset == 32 and t.decode_steps.offset == 16 and t.gemm_launches.offset == 24
    assert C.sizeof(hip.NhVadParams) == 44 and hip.NhVadParams.lo_ratio.offset == 20 and hip.NhVadParams.min_speech_frames.offset == 32
    g = hip.NhGuardParams
    assert C.sizeof(g) == 20 and g.repetition_penalty.offset == 4 and dict(g._fields_)["repetition_penalty"] is C.c_float
    assert C.sizeof(hip.NhCutParams) == 12 and C.sizeof(hip.NhAlignHead) == 8
    assert [n for n, _ in hip.NhAlignHead._fields_] == ["layer", "head"]
    assert [n for n, _ in hip.NhTokens._fields_] == ["sot", "eot", "lang", "task", "no_speech", "no_timestamps", "zero_sec", "one_sec"]
    assert [n for n, _ in hip.NhConfig._fields_] == [
        "num_mel_bins", "max_source_positions", "d_model", "encoder_attention_heads", "encoder_layers", "vocab_size",
        "max_target_positions", "decoder_attention_heads", "decoder_layers"]
    # positional construction in the header's order, and NhVadParams.of on a tuple
    q = hip.NhVadParams.of((3000, 2000, 15, 100, 900, 4.0, 0.01, 0.0, 10, 20, 100))
    assert (q.max_frames, q.hi_permille, q.lo_ratio, q.min_gap_frames) == (3000, 900, 4.0, 100) and hip.NhVadParams.of(q) is q
    p = hip.NhGuardParams(3, 1.5, 4, 2, 1)
    assert (p.no_repeat_ngram, p.repetition_penalty, p.loop_period, p.loop_repeats, p.bias) == (3, 1.5, 4, 2, 1)


def test_constants_equal_the_literals_the_module_used_to_restate():
    want = dict(NH_OPT_DECODE_GRAPHS=0, NH_OPT_FUSE_DECODE_LAYERNORM=1, NH_OPT_DECODER_LAYER_LIMIT=2, NH_OPT_ABSORBED_XATTN=3,
                NH_OPT_ALIGN_KEEP=4, NH_OPT_PROMPT_STEPWISE=5, NH_MAX_BEAMS=8, NH_GUARD_MAX_BIAS=256, NH_ALIGN_MAX_HEADS=32,
                NH_LANG_DETECT=-2, NH_CUT_HOP=160, NH_DTYPE_F32=0, NH_DTYPE_F16=1, NH_ERR_NOMEM=4, N_SAMPLES=480000, N_FRAMES=3000,
                NH_N_SAMPLES=480000, NH_N_FRAMES=3000, NH_OK=0, NH_ERR_INVALID=1, NH_ERR_HIP=2, NH_ERR_STATE=3, NH_MAX_BATCH=96)
    for name, value in want.items():
        assert getattr(hip, name) == value and type(getattr(hip, name)) is int, name
    assert hip.SAMPLE_DTYPES == {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.int8): 2, np.dtype(np.int16): 3,
                                 np.dtype(np.int32): 4, np.dtype(np.int64): 5, np.dtype(np.uint8): 6, np.dtype(np.uint16): 7,
                                 np.dtype(np.uint32): 8, np.dtype(np.uint64): 9}
    assert hip.SAMPLE_DTYPES[np.dtype(np.uint64)] == 9
    assert "NORMA_HIP_H" not in cabi.read(hip.HEADER_PATH).constants   # the include guard is no constant
    N = cabi.read(host.HEADER_PATH).constants
    assert N["NM_DEVICE_ROCM"] == 3 and N["NM_MODEL_LARGE_V3"] == 15 and "NORMA_HOST_H" not in N


def test_host_enums_are_the_headers_constants_under_the_references_names():
    """SelectedDevice's kinds and ModelType's members go straight into nm_definition_new: they are NM_DEVICE_* / NM_MODEL_*
    read from norma_host.h, and equal the literals the module used to restate"""
    want = dict(TinyEn=0, BaseEn=1, SmallEn=2, MediumEn=3, DistilMediumEn=4, DistilLargeEnV2=5, DistilLargeEnV3=6,
                QuantizedTinyEn=7, QuantizedTiny=8, Tiny=9, Base=10, Small=11, Medium=12, Large=13, LargeV2=14, LargeV3=15)
    assert {m.name: m.value for m in host.ModelType} == want and len(host.ModelType) == 16
    assert issubclass(host.ModelType, int) and host.ModelType.DistilLargeEnV3 == 6 and host.ModelType(9) is host.ModelType.Tiny
    assert host.QUANTIZED_EXT == {host.ModelType.QuantizedTinyEn: "tiny-en", host.ModelType.QuantizedTiny: "tiny"}
    D = host.SelectedDevice
    assert (D.Cpu(), D.Cuda(2), D.Metal(), D.Rocm(5), D()) == (D(0, 0), D(1, 2), D(2, 0), D(3, 5), D(0, 0))
    N = cabi.read(host.HEADER_PATH).constants
    assert [N[k] for k in ("NM_DEVICE_CPU", "NM_DEVICE_CUDA", "NM_DEVICE_METAL", "NM_DEVICE_ROCM")] == [0, 1, 2, 3]
    assert sum(k.startswith("NM_MODEL_") for k in N) == 16 and len(N) == 20


ACCEPTED = """
#ifndef X_H
#define X_H
#define X_PI 3.14
#define X_NAME "x"
#define X_NEG (-7)
#define X_HEX 0x10
#ifdef __cplusplus
extern "C" {
#endif
typedef struct x_ctx x_ctx;
typedef struct x_pair { int32_t a, b; double c; } x_pair;
/* x_ghost(int) is named in a comment only */
int x_split(x_ctx *ctx,
            const float *in /* ( ; */, int64_t n,
            x_pair *out);
void x_array(float levels[3], uint8_t mask[], const x_pair *p);
const char *x_name(void);
x_ctx *x_open(const char *path, x_ctx **out);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reader_accepts_split_prototypes_comments_in_parameter_lists_and_arrays():
    H = cabi.parse(ACCEPTED)
    assert H.constants == {"X_NEG": -7, "X_HEX": 16}
    assert list(H.prototypes) == ["x_split", "x_array", "x_name", "x_open"] and H.opaque == {"x_ctx"}
    pair = H.structs["x_pair"]
    assert pair._fields_ == [("a", C.c_int32), ("b", C.c_int32), ("c", C.c_double)] and C.sizeof(pair) == 16
    assert H.prototypes["x_split"] == (c_int, [c_void_p, POINTER(C.c_float), c_int64, POINTER(pair)], ["ctx", "in", "n", "out"])
    assert H.prototypes["x_array"] == (None, [POINTER(C.c_float), POINTER(C.c_uint8), POINTER(pair)], ["levels", "mask", "p"])
    assert H.prototypes["x_name"] == (c_char_p, [], [])
    assert H.prototypes["x_open"] == (c_void_p, [c_char_p, POINTER(c_void_p)], ["path", "out"])


@pytest.mark.parametrize("what, decl", [
    ("an unknown type", "int f(x_ctx *c, wchar_t w);"),
    ("an unknown pointee", "int f(x_ctx *c, long *n);"),
    ("an unknown return type", "unsigned f(x_ctx *c);"),
    ("a struct by value", "int f(x_ctx *c, x_pair p);"),
    ("a struct returned by value", "x_pair f(x_ctx *c);"),
    ("an opaque struct by value", "int f(x_ctx c);"),
    ("a function pointer", "int f(x_ctx *c, void (*done)(int), int n);"),
    ("an attribute", "int f(x_ctx *c) __attribute__((warn_unused_result));"),
    ("a pointer field", "typedef struct x_bad { int32_t n; float *p; } x_bad;"),
    ("a struct field", "typedef struct x_bad { x_pair p; } x_bad;"),
    ("an array field", "typedef struct x_bad { int32_t n[4]; } x_bad;"),
    ("a pointer to a pointer to a scalar", "int f(float **rows);"),
    ("void by value", "int f(void v);"),
    ("a union", "typedef union x_u { int32_t i; float f; } x_u;"),
    ("an inline body", "static inline int f(int a) { return a; }"),
])
def test_reader_refuses_what_it_cannot_map_and_quotes_the_declaration(what, decl):
    head = "typedef struct x_ctx x_ctx;\ntypedef struct x_pair { int32_t a, b; } x_pair;\nint ok(x_ctx *c);\n"
    assert list(cabi.parse(head).prototypes) == ["ok"]
    with pytest.raises(cabi.HeaderError) as e:
        cabi.parse(head + decl + "\nint after(int a);\n")
    quoted = re.search(r"`([^`]*)`$", str(e.value))
    assert quoted and quoted.group(1)[:12] in " ".join(decl.split()), (what, str(e.value))
