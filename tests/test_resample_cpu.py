"""CPU: the audio ingest contract without a GPU.  The filter's figures recomputed from the float64 reference, what
resample_bound means and what it catches (tests/resample_ref.py), the streaming bookkeeping nm_resample_plan against its
Python twin, and the new symbols of both C headers."""
import ctypes as C
import os
import re
import zlib

import numpy as np
import pytest

import common
import resample_ref as RR
from norma_amd import hip, host


def rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def stereo_i16(n, *key):
    return rng("frames", *key).integers(-32768, 32768, size=(n, 2)).astype(np.int16)


# ---- the filter -------------------------------------------------------------------------------------------------------------
def response_db(src_hz):
    """(frequencies in Hz, gain in dB) of the prototype filter: the table's rows are its samples at spacing 1/L frame"""
    L, M, T, Wc, c, W = RR.design(src_hz)
    tab = RR.table(src_hz)
    k = np.arange(T) - Wc + 1
    j = np.arange(L)[:, None] - k[None, :] * L + Wc * L   # u L = p - k L, shifted to start at 0
    assert j.min() == 0 and j.max() == L * T - 1
    proto = np.zeros(L * T)
    proto[j.ravel()] = tab.ravel()
    n = 1 << max(16, int(np.ceil(np.log2(32 * len(proto)))))
    Hf = np.abs(np.fft.rfft(proto, n)) / L
    return np.arange(len(Hf)) * (L * src_hz / n), 20 * np.log10(np.maximum(Hf, 1e-300))


@pytest.mark.parametrize("src_hz,taps", [(44100, 192), (48000, 210)])
def test_filter_figures(src_hz, taps):
    """stop band at or below -86 dB from min(8 kHz, src_hz / 2) on, pass band within 0.01 dB up to 6.7 kHz"""
    assert RR.design(src_hz)[2] == taps
    f, db = response_db(src_hz)
    stop, ripple = db[f >= min(8000.0, src_hz / 2)].max(), np.abs(db[f <= 6700.0]).max()
    below3 = f[np.argmax(db < -3.0103)]
    print(f"{src_hz} Hz: stop band {stop:.2f} dB, pass band +-{ripple:.5f} dB to 6.7 kHz, -3 dB at {below3:.0f} Hz")
    assert stop <= -86.0
    assert ripple <= 0.01
    assert 7100 <= below3 <= 7400


def test_tap_counts_of_the_standard_rates():
    got = [RR.design(r)[2] for r in (8000, 11025, 22050, 32000, 44100, 48000, 96000)]
    assert got == [70, 70, 96, 140, 192, 210, 418]
    assert max(RR.design(r)[0] * RR.design(r)[2] for r in (8000, 11025, 22050, 32000, 44100, 48000, 96000)) == 640 * 70
    L = hip.load_library()
    for r in (8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000, 192000):
        l_, m_, t_ = C.c_int32(), C.c_int32(), C.c_int32()
        assert L.nh_resample_table(None, r, None, C.byref(l_), C.byref(m_), C.byref(t_)) == 0
        assert (l_.value, m_.value, t_.value) == RR.design(r)[:3], r
        assert L.nh_resample_len(r, 3001) == RR.out_len(r, 3001)
    for r in (7999, 192001, 0, -1, 191999):   # out of range; the last one would need a table of L * T > 2^20 entries
        assert L.nh_resample_table(None, r, None, None, None, None) == 1 and L.nh_resample_len(r, 100) == -1
    assert L.nh_resample_len(48000, 1440000) == 480000 and L.nh_resample_len(48000, 1440001) == -1
    assert L.nh_resample_len(48000, 0) == -1


# ---- the bound ----------------------------------------------------------------------------------------------------------------
RATES = (48000, 44100, 22050, 8000)


@pytest.mark.parametrize("src_hz", RATES)
def test_f32_accumulation_stays_inside_the_bound(src_hz):
    frames = stereo_i16(3001, src_hz)
    coef = RR.table(src_hz).astype(np.float32)
    T = RR.design(src_hz)[2]
    m32 = RR.mono32(frames)
    assert np.array_equal(m32.astype(np.float64), RR.mono64(frames)), "stereo i16 mixes down exactly"
    ref, sabs = RR.resample64(m32, src_hz, coef)
    got = RR.resample_f32(m32, src_hz, coef)
    used = np.abs(got.astype(np.float64) - ref) / RR.resample_bound(sabs, T)
    print(f"{src_hz} Hz: f32 accumulation uses at most {used.max():.3f} of the bound")
    assert len(ref) == RR.out_len(src_hz, 3001) and used.max() <= 1.0


@pytest.mark.parametrize("src_hz", RATES)
def test_bound_catches_wrong_variants(src_hz):
    """every planted mistake misses the bound by more than a factor of two on nearly every output"""
    frames = stereo_i16(3001, src_hz)
    L, M, T = RR.design(src_hz)[:3]
    coef = RR.table(src_hz).astype(np.float32)
    mono = RR.mono64(frames)
    ref, sabs = RR.resample64(mono, src_hz, coef)
    bound = RR.resample_bound(sabs, T)
    wrong = {"frame index off by one": RR.resample64(mono, src_hz, coef, frame_shift=1)[0],
             "channel 0 alone": RR.resample64(RR.mono64(frames[:, 0]), src_hz, coef)[0],
             "no window": RR.resample64(mono, src_hz, RR.table(src_hz, window=False).astype(np.float32))[0]}
    if L > 1:
        wrong["phase off by 1/L"] = RR.resample64(mono, src_hz, coef, phase_shift=1)[0]
    if M > L:
        wrong["no cut-off scaling"] = RR.resample64(mono, src_hz, RR.table(src_hz, scale_cutoff=False).astype(np.float32))[0]
    for name, y in wrong.items():
        miss = np.abs(y - ref) / bound
        print(f"{src_hz} Hz, {name}: {100 * (miss > 2).mean():.1f} % of outputs miss by > 2x, median {np.median(miss):.0f}x")
        assert (miss > 2).mean() >= 0.98, name


@pytest.mark.parametrize("src_hz", RATES)
def test_bound_catches_a_truncated_window_on_an_impulse(src_hz):
    """The outermost coefficients are ~1e-3 of the centre and vanish in random input; a single 1.0 in silence returns the
    coefficient rows themselves, and every non-zero tap that is dropped is then over the bound on its own.  The impulse is put
    where an output of the phase with the largest outermost coefficient meets it with that tap."""
    L, M, T, Wc = RR.design(src_hz)[:4]
    coef = RR.table(src_hz).astype(np.float32)
    nzc = np.abs(coef[coef != 0]).astype(np.float64)
    assert (nzc > 2 * RR.resample_bound(nzc, T)).all(), "the response to a unit impulse is one coefficient: dropping it must show"
    n_frames = 3001
    i, p = RR.positions(src_hz, RR.out_len(src_hz, n_frames))
    planted = 0
    for name, kw, edge in (("first tap dropped", dict(k_lo=1), -Wc + 1), ("last tap dropped", dict(k_hi=1), Wc)):
        col = coef[:, edge + Wc - 1]
        if not col.any():
            continue   # h is zero there for every phase (|u| >= W): nothing to drop
        ph = int(np.argmax(np.abs(col)))
        n = int(np.flatnonzero((p == ph) & (i > 1000))[0])
        j0 = int(i[n]) + edge
        mono = np.zeros(n_frames)
        mono[j0] = 1.0
        ref, sabs = RR.resample64(mono, src_hz, coef)
        bound = RR.resample_bound(sabs, T)
        k = j0 - i                                    # the tap that meets the impulse at each output
        hit = (k >= -Wc + 1) & (k <= Wc)
        assert np.array_equal(ref[hit], coef[p[hit], k[hit] + Wc - 1].astype(np.float64)) and not ref[~hit].any()
        y = RR.resample64(mono, src_hz, coef, **kw)[0]
        at = hit & (k == edge) & (ref != 0)
        assert at[n] and (np.abs(y[at] - ref[at]) > 2 * bound[at]).all(), name
        assert np.array_equal(y[k != edge], ref[k != edge])
        planted += 1
    assert planted >= 1


# ---- streaming bookkeeping ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_hz", RATES + (16000, 11025))
def test_resample_plan_matches_its_twin_over_random_splits(src_hz):
    L, M, T, Wc = RR.design(src_hz)[:4]
    r = rng("plan", src_hz)
    for trial in range(20):
        received = emitted = first_kept = 0
        sizes = [int(x) for x in r.choice([0, 1, 2, 160, 479, 4799, 30011], size=r.integers(1, 12))]
        for s_i, n in enumerate(sizes):
            final = s_i == len(sizes) - 1
            received += n
            got = host.resample_plan(src_hz, received, emitted, first_kept, final)
            assert got == RR.plan(src_hz, received, emitted, first_kept, final), (src_hz, received, emitted, first_kept, final)
            n_ready, f0, num0, drop = got
            assert n_ready >= 0 and first_kept <= f0 and num0 == emitted * M - f0 * L and num0 >= 0
            if n_ready:
                first, last = emitted, emitted + n_ready - 1
                assert f0 <= max(0, first * M // L - max(Wc - 1, 0)), "the lowest tap of the first output is in the window"
                assert first_kept <= max(0, first * M // L - max(Wc - 1, 0)), "... and was kept"
                if final:
                    assert last * M // L <= received - 1
                else:
                    assert last * M // L + Wc <= received - 1, "every tap of every ready output has been received"
            nxt = emitted + n_ready                                   # maximal: the next output is not ready
            if final:
                assert nxt == -(-received * L // M), "final emits ceil(received L / M) in total"
                assert drop == received
            else:
                assert nxt * M // L + Wc > received - 1 or received <= Wc
                assert drop <= max(first_kept, nxt * M // L - max(Wc - 1, 0)) and first_kept <= drop <= received, "keeps what the next output needs"
            emitted, first_kept = nxt, drop                           # nothing emitted twice or skipped: emitted only moves by n_ready
    assert host.resample_plan(7999, 10, 0, 0, False) is None and host.resample_plan(48000, 10, 0, 11, False) is None
    assert host.resample_plan(48000, -1, 0, 0, False) is None


# ---- symbols --------------------------------------------------------------------------------------------------------------------
NH_NEW = ("nh_resample_len", "nh_resample_table", "nh_resample", "nh_logmel_resampled_rows")
NM_NEW = ("nm_resample_plan", "nm_resampler_new", "nm_resampler_free", "nm_resampler_push", "nm_resampler_read", "nm_resampler_state",
          "nm_definition_set_input_format", "nm_model_set_input_format", "nm_model_transcribe_frames")


def test_new_symbols_are_declared_exported_and_bound():
    L = hip.load_library()
    declared = set(hip.declared_symbols())
    with open(os.path.join(common.ROOT, "include", "norma_host.h")) as f:
        host_h = f.read()
    with open(os.path.join(common.ROOT, "INTEGRATION.md")) as f:
        md = f.read()
    for s in NH_NEW:
        assert s in declared and hasattr(L, s) and f"pub fn {s}(" in md, s
        assert getattr(L, s).argtypes is not None, f"{s}: no ctypes declaration in hip.py"
    for s in NM_NEW:
        assert re.search(rf"\b{s}\s*\(", host_h) and hasattr(L, s), s
    strict = C.CDLL(hip.STRICT_LIB_PATH)
    assert all(hasattr(strict, s) for s in NH_NEW + NM_NEW)
    for m in ("resample", "resample_table", "logmel_resampled", "logmel_resampled_rows"):
        assert callable(getattr(hip.HipWhisper, m, None)), m
    assert callable(getattr(host.Model, "transcribe_frames", None)) and callable(getattr(host.Model, "set_input_format", None))
    assert callable(getattr(host.Definition, "set_input_format", None)) and hasattr(host, "Resampler")
