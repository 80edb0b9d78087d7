"""No GPU: the numpy reference of nh_cut_plan (tests/cut_ref.py) against itself and against planted mistakes, longform.stitch
on hand-written token lists, and the parts of the ABI that need no device.  The GPU side is tests/test_gpu_cut.py; the
contract is in include/norma_hip.h and DESIGN.md 11."""
import ctypes as C

import numpy as np

import common
import cut_ref as CR
from norma_amd import hip, longform

SMALL = (300, 100, 15)


# ---- the reference against itself ------------------------------------------------------------------------------------------
def test_f32_frame_energies_within_the_summation_bound_of_float64():
    """160 products and 160 additions, each rounding once: |e - e64| <= 160 * 2^-24 * e64 (all terms are >= 0)"""
    x = CR.noise(1600000, "bound", amp=0.5)
    e, _ = CR.energies(x, 0)
    ref = CR.e64(x)
    rel = np.abs(e.astype(np.float64) - ref) / ref
    print(f"100 s of noise: worst relative error {rel.max():.2e}, bound {160 * 2.0 ** -24:.2e}")
    assert (np.abs(e.astype(np.float64) - ref) <= 160 * 2.0 ** -24 * ref).all()


def test_window_energy_is_the_ordered_sum_with_zeros_outside():
    x = CR.noise(160 * 40 + 7, "window")
    e, E = CR.energies(x, 3)
    assert len(e) == len(E) == 41
    for f in (0, 2, 20, 38, 40):
        acc = np.float32(0)
        for k in range(-3, 4):
            acc = np.float32(acc + (e[f + k] if 0 <= f + k < 41 else np.float32(0)))
        assert acc.view(np.int32) == E[f].view(np.int32)
    assert np.array_equal(CR.energies(x, 0)[1].view(np.int32), e.view(np.int32))
    # the last frame holds 7 samples: the rest counts as 0
    assert e[40] == CR.energies(x[160 * 40:], 0)[0][0]


def test_silence_and_an_all_nan_recording_cut_at_every_max_frames():
    n = 160 * 1000 + 33
    for x in (np.zeros(n, dtype=np.float32), np.full(n, np.nan, dtype=np.float32)):
        starts, lens, _, E = CR.plan(x, SMALL)
        assert starts.tolist() == [160 * 300 * k for k in range(4)]
        assert lens.tolist() == [48000, 48000, 48000, 160 * 100 + 33]
        assert np.isnan(E).all() or not E.any()


def test_one_chunk_up_to_max_frames_and_two_one_frame_later():
    assert [len(CR.plan(CR.noise(n, n), SMALL)[0]) for n in (160 * 300 - 159, 160 * 300, 160 * 300 + 1)] == [1, 1, 2]
    starts, lens, _, _ = CR.plan(CR.noise(160 * 300 + 1, 1), SMALL)
    assert 100 * 160 <= starts[1] <= 300 * 160 and lens.sum() == 160 * 300 + 1 and (lens <= 48000).all()


# ---- what the rules catch: each planted mistake moves a cut on an input built for it -----------------------------------------
def test_inputs_have_the_property_they_are_named_for():
    _, _, _, E = CR.plan(CR.plateau(), SMALL)
    assert (E[165:235] == 0).all() and (E[100:165] > 0).all() and (E[235:301] > 0).all()
    starts, _, e, E = CR.plan(CR.one_nan(), SMALL)
    assert np.isnan(e[250]) and np.isnan(E[235:266]).all() and not np.isnan(E[100:235]).any() and not np.isnan(E[266:301]).any()
    ok = np.where(np.isnan(E[100:301]), np.inf, E[100:301])
    assert 100 < 100 + int(np.argmin(ok)) < 300 and starts[1] == 160 * (100 + int(np.argmin(ok)))
    _, _, _, E = CR.plan(CR.quiet_last_candidate(), SMALL)
    assert int(np.argmin(E[100:301])) == 200 and E[300] < E[100:300].min()
    starts, _, _, E = CR.plan(CR.nan_range(), SMALL)
    assert np.isnan(E[100:301]).all() and not np.isnan(E[400:]).any() and starts[1] == 160 * 300 and 160 * 400 <= starts[2] < 160 * 600


def test_planted_mistakes_move_a_cut():
    right = CR.plan(CR.plateau(), SMALL)[0]
    assert right[1] == 160 * 234, "the latest frame of the plateau"
    assert CR.plan(CR.plateau(), SMALL, earliest=True)[0][1] == 160 * 165
    right = CR.plan(CR.one_nan(), SMALL)[0]
    wrong = CR.plan(CR.one_nan(), SMALL, nan_least=True)[0]
    assert wrong[1] == 160 * 265 and right[1] != wrong[1]
    right = CR.plan(CR.quiet_last_candidate(), SMALL)[0]
    wrong = CR.plan(CR.quiet_last_candidate(), SMALL, short=1)[0]
    assert right[1] == 160 * 300 and wrong[1] != right[1]
    # silence alone tells the first and the third apart as well
    z = np.zeros(160 * 700, dtype=np.float32)
    assert CR.plan(z, SMALL)[0][1] == 160 * 300 and CR.plan(z, SMALL, earliest=True)[0][1] == 160 * 100
    assert CR.plan(z, SMALL, short=1)[0][1] == 160 * 299


def test_the_reference_cuts_bursty_audio_inside_its_pauses():
    for seed in range(5):
        x, pauses = CR.bursts(seed)
        starts, lens, _, _ = CR.plan(x, SMALL)
        print(f"seed {seed}: {len(starts) - 1} cuts, {len(pauses)} pauses")
        assert len(starts) - 1 >= 6 and CR.cuts_in_pauses(starts, pauses, SMALL[2])
        assert lens.sum() == len(x) and (starts[1:] == starts[:-1] + lens[:-1]).all()


# ---- stitch -------------------------------------------------------------------------------------------------------------------
def test_stitch_joins_chunks_on_one_time_axis():
    tk = common.tokens_for("test-d128")
    ts = lambda sec: tk.no_timestamps + 1 + int(round(sec / 0.02))
    prompt = [tk.sot, tk.en, tk.transcribe]
    a = dict(tokens=prompt + [ts(0.0), 400, 401, ts(1.2), ts(1.4), 402, ts(2.5), tk.eot], no_speech_exit=False, start_sample=0, n_samples=41600)
    silent = dict(tokens=prompt + [tk.eot], no_speech_exit=True, start_sample=41600, n_samples=32000)
    b = dict(tokens=prompt + [ts(0.1), 403, ts(0.9), ts(1.0), 404, 405, ts(2.0), ts(2.2), 406, 407, tk.eot], no_speech_exit=False,
             start_sample=73600, n_samples=48000)
    segs = longform.stitch([a, silent, b], tk)
    assert [s[2] for s in segs] == [[400, 401], [402], [403], [404, 405], [406, 407]]
    want = [(0.0, 1.2), (1.4, 2.5), (4.6 + 0.1, 4.6 + 0.9), (4.6 + 1.0, 4.6 + 2.0), (4.6 + 2.2, (73600 + 48000) / 16000)]
    for (s0, s1, _), (w0, w1) in zip(segs, want):
        assert abs(s0 - w0) < 1e-9 and abs(s1 - w1) < 1e-9
    assert all(segs[i][1] <= segs[i + 1][0] + 1e-9 for i in range(len(segs) - 1)), "segments of neighbouring chunks join in order"
    # nothing but boundaries, or no closing boundary at all: no segment
    assert longform.stitch([dict(tokens=prompt + [ts(0.0), ts(1.0), tk.eot], no_speech_exit=False, start_sample=0, n_samples=16000)], tk) == []
    assert longform.stitch([dict(tokens=prompt + [ts(0.0), 400], no_speech_exit=False, start_sample=0, n_samples=16000)], tk) == []


def test_groups_keep_a_short_final_chunk_alone():
    assert longform._groups([48000] * 7, 6) == [(0, 6), (6, 7)]
    assert longform._groups([48000, 48000, 159], 6) == [(0, 2), (2, 3)]
    assert longform._groups([159], 6) == [(0, 1)]
    assert longform._groups([48000, 160], 6) == [(0, 2)]


# ---- the ABI, as far as no device is needed ---------------------------------------------------------------------------------
def test_struct_and_symbols():
    assert C.sizeof(hip.NhCutParams) == 12
    L = hip.load_library()
    assert {"nh_cut_plan", "nh_cut_energy", "nh_logmel_chunks_rows"} <= set(hip.declared_symbols())
    for s in ("nh_cut_plan", "nh_cut_energy", "nh_logmel_chunks_rows"):
        assert hasattr(L, s)


def test_calls_without_a_context_are_refused_and_write_nothing():
    """parameter refusals need a context, and a context needs a device: they are in tests/test_gpu_cut.py"""
    L = hip.load_library()
    x = CR.noise(1600, "abi")
    starts, lens, cnt = np.full(4, -7, dtype=np.int64), np.full(4, -7, dtype=np.int32), C.c_int32(-7)
    q = hip.NhCutParams(300, 100, 15)
    assert L.nh_cut_plan(None, x.ctypes.data_as(C.c_void_p), 0, len(x), C.byref(q), starts.ctypes.data_as(C.POINTER(C.c_int64)),
                         lens.ctypes.data_as(C.POINTER(C.c_int32)), 4, C.byref(cnt)) == 1
    assert (starts == -7).all() and (lens == -7).all() and cnt.value == -7
    e = np.full(10, 7.5, dtype=np.float32)
    assert L.nh_cut_energy(None, e.ctypes.data_as(C.POINTER(C.c_float)), None, 10) == 1 and (e == 7.5).all()
    assert L.nh_logmel_chunks_rows(None, x.ctypes.data_as(C.c_void_p), 0, starts.ctypes.data_as(C.POINTER(C.c_int64)),
                                   lens.ctypes.data_as(C.POINTER(C.c_int32)), 1, 0) == 1
