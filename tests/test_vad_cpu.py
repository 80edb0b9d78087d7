"""No GPU: the numpy reference of nh_vad_plan (tests/vad_ref.py) against the properties its signals were built for and against
planted mistakes, longform.to_recording / stitch_speech on hand-written token lists, and the parts of the ABI that need no
device.  The GPU side is tests/test_gpu_vad.py; the contract is in include/norma_hip.h and DESIGN.md 12."""
import ctypes as C

import numpy as np

import common
import cut_ref as CR
import vad_ref as VR
from norma_amd import hip, longform

SMALL = VR.SMALL
NEW = ("nh_vad_plan", "nh_vad_view", "nh_logmel_pieces_rows")


# ---- the ABI, as far as no device is needed ---------------------------------------------------------------------------------
def test_struct_and_symbols():
    assert C.sizeof(hip.NhVadParams) == 44
    q = hip.NhVadParams.of(VR.DEFAULTS)
    assert (q.max_frames, q.hi_permille, q.min_gap_frames) == (3000, 900, 100) and q.lo_ratio == 4.0 and abs(q.hi_ratio - 0.01) < 1e-9
    assert set(NEW) <= set(hip.declared_symbols())


def test_the_library_exports_the_three_entry_points():
    L = hip.load_library()
    for s in NEW:
        assert hasattr(L, s), s
    assert all(hasattr(C.CDLL(hip.STRICT_LIB_PATH), s) for s in NEW)


def test_calls_without_a_context_are_refused_and_write_nothing():
    """parameter refusals need a context, and a context needs a device: they are in tests/test_gpu_vad.py"""
    L = hip.load_library()
    x = CR.noise(1600, "abi")
    starts, lens, first = np.full(4, -7, dtype=np.int64), np.full(4, -7, dtype=np.int32), np.full(5, -7, dtype=np.int32)
    n_p, n_c = C.c_int32(-7), C.c_int32(-7)
    i64, i32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    q = hip.NhVadParams.of(SMALL)
    assert L.nh_vad_plan(None, x.ctypes.data_as(C.c_void_p), 0, len(x), C.byref(q), starts.ctypes.data_as(i64), lens.ctypes.data_as(i32), 4,
                         C.byref(n_p), first.ctypes.data_as(i32), 4, C.byref(n_c)) == 1
    assert (starts == -7).all() and (lens == -7).all() and (first == -7).all() and n_p.value == -7 and n_c.value == -7
    E = np.full(10, 7.5, dtype=np.float32)
    assert L.nh_vad_view(None, E.ctypes.data_as(C.POINTER(C.c_float)), None, 10, None, None, 0, None) == 1 and (E == 7.5).all()
    assert L.nh_logmel_pieces_rows(None, x.ctypes.data_as(C.c_void_p), 0, starts.ctypes.data_as(i64), lens.ctypes.data_as(i32),
                                   first.ctypes.data_as(i32), 1, 0) == 1


# ---- the reference on its signals -------------------------------------------------------------------------------------------
def test_bursts_lose_frames_only_inside_pauses_and_every_full_pause_loses_some():
    for seed in range(5):
        x, pauses = CR.bursts(seed)
        p = VR.plan(x, SMALL)
        gone = VR.dropped_frames(p)
        per_pause = [int(((gone >= -(-a // 160)) & (gone < b // 160)).sum()) for a, b in pauses]
        print(f"seed {seed}: {len(gone)} of {len(p.speech)} frames dropped, per pause {sorted(set(per_pause))}, {len(p.regions)} regions, "
              f"{len(p.piece_starts)} pieces, {len(p.chunk_first) - 1} chunks")
        for f in gone:
            assert any(a <= 160 * f and 160 * (f + 1) <= b for a, b in pauses), f"seed {seed}: frame {f} is dropped outside the pauses"
        for (a, b), n in zip(pauses, per_pause):
            assert b - a < 8000 or n >= 1, f"seed {seed}: the pause at sample {a} loses nothing"
        assert len(gone) > 0 and (np.diff(p.chunk_first) >= 1).all()
        frames = np.add.reduceat(np.array(p.piece_frames), p.chunk_first[:-1])
        assert (frames <= SMALL[0]).all() and frames.sum() == len(p.speech) - len(gone)


def test_noise_at_one_level_is_kept_whole_and_cut_like_a_recording():
    x = VR.all_speech()
    p = VR.plan(x, VR.with_shaping((300, 100, 15) + SMALL[3:8], 5, 5, 20))
    assert p.regions.tolist() == [[0, 701]] and p.speech.all()
    want = CR.cuts(p.E, 701, 100, 300)
    print(f"pieces start at frames {want}")
    assert want == [0, 295, 574] and p.piece_starts.tolist() == [160 * c for c in want]
    assert p.piece_lens.sum() == len(x) and p.piece_lens[-1] == len(x) - 160 * want[-1]
    assert p.chunk_first.tolist() == [0, 1, 2, 3], "295, 279 and 127 frames: no two share 300"
    starts, lens, _, _ = CR.plan(x, (300, 100, 15))
    assert starts.tolist() == p.piece_starts.tolist() and lens.tolist() == p.piece_lens.tolist(), "the cut planner's chunks"


def test_silence_has_no_speech():
    p = VR.plan(np.zeros(160 * 500 + 3, dtype=np.float32), SMALL)
    assert p.levels.tolist() == [0, 0, 0] and not p.speech.any()
    assert len(p.regions) == 0 and len(p.piece_starts) == 0 and p.chunk_first.tolist() == [0]


def test_a_nan_is_kept_infinity_is_kept_and_only_the_quiet_stretch_goes():
    p = VR.plan(VR.nan_inf_quiet(), SMALL)
    assert np.isnan(p.E[95:106]).all() and np.isinf(p.E[295:306]).all() and np.isfinite(p.levels).all()
    assert VR.dropped_frames(p).tolist() == list(range(510, 550)), "W = 5 and pad = 5 inside frames 500 .. 559"
    assert p.regions.tolist() == [[0, 510], [550, 700]]


# ---- what the rules catch: each planted mistake changes the plan on an input built for it -------------------------------------
def differs(x, params, **mistake):
    right, wrong = VR.plan(x, params), VR.plan(x, params, **mistake)
    same = (right.piece_starts.tolist() == wrong.piece_starts.tolist() and right.piece_lens.tolist() == wrong.piece_lens.tolist()
            and right.chunk_first.tolist() == wrong.chunk_first.tolist())
    return right, wrong, not same


def test_a_nan_admitted_to_the_statistic_moves_the_levels():
    x = VR.many_nans()
    right, wrong, moved = differs(x, SMALL, admit_nan=True)
    assert np.isnan(right.E[:140]).all() and int(np.isnan(right.E).sum()) * 10 > len(right.E), "more NaN frames than the loud decile"
    assert right.speech.all() and np.isfinite(right.levels).all(), "the quiet stretch is 14 dB down: kept"
    assert np.isnan(wrong.levels[1]) and moved


def test_less_than_in_place_of_less_or_equal_keeps_silence():
    z = np.zeros(160 * 500, dtype=np.float32)
    right, wrong, moved = differs(z, SMALL, strict=True)
    assert SMALL[7] == 0.0 and right.levels[2] == 0 and not right.E.any()
    assert len(right.piece_starts) == 0 and wrong.speech.all() and moved


def test_the_larger_of_the_two_levels_drops_speech():
    right, wrong, moved = differs(VR.all_speech(), SMALL, take_max=True)
    assert right.speech.all() and right.levels[2] < right.E.min() and 4 * right.levels[0] > right.E.max()
    assert not wrong.speech.any() and moved


def test_shaping_order_gap_length_and_leading_silence():
    x = VR.blips_and_gaps()
    params = (300, 100, 0) + SMALL[3:]
    right = VR.plan(x, params)
    assert VR.runs(right.raw) == [(12, 40), (69, 100), (130, 160), (250, 253), (300, 330)] and right.levels[2] == 0
    assert right.regions.tolist() == [[7, 105], [125, 165], [295, 335]]
    assert differs(x, params, dilate_first=True)[1].regions.tolist() == [[7, 105], [125, 165], [245, 258], [295, 335]]
    assert differs(x, params, gap_le=True)[1].regions.tolist() == [[7, 165], [295, 335]]
    assert differs(x, params, fill_leading=True)[1].regions.tolist() == [[0, 105], [125, 165], [295, 335]]
    for m in ("dilate_first", "gap_le", "fill_leading"):
        assert differs(x, params, **{m: True})[2], m


def test_packing_with_less_than_opens_a_chunk_too_early():
    """two regions of 150 frames each fill a chunk of 300 exactly"""
    x = np.zeros(160 * 400, dtype=np.float32)
    for a in (10, 200):
        x[160 * a:160 * (a + 150)] = CR.noise(160 * 150, ("pack", a), amp=0.3)
    params = (300, 100, 0) + SMALL[3:8] + (1, 0, 1)
    right, wrong, moved = differs(x, params, pack_lt=True)
    assert right.piece_frames == [150, 150] and right.chunk_first.tolist() == [0, 2]
    assert wrong.chunk_first.tolist() == [0, 1, 2] and moved


def test_to_recording_keeps_an_end_in_front_of_the_dropped_silence():
    pieces = [(0, 1000, 3200), (3200, 9000, 1600)]
    for fn in (longform.to_recording, VR.to_recording):
        assert fn(pieces, 0) == 1000 and fn(pieces, 3199) == 4199
        assert fn(pieces, 3200) == 9000, "a start on the boundary begins behind the silence"
        assert fn(pieces, 3200, end=True) == 4200, "an end on the boundary stays in front of it"
        assert fn(pieces, 3201, end=True) == 9001 and fn(pieces, 4800, end=True) == 10600
        assert fn(pieces, 4800) == 10600 and fn(pieces, 9999) == 10600 and fn(pieces, 9999, end=True) == 10600, "past the last piece"
        assert fn(pieces, 0, end=True) == 1000
    assert VR.to_recording(pieces, 3200, swapped=True) == 4200 and VR.to_recording(pieces, 3200, end=True, swapped=True) == 9000
    for tau in range(0, 5000, 37):
        for end in (False, True):
            assert longform.to_recording(pieces, tau, end) == VR.to_recording(pieces, tau, end)


# ---- stitch_speech ----------------------------------------------------------------------------------------------------------
def test_stitch_speech_maps_segments_through_the_pieces():
    tk = common.tokens_for("test-d128")
    ts = lambda sec: tk.no_timestamps + 1 + int(round(sec / 0.02))
    prompt = [tk.sot, tk.en, tk.transcribe]
    # chunk a: 2 s from second 1 and 1 s from second 10; chunk b: 1.5 s from second 20 and 0.5 s from second 30
    a = dict(tokens=prompt + [ts(0.0), 400, 401, ts(2.0), ts(2.0), 402, ts(2.5), ts(2.6), 403, tk.eot], no_speech_exit=False,
             pieces=[(0, 16000, 32000), (32000, 160000, 16000)], n_samples=48000)
    silent = dict(tokens=prompt + [tk.eot], no_speech_exit=True, pieces=[(0, 200000, 16000)], n_samples=16000)
    b = dict(tokens=prompt + [ts(0.5), 404, ts(1.7), tk.eot], no_speech_exit=False, pieces=[(0, 320000, 24000), (24000, 480000, 8000)],
             n_samples=32000)
    segs = longform.stitch_speech([a, silent, b], tk)
    assert [s[2] for s in segs] == [[400, 401], [402], [403], [404]]
    want = [(1.0, 3.0),        # ends on the boundary: in front of the silence between second 3 and second 10
            (10.0, 10.5),      # starts on the boundary: behind it
            (10.6, 11.0),      # closed by eot: the end of the chunk's last piece
            (20.5, 30.2)]      # from the first piece into the second
    for (s0, s1, _), (w0, w1) in zip(segs, want):
        assert abs(s0 - w0) < 1e-9 and abs(s1 - w1) < 1e-9, (s0, s1, w0, w1)
    assert all(segs[i][1] <= segs[i + 1][0] + 1e-9 for i in range(len(segs) - 1))
    # a one-piece chunk is stitch itself
    one = dict(tokens=prompt + [ts(0.0), 400, ts(1.2), ts(1.4), 401, tk.eot], no_speech_exit=False, pieces=[(0, 8000, 41600)], n_samples=41600,
               start_sample=8000)
    got, same = longform.stitch_speech([one], tk), longform.stitch([one], tk)
    assert len(got) == len(same) == 2 and all(abs(g[0] - s[0]) < 1e-9 and abs(g[1] - s[1]) < 1e-9 and g[2] == s[2] for g, s in zip(got, same))
