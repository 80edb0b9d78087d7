"""GPU: the speech map of long recordings on the device (nh_vad_plan, nh_vad_view, nh_logmel_pieces_rows,
longform.transcribe_speech) against the bit-exact numpy reference of tests/vad_ref.py and against the existing log-mel / encode /
decode path, on a test-d128 context.  The contract is in include/norma_hip.h and DESIGN.md 12; what the reference's rules catch
is shown without a GPU in tests/test_vad_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import common
import cut_ref as CR
import vad_ref as VR
from norma_amd import config, hip, longform

pytestmark = pytest.mark.gpu

HIST_TILE = 4096     # NH_VAD_HIST_TILE: frames per workgroup of the select's histogram kernel
TILE = 2048          # NH_VAD_TILE: frames per workgroup of the shaping kernels
CARRY_THREADS = 256  # the carry kernel takes more than one tile per thread above this many tiles
STAGE_FRAMES = (256 << 20) // (4 * CR.HOP)   # frames per staging group of host PCM
MAX_BATCH = 6
SMALL = VR.SMALL
HEADS = [(0, 1), (1, 0)]
INVALID, STATE = 1, 3
I32, I64, F32, U8 = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


def f64_bits(v):
    return np.float64(v).view(np.int64)


@pytest.fixture(scope="module")
def tk():
    return common.tokens_for("test-d128")


@pytest.fixture(scope="module")
def script(tk):
    return common.transcript_script(tk, n_segments=2, words_per_segment=4)


@pytest.fixture(scope="module")
def hm(tk, script):
    cfg = config.preset("test-d128")
    m = common.build_hip(cfg, tk, overrides=common.scripted_overrides(cfg, tk, script), max_batch=MAX_BATCH)
    yield m
    m.close()


def check_against(hm, ref, what, got):
    """a device plan (what vad_plan returned) and its view against a reference plan, bit for bit"""
    starts, lens, first = got
    E, speech, levels, regions = hm.vad_view()
    assert same_bits(E, ref.E), f"{what}: window energies, first difference at frame {int(np.argmax(E.view(np.int32) != ref.E.view(np.int32)))}"
    assert same_bits(levels, ref.levels), f"{what}: levels {levels.tolist()} for {ref.levels.tolist()}"
    assert speech.dtype == np.uint8 and np.array_equal(speech, ref.speech), f"{what}: speech, first difference at frame {int(np.argmax(speech != ref.speech))}"
    assert regions.dtype == np.int64 and regions.tolist() == ref.regions.tolist(), what
    assert starts.dtype == np.int64 and lens.dtype == np.int32 and first.dtype == np.int32
    assert starts.tolist() == ref.piece_starts.tolist() and lens.tolist() == ref.piece_lens.tolist(), what
    assert first.tolist() == ref.chunk_first.tolist(), what
    return ref


def check_plan(hm, x, params, what, src=None, n=None):
    return check_against(hm, VR.plan(x, VR.DEFAULTS if params is None else params), what, hm.vad_plan(x if src is None else src, n, params))


# ---- bit equality -------------------------------------------------------------------------------------------------------------
SIZES = [1, 159, 160, 161, 160 * 255 + 7, 160 * 256, 160 * 257 + 1, 160 * 1025 + 33, 320000 - 37,
         160 * TILE, 160 * TILE + 1, 160 * HIST_TILE, 160 * HIST_TILE + 1]


@pytest.mark.parametrize("shaping", [(1, 0, 1), (5, 5, 20)])
@pytest.mark.parametrize("n", SIZES)
def test_every_output_equals_the_reference_bit_for_bit(hm, n, shaping):
    x = VR.loguniform(n, ("bits", n))
    ref = check_plan(hm, x, VR.with_shaping(SMALL, *shaping), f"{n} samples, shaping {shaping}")
    if n == 320000 - 37:   # the signal's property: every pass of the select has work
        key = ref.E.view(np.uint32) | np.uint32(0x80000000)
        spread = [len(np.unique((key >> s) & 255)) for s in (0, 8, 16, 24)]
        print(f"distinct key bytes, low to high: {spread}; {len(ref.regions)} regions, {len(ref.piece_starts)} pieces")
        assert min(spread[:3]) >= 240 and spread[3] >= 8 and 0 < ref.speech.sum() < len(ref.speech)


def test_more_tiles_than_the_carry_kernel_has_threads(hm):
    """a host recording of 256 shaping tiles and a bit (two staging groups): silence with bursts across the places where a
    carry changes hands -- a tile's edge, the edge between two threads' tiles, the recording's ends -- and a long region"""
    F = CARRY_THREADS * TILE + 2 * TILE + 5
    x = np.zeros(160 * F - 3, dtype=np.float32)
    for a, b in ((0, 40), (TILE - 3, TILE + 3), (2 * TILE - 9, 2 * TILE - 1), (2 * TILE + 1, 2 * TILE + 2), (4 * TILE, 4 * TILE + 700),
                 (255 * TILE - 4, 255 * TILE + 4), (256 * TILE + 17, 257 * TILE + 400), (F - 30, F)):
        x[160 * a:160 * b] = CR.noise(160 * (b - a), ("carry", a), amp=0.3)[:len(x[160 * a:160 * b])]
    ref = check_plan(hm, x, (300, 100, 2) + SMALL[3:8] + (3, 4, 12), "more than 256 tiles")
    assert len(ref.regions) == 7 and ref.regions[0][0] == 0 and ref.regions[-1][1] == F and len(ref.piece_starts) > 12


# ---- ties ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floor", [0.0, 0.5])
def test_silence_has_no_speech_whatever_the_floor(hm, floor):
    ref = check_plan(hm, np.zeros(160 * 500 + 3, dtype=np.float32), SMALL[:7] + (floor,) + SMALL[8:], f"silence, floor {floor}")
    assert ref.levels.tolist() == [0, 0, floor] and ref.chunk_first.tolist() == [0] and len(ref.piece_starts) == 0


@pytest.mark.parametrize("lo,hi", [(100, 900), (500, 500), (0, 1000), (0, 0), (1000, 1000)])
def test_a_two_valued_recording_and_every_rank(hm, lo, hi):
    """frames of constant samples 0.25 or 0.5 (W = 0: E takes two values, 60 : 40), every select pass a two-way tie"""
    loud = np.random.default_rng(5).uniform(size=1000) < 0.4
    x = np.where(loud, np.float32(0.5), np.float32(0.25)).astype(np.float32).repeat(160)
    ref = check_plan(hm, x, (300, 100, 0, lo, hi, 2.0, 0.5, 0.0, 1, 0, 1), f"two values, ranks {lo} / {hi}")
    assert len(np.unique(ref.E)) == 2 and set(ref.levels[:2].tolist()) <= set(np.unique(ref.E).tolist())


def test_no_valid_frame_and_one_valid_frame(hm):
    nan = np.full(160 * 40 + 9, np.nan, dtype=np.float32)
    ref = check_plan(hm, nan, SMALL[:7] + (0.125,) + SMALL[8:], "all NaN")
    assert ref.levels.tolist() == [0, 0, 0.125] and ref.speech.all() and ref.regions.tolist() == [[0, 41]]
    one = nan.copy()
    one[160 * 17:160 * 18] = CR.noise(160, "one frame", amp=0.3)
    ref = check_plan(hm, one, (300, 100, 0) + SMALL[3:8] + (1, 0, 1), "one valid frame")
    assert int((~np.isnan(ref.E)).sum()) == 1 and ref.levels[0] == ref.levels[1] == ref.E[17]


# ---- shapes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames,n_pieces", [(300, 1), (301, 2)])
def test_a_region_of_max_frames_is_one_piece_and_one_frame_more_is_two(hm, frames, n_pieces):
    x = np.zeros(160 * 500, dtype=np.float32)
    x[160 * 100:160 * (100 + frames)] = CR.noise(160 * frames, ("region", frames), amp=0.3)
    ref = check_plan(hm, x, (300, 100, 0) + SMALL[3:8] + (1, 0, 1), f"a region of {frames} frames")
    assert ref.regions.tolist() == [[100, 100 + frames]] and len(ref.piece_starts) == n_pieces and len(ref.chunk_first) == n_pieces + 1


def test_noise_at_one_level_is_one_region_cut_like_a_recording(hm):
    x = VR.all_speech()
    ref = check_plan(hm, x, (300, 100, 15) + SMALL[3:], "all speech")
    assert ref.regions.tolist() == [[0, 701]] and ref.piece_starts.tolist() == [0, 160 * 295, 160 * 574] and ref.chunk_first.tolist() == [0, 1, 2, 3]
    starts, lens = hm.cut_plan(x, params=(300, 100, 15))
    assert starts.tolist() == ref.piece_starts.tolist() and lens.tolist() == ref.piece_lens.tolist()


def test_padding_wider_than_the_recording_and_the_shaping_signal(hm):
    x = VR.blips_and_gaps()
    ref = check_plan(hm, x, (300, 100, 0) + SMALL[3:], "blips and gaps")
    assert ref.regions.tolist() == [[7, 105], [125, 165], [295, 335]]
    ref = check_plan(hm, x, (300, 100, 0) + SMALL[3:8] + (5, 3000, 20), "pad 3000 on 400 frames")
    assert ref.regions.tolist() == [[0, 400]] and len(ref.piece_starts) == 2


def test_nan_and_infinity_are_kept_and_the_quiet_stretch_goes(hm):
    ref = check_plan(hm, VR.nan_inf_quiet(), SMALL, "NaN, inf, a quiet stretch")
    assert ref.regions.tolist() == [[0, 510], [550, 700]] and np.isfinite(ref.levels).all()


@pytest.mark.parametrize("seed", range(5))
def test_bursts_lose_frames_only_inside_pauses(hm, seed):
    x, pauses = CR.bursts(seed)
    ref = check_plan(hm, x, SMALL, f"bursts {seed}")
    _, speech, _, _ = hm.vad_view()
    gone = np.flatnonzero(speech == 0)
    print(f"seed {seed}: {len(gone)} frames dropped, {len(ref.regions)} regions, {len(ref.chunk_first) - 1} chunks")
    for f in gone:
        assert any(a <= 160 * f and 160 * (f + 1) <= b for a, b in pauses), f"frame {f} is dropped outside the pauses"
    for a, b in pauses:
        assert b - a < 8000 or ((gone >= -(-a // 160)) & (gone < b // 160)).any(), f"the pause at sample {a} loses nothing"


def test_the_defaults_on_70_seconds(hm):
    """pauses of 0.5 s are bridged by the default min_gap of 1 s; five seconds at the pauses' level are not"""
    x, _ = CR.bursts(7, 70.0)
    x[160 * 2000:160 * 2500] *= np.float32(1e-3 / 0.3)
    ref = check_plan(hm, x, None, "defaults")
    assert len(ref.regions) == 2 and len(ref.chunk_first) - 1 == 3 and 400 < len(ref.speech) - ref.speech.sum() < 500


# ---- memory and state ---------------------------------------------------------------------------------------------------------
def test_host_pcm_larger_than_one_staging_group(hm):
    """a recording three frames and five samples longer than one 256 MiB staging group: a period of 4099 frames of bursts and
    pauses repeated (W = 0), so the reference starts from one period's energies repeated"""
    period = CR.bursts(3, 4099 * 160 / 16000.0)[0]
    assert len(period) == 160 * 4099
    n = 160 * (STAGE_FRAMES + 3) + 5
    x = np.tile(period, n // len(period) + 1)[:n]
    params = (3000, 2000, 0) + VR.DEFAULTS[3:8] + (5, 5, 20)
    got = hm.vad_plan(x, params=params)
    F = CR.n_frames(n)
    E = np.tile(CR.energies(period, 0)[0], F // 4099 + 1)[:F].copy()
    E[F - 1] = CR.energies(x[160 * (F - 1):], 0)[0][0]
    ref = check_against(hm, VR.from_energies(E, n, params), "one staging group and a bit", got)
    assert len(ref.regions) > 1000 and ref.piece_lens.sum() < n


def test_host_and_device_memory_a_fresh_context_and_the_cut_planners_view(hm):
    x, _ = CR.bursts(11, 12.0)
    longer, _ = CR.bursts(12, 31.0)
    fresh = hip.HipWhisper(config.preset("test-d128"), device=0, max_batch=1)   # no tensors loaded: legal for a plan
    with pytest.raises(hip.HipError) as ei:
        fresh._vad_frames = 10
        fresh.vad_view()
    assert ei.value.code == STATE
    alone = fresh.vad_plan(x, params=SMALL)
    check_against(fresh, VR.plan(x, SMALL), "alone, on a context without weights", alone)
    fresh.close()
    hm.cut_plan(longer, params=(300, 100, 15))
    e0, E0 = hm.cut_energy()
    check_plan(hm, longer, SMALL, "longer")
    after = hm.vad_plan(x, params=SMALL)
    check_against(hm, VR.plan(x, SMALL), "after a longer recording", after)
    dev = hip.DeviceBuffer(x)
    from_dev = hm.vad_plan(dev.ptr, len(x), SMALL)
    check_against(hm, VR.plan(x, SMALL), "device memory", from_dev)
    dev.free()
    for got in (after, from_dev):
        assert all(g.tolist() == a.tolist() for g, a in zip(got, alone))
    e1, E1 = hm.cut_energy()
    assert same_bits(e0, e1) and same_bits(E0, E1), "the view of nh_cut_energy changed"


# ---- in front of the log-mel --------------------------------------------------------------------------------------------------
FIRST = [0, 1, 6, 8, 11, 13, 16]   # six rows: a one-piece chunk beside a five-piece chunk; the last row ends with the ragged piece


@pytest.fixture(scope="module")
def gathered(hm):
    """a recording whose last piece is ragged, its 16 pieces, and the log-mel of the six rows' numpy concatenations"""
    x = CR.bursts(21, 20.0)[0][:-37]
    p = VR.plan(x, SMALL)
    n = len(p.piece_starts)
    assert n >= 16 and p.piece_starts[n - 1] + p.piece_lens[n - 1] == len(x) and p.piece_lens[n - 1] % 160 == 123
    starts, lens = p.piece_starts[n - 16:].copy(), p.piece_lens[n - 16:].copy()
    rows = [np.concatenate([x[starts[j]:starts[j] + lens[j]] for j in range(FIRST[b], FIRST[b + 1])]) for b in range(6)]
    hm.logmel(rows)
    return x, starts, lens, [hm.get_mel(b) for b in range(6)]


@pytest.mark.parametrize("where", ["host", "device", "device, base off 16 bytes"])
def test_logmel_pieces_rows_is_logmel_of_the_concatenations(hm, gathered, where):
    x, starts, lens, want = gathered
    dev = None if where == "host" else hip.DeviceBuffer(x if where == "device" else np.concatenate([np.zeros(1, dtype=np.float32), x]))
    src = x if dev is None else dev.ptr + (0 if where == "device" else 4)   # + 4: the dword path
    hm.logmel([np.zeros(4000, dtype=np.float32)] * 6)   # what the rows held before
    hm.logmel_pieces_rows(src, starts, lens, FIRST[:4])
    assert hm.batch == 3
    for b in range(3):
        assert same_bits(hm.get_mel(b), want[b]), f"{where}: chunk {b}"
    hm.logmel_pieces_rows(src, starts, lens, FIRST[3:], row0=3)   # a second group behind the first, its pieces rebased
    assert hm.batch == 6
    for b in range(6):
        assert same_bits(hm.get_mel(b), want[b]), f"{where}: chunk {b} by rows"
    if dev is not None:
        dev.free()


# ---- the one-call form --------------------------------------------------------------------------------------------------------
def test_transcribe_speech_equals_the_existing_path_on_the_concatenations(hm, tk, script):
    x, _ = CR.bursts(31, 25.0)
    p = VR.plan(x, SMALL)
    n_chunks = len(p.chunk_first) - 1
    assert n_chunks > MAX_BATCH, "more than one group"
    clips = [VR.concatenation(x, p, k) for k in range(n_chunks)]
    keys = [-(-len(c) // 320) for c in clips]
    hm.align_capture(HEADS)
    direct = []
    for a in range(0, n_chunks, MAX_BATCH):
        hm.logmel(clips[a:a + MAX_BATCH])
        hm.encode()
        res = hm.decode_greedy()
        first, last = hm.align_decoded(n_keys=keys[a:a + MAX_BATCH])
        for i, r in enumerate(res):
            r.update(token_first=first[i].copy(), token_last=last[i].copy())
        direct += res
    dev = hip.DeviceBuffer(x)
    for what, got in (("aligned", longform.transcribe_speech(hm, x, SMALL, align=True)),
                      ("device memory", longform.transcribe_speech(hm, (dev.ptr, len(x)), SMALL, align=True)),
                      ("plain", longform.transcribe_speech(hm, x, SMALL))):
        assert len(got) == len(direct), what
        for k, (g, d) in enumerate(zip(got, direct)):
            assert g["tokens"] == d["tokens"] == [tk.sot, tk.en, tk.transcribe] + script, f"{what}: chunk {k}"
            assert f64_bits(g["avg_logprob"]) == f64_bits(d["avg_logprob"]) and f64_bits(g["no_speech_prob"]) == f64_bits(d["no_speech_prob"])
            assert (g["pieces"], g["n_samples"], g["n_keys"]) == (VR.chunk_pieces(p, k), len(clips[k]), keys[k])
            if what != "plain":
                assert np.array_equal(g["token_first"], d["token_first"]) and np.array_equal(g["token_last"], d["token_last"])
            else:
                assert "token_first" not in g
    dev.free()
    hm.align_capture([])
    # the scripted decode gives every chunk the script's two segments; each starts in its chunk's first piece
    segs = longform.stitch_speech(got, tk)
    assert len(segs) == 2 * len(got)
    first_ts = 320 * (script[0] - tk.no_timestamps - 1)
    assert [round(s[0], 6) for s in segs[::2]] == [round(longform.to_recording(g["pieces"], first_ts) / 16000, 6) for g in got]
    assert all(a[1] <= b[0] + 1e-9 for a, b in zip(segs[:-1], segs[1:]))


def test_a_silent_recording_and_a_final_chunk_of_one_sample(hm):
    assert longform.transcribe_speech(hm, np.zeros(160 * 900, dtype=np.float32), SMALL) == []
    x = np.zeros(160 * 330 + 1, dtype=np.float32)
    x[:160 * 300] = CR.noise(160 * 300, "short tail", amp=0.3)
    x[-1] = 0.5
    params = (300, 100, 0) + SMALL[3:8] + (1, 0, 1)
    ref = check_plan(hm, x, params, "a one-sample piece")
    assert ref.piece_lens.tolist() == [48000, 1] and ref.chunk_first.tolist() == [0, 1, 2]
    got = longform.transcribe_speech(hm, x, params)
    assert [g["n_samples"] for g in got] == [48000, 1] and [g["n_keys"] for g in got] == [150, 1]
    assert got[1]["pieces"] == [(0, 160 * 330, 1)]
    for k, g in enumerate(got):
        hm.logmel([VR.concatenation(x, ref, k)])
        hm.encode()
        d = hm.decode_greedy()[0]
        assert g["tokens"] == d["tokens"] and f64_bits(g["avg_logprob"]) == f64_bits(d["avg_logprob"])


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_and_the_view_of_the_plan_before_untouched(hm):
    L = hm.L
    x0, _ = CR.bursts(41, 6.0)
    x1, _ = CR.bursts(42, 25.0)
    before = check_plan(hm, x0, SMALL, "the plan before")
    starts, lens, first = np.full(8, -7, dtype=np.int64), np.full(8, -7, dtype=np.int32), np.full(5, -7, dtype=np.int32)
    n_p, n_c = C.c_int32(-7), C.c_int32(-7)

    def call(n=len(x1), cap_p=8, cap_c=4, **kw):
        v = dict(zip(("mx", "mn", "W", "lo", "hi", "lo_r", "hi_r", "floor", "speech", "pad", "gap"), SMALL))
        v.update(kw)
        q = hip.NhVadParams.of(tuple(v.values()))
        return L.nh_vad_plan(hm._h, x1.ctypes.data_as(C.c_void_p), 0, n, C.byref(q), starts.ctypes.data_as(I64), lens.ctypes.data_as(I32), cap_p,
                             C.byref(n_p), first.ctypes.data_as(I32), cap_c, C.byref(n_c))

    def untouched(name):
        assert (starts == -7).all() and (lens == -7).all() and (first == -7).all(), f"{name}: the outputs were written"
        hm._vad_frames = len(before.E)
        check_against(hm, before, f"{name}: the view of the plan before", (before.piece_starts, before.piece_lens, before.chunk_first))

    nan, inf = float("nan"), float("inf")
    refused = dict(no_samples=dict(n=0), negative=dict(n=-5), too_many=dict(n=2 ** 31), max_zero=dict(mx=0), max_over=dict(mx=3001),
                   min_zero=dict(mn=0), min_over_max=dict(mn=301), window_negative=dict(W=-1), window_over=dict(W=101),
                   lo_negative=dict(lo=-1), hi_over=dict(hi=1001), lo_over_hi=dict(lo=901), lo_ratio_negative=dict(lo_r=-1.0),
                   lo_ratio_nan=dict(lo_r=nan), hi_ratio_inf=dict(hi_r=inf), floor_nan=dict(floor=nan), floor_negative=dict(floor=-0.5),
                   speech_zero=dict(speech=0), speech_over=dict(speech=3001), pad_negative=dict(pad=-1), pad_over=dict(pad=3001),
                   gap_zero=dict(gap=0), gap_over=dict(gap=3001), cap_negative=dict(cap_p=-1))
    for name, kw in refused.items():
        assert call(**kw) == INVALID, name
        assert n_p.value == -7 and n_c.value == -7 and L.nh_last_error(hm._h), name
        untouched(name)
    # caps: the plan of x1 has more than 8 pieces in more than 4 chunks; the call says how many, and nothing else shows
    want = VR.plan(x1, SMALL)
    counts = (len(want.piece_starts), len(want.chunk_first) - 1)
    assert counts[0] > 8 and counts[1] > 4
    for name, kw in dict(both=dict(), pieces=dict(cap_c=counts[1]), chunks=dict(cap_p=counts[0], cap_c=0), none=dict(cap_p=0, cap_c=0)).items():
        if name == "chunks":
            starts, lens = np.full(counts[0], -7, dtype=np.int64), np.full(counts[0], -7, dtype=np.int32)
        if name == "pieces":
            first = np.full(counts[1] + 1, -7, dtype=np.int32)
        n_p.value = n_c.value = -7
        assert call(**kw) == INVALID and (n_p.value, n_c.value) == counts, name
        untouched(f"cap: {name}")
    # the view: too little room is refused with nothing written, NULL pointers are fine
    F = len(before.E)
    E, sp, reg, cnt = np.full(F, 7.5, dtype=np.float32), np.full(F, 7, dtype=np.uint8), np.full(2 * len(before.regions), -7, dtype=np.int64), C.c_int32(-7)
    assert L.nh_vad_view(hm._h, E.ctypes.data_as(F32), sp.ctypes.data_as(U8), F - 1, None, None, 0, None) == INVALID
    assert L.nh_vad_view(hm._h, E.ctypes.data_as(F32), None, F, None, reg.ctypes.data_as(I64), len(before.regions) - 1, C.byref(cnt)) == INVALID
    assert (E == 7.5).all() and (sp == 7).all() and (reg == -7).all() and cnt.value == len(before.regions)
    assert L.nh_vad_view(hm._h, None, None, 0, None, None, 0, None) == 0
    # vad_plan grows the caps by itself, and the successful plan becomes the view
    check_plan(hm, x1, SMALL, "after the refusals")
    # nh_logmel_pieces_rows
    hm.logmel([x0[:48000]])
    mel = hm.get_mel(0)

    def rows(st, ln, cf, batch=None, row0=0):
        st, ln, cf = np.array(st, dtype=np.int64), np.array(ln, dtype=np.int32), np.array(cf, dtype=np.int32)
        return L.nh_logmel_pieces_rows(hm._h, x1.ctypes.data_as(C.c_void_p), 0, st.ctypes.data_as(I64), ln.ctypes.data_as(I32), cf.ctypes.data_as(I32),
                                       len(cf) - 1 if batch is None else batch, row0)

    two = ([0, 16000], [1600, 1600])
    for name, args in dict(descending=(*two, [0, 2, 1]), no_piece=(*two, [0, 0, 2]), negative_first=(*two, [-1, 2]), empty_piece=([0, 16000], [1600, 0], [0, 2]),
                           negative_start=([0, -160], [1600, 1600], [0, 2]), too_long=([0, 0], [240000, 240001], [0, 2]),
                           short_beside_long=(*two[:1], [1600, 159], [0, 1, 2]), no_batch=(*two, [0, 2], 0), rows_over=(*two, [0, 2], MAX_BATCH + 1),
                           row_negative=(*two, [0, 2], None, -1), rows_past_the_end=(*two, [0, 1, 2], None, MAX_BATCH - 1)).items():
        assert rows(*args) == INVALID, name
    assert same_bits(hm.get_mel(0), mel), "the context's mel was touched"
    assert rows([0, 0], [240000, 240000], [0, 2]) == 0, "480 000 samples in two pieces fit a row"
