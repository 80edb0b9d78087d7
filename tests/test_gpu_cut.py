"""GPU: cutting long recordings on the device (nh_cut_plan, nh_cut_energy, nh_logmel_chunks_rows, longform.transcribe_recording)
against the bit-exact numpy reference of tests/cut_ref.py and against the existing log-mel / encode / decode path, on a
test-d128 context.  The contract is in include/norma_hip.h and DESIGN.md 11; what the reference's rules catch is shown without
a GPU in tests/test_cut_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import common
import cut_ref as CR
from norma_amd import config, hip, longform

pytestmark = pytest.mark.gpu

TILE = 128           # NH_CUT_TILE: frames per workgroup of the energy kernel
STAGE_FRAMES = (256 << 20) // (4 * CR.HOP)   # frames per staging group of host PCM
MAX_BATCH = 6
SMALL = (300, 100, 15)
HEADS = [(0, 1), (1, 0)]
INVALID, STATE = 1, 3
I32, I64, F32 = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)


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


def check_plan(hm, x, params, what, src=None, n=None):
    """plan x on the device (src: what to hand to cut_plan instead of x) and compare every output with the reference"""
    starts, lens = hm.cut_plan(x if src is None else src, n, params)
    e, E = hm.cut_energy()
    rs, rl, re, rE = CR.plan(x, CR.DEFAULTS if params is None else params)
    assert same_bits(e, re), f"{what}: frame energies, first difference at frame {int(np.argmax(e.view(np.int32) != re.view(np.int32)))}"
    assert same_bits(E, rE), f"{what}: window energies, first difference at frame {int(np.argmax(E.view(np.int32) != rE.view(np.int32)))}"
    assert starts.dtype == np.int64 and lens.dtype == np.int32
    assert starts.tolist() == rs.tolist() and lens.tolist() == rl.tolist(), what
    return starts, lens, e, E


# ---- bit equality -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 159, 160, 161, 160 * (TILE - 1), 160 * TILE - 1, 160 * TILE, 160 * TILE + 1, 160 * 255 + 7, 160 * 256,
                               160 * 257 + 1, 160 * 1025 + 33, 320000 - 37])
def test_energies_and_cuts_equal_the_reference_bit_for_bit(hm, n):
    check_plan(hm, CR.noise(n, ("bits", n)), SMALL, f"{n} samples")


def test_window_of_one_frame_and_a_window_wider_than_the_recording(hm):
    x = CR.noise(160 * 700 + 11, "w0")
    _, _, e, E = check_plan(hm, x, (300, 100, 0), "W = 0")
    assert same_bits(e, E)
    check_plan(hm, CR.noise(160 * 40 - 3, "w100"), (300, 100, 100), "W = 100 on 40 frames")


def test_one_chunk_at_max_frames_and_two_one_frame_later(hm):
    a = check_plan(hm, CR.noise(160 * 300, "one"), SMALL, "F = max_frames")
    assert a[0].tolist() == [0] and a[1].tolist() == [48000]
    b = check_plan(hm, CR.noise(160 * 300 + 1, "two"), SMALL, "F = max_frames + 1")
    assert len(b[0]) == 2 and b[1].sum() == 48001


def test_defaults_on_70_seconds(hm):
    x, _ = CR.bursts(7, 70.0)
    starts, lens, _, _ = check_plan(hm, x, None, "defaults")
    assert len(starts) == 3 and (lens <= 480000).all() and (lens[:-1] >= 320000).all() and lens.sum() == len(x)


def test_host_pcm_larger_than_one_staging_group(hm):
    """the energies of a recording three frames and five samples longer than one 256 MiB staging group: a period of 4099
    frames of noise repeated, so the reference is one period's energies repeated"""
    period = CR.noise(160 * 4099, "period")
    n = 160 * (STAGE_FRAMES + 3) + 5
    x = np.tile(period, n // len(period) + 1)[:n]
    mx, mn = 3000, 2000
    starts, lens = hm.cut_plan(x, params=(mx, mn, 0))
    e, E = hm.cut_energy()
    F = CR.n_frames(n)
    ref = np.tile(CR.energies(period, 0)[0], F // 4099 + 1)[:F].copy()
    ref[F - 1] = CR.energies(x[160 * (F - 1):], 0)[0][0]
    assert same_bits(e, ref) and same_bits(E, ref)
    s = CR.cuts(ref, F, mn, mx)
    assert starts.tolist() == [160 * v for v in s] and lens.sum() == n and lens[-1] == n - starts[-1]


# ---- ties and NaN -------------------------------------------------------------------------------------------------------------
def test_silence_cuts_at_every_max_frames(hm):
    starts, lens, e, E = check_plan(hm, np.zeros(160 * 1000 + 33, dtype=np.float32), SMALL, "silence")
    assert starts.tolist() == [0, 48000, 96000, 144000] and not e.any() and not E.any()


def test_the_latest_frame_of_a_plateau_wins(hm):
    x = CR.plateau()
    E = CR.energies(x, 15)[1]
    assert (E[165:235] == 0).all() and (E[100:165] > 0).all() and (E[235:301] > 0).all()
    assert check_plan(hm, x, SMALL, "plateau")[0][1] == 160 * 234


def test_a_nan_sample_is_never_chosen(hm):
    x = CR.one_nan()
    E = CR.energies(x, 15)[1]
    assert np.isnan(E[235:266]).all() and not np.isnan(E[100:235]).any() and not np.isnan(E[266:301]).any()
    best = 100 + int(np.argmin(np.where(np.isnan(E[100:301]), np.inf, E[100:301])))
    assert 100 < best < 300
    assert check_plan(hm, x, SMALL, "one NaN")[0][1] == 160 * best


def test_an_all_nan_range_cuts_at_max_frames(hm):
    x = CR.nan_range()
    E = CR.energies(x, 15)[1]
    assert np.isnan(E[100:301]).all() and not np.isnan(E[400:]).any()
    starts = check_plan(hm, x, SMALL, "NaN range")[0]
    assert starts[1] == 160 * 300 and 160 * 400 <= starts[2] < 160 * 600
    nan = np.full(160 * 1000 + 33, np.nan, dtype=np.float32)
    assert check_plan(hm, nan, SMALL, "all NaN")[0].tolist() == [0, 48000, 96000, 144000]


# ---- cuts land in pauses ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
def test_cuts_land_in_pauses(hm, seed):
    x, pauses = CR.bursts(seed)
    starts, lens = hm.cut_plan(x, params=SMALL)
    print(f"seed {seed}: cuts at {[int(s) // 160 for s in starts[1:]]}")
    assert len(starts) >= 7 and (lens <= 48000).all() and lens.sum() == len(x)
    for c in starts[1:]:
        assert any(a + 160 * SMALL[2] <= c <= b - 160 * SMALL[2] for a, b in pauses), f"the cut at sample {c} is in no pause"


# ---- placement independence -------------------------------------------------------------------------------------------------
def test_host_and_device_memory_and_a_reused_workspace_give_the_same_bits(hm):
    x, _ = CR.bursts(11, 12.0)
    longer, _ = CR.bursts(12, 31.0)
    fresh = hip.HipWhisper(config.preset("test-d128"), device=0, max_batch=1)   # no tensors loaded: legal for a plan
    with pytest.raises(hip.HipError) as ei:
        fresh.cut_energy()
    assert ei.value.code == STATE
    alone = check_plan(fresh, x, SMALL, "alone, on a context without weights")
    fresh.close()
    check_plan(hm, longer, SMALL, "longer")
    after = check_plan(hm, x, SMALL, "after a longer recording")
    dev = hip.DeviceBuffer(x)
    from_dev = check_plan(hm, x, SMALL, "device memory", src=dev.ptr, n=len(x))
    dev.free()
    for got in (after, from_dev):
        assert got[0].tolist() == alone[0].tolist() and got[1].tolist() == alone[1].tolist()
        assert same_bits(got[2], alone[2]) and same_bits(got[3], alone[3])


# ---- in front of the log-mel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True])
def test_logmel_chunks_rows_is_logmel_of_the_slices(hm, on_device):
    x, _ = CR.bursts(21, 16.0)
    starts, lens = hm.cut_plan(x, params=SMALL)
    assert len(starts) >= 6
    slices = [x[s:s + n] for s, n in zip(starts[:6], lens[:6])]
    hm.logmel(slices)
    want = [hm.get_mel(b) for b in range(6)]
    dev = hip.DeviceBuffer(x) if on_device else None
    src = dev.ptr if on_device else x
    hm.logmel_chunks_rows(src, starts[:3], lens[:3])
    assert hm.batch == 3
    for b in range(3):
        assert same_bits(hm.get_mel(b), want[b]), f"chunk {b}"
    hm.logmel_chunks_rows(src, starts[3:6], lens[3:6], row0=3)   # a second group behind the first
    assert hm.batch == 6
    for b in range(6):
        assert same_bits(hm.get_mel(b), want[b]), f"chunk {b} by rows"
    if dev is not None:
        dev.free()


# ---- the one-call form ------------------------------------------------------------------------------------------------------
def test_transcribe_recording_equals_the_existing_path_on_the_same_slices(hm, tk, script):
    x, _ = CR.bursts(31, 25.0)
    starts, lens = hm.cut_plan(x, params=SMALL)
    assert len(starts) > MAX_BATCH, "more than one group"
    keys = [-(-int(n) // 320) for n in lens]
    hm.align_capture(HEADS)
    direct = []
    for a in range(0, len(starts), MAX_BATCH):
        hm.logmel([x[s:s + n] for s, n in zip(starts[a:a + MAX_BATCH], lens[a:a + MAX_BATCH])])
        hm.encode()
        res = hm.decode_greedy()
        first, last = hm.align_decoded(n_keys=keys[a:a + MAX_BATCH])
        for i, r in enumerate(res):
            r.update(token_first=first[i].copy(), token_last=last[i].copy())
        direct += res
    dev = hip.DeviceBuffer(x)
    for what, got in (("aligned", longform.transcribe_recording(hm, x, SMALL, align=True)),
                      ("device memory", longform.transcribe_recording(hm, (dev.ptr, len(x)), SMALL, align=True)),
                      ("plain", longform.transcribe_recording(hm, x, SMALL))):
        assert len(got) == len(direct), what
        for k, (g, d) in enumerate(zip(got, direct)):
            assert g["tokens"] == d["tokens"] == [tk.sot, tk.en, tk.transcribe] + script, f"{what}: chunk {k}"
            assert f64_bits(g["avg_logprob"]) == f64_bits(d["avg_logprob"]) and f64_bits(g["no_speech_prob"]) == f64_bits(d["no_speech_prob"])
            assert (g["start_sample"], g["n_samples"], g["n_keys"]) == (int(starts[k]), int(lens[k]), keys[k])
            if what != "plain":
                assert np.array_equal(g["token_first"], d["token_first"]) and np.array_equal(g["token_last"], d["token_last"])
                assert (g["token_first"][3:len(script) + 2] >= 0).all() and (g["token_last"] < keys[k]).all()
            else:
                assert "token_first" not in g
    dev.free()
    hm.align_capture([])
    # the scripted decode gives every chunk the script's two segments: on one axis they start a chunk apart
    segs = longform.stitch(got, tk)
    assert len(segs) == 2 * len(got)
    first_ts = 0.02 * (script[0] - tk.no_timestamps - 1)
    assert [round(s[0] - first_ts, 6) for s in segs[::2]] == [round(int(s) / 16000, 6) for s in starts]


def test_a_final_chunk_shorter_than_a_frame_is_submitted_alone(hm, tk, script):
    x = CR.noise(160 * 300 + 1, "short tail")
    x[160 * 280:] = 0.0    # the quietest window ends the recording: the cut falls on frame 300, the tail is one sample
    starts, lens = hm.cut_plan(x, params=SMALL)
    assert lens.tolist() == [48000, 1]
    got = longform.transcribe_recording(hm, x, SMALL)
    assert [g["n_samples"] for g in got] == [48000, 1] and [g["n_keys"] for g in got] == [150, 1]
    for k, g in enumerate(got):
        hm.logmel([x[starts[k]:starts[k] + lens[k]]])
        hm.encode()
        d = hm.decode_greedy()[0]
        assert g["tokens"] == d["tokens"] and f64_bits(g["avg_logprob"]) == f64_bits(d["avg_logprob"])


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_and_the_view_of_the_plan_before_untouched(hm):
    L = hm.L
    x0 = CR.noise(160 * 450 + 9, "before")
    x1 = CR.noise(160 * 3000 + 77, "refused")
    check_plan(hm, x0, SMALL, "the plan before")
    e0, E0 = hm.cut_energy()
    starts, lens, cnt = np.full(8, -7, dtype=np.int64), np.full(8, -7, dtype=np.int32), C.c_int32(-7)

    def call(n=len(x1), mx=300, mn=100, W=15, cap=8, params=True):
        q = hip.NhCutParams(mx, mn, W)
        return L.nh_cut_plan(hm._h, x1.ctypes.data_as(C.c_void_p), 0, n, C.byref(q) if params else None,
                             starts.ctypes.data_as(I64), lens.ctypes.data_as(I32), cap, C.byref(cnt))

    def untouched(name):
        assert (starts == -7).all() and (lens == -7).all(), f"{name}: the outputs were written"
        e, E = hm.cut_energy()
        assert same_bits(e, e0) and same_bits(E, E0), f"{name}: the view of the plan before changed"

    refused = dict(no_samples=dict(n=0), negative=dict(n=-5), too_many=dict(n=2 ** 31), max_zero=dict(mx=0), max_over=dict(mx=3001),
                   min_zero=dict(mn=0), min_over_max=dict(mn=301), window_negative=dict(W=-1), window_over=dict(W=101))
    for name, kw in refused.items():
        assert call(**kw) == INVALID, name
        assert cnt.value == -7 and L.nh_last_error(hm._h), name
        untouched(name)
    # cap: the plan of x1 has more chunks than 8; the call says how many, and nothing else shows
    want = CR.plan(x1, SMALL)
    assert len(want[0]) > 8
    assert call() == INVALID and cnt.value == len(want[0])
    untouched("cap")
    assert call(cap=0) == INVALID and cnt.value == len(want[0])
    untouched("cap 0")
    # the view: too little room is refused, NULL pointers are fine
    e = np.full(len(e0), 7.5, dtype=np.float32)
    assert L.nh_cut_energy(hm._h, e.ctypes.data_as(F32), None, len(e0) - 1) == INVALID and (e == 7.5).all()
    assert L.nh_cut_energy(hm._h, None, e.ctypes.data_as(F32), len(e0)) == 0 and same_bits(e, E0)
    assert L.nh_cut_energy(hm._h, None, None, len(e0)) == 0
    # cut_plan grows cap by itself, and the successful plan becomes the view
    got = check_plan(hm, x1, SMALL, "after the refusals")
    assert got[0].tolist() == want[0].tolist()
    # nh_logmel_chunks_rows
    hm.logmel([x0[:48000]])
    mel = hm.get_mel(0)
    st = np.zeros(MAX_BATCH + 1, dtype=np.int64)
    for name, (s0, n0, batch, row0) in dict(negative_start=(-1, 48000, 1, 0), empty=(0, 0, 1, 0), too_long=(0, 480001, 1, 0),
                                           no_batch=(0, 48000, 0, 0), rows_over=(0, 48000, MAX_BATCH + 1, 0), row_negative=(0, 48000, 1, -1),
                                           rows_past_the_end=(0, 48000, 2, MAX_BATCH - 1)).items():
        st[:] = s0
        ns = np.full(MAX_BATCH + 1, n0, dtype=np.int32)
        assert L.nh_logmel_chunks_rows(hm._h, x1.ctypes.data_as(C.c_void_p), 0, st.ctypes.data_as(I64), ns.ctypes.data_as(I32), batch, row0) == INVALID, name
    assert same_bits(hm.get_mel(0), mel), "the context's mel was touched"
