"""GPU: audio ingest on the device (nh_resample, nh_logmel_resampled_rows, host.Resampler, Model.transcribe_frames) against
the float64 reference and the bound of tests/resample_ref.py, on a test-d128 context.  The contract is in include/norma_hip.h
and DESIGN.md 10; what the bound catches is shown without a GPU in tests/test_resample_cpu.py."""
import ctypes as C
import zlib

import numpy as np
import pytest

import common
import resample_ref as RR
from norma_amd import assets_io, config, hip, host, synth

pytestmark = pytest.mark.gpu

TILE = 2048          # NH_RS_TILE: outputs per workgroup
MAX_BATCH = 6
RATES = (48000, 44100, 22050, 8000)
KINDS = ("stereo i16", "mono f32", "stereo u8")


def rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def clip_lengths(src_hz):
    """1, 257, 3001, 5000 frames, and one clip of TILE + 1 outputs (5000 frames stay inside one tile when downsampling)"""
    L, M = RR.design(src_hz)[:2]
    n = (TILE + 1) * M // L
    while RR.out_len(src_hz, n) < TILE + 1:
        n += 1
    return [1, 257, 3001, 5000, n]


def random_clip(kind, n, *key):
    r = rng(kind, n, *key)
    if kind == "stereo i16":
        return r.integers(-32768, 32768, size=(n, 2)).astype(np.int16)
    if kind == "stereo u8":
        return r.integers(0, 256, size=(n, 2)).astype(np.uint8)
    return r.uniform(-1, 1, size=n).astype(np.float32)


def pack(clips):
    """[B][max frames][channels] (or [B][max frames]) and the frame counts"""
    n = [len(c) for c in clips]
    buf = np.zeros((len(clips), max(n)) + clips[0].shape[1:], dtype=clips[0].dtype)
    for b, c in enumerate(clips):
        buf[b, :len(c)] = c
    return buf, n


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


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


_tables = {}


def device_table(hm, src_hz):
    if src_hz not in _tables:
        _tables[src_hz] = hm.resample_table(src_hz)[0]
    return _tables[src_hz]


def check_against_fp64(hm, got, clip, src_hz, what, num0=0):
    coef = device_table(hm, src_hz)
    T = RR.design(src_hz)[2]
    ref, sabs = RR.resample64(RR.mono64(clip), src_hz, coef, num0=num0, n_out=len(got))
    bound = RR.resample_bound(sabs, T)
    err = np.abs(got.astype(np.float64) - ref)
    worst = int(np.argmax(err / bound))
    print(f"{what}: {len(got)} outputs, uses at most {(err / bound).max():.3f} of the bound")
    assert (err <= bound).all(), f"{what}: output {worst} is off by {err[worst]:.3e}, bound {bound[worst]:.3e}"


# ---- the table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_hz", RATES + (11025, 96000))
def test_table_is_f32_of_h(hm, src_hz):
    coef, L, M, T = hm.resample_table(src_hz)
    assert (L, M, T) == RR.design(src_hz)[:3] and coef.shape == (L, T)
    ref = RR.table(src_hz).astype(np.float32)
    ulp = np.spacing(np.abs(ref))
    assert (np.abs(coef.astype(np.float64) - ref.astype(np.float64)) <= ulp).all(), "more than one f32 ulp from f32(h)"
    assert hm.resample_table(16000)[1:] == (1, 1, 0)


# ---- steps 1 and 2 alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [2, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.int16, np.uint8])
def test_mono_stage_is_bit_exact_at_16k(hm, dtype, channels):
    r = rng("mono", np.dtype(dtype).name, channels)
    clips = []
    for n in clip_lengths(16000):
        if dtype == np.float32:
            clips.append(r.uniform(-1, 1, size=(n, channels)).astype(np.float32))
        else:
            info = np.iinfo(dtype)
            clips.append(r.integers(info.min, info.max + 1, size=(n, channels)).astype(dtype))
    buf, n = pack(clips)
    out = hm.resample(buf, 16000, n_frames=n)
    for b, c in enumerate(clips):
        assert same_bits(out[b], RR.mono32(c)), f"clip {b} ({n[b]} frames)"


# ---- step 3 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("src_hz", RATES)
def test_outputs_within_bound_of_fp64(hm, src_hz, kind):
    clips = [random_clip(kind, n, src_hz) for n in clip_lengths(src_hz)]
    buf, n = pack(clips)
    out = hm.resample(buf, src_hz, n_frames=n)
    for b, c in enumerate(clips):
        assert len(out[b]) == RR.out_len(src_hz, n[b])
        check_against_fp64(hm, out[b], c, src_hz, f"{src_hz} Hz {kind} clip {b} ({n[b]} frames)")


@pytest.mark.parametrize("src_hz", RATES)
def test_impulses_near_both_ends(hm, src_hz):
    """a single 1.0 in silence returns the coefficient rows: every tap shows (tests/test_resample_cpu.py), at the clip's edges
    too, where part of the window lies outside the clip"""
    clips = []
    for n in clip_lengths(src_hz)[2:]:
        for at in (0, 2, n - 3, n - 1):
            c = np.zeros(n, dtype=np.float32)
            c[at] = 1.0
            clips.append(c)
    for g in range(0, len(clips), MAX_BATCH):
        buf, n = pack(clips[g:g + MAX_BATCH])
        out = hm.resample(buf, src_hz, n_frames=n)
        for b, c in enumerate(clips[g:g + MAX_BATCH]):
            check_against_fp64(hm, out[b], c, src_hz, f"{src_hz} Hz impulse at {int(np.argmax(c))} of {len(c)}")
            assert out[b].any()


def test_clip_at_the_cap(hm):
    """30 s at 48 000 Hz mono i16 -> 480 000 outputs, the most a row holds"""
    clip = rng("cap").integers(-32768, 32768, size=1440000).astype(np.int16)
    out = hm.resample(clip[None, :], 48000)[0]
    assert len(out) == 480000
    check_against_fp64(hm, out, clip, 48000, "cap")


@pytest.mark.parametrize("src_hz", RATES + (16000,))
def test_shifted_window_gives_the_whole_clip_values(hm, src_hz):
    L, M, T, Wc = RR.design(src_hz)[:4]
    clip = random_clip("stereo i16", 5000, "win", src_hz)
    whole = hm.resample(clip[None], src_hz)[0]
    n_all = len(whole)
    for a, b, slack in ((0, 40, 0), (n_all // 3, n_all // 3 + 700, 3), (n_all - 300, n_all, 0), (n_all - 1, n_all, 1)):
        lo = max(Wc - 1, 0)
        f_lo = max(0, a * M // L - lo - slack)
        f_hi = min(len(clip), (b - 1) * M // L + Wc + 1 + slack)
        got = hm.resample(clip[None, f_lo:f_hi], src_hz, num0=[a * M - f_lo * L], n_out=[b - a])[0]
        assert np.array_equal(got, whole[a:b]), f"outputs [{a}, {b}) from frames [{f_lo}, {f_hi})"


# ---- determinism ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_hz,kind", [(44100, "stereo i16"), (48000, "stereo u8"), (8000, "mono f32")])
def test_bit_identity_alone_in_batch_host_and_device(hm, src_hz, kind):
    clips = [random_clip(kind, n, "det", src_hz) for n in clip_lengths(src_hz)]
    buf, n = pack(clips)
    batch = hm.resample(buf, src_hz, n_frames=n)
    for b, c in enumerate(clips):
        assert same_bits(hm.resample(c[None], src_hz)[0], batch[b]), f"clip {b} alone"
    dev = hip.DeviceBuffer(buf)    # the same bytes in HBM
    ch = 1 if buf.ndim == 2 else buf.shape[2]
    from_dev = hm.resample(dev.ptr, src_hz, n_frames=n, stride_frames=buf.shape[1], dtype=buf.dtype, channels=ch)
    for b in range(len(clips)):
        assert same_bits(from_dev[b], batch[b]), f"clip {b} from device memory"
    dev.free()


# ---- one staging for every host-fed route ---------------------------------------------------------------------------------------
def test_one_staging_serves_resample_cut_plan_and_logmel_samples(hm):
    """one fresh context, its calls back to back: resample (makes the staging), cut_plan of a recording larger than that
    staging (grows it), logmel_samples and a resample right behind it with no synchronise in between (the second copy lands
    where the first kernel reads), then the view of the plan.  Every result equals the same call on device-memory input or
    on f32 host input, neither of which is staged."""
    cfg = config.preset("test-d128")
    stereo = random_clip("stereo i16", 3001, "staging")
    rec = rng("staging", "recording").uniform(-0.5, 0.5, size=80000 + 37).astype(np.float32)   # about 5 s, 27 times the 3001 frames
    mono = np.stack([random_clip("stereo i16", 5000, "staging", k)[:, 0] for k in range(2)])
    cut = (300, 100, 15)
    d_stereo, d_rec = hip.DeviceBuffer(stereo), hip.DeviceBuffer(rec)
    want_rs = hm.resample(d_stereo.ptr, 48000, n_frames=[3001], stride_frames=3001, dtype=np.int16, channels=2)[0]
    want_plan = hm.cut_plan(d_rec.ptr, len(rec), cut)
    want_e = hm.cut_energy()
    hm.logmel_array(np.ascontiguousarray(mono.astype(np.float32) / np.float32(32768)))
    want_mel = [hm.get_mel(b) for b in range(2)]
    d_stereo.free()
    d_rec.free()
    one = hip.HipWhisper(cfg, device=0, max_batch=2)
    one.set_mel_filters(assets_io.mel_filters(cfg.num_mel_bins))
    first = one.resample(stereo[None], 48000)[0]
    plan = one.cut_plan(rec, params=cut)
    one.logmel_samples(np.ascontiguousarray(mono))
    again = one.resample(stereo[None], 48000)[0]
    e, E = one.cut_energy()
    mel = [one.get_mel(b) for b in range(2)]
    one.close()
    assert len(want_rs) == 1001 and same_bits(first, want_rs) and same_bits(again, want_rs)
    assert len(plan[0]) >= 2 and plan[0].tolist() == want_plan[0].tolist() and plan[1].tolist() == want_plan[1].tolist()
    assert same_bits(e, want_e[0]) and same_bits(E, want_e[1]), "cut_energy is not the view of the plan"
    for b in range(2):
        assert same_bits(mel[b], want_mel[b]), f"log-mel of clip {b}"


# ---- tones ------------------------------------------------------------------------------------------------------------------------
def test_analytic_tones(hm):
    """tones sampled analytically at 48 kHz come out as their analytic 16 kHz samples, up to the filter's own gain error at
    each tone (from the device's table, float64) and the accumulation bound; a 10 kHz tone on top leaves less than -86 dB"""
    src_hz, n = 48000, 9600
    L, M, T, Wc, c, W = RR.design(src_hz)
    coef = device_table(hm, src_hz)
    tones = [(0.3, 440.0, 0.1), (0.2, 3000.0, 1.3), (0.1, 6000.0, 2.9)]
    t48, t16 = np.arange(n) / 48000.0, np.arange(n // 3) / 16000.0
    x48 = sum(A * np.cos(2 * np.pi * f * t48 + ph) for A, f, ph in tones)
    x16 = sum(A * np.cos(2 * np.pi * f * t16 + ph) for A, f, ph in tones)
    gain_err = sum(A * abs(RR.gain(coef, src_hz, f) - 1.0) for A, f, _ in tones)
    inner = (np.arange(n // 3) * 3 > W) & (np.arange(n // 3) * 3 < n - 1 - W)
    A10 = 0.25
    with10 = x48 + A10 * np.cos(2 * np.pi * 10000.0 * t48 + 0.7)
    out = hm.resample(np.stack([x48, with10]).astype(np.float32), src_hz)
    for b, (x, extra) in enumerate(((x48, 0.0), (with10, A10 * 10 ** (-86 / 20)))):
        sabs = RR.resample64(x.astype(np.float32), src_hz, coef)[1]
        allowed = gain_err + extra + RR.resample_bound(sabs, T)
        err = np.abs(out[b].astype(np.float64) - x16)
        print(f"tones{' + 10 kHz' if b else ''}: worst error {err[inner].max():.3e}, allowed {allowed[inner].min():.3e} (gain term {gain_err:.3e})")
        assert inner.sum() > 3000 and (err[inner] <= allowed[inner]).all()


# ---- in front of the log-mel ------------------------------------------------------------------------------------------------------
def test_logmel_resampled_is_logmel_of_the_resampled_clips(hm, tk, script):
    src_hz = 44100
    clips = [random_clip("stereo i16", n, "mel") // 8 for n in (600, 3001, 5000)]
    buf, n = pack(clips)
    pcm = hm.resample(buf, src_hz, n_frames=n)
    hm.logmel(pcm)
    want = [hm.get_mel(b) for b in range(3)]
    hm.encode()
    want_tokens = [r["tokens"] for r in hm.decode_greedy()]
    assert want_tokens[0] == [tk.sot, tk.en, tk.transcribe] + script
    hm.logmel_resampled(buf, src_hz, n_frames=n)
    for b in range(3):
        assert same_bits(hm.get_mel(b), want[b]), f"clip {b}"
    hm.encode()
    assert [r["tokens"] for r in hm.decode_greedy()] == want_tokens
    # rows: two clips, then the third behind them
    hm.logmel_resampled_rows(buf[:2], src_hz, 0, n_frames=n[:2])
    hm.logmel_resampled_rows(buf[2:], src_hz, 2, n_frames=n[2:])
    for b in range(3):
        assert same_bits(hm.get_mel(b), want[b]), f"clip {b} by rows"
    hm.encode_rows(0, 3)
    assert [r["tokens"] for r in hm.decode_greedy()] == want_tokens


# ---- streaming ------------------------------------------------------------------------------------------------------------------
def _host_model(tk, script):
    cfg = config.preset("test-d128")
    over = common.scripted_overrides(cfg, tk, script)
    d = host.Definition(host.ModelType.TinyEn, host.SelectedDevice.Rocm(0))
    return d, lambda: d.blocking_try_to_model(cfg, tk, tk.en, tk.transcribe,
                                              ((n, a.astype(np.float16)) for n, a in synth.synth_weights(cfg, 0, over)))


@pytest.mark.parametrize("src_hz", [44100, 16000])
def test_streaming_resampler_equals_the_whole_clip(hm, tk, script, src_hz):
    clip = random_clip("stereo i16", 5000, "stream", src_hz)
    whole = hm.resample(clip[None], src_hz)[0]
    _, make = _host_model(tk, script)
    model = make()
    for piece in (1, 160, 4799, 5000):
        rs = host.Resampler(model, src_hz, 2, np.int16)
        got = []
        for a in range(0, 5000, piece):
            got.append(rs.push(clip[a:a + piece], final=a + piece >= 5000))
            if a + piece < 5000:
                st = rs.state()
                assert st["received"] == a + piece and st["emitted"] == sum(len(g) for g in got) and st["kept"] <= RR.design(src_hz)[2] + piece
        got = np.concatenate(got)
        assert np.array_equal(got, whole), f"pieces of {piece}"
        assert rs.state() == dict(received=0, emitted=0, kept=0), "final resets"
        rs.close()
    model.close()


def test_transcribe_frames_in_pieces_equals_transcribe_on_the_resampled_stream(hm, tk, script):
    src_hz, n = 48000, 144000
    t = np.arange(n) / src_hz
    tone = 0.2 * np.sin(2 * np.pi * 330.0 * t) + 0.1 * np.sin(2 * np.pi * 2500.0 * t)
    frames = np.stack([tone, 0.5 * tone], axis=1)
    frames = np.round(frames * 32767).astype(np.int16)
    whole = hm.resample(frames[None], src_hz)[0]
    d, make = _host_model(tk, script)
    d.set_input_format(src_hz, 2)
    a, b = make(), make()
    cuts = [0, 20000, 70000, n]
    received = emitted = first_kept = 0
    for i in range(3):
        final = i == 2
        segs = a.transcribe_frames(frames[cuts[i]:cuts[i + 1]], final_chunk=final)
        received = cuts[i + 1]
        n_ready, _, _, first_kept = RR.plan(src_hz, received, emitted, first_kept, final)
        want = b.transcribe(whole[emitted:emitted + n_ready], final_chunk=final)
        emitted += n_ready
        assert segs == want and a.buffered_samples == b.buffered_samples, f"piece {i}"
    assert emitted == len(whole) == 48000
    a.close()
    b.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(hm):
    L = hm.L
    clip = random_clip("stereo i16", 3001, "refuse")
    hm.logmel([synth.synth_pcm(0, 48000)])
    hm.encode()
    before = hm.decode_greedy()
    mel = hm.get_mel(0)
    out = np.full((MAX_BATCH, 2048), 7.5, dtype=np.float32)
    i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)

    def call(dt=3, ch=2, hz=48000, nf=3001, batch=1, num0=None, n_out=None):
        nfa = np.full(max(batch, 1), nf, dtype=np.int32)
        z = None if num0 is None else np.full(max(batch, 1), num0, dtype=np.int64)
        no = None if n_out is None else np.full(max(batch, 1), n_out, dtype=np.int32)
        return L.nh_resample(hm._h, clip.ctypes.data_as(C.c_void_p), 0, dt, ch, hz, nfa.ctypes.data_as(i32), 0, batch,
                             None if z is None else z.ctypes.data_as(i64), None if no is None else no.ctypes.data_as(i32),
                             out.ctypes.data_as(C.POINTER(C.c_float)), out.shape[1])

    refused = dict(unknown_type=dict(dt=10), negative_type=dict(dt=-1), no_channels=dict(ch=0), nine_channels=dict(ch=9),
                   rate_low=dict(hz=7999), rate_high=dict(hz=192001), table_too_large=dict(hz=191999), no_frames=dict(nf=0),
                   too_long=dict(nf=1440001), n_out_zero=dict(n_out=0), n_out_over=dict(n_out=480001), num0_negative=dict(num0=-1),
                   no_batch=dict(batch=0), batch_over=dict(batch=MAX_BATCH + 1))
    for name, kw in refused.items():
        assert call(**kw) == 1, name
        assert (out == 7.5).all(), f"{name}: the output buffer was written"
        assert L.nh_last_error(hm._h), name
    nfa = np.full(2, 3001, dtype=np.int32)
    for name, (hz, batch, row0) in dict(rows_over=(48000, 2, MAX_BATCH - 1), row_negative=(48000, 1, -1), rate=(7999, 1, 0)).items():
        assert L.nh_logmel_resampled_rows(hm._h, clip.ctypes.data_as(C.c_void_p), 0, 3, 2, hz, nfa.ctypes.data_as(i32), 0, batch, row0) == 1, name
    assert call() == 0 and not (out[0, :1001] == 7.5).any() and (out[0, 1001:] == 7.5).all() and (out[1:] == 7.5).all()
    assert same_bits(hm.get_mel(0), mel), "the context's mel was touched"
    after = hm.decode_greedy()
    assert after[0]["tokens"] == before[0]["tokens"]
    assert np.float64(after[0]["avg_logprob"]).view(np.int64) == np.float64(before[0]["avg_logprob"]).view(np.int64)
    assert np.float64(after[0]["no_speech_prob"]).view(np.int64) == np.float64(before[0]["no_speech_prob"]).view(np.int64)


def test_refused_logmel_calls_queue_nothing(hm):
    """every host-fed route into the PCM rows, refused for unequal mel frames (100 samples beside 48000), for a zero-length
    clip and -- where the call has a row0 -- for a row gap: the mel of the batch before, what it decodes to, and the
    captured sequences of its lockstep decode (align_decoded) are what they were"""
    L = hm.L
    vp, i32, i64, f32 = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
    pcm = np.stack([synth.synth_pcm(k, 48000) for k in range(2)]).astype(np.float32)
    other = np.ascontiguousarray(pcm[::-1] * np.float32(0.5))     # what a refused call would leave in the rows
    other16 = np.round(other * 32767).astype(np.int16)
    frames48 = np.ascontiguousarray(np.repeat(other16, 3, axis=1)[:, :, None].repeat(2, axis=2))   # [2][144000][2]
    starts = np.array([0, 48000], dtype=np.int64)

    def ns(lens, scale=1):
        return (np.asarray(lens, dtype=np.int32) * scale).ctypes.data_as(i32)

    calls = {
        "logmel_array": lambda lens, row0: L.nh_logmel(hm._h, other.ctypes.data_as(f32), ns(lens), 48000, len(lens)),
        "logmel_array_rows": lambda lens, row0: L.nh_logmel_rows(hm._h, other.ctypes.data_as(f32), ns(lens), 48000, len(lens), row0),
        "logmel_samples": lambda lens, row0: L.nh_logmel_samples(hm._h, other16.ctypes.data_as(vp), 3, ns(lens), 48000, len(lens)),
        "logmel_chunks_rows": lambda lens, row0: L.nh_logmel_chunks_rows(hm._h, other.ctypes.data_as(vp), 0, starts.ctypes.data_as(i64),
                                                                         ns(lens), len(lens), row0),
        "logmel_resampled_rows": lambda lens, row0: L.nh_logmel_resampled_rows(hm._h, frames48.ctypes.data_as(vp), 0, 3, 2, 48000,
                                                                               ns(lens, 3), 144000, len(lens), row0),
    }
    hm.align_capture([(0, 1), (1, 0)])
    try:
        hm.logmel_array(pcm)
        mel = [hm.get_mel(b) for b in range(2)]
        hm.encode()
        tokens = [r["tokens"] for r in hm.decode_greedy()]
        first, last = hm.align_decoded()
        assert (first >= 0).any()
        for name, call in calls.items():
            cases = [("unequal mel frames", [100, 48000], 0, 1), ("a zero-length clip", [48000, 0], 0, 1)]
            if name.endswith("_rows"):
                cases.append(("a row gap", [48000], 4, 3))
            for why, lens, row0, status in cases:
                what = f"{name} refused for {why}"
                assert call(lens, row0) == status and L.nh_last_error(hm._h), what
                f, l = hm.align_decoded()
                assert np.array_equal(f, first) and np.array_equal(l, last), what
                for b in range(2):
                    assert same_bits(hm.get_mel(b), mel[b]), what
                hm.encode()
                assert [r["tokens"] for r in hm.decode_greedy()] == tokens, what
    finally:
        hm.align_capture([])
