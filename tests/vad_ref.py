"""numpy reference of nh_vad_plan (include/norma_hip.h) on top of cut_ref.energies and cut_ref.cuts: the levels
(an order statistic of the non-NaN window energies, two f32 products and two selects), the raw flags, the three shaping steps on
runs of frames, regions, pieces and the greedy chunks, and the time map back to the recording.  Every float step is a single f32
operation and everything else is integer, so the device has to reproduce every bit.  The keyword arguments are the planted
mistakes of tests/test_vad_cpu.py.  Also the test signals the CPU and the GPU tests share."""
import types
import zlib

import numpy as np

import cut_ref as CR

HOP = CR.HOP
#           max   min   W   lo   hi   lo_ratio hi_ratio floor speech pad gap
DEFAULTS = (3000, 2000, 15, 100, 900, 4.0, 0.01, 0.0, 10, 20, 100)
SMALL = (300, 100, 5, 100, 900, 4.0, 0.01, 0.0, 5, 5, 20)


def with_shaping(params, min_speech, pad, min_gap):
    return tuple(params[:8]) + (min_speech, pad, min_gap)


def levels(E, lo_permille, hi_permille, lo_ratio, hi_ratio, abs_floor, admit_nan=False, take_max=False):
    """f32 [3] = Q_lo, Q_hi, T.  admit_nan: the NaN frames stay in the statistic (numpy sorts them last); take_max: the larger
    of the two ratios' levels instead of the smaller"""
    E = np.asarray(E, dtype=np.float32)
    S = np.sort(E if admit_nan else E[~np.isnan(E)])
    n = len(S)
    floor = np.float32(abs_floor)
    if n == 0:
        return np.array([0, 0, floor], dtype=np.float32)
    q_lo, q_hi = S[int(lo_permille) * (n - 1) // 1000], S[int(hi_permille) * (n - 1) // 1000]
    with np.errstate(all="ignore"):
        a = np.float32(lo_ratio) * q_lo
        b = np.float32(hi_ratio) * q_hi
        assert a.dtype == np.float32 and b.dtype == np.float32
        if take_max:
            r = b if b > a else a
        else:
            r = b if b < a else a
        T = r if r > floor else floor
    return np.array([q_lo, q_hi, T], dtype=np.float32)


def flags(E, T, strict=False):
    """raw[f] = !(E[f] <= T): a NaN frame is speech.  strict: E < T in place of E <= T"""
    with np.errstate(all="ignore"):
        return ~(E < T) if strict else ~(E <= T)


def runs(v):
    """[(a, b)]: the maximal runs [a, b) of true values, ascending"""
    d = np.diff(np.concatenate(([0], np.asarray(v, dtype=np.int8), [0])))
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def shape(raw, min_speech, pad, min_gap, dilate_first=False, gap_le=False, fill_leading=False):
    """v3 of the contract.  dilate_first: (b) before (a); gap_le: a gap of exactly min_gap frames is filled too; fill_leading:
    silence in front of the first speech is a gap like any other"""
    F = len(raw)

    def short_runs_cleared(v):
        out = np.zeros(F, dtype=bool)
        for a, b in runs(v):
            if b - a >= min_speech:
                out[a:b] = True
        return out

    def dilated(v):
        out = np.zeros(F, dtype=bool)
        for a, b in runs(v):
            out[max(0, a - pad):min(F, b + pad)] = True
        return out

    v2 = short_runs_cleared(dilated(raw)) if dilate_first else dilated(short_runs_cleared(raw))
    v3 = v2.copy()
    for a, b in runs(~v2):
        inner = (a > 0 or fill_leading) and b < F
        if inner and v2.any() and (b - a <= min_gap if gap_le else b - a < min_gap):
            v3[a:b] = True
    return v3


def regions(v3):
    return np.array(runs(v3), dtype=np.int64).reshape(-1, 2)


def pieces(reg, E, n, max_frames, min_frames):
    """(starts i64 in samples, lens i32 in samples, frames per piece): every region, cut by cut_ref.cuts where it is longer
    than max_frames"""
    starts, lens, frames = [], [], []
    for a, b in np.asarray(reg).reshape(-1, 2).tolist():
        s = [a + c for c in CR.cuts(E[a:b], b - a, min_frames, max_frames)] + [b]
        for s0, s1 in zip(s[:-1], s[1:]):
            starts.append(HOP * s0)
            lens.append(min(HOP * (s1 - s0), n - HOP * s0))
            frames.append(s1 - s0)
    return np.array(starts, dtype=np.int64), np.array(lens, dtype=np.int32), frames


def chunks(frames, max_frames, pack_lt=False):
    """chunk_first i32 [n_chunks + 1].  pack_lt: a chunk takes a piece only while its total stays below max_frames"""
    first, held = [], 0
    for j, f in enumerate(frames):
        fits = held + f < max_frames if pack_lt else held + f <= max_frames
        if held == 0 or not fits:
            first.append(j)
            held = 0
        held += f
    return np.array(first + [len(frames)], dtype=np.int32)


def plan(x, params=DEFAULTS, **mistake):
    """everything nh_vad_plan and nh_vad_view return: E, levels, raw, speech (u8), regions, piece_starts, piece_lens,
    piece_frames, chunk_first"""
    return from_energies(CR.energies(x, params[2])[1], len(x), params, **mistake)


def from_energies(E, n, params, **mistake):
    """plan, from the window energies of a recording of n samples"""
    mx, mn, _, lo, hi, lo_r, hi_r, floor, min_speech, pad, min_gap = params
    pick = lambda *names: {k: v for k, v in mistake.items() if k in names}
    assert set(mistake) <= {"admit_nan", "take_max", "strict", "dilate_first", "gap_le", "fill_leading", "pack_lt"}
    lv = levels(E, lo, hi, lo_r, hi_r, floor, **pick("admit_nan", "take_max"))
    raw = flags(E, lv[2], **pick("strict"))
    v3 = shape(raw, min_speech, pad, min_gap, **pick("dilate_first", "gap_le", "fill_leading"))
    reg = regions(v3)
    starts, lens, frames = pieces(reg, E, n, mx, mn)
    return types.SimpleNamespace(E=E, levels=lv, raw=raw, speech=v3.astype(np.uint8), regions=reg, piece_starts=starts, piece_lens=lens,
                                 piece_frames=frames, chunk_first=chunks(frames, mx, **pick("pack_lt")))


def chunk_pieces(p, k):
    """[(offset_in_chunk, start_sample, n_samples)] of chunk k of a plan"""
    out, off = [], 0
    for j in range(int(p.chunk_first[k]), int(p.chunk_first[k + 1])):
        out.append((off, int(p.piece_starts[j]), int(p.piece_lens[j])))
        off += int(p.piece_lens[j])
    return out


def concatenation(x, p, k):
    return np.concatenate([x[s:s + n] for _, s, n in chunk_pieces(p, k)])


def to_recording(pieces_, tau, end=False, swapped=False):
    """the contract of longform.to_recording, by cases.  swapped: the start rule for ends and the end rule for starts"""
    if swapped:
        end = not end
    last_off, last_start, last_n = pieces_[-1]
    if tau > last_off + last_n or (tau == last_off + last_n and not end):
        return last_start + last_n
    for off, start, n in pieces_:
        inside = off < tau <= off + n if end else off <= tau < off + n
        if inside:
            return start + (tau - off)
    return pieces_[0][1]   # an end at 0


def dropped_frames(p):
    return np.flatnonzero(p.speech == 0)


# ---- signals ------------------------------------------------------------------------------------------------------------------
def loguniform(n, key):
    """every frame at its own amplitude, drawn log-uniformly from 2^-18 .. 1; samples below 2^-40 are zeroed.  The window
    energies then spread over many binades: every byte of the select's key has work"""
    r = np.random.default_rng(zlib.crc32(repr(key).encode()))
    F = CR.n_frames(n)
    amp = np.exp2(r.uniform(-18.0, 0.0, size=F)).repeat(HOP)[:n]
    x = (r.uniform(-1.0, 1.0, size=n) * amp).astype(np.float32)
    x[np.abs(x) < 2.0 ** -40] = 0.0
    return x


def all_speech():
    """noise at one level throughout: the quiet decile x 4 lies above every frame, the loud decile - 20 dB below every frame"""
    return CR.noise(160 * 700 + 11, "allspeech", amp=0.3)


def nan_inf_quiet():
    """noise with one NaN sample (frame 100), one sample of 3e38 (frame 300: E = +inf around it) and frames 500 .. 559 scaled
    by 1e-3"""
    x = CR.noise(160 * 700, "nan inf quiet", amp=0.3)
    x[160 * 100 + 7] = np.nan
    x[160 * 300 + 9] = np.float32(3e38)
    x[160 * 500:160 * 560] *= np.float32(1e-3)
    return x


def many_nans():
    """all_speech with every sample of frames 0 .. 139 NaN (a fifth of the frames) and frames 400 .. 459 scaled by 0.2: 14 dB
    down, inside the 20 dB the right levels keep"""
    x = all_speech().copy()
    x[:160 * 140] = np.nan
    x[160 * 400:160 * 460] *= np.float32(0.2)
    return x


def blips_and_gaps():
    """silence with speech runs placed for the shaping rules at {min_speech 5, pad 5, min_gap 20} and W = 0: a 3-frame blip
    (cleared first, or kept when dilation comes first), two runs 29 frames apart (a gap of 19 after padding: filled), two
    runs 30 frames apart (a gap of exactly 20: kept), and 12 frames of leading silence (7 after padding: shorter than
    min_gap, never filled)"""
    x = np.zeros(160 * 400, dtype=np.float32)
    for a, b in ((12, 40), (69, 100), (130, 160), (250, 253), (300, 330)):
        x[160 * a:160 * b] = CR.noise(160 * (b - a), ("blips", a), amp=0.3)
    return x
