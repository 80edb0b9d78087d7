"""GPU: launch_logmel_grp and launch_mel_finish_ex called directly (tools/kref.hip -> tools/bin/libnh_kref.so) and compared with
the fp64 reference of tests/kref.py ("log-mel") on the exact f32 inputs, and with rules that IEEE arithmetic makes exact.

The fp64 comparison is an interval, with no case excluded: the kernel's value must lie in
[log10 max(S - dS, 1e-10) - e, log10 max(S + dS, 1e-10) + e], dS derived from the kernel's arithmetic (kref.mel_bound), e the
documented error of the device log10f (kref.mel_interval).  tests/test_kref_cpu.py shows on the same data that an f32 emulation of
the kernel stays inside, that three plausible bugs do not, and that the broadband intervals are narrow.  Nothing here reads the C
oracle; the tests that agree with it bit for bit (test_gpu_parity.py) stay the product's contract next to these."""
import numpy as np
import pytest

import kref as K
from norma_amd import assets_io

pytestmark = pytest.mark.gpu

N_MEL = [80, 128]
PAD = 96                      # canary floats on either side of the mel32 window
_cache = {}


def _setup(n_mel):
    if n_mel not in _cache:
        filt = assets_io.mel_filters(n_mel)
        _cache[n_mel] = (K.mel_tables(), filt, K.mel_groups(filt))
    return _cache[n_mel]


def _pattern32(n, salt=0):
    """finite f32 canaries with distinct bits"""
    return (1.0e6 + ((np.arange(n, dtype=np.int64) * 7919 + salt) % 65521)).astype(np.float32)


def _pattern16(n, salt=0):
    return ((np.arange(n, dtype=np.int64) * 7919 + 13 + salt) & 0xFFFF).astype(np.uint16)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _launch(pcm, ns, frames, n_mel):
    """one launch into the middle of canaried buffers: checks the untouched memory and the chunk_max rule, returns
    (mel32 [B][n_mel][frames], chunk_max [B])"""
    t, filt, grp = _setup(n_mel)
    B = pcm.shape[0]
    n = B * n_mel * frames
    mel = np.concatenate([_pattern32(PAD), np.full(n, np.nan, np.float32), _pattern32(PAD, 5)])
    cm = np.array([0xDEADBEEF] + [0] * B + [0x12345678], dtype=np.uint32)      # own rows zero, as the product's memset leaves them
    before = mel.copy()
    K.logmel(pcm, ns, frames, t, filt, grp, mel32=mel, mel_off=PAD, chunk_max=cm, cm_off=1)
    assert np.array_equal(_bits(mel[:PAD]), _bits(before[:PAD])) and np.array_equal(_bits(mel[PAD + n:]), _bits(before[PAD + n:])), \
        "mel32 outside [B][n_mel][frames] was written"
    assert cm[0] == 0xDEADBEEF and cm[-1] == 0x12345678, "chunk_max of other rows was written"
    got = mel[PAD:PAD + n].reshape(B, n_mel, frames)
    assert not np.isnan(got).any(), "a live output was not written"
    # chunk_max == the ordered encoding of the maximum of the kernel's own outputs, bit for bit
    assert np.array_equal(cm[1:1 + B], K.f32_ordered(got.max(axis=(1, 2)))), (cm[1:1 + B], got.max(axis=(1, 2)))
    return got, cm[1:1 + B].copy()


def _decode_ordered(u):
    u = np.asarray(u, dtype=np.uint32)
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("n_mel", N_MEL)
@pytest.mark.parametrize("family", K.MEL_FAMILIES)
def test_logmel_lies_in_its_fp64_interval(family, n_mel):
    t, filt, grp = _setup(n_mel)
    worst, narrow, total = 0.0, 0, 0
    for frames in K.MEL_FRAMES:
        for B in ((1, 3, 4) if family == "noise-0.1" else (1, 3)):
            pcm, ns = K.mel_case(family, frames, B)
            lo, hi, ref = K.mel_reference(pcm, ns, frames, t, filt, grp)
            got, cm = _launch(pcm, ns, frames, n_mel)
            worst = max(worst, K.mel_inside(got, lo, hi, f"{family} n_mel={n_mel} frames={frames} B={B}", ref))
            narrow += int(((hi - lo) < 1e-3).sum()); total += lo.size
            if family == "noise-3e-4":
                # every log negative, the maximum above the floor: the negative branch of the encoding.  (A narrow filter's sum
                # is close to exponentially distributed, so about one output in 10^4 does fall to the 1e-10 floor.)
                assert (got < 0).all() and (got > -10).mean() > 0.99 and (got.max(axis=(1, 2)) > -10).all() and (cm < 0x80000000).all()
                assert np.array_equal(_bits(_decode_ordered(cm)), _bits(got.max(axis=(1, 2))))
            if family in ("burst", "dc", "square"):
                assert (cm > 0x80000000).all() and (got.max(axis=(1, 2)) > 0).all()      # a positive maximum
    print(f"{family} n_mel={n_mel}: largest |got - ref| / half-width = {worst:.4f}; "
          f"{100 * narrow / total:.2f} % of the intervals narrower than 1e-3")
    if family in K.MEL_BROADBAND:
        assert narrow >= 0.99 * total, (narrow, total)


@pytest.mark.parametrize("n_mel", N_MEL)
def test_logmel_of_silence_is_exactly_minus_ten(n_mel):
    """all-zero clips, and clips of length 0 whose buffer holds the canary: every value -10, chunk_max its encoding"""
    for frames in K.MEL_FRAMES:
        for B in (1, 3):
            stride = K.mel_full_length(frames) + 67
            pcm = np.zeros((B, stride), np.float32)
            ns = np.full(B, K.mel_full_length(frames), np.int32)
            if B == 3:
                pcm[1] = K.MEL_CANARY; ns[1] = 0
                pcm[2] = -0.0
            got, cm = _launch(pcm, ns, frames, n_mel)
            assert np.array_equal(_bits(got), _bits(np.full_like(got, -10.0))), (frames, B)
            assert (cm == K.f32_ordered(np.float32(-10.0))).all()


@pytest.mark.parametrize("n_mel", N_MEL)
def test_logmel_one_nan_sample_blanks_exactly_its_frames(n_mel):
    frames, B = 33, 3
    pcm, ns = K.mel_case("noise-0.1", frames, B)
    ns[:] = K.mel_full_length(frames)
    pcm = K.f32(0.1 * np.random.default_rng(7).standard_normal(pcm.shape))
    base, _ = _launch(pcm, ns, frames, n_mel)
    for b, p in ((1, 5 * 160 + 37), (0, 0), (2, K.mel_full_length(frames) - 1), (1, 16 * 160 + 399)):
        bad = pcm.copy(); bad[b, p] = np.nan
        got, _ = _launch(bad, ns, frames, n_mel)
        hit = np.zeros((B, frames), bool)
        f = np.arange(frames)
        hit[b] = (160 * f <= p) & (p < 160 * f + 400)
        assert hit.any()
        m = np.broadcast_to(hit[:, None, :], got.shape)
        assert np.array_equal(_bits(got[m]), _bits(np.full(int(m.sum()), -10.0, np.float32))), (b, p)
        assert np.array_equal(_bits(got[~m]), _bits(base[~m])), (b, p)


# Impulses: a reference that involves no FFT.  One clip of 1600 frames with unit samples more than 400 apart, so that every
# frame holds at most one impulse, at a known offset o; then S_m = hann_o^2 sum_k w_k f[m][k] (kref.mel_impulse_expected).
# "642j": a unit sample at 641 j + j.  Frame starts are multiples of 160 and 642 j = 2 j (mod 160), so this reaches only the
# even offsets; "641j" (frame 4 j holds its impulse at offset j, and so do the frames before it at j + 160 and j + 320) reaches
# all 400, which the test asserts: every input position, into every bin, with the right weight.
@pytest.mark.parametrize("n_mel", N_MEL)
@pytest.mark.parametrize("step", [642, 641], ids=["642j", "641j"])
def test_logmel_impulses_reach_every_bin_with_the_right_weight(step, n_mel):
    t, filt, grp = _setup(n_mel)
    frames = 1600
    full = K.mel_full_length(frames)
    pos = step * np.arange(400)
    assert pos[-1] < full
    pcm = np.zeros((1, full + 64), np.float32)
    pcm[0, pos] = 1.0
    pcm[0, full:] = K.MEL_CANARY
    ns = np.array([full], np.int32)
    start = 160 * np.arange(frames)
    j = np.searchsorted(pos, start)                                    # the first impulse at or after the frame's start
    has = (j < 400) & (pos[np.minimum(j, 399)] < start + 400)
    off = np.where(has, pos[np.minimum(j, 399)] - start, 0)
    assert ((pcm[0, start[:, None] + np.arange(400)[None, :]] != 0).sum(axis=1) == has).all()     # at most one, where expected
    seen = np.unique(off[has])
    assert seen.size == (400 if step == 641 else 200), seen.size
    S, dS = K.mel_impulse_expected(off, t, filt)
    S[~has] = 0.0
    lo, hi = K.mel_interval(S, dS)
    got, _ = _launch(pcm, ns, frames, n_mel)
    K.mel_inside(got[0].T, lo, hi, f"impulses {step} j, n_mel={n_mel}")
    dev = np.abs(K.d64(got[0].T) - np.log10(np.maximum(S, K.MEL_FLOOR))).max()
    print(f"impulses {step} j n_mel={n_mel}: largest |got - log10 S| = {dev:.3e} (widest interval {np.max(hi - lo):.3e})")


@pytest.mark.parametrize("n_mel", N_MEL)
def test_logmel_bits_do_not_depend_on_where_a_frame_sits(n_mel):
    """the same 400 samples at frame 0, frame 5 (another wave) and frame 16 (another workgroup), in clip 0 and clip 2, and a
    second identical launch"""
    frames, B = 33, 3
    r = np.random.default_rng(11)
    seg = K.f32(0.1 * r.standard_normal(400))
    full = K.mel_full_length(frames)
    pcm = np.zeros((B, full + 67), np.float32)
    pcm[1] = K.f32(0.1 * r.standard_normal(full + 67))
    for b in (0, 2):
        for f in (0, 5, 16):
            pcm[b, 160 * f:160 * f + 400] = seg
    ns = np.full(B, full, np.int32)
    got, cm = _launch(pcm, ns, frames, n_mel)
    want = _bits(got[0, :, 0])
    assert got[0, :, 0].max() > -10
    for b in (0, 2):
        for f in (0, 5, 16):
            assert np.array_equal(_bits(got[b, :, f]), want), (b, f)
    again, cm2 = _launch(pcm, ns, frames, n_mel)
    assert np.array_equal(_bits(again), _bits(got)) and np.array_equal(cm, cm2)


def _finish_data(r, n_mel, frames, m):
    """mel32 of one clip in [-10, 4] with the values at which the rule can go wrong planted: exact ties at m - 8, -0.0, values
    whose result is halfway between two fp16 neighbours, values in the fp16 subnormal range (and halfway between two of those)"""
    v = r.uniform(-10.0, 4.0, size=(n_mel, frames)).astype(np.float32)
    m8 = np.float32(m) - np.float32(8.0)
    special = np.array([m8, np.nextafter(m8, np.float32(4)), np.nextafter(m8, np.float32(-10)), -0.0, 0.0, -10.0, 4.0,
                        2.0 ** -9,                       # / 4 + 1 = 1 + 2^-11: halfway between fp16 1 and 1 + 2^-10 (tie to even)
                        3 * 2.0 ** -9,                   # 1 + 3 * 2^-11: halfway, the odd neighbour below
                        1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,     # the same halves for normalise = 0
                        2.0 ** -25, 3 * 2.0 ** -25, 5 * 2.0 ** -25, -3 * 2.0 ** -25,   # halves between fp16 subnormals
                        5e-8, 1e-6, -3e-7, 6.1e-5, 2.0 ** -14, 2.0 ** -24,            # fp16 subnormals, the smallest normal
                        -4.0, np.nextafter(np.float32(-4), np.float32(0))], dtype=np.float32)
    flat = v.reshape(-1)
    idx = r.permutation(flat.size)[:min(special.size, flat.size)]
    flat[idx] = special[:idx.size]
    return v


@pytest.mark.parametrize("normalise", [1, 0])
@pytest.mark.parametrize("frames", [1, 31, 32, 33, 70])
@pytest.mark.parametrize("n_mel", N_MEL)
def test_mel_finish_is_the_f32_rule_and_leaves_the_rest_alone(n_mel, frames, normalise):
    """two clips in the middle of buffers that hold four: max(v, m - 8) / 4 + 1 in f32 (or nothing) bit for bit, the image its
    astype(float16) at [b][t + 1][c], every other byte as it was"""
    r = np.random.default_rng(1000 * n_mel + 10 * frames + normalise)
    B, NB = 2, 4
    maxima = np.array([9.0, 2.5, -1.0, 9.0], np.float32)
    mel = np.stack([_finish_data(r, n_mel, frames, maxima[b]) for b in range(NB)])
    cm = K.f32_ordered(maxima)
    img = _pattern16(NB * (frames + 2) * 128).reshape(NB, frames + 2, 128)
    mel0, cm0, img0 = mel.copy(), cm.copy(), img.copy()
    K.mel_finish(mel.reshape(-1), n_mel * frames, cm, 1, img.reshape(-1), (frames + 2) * 128, B, n_mel, frames, normalise)
    assert np.array_equal(cm, cm0)
    want = mel0.copy()
    if normalise:
        m8 = (maxima - np.float32(8.0))[:, None, None]
        want[1:3] = (np.maximum(mel0, m8) / np.float32(4.0) + np.float32(1.0))[1:3]
        assert want.dtype == np.float32
        assert (mel0[1:3] < m8[1:3]).any() and (mel0[1:3] == m8[1:3]).any()
    assert np.array_equal(_bits(mel), _bits(want)), "mel32"
    want_img = img0.copy()
    want_img[1:3, 1:frames + 1, :n_mel] = want[1:3].astype(np.float16).view(np.uint16).transpose(0, 2, 1)
    assert np.array_equal(img, want_img), "conv1 image"
    # what the comparison above includes, spelled out: rows 0 and frames + 1, the pad columns, the other clips
    assert np.array_equal(img[:, 0], img0[:, 0]) and np.array_equal(img[:, frames + 1], img0[:, frames + 1])
    assert np.array_equal(img[:, :, n_mel:], img0[:, :, n_mel:]) and np.array_equal(img[[0, 3]], img0[[0, 3]])


@pytest.mark.parametrize("n_mel", N_MEL)
def test_finish_clamps_the_quiet_frames_of_a_burst(n_mel):
    """logmel -> finish on the tone burst followed by near-silence: the max - 8 clamp engages on the kernel's own output, and the
    finish is still the f32 rule bit for bit"""
    frames, B = 33, 3
    pcm, ns = K.mel_case("burst", frames, B)
    got, cm = _launch(pcm, ns, frames, n_mel)
    m8 = (got.max(axis=(1, 2)) - np.float32(8.0))[:, None, None]
    assert ((got < m8).mean(axis=(1, 2)) > 0.5).all(), "the clamp does not engage on this data"
    want = np.maximum(got, m8) / np.float32(4.0) + np.float32(1.0)
    mel = got.copy()
    img = _pattern16(B * (frames + 2) * 128).reshape(B, frames + 2, 128)
    img0 = img.copy()
    K.mel_finish(mel.reshape(-1), 0, cm, 0, img.reshape(-1), 0, B, n_mel, frames, 1)
    assert np.array_equal(_bits(mel), _bits(want))
    img0[:, 1:frames + 1, :n_mel] = want.astype(np.float16).view(np.uint16).transpose(0, 2, 1)
    assert np.array_equal(img, img0)
