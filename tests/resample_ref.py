"""Float64 reference of the audio ingest contract (include/norma_hip.h): sample conversion, channel mixdown,
polyphase resampling to 16 kHz; the error bound of the device's f32 accumulation; a Python twin of nm_resample_plan.
Nothing here touches the GPU or the library."""
import math

import numpy as np

TARGET_HZ = 16000
ZERO_CROSSINGS, ROLLOFF, BETA = 32.0, 0.92, 8.6
N_SAMPLES = 480000
U = 2.0 ** -24        # unit roundoff of f32


# ---- step 3's filter ------------------------------------------------------------------------------------------------------
def design(src_hz):
    """(L, M, T, Wc, c, W) of a source rate; T == 0 at 16 kHz (no filter)"""
    g = math.gcd(TARGET_HZ, src_hz)
    L, M = TARGET_HZ // g, src_hz // g
    if src_hz == TARGET_HZ:
        return L, M, 0, 0, 1.0, 0.0
    c = ROLLOFF * (L / M if L < M else 1.0)
    W = ZERO_CROSSINGS / c
    Wc = int(math.ceil(W))
    return L, M, 2 * Wc, Wc, c, W


def h(u, c, W):
    """the prototype filter at offsets u (frames), float64: c sinc(c u) I0(beta sqrt(1 - (u/W)^2)) / I0(beta) inside |u| < W"""
    u = np.asarray(u, dtype=np.float64)
    inside = np.abs(u) < W
    r = np.where(inside, u / W, 0.0)
    win = np.i0(BETA * np.sqrt(1.0 - r * r)) / np.i0(BETA)
    return np.where(inside, c * np.sinc(c * u) * win, 0.0)


def table(src_hz, window=True, scale_cutoff=True):
    """coef[p][j] = h(p/L - k), k = j - Wc + 1, float64 [L][T].  window / scale_cutoff = False: the wrong variants"""
    L, M, T, Wc, c, W = design(src_hz)
    k = np.arange(T) - Wc + 1
    u = np.arange(L)[:, None] / L - k[None, :]
    if not scale_cutoff:
        c = ROLLOFF
    if not window:
        return np.where(np.abs(u) < W, c * np.sinc(c * u), 0.0)
    return h(u, c, W)


# ---- steps 1 and 2 -----------------------------------------------------------------------------------------------------
def convert32(x):
    """dasp_sample's conversion to f32 (exact in f32 for every type up to 24 bits; f64 and the wide integers round once)"""
    x = np.asarray(x)
    if x.dtype == np.float32:
        return x
    if x.dtype == np.float64:
        return x.astype(np.float32)
    bits = 8 * x.dtype.itemsize
    if x.dtype.kind == "u" and bits == 64:
        v = (x ^ np.uint64(1 << 63)).view(np.int64)
    elif x.dtype.kind == "u":
        v = x.astype(np.int64) - (1 << (bits - 1))
    else:
        v = x.astype(np.int64)
    return v.astype(np.float32) * np.float32(2.0 ** -(bits - 1))


def mono32(frames):
    """step 2 as the device does it: f32 additions in channel order, one f32 division.  frames [n][channels] or [n]"""
    s = convert32(frames)
    if s.ndim == 1:
        return s
    m = s[:, 0].copy()
    for ch in range(1, s.shape[1]):
        m = (m + s[:, ch]).astype(np.float32)
    return (m / np.float32(s.shape[1])).astype(np.float32) if s.shape[1] > 1 else m


def mono64(frames):
    """steps 1 and 2 in float64 (the conversion formulas are exact in float64 for every type the tests use)"""
    s = convert32(frames).astype(np.float64)
    return s if s.ndim == 1 else s.sum(axis=1) / s.shape[1]


# ---- step 3 -------------------------------------------------------------------------------------------------------------
def out_len(src_hz, n_frames):
    L, M = design(src_hz)[:2]
    return -(-n_frames * L // M)


def positions(src_hz, n_out, num0=0):
    """(i, p) of outputs 0 .. n_out - 1, exact integers"""
    L, M = design(src_hz)[:2]
    num = num0 + np.arange(n_out, dtype=np.int64) * M
    return num // L, num % L


def resample64(mono, src_hz, coef, num0=0, n_out=None, frame_shift=0, phase_shift=0, k_lo=0, k_hi=0, chunk=8192):
    """y[n] = sum_k coef[p][k] mono[i + k] in float64, and sum_k |coef[p][k] mono[i + k]| (what the bound is made of).
    coef: [L][T] (the device's f32 table, or table()).  frame_shift / phase_shift / k_lo / k_hi plant the wrong variants: the
    frame index or the phase off by one, the first k_lo or last k_hi taps dropped."""
    mono = np.asarray(mono, dtype=np.float64)
    L, M, T, Wc = design(src_hz)[:4]
    if n_out is None:
        n_out = out_len(src_hz, len(mono))
    i, p = positions(src_hz, n_out, num0)
    if T == 0:
        ok = (i >= 0) & (i < len(mono))
        y = np.where(ok, mono[np.clip(i, 0, len(mono) - 1)], 0.0)
        return y, np.abs(y)
    coef = np.asarray(coef, dtype=np.float64)
    p = (p + phase_shift) % L
    k = np.arange(T) - Wc + 1
    use = np.ones(T)
    use[:k_lo] = 0
    if k_hi:
        use[T - k_hi:] = 0
    y, sabs = np.zeros(n_out), np.zeros(n_out)
    for a in range(0, n_out, chunk):
        b = min(n_out, a + chunk)
        idx = i[a:b, None] + frame_shift + k[None, :]
        ok = (idx >= 0) & (idx < len(mono))
        g = np.where(ok, mono[np.clip(idx, 0, len(mono) - 1)], 0.0)
        t = coef[p[a:b]] * use[None, :] * g
        y[a:b], sabs[a:b] = t.sum(axis=1), np.abs(t).sum(axis=1)
    return y, sabs


def resample_bound(sabs, T):
    """|device - float64| per output for T fused multiply-adds of exact f32 operands into one f32 accumulator: every fmaf rounds
    its partial sum once (relative 2^-24), so the error is at most ((1 + u)^T - 1) sum |coef mono| <= (T + 2) u sum |coef mono| for
    T u << 1, plus the smallest subnormal for a result that underflows"""
    return (T + 2) * U * np.asarray(sabs) + 2.0 ** -149


def resample_f32(mono, src_hz, coef32, num0=0, n_out=None):
    """the device's accumulation emulated in numpy: acc = f32(coef * mono + acc), taps ascending.  (The product of two f32 is
    exact in float64; the sum rounds to 53 bits and then to 24, which differs from a true fmaf at rare double-rounding ties.)"""
    mono = np.asarray(mono, dtype=np.float32)
    L, M, T, Wc = design(src_hz)[:4]
    if n_out is None:
        n_out = out_len(src_hz, len(mono))
    i, p = positions(src_hz, n_out, num0)
    acc = np.zeros(n_out, dtype=np.float32)
    for j in range(T):
        idx = i + (j - Wc + 1)
        ok = (idx >= 0) & (idx < len(mono))
        g = np.where(ok, mono[np.clip(idx, 0, len(mono) - 1)], np.float32(0)).astype(np.float64)
        acc = (coef32[p, j].astype(np.float64) * g + acc.astype(np.float64)).astype(np.float32)
    return acc


def gain(coef, src_hz, f_hz):
    """H(f): what a tone of f_hz keeps of its amplitude, from a table [L][T] in float64, averaged over nothing: the polyphase rows
    are samples of ONE filter h at spacing 1/L, and H(f) = (1/L) sum over all of them of h(u) exp(-2 pi i f u / src_hz)"""
    L, M, T, Wc = design(src_hz)[:4]
    k = np.arange(T) - Wc + 1
    u = (np.arange(L)[:, None] / L - k[None, :]).ravel()
    return np.sum(np.asarray(coef, dtype=np.float64).ravel() * np.exp(-2j * np.pi * f_hz / src_hz * u)) / L


# ---- the streaming bookkeeping (twin of nm_resample_plan) --------------------------------------------------------------
def plan(src_hz, received, emitted, first_kept, final):
    """(n_ready, f0, num0, drop_before)"""
    L, M, T, Wc = design(src_hz)[:4]
    lo = Wc - 1 if Wc > 0 else 0
    usable = received if final else received - Wc
    total = -(-usable * L // M) if usable > 0 else 0
    n_ready = max(0, total - emitted)
    f0 = max(first_kept, emitted * M // L - lo)
    num0 = emitted * M - f0 * L
    drop = received if final else min(received, max(first_kept, (emitted + n_ready) * M // L - lo))
    return n_ready, f0, num0, drop
