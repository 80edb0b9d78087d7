"""numpy reference of nh_cut_plan (include/norma_hip.h): frame energies and window energies in f32 with the
contract's additions in the contract's order -- numpy's f32 multiply and add are single IEEE operations, so every bit is
reproduced --, the sequential cut loop, float64 frame energies for the error bound, and the test signals the CPU and the
GPU tests share."""
import zlib

import numpy as np

HOP = 160
DEFAULTS = (3000, 2000, 15)   # max_frames, min_frames, half_window


def n_frames(n):
    return -(-int(n) // HOP)


def _framed(x, dtype):
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    F = n_frames(len(x))
    X = np.zeros(F * HOP, dtype=dtype)
    X[:len(x)] = x
    return X.reshape(F, HOP)


def energies(x, W):
    """(e, E) f32 [F]: 160 ordered adds of x * x per frame, then 2 W + 1 ordered adds per window (0.0f outside [0, F))"""
    X = _framed(x, np.float32)
    F = len(X)
    with np.errstate(all="ignore"):
        e = np.zeros(F, dtype=np.float32)
        for j in range(HOP):
            p = X[:, j] * X[:, j]
            e = e + p
        pad = np.zeros(F + 2 * W, dtype=np.float32)
        pad[W:W + F] = e
        E = np.zeros(F, dtype=np.float32)
        for k in range(2 * W + 1):
            E = E + pad[k:k + F]
    assert e.dtype == np.float32 and E.dtype == np.float32
    return e, E


def e64(x):
    """float64 frame energies"""
    X = _framed(x, np.float64)
    return (X * X).sum(axis=1)


def cuts(E, F, min_frames, max_frames, earliest=False, nan_least=False, short=0):
    """[s_0 = 0, s_1, ..]: the sequential loop of the contract.  The keyword arguments are the planted mistakes of
    tests/test_cut_cpu.py: the earliest minimum instead of the latest, a NaN comparing as least, a search range that ends
    `short` frames early."""
    s, out = 0, [0]
    while F - s > max_frames:
        best, c_star = np.float32(np.inf), s + max_frames
        for c in range(s + min_frames, s + max_frames - short + 1):
            v = E[c]
            if nan_least and np.isnan(v):
                take = True
            elif np.isnan(best):
                take = False
            else:
                take = bool(v < best) if earliest else bool(v <= best)
            if take:
                best, c_star = v, c
        s = c_star
        out.append(s)
    return out


def plan(x, params=DEFAULTS, **mistake):
    """(starts i64, lens i32, e, E) of a recording"""
    mx, mn, W = params
    n = len(x)
    e, E = energies(x, W)
    s = cuts(E, len(E), mn, mx, **mistake)
    starts = np.array([HOP * v for v in s], dtype=np.int64)
    ends = np.array([HOP * v for v in s[1:]] + [n], dtype=np.int64)
    return starts, np.minimum(ends - starts, n - starts).astype(np.int32), e, E


def noise(n, key, amp=0.1):
    """uniform noise whose squares are far from subnormal (|x| >= 2^-40 or exactly 0 is what the contract specifies);
    key: anything with a repr"""
    x = (np.random.default_rng(zlib.crc32(repr(key).encode())).uniform(-1.0, 1.0, size=n) * amp).astype(np.float32)
    x[np.abs(x) < 2.0 ** -40] = 0.0
    return x


# inputs named for a property; tests/test_cut_cpu.py checks that each has it (for the parameters {300, 100, 15})
def plateau():
    """noise with an exactly silent stretch: frames 150 .. 249 are zero, so E is exactly 0 on frames 165 .. 234"""
    x = noise(160 * 700, "plateau")
    x[160 * 150:160 * 250] = 0.0
    return x


def one_nan():
    """noise, quietest around frame 200 (interior to the first search range 100 .. 300), one NaN sample in frame 250"""
    x = noise(160 * 700, "nan")
    x[160 * 190:160 * 211] *= np.float32(0.01)
    x[160 * 250 + 5] = np.nan
    return x


def quiet_last_candidate():
    """noise, quietest at frame 300 = s + max_frames of the first search"""
    x = noise(160 * 700, "last")
    x[160 * 285:160 * 316] *= np.float32(0.01)
    return x


def nan_range():
    """noise with NaN samples in frames 85 .. 315: E is NaN on the whole first search range 100 .. 300"""
    x = noise(160 * 700, "nan range")
    x[160 * 85 + 3:160 * 316:160] = np.nan
    return x


def bursts(seed, seconds=20.0):
    """noise bursts of 0.2 .. 1.2 s at amplitude 0.3 separated by 0.5 s pauses at amplitude 1e-3; returns (x, pauses) with
    pauses = [(first sample, end sample)]"""
    r = np.random.default_rng([4242, seed])
    n = int(seconds * 16000)
    x = np.zeros(n, dtype=np.float32)
    pauses, at = [], 0
    while at < n:
        b = int(r.integers(3200, 19201))
        x[at:at + b] = r.uniform(-0.3, 0.3, size=len(x[at:at + b]))
        at += b
        if at >= n:
            break
        x[at:at + 8000] = r.uniform(-1e-3, 1e-3, size=len(x[at:at + 8000]))
        pauses.append((at, min(at + 8000, n)))
        at += 8000
    x[np.abs(x) < 2.0 ** -40] = 0.0
    return x, pauses


def cuts_in_pauses(starts, pauses, W):
    """every cut (a start but the first) lies at least W frames inside a pause"""
    return all(any(a + HOP * W <= c <= b - HOP * W for a, b in pauses) for c in starts[1:])
