"""GPU, kernel level: the ragged form of prefill_attn_kernel (k_prefill.hip) that a decode pool's prefixes go through
(nh_pool_prefix), by way of tools/kref.hip's kref_prefill_self_attention_ragged / kref_prefill_cross_attention_ragged.

One launch holds clips of T = 1, 16, 17, 64, 65 and 223 positions -- one query, one wave against two, one key block against two,
the longest prefix of a decode -- packed back to back (offsets 0, 1, 17, 34, 98, 163: off the multiples of 16), their caches in
a non-identity choice of context rows.  Every clip is held against kref.prefill_attention in fp64 within kref.prefill_bound
(nothing fitted: the bound of the uniform tests), and bit for bit against the uniform launch of that clip alone.  Canaries
(7.25, -3.5) fill what the launch must leave alone: the caches of the context rows no clip names, the cache slots past a
clip's own T, the out rows past the packed ones."""
import ctypes as C

import numpy as np
import pytest

import kref as K

pytestmark = pytest.mark.gpu

H, CTX = 2, 448
D = 64 * H
TS = (1, 16, 17, 64, 65, 223)
ROWS = (5, 0, 7, 2, 6, 3)          # context row of every clip; rows 1 and 4 of the 8 belong to nobody
CACHE_ROWS, PAD_ROWS = 8, 3
OFFS = tuple(int(o) for o in np.cumsum((0,) + TS[:-1]))
M = sum(TS)


def _lib():
    L = K.lib()
    vp, i, l = C.c_void_p, C.c_int, C.c_long
    L.kref_prefill_self_attention_ragged.restype = L.kref_prefill_cross_attention_ragged.restype = C.c_int
    L.kref_prefill_self_attention_ragged.argtypes = [vp, vp, vp, l, vp, l, vp, vp, vp, i, i, i, i, i]
    L.kref_prefill_cross_attention_ragged.argtypes = [vp, l, vp, vp, vp, l, vp, i, i, i, i, i]
    return L


def _table(rows=ROWS, ts=TS, offs=OFFS):
    return np.ascontiguousarray([[r, t, o, 0] for r, t, o in zip(rows, ts, offs)], dtype=np.int32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _rng(*key):
    return np.random.default_rng([20, 7] + [int(k) for k in key])


def test_ragged_self_attention_every_clip_in_its_own_rows_and_cache_row():
    L = _lib()
    r = _rng(1)
    q, k, v = (K.f16(r.standard_normal((M + PAD_ROWS, D))) for _ in range(3))
    out = np.full((M + PAD_ROWS, D), np.float16(7.25), np.float16)
    ck = np.full((CACHE_ROWS, H, CTX, 64), np.float16(7.25), np.float16)
    cv = np.full((CACHE_ROWS, H, CTX, 64), np.float16(-3.5), np.float16)
    tab = _table()
    rc = L.kref_prefill_self_attention_ragged(K.ptr(q), K.ptr(k), K.ptr(v), D, K.ptr(out), D, K.ptr(ck), K.ptr(cv), K.ptr(tab),
                                              len(TS), M + PAD_ROWS, CACHE_ROWS, H, CTX)
    K.check_rc(rc, "ragged launch_prefill_self_attention")
    assert np.all(out[M:] == np.float16(7.25)), "out rows past the packed ones were written"
    for row in set(range(CACHE_ROWS)) - set(ROWS):
        assert np.all(ck[row] == np.float16(7.25)) and np.all(cv[row] == np.float16(-3.5)), f"the cache of context row {row}, which no clip names, was written"
    for row, T, off in zip(ROWS, TS, OFFS):
        what = f"ragged self T={T} row={row} off={off}"
        qi, ki, vi = (np.ascontiguousarray(a[off:off + T]) for a in (q, k, v))
        ref, sabs, vst, n = K.prefill_attention(qi, ki, vi, 1, T, H, T, True)
        bound = K.prefill_bound(ref, sabs, n, vst, floor=K.prefill_p16_floor(qi, ki, vi, 1, T, H, T, True))
        print(what, "worst |err| / bound", K.violation(ref, bound, out[off:off + T]))
        K.within(out[off:off + T], ref, bound, what)
        for name, cache, src, canary in (("ck", ck, ki, 7.25), ("cv", cv, vi, -3.5)):
            want = K.head_major(src.reshape(1, T, D), H)[0]
            assert np.array_equal(_bits(cache[row, :, :T]), _bits(want)), f"{what}: {name} slots 0..T-1 are not the clip's rows"
            assert np.all(cache[row, :, T:] == np.float16(canary)), f"{what}: {name} written past slot T-1"
        # the uniform launch of that clip alone: the same bits
        o1 = np.full((T, D), np.float16(7.25), np.float16)
        ck1 = np.full((1, H, CTX, 64), np.float16(7.25), np.float16)
        cv1 = np.full((1, H, CTX, 64), np.float16(-3.5), np.float16)
        K.check_rc(L.kref_prefill_self_attention(K.ptr(qi), K.ptr(ki), K.ptr(vi), D, K.ptr(o1), D, K.ptr(ck1), K.ptr(cv1), 1, T, H, CTX), what)
        assert np.array_equal(_bits(out[off:off + T]), _bits(o1)), f"{what}: not the bits of the uniform launch"
        assert np.array_equal(_bits(ck[row]), _bits(ck1[0])) and np.array_equal(_bits(cv[row]), _bits(cv1[0]))


@pytest.mark.parametrize("S", (1500, 65))
def test_ragged_cross_attention_reads_the_cross_cache_of_the_clips_row(S):
    L = _lib()
    r = _rng(2, S)
    q = K.f16(r.standard_normal((M + PAD_ROWS, D)))
    ck, cv = K.f16(r.standard_normal((CACHE_ROWS, H, S, 64))), K.f16(r.standard_normal((CACHE_ROWS, H, S, 64)))
    out = np.full((M + PAD_ROWS, D), np.float16(7.25), np.float16)
    ck2, cv2, tab = ck.copy(), cv.copy(), _table()
    rc = L.kref_prefill_cross_attention_ragged(K.ptr(q), D, K.ptr(ck2), K.ptr(cv2), K.ptr(out), D, K.ptr(tab), len(TS), M + PAD_ROWS,
                                               CACHE_ROWS, H, S)
    K.check_rc(rc, f"ragged launch_prefill_cross_attention S={S}")
    assert np.all(out[M:] == np.float16(7.25)), "out rows past the packed ones were written"
    assert np.array_equal(_bits(ck2), _bits(ck)) and np.array_equal(_bits(cv2), _bits(cv)), "the cross K/V were written"
    for row, T, off in zip(ROWS, TS, OFFS):
        what = f"ragged cross S={S} T={T} row={row} off={off}"
        qi = np.ascontiguousarray(q[off:off + T])
        ku, vu = K.pf_from_head_major(ck[row:row + 1], 1, H, S), K.pf_from_head_major(cv[row:row + 1], 1, H, S)
        ref, sabs, vst, n = K.prefill_attention(qi, ku, vu, 1, T, H, S, False)
        bound = K.prefill_bound(ref, sabs, n, vst, floor=K.prefill_p16_floor(qi, ku, vu, 1, T, H, S, False))
        # the neighbouring context row's keys are another answer altogether: the row map matters to the bound
        other = (row + 1) % CACHE_ROWS
        wrong = K.prefill_attention(qi, K.pf_from_head_major(ck[other:other + 1], 1, H, S), K.pf_from_head_major(cv[other:other + 1], 1, H, S),
                                    1, T, H, S, False, stats=False)[0]
        K.discriminates(ref, bound, {"the cross K/V of the next context row": wrong})
        print(what, "worst |err| / bound", K.violation(ref, bound, out[off:off + T]))
        K.within(out[off:off + T], ref, bound, what)
        o1 = np.full((T, D), np.float16(7.25), np.float16)
        c1, v1 = np.ascontiguousarray(ck[row:row + 1]), np.ascontiguousarray(cv[row:row + 1])
        K.check_rc(L.kref_prefill_cross_attention(K.ptr(qi), D, K.ptr(c1), K.ptr(v1), K.ptr(o1), D, 1, T, H, S), what)
        assert np.array_equal(_bits(out[off:off + T]), _bits(o1)), f"{what}: not the bits of the uniform launch"


def test_ragged_launches_refuse_tables_that_leave_their_buffers():
    """the wrapper's own bounds check, which stands in front of every launch above: nothing is launched, nothing written"""
    L = _lib()
    q = K.f16(np.zeros((40, D)))
    out = np.full((40, D), np.float16(7.25), np.float16)
    ck = np.full((2, H, CTX, 64), np.float16(7.25), np.float16)
    cv = ck.copy()
    for rows, ts, offs in (((2,), (8,), (0,)),          # context row outside the caches
                           ((0,), (41,), (0,)),         # more positions than packed rows
                           ((0,), (8,), (33,)),         # the clip's rows run past the buffer
                           ((0, 1), (8, 8), (0, 7)),    # two clips share a packed row
                           ((0, 0), (8, 8), (0, 8)),    # two clips share a cache row
                           ((0,), (0,), (0,))):
        tab = _table(rows, ts, offs)
        rc = L.kref_prefill_self_attention_ragged(K.ptr(q), K.ptr(q), K.ptr(q), D, K.ptr(out), D, K.ptr(ck), K.ptr(cv), K.ptr(tab), len(ts),
                                                  40, 2, H, CTX)
        assert rc == -1, (rows, ts, offs, rc)
    assert np.all(out == np.float16(7.25)) and np.all(ck == np.float16(7.25))
