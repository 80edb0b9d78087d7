"""GPU: token-level timestamps from the decode itself (nh_align_capture / nh_align_decoded, DESIGN.md 9 "Alignment from the
decode").  Kernel level: the capture kernel and the row map of the three stage launchers through tools/kref.hip, bit for bit.
C ABI level: whatever a context decoded -- a lockstep batch, greedy or sampled; rows of a pool at their own positions, refilled,
retried, detecting their language -- aligned from the queries it kept must equal nh_align on a lockstep context of the same
weights that holds that clip alone and is given the returned tokens: integer for integer, and the KEEP = 1 views bit for bit
(the queries come from the same kernels on the same inputs).  No tolerance anywhere."""
import zlib

import numpy as np
import pytest

import align_live_ref as AL
import align_ref as AR
import common
import kref as K
from test_gpu_align import _overrides
from test_gpu_pool import _encode_into

pytestmark = pytest.mark.gpu

NAME = "test-d128"
HEADS = [(0, 1), (1, 0)]
HEADS_B = [(1, 1), (0, 0), (0, 1)]
P_LEN = 3
MAX_NEW = 24
N_KEYS = (1500, 750, 37)
INVALID, STATE = 1, 3


def rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _same(a, b):
    """two decode results with the same bits (this fixture's avg_logprob is NaN for some clips: a NaN equals itself here)"""
    f = lambda v: np.float64(v).tobytes()
    return (a["tokens"] == b["tokens"] and f(a["avg_logprob"]) == f(b["avg_logprob"]) and f(a["no_speech_prob"]) == f(b["no_speech_prob"])
            and a["no_speech_exit"] == b["no_speech_exit"])


# ---- the capture kernel -----------------------------------------------------------------------------------------------------
NPOS = 7
POS = [0, NPOS - 1, NPOS, 2]          # the first and the last position of the buffer, one past it (never written), one inside
DONE = [0, 0, 1, 2, 3]                # running (twice as likely), finished, no-speech exit, empty


@pytest.mark.parametrize("from_device", [True, False])
@pytest.mark.parametrize("d,H", [(128, 2), (384, 6)])
@pytest.mark.parametrize("B", [1, 3, 65])
def test_capture_kernel_writes_the_running_rows_at_their_positions_and_nothing_else(B, d, H, from_device):
    """the first and the last head of the layer; per-row positions 0, npos - 1, npos (not written) and one inside, done flags
    0 / 1 / 2 / 3, every pair of the two over the variants; a buffer with more rows than the step has (a pool's), pre-filled
    with NaNs of distinct payloads; once with the positions in device memory, once with one host position for all rows"""
    r = rng("cap", B, d, H)
    heads = [0, H - 1]
    ldb = B + 2
    wrote = 0
    for v in range(20 if B == 1 else 5):
        dq = K.f16(r.standard_normal((B, d)))
        buf = AL.nan_pattern((len(heads), NPOS, ldb, 64))
        done = [DONE[(b + 2 * v) % 5] for b in range(B)]
        pos_ptr = [POS[(b + v) % 4] for b in range(B)] if from_device else None
        pos = -5 if from_device else POS[v % 4]            # with device positions the host one must not matter
        got = AL.gpu_qsave_rows(dq, buf, heads, ldb, NPOS, pos=pos, pos_ptr=pos_ptr, done=done)
        want = AL.qsave_rows_expected(dq, buf, heads, NPOS, pos=pos, pos_ptr=pos_ptr, done=done)
        assert np.array_equal(got, want), (v, np.argwhere(got != want)[:4].tolist())
        wrote += int((want != buf).any(axis=-1).sum())
    assert wrote > 0
    # done == nullptr: every row is running
    dq = K.f16(r.standard_normal((B, d)))
    buf = AL.nan_pattern((len(heads), NPOS, ldb, 64))
    pp = [POS[b % 4] for b in range(B)]
    got = AL.gpu_qsave_rows(dq, buf, heads, ldb, NPOS, pos=3, pos_ptr=pp if from_device else None)
    assert np.array_equal(got, AL.qsave_rows_expected(dq, buf, heads, NPOS, pos=3, pos_ptr=pp if from_device else None))


# ---- the row map ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nk", [4, 65, 750])
def test_row_map_reads_the_mapped_rows_and_changes_nothing_else(nk):
    """B = 3 context rows with 1 / 17 / 33 query rows; maps [2, 0] and [1]: every stage gives, bit for bit, what the unmapped
    launcher gives on the gathered inputs; a null map is the unmapped launcher.  Keys at or beyond nk would own the softmax."""
    r = rng("map", nk)
    B, H, heads, rows, max_rows, S = 3, 2, [1, 0], np.array([1, 17, 33]), 33, nk + 5
    q = K.f16(r.standard_normal((len(heads), max_rows, B, 64)))
    k = K.f16(r.standard_normal((B, H, S, 64)))
    k[:, :, nk:] = K.f16(20.0 * r.standard_normal((B, H, S - nk, 64)))
    full = AR.gpu_weights(q, k, heads, rows, [nk] * B)
    assert same_bits(AL.gpu_weights_rows(q, k, heads, None, rows, [nk] * B), full)
    for m in ([2, 0], [1]):
        n = len(m)
        Wm = AL.gpu_weights_rows(q, k, heads, m, rows[m], [nk] * n)
        Wg = AR.gpu_weights(np.ascontiguousarray(q[:, :, m]), np.ascontiguousarray(k[m]), heads, rows[m], [nk] * n)
        assert same_bits(Wm, Wg) and same_bits(Wm, full[m]), m
        for g, b in enumerate(m):
            assert np.isfinite(Wm[g, :, :rows[b], :nk]).all() and np.isnan(Wm[g, :, rows[b]:]).all() and np.isnan(Wm[g, :, :, nk:]).all()
        for P in (1, 3):
            nr = [int(rows[b]) if rows[b] + 1 - P >= 1 else 0 for b in m]
            Mm = AL.gpu_reduce_rows(Wm, m, nr, [nk] * n, P)
            assert same_bits(Mm, AR.gpu_reduce(Wg, nr, [nk] * n, P)) and same_bits(Mm, AL.gpu_reduce_rows(Wm, None, nr, [nk] * n, P)), (m, P)
            fm, lm = AL.gpu_dtw_rows(Mm, m, nr, [nk] * n, P)
            fg, lg = AR.gpu_dtw(Mm, nr, [nk] * n, P)
            fn, ln = AL.gpu_dtw_rows(Mm, None, nr, [nk] * n, P)
            assert np.array_equal(fm, fg) and np.array_equal(lm, lg) and np.array_equal(fm, fn) and np.array_equal(lm, ln), (m, P)
            for g in range(n):
                R = nr[g] + 1 - P
                if R >= 1:
                    assert fm[g, P] == 0 and lm[g, P + R - 1] == nk - 1


# ---- through the C ABI ------------------------------------------------------------------------------------------------------
class Fixture:
    """one weight set; a lockstep context of three clips, a pool context (two rows + three staging rows), and the reference:
    a lockstep context that holds one clip alone and aligns given tokens with nh_align (views kept)"""

    def __init__(self):
        from norma_amd import hip, synth
        self.hip = hip
        self.cfg, self.tk = common.make_config(NAME), common.tokens_for(NAME)
        self.over = _overrides(self.cfg)
        self.hm = common.build_hip(self.cfg, self.tk, overrides=self.over, max_batch=3)
        self.clips = np.stack([synth.synth_pcm(k) for k in range(3)])
        self.hp = self.shared(5)
        self.ref = self.shared(1)
        self.ref.set_option(hip.NH_OPT_ALIGN_KEEP, 1)
        self.ref_clip = None
        self.hm.set_option(hip.NH_OPT_ALIGN_KEEP, 1)
        self.hp.set_option(hip.NH_OPT_ALIGN_KEEP, 1)
        self._cache = {}

    def shared(self, max_batch):
        h = self.hip.HipWhisper(self.cfg, device=0, max_batch=max_batch, share_with=self.hm)
        h.set_tokens(self.tk, self.tk.en, self.tk.transcribe)
        return h

    def close(self):
        for h in (self.hp, self.ref, self.hm):
            h.close()

    def encode_all(self):
        self.hm.logmel_array(self.clips)
        self.hm.encode()

    def reference(self, clip, tokens, heads=HEADS, nk=None):
        """nh_align of `tokens` on clip `clip` alone: (first, last, [weights per head], matrix); computed once per question"""
        key = (clip, tuple(tokens), tuple(heads), nk)
        if key not in self._cache:
            if self.ref_clip != clip:
                self.ref.logmel_array(np.ascontiguousarray(self.clips[clip:clip + 1]))
                self.ref.encode()
                self.ref_clip = clip
            f, l = self.ref.align([tokens], prompt_len=P_LEN, heads=heads, n_keys=None if nk is None else [nk])
            self._cache[key] = (f[0].copy(), l[0].copy(), [self.ref.align_weights(0, a) for a in range(len(heads))], self.ref.align_matrix(0))
        return self._cache[key]

    def check(self, h, i, clip, tokens, first, last, heads=HEADS, nk=None, views=True):
        """entry i of the last align_decoded of context h against the reference"""
        rf, rl, rW, rM = self.reference(clip, tokens, heads, nk)
        n = len(tokens)
        assert n > P_LEN
        assert first[i].tolist() == rf.tolist() and last[i].tolist() == rl.tolist(), (clip, i)
        assert (first[i, :P_LEN] == -1).all() and (first[i, n:] == -1).all() and first[i, P_LEN] == 0
        if views:
            for a in range(len(heads)):
                assert same_bits(h.align_weights(i, a), rW[a]), ("weights", clip, i, a)
            assert same_bits(h.align_matrix(i), rM), ("matrix", clip, i)


@pytest.fixture(scope="module")
def fx():
    f = Fixture()
    yield f
    f.close()


def _finish(hp, rows, step=1, limit=600):
    """pool steps until every row of `rows` has finished"""
    for _ in range(limit):
        flags = hp.pool_step(step)
        if all(flags[r] in (1, 2) for r in rows):
            return flags
    raise AssertionError("rows did not finish")


@pytest.mark.parametrize("n_keys", [None, N_KEYS])
def test_lockstep_greedy_equals_nh_align_on_the_returned_tokens(fx, n_keys):
    fx.hm.align_capture(HEADS)
    fx.encode_all()
    res = fx.hm.decode_greedy(max_new_tokens=MAX_NEW)
    first, last = fx.hm.align_decoded(n_keys=n_keys)
    assert any(not r["no_speech_exit"] for r in res)
    for b, r in enumerate(res):
        assert not r["no_speech_exit"]
        fx.check(fx.hm, b, b, r["tokens"], first, last, nk=None if n_keys is None else n_keys[b])
    # still valid: the same sequences over other keys, then over the first ones again
    f2, l2 = fx.hm.align_decoded(n_keys=[700, 1500, 9])
    fx.check(fx.hm, 1, 1, res[1]["tokens"], f2, l2, nk=1500)
    f3, l3 = fx.hm.align_decoded(n_keys=n_keys)
    assert np.array_equal(f3, first) and np.array_equal(l3, last)


def test_lockstep_sampled_equals_nh_align_on_the_returned_tokens(fx):
    fx.hm.align_capture(HEADS)
    fx.encode_all()
    greedy = fx.hm.decode_greedy(max_new_tokens=MAX_NEW)
    res = fx.hm.decode_sampled(0.8, seed=0xA11C, clip0=40, attempt=2, max_new_tokens=MAX_NEW)
    assert any(r["tokens"] != g["tokens"] for r, g in zip(res, greedy))
    first, last = fx.hm.align_decoded(n_keys=N_KEYS)
    for b, r in enumerate(res):
        fx.check(fx.hm, b, b, r["tokens"], first, last, nk=N_KEYS[b])


def _pool_run(fx, **kw):
    from norma_amd import pool
    dp = pool.DecodePool(fx.hp, rows=2, staging=3, max_new_tokens=MAX_NEW, check_every=3, **kw)
    return dp, dp.run(3, _encode_into(fx.hp, fx.clips))


def test_capture_changes_no_token_and_no_logprob_and_a_new_head_list_replaces_the_old_one(fx):
    hm = fx.hm
    fx.encode_all()
    hm.align_capture([])
    off = hm.decode_greedy(max_new_tokens=MAX_NEW)
    hm.align_capture(HEADS)
    on = hm.decode_greedy(max_new_tokens=MAX_NEW)
    fa, la = hm.align_decoded()
    hm.align_capture(HEADS_B)                      # the step graphs captured with HEADS are stale now
    on_b = hm.decode_greedy(max_new_tokens=MAX_NEW)
    fb, lb = hm.align_decoded()
    for b in range(3):
        assert _same(off[b], on[b]) and _same(off[b], on_b[b])
        fx.check(hm, b, b, on_b[b]["tokens"], fb, lb, heads=HEADS_B)
    rf, rl, _, _ = fx.reference(0, on[0]["tokens"], HEADS)
    assert fa[0].tolist() == rf.tolist() and la[0].tolist() == rl.tolist()
    assert not (np.array_equal(fa, fb) and np.array_equal(la, lb)), "the two head lists cannot be told apart on this data"
    hm.align_capture([])
    assert all(_same(a, b) for a, b in zip(off, hm.decode_greedy(max_new_tokens=MAX_NEW)))
    # pooled
    _, plain = _pool_run(fx)
    dp, timed = _pool_run(fx, align_heads=HEADS)
    assert dp.aligned == sum(1 for r in timed if not r["no_speech_exit"]) > 0
    for c in range(3):
        assert _same(plain[c], timed[c]) and _same(plain[c], off[c])
        assert "token_first" not in plain[c]
    fx.hp.align_capture([])


def test_pool_rows_at_their_own_positions_refilled_and_beside_running_finished_and_empty_neighbours(fx):
    hp = fx.hp
    hp.pool_begin(2, MAX_NEW, False)
    hp.align_capture(HEADS)
    _encode_into(hp, fx.clips)(0, 3, 2)
    hp.pool_admit(2 + 0, 0)
    hp.pool_step(2)                                 # row 0 is two positions ahead of row 1 from here on
    hp.pool_admit(2 + 1, 1)
    owner, toks, seen, states = {0: 0, 1: 1}, {}, {}, set()
    refilled = False
    for _ in range(600):
        flags = hp.pool_step(1)
        for r in [r for r in sorted(owner) if flags[r] in (1, 2)]:
            c = owner.pop(r)
            res = hp.pool_collect([r])[0]
            assert not res["no_speech_exit"]
            toks[r] = (c, res["tokens"])
            first, last = hp.align_decoded([r], n_keys=[N_KEYS[c]])
            fx.check(hp, 0, c, res["tokens"], first, last, nk=N_KEYS[c])
            seen[(r, c)] = (first[0].copy(), last[0].copy())
            states.add("running" if owner else "idle")
        if 0 not in owner and 0 in toks and not refilled:      # row 0 is refilled while row 1 keeps what it decoded (or still decodes)
            hp.pool_admit(2 + 2, 0)
            owner[0], refilled = 2, True
            with pytest.raises(fx.hip.HipError) as ei:
                hp.align_decoded([0])
            assert ei.value.code == STATE
            if 1 in toks and 1 not in owner:                   # row 1 beside a neighbour that is running again
                c, t = toks[1]
                first, last = hp.align_decoded([1], n_keys=[N_KEYS[c]])
                assert np.array_equal(first[0], seen[(1, c)][0]) and np.array_equal(last[0], seen[(1, c)][1])
                states.add("running")
        if not owner and refilled:
            break
    assert not owner and {c for _, c in seen} == {0, 1, 2} and "running" in states, (owner, states)
    # both rows in one call, in map order [1, 0], each beside a finished neighbour
    rows = [1, 0]
    first, last = hp.align_decoded(rows, n_keys=[N_KEYS[toks[r][0]] for r in rows])
    for i, r in enumerate(rows):
        c, t = toks[r]
        fx.check(hp, i, c, t, first, last, nk=N_KEYS[c])
        assert np.array_equal(first[i], seen[(r, c)][0]) and np.array_equal(last[i], seen[(r, c)][1])
    # an empty neighbour: a fresh pool whose row 0 never holds a clip
    hp.pool_begin(2, MAX_NEW, False)
    _encode_into(hp, fx.clips)(1, 1, 2)
    hp.pool_admit(2, 1)
    _finish(hp, [1], step=4)
    res = hp.pool_collect([1])[0]
    first, last = hp.align_decoded([1], n_keys=[N_KEYS[1]])
    fx.check(hp, 0, 1, res["tokens"], first, last, nk=N_KEYS[1])
    assert np.array_equal(first[0], seen[(1, 1)][0]) and np.array_equal(last[0], seen[(1, 1)][1])
    hp.align_capture([])


def test_a_retried_row_is_aligned_on_its_retry_and_a_detecting_row_with_its_language(fx):
    hp, tk = fx.hp, fx.tk
    hp.pool_begin(2, MAX_NEW, True)
    langs = [tk.en + k for k in range(5)]
    hp.pool_detect_languages(langs)
    hp.align_capture(HEADS)
    _encode_into(hp, fx.clips)(0, 3, 2)
    hp.pool_admit(2 + 0, 0, fx.hip.NH_LANG_DETECT)
    hp.pool_admit(2 + 1, 1, tk.en + 2)
    _finish(hp, [0, 1], step=4)
    g = hp.pool_collect([0, 1])
    lang, _ = hp.pool_languages([0])
    assert g[0]["tokens"][1] == lang[0] and lang[0] in langs and g[1]["tokens"][1] == tk.en + 2
    first, last = hp.align_decoded([0, 1])
    for r in range(2):
        fx.check(hp, r, r, g[r]["tokens"], first, last)
    # row 0 again, sampled; meanwhile it cannot be aligned, row 1 can
    hp.pool_retry(0, 0.8, 0xBEEF, 7, 1)
    with pytest.raises(fx.hip.HipError) as ei:
        hp.align_decoded([0])
    assert ei.value.code == STATE
    f1, l1 = hp.align_decoded([1])
    assert np.array_equal(f1[0], first[1]) and np.array_equal(l1[0], last[1])
    _finish(hp, [0], step=4)
    s = hp.pool_collect([0])[0]
    assert s["tokens"] != g[0]["tokens"] and s["tokens"][1] == lang[0]          # the retry keeps the detected language
    fr, lr = hp.align_decoded([0], n_keys=[N_KEYS[1]])
    fx.check(hp, 0, 0, s["tokens"], fr, lr, nk=N_KEYS[1])
    hp.align_capture([])


def _refused(h, code, fn, *a, **kw):
    from norma_amd import hip
    with pytest.raises(hip.HipError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, str(ei.value)


def _decoded_refused(h, code, rows=None, n_keys=None):
    """nh_align_decoded itself, on buffers of the test's own: the code, and outputs pre-filled with -2 left as they are"""
    r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
    n = h.batch if r is None else len(r)
    nk = None if n_keys is None else np.ascontiguousarray(n_keys, dtype=np.int32)
    first = np.full((max(n, 1), h.cfg.max_target_positions), -2, dtype=np.int32)
    last = first.copy()
    ip = lambda a: None if a is None else a.ctypes.data_as(h.L.nh_align_decoded.argtypes[1])
    rc = h.L.nh_align_decoded(h._h, ip(r), n, ip(nk), ip(first), ip(last))
    assert rc == code, (rc, h.L.nh_last_error(h._h).decode())
    assert (first == -2).all() and (last == -2).all(), "a refused call wrote its outputs"


def test_refusals(fx):
    hip = fx.hip
    hm, hp = fx.hm, fx.hp
    fx.encode_all()
    # ---- nh_align_capture
    _refused(hm, INVALID, hm.align_capture, [(0, 0)] * 33)
    hs = (hip.NhAlignHead * 1)(hip.NhAlignHead(0, 0))
    assert hm.L.nh_align_capture(hm._h, hs, -1) == INVALID
    for bad in [(2, 0), (-1, 0), (0, 2), (0, -1)]:
        _refused(hm, INVALID, hm.align_capture, [(0, 0), bad])
    hm.set_option(hip.NH_OPT_DECODER_LAYER_LIMIT, 1)
    _refused(hm, INVALID, hm.align_capture, [(1, 0)])
    hm.set_option(hip.NH_OPT_DECODER_LAYER_LIMIT, 0)
    hm.set_option(hip.NH_OPT_ABSORBED_XATTN, 1)
    _refused(hm, STATE, hm.align_capture, HEADS)
    hm.set_option(hip.NH_OPT_ABSORBED_XATTN, 0)
    # ---- nh_align_decoded, lockstep
    hm.align_capture([])
    hm.decode_greedy(max_new_tokens=MAX_NEW)
    _decoded_refused(hm, STATE)                                         # no heads set
    hm.align_capture(HEADS)
    _decoded_refused(hm, STATE)                                         # decoded before the heads were set
    res = hm.decode_greedy(max_new_tokens=MAX_NEW)
    _decoded_refused(hm, INVALID, rows=[0, 1, 2])                       # rows on a lockstep context
    _decoded_refused(hm, INVALID, n_keys=[1500, 0, 1500])
    _decoded_refused(hm, INVALID, n_keys=[1500, 1500, 1501])
    hm.batch = 2
    _decoded_refused(hm, INVALID)                                       # n is not the batch
    hm.batch = 3
    first, last = hm.align_decoded()                                    # the refusals launched nothing and spoiled nothing
    fx.check(hm, 2, 2, res[2]["tokens"], first, last)
    toks = [r["tokens"] for r in res]
    spoilers = [lambda: hm.align(toks, prompt_len=P_LEN, heads=HEADS),
                lambda: hm.decoder_forward(np.array([t[:4] for t in toks], dtype=np.int32)),
                lambda: hm.detect_language([fx.tk.en, fx.tk.en + 1]),
                lambda: hm.encode(),
                lambda: hm.logmel_array(fx.clips),
                lambda: hm.align_capture(HEADS)]
    for spoil in spoilers:
        hm.set_languages(None)
        fx.encode_all()
        hm.decode_greedy(max_new_tokens=MAX_NEW)
        hm.align_decoded()
        spoil()
        _decoded_refused(hm, STATE)
    hm.set_languages(None)
    # ---- nh_align_decoded, pool
    hp.pool_begin(2, MAX_NEW, False)
    hp.align_capture([])
    _encode_into(hp, fx.clips)(0, 3, 2)
    hp.pool_admit(2, 0)
    _refused(hp, STATE, hp.align_capture, HEADS)                        # a row is busy
    _finish(hp, [0], step=4)
    hp.pool_collect([0])
    _decoded_refused(hp, STATE, rows=[0])                               # no heads set
    hp.align_capture(HEADS)
    _decoded_refused(hp, STATE, rows=[0])                               # decoded before the current head list was set
    _decoded_refused(hp, STATE, rows=[1])                               # never admitted
    _decoded_refused(hp, INVALID, rows=[2])                             # outside the pool
    _decoded_refused(hp, INVALID, rows=[-1])
    hp.batch = 1
    _decoded_refused(hp, INVALID)                                       # rows == NULL on a pool context
    hp.pool_admit(3, 1)
    _decoded_refused(hp, STATE, rows=[1])                               # busy
    _finish(hp, [1], step=4)
    res = hp.pool_collect([1])[0]
    _decoded_refused(hp, INVALID, rows=[1], n_keys=[0])
    _decoded_refused(hp, INVALID, rows=[1], n_keys=[1501])
    _decoded_refused(hp, INVALID, rows=[1, 1, 1])                       # more entries than the pool has rows
    first, last = hp.align_decoded([1])
    fx.check(hp, 0, 1, res["tokens"], first, last)
    hp.pool_retry(1, 0.6, 5, 1, 1)
    _decoded_refused(hp, STATE, rows=[1])                               # retried and not collected since
    _finish(hp, [1], step=4)
    hp.pool_collect([1])
    hp.align_capture(HEADS_B)
    _decoded_refused(hp, STATE, rows=[1])                               # collected under the list before
    hp.pool_admit(4, 0)
    _decoded_refused(hp, STATE, rows=[0])                               # refilled and not collected since
    _finish(hp, [0], step=4)
    res = hp.pool_collect([0])[0]
    first, last = hp.align_decoded([0])
    fx.check(hp, 0, 2, res["tokens"], first, last, heads=HEADS_B)
    hp.align_capture([])
    hm.align_capture([])


def _fresh(fx):
    """a lockstep context of the fixture's weights that has never aligned (no query buffer yet), the three clips encoded"""
    h = fx.shared(3)
    h.set_option(fx.hip.NH_OPT_ALIGN_KEEP, 1)
    h.logmel_array(fx.clips)
    h.encode()
    return h


def _align_equals_reference(fx, h, toks, heads):
    """nh_align of the whole batch on h against the reference context, clip by clip; returns (first, last, views)"""
    first, last = h.align(toks, prompt_len=P_LEN, heads=heads)
    views = [[h.align_weights(b, a) for a in range(len(heads))] + [h.align_matrix(b)] for b in range(3)]
    for b in range(3):
        rf, rl, rW, rM = fx.reference(b, toks[b], heads)
        assert first[b].tolist() == rf.tolist() and last[b].tolist() == rl.tolist(), b
        assert all(same_bits(v, r) for v, r in zip(views[b], rW + [rM])), b
    return first, last, views


def test_nh_align_with_more_heads_moves_the_query_buffer_under_captured_step_graphs(fx):
    """the context's one query buffer holds 2 heads and the captured steps hold its address when nh_align asks for 3: the
    buffer moves, what the decode kept is gone (refused, not read), and the next decode captures its steps again and keeps its
    queries in the new buffer -- same tokens, same log-probs, same times as before the move"""
    h = _fresh(fx)
    h.align_capture(HEADS)
    res = h.decode_greedy(max_new_tokens=MAX_NEW)                       # the step graphs are captured here
    toks = [r["tokens"] for r in res]
    f0, l0 = h.align_decoded()
    _align_equals_reference(fx, h, toks, HEADS_B)
    _decoded_refused(h, STATE)
    again = h.decode_greedy(max_new_tokens=MAX_NEW)
    assert all(_same(a, b) for a, b in zip(res, again))
    f1, l1 = h.align_decoded()
    assert np.array_equal(f1, f0) and np.array_equal(l1, l0)
    for b in range(3):
        fx.check(h, b, b, toks[b], f1, l1, heads=HEADS)
    h.close()


def test_a_capture_of_fewer_heads_uses_the_buffer_nh_align_made(fx):
    """the other order: nh_align allocates the buffer for 3 heads, nh_align_capture of 2 heads does not grow it, and the decode
    keeps its queries there; nh_align over it again gives what it gave the first time"""
    h = _fresh(fx)
    toks = [r["tokens"] for r in h.decode_greedy(max_new_tokens=MAX_NEW)]   # no heads set: there is no buffer yet
    fa, la, va = _align_equals_reference(fx, h, toks, HEADS_B)
    h.align_capture(HEADS)
    res = h.decode_greedy(max_new_tokens=MAX_NEW)
    assert [r["tokens"] for r in res] == toks
    first, last = h.align_decoded()
    for b in range(3):
        fx.check(h, b, b, toks[b], first, last, heads=HEADS)
    fb, lb, vb = _align_equals_reference(fx, h, toks, HEADS_B)
    assert np.array_equal(fa, fb) and np.array_equal(la, lb)
    assert all(same_bits(x, y) for p, q in zip(va, vb) for x, y in zip(p, q))
    h.close()


def test_a_no_speech_exit_has_nothing_to_align():
    """model.rs:308-315: position-0 logits put their mass on the no-speech token -> bare prompt; lockstep and pooled: all -1"""
    from norma_amd import hip, synth
    cfg, tk = common.make_config(NAME), common.tokens_for(NAME)
    over = common.scripted_overrides(cfg, tk, [tk.zero_sec, 500, tk.eot])
    emb = over["model.decoder.embed_tokens.weight"]
    pos = over["model.decoder.embed_positions.weight"].copy()
    pos[0] += np.float32(4.0) * emb[tk.no_speech]
    over["model.decoder.embed_positions.weight"] = pos.astype(np.float16).astype(np.float32)
    hm = common.build_hip(cfg, tk, overrides=over, max_batch=3)
    clips = np.stack([synth.synth_pcm(k) for k in range(2)])
    hm.align_capture(HEADS)
    hm.logmel_array(clips); hm.encode()
    res = hm.decode_greedy()
    assert all(r["no_speech_exit"] for r in res)
    first, last = hm.align_decoded()
    assert (first == -1).all() and (last == -1).all()
    hm.pool_begin(1, 0, False)
    _encode_into(hm, clips)(0, 2, 1)
    hm.pool_admit(1, 0)
    _finish(hm, [0])
    assert hm.pool_collect([0])[0]["no_speech_exit"]
    first, last = hm.align_decoded([0])
    assert (first == -1).all() and (last == -1).all()
    hm.close()


def test_decode_pool_with_fallback_times_the_accepted_attempt_of_every_clip():
    """DecodePool(align_heads=.., fallback=True) on weights whose log-probs are finite and whose transcripts end where the audio
    says (the varlen weights of tests/test_gpu_pool_fallback.py; the alignment fixture's avg_logprob is NaN, which no threshold
    ever sends through a retry).  Expected: model.rs:175-190 evaluated on lockstep decodes of the whole batch, one per
    temperature.  Every clip is timed on the attempt that policy accepts -- equal to nh_align of that attempt's tokens on the clip
    alone --, rejected attempts and dropped clips are never timed.  The temperatures are low ones, where a retry differs from
    the greedy decode only at near-ties, and the threshold is the lowest avg_logprob of a retry that beats its clip's greedy
    one: that clip is retried and a retry of it is accepted.  (At the reference's own temperatures a retry is a near-uniform
    draw far below every greedy log-prob, see test_gpu_pool_fallback.py; where no retry beats its greedy decode the threshold
    is the median and the accepted attempts are all attempt 0.)

    Measured on the MI355X: none of the 80 retries beats its clip's greedy decode, so the median branch runs: 8 clips are
    accepted and timed at attempt 0, 8 go through five retries each (40 pool_retry calls) and are dropped, untimed.  An accepted
    retry is aligned at the C ABI in test_a_retried_row_is_aligned_on_its_retry_and_a_detecting_row_with_its_language and in the
    policy in tests/test_pool_align_cpu.py."""
    from norma_amd import hip, pool
    from test_gpu_pool_fallback import _lockstep_attempts, _policy, _setup
    N, rows, staging, seed, clip0 = 16, 4, 4, 0xFA11BACC, 300
    T = (0.0, 0.02, 0.05, 0.1, 0.2, 0.4)
    cfg, tk, hm, hp, clips = _setup(N, rows + staging)
    ref = hip.HipWhisper(cfg, device=0, max_batch=1, share_with=hm)
    ref.set_tokens(tk, tk.en, tk.transcribe)
    attempts = _lockstep_attempts(hm, T, seed, clip0)
    lp = np.array([[r["avg_logprob"] for r in a] for a in attempts])          # [attempt][clip]
    assert np.isfinite(lp).all()
    better = [float(lp[a, c]) for c in range(N) for a in range(1, len(T)) if lp[a, c] > lp[0, c] and not attempts[0][c]["no_speech_prob"] > 0.6]
    thr = min(better) if better else float(np.median(lp[0]))
    want = _policy(attempts, T, thr)
    print(f"\nretries that beat their greedy decode: {len(better)}; threshold {thr:.4f}; accepted attempts {[w['attempt'] for w in want if w['accepted']]}")
    n_keys = [1500 - 40 * c for c in range(N)]
    dp = pool.DecodePool(hp, rows=rows, staging=staging, check_every=3, fallback=True, seed=seed, clip0=clip0, temperatures=T,
                         logprob_threshold=thr, align_heads=HEADS)
    got = dp.run(N, _encode_into(hp, clips), n_keys=n_keys)
    assert dp.retries == sum(w["attempt"] for w in want) and dp.retries >= 1
    timed = []
    for c, (g, w) in enumerate(zip(got, want)):
        assert _same(g, w) and (g["attempt"], g["accepted"]) == (w["attempt"], w["accepted"]), c
        if not g["accepted"] or g["no_speech_exit"]:
            assert "token_first" not in g and "token_last" not in g
            continue
        ref.logmel_array(np.ascontiguousarray(clips[c:c + 1])); ref.encode()
        rf, rl = ref.align([g["tokens"]], prompt_len=P_LEN, heads=HEADS, n_keys=[n_keys[c]])
        n = len(g["tokens"])
        assert g["token_first"] == rf[0, :n].tolist() and g["token_last"] == rl[0, :n].tolist(), c
        assert g["token_first"][:P_LEN] == [-1] * P_LEN and g["token_first"][P_LEN] == 0 and g["token_last"][-1] == n_keys[c] - 1
        timed.append(g["attempt"])
    assert len(timed) == dp.aligned >= 1
    if better:
        assert max(timed) > 0, "a retry was accepted and must have been timed"
    for h in (ref, hp, hm):
        h.close()
