"""CPU: per-clip decoder prompt prefixes in the decode pool's refill policy (norma_amd/pool.py: prefix=, after=,
condition_on_previous) against the scripted stand-in engine.  A clip that follows another is admitted only once that clip's
result is final, and its prefix is made from that result; without the keywords the engine never hears of prefixes.
The GPU side is tests/test_gpu_pool_prompt.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from norma_amd import cabi, hip, pool
from norma_amd.hip import NH_LANG_DETECT
import pool_standin
from pool_standin import BAD, GOOD, Encoder, feeder

SOP, EOT = 50360, 50256


class Engine(pool_standin.Engine):
    """... that takes prefixes under nh_pool_prefix's rules: into a free row only; a detecting admission finds none pending"""

    def pool_begin(self, rows, max_new, per_clip_language):
        super().pool_begin(rows, max_new, per_clip_language)
        self.pending = [None] * rows

    def pool_prefix(self, row, ids):
        assert 0 <= row < self.rows and self.left[row] is None, "NH_ERR_INVALID: prefix into a busy row"
        assert len(ids) >= 1 and all(isinstance(t, int) for t in ids)
        self.pending[row] = list(ids)
        self.log.append(("prefix", row, tuple(ids)))

    def _admit(self, c, dst, lang):
        assert not (lang == NH_LANG_DETECT and self.pending[dst]), "NH_ERR_INVALID: NH_LANG_DETECT into a row with a pending prefix"
        super()._admit(c, dst, lang)
        self.pending[dst] = None


def _chain(stride):
    """clip c follows clip c - stride: `stride` recordings in flight, their chunks interleaved"""
    return lambda c: c - stride if c >= stride else None


def _run(kind, e, n, rows, **kw):
    finals = lambda c, r: e.log.append(("final", c))
    langs = list(range(1000, 1000 + n))
    if kind == "staged":
        return pool.DecodePool(e, rows=rows, staging=3, check_every=2, **kw).run(n, e.encode, langs=langs, on_result=finals)
    encs = [Encoder(), Encoder()]
    return pool.FedDecodePool(e, encs, rows=rows, batch=3, check_every=2, **kw).run(n, feeder(encs), langs=langs, on_result=finals)


@pytest.mark.parametrize("kind", ("staged", "fed"))
def test_without_the_keywords_no_prefix_is_ever_set(kind):
    e = Engine([5, 9, 3, 12, 4, 7, 6])
    res = _run(kind, e, 7, 3)
    assert [r["clip"] for r in res] == list(range(7))
    assert not [x for x in e.log if x[0] == "prefix"]


@pytest.mark.parametrize("kind", ("staged", "fed"))
@pytest.mark.parametrize("rows,stride,fallback", [(1, 1, False), (4, 2, False), (4, 2, True), (1, 1, True), (3, 5, True)])
def test_a_clip_is_admitted_only_after_its_predecessors_final_result(kind, rows, stride, fallback):
    rng = np.random.default_rng(rows * 10 + stride)
    N = 17
    lengths = [int(x) for x in rng.choice([3, 10, 25, 40], size=N)]
    script = [[BAD, GOOD] if c % 3 == 1 else [GOOD] for c in range(N)] if fallback else None
    e = Engine(lengths, script=script)
    seen = {}

    def prefix(clip, prev):
        seen[clip] = prev
        return None if prev is None else [SOP] + [int(t) for t in prev["tokens"]]
    res = _run(kind, e, N, rows, prefix=prefix, after=_chain(stride), fallback=fallback)
    assert [r["clip"] for r in res] == list(range(N))
    at = {(x[0], x[1]): i for i, x in enumerate(e.log) if x[0] in ("admit", "final")}
    assert [x[1] for x in e.log if x[0] == "admit"] == list(range(N))           # still in clip order
    for c in range(N):
        if c >= stride:
            assert at[("final", c - stride)] < at[("admit", c)], c
            assert seen[c] is res[c - stride]                                      # prev is that clip's FINAL result
            if fallback and (c - stride) % 3 == 1:
                assert seen[c]["attempt"] == 1 and seen[c]["accepted"]             # ... the accepted retry, not the rejected t = 0 attempt
        else:
            assert seen[c] is None
    if fallback:
        assert [x for x in e.log if x[0] == "retry"]
    # every clip with a predecessor got that predecessor's tokens as its prefix, into the row it was then admitted to
    pre = {}
    for i, x in enumerate(e.log):
        if x[0] == "prefix":
            nxt = e.log[i + 1]
            assert nxt[0] == "admit" and nxt[2] == x[1]
            pre[nxt[1]] = x[2]
    assert pre == {c: (SOP,) + tuple(res[c - stride]["tokens"]) for c in range(stride, N)}


def test_bias_then_prefix_then_admit():
    e = Engine([4, 6, 5, 3], guard=True)
    dp = pool.DecodePool(e, rows=2, staging=2, check_every=2, guard=dict(bias=True), bias=lambda c: {7: 1.0},
                         prefix=lambda c, prev: [SOP, 100 + c])
    dp.run(4, e.encode)
    calls = [x for x in e.log if x[0] in ("guard_bias", "prefix", "admit")]
    assert [x[0] for x in calls] == ["guard_bias", "prefix", "admit"] * 4
    for k in range(4):
        b, p, a = calls[3 * k:3 * k + 3]
        assert b[1] == p[1] == a[2] and a[1] == k and p[2] == (SOP, 100 + k)


def test_an_empty_answer_sets_no_prefix():
    e = Engine([4, 6, 5])
    pool.DecodePool(e, rows=2, staging=2, check_every=2, prefix=lambda c, prev: [] if c == 1 else None).run(3, e.encode)
    assert not [x for x in e.log if x[0] == "prefix"]


def test_the_two_value_errors():
    e = Engine([4, 6, 5], align=True)
    with pytest.raises(ValueError):
        pool.DecodePool(e, rows=2, staging=2, align_heads=[(0, 0)], prefix=lambda c, prev: None)
    with pytest.raises(ValueError):
        pool.FedDecodePool(e, [Encoder()], rows=2, batch=2, align_heads=[(0, 0)], prefix=lambda c, prev: None)
    for bad in (lambda c: c, lambda c: c + 1, lambda c: -1):
        e = Engine([4, 6, 5])
        with pytest.raises(ValueError):
            pool.DecodePool(e, rows=2, staging=2, check_every=2, after=bad).run(3, e.encode)


def test_condition_on_previous_cuts_and_declines():
    f = pool.condition_on_previous(SOP, EOT)
    sot, en, task, ts0 = 50257, 50258, 50358, 50363
    text = list(range(300, 300 + 400))
    prev = dict(tokens=[sot, en, task, ts0] + text[:200] + [ts0 + 5, ts0 + 5] + text[200:] + [ts0 + 9, EOT], no_speech_exit=False,
                accepted=True, temperature=0.0)
    got = f(5, prev)
    assert got == [SOP] + text[-222:] and len(got) == 223
    assert pool.condition_on_previous(SOP, EOT, max_prefix=4)(5, prev) == [SOP] + text[-3:]
    short = dict(prev, tokens=[sot, task, ts0, 11, 12, ts0 + 1, EOT])                  # a two-token prompt: no language
    assert f(1, short) == [SOP, 11, 12]
    assert f(1, dict(short, temperature=0.4)) == [SOP, 11, 12]
    assert f(1, {"tokens": [sot, task, 11, 12, EOT], "no_speech_exit": False}) == [SOP, 11, 12]   # a pool without fallback
    assert f(1, None) is None
    assert f(1, dict(short, no_speech_exit=True)) is None
    assert f(1, dict(short, accepted=False)) is None
    assert f(1, dict(short, temperature=0.6)) is None
    assert f(1, dict(short, tokens=[sot, task, ts0, ts0 + 1, EOT])) is None            # no text: nothing to condition on


def test_condition_on_previous_through_the_pool():
    """chunks of two recordings interleaved; the stand-in's tokens are [clip, attempt]: both count as text here"""
    e = Engine([6, 3, 8, 4, 5, 7], script=[[GOOD], [BAD, GOOD], [GOOD], [GOOD], [BAD] * 6, [GOOD]])
    res = pool.DecodePool(e, rows=2, staging=2, check_every=2, fallback=True, after=_chain(2),
                          prefix=pool.condition_on_previous(SOP, EOT)).run(6, e.encode, langs=[9] * 6)
    pre = {e.log[i + 1][1]: x[2] for i, x in enumerate(e.log) if x[0] == "prefix"}
    # clip 3 follows clip 1, accepted on its retry at t = 0.2; clip 5 follows clip 3; clip 4 was dropped, nothing follows it
    assert pre == {2: (SOP, 0, 0), 3: (SOP, 1, 1), 4: (SOP, 2, 0), 5: (SOP, 3, 0)}
    assert res[4]["accepted"] is False and res[1]["temperature"] == 0.2


def test_the_pool_header_is_bound_exported_and_in_integration_md():
    """include/norma_hip_pool.h: the one prototype it declares, bound on the library hip.py loads with the types the header
    states, exported by both builds, and declared in INTEGRATION.md's block for that header"""
    H = cabi.read(hip.POOL_HEADER_PATH)
    assert sorted(H.prototypes) == ["nh_pool_prefix"] and not set(H.prototypes) & set(hip.declared_symbols())
    restype, argtypes, names = H.prototypes["nh_pool_prefix"]
    assert names == ["ctx", "row", "tokens", "n_prefix"] and restype is C.c_int
    fn = hip.load_library().nh_pool_prefix
    assert fn.restype is C.c_int and fn.argtypes == [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int] == argtypes
    assert hasattr(C.CDLL(hip.STRICT_LIB_PATH), "nh_pool_prefix")
    assert H.structs["nh_config"] is hip.NhConfig                      # the first header's classes, not second ones
    with open(os.path.join(os.path.dirname(hip.POOL_HEADER_PATH), os.pardir, "INTEGRATION.md")) as f:
        md = f.read()
    block = md[md.index("include/norma_hip_pool.h\n"):]
    block = block[:block.index("```")]
    assert set(re.findall(r"pub fn (nh_[a-z_0-9]+)", block)) == set(H.prototypes)
