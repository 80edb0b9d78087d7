"""CPU: the repetition guard.  The numpy contract (tests/guard_ref.py) on hand-written cases, the ABI's new
symbols, the pool policy (guard=, bias=, loop_fallback=) against a counting stand-in, and the decode fixtures of
tests/guard_fixture.py on the CPU oracle: every decision at least MARGIN from its runner-up before any GPU run.  No GPU."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest

import beam_fixture as F
import common
import guard_fixture as GF
import guard_ref as G
import pool_standin
from norma_amd import hip, pool

# a toy vocabulary: text 0 .. 4, eot 5, specials 6 .. 8 (no_timestamps 8), timestamps 9 .. 11
TK = SimpleNamespace(eot=5, no_timestamps=8, zero_sec=9, one_sec=10, sot=6)
INF = math.inf


def ed(logits, gen, p, bias=None, prompt=(6,)):
    toks = list(prompt) + list(gen)
    x, ex = G.edit(np.array(logits, dtype=np.float32), toks, len(toks), len(prompt), p, bias, TK)
    return x.tolist(), ex


L = [1.0, -2.0, 0.0, -0.0, 4.0, 0.5, 3.0, 3.0, 3.0, 1.0, 1.0, 1.0]


def test_penalty_once_per_distinct_token_and_by_sign():
    x, ex = ed(L, [9, 0, 1, 0, 2, 3, 10], G.params(repetition_penalty=2.0))
    #          0: 1 / 2 once; 1: -2 * 2; 2: 0 / 2; 3: -0 / 2 = -0; 4 and the timestamps untouched
    assert x == [0.5, -4.0, 0.0, -0.0, 4.0, 0.5, 3.0, 3.0, 3.0, 1.0, 1.0, 1.0] and ex == 0
    assert math.copysign(1.0, x[3]) == -1.0 and math.copysign(1.0, x[2]) == 1.0
    x, _ = ed(L, [9, 0, 1], G.params(repetition_penalty=0.5))
    assert x[:2] == [2.0, -1.0]


def test_bias_after_penalty_before_ban():
    p = G.params(repetition_penalty=2.0, bias=True, no_repeat_ngram=1)
    x, _ = ed(L, [9, 0], p, bias={0: 1.0, 4: -INF, 11: 0.25})
    assert x[0] == -INF                       # (1 / 2 + 1), then banned
    assert x[4] == -INF and x[11] == 1.25 and x[1] == -2.0
    x, _ = ed(L, [9, 0], G.params(repetition_penalty=2.0, bias=True), bias={0: 1.0})
    assert x[0] == 1.5
    x, _ = ed(L, [9, 0], G.params(repetition_penalty=2.0), bias={0: 1.0})     # a list without bias=True is not applied
    assert x[0] == 0.5


def test_ngram_cases():
    banned = lambda gen, N: [i for i, v in enumerate(ed(L, gen, G.params(no_repeat_ngram=N))[0]) if v == -INF]
    assert banned([9, 0, 1, 2, 0, 1], 3) == [2]
    assert banned([9, 0, 1, 2, 0], 3) == []                       # s = (2, 0) has not occurred before
    assert banned([9, 0], 3) == [] and banned([9], 3) == []       # m = N - 2 and m = 0
    assert banned([9, 0, 1], 3) == []                             # m = N - 1: nothing to compare with
    assert banned([9, 0, 0, 0], 3) == [0]                         # m = N: the one window, overlapping itself
    assert banned([9, 0, 1, 10, 11, 2, 0, 1], 3) == [2]           # timestamps are not history: the trigram spans them
    assert banned([9, 0, 1, 0, 2, 0], 2) == [1, 2]                # every continuation of 0
    assert banned([9, 3, 1, 3], 1) == [1, 3]                      # N = 1: every token of h
    assert banned([9, 0, 1, 2, 0, 1], 3) == banned([0, 1, 2, 9, 10, 0, 1], 3)
    # a prefix in front of the prompt is no history
    x, _ = G.edit(np.array(L, dtype=np.float32), [0, 1, 2, 6, 9, 0, 1], 7, 4, G.params(no_repeat_ngram=3), None, TK)
    assert -INF not in x.tolist()


def test_loop_exit_cases_and_deferral():
    p = G.params(loop_period=2, loop_repeats=3)
    only_eot = [-INF] * 5 + [0.5] + [-INF] * 6
    assert ed(L, [9, 0, 0, 0], p) == (only_eot, 1)                        # p = 1, p * R == m, last token text
    assert ed(L, [9, 0, 0], p)[1] == 0
    assert ed(L, [9, 0, 1, 0, 1, 0, 1], p) == (only_eot, 1)               # p = Pmax
    assert ed(L, [9, 2, 0, 1, 0, 1, 0, 1], p)[1] == 1                     # p * R one short of m
    assert ed(L, [9, 1, 0, 1, 0, 1], p)[1] == 0                           # m one short of p * R
    assert ed(L, [9, 0, 1, 2] * 3, p)[1] == 0                             # period 3 > Pmax (the timestamps are dropped)
    assert ed(L, [9, 0, 1, 10, 11, 0, 1, 10, 11, 0, 1], p)[1] == 1        # copies under different timestamps
    assert ed(L, [9, 0, 0, 0, 10], p) == ([float(np.float32(v)) for v in L], 0)   # text + timestamp: timestamps only, deferred
    assert ed(L, [9, 0, 0, 0, 10, 10], p) == (only_eot, 1)                # two timestamps: text only, taken
    assert ed(L, [0, 0, 0], p)[1] == 0                                    # nothing but text generated: the first-token rule, deferred
    assert ed(L, [9, 0, 0, 0, 1], p)[1] == 0                              # the copies must end the history


def test_greedy_ref_on_a_table():
    """a model that says 0 forever: greedy runs to max_new_tokens, the exit ends it after R copies with log-prob 0 for eot"""
    lg = np.full(12, -20.0, dtype=np.float32)
    lg[0], lg[9] = 5.0, 4.0
    sup = np.zeros(12, dtype=bool)
    sup[[6, 7, 8]] = True
    step = lambda toks: lg
    r = G.greedy_ref(step, [6], G.params(), None, TK, sup, cap=40, max_new=12)
    assert r["raw"] == [6, 9] + [0] * 11 + [5] and r["loop_exit"] == 0
    r2 = G.greedy_ref(step, [6], G.params(loop_period=1, loop_repeats=4), None, TK, sup, cap=40, max_new=12)
    assert r2["raw"] == [6, 9, 0, 0, 0, 0, 5] and r2["loop_exit"] == 1
    pr = np.exp(lg.astype(np.float64))
    a, b = math.log(pr[9] / pr.sum()), math.log(pr[0] / pr.sum())           # the first timestamp, then every 0
    assert r["avg_logprob"] * len(r["raw"]) == pytest.approx(a + 11 * b, rel=1e-9)
    assert r2["avg_logprob"] * len(r2["raw"]) == pytest.approx(a + 4 * b, rel=1e-9)   # eot after the exit: log 1 = 0
    r3 = G.greedy_ref(step, [6], G.params(no_repeat_ngram=1), None, TK, sup, cap=40, max_new=4)
    assert r3["raw"][:3] == [6, 9, 0] and 0 not in r3["raw"][3:]


def test_new_symbols_are_declared_and_exported():
    new = {"nh_set_guard", "nh_guard_bias", "nh_guard_report", "nh_guard_apply"}
    assert new <= set(hip.declared_symbols())
    L_ = hip.load_library()
    assert all(hasattr(L_, s) for s in new)
    import ctypes as C
    assert C.sizeof(hip.NhGuardParams) == 20 and C.sizeof(hip.NhDecodeResult) == 24


# ---- the pool policy -------------------------------------------------------------------------------------------------------
def Engine(loops=(), always=(), logprob=-0.5, nsp=0.1, with_guard=True):
    """every clip decodes for 2 steps (+ attempt) and collects as (logprob, nsp); with_guard=False: an engine without the
    guard's methods at all -- the pool must not ask for them"""
    return pool_standin.Engine([2] * 8, [[(logprob, nsp)] * 6] * 8, guard=with_guard, loops=loops, always=always)


GUARD = dict(no_repeat_ngram=3, loop_period=4, loop_repeats=3)


def test_pool_without_the_keywords_calls_no_guard_method():
    e = Engine(with_guard=False)
    res = pool.DecodePool(e, rows=2, staging=2, check_every=2, fallback=True).run(5, e.encode)
    assert [r["tokens"] for r in res] == [[c, 0] for c in range(5)]
    assert all("loop_exit" not in r for r in res)


def test_pool_sets_the_guard_once_and_reports_loop_exit():
    e = Engine(loops={1, 3})
    p = pool.DecodePool(e, rows=2, staging=2, check_every=2, guard=GUARD)
    res = p.run(5, e.encode)
    assert [c for c in e.log if c[0] == "set_guard"] == [("set_guard", GUARD)]
    assert [c[0] for c in e.log[:2]] == ["begin", "set_guard"]          # before the first admission
    assert [r["loop_exit"] for r in res] == [False, True, False, True, False]
    assert p.retries == 0 and not any(c[0] == "guard_bias" for c in e.log)
    # a guard without a loop exit: nothing to report, nothing asked
    e = Engine()
    res = pool.DecodePool(e, rows=2, staging=2, check_every=2, guard=dict(no_repeat_ngram=3)).run(3, e.encode)
    assert not any(c[0] == "guard_report" for c in e.log) and all("loop_exit" not in r for r in res)


def test_pool_bias_goes_to_the_row_before_its_admission():
    e = Engine()
    bias = lambda c: {100 + c: -INF} if c % 2 else None
    pool.DecodePool(e, rows=2, staging=2, check_every=2, guard=dict(bias=True), bias=bias).run(4, e.encode)
    seq = [c for c in e.log if c[0] in ("guard_bias", "admit")]
    for i in range(0, len(seq), 2):
        (_, row, b), (_, clip, dst, _lang) = seq[i], seq[i + 1]
        assert row == dst and b == bias(clip)
    assert len(seq) == 8


def test_loop_fallback_retries_the_looping_clip_only():
    e = Engine(loops={2}, always={4})
    p = pool.DecodePool(e, rows=2, staging=3, check_every=2, guard=GUARD, fallback=True, loop_fallback=True)
    res = p.run(6, e.encode)
    assert sorted((c[1], c[6]) for c in e.log if c[0] == "retry") == [(2, 1)] + [(4, a) for a in range(1, 6)]
    assert [r["attempt"] for r in res] == [0, 0, 1, 0, 5, 0]
    assert [r["accepted"] for r in res] == [True, True, True, True, False, True]      # clip 4 loops at every temperature: dropped
    assert res[2]["loop_exit"] is False and res[4]["loop_exit"] is True
    # without loop_fallback the flag is reported and nothing is retried; a silent clip is accepted although it looped
    e = Engine(loops={2}, always={4})
    p = pool.DecodePool(e, rows=2, staging=3, check_every=2, guard=GUARD, fallback=True)
    assert [r["attempt"] for r in p.run(6, e.encode)] == [0] * 6 and p.retries == 0
    e = Engine(always={1}, nsp=0.9)
    p = pool.DecodePool(e, rows=2, staging=3, check_every=2, guard=GUARD, fallback=True, loop_fallback=True)
    assert [r["attempt"] for r in p.run(3, e.encode)] == [0] * 3 and p.retries == 0


def test_fed_pool_guard_bias_and_loop_fallback():
    e, encs = Engine(loops={1}), [pool_standin.Encoder(), pool_standin.Encoder()]
    bias = lambda c: {100 + c: 1.0} if c % 2 else None
    p = pool.FedDecodePool(e, encs, rows=2, batch=2, check_every=2, guard=dict(GUARD, bias=True), bias=bias, fallback=True, loop_fallback=True)
    res = p.run(5, pool_standin.feeder(encs))
    assert e.log[0][0] == "begin" and e.log[1] == ("set_guard", dict(GUARD, bias=True)) and sum(c[0] == "set_guard" for c in e.log) == 1
    seq = [c for c in e.log if c[0] in ("guard_bias", "admit")]
    assert len(seq) == 10
    for i in range(0, len(seq), 2):
        (_, row, b), (_, clip, dst, _lang) = seq[i], seq[i + 1]
        assert row == dst and b == bias(clip)
    assert [r["attempt"] for r in res] == [0, 1, 0, 0, 0] and [r["loop_exit"] for r in res] == [False] * 5
    assert [(c[1], c[6]) for c in e.log if c[0] == "retry"] == [(1, 1)]
    # without the keywords: an engine that has none of the guard's methods
    e, encs = Engine(with_guard=False), [pool_standin.Encoder(), pool_standin.Encoder()]
    res = pool.FedDecodePool(e, encs, rows=2, batch=2, check_every=2).run(3, pool_standin.feeder(encs))
    assert [r["tokens"] for r in res] == [[c, 0] for c in range(3)]


# ---- the decode fixtures on the CPU oracle ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture_model(name):
    cfg, tk = common.make_config(name), common.tokens_for(name)
    steps = GF.loop_script(tk)
    om = common.build_oracle(cfg, tk, overrides=GF.overrides(cfg, tk, steps))
    return cfg, tk, steps, om, F.oracle_encodings(om, cfg, 2)


def sup_array(cfg, tk):
    sup = np.zeros(cfg.vocab_size, dtype=bool)
    sup[np.asarray(cfg.suppress_tokens, dtype=np.int64)] = True
    sup[tk.no_timestamps] = True
    return sup


@functools.lru_cache(maxsize=None)
def fixture_decode(name, case, b):
    cfg, tk, steps, om, xas = fixture_model(name)
    p, bias = GF.CASES[case]
    return G.greedy_ref(GF.oracle_logits(om, xas[b]), [tk.sot, tk.en, tk.transcribe], p, bias, tk, sup_array(cfg, tk),
                        cfg.max_target_positions - 1, max_new=len(steps))


@pytest.mark.parametrize("name", ["test-d128", "test-d256-mel128"])
def test_fixture_margins_and_events(name):
    cfg, tk, steps, om, xas = fixture_model(name)
    margins = {(case, b): fixture_decode(name, case, b)["min_margin"] for case in GF.CASES for b in range(2)}
    print(name, "margins", margins, "bar", GF.MARGIN)
    assert min(margins.values()) >= GF.MARGIN, margins
    off, X = fixture_decode(name, "off", 0), GF.X
    text = lambda r: [t for t in r["raw"][3:] if t < tk.eot]
    assert text(off) == X * GF.COPIES and off["loop_exit"] == 0            # the unguarded decode loops to the script's end
    g = om.decode(xas[0], max_new_tokens=len(steps))
    # guard off: the oracle's own decode (it sums its softmax serially in f32: ~1e-5 relative per step, 24 tokens)
    assert off["tokens"] == g["tokens"] and abs(off["avg_logprob"] - g["avg_logprob"]) < 5e-4
    ng = text(fixture_decode(name, "ngram", 0))
    assert not any(ng[i:i + 3] == ng[j:j + 3] for i in range(len(ng) - 2) for j in range(i + 1, len(ng) - 2)) and ng != text(off)
    pen = text(fixture_decode(name, "penalty", 0))
    assert pen != text(off) and pen[:3] == X
    ex = fixture_decode(name, "exit", 0)
    assert text(ex) == X * 2 and ex["loop_exit"] == 1 and ex["raw"][-1] == tk.eot and len(ex["raw"]) < len(off["raw"])
    assert 12000 not in text(fixture_decode(name, "all", 0))
