"""CPU: the temperature fallback of the decode pool (norma_amd/pool.py, fallback=True) against the scripted stand-in for the
engine (tests/pool_standin.py).  decode_with_fallback (src/models/whisper/model.rs:164-191) walks TEMPERATURES until avg_logprob >= -1 or
no_speech_prob > 0.6 and drops the clip otherwise; the pool does that per row: an admitted clip is attempt 0, every further
attempt is a pool_retry of the row the clip already sits in.  The GPU side is tests/test_gpu_pool_fallback.py."""
import numpy as np
import pytest

from norma_amd import pool
from pool_standin import BAD, GOOD, SILENT, Encoder, Engine, feeder


def make_script(N, rng):
    """accepted at attempt k (k = 0 .. 5), accepted by no_speech_prob at attempt k, or failing all six"""
    script, want = [], []
    for c in range(N):
        kind = c % 9 if c < 18 else int(rng.integers(0, 9))
        if kind <= 5:                                     # good at attempt `kind`
            script.append([BAD] * kind + [GOOD] * (6 - kind)); want.append((kind, True))
        elif kind == 6:                                   # silent at attempt 0: accepted although avg_logprob < -1
            script.append([SILENT] * 6); want.append((0, True))
        elif kind == 7:                                   # silent at attempt 2
            script.append([BAD, BAD, SILENT, BAD, BAD, BAD]); want.append((2, True))
        else:                                             # never
            script.append([BAD] * 6); want.append((5, False))
    return script, want


def run_pool(kind, N, lengths, script, rows, feed, check, **kw):
    e = Engine(lengths, script, clip0=kw.get("clip0", 0))
    if kind == "plain":
        p = pool.DecodePool(e, rows=rows, staging=feed, check_every=check, **kw)
        return e, p, p.run(N, e.encode, langs=list(range(1000, 1000 + N)))
    encs = [Encoder(), Encoder()]
    p = pool.FedDecodePool(e, encs, rows=rows, batch=feed, check_every=check, **kw)
    return e, p, p.run(N, feeder(encs), langs=list(range(1000, 1000 + N)))


@pytest.mark.parametrize("kind", ["plain", "fed"])
@pytest.mark.parametrize("rows,feed,check", [(4, 3, 2), (8, 8, 16), (2, 5, 1), (16, 6, 3)])
def test_fallback_walks_the_temperatures_per_clip_in_the_row_the_clip_sits_in(kind, rows, feed, check):
    rng = np.random.default_rng(rows * 10 + feed)
    N, clip0, seed = 41, 700, 0x1234_5678_9ABC
    lengths = [int(x) for x in rng.choice([3, 10, 40, 41], size=N)]
    script, want = make_script(N, rng)
    e, p, res = run_pool(kind, N, lengths, script, rows, feed, check, fallback=True, seed=seed, clip0=clip0)
    T = pool.TEMPERATURES
    assert T == (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)
    # results: clip order, the first accepted attempt (or the last one, dropped), with its numbers
    assert [r["clip"] for r in res] == list(range(N))
    for c, (r, (k, ok)) in enumerate(zip(res, want)):
        assert (r["attempt"], r["accepted"], r["temperature"]) == (k, ok, T[k]), c
        assert (r["avg_logprob"], r["no_speech_prob"]) == script[c][k] and r["tokens"] == [c, k], c
    assert any(r["accepted"] and r["avg_logprob"] < -1.0 and r["no_speech_prob"] > 0.6 for r in res)   # the no-speech half
    # every clip admitted once, in clip order
    assert [x[1] for x in e.log if x[0] == "admit"] == list(range(N))
    # retries: per clip attempts 1 .. k in order, temperature = T[attempt], clip id = clip0 + clip, the caller's seed,
    # and always in the row the clip was admitted to
    row_of = {x[1]: x[2] for x in e.log if x[0] == "admit"}
    per_clip = {c: [] for c in range(N)}
    for x in e.log:
        if x[0] == "retry":
            _, c, row, t, sd, cid, a = x
            assert row == row_of[c] and t == T[a] and sd == seed and cid == clip0 + c
            per_clip[c].append(a)
    for c, (k, ok) in enumerate(want):
        assert per_clip[c] == list(range(1, k + 1)), (c, per_clip[c], k)
    assert [len(per_clip[c]) for c in range(N) if not want[c][1]] == [5] * sum(not ok for _, ok in want)
    assert p.retries == sum(k for k, _ in want) == sum(1 for x in e.log if x[0] == "retry")
    # a row that owes a retry is never the target of an admit: between the collect that returned a failing attempt and the
    # clip's final answer, the only calls naming that row are the clip's own retries (the stand-in also refuses an admit
    # into a busy row; this covers the moment between collect and retry)
    owner = {}
    for x in e.log:
        if x[0] == "admit":
            assert x[2] not in owner, ("admitted into a row a clip still owns", x)
            owner[x[2]] = [x[1], 0]
        elif x[0] == "retry":
            assert owner[x[2]][0] == x[1]
            owner[x[2]][1] = x[6]
        elif x[0] == "collect":
            for r in x[1]:
                c, a = owner[r]
                if a == want[c][0]:
                    del owner[r]              # final: the row is free
    assert not owner
    assert p.steps % check == 0 and p.row_steps >= sum(lengths[c] * (want[c][0] + 1) for c in range(N))


@pytest.mark.parametrize("kind", ["plain", "fed"])
def test_thresholds_and_temperatures_are_the_callers(kind):
    N = 12
    lengths = [5] * N
    script = [[(-0.3 - 0.1 * c, 0.5)] * 3 for c in range(N)]       # avg_logprob -0.3 .. -1.4, the same at every attempt
    e, p, res = run_pool(kind, N, lengths, script, 4, 4, 2, fallback=True, seed=3, temperatures=(0.0, 0.5, 0.9), logprob_threshold=-0.85)
    for c, r in enumerate(res):
        fails = script[c][0][0] < -0.85
        assert (r["attempt"], r["accepted"], r["temperature"]) == ((2, False, 0.9) if fails else (0, True, 0.0)), c
    assert [(x[3], x[6]) for x in e.log if x[0] == "retry" and x[1] == N - 1] == [(0.5, 1), (0.9, 2)]
    # no_speech_threshold: 0.5 > 0.4 accepts everything at attempt 0
    e, p, res = run_pool(kind, N, lengths, script, 4, 4, 2, fallback=True, logprob_threshold=-0.85, no_speech_threshold=0.4)
    assert all(r["attempt"] == 0 and r["accepted"] for r in res) and not [x for x in e.log if x[0] == "retry"]


@pytest.mark.parametrize("kind", ["plain", "fed"])
def test_without_fallback_the_calls_are_what_they_were(kind):
    """fallback=False (the default): no pool_retry, whatever the numbers, and the very call sequence of a pool that knows
    nothing about fallback -- the one a run over all-accepted results makes."""
    rng = np.random.default_rng(5)
    N = 30
    lengths = [int(x) for x in rng.choice([3, 10, 40], size=N)]
    bad = [[BAD] * 6 for _ in range(N)]
    good = [[GOOD] * 6 for _ in range(N)]
    e0, p0, r0 = run_pool(kind, N, lengths, bad, 4, 3, 2)
    assert not [x for x in e0.log if x[0] == "retry"] and p0.retries == 0
    assert [r["clip"] for r in r0] == list(range(N))
    assert all((r["attempt"], r["temperature"], r["accepted"]) == (0, 0.0, True) for r in r0)
    if kind == "plain":                       # (the fed pool's admit / step interleaving depends on its encoder thread)
        e1, p1, r1 = run_pool(kind, N, lengths, good, 4, 3, 2, fallback=True)
        assert e0.log == e1.log and (p0.steps, p0.row_steps, p0.encodes) == (p1.steps, p1.row_steps, p1.encodes)
        # today's sequence, spelled out for the head of the run: begin, encode 3, admit 3, step, ...
        assert e0.log[:6] == [("begin", 4, False), ("encode", 0, 3), ("admit", 0, 0, 1000), ("admit", 1, 1, 1001), ("admit", 2, 2, 1002), ("step", 2)]
    assert {x[0] for x in e0.log} == {"begin", "encode", "admit", "step", "collect"} - ({"encode"} if kind == "fed" else set())


def test_constructor_keeps_its_positional_arguments():
    """bench.py and the tools construct the pools positionally and by keyword: the new arguments come last, with defaults"""
    p = pool.DecodePool(None, 64, 32, 0, 16, False)
    assert (p.rows, p.staging, p.max_new, p.check_every, p.per_clip_language, p.fallback) == (64, 32, 0, 16, False, False)
    f = pool.FedDecodePool(None, [None], 64, 32, 0, 16, False)
    assert (f.rows, f.batch, f.fallback, f.temperatures) == (64, 32, False, pool.TEMPERATURES)
    with pytest.raises(AssertionError):
        pool.DecodePool(None, fallback=True, temperatures=(0.2, 0.4))     # attempt 0 is the admitted, greedy decode
