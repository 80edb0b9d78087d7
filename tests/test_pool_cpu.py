"""CPU: the decode pool's refill policy (norma_amd/pool.py) against a counting stand-in for the engine -- every clip is
admitted once into a free row, collected once after it finished, results come back in clip order, the encoder is fed
`staging` clips at a time.  (The reference decodes one stream at a time, src/lib.rs:462-464, and ends each sequence at eot,
model.rs:317: no counterpart; the GPU side is tests/test_gpu_pool.py.)"""
import json
import os
import threading

import numpy as np
import pytest

from norma_amd import pool
from pool_standin import MUTE, TABLE, Encoder, Engine, feeder
from test_pool_fallback_cpu import make_script


@pytest.mark.parametrize("rows,staging,check", [(4, 3, 2), (8, 8, 16), (2, 5, 1), (64, 32, 16)])
def test_every_clip_is_admitted_once_collected_once_and_returned_in_clip_order(rows, staging, check):
    rng = np.random.default_rng(rows * 100 + staging)
    N = 57
    lengths = [int(x) for x in rng.choice([3, 10, 40, 41, 120], size=N)]
    e = Engine(lengths)
    e.busy_every = 3 if rows % 2 == 0 else 0   # half of the cases: an encoder that says "busy" two times out of three
    dp = pool.DecodePool(e, rows=rows, staging=staging, check_every=check)
    seen = []
    res = dp.run(N, e.encode, langs=list(range(1000, 1000 + N)), on_result=lambda c, r: seen.append(c))
    assert [r["clip"] for r in res] == list(range(N)) and [r["lang"] for r in res] == list(range(1000, 1000 + N))
    assert sorted(seen) == list(range(N))
    assert [x[1] for x in e.log if x[0] == "admit"] == list(range(N))          # admitted in clip order
    enc = [x for x in e.log if x[0] == "encode"]
    assert [x[1] for x in enc] == list(range(0, N, staging)) and sum(x[2] for x in enc) == N
    assert dp.encodes == len(enc) and e.max_concurrent <= rows
    assert dp.row_steps >= sum(lengths) and dp.steps % check == 0
    if N > rows + staging:
        assert e.max_concurrent == rows                                        # the pool does fill up


def test_pool_keeps_rows_busy_where_lockstep_batches_wait_for_the_longest():
    lengths = [300 if k % 16 == 0 else 20 for k in range(256)]
    e = Engine(lengths)
    dp = pool.DecodePool(e, rows=32, staging=32, check_every=4)
    dp.run(len(lengths), e.encode)
    lockstep = sum(32 * max(lengths[g:g + 32]) for g in range(0, len(lengths), 32))
    assert dp.row_steps < 0.5 * lockstep


@pytest.mark.parametrize("rows,batch,n_enc,check", [(8, 5, 2, 4), (64, 32, 2, 16), (3, 7, 1, 1), (16, 4, 3, 2)])
def test_one_pool_fed_by_encoder_contexts_admits_every_clip_once_in_order_and_reuses_a_context_only_when_it_is_drained(rows, batch, n_enc, check):
    rng = np.random.default_rng(rows + batch)
    N = 83
    lengths = [int(x) for x in rng.choice([3, 10, 40, 120], size=N)]
    e, encs = Engine(lengths), [Encoder() for _ in range(n_enc)]
    submissions = []
    fp = pool.FedDecodePool(e, encs, rows=rows, batch=batch, check_every=check)
    res = fp.run(N, feeder(encs, submissions), langs=list(range(500, 500 + N)))
    assert [r["clip"] for r in res] == list(range(N)) and [r["lang"] for r in res] == list(range(500, 500 + N))
    assert [x[1] for x in e.log if x[0] == "admit"] == list(range(N))
    assert [sbm[1] for sbm in submissions] == list(range(0, N, batch)) and [sbm[0] for sbm in submissions] == [k % n_enc for k in range(len(submissions))]
    assert fp.encodes == len(submissions) and fp.row_steps >= sum(lengths) and e.max_concurrent <= rows


def test_an_error_on_the_encoder_thread_reaches_the_caller():
    e, encs = Engine([5] * 20), [Encoder()]

    def encode(i, first, n):
        if first >= 8:
            raise RuntimeError("encoder failed")
        encs[i].rows = {k: first + k for k in range(n)}
    with pytest.raises(RuntimeError):
        pool.FedDecodePool(e, encs, rows=4, batch=4, check_every=2).run(20, encode)


def test_the_fed_pool_delivers_every_result_to_on_result_too():
    e, encs = Engine([3, 9, 4, 12, 5, 2, 7]), [Encoder(), Encoder()]
    seen = []
    res = pool.FedDecodePool(e, encs, rows=2, batch=3, check_every=2).run(7, feeder(encs), on_result=lambda c, r: seen.append((c, r)))
    assert sorted(c for c, _ in seen) == list(range(7)) and all(r is res[c] for c, r in seen)


@pytest.mark.parametrize("fail", [("pool_step", 1), ("pool_collect", 3)])
def test_an_error_on_the_calling_thread_stops_the_encoder_thread_and_reaches_the_caller(fail):
    """2 encoder contexts, 50 batches: the encoder thread needs one hand-back per batch, and a caller that has raised hands
    nothing back.  run() on a thread of its own with a 5 s cap: the stand-in does no work, and a run() that waits for its
    encoder thread never returns."""
    N, batch = 200, 4
    e, encs = Engine([3 + c % 5 for c in range(N)], fail=fail), [Encoder(), Encoder()]
    submissions, out = [], []
    fp = pool.FedDecodePool(e, encs, rows=4, batch=batch, check_every=2)

    def encode(i, first, n):
        encs[i].rows = {k: first + k for k in range(n)}
        submissions.append((i, first, n))

    def call():
        try:
            fp.run(N, encode)
        except BaseException as ex:   # noqa: BLE001 -- compared below
            out.append((ex, len(submissions), set(threading.enumerate())))
    before = set(threading.enumerate())
    th = threading.Thread(target=call, daemon=True)
    th.start()
    th.join(5.0)
    assert not th.is_alive(), "run() has not returned"
    (ex, encodes, threads), = out
    assert ex is e.error
    if fail[0] == "pool_collect":
        assert sum(x[0] == "collect" for x in e.log) == fail[1] - 1 > 0       # some clips had finished
    # the encoder thread was joined before run() raised: no thread of the pool's is left, and no encode came after
    assert threads - {th} == before and len(submissions) == encodes < N // batch


# ---- the plain pool's engine-call sequence -----------------------------------------------------------------------------------
TRACE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pool_trace_parent.json")
TRACE_GRID = [(4, 3, 2), (8, 8, 16), (2, 5, 1), (64, 32, 16)]
TRACE_GUARD = dict(no_repeat_ngram=3, loop_period=4, loop_repeats=3, bias=True)
TRACE_VARIANTS = {      # name: (the stand-in's switches, the pool's keywords)
    "plain": ({}, {}),
    "busy_encoder": ({}, {}),
    "fallback_detect": (dict(detect=True), dict(fallback=True, seed=11, clip0=700, detect_languages=TABLE)),
    "align": (dict(align=True), dict(fallback=True, seed=11, clip0=700, align_heads=[(1, 0), (0, 1)])),
    "guard_bias": (dict(guard=True, loops={2, 9, 30}, always={4, 17}),
                   dict(fallback=True, seed=11, clip0=700, guard=TRACE_GUARD, loop_fallback=True, bias=lambda c: {100 + c: 0.5 * c} if c % 3 else None)),
}


def pool_trace(variant, rows, staging, check):
    """the stand-in's call log of one DecodePool.run and the pool's counters, as JSON holds them"""
    N = 31                                                            # few clips and short decodes: the log is mostly steps
    rng = np.random.default_rng(rows * 100 + staging)
    lengths = [int(x) for x in rng.choice([2, 3, 5, 8], size=N)]
    script, _ = make_script(N, rng)
    for c in range(5, N, 11):
        script[c] = [MUTE] * 6
    switches, kw = TRACE_VARIANTS[variant]
    e = Engine(lengths, script, clip0=kw.get("clip0", 0), **switches)
    e.busy_every = 3 if variant == "busy_encoder" else 0
    p = pool.DecodePool(e, rows=rows, staging=staging, check_every=check, **kw)
    langs = [None if c % 3 else 51000 + c for c in range(N)] if "detect_languages" in kw else list(range(1000, 1000 + N))
    p.run(N, e.encode, langs=langs, n_keys=[1500 - 7 * c for c in range(N)])
    counters = dict(steps=p.steps, row_steps=p.row_steps, encodes=p.encodes, retries=p.retries, aligned=p.aligned)
    return json.loads(json.dumps(dict(log=e.log, counters=counters)))


@pytest.mark.parametrize("rows,staging,check", TRACE_GRID)
@pytest.mark.parametrize("variant", list(TRACE_VARIANTS))
def test_the_plain_pool_makes_the_engine_calls_it_made_before_the_two_run_loops_became_one(variant, rows, staging, check):
    """pool_trace_parent.json: pool_trace of every case, written by this file run as a script at the last commit that had
    DecodePool.run and FedDecodePool.run as two loops"""
    with open(TRACE_PATH) as f:
        want = json.load(f)[f"{variant}-{rows}-{staging}-{check}"]
    got = pool_trace(variant, rows, staging, check)
    assert got["counters"] == want["counters"]
    assert got["log"] == want["log"]


if __name__ == "__main__":
    with open(TRACE_PATH, "w") as f:
        json.dump({f"{v}-{r}-{s}-{c}": pool_trace(v, r, s, c) for v in TRACE_VARIANTS for r, s, c in TRACE_GRID}, f, separators=(",", ":"))
        f.write("\n")
