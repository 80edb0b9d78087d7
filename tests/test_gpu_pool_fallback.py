"""GPU: the temperature fallback of the decode pool -- nh_pool_retry and norma_amd/pool.py with fallback=True.

decode_with_fallback (src/models/whisper/model.rs:164-191) decodes a slice at TEMPERATURES = 0, 0.2 .. 1.0 until
avg_logprob >= -1 or no_speech_prob > 0.6 and drops it otherwise.  The lockstep path has that (nh_decode_sampled under the
seeded sampling contract of include/norma_hip.h, checked against the oracle in tests/test_gpu_sampling.py); here a row of a
pool that decodes its clip again, sampled, beside rows that are greedy, in their prompt, or sampled at another temperature
and another position, must give bit for bit what the clip gives in nh_decode_sampled of a lockstep batch -- and the greedy
rows beside it what they give in nh_decode_greedy.  No tolerance anywhere: every comparison is ==."""
import numpy as np
import pytest

import common
from norma_amd import config, pool, synth
from test_gpu_pool import _encode_into, _same, _varlen_weights

pytestmark = pytest.mark.gpu

NAME = "test-d128"            # vocabulary 51864: the large-vocabulary shape of the token kernels
INVALID, STATE = 1, 3         # NH_ERR_INVALID, NH_ERR_STATE


def _hip():
    from norma_amd import hip
    return hip


def _setup(N, pool_batch, graphs=True):
    hip = _hip()
    cfg, tk = config.preset(NAME), common.tokens_for(NAME)
    hm = _varlen_weights(cfg, tk, eot_steps=[2, 5, 9, 14, 22], text_steps=40, n_calib=8, max_batch=N)
    clips = np.stack([synth.synth_pcm(k) for k in range(N)])
    hm.logmel_array(clips); hm.encode()
    hp = hip.HipWhisper(cfg, device=0, max_batch=pool_batch, share_with=hm)
    hp.set_tokens(tk, tk.en, tk.transcribe)
    if not graphs:
        hp.set_option(hip.NH_OPT_DECODE_GRAPHS, 0)
    return cfg, tk, hm, hp, clips


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("check_every", [1, 16])
def test_sampled_retries_beside_greedy_rows_give_the_lockstep_bits(graphs, check_every):
    """Rows 0 .. 4 of an 8-row pool decode their clips again -- rows 0, 1, 3 first, rows 2 and 4 one pool_step call later, so
    with check_every = 1 the second retry lands off a NH_GRAPH_STEPS boundary and with 16 on one; rows 0 - 2 at (t1, attempt 1),
    rows 3, 4 at (t2, attempt 5) -- while fresh clips are admitted, greedy, into the other rows, and two more into the rows
    the first retries leave while the second ones still run.  Sampled rows, greedy rows and rows still in their prompt share
    steps at different positions."""
    N, R, seed, clip0 = 16, 8, 0x5EED_0123_4567_89AB, 1000
    (t1, a1), (t2, a2) = (0.4, 1), (1.0, 5)
    cfg, tk, hm, hp, clips = _setup(N, R + 8, graphs)
    want_g = hm.decode_greedy()
    want_s = {a1: hm.decode_sampled(t1, seed, clip0, a1), a2: hm.decode_sampled(t2, seed, clip0, a2)}
    assert len({len(r["tokens"]) for r in want_g}) >= 4                      # the greedy transcripts end at different steps
    assert all(not _same(want_s[a][c], want_g[c]) for a in (a1, a2) for c in range(N) if not want_g[c]["no_speech_exit"])
    encode = _encode_into(hp, clips)
    bad = []

    def check(kind, c, got, want):
        if not _same(got, want):
            bad.append((kind, c))

    # round 0: clips 0 .. 7, greedy, rows 0 .. 7
    hp.pool_begin(R, 0, False)
    encode(0, 8, R)
    for c in range(8):
        hp.pool_admit(R + c, c)
    owner = {r: ("g", r) for r in range(R)}          # row -> (kind, clip); kind "g" or the attempt of a retry
    for _ in range(2000):
        flags = hp.pool_step(check_every)
        if all(flags[r] in (1, 2) for r in range(R)):
            break
    for r, res in zip(range(R), hp.pool_collect(list(range(R)))):
        check("g", r, res, want_g[r])
    owner.clear()
    # round 1: retries of rows 0 .. 4 in two waves, clips 8 .. 15 greedy into whatever else is free
    encode(8, 8, R)                                  # staging rows R .. R + 7 hold clips 8 .. 15
    fresh, late = list(range(8, 14)), [14, 15]       # late: kept for the rows that the first retries leave
    ex_sampled = set()                               # rows whose last decode was a retry: an admit must make them greedy again
    waves = [[(0, t1, a1), (1, t1, a1), (3, t2, a2)], [(2, t1, a1), (4, t2, a2)]]
    held = {2, 4}                                    # rows that wait for the second wave: no admit into them
    shared = 0                                       # pool_step calls in which sampled and greedy rows were both busy
    for it in range(4000):
        if it < len(waves):
            for r, t, a in waves[it]:
                hp.pool_retry(r, t, seed, clip0 + r, a)
                owner[r] = (a, r)
                held.discard(r)
        for r in range(R):
            src = late if r in ex_sampled else fresh
            if r not in owner and r not in held and src:
                c = src.pop(0)
                hp.pool_admit(R + (c - 8), r)
                owner[r] = ("g", c)
                ex_sampled.discard(r)
        if not owner:
            break
        kinds = {k for k, _ in owner.values()}
        shared += ("g" in kinds and len(kinds) > 1)
        flags = hp.pool_step(check_every)
        fin = [r for r in sorted(owner) if flags[r] in (1, 2)]
        if fin:
            for r, res in zip(fin, hp.pool_collect(fin)):
                kind, c = owner.pop(r)
                check(kind, c, res, want_g[c] if kind == "g" else want_s[kind][c])
                if kind != "g":
                    ex_sampled.add(r)
    assert not owner and not fresh and not late, (owner, fresh, late)
    assert shared >= 2, shared
    assert not bad, bad
    hm.close(); hp.close()


def _policy(attempts, T, logprob_threshold, no_speech_threshold=0.6):
    """model.rs:175-190 on the lockstep decodes attempts[a][clip]"""
    out = []
    for c in range(len(attempts[0])):
        for a in range(len(T)):
            r = attempts[a][c]
            needs = r["avg_logprob"] < logprob_threshold
            if not needs or r["no_speech_prob"] > no_speech_threshold:
                out.append(dict(r, attempt=a, temperature=T[a], accepted=True))
                break
        else:
            out.append(dict(attempts[-1][c], attempt=len(T) - 1, temperature=T[-1], accepted=False))
    return out


def _lockstep_attempts(hm, T, seed, clip0):
    return [hm.decode_greedy()] + [hm.decode_sampled(T[a], seed, clip0, a) for a in range(1, len(T))]


def _assert_fallback_results(got, want):
    N = len(want)
    assert len(got) == N
    bad = [c for c in range(N) if not (_same(got[c], want[c]) and got[c]["attempt"] == want[c]["attempt"]
                                       and got[c]["accepted"] == want[c]["accepted"] and got[c]["temperature"] == want[c]["temperature"])]
    assert not bad, [(c, got[c]["attempt"], want[c]["attempt"], got[c]["accepted"], want[c]["accepted"]) for c in bad]


def _median_threshold(greedy):
    """a threshold that splits the clip set whatever the synthetic weights' confidence is: the median greedy avg_logprob"""
    thr = float(np.median([r["avg_logprob"] for r in greedy]))
    N = len(greedy)
    first = sum(1 for r in greedy if not r["avg_logprob"] < thr or r["no_speech_prob"] > 0.6)
    assert first >= N / 4 and N - first >= N / 4, (first, N, thr)     # precondition: a real mix of accepted and retried clips
    return thr


@pytest.mark.parametrize("rows,staging,check_every", [(6, 5, 8), (4, 7, 3)])
def test_fallback_through_the_pool_is_the_policy_on_six_lockstep_decodes(rows, staging, check_every):
    """DecodePool(fallback=True) against model.rs:175-190 evaluated on six lockstep decodes of the whole batch (t = 0, then
    nh_decode_sampled at 0.2 .. 1.0 with attempt = 1 .. 5): per clip the first accepted attempt, with its bits.

    The reference samples from softmax(q / t) over the rule-masked PROBABILITIES q in [0, 1], not over logits (model.rs:340-348),
    so at t <= 1 the weights differ by a factor of e^(1/t) at most over ~50 000 tokens: a retry is a near-uniform draw, its
    avg_logprob is far below any greedy one, and most retried clips end as dropped (accepted=False after five retries).  That
    is the reference's behaviour and what this test expects; it is not worked around."""
    N, seed, clip0 = 16, 0xFA11BACC, 300
    cfg, tk, hm, hp, clips = _setup(N, rows + staging)
    T = pool.TEMPERATURES
    attempts = _lockstep_attempts(hm, T, seed, clip0)
    thr = _median_threshold(attempts[0])
    want = _policy(attempts, T, thr)
    dp = pool.DecodePool(hp, rows=rows, staging=staging, check_every=check_every, fallback=True, seed=seed, clip0=clip0, logprob_threshold=thr)
    got = dp.run(N, _encode_into(hp, clips))
    _assert_fallback_results(got, want)
    assert dp.retries == sum(w["attempt"] for w in want) and dp.retries >= N / 4
    # the same pool object state without fallback: today's greedy results
    plain = pool.DecodePool(hp, rows=rows, staging=staging, check_every=check_every).run(N, _encode_into(hp, clips))
    assert all(_same(g, w) for g, w in zip(plain, attempts[0]))
    hm.close(); hp.close()


def test_fallback_through_a_pool_fed_by_two_encoder_contexts():
    hip = _hip()
    N, rows, batch, seed, clip0 = 16, 5, 4, 77, 9
    cfg, tk, hm, hp, clips = _setup(N, rows + 1)
    encs = [hip.HipWhisper(cfg, device=0, max_batch=batch, share_with=hm) for _ in range(2)]
    for h in encs:
        h.set_tokens(tk, tk.en, tk.transcribe)

    def encode(i, first, n):
        encs[i].logmel_array(np.ascontiguousarray(clips[first:first + n])); encs[i].encode()
    T = pool.TEMPERATURES
    attempts = _lockstep_attempts(hm, T, seed, clip0)
    thr = _median_threshold(attempts[0])
    want = _policy(attempts, T, thr)
    fp = pool.FedDecodePool(hp, encs, rows=rows, batch=batch, check_every=5, fallback=True, seed=seed, clip0=clip0, logprob_threshold=thr)
    got = fp.run(N, encode)
    _assert_fallback_results(got, want)
    assert fp.retries == sum(w["attempt"] for w in want)
    hm.close(); hp.close()
    for h in encs:
        h.close()


def test_retry_refusals_leave_the_pool_usable():
    hip = _hip()
    N, R, seed, clip0 = 8, 3, 11, 40                  # clips 0 .. 3 are used
    cfg, tk, hm, hp, clips = _setup(N, R + 4)
    want_g = hm.decode_greedy()
    want_s = hm.decode_sampled(0.6, seed, clip0, 3)

    def refused(code, match, *args):
        with pytest.raises(hip.HipError, match=match) as e:
            hp.pool_retry(*args)
        assert e.value.code == code, str(e.value)

    def finish(rows):
        for _ in range(2000):
            flags = hp.pool_step(4)
            if all(flags[r] in (1, 2) for r in rows):
                return hp.pool_collect(rows)
        raise AssertionError("rows did not finish")

    refused(STATE, "no decode pool", 0, 0.6, seed, clip0, 3)             # no pool
    hp.pool_begin(R, 0, False)
    refused(INVALID, "outside the pool", -1, 0.6, seed, clip0, 3)        # row out of range
    refused(INVALID, "outside the pool", R, 0.6, seed, clip0, 3)
    refused(STATE, "admitted", 1, 0.6, seed, clip0 + 1, 3)               # never admitted since nh_pool_begin
    _encode_into(hp, clips)(0, 4, R)
    hp.pool_admit(R + 0, 0); hp.pool_admit(R + 1, 1)
    refused(STATE, "busy", 0, 0.6, seed, clip0, 3)                       # busy (admitted, not collected)
    refused(STATE, "admitted", 2, 0.6, seed, clip0 + 2, 3)               # still never admitted
    hp.pool_step(2)
    refused(STATE, "busy", 1, 0.6, seed, clip0 + 1, 3)                   # busy, in the middle of its transcript
    got = finish([0, 1])
    assert _same(got[0], want_g[0]) and _same(got[1], want_g[1])         # the refusals launched nothing
    for t in (0.0, -0.5, float("nan"), float("inf")):                    # temperature <= 0, NaN, not finite
        refused(INVALID, "temperature", 0, t, seed, clip0, 3)
    hp.pool_retry(0, 0.6, seed, clip0 + 0, 3)
    refused(STATE, "busy", 0, 0.6, seed, clip0, 3)                       # busy on its retry
    hp.pool_admit(R + 2, 2)                                              # a greedy clip beside the retry
    refused(INVALID, "temperature", 1, 0.0, seed, clip0 + 1, 3)
    got = finish([0, 2])
    assert _same(got[0], want_s[0]) and _same(got[1], want_g[2])
    hp.pool_admit(R + 3, 0)                                              # the retried row, refilled: greedy again
    hp.pool_retry(1, 0.6, seed, clip0 + 1, 3)                            # row 1 still holds clip 1
    got = finish([0, 1])
    assert _same(got[0], want_g[3]) and _same(got[1], want_s[1])
    hp.pool_begin(R, 0, False)                                           # a new pool: nothing admitted yet
    refused(STATE, "admitted", 0, 0.6, seed, clip0, 3)
    hm.close(); hp.close()
