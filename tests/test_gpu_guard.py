"""GPU: the repetition guard inside the decodes (nh_set_guard): greedy against tests/guard_ref.py driven by the
CPU oracle, the loop exit without relying on the model, guard off == never guarded bit for bit, the pool, sampled decodes and
their pool retries, beam search, the refusals.  The fixtures are tests/guard_fixture.py: tests/test_guard_cpu.py asserts that
every decision of every case is at least MARGIN from its runner-up on the oracle, so no case is ever skipped as undecided."""
import ctypes as C
import functools

import numpy as np
import pytest

import beam_fixture as F
import common
import guard_fixture as GF
import guard_ref as G
from norma_amd import hip, pool, synth
from test_gpu_pool import _encode_into, _same

pytestmark = pytest.mark.gpu

INVALID, STATE = 1, 3
NAME = "test-d128"
INF = float("inf")


@functools.lru_cache(maxsize=None)
def _fixture(name=NAME):
    """the oracle and one context (max_batch 16) on the loop fixture's weights; two clips encoded on the oracle"""
    cfg, tk = common.make_config(name), common.tokens_for(name)
    steps = GF.loop_script(tk)
    om, (hm,) = common.build_together(cfg, tk, overrides=GF.overrides(cfg, tk, steps), batches=(16,))
    return cfg, tk, steps, om, hm, F.clips(2), F.oracle_encodings(om, cfg, 2)


def _sup(cfg, tk):
    sup = np.zeros(cfg.vocab_size, dtype=bool)
    sup[np.asarray(cfg.suppress_tokens, dtype=np.int64)] = True
    sup[tk.no_timestamps] = True
    return sup


def _guard(hm, p, bias=None, rows=()):
    hm.set_guard(**vars(p))
    for r in rows:
        hm.guard_bias(r, bias)


def _clear(hm, rows=range(16)):
    hm.set_guard(None)
    for r in rows:
        hm.guard_bias(r, None)


def _text(tokens, tk):
    return [t for t in tokens[3:] if t < tk.eot]


def _bits(results):
    return [(r["tokens"], r["avg_logprob"], r["no_speech_prob"], r["no_speech_exit"]) for r in results]


# ------------------------------------------------------------------------------------------------ 1. greedy vs the reference
@pytest.mark.parametrize("name", [NAME, "test-d256-mel128"])
@pytest.mark.parametrize("case", sorted(GF.CASES))
def test_greedy_decode_matches_the_reference(name, case):
    cfg, tk, steps, om, hm, clips, xas = _fixture(name)
    p, bias = GF.CASES[case]
    hm.logmel(clips); hm.encode()
    _guard(hm, p, bias, rows=range(2))
    got = hm.decode_greedy(max_new_tokens=len(steps))
    flags = hm.guard_report()
    _clear(hm)
    for b in range(2):
        ref = G.greedy_ref(GF.oracle_logits(om, xas[b]), [tk.sot, tk.en, tk.transcribe], p, bias, tk, _sup(cfg, tk),
                           cfg.max_target_positions - 1, max_new=len(steps))
        print(name, case, b, "margin", ref["min_margin"], "avg_logprob", got[b]["avg_logprob"], ref["avg_logprob"], "loop_exit", flags[b])
        assert ref["min_margin"] >= GF.MARGIN                     # decided: the comparison below is never skipped
        assert got[b]["tokens"] == ref["tokens"], (b, got[b]["tokens"], ref["tokens"])
        assert len(got[b]["tokens"]) == ref["n_tokens"]
        assert flags[b] == ref["loop_exit"]
        assert abs(got[b]["avg_logprob"] - ref["avg_logprob"]) <= 5e-3, (got[b]["avg_logprob"], ref["avg_logprob"])


# ------------------------------------------------------------------------------------------- 2. the exit, model or no model
def test_loop_exit_ends_a_decode_that_a_bias_forces_into_a_loop():
    cfg, tk, steps, om, hm, clips, xas = _fixture()
    T, R, max_new = 777, 5, 30
    hm.logmel(clips); hm.encode()
    _guard(hm, G.params(bias=True, loop_period=1, loop_repeats=R), {T: 1e4}, rows=range(2))
    got = hm.decode_greedy(max_new_tokens=max_new)
    flags = hm.guard_report()
    _guard(hm, G.params(bias=True), {T: 1e4}, rows=range(2))
    loop = hm.decode_greedy(max_new_tokens=max_new)
    flags_off = hm.guard_report()
    _clear(hm)
    for b in range(2):
        t = got[b]["tokens"]
        # the first-token rule forces a timestamp, then text only, then R copies of T and eot right behind them
        assert t[:3] == [tk.sot, tk.en, tk.transcribe] and t[3] > tk.no_timestamps and t[4:] == [T] * R + [tk.eot], t
        assert flags[b] == 1 and flags_off[b] == 0
        assert loop[b]["tokens"][4:] == [T] * (max_new - 1) + [tk.eot]       # without the exit: to max_new_tokens


# --------------------------------------------------------------------------------------------------------------- 3. guard off
def test_guard_off_leaves_every_bit_and_a_change_reaches_the_captured_steps():
    cfg, tk, steps, om, hm, clips, xas = _fixture()
    n = len(steps)
    fresh = hip.HipWhisper(cfg, device=0, max_batch=4, share_with=hm)       # a context that never saw the API
    fresh.set_tokens(tk, tk.en, tk.transcribe)
    fresh.logmel(clips); fresh.encode()
    base = fresh.decode_greedy(max_new_tokens=n)
    base_s = fresh.decode_sampled(0.7, seed=5, clip0=3, attempt=2, max_new_tokens=n)
    hm.logmel(clips); hm.encode()
    _guard(hm, *GF.CASES["all"], rows=range(2))
    assert _bits(hm.decode_greedy(max_new_tokens=n)) != _bits(base)
    hm.set_guard(None)                                                      # the lists stay: off is off
    assert _bits(hm.decode_greedy(max_new_tokens=n)) == _bits(base)
    assert _bits(hm.decode_sampled(0.7, seed=5, clip0=3, attempt=2, max_new_tokens=n)) == _bits(base_s)
    assert hm.guard_report() == [0, 0]
    _clear(hm)
    # off -> on -> off on one context, graphs enabled (the default), one shape: the graph key carries the guard
    first = fresh.decode_greedy(max_new_tokens=n)
    fresh.set_guard(no_repeat_ngram=3)
    second = fresh.decode_greedy(max_new_tokens=n)
    fresh.set_guard(no_repeat_ngram=3, repetition_penalty=1.6)              # on -> on with other parameters
    other = fresh.decode_greedy(max_new_tokens=n)
    fresh.set_guard(None)
    third = fresh.decode_greedy(max_new_tokens=n)
    assert _bits(first) == _bits(base) == _bits(third)
    assert _bits(second) != _bits(first) and _bits(other) != _bits(second)
    fresh.close()


# -------------------------------------------------------------------------------------------------------------------- 4. pool
N_POOL = 6


@functools.lru_cache(maxsize=None)
def _pool_setup():
    cfg, tk, steps, om, hm, _, _ = _fixture()
    clips = np.stack([synth.synth_pcm(k) for k in range(N_POOL)])
    hp = hip.HipWhisper(cfg, device=0, max_batch=3 + 3, share_with=hm)
    hp.set_tokens(tk, tk.en, tk.transcribe)
    return cfg, tk, steps, hm, hp, clips


def _clip_bias(c):
    """odd clips may not say X0 (so they never loop), clip 4 has a hotword"""
    return {GF.X[0]: -INF} if c % 2 else ({GF.RUNNERS[1]: 3.0} if c == 4 else None)


POOL_GUARD = dict(no_repeat_ngram=5, repetition_penalty=1.02, loop_period=3, loop_repeats=2, bias=True)


def _lockstep_guarded(hm, clips, n):
    hm.logmel_array(clips); hm.encode()
    hm.set_guard(**POOL_GUARD)
    for c in range(len(clips)):
        hm.guard_bias(c, _clip_bias(c))
    want = hm.decode_greedy(max_new_tokens=n)
    flags = hm.guard_report()
    _clear(hm)
    return want, flags


def test_guarded_pool_rows_give_the_guarded_lockstep_bits():
    cfg, tk, steps, hm, hp, clips = _pool_setup()
    n = len(steps)
    want, flags = _lockstep_guarded(hm, clips, n)
    dp = pool.DecodePool(hp, rows=3, staging=3, max_new_tokens=n, check_every=4, guard=POOL_GUARD, bias=_clip_bias)
    got = dp.run(N_POOL, _encode_into(hp, clips))
    _clear(hp, range(6))
    for c in range(N_POOL):
        assert _same(got[c], want[c]), (c, got[c]["tokens"], want[c]["tokens"])
        assert got[c]["loop_exit"] == bool(flags[c])
        # per-row bias: -inf keeps X0 out of the odd clips' rows only
        assert (GF.X[0] in got[c]["tokens"]) == (c % 2 == 0)
    assert [bool(f) for f in flags] == [c % 2 == 0 for c in range(N_POOL)]      # the even clips loop and leave by the exit
    assert len({len(r["tokens"]) for r in got}) >= 2


def test_probe_prompt_and_language_detection_keep_their_bits_beside_guarded_rows():
    """2 rows, 6 clips: every clip after the second is admitted while the other row generates, so its probe, its language
    detection and its prompt positions share steps with a row the guard edits"""
    cfg, tk, steps, hm, hp, clips = _pool_setup()
    n = len(steps)
    langs = [tk.en, tk.en + 1, tk.en + 2, tk.en + 5]
    runs = []
    for guard in (None, POOL_GUARD):
        dp = pool.DecodePool(hp, rows=2, staging=3, max_new_tokens=n, check_every=3, detect_languages=langs, guard=guard,
                             bias=_clip_bias if guard else None)
        runs.append(dp.run(N_POOL, _encode_into(hp, clips)))
        _clear(hp, range(6))
    for c, (a, g) in enumerate(zip(*runs)):
        assert a["no_speech_prob"] == g["no_speech_prob"] and a["language"] == g["language"], c
        assert np.array_equal(np.asarray(a["language_probs"]).view(np.uint32), np.asarray(g["language_probs"]).view(np.uint32)), c
    assert any(a["tokens"] != g["tokens"] for a, g in zip(*runs))


def test_set_guard_is_refused_while_a_row_is_busy():
    cfg, tk, steps, hm, hp, clips = _pool_setup()
    n = len(steps)
    hm.logmel_array(clips[:2]); hm.encode()
    want = hm.decode_greedy(max_new_tokens=n)
    hp.pool_begin(3, n, False)
    _encode_into(hp, clips)(0, 2, 3)
    hp.pool_admit(3, 0); hp.pool_admit(4, 1)
    hp.pool_step(2)
    for kw in (dict(no_repeat_ngram=3), None):
        with pytest.raises(hip.HipError) as ei:
            hp.set_guard(**kw) if kw else hp.set_guard(None)
        assert ei.value.code == STATE
    for _ in range(40):
        flags = hp.pool_step(4)
        if all(flags[r] in (1, 2) for r in (0, 1)):
            break
    got = hp.pool_collect([0, 1])
    assert all(_same(g, w) for g, w in zip(got, want))           # the refused calls changed nothing
    assert hp.guard_report([0, 1]) == [0, 0]
    hp.set_guard(no_repeat_ngram=3)                              # no row busy: accepted
    hp.set_guard(None)


def test_loop_fallback_retries_the_looping_clips_only():
    cfg, tk, steps, hm, hp, clips = _pool_setup()
    n = len(steps)
    dp = pool.DecodePool(hp, rows=3, staging=3, max_new_tokens=n, check_every=4, guard=POOL_GUARD, bias=_clip_bias,
                         fallback=True, loop_fallback=True, seed=7, temperatures=(0.0, 0.8, 1.0), logprob_threshold=-50.0)
    got = dp.run(N_POOL, _encode_into(hp, clips))
    _clear(hp, range(6))
    for c, r in enumerate(got):
        if c % 2:
            assert r["attempt"] == 0 and r["accepted"] and not r["loop_exit"], (c, r)
        else:                                                    # took the exit at t = 0: retried whatever its avg_logprob
            assert r["attempt"] >= 1 and (r["accepted"] != r["loop_exit"]), (c, r)
    assert dp.retries >= 3


# ----------------------------------------------------------------------------------------------------------------- 5. sampled
def test_sampled_decode_under_a_guard_and_its_pool_retry():
    cfg, tk, steps, hm, hp, clips = _pool_setup()
    # the contract samples from softmax(q / t) over PROBABILITIES q: t = 0.04 keeps most draws on the likely tokens
    n, t, seed, clip0, att = len(steps), 0.04, 0xABCDEF12345, 40, 3
    p = dict(no_repeat_ngram=2, repetition_penalty=1.3)
    hm.logmel_array(clips[:3]); hm.encode()
    hm.set_guard(**p)
    want = hm.decode_sampled(t, seed, clip0, att, max_new_tokens=n)
    hm.set_guard(None)
    plain = hm.decode_sampled(t, seed, clip0, att, max_new_tokens=n)
    assert _bits(plain) != _bits(want)
    for r in want:                                               # no text bigram twice
        tx = _text(r["tokens"], tk)
        big = list(zip(tx, tx[1:]))
        assert len(big) == len(set(big)), tx
    hp.pool_begin(3, n, False)
    hp.set_guard(**p)
    _encode_into(hp, clips)(0, 3, 3)
    for c in range(3):
        hp.pool_admit(3 + c, c)

    def finish():
        for _ in range(40):
            flags = hp.pool_step(4)
            if all(flags[r] in (1, 2) for r in range(3)):
                return hp.pool_collect([0, 1, 2])
        raise AssertionError("rows did not finish")
    finish()
    for c in range(3):
        hp.pool_retry(c, t, seed, clip0 + c, att)
    got = finish()
    hp.set_guard(None)
    assert all(_same(g, w) for g, w in zip(got, want)), [(g["tokens"], w["tokens"]) for g, w in zip(got, want)]


# -------------------------------------------------------------------------------------------------------------------- 6. beam
def test_beam_search_under_a_guard():
    cfg, tk, steps, om, hm, clips, xas = _fixture()
    n, N = len(steps), 3
    hm.logmel(clips); hm.encode()
    hm.set_guard(no_repeat_ngram=N, bias=True)
    hm.guard_bias(0, {GF.X[1]: -INF})
    greedy = hm.decode_greedy(max_new_tokens=n)
    k1 = hm.decode_beam(1, max_new_tokens=n)
    assert [r["tokens"] for r in k1] == [r["tokens"] for r in greedy]
    k3 = hm.decode_beam(3, max_new_tokens=n)
    with pytest.raises(hip.HipError) as ei:
        hm.guard_report()
    assert ei.value.code == STATE
    for b, r in enumerate(k3):
        assert len(r["hypotheses"]) >= 1
        for toks, _ in r["hypotheses"]:
            tx = _text(toks, tk)
            grams = [tuple(tx[i:i + N]) for i in range(len(tx) - N + 1)]
            assert len(grams) == len(set(grams)), (b, tx)
            # clip 0's -inf holds in every hypothesis row of clip 0 and in none of clip 1's
            assert (GF.X[1] in tx) == (b == 1), (b, tx)
    hm.decode_greedy(max_new_tokens=n)
    assert hm.guard_report() == [0, 0]                           # a greedy decode afterwards is reported on again
    _clear(hm)


# --------------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_leave_parameters_lists_and_the_next_decode_untouched():
    cfg, tk, steps, om, hm, clips, xas = _fixture()
    n, V = len(steps), cfg.vocab_size
    hm.logmel(clips); hm.encode()
    _guard(hm, *GF.CASES["all"], rows=range(2))
    want = _bits(hm.decode_greedy(max_new_tokens=n))
    want_flags = hm.guard_report()

    def refused(fn, *a, **kw):
        with pytest.raises(hip.HipError) as ei:
            fn(*a, **kw)
        assert ei.value.code == INVALID, (a, kw, ei.value)
        assert _bits(hm.decode_greedy(max_new_tokens=n)) == want and hm.guard_report() == want_flags, (a, kw)
    for kw in (dict(repetition_penalty=float("nan")), dict(repetition_penalty=0.0), dict(repetition_penalty=-1.5),
               dict(repetition_penalty=INF), dict(no_repeat_ngram=17), dict(no_repeat_ngram=-1), dict(loop_period=65, loop_repeats=2),
               dict(loop_period=-1), dict(loop_period=64, loop_repeats=8), dict(loop_period=2, loop_repeats=1),
               dict(loop_period=2, loop_repeats=17), dict(loop_period=2)):
        refused(hm.set_guard, **kw)
    refused(hm.guard_bias, -1, {5: 1.0})
    refused(hm.guard_bias, 16, {5: 1.0})
    refused(hm.guard_bias, 0, {300 + i: 0.5 for i in range(hip.NH_GUARD_MAX_BIAS + 1)})
    refused(hm.guard_bias, 0, {V: 1.0})
    refused(hm.guard_bias, 1, {-1: 1.0})
    refused(hm.guard_bias, 0, {5: float("nan")})
    refused(hm.guard_bias, 1, {5: INF})

    def twice(row):       # an id twice: not expressible as a dict
        tk_, bv = np.array([9, 12000, 9], dtype=np.int32), np.array([1.0, 2.0, 3.0], dtype=np.float32)
        hm._chk(hm.L.nh_guard_bias(hm._h, row, tk_.ctypes.data_as(C.POINTER(C.c_int32)), bv.ctypes.data_as(C.POINTER(C.c_float)), 3))
    refused(twice, 0)
    _clear(hm)


# --------------------------------------------------------------------------------------------------------------- 8. host API
def test_host_model_guard_and_loop_exit():
    from norma_amd import host
    cfg, tk = common.make_config(NAME), common.tokens_for(NAME)
    steps = GF.loop_script(tk)
    over = GF.overrides(cfg, tk, steps)
    d = host.Definition(host.ModelType.TinyEn, host.SelectedDevice.Rocm(0))
    model = d.blocking_try_to_model(cfg, tk, tk.en, tk.transcribe,
                                    ((n, a.astype(np.float16)) for n, a in synth.synth_weights(cfg, 0, over)))
    model.set_temperature_fallback(False, 0)
    pcm = synth.synth_pcm(0)

    def flat(segs):
        out = []
        for s in segs:
            out += [int(t) for t in (s if isinstance(s, (list, tuple)) else s.tokens)]
        return out
    plain = flat(model.transcribe(pcm, final_chunk=True))
    r0 = model.last_result()
    assert r0["loop_exit"] is False and plain.count(GF.X[0]) == GF.COPIES
    model.set_repetition_guard(loop_period=3, loop_repeats=2)
    cut = flat(model.transcribe(pcm, final_chunk=True))
    r1 = model.last_result()
    assert r1["loop_exit"] is True and cut.count(GF.X[0]) == 2 and r1["n_tokens"] < r0["n_tokens"]
    model.set_repetition_guard(bias=True)
    model.set_token_bias({GF.X[0]: -INF})
    biased = flat(model.transcribe(pcm, final_chunk=True))
    assert GF.X[0] not in biased and GF.X[1] in biased and model.last_result()["loop_exit"] is False
    with pytest.raises(host.WhisperError):
        model.set_repetition_guard(repetition_penalty=0.0)
    with pytest.raises(host.WhisperError):
        model.set_token_bias({cfg.vocab_size: 1.0})
    assert flat(model.transcribe(pcm, final_chunk=True)) == biased          # the refused calls changed nothing
    model.set_repetition_guard()
    model.set_token_bias(None)
    assert flat(model.transcribe(pcm, final_chunk=True)) == plain and model.last_result() == r0
    model.close()


# ---------------------------------------------------------------------------------------------------------------- 9. longform
def test_longform_passes_guard_and_bias_through():
    from norma_amd import longform
    cfg, tk, steps, om, hm, clips, xas = _fixture()
    n = len(steps)
    rec = np.concatenate([synth.synth_pcm(0, 400000), synth.synth_pcm(1, 300000)])      # 43.75 s: more than one chunk
    plain = longform.transcribe_recording(hm, rec, max_new_tokens=n)
    assert len(plain) >= 2 and all("loop_exit" not in r for r in plain)
    assert all(_text(r["tokens"], tk).count(GF.X[0]) == GF.COPIES for r in plain)
    cut = longform.transcribe_recording(hm, rec, max_new_tokens=n, guard=dict(loop_period=3, loop_repeats=2))
    assert [r["start_sample"] for r in cut] == [r["start_sample"] for r in plain]
    assert all(r["loop_exit"] is True and _text(r["tokens"], tk) == GF.X * 2 for r in cut)
    biased = longform.transcribe_recording(hm, rec, max_new_tokens=n, guard=dict(bias=True, loop_period=3, loop_repeats=2),
                                           bias={GF.X[0]: -INF})
    assert all(r["loop_exit"] is False and GF.X[0] not in r["tokens"] and GF.X[1] in r["tokens"] for r in biased)
    # the call owns the context's guard: off and the lists cleared afterwards
    again = longform.transcribe_recording(hm, rec, max_new_tokens=n)
    assert [_bits([r]) for r in again] == [_bits([r]) for r in plain]
    speech = longform.transcribe_speech(hm, rec, max_new_tokens=n, guard=dict(loop_period=3, loop_repeats=2))
    assert len(speech) >= 1 and all(r["loop_exit"] is True for r in speech)
