"""GPU: transcript scoring (nh_score, HipWhisper.score) end to end on tiny.en-sized synthetic weights whose
greedy decode follows a script (tests/common.py).

The bar.  Measured on the MI355X over the fixture's three clips (the scripted transcript of 17 tokens each): the largest
|hm.score - fp64 log-softmax of the CPU oracle's logits| of any scored token was 1.0755e-4 (printed by
test_score_matches_the_oracle; MEASURED below rounds it up); the bar is ten times that, 1.08e-3, the convention of
beam_fixture.G.  The difference is the fp16 decoder (one-pass forward, fp16 LayerNorm rows and embedding, f32 accumulation)
against the f32 oracle.  Against the decode's own sum_logprob the same run gave differences of 1.0e-4, 1.5e-5 and 1.2e-4 over
14 tokens, under a bar of 14 * 1.08e-3.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import beam_fixture as F
import common
import cut_ref as CR
from norma_amd import hip, longform

pytestmark = pytest.mark.gpu

NH_ERR_INVALID, NH_ERR_STATE = 1, 3
NAME = "tiny.en"
MEASURED = 1.08e-4
BAR = 10 * MEASURED
SMALL = (300, 100, 15)
CANARY = np.float32(7.25)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def fixture():
    """One oracle and one context (max_batch 4) on scripted weights; three clips of different lengths, encoded on the oracle."""
    cfg, tk = common.make_config(NAME), common.tokens_for(NAME)
    script = common.transcript_script(tk, n_segments=2, words_per_segment=5)
    om, (hm,) = common.build_together(cfg, tk, overrides=common.scripted_overrides(cfg, tk, script), batches=(4,))
    clips = F.clips(3)
    return cfg, tk, script, om, hm, clips, F.oracle_encodings(om, cfg, 3)


def encoded(clips=None):
    cfg, tk, script, om, hm, all_clips, xas = fixture()
    hm.logmel(all_clips if clips is None else clips)
    hm.encode()
    return hm


def oracle_logprobs(om, xa, tokens):
    """fp64 log-softmax of the oracle's logits at every given token but the first: entry i belongs to tokens[i]"""
    h = om.decoder_forward(list(tokens[:-1]), xa, True)
    lg = om.final_linear(h).astype(np.float64)
    lg -= lg.max(axis=1, keepdims=True)
    lsm = lg - np.log(np.exp(lg).sum(axis=1, keepdims=True))
    out = np.zeros(len(tokens))
    out[1:] = lsm[np.arange(len(tokens) - 1), np.asarray(tokens[1:])]
    return out


def test_score_matches_the_oracle():
    cfg, tk, script, om, hm, clips, xas = fixture()
    encoded()
    res = hm.decode_greedy()
    lp = hm.score([r["tokens"] for r in res])
    worst = 0.0
    for b, r in enumerate(res):
        t = r["tokens"]
        assert t == [tk.sot, tk.en, tk.transcribe] + script
        want = oracle_logprobs(om, xas[b], t)
        got = lp[b, :len(t)].astype(np.float64)
        assert (got[:3] == 0).all() and (lp[b, len(t):] == 0).all()
        assert np.isfinite(got).all() and (got[3:] < 0).all()
        worst = max(worst, float(np.abs(got[3:] - want[3:]).max()))
    print(f"largest |device - oracle| log-probability over {len(res)} clips: {worst:.4e}")
    assert worst <= BAR, worst


def test_score_sums_to_the_decodes_own_sum_logprob():
    """decode_beam(1) keeps the untrimmed sequence and its sum_logprob (nh_beam_hypotheses): the sum of the scores from the
    first generated token on is that sum.  The fixture ends by a natural eot, so no forced eot is part of it."""
    cfg, tk, script, om, hm, clips, xas = fixture()
    encoded()
    res = hm.decode_beam(1)
    seqs, sums = [], []
    for r in res:
        assert len(r["hypotheses"]) == 1
        t, s = r["hypotheses"][0]
        assert t[-1] == tk.eot and len(t) < cfg.max_target_positions - 1, "the hypothesis hit the length cap"
        seqs.append(t); sums.append(s)
    lp = hm.score(seqs)
    for b, (t, s) in enumerate(zip(seqs, sums)):
        got = float(lp[b, 3:len(t)].astype(np.float64).sum())
        print(f"clip {b}: sum of scores {got:.6f}, sum_logprob {s:.6f}, n - P = {len(t) - 3}")
        assert abs(got - s) <= (len(t) - 3) * BAR, (b, got, s)


def test_a_clip_has_the_same_bits_in_any_batch_and_under_any_padding():
    cfg, tk, script, om, hm, clips, xas = fixture()
    Cn = cfg.max_target_positions
    full = [tk.sot, tk.en, tk.transcribe] + script
    assert len(full) >= 17
    ns = [5, 9, 17]
    toks = np.zeros((3, Cn), dtype=np.int32)
    for b, n in enumerate(ns):
        toks[b, :n] = full[:n]
    encoded()
    together = hm.score(toks, n_tokens=ns)
    for b, n in enumerate(ns):
        assert (together[b, :3] == 0).all() and (together[b, n:] == 0).all() and (together[b, 3:n] < 0).all()
    noisy = toks.copy()
    rng = np.random.default_rng(9)
    for b, n in enumerate(ns):
        noisy[b, n:] = rng.integers(0, cfg.vocab_size, size=Cn - n)
    assert same_bits(hm.score(noisy, n_tokens=ns), together)
    for b, n in enumerate(ns):
        encoded(clips[b:b + 1])
        alone = hm.score(toks[b:b + 1], n_tokens=[n])
        assert same_bits(alone[0], together[b]), b


def test_score_leaves_the_next_decode_alone_and_ends_the_kept_alignment():
    cfg, tk, script, om, hm, clips, xas = fixture()
    encoded()
    g0 = hm.decode_greedy()
    hm.score([r["tokens"] for r in g0])
    assert hm.decode_greedy() == g0
    hm.align_capture([(0, 0)])
    try:
        g1 = hm.decode_greedy()
        first, last = hm.align_decoded()
        hm.score([r["tokens"] for r in g1])
        with pytest.raises(hip.HipError) as e:
            hm.align_decoded()
        assert e.value.code == NH_ERR_STATE
        assert hm.decode_greedy() == g1
        f2, l2 = hm.align_decoded()
        assert np.array_equal(first, f2) and np.array_equal(last, l2)
    finally:
        hm.align_capture([])
    assert hm.decode_greedy() == g0


def _refused(hm, code, toks, nt, prompt_len=3, null=()):
    out = np.full((hm.batch, hm.cfg.max_target_positions), CANARY, dtype=np.float32)
    a = None if "tokens" in null else hip._ip(toks)
    n = None if "n_tokens" in null else hip._ip(nt)
    o = None if "out" in null else hip._fp(out)
    assert hm.L.nh_score(hm._h, a, n, prompt_len, o) == code, (code, null, prompt_len, nt)
    assert (out == CANARY).all()


def test_refusals_leave_the_output_untouched():
    cfg, tk, script, om, hm, clips, xas = fixture()
    Cn, V = cfg.max_target_positions, cfg.vocab_size
    full = [tk.sot, tk.en, tk.transcribe] + script
    encoded()
    g0 = hm.decode_greedy()
    toks = np.zeros((3, Cn), dtype=np.int32)
    toks[:, :len(full)] = full
    nt = np.full(3, len(full), dtype=np.int32)
    for null in ("tokens", "n_tokens", "out"):
        _refused(hm, NH_ERR_INVALID, toks, nt, null=(null,))
    assert hm.L.nh_score(None, hip._ip(toks), hip._ip(nt), 3, None) == NH_ERR_INVALID
    for p in (0, -1):
        _refused(hm, NH_ERR_INVALID, toks, nt, prompt_len=p)
    for bad in (3, 2, 0, -1, Cn + 1):                       # n_tokens outside (prompt_len, max_target_positions]
        n2 = nt.copy(); n2[1] = bad
        _refused(hm, NH_ERR_INVALID, toks, n2)
    for bad in (-1, V, V + 7):                              # a token id outside the vocabulary among the first n_tokens
        t2 = toks.copy(); t2[2, len(full) - 1] = bad
        _refused(hm, NH_ERR_INVALID, t2, nt)
    t2 = toks.copy(); t2[:, len(full):] = V + 7              # ... past them it is not looked at
    want = hm.score(toks, n_tokens=nt)
    assert same_bits(hm.score(t2, n_tokens=nt), want)
    n2 = nt.copy(); n2[0] = Cn                               # the upper end of the range is accepted
    t3 = toks.copy(); t3[0, len(full):] = 1000
    assert np.isfinite(hm.score(t3, n_tokens=n2)).all()
    hm.set_option(hip.NH_OPT_ABSORBED_XATTN, 1)
    try:
        _refused(hm, NH_ERR_STATE, toks, nt)
    finally:
        hm.set_option(hip.NH_OPT_ABSORBED_XATTN, 0)
    encoded()
    hm.pool_begin(1)                                         # a running decode pool
    _refused(hm, NH_ERR_STATE, toks, nt)
    hm.logmel(clips)                                         # a fresh batch ends the pool; nothing is encoded yet
    _refused(hm, NH_ERR_STATE, toks, nt)
    hm.encode()
    assert same_bits(hm.score(toks, n_tokens=nt), want)
    assert hm.decode_greedy() == g0


def test_a_width_that_is_no_multiple_of_128_is_refused():
    cfg = common.make_config("test-d128", d_model=64, encoder_attention_heads=1, decoder_attention_heads=1)
    try:
        hm = hip.HipWhisper(cfg, max_batch=1)
    except hip.HipError as e:
        pytest.skip(f"no context exists at d_model = 64 to refuse on (nh_create: {e})")
    hm.close()
    pytest.fail("nh_create accepts d_model = 64 now: build the d = 64 fixture and check nh_score's NH_ERR_STATE here")


def test_transcribe_recording_with_scores():
    cfg, tk, script, om, hm, clips, xas = fixture()
    x = CR.noise(160 * 1400, "score")
    plain = longform.transcribe_recording(hm, x, SMALL)
    scored = longform.transcribe_recording(hm, x, SMALL, score=True)
    assert len(plain) == len(scored) > hm.max_batch, "more than one group"
    for p, s in zip(plain, scored):
        assert set(s) == set(p) | {"token_logprob"}
        for k in p:
            assert np.array_equal(p[k], s[k]) if isinstance(p[k], np.ndarray) else p[k] == s[k], k
    starts, lens = hm.cut_plan(x, params=SMALL)
    for a in range(0, len(starts), hm.max_batch):
        hm.logmel([x[s:s + n] for s, n in zip(starts[a:a + hm.max_batch], lens[a:a + hm.max_batch])])
        hm.encode()
        res = hm.decode_greedy()
        lp = hm.score([r["tokens"] for r in res])
        for i, r in enumerate(res):
            got = scored[a + i]["token_logprob"]
            assert got.dtype == np.float32 and same_bits(got, lp[i, :len(r["tokens"])]), a + i
            assert (got[:3] == 0).all() and (got[3:] < 0).all()


def test_transcribe_recording_scores_under_a_prompt():
    """score=True with prompt=: the prefix goes in front of the returned tokens and prompt_len counts it"""
    cfg, tk, script, om, hm, clips, xas = fixture()
    x = CR.noise(160 * 500, "score under a prompt")
    prefix = [tk.no_speech - 1, 1111, 2222, 3333, 4444]          # <|startofprev|> and four words: the one-pass prefill
    scored = longform.transcribe_recording(hm, x, SMALL, prompt=prefix, score=True)
    assert scored == [] or "token_logprob" in scored[0]
    starts, lens = hm.cut_plan(x, params=SMALL)
    assert 1 <= len(starts) <= hm.max_batch
    hm.logmel([x[s:s + n] for s, n in zip(starts, lens)])
    hm.encode()
    hm.set_prompts([prefix] * len(starts))
    res = hm.decode_greedy()
    assert [r["tokens"] for r in res] == [s["tokens"] for s in scored]
    assert all(len(r["tokens"]) > 3 for r in res), "a no-speech exit: nothing to score in this fixture"
    lp = hm.score([prefix + r["tokens"] for r in res], prompt_len=len(prefix) + 3)
    for i, r in enumerate(res):
        n = len(r["tokens"])
        got = scored[i]["token_logprob"]
        assert same_bits(got, lp[i, len(prefix):len(prefix) + n]), i
        assert (got[:3] == 0).all() and (got[3:] < 0).all() and (lp[i, :len(prefix) + 3] == 0).all()
        # the decode summed the same tokens' log-probabilities: avg_logprob is that sum over the returned length
        if r["tokens"][-1] == tk.eot and n < cfg.max_target_positions - len(prefix) - 1 and r["tokens"][-2] <= tk.no_timestamps:
            assert abs(float(got.astype(np.float64).sum()) / n - r["avg_logprob"]) <= BAR
