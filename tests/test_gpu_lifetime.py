"""GPU: who owns a context's device memory.  One test-d128 context (scripted weights) makes every buffer a feature allocates
on first use -- alignment workspace and query buffer, guard flags and bias table, cut and speech-map workspaces, resample
records, beam and score buffers, the absorbed-attention scratch -- and must decode afterwards what it decoded before, bit for
bit; it is closed, and a second context in the same process decodes the same.  The allocation failures these owners exist for
cannot be provoked here; what runs is every path that creates, carves and releases them."""
import numpy as np
import pytest

import common
import cut_ref as CR
from norma_amd import config, hip, synth

pytestmark = pytest.mark.gpu

NAME = "test-d128"
HEADS3 = [(0, 1), (1, 0), (0, 0)]


def _bits(v):
    return np.float64(v).tobytes()   # identical means the same bits (a NaN equals itself here)


def _same(a, b):
    return len(a) == len(b) and all(x["tokens"] == y["tokens"] and _bits(x["avg_logprob"]) == _bits(y["avg_logprob"]) and
                                    _bits(x["no_speech_prob"]) == _bits(y["no_speech_prob"]) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def setup():
    cfg, tk = config.preset(NAME), common.tokens_for(NAME)
    script = common.transcript_script(tk, n_segments=3, words_per_segment=6)
    return cfg, tk, script, common.scripted_overrides(cfg, tk, script)


def _decode(hm, clip):
    hm.logmel([clip])
    hm.encode()
    return hm.decode_greedy()


def test_a_context_that_made_every_lazy_buffer_decodes_as_before_and_dies_cleanly(setup):
    cfg, tk, script, over = setup
    clip = synth.synth_pcm(0)
    hm = common.build_hip(cfg, tk, overrides=over, max_batch=3)
    R0 = _decode(hm, clip)
    toks = R0[0]["tokens"]
    assert toks == [tk.sot, tk.en, tk.transcribe] + script
    # alignment: the workspace and the query buffer of three heads, then the decode's own queries, then the DTW alone
    first, last = hm.align([toks], prompt_len=3, heads=HEADS3)
    assert first[0, 3] == 0 and last[0, len(toks) - 1] == 1499
    hm.align_capture(HEADS3[:2])
    assert _same(hm.decode_greedy(), R0)
    f2, l2 = hm.align_decoded()
    assert f2[0, 3] == 0 and l2[0, len(toks) - 1] == 1499
    hm.align_capture([])
    gf, gl = hm.align_path(np.arange(20 * 7, dtype=np.float32).reshape(20, 7) % 5)
    assert gf[0] == 0 and gl[-1] == 6
    # the guard: flags and bias table
    hm.set_guard(no_repeat_ngram=3, bias=True)
    hm.guard_bias(0, {int(script[1]): -0.25, int(script[2]): 0.5})
    assert len(hm.decode_greedy()[0]["tokens"]) > 3 and hm.guard_report() == [0]
    hm.set_guard()
    # long recordings: the cut planner and the speech map on 70 s
    rec, _ = CR.bursts(7, 70.0)
    starts, lens = hm.cut_plan(rec)
    assert len(starts) >= 3 and starts[0] == 0 and (lens > 0).all()
    p_starts, p_lens, chunk_first = hm.vad_plan(rec)
    assert len(p_starts) >= 1 and chunk_first[0] == 0 and chunk_first[-1] == len(p_starts)
    # audio ingest: one 44.1 kHz clip
    t = np.arange(44100, dtype=np.float64) / 44100.0
    out = hm.resample(np.sin(2 * np.pi * 440.0 * t).astype(np.float32)[None], 44100)
    assert len(out) == 1 and abs(len(out[0]) - 16000) <= 1 and np.isfinite(out[0]).all() and np.abs(out[0]).max() > 0.5
    # beam search and scoring
    beam = hm.decode_beam(2)
    assert beam[0]["tokens"][:3] == toks[:3] and len(beam[0]["hypotheses"]) >= 1
    lp = hm.score([toks])
    assert np.isfinite(lp).all() and (lp[0, 3:len(toks)] <= 0).all() and not lp[0, len(toks):].any()
    # the absorbed cross-attention prototype and back
    hm.set_option(hip.NH_OPT_ABSORBED_XATTN, 1)
    assert hm.decode_greedy()[0]["tokens"][:3] == toks[:3]
    hm.set_option(hip.NH_OPT_ABSORBED_XATTN, 0)
    # ... and the context decodes what it decoded before any of it
    assert _same(hm.decode_greedy(), R0)
    hm.close()
    h2 = common.build_hip(cfg, tk, overrides=over, max_batch=3)
    try:
        assert _same(_decode(h2, clip), R0)
    finally:
        h2.close()


def test_apply_rules_twice_on_a_context_of_one_row(setup):
    """a max_batch 1 context has no second logits row: the masked row goes through a buffer that lives for the call"""
    cfg, tk, script, over = setup
    hm = common.build_hip(cfg, tk, overrides=over, max_batch=1)
    try:
        r = np.random.default_rng(11)
        e = np.exp(r.standard_normal(cfg.vocab_size) * 3)
        probs = (e / e.sum()).astype(np.float32)
        tokens = [tk.sot, tk.en, tk.transcribe, tk.zero_sec + 5, 700]   # after an opening timestamp and one word
        m1, a1 = hm.apply_rules(probs, tokens, tk.zero_sec + 5)
        m2, a2 = hm.apply_rules(probs, tokens, tk.zero_sec + 5)
        assert a1 == a2 and 0 <= a1 < cfg.vocab_size and np.array_equal(m1.view(np.uint32), m2.view(np.uint32))
        assert not np.array_equal(m1.view(np.uint32), probs.view(np.uint32)), "the rules masked nothing"
    finally:
        hm.close()
