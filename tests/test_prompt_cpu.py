"""CPU: the reference for prompted decodes (tests/prompt_ref.py) against the oracle's own decode, the meaning of a prefix
(cap, early exit, trailing-timestamp trim, what comes back), the history rule of host.Model on its pure-Python model, and
the margins of the scripted fixture the GPU tests of tests/test_gpu_prompt.py decode: checked here, before any GPU run."""
import numpy as np

import common
import prompt_ref as R
from norma_amd import assets_io, synth


def _small(script, name="test-d128", **over):
    O = common.oracle_module()
    cfg, tk = common.make_config(name, **over), common.tokens_for(name)
    om = common.build_oracle(cfg, tk, overrides=common.scripted_overrides(cfg, tk, script))
    xa = om.encoder_forward(O.pcm_to_mel(synth.synth_pcm(0), assets_io.mel_filters(cfg.num_mel_bins))[:, :3000])
    return cfg, tk, om, xa


def test_empty_prefix_is_the_oracles_decode_exactly():
    tk = common.tokens_for("test-d128")
    cfg, tk, om, xa = _small(common.transcript_script(tk, n_segments=3, words_per_segment=5))
    for kw in (dict(), dict(max_new_tokens=7), dict(max_new_tokens=8, temperature=0.6, seed=5, clip=2, attempt=3)):
        want, got = om.decode(xa, **kw), R.prompted_decode(om, xa, [], **kw)
        assert got["tokens"] == want["tokens"], kw
        assert got["avg_logprob"] == want["avg_logprob"] and got["no_speech_prob"] == want["no_speech_prob"], kw
    om.close()


def test_argmax_total_keeps_the_last_maximum_and_ranks_nan_first():
    import ctypes as C
    O = common.oracle_module()
    rng = np.random.default_rng(2)
    for case in range(6):
        p = rng.random(500).astype(np.float32)
        if case & 1:
            p[[17, 300]] = p.max() + 1           # a tie: the last one wins
        if case & 2:
            p[44] = -np.inf
        if case == 5:
            p[123] = np.nan
        assert R.argmax_total(p) == O.lib().wo_argmax_total(p.ctypes.data_as(C.POINTER(C.c_float)), len(p))


def test_prefix_shifts_positions_and_is_not_part_of_what_comes_back():
    tk = common.tokens_for("test-d128")
    cfg, tk, om, xa = _small(R.long_script(tk))
    script = R.long_script(tk)
    for n in (1, 5):
        r = R.prompted_decode(om, xa, R.prefix_tokens(tk, n))
        k = script.index(tk.eot, n)
        assert r["tokens"] == [tk.sot, tk.en, tk.transcribe] + script[n:k + 1], n   # generation starts at script[n]
        assert r["physical_len"] == n + len(r["tokens"]) and not r["no_speech_exit"]
        assert r["min_gap"] >= 10 * R.LOGIT_BAR
    # the trailing-timestamp trim works on the returned sequence: 6 new tokens end on the first segment's closing timestamp
    r = R.prompted_decode(om, xa, R.prefix_tokens(tk, 5), max_new_tokens=6)
    assert script[10] > tk.no_timestamps and r["physical_len"] == 5 + 3 + 6 + 1
    assert r["tokens"] == [tk.sot, tk.en, tk.transcribe] + script[5:10] + [tk.eot]
    # avg_logprob is over the sequence from sot on (before the trim), whatever the prefix length
    full = R.prompted_decode(om, xa, R.prefix_tokens(tk, 5))
    assert -0.5 < full["avg_logprob"] < 0.0
    om.close()


def test_length_cap_counts_the_physical_sequence():
    """on a 64-position decoder (the loop re-runs the whole sequence per token): the largest prefix, 64 / 2 - 1, and a
    segment that never closes"""
    tk = common.tokens_for("test-d128")
    C, n = 64, 31
    cfg, tk, om, xa = _small(R.long_script(tk, endless_from=n, C=C), max_target_positions=C)
    r = R.prompted_decode(om, xa, R.prefix_tokens(tk, n))
    assert r["physical_len"] == C and len(r["tokens"]) == C - n and r["tokens"][-1] == tk.eot
    assert r["tokens"][:4] == [tk.sot, tk.en, tk.transcribe, tk.zero_sec] and r["min_gap"] >= 10 * R.LOGIT_BAR
    om.close()


def test_no_speech_exit_reads_the_logits_at_sots_position():
    """the probe fires on position n's logits: a positional row that points at <|nospeech|> there, and nowhere else"""
    name = "test-d128"
    cfg, tk = common.make_config(name), common.tokens_for(name)
    n = 5
    script = [R.FILLER] * 448
    script[n:n + 3] = [tk.zero_sec, 700, tk.eot]
    over = common.scripted_overrides(cfg, tk, script)
    emb = over["model.decoder.embed_tokens.weight"]
    pos = over["model.decoder.embed_positions.weight"].copy()
    gain = np.float32(1.2 / (0.02 * max(1.0, 14.0 / (cfg.d_model * 0.02))))
    pos[n] = (gain * emb[tk.no_speech]).astype(np.float16).astype(np.float32)
    over["model.decoder.embed_positions.weight"] = pos
    O = common.oracle_module()
    om = common.build_oracle(cfg, tk, overrides=over)
    xa = om.encoder_forward(O.pcm_to_mel(synth.synth_pcm(0), assets_io.mel_filters(cfg.num_mel_bins))[:, :3000])
    r = R.prompted_decode(om, xa, R.prefix_tokens(tk, n))
    assert r["no_speech_exit"] and r["no_speech_prob"] > 0.6 and r["avg_logprob"] == 0.0
    assert r["tokens"] == [tk.sot, tk.en, tk.transcribe]
    assert not R.prompted_decode(om, xa, R.prefix_tokens(tk, 1))["no_speech_exit"]   # sot elsewhere: no exit
    om.close()


def test_history_and_truncation_rule_of_the_host_model():
    C, sop = 448, 50360
    h = R.PromptHistory(sop, C)                                   # both settings off: never a prefix
    h.accept([1, 2, 3])
    assert h.prefix() == []
    h = R.PromptHistory(sop, C, initial=[7, 8])                   # an initial prompt alone: the same prefix for every slice
    h.accept([1, 2, 3])
    assert h.prefix() == [sop, 7, 8]
    h = R.PromptHistory(sop, C, initial=[7, 8], condition_on_previous=True)
    assert h.prefix() == [sop, 7, 8]
    h.accept([1, 2, 3]); h.accept([4])
    assert h.prefix() == [sop, 7, 8, 1, 2, 3, 4]
    h.accept(list(range(100, 400)))                               # cut to the LAST C / 2 - 2 ids behind <|startofprev|>
    p = h.prefix()
    assert len(p) == C // 2 - 1 and p[0] == sop and p[1:] == list(range(400 - 222, 400))
    h.accept([5, 6], temperature=0.6)                             # accepted above 0.5: the history goes, the slice's text too
    assert h.prefix() == [sop, 7, 8]
    h.accept([9], temperature=0.4)
    assert h.prefix() == [sop, 7, 8, 9]
    h.final_chunk()
    assert h.prefix() == [sop, 7, 8] and h.history == []
    h = R.PromptHistory(sop, C, condition_on_previous=True)       # history alone
    assert h.prefix() == []
    h.accept([1])
    assert h.prefix() == [sop, 1]


def test_scripted_tiny_en_margins_are_ten_times_the_logit_bar():
    """the fixture of tests/test_gpu_prompt.py: at every generated step of every decode it asks for, the oracle's top-2 gap
    among the tokens the rules allow is at least 10 x the logit bar (0.04 sigma), so a token mismatch on the GPU cannot be a tie"""
    cfg, tk, over, om, xas, mels = R.scripted_fixture()
    script = R.long_script(tk)
    for n in R.PREFIX_LENGTHS:
        for b in range(2):
            r = R.prompted_decode(om, xas[b], R.prefix_tokens(tk, n, b))
            k = script.index(tk.eot, n)
            assert r["tokens"] == [tk.sot, tk.en, tk.transcribe] + script[n:k + 1], (n, b)
            assert r["min_gap"] >= 10 * R.LOGIT_BAR, (n, b, r["min_gap"])
