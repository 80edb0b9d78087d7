"""GPU: decoder prompts (nh_set_prompts) and the one-pass teacher-forced decoder forward (nh_decoder_forward_onepass).

References: the oracle's decoder_forward / final_linear for the one-pass forward (the project's own bars: hidden <= 5e-3,
logits <= 4e-3 max(sigma, 0.1)), tests/prompt_ref.py for prompted decodes (tokens identical -- tests/test_prompt_cpu.py
asserts the fixture's margins at ten times the logit bar --, avg_logprob and no_speech_prob within the 1e-3 of the existing
decode tests)."""
import numpy as np
import pytest

import common
import prompt_ref as R
from norma_amd import assets_io, config, hip, host, longform, synth

pytestmark = pytest.mark.gpu

NH_ERR_INVALID, NH_ERR_STATE = 1, 3


def _oracle():
    from oracle import oracle as O
    return O


# ------------------------------------------------------------------------------------------------ the one-pass forward
def _forward_parity(name, enc, dec, B, Ts, seed=3):
    O = _oracle()
    cfg = common.make_config(name, encoder_layers=enc, decoder_layers=dec)
    tk = common.tokens_for(name)
    om = common.build_oracle(cfg, tk)
    hm = common.build_hip(cfg, tk, max_batch=B)
    filt = assets_io.mel_filters(cfg.num_mel_bins)
    mels = np.stack([O.pcm_to_mel(synth.synth_pcm(k), filt)[:, :3000] for k in range(B)])
    hm.set_mel(mels)
    hm.encode()
    xas = [om.encoder_forward(m) for m in mels]
    rng = np.random.default_rng(seed)
    out = []
    for T in Ts:
        toks = rng.integers(0, cfg.vocab_size, size=(B, T)).astype(np.int32)
        hid = hm.decoder_forward_onepass(toks)
        for b in range(B):
            ref_h = om.decoder_forward(toks[b], xas[b], True)
            ref_l, got_l = om.final_linear(ref_h), hm.final_linear(hid[b])
            r = dict(name=name, T=T, b=b, hid_err=float(np.abs(hid[b] - ref_h).max()), logit_err=float(np.abs(got_l - ref_l).max()),
                     logit_std=float(ref_l.std()))
            print(r)
            out.append(r)
    hm.close(); om.close()
    return out


# T: one position, less than / exactly / more than one 16-query wave and one 32-key k-step, one and more than one 64-key block,
# the largest prefix of a decode (223: 14 waves, four key blocks)
@pytest.mark.parametrize("name,enc,dec,B,Ts", [("test-d128", 1, 2, 3, (1, 2, 31, 32, 33, 64, 65, 223)),
                                               ("test-d256-mel128", 1, 2, 2, (33,)),
                                               ("distil-large-v3", 1, 1, 2, (33,))])
def test_onepass_forward_matches_the_oracle(name, enc, dec, B, Ts):
    for r in _forward_parity(name, enc, dec, B, Ts):
        assert r["hid_err"] <= 5e-3, r
        assert r["logit_err"] <= 4e-3 * max(r["logit_std"], 0.1), r


def test_onepass_forward_past_one_query_tile():
    """T > 256: two query tiles per (clip, head), the second with keys the first never stages"""
    for r in _forward_parity("test-d128", 0, 2, 2, (300,)):
        assert r["hid_err"] <= 5e-3 and r["logit_err"] <= 4e-3 * max(r["logit_std"], 0.1), r


def test_a_clip_is_bit_identical_alone_and_in_a_batch():
    name = "test-d128"
    cfg, tk = common.make_config(name), common.tokens_for(name)
    over = common.scripted_overrides(cfg, tk, R.long_script(tk))
    _, (h3, h1) = common.build_together(cfg, tk, overrides=over, batches=(3, 1), with_oracle=False)
    clips = [synth.synth_pcm(k) for k in range(3)]
    h3.logmel(clips); h3.encode()
    h1.logmel(clips[1:2]); h1.encode()
    rng = np.random.default_rng(8)
    for T in (65, 223):
        toks = rng.integers(0, cfg.vocab_size, size=(3, T)).astype(np.int32)
        assert np.array_equal(h3.decoder_forward_onepass(toks)[1], h1.decoder_forward_onepass(toks[1:2])[0]), T
    for n in (5, 223):
        pre = [R.prefix_tokens(tk, n, b) for b in range(3)]
        h3.set_prompts(pre); h1.set_prompts(pre[1:2])
        a, b = h3.decode_greedy()[1], h1.decode_greedy()[0]
        assert a == b and len(a["tokens"]) > 4, n   # tokens, avg_logprob and no_speech_prob: the same bits
    h3.close(); h1.close()


@pytest.mark.parametrize("n", (33, 223))
def test_the_one_pass_leaves_the_prefix_in_the_self_cache(n):
    """What the positions after the prefix read is the self K/V cache the one pass filled, and the scripted fixtures hardly
    look at it (their positional rows decide).  Here self-attention is loud (v_proj and out_proj x 4 on the seed-0 weights),
    so that the no-speech probability -- read at sot's position, right behind the prefix -- moves with the prefix's
    CONTENTS: four clips, four prefixes, a fresh context (a cache left unwritten would hold zeros), the one-pass route.
    Bar: every logit within 4e-3 max(sigma, 0.1) (the project's logit bar) puts log p within twice that."""
    O = _oracle()
    name = "test-d128"
    cfg, tk = common.make_config(name), common.tokens_for(name)
    over = {}
    for l in range(cfg.decoder_layers):
        for w in ("v_proj", "out_proj"):
            key = f"model.decoder.layers.{l}.self_attn.{w}.weight"
            over[key] = (synth.synth_tensor_by_name(cfg, key, 0) * np.float32(4)).astype(np.float16).astype(np.float32)
    om, (hm,) = common.build_together(cfg, tk, overrides=over, batches=(4,))
    filt = assets_io.mel_filters(cfg.num_mel_bins)
    mel = O.pcm_to_mel(synth.synth_pcm(0), filt)[:, :3000]
    hm.set_mel(np.stack([mel] * 4))                        # the same audio four times: only the prefixes differ
    hm.encode()
    xa = om.encoder_forward(mel)
    pre = [R.prefix_tokens(tk, n, c) for c in range(4)]
    want, sigma = [], 0.0
    for c in range(4):
        lg = om.final_linear(om.decoder_forward(pre[c] + [tk.sot], xa, True)[-1])[0]
        want.append(float(np.log(R.softmax_f32(lg)[tk.no_speech])))
        sigma = max(sigma, float(lg.std()))
    tol = 2 * 4e-3 * max(sigma, 0.1)
    hm.set_prompts(pre)
    got = [float(np.log(r["no_speech_prob"])) for r in hm.decode_greedy(max_new_tokens=1)]
    print(n, "want", want, "got", got, "tol", tol)
    assert max(want) - min(want) >= 10 * tol               # the contents matter, far beyond the bar
    assert max(abs(g - w) for g, w in zip(got, want)) <= tol
    hm.set_option(hip.NH_OPT_PROMPT_STEPWISE, 1)
    step = [float(np.log(r["no_speech_prob"])) for r in hm.decode_greedy(max_new_tokens=1)]
    assert max(abs(g - w) for g, w in zip(step, want)) <= tol
    hm.close(); om.close()


# ------------------------------------------------------------------------------------------------ prompted decodes
@pytest.fixture(scope="module")
def tiny():
    cfg, tk, over, om, xas, mels = R.scripted_fixture()
    hm = common.build_hip(cfg, tk, overrides=over, max_batch=2)
    hm.set_mel(mels)
    hm.encode()
    refs = {}

    def ref(n, b, **kw):
        key = (n, b, tuple(sorted(kw.items())))
        if key not in refs:
            refs[key] = R.prompted_decode(om, xas[b], R.prefix_tokens(tk, n, b), **kw)
        return refs[key]
    yield cfg, tk, hm, ref
    hm.close()


def _same(got, want, tol=1e-3):
    assert got["tokens"] == want["tokens"]
    assert abs(got["avg_logprob"] - want["avg_logprob"]) <= tol and abs(got["no_speech_prob"] - want["no_speech_prob"]) <= tol
    assert got["no_speech_exit"] == want["no_speech_exit"]


@pytest.mark.parametrize("n", R.PREFIX_LENGTHS)
def test_prompted_greedy_decode_stepwise_and_one_pass_match_the_reference(tiny, n):
    """n = 1 lies below the length from which the default route takes the one pass (4): both runs are stepwise there"""
    cfg, tk, hm, ref = tiny
    pre = [R.prefix_tokens(tk, n, b) for b in range(2)]
    for stepwise in (1, 0):
        hm.set_option(hip.NH_OPT_PROMPT_STEPWISE, stepwise)
        hm.set_prompts(pre)
        res = hm.decode_greedy()
        for b in range(2):
            print(n, stepwise, b, res[b]["avg_logprob"] - ref(n, b)["avg_logprob"], res[b]["no_speech_prob"] - ref(n, b)["no_speech_prob"])
            _same(res[b], ref(n, b))
            assert res[b]["tokens"][:3] == [tk.sot, tk.en, tk.transcribe]   # the prefix is not part of what comes back
    hm.set_prompts(None)


def test_step_graphs_are_keyed_by_the_prefix_length(tiny):
    """a new n_prefix captures the step again, an equal one replays; eager launches give the same bits"""
    cfg, tk, hm, ref = tiny
    hm.set_option(hip.NH_OPT_PROMPT_STEPWISE, 0)
    runs = []
    for n, graphs in ((5, 1), (223, 1), (5, 1), (5, 0)):
        hm.set_option(hip.NH_OPT_DECODE_GRAPHS, graphs)
        hm.set_prompts([R.prefix_tokens(tk, n, b) for b in range(2)])
        runs.append(hm.decode_greedy())
    hm.set_option(hip.NH_OPT_DECODE_GRAPHS, 1)
    hm.set_prompts(None)
    assert runs[0] == runs[2] == runs[3] and runs[0] != runs[1]
    _same(runs[1][0], ref(223, 0))


@pytest.mark.parametrize("n", (5, 223))
def test_prompted_sampled_decode_matches_the_reference(tiny, n):
    cfg, tk, hm, ref = tiny
    kw = dict(temperature=0.6, seed=77, attempt=2, max_new_tokens=8)
    hm.set_option(hip.NH_OPT_PROMPT_STEPWISE, 0)
    hm.set_prompts([R.prefix_tokens(tk, n, b) for b in range(2)])
    res = hm.decode_sampled(0.6, seed=77, clip0=10, attempt=2, max_new_tokens=8)
    greedy = hm.decode_greedy(max_new_tokens=8)
    hm.set_prompts(None)
    for b in range(2):
        want = ref(n, b, clip=10 + b, **kw)   # step = the physical token count: it is what the reference draws with
        _same(res[b], want, tol=2e-2)         # the bar of tests/test_gpu_sampling.py: a flat sampled distribution
        assert want["avg_logprob"] < -1.0 and res[b]["tokens"] != greedy[b]["tokens"]


def test_returned_shape_and_length_cap():
    """n_prefix = 223 and a segment that never closes: the decode ends at physical length C; tokens and n_tokens exclude the
    prefix.  On a 64-position decoder the same against the reference."""
    name = "test-d128"
    tk = common.tokens_for(name)
    for C, n in ((448, 223), (64, 31)):
        cfg = common.make_config(name, max_target_positions=C)
        over = common.scripted_overrides(cfg, tk, R.long_script(tk, endless_from=n, C=C))
        hm = common.build_hip(cfg, tk, overrides=over, max_batch=2)
        clips = [synth.synth_pcm(0), synth.synth_pcm(1)]
        hm.logmel(clips); hm.encode()
        with pytest.raises(hip.HipError) as e:
            hm.set_prompts([R.prefix_tokens(tk, n + 1, b) for b in range(2)])   # C / 2 is one too many
        assert e.value.code == NH_ERR_INVALID
        hm.set_prompts([R.prefix_tokens(tk, n, b) for b in range(2)])
        res = hm.decode_greedy()
        for b in range(2):
            t = res[b]["tokens"]
            assert len(t) == C - n and t[-1] == tk.eot and t[:4] == [tk.sot, tk.en, tk.transcribe, tk.zero_sec], (C, b)
            assert tk.eot not in t[:-1]
        if C == 64:
            O = _oracle()
            om = common.build_oracle(cfg, tk, overrides=over)
            filt = assets_io.mel_filters(cfg.num_mel_bins)
            for b in range(2):
                _same(res[b], R.prompted_decode(om, om.encoder_forward(O.pcm_to_mel(clips[b], filt)[:, :3000]), R.prefix_tokens(tk, n, b)))
            om.close()
        hm.close()


def _small_pair(max_batch=2, with_oracle=False):
    name = "test-d128"
    cfg, tk = common.make_config(name), common.tokens_for(name)
    over = common.scripted_overrides(cfg, tk, R.long_script(tk))
    om, (hm,) = common.build_together(cfg, tk, overrides=over, batches=(max_batch,), with_oracle=with_oracle)
    return cfg, tk, om, hm


def test_no_prefix_leaves_todays_decode_alone():
    cfg, tk, _, hm = _small_pair()
    clips = [synth.synth_pcm(0), synth.synth_pcm(1)]
    hm.logmel(clips); hm.encode()
    plain = hm.decode_greedy()
    plain_s = hm.decode_sampled(0.4, seed=3, clip0=1, attempt=1, max_new_tokens=6)
    hm.set_prompts(None)
    assert hm.decode_greedy() == plain
    hm.set_prompts([[], []])                      # n_prefix = 0
    assert hm.decode_greedy() == plain
    hm.set_prompts([R.prefix_tokens(tk, 5, b) for b in range(2)])
    prompted = hm.decode_greedy()
    assert prompted != plain
    hm.set_prompts(None)                          # cleared by hand ...
    assert hm.decode_greedy() == plain
    hm.set_prompts([R.prefix_tokens(tk, 5, b) for b in range(2)])
    hm.logmel(clips); hm.encode()                 # ... and by a fresh batch
    assert hm.decode_greedy() == plain
    assert hm.decode_sampled(0.4, seed=3, clip0=1, attempt=1, max_new_tokens=6) == plain_s
    hm.close()


def test_refusals_leave_state_and_outputs_untouched():
    cfg, tk, _, hm = _small_pair(max_batch=3)
    L, h = hm.L, hm._h
    clips = [synth.synth_pcm(0), synth.synth_pcm(1)]
    hm.logmel(clips); hm.encode()
    good = [R.prefix_tokens(tk, 5, b) for b in range(2)]
    hm.set_prompts(good)
    want = hm.decode_greedy()

    def refused(code, arr, n, stride, batch):
        a = np.ascontiguousarray(arr, dtype=np.int32)
        assert L.nh_set_prompts(h, hip._ip(a), n, stride, batch) == code
        assert hm.decode_greedy() == want          # the prefix set before is still the one in force

    refused(NH_ERR_INVALID, good, 5, 5, 3)                                  # batch != the current batch
    refused(NH_ERR_INVALID, good, 5, 5, 1)
    refused(NH_ERR_INVALID, np.zeros((2, 300)), cfg.max_target_positions // 2, 300, 2)   # one past the largest prefix
    refused(NH_ERR_INVALID, good, -1, 5, 2)
    refused(NH_ERR_INVALID, good, 5, 4, 2)                                  # stride < n_prefix
    for bad in (-1, cfg.vocab_size):
        t = np.array(good); t[1, 3] = bad
        refused(NH_ERR_INVALID, t, 5, 5, 2)                                 # a token id outside the vocabulary
    # a decode whose batch is not the one the prefix was set for: rows joined since
    hm.logmel_array_rows(synth.synth_pcm(2)[None, :], 2)
    hm.encode_rows(2, 1)
    toks = np.full((3, cfg.max_target_positions), -7, dtype=np.int32)
    res = (hip.NhDecodeResult * 3)()
    assert L.nh_decode_greedy(h, hip._ip(toks), res, 0) == NH_ERR_STATE and (toks == -7).all()
    # align_decoded after a prompted decode refuses
    hm.logmel(clips); hm.encode()
    hm.align_capture([(0, 0), (1, 1)])
    hm.set_prompts(good)
    assert hm.decode_greedy() == want              # keeping the queries changes no bit
    with pytest.raises(hip.HipError) as e:
        hm.align_decoded()
    assert e.value.code == NH_ERR_STATE
    hm.set_prompts(None)
    hm.decode_greedy()
    hm.align_decoded()                             # an unprompted decode aligns as ever
    hm.align_capture([])
    # a running pool takes no prefix, and pool_begin drops the one that was set
    hm.set_prompts(good)
    hm.pool_begin(1)
    a = np.ascontiguousarray(good[:1], dtype=np.int32)
    assert L.nh_set_prompts(h, hip._ip(a), 5, 5, 1) == NH_ERR_STATE
    hm.logmel(clips); hm.encode()                  # a fresh batch ends the pool
    plain = hm.decode_greedy()
    hm.set_prompts(None)
    assert hm.decode_greedy() == plain and plain != want
    hm.close()


def test_detect_language_ignores_the_prefix():
    name = "test-d256-mel128"
    cfg, tk = common.make_config(name, encoder_layers=1), common.tokens_for(name)
    hm = common.build_hip(cfg, tk, max_batch=2)
    hm.logmel([synth.synth_pcm(0), synth.synth_pcm(1)]); hm.encode()
    langs = [tk.en + i for i in range(tk.n_languages)]
    want = hm.detect_language(langs)
    hm.set_prompts([[tk.no_speech - 1, 500, 600]] * 2)
    got = hm.detect_language(langs)
    assert got[0] == want[0] and np.array_equal(got[1], want[1])
    hm.close()


# ------------------------------------------------------------------------------------------------ the layers above
def test_model_history_conditions_the_next_slice():
    """Two 30 s slices.  Initial prompt + history longer than the room: both slices decode under 223 ids, the second under
    the LAST 222 of (initial + the first slice's text) behind <|startofprev|>."""
    name = "test-d128"
    cfg, tk = config.preset(name), common.tokens_for(name)
    O = _oracle()
    script = [R.FILLER] * 448
    text = [700, 800, 900]
    script[223:228] = [tk.zero_sec] + text + [tk.eot]   # one segment from 0.00: the whole window is consumed
    over = common.scripted_overrides(cfg, tk, script)
    om = common.build_oracle(cfg, tk, overrides=over)
    d = host.Definition(host.ModelType.TinyEn, host.SelectedDevice.Rocm(0))
    model = d.blocking_try_to_model(cfg, tk, tk.en, tk.transcribe, ((n, a.astype(np.float16)) for n, a in synth.synth_weights(cfg, 0, over)))
    sop = tk.no_speech - 1
    initial = [int(t) for t in np.random.default_rng(4).integers(300, 40000, size=230)]
    model.set_startofprev_token(sop)
    model.set_prompt_tokens(initial)
    model.set_condition_on_previous(True)
    model.set_temperature_fallback(False)
    hist = R.PromptHistory(sop, cfg.max_target_positions, initial, True)
    assert model.prompt_prefix() == hist.prefix() and len(hist.prefix()) == 223
    pcm = np.concatenate([synth.synth_pcm(3), synth.synth_pcm(4)])   # 60 s: two full slices, each consumed whole
    filt = assets_io.mel_filters(cfg.num_mel_bins)
    assert model.transcribe(pcm[:480000].copy(), final_chunk=False) == [text] and model.buffered_samples == 0
    hist.accept(text)
    p2 = hist.prefix()
    assert model.prompt_prefix() == p2 and p2[-3:] == text and p2[1:-3] == initial[-219:]
    assert model.transcribe(pcm[480000:].copy(), final_chunk=False) == [text] and model.buffered_samples == 0
    want = R.prompted_decode(om, om.encoder_forward(O.pcm_to_mel(pcm[480000:], filt)[:, :3000]), p2)
    assert want["tokens"][3:] == [tk.zero_sec] + text + [tk.eot]
    last = model.last_result()
    assert last["n_tokens"] == len(want["tokens"]) and abs(last["avg_logprob"] - want["avg_logprob"]) <= 1e-3
    hist.accept(text)
    assert model.prompt_prefix() == hist.prefix()
    model.transcribe(np.zeros(0, np.float32), final_chunk=True)   # the history goes where the language state goes
    hist.final_chunk()
    assert model.prompt_prefix() == hist.prefix() == [sop] + initial[-222:]
    model.close(); om.close()


def test_model_without_prompt_settings_is_todays_model():
    name = "test-d128"
    cfg, tk = config.preset(name), common.tokens_for(name)
    script = common.transcript_script(tk, n_segments=3, words_per_segment=4)
    over = common.scripted_overrides(cfg, tk, script)
    om = common.build_oracle(cfg, tk, overrides=over)
    d = host.Definition(host.ModelType.TinyEn, host.SelectedDevice.Rocm(0))
    weights = lambda: ((n, a.astype(np.float16)) for n, a in synth.synth_weights(cfg, 0, over))
    model = d.blocking_try_to_model(cfg, tk, tk.en, tk.transcribe, weights())
    model.set_startofprev_token(tk.no_speech - 1)
    model.set_condition_on_previous(True)
    model.set_condition_on_previous(False)            # off again: no prefix, whatever was decoded before
    pcm = synth.synth_pcm(0)
    ref, _, info = om.transcribe(pcm, assets_io.mel_filters(cfg.num_mel_bins), final_chunk=True)
    assert model.transcribe(pcm, final_chunk=True) == ref and len(ref) == 3 and model.prompt_prefix() == []
    assert abs(model.last_result()["avg_logprob"] - info["avg_logprob"]) < 5e-3
    model.close(); om.close()


def test_longform_prompt_is_set_for_every_group():
    cfg, tk, _, hm = _small_pair(max_batch=2)
    rec = np.concatenate([synth.synth_pcm(k) for k in range(3)])   # 90 s: three chunks, two groups
    ids = R.prefix_tokens(tk, 5)
    got = longform.transcribe_recording(hm, rec, prompt=ids)
    starts, lens = hm.cut_plan(rec)
    assert len(got) == len(starts) >= 3
    for i in range(len(starts)):
        hm.logmel_chunks_rows(rec, starts[i:i + 1], lens[i:i + 1], 0)
        hm.encode()
        hm.set_prompts([ids])
        want = hm.decode_greedy()[0]
        assert {k: got[i][k] for k in want} == want, i
        assert want["tokens"][3] == R.long_script(tk)[5]
    assert [r["tokens"] for r in longform.transcribe_recording(hm, rec)] != [r["tokens"] for r in got]
    sp = longform.transcribe_speech(hm, rec, prompt=ids)
    assert len(sp) >= 1 and all(r["tokens"][3] == R.long_script(tk)[5] for r in sp)
    with pytest.raises(ValueError):
        longform.transcribe_recording(hm, rec, align=True, prompt=ids)
    hm.close()
