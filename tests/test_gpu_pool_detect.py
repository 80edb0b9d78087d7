"""GPU: language detection inside the decode pool -- NH_LANG_DETECT, nh_pool_detect_languages, nh_pool_languages and
norma_amd/pool.py with detect_languages=...

Model::detect_language (src/models/whisper/model.rs:194-210) is one decoder forward on [[sot]] and a softmax over the
language-token logits; a pooled row's first step is that forward, so the row detects there and writes the token into its own
prompt before the step that reads it.  The reference of every case is this project's own lockstep path on a context with
private rows -- logmel -> encode -> detect_language(langs) -> decode_greedy -- and every comparison is == (the probabilities
as uint32 bit patterns): the pool runs the same step kernels, and the softmax is one device function for both paths.  Only
the last-but-one case compares against the CPU oracle, with the bar of tests/test_gpu_multilingual.py.

The fixture lets the AUDIO decide the language, so that a row mix-up shows: position 0 steers towards four candidate
languages equally and the last decoder layer's cross-attention votes among them with what it read out of the clip's
encoder output (the construction of tests/common.py:audio_overrides, here with three vote directions at position 0)."""
import numpy as np
import pytest

import common
from norma_amd import assets_io, config, pool, synth
from test_gpu_pool import _same

pytestmark = pytest.mark.gpu

NAME = "test-d256-mel128"     # V2 vocabulary: 51866 tokens, 99 language tokens tk.en + i; two decoder layers, d = 256
N = 10                        # clips synth.synth_pcm(0 .. 9)
MAXNEW = 24                   # generated tokens per clip (the script is longer): every row runs 26 steps and shares steps at many positions
CAND = (7, 42, 13, 90)        # candidate languages tk.en + ...
POS_RMS, PEAK, VOTE = 4.0, 14.0, 4.0
INVALID, STATE = 1, 3         # NH_ERR_INVALID, NH_ERR_STATE


def _hip():
    from norma_amd import hip
    return hip


def _lang_tokens(tk):
    return [tk.en + i for i in range(99)]   # Language::iter() order == vocabulary order for the 99 reference languages


def _f16(a):
    return np.asarray(a).astype(np.float16).astype(np.float32)


def detect_overrides(cfg, tk, att_ref, gamma, no_speech=0.0, seed=0):
    """Weights whose position-0 language logits are decided by the audio.  att_ref [d], gamma: from detect_calibrate (0 and
    zeros: the vote is off, the encoder is already the fixture's).  no_speech > 0: position 0 also carries the no-speech
    token, no_speech times as strongly as one candidate language.  From position 2 on the table steers along a well-formed
    transcript (synth.script_positions' construction): with the plain seed-0 rows the greedy decode runs into steps where every
    candidate is masked, and avg_logprob is NaN, which == cannot compare."""
    d = cfg.d_model
    emb = synth.synth_tensor_by_name(cfg, "model.decoder.embed_tokens.weight", seed)
    scale = max(1.0, PEAK / (d * 0.02))
    emb = _f16(emb * np.float32(scale))                              # as common.scripted_overrides scales it
    gain = POS_RMS / (0.02 * scale)
    cand = [tk.en + o for o in CAND]
    pos = synth.synth_tensor_by_name(cfg, "model.decoder.embed_positions.weight", seed).copy()
    pos[0] += np.float32(gain / 2) * emb[cand].sum(0)
    if no_speech:
        pos[0] += np.float32(no_speech * gain / 2) * emb[tk.no_speech]
    for i, t in enumerate(common.transcript_script(tk, n_segments=4, words_per_segment=6, seed=5)):
        pos[2 + i] += np.float32(gain) * emb[t]
    over = {"model.decoder.embed_tokens.weight": emb, "model.decoder.embed_positions.weight": _f16(pos)}
    for n in ("model.encoder.conv1.weight", "model.encoder.conv2.weight"):
        over[n] = _f16(synth.synth_tensor_by_name(cfg, n, seed) * np.float32(10.0))
    last = f"model.decoder.layers.{cfg.decoder_layers - 1}.encoder_attn.out_proj"
    w0 = synth.synth_tensor_by_name(cfg, last + ".weight", seed).astype(np.float64)
    bo = synth.synth_tensor_by_name(cfg, last + ".bias", seed).astype(np.float64)
    E = emb[cand].astype(np.float64)
    es = [E[0] - E[1], E[2] - E[3], E[0] + E[1] - E[2] - E[3]]
    wo = w0.copy()
    for j, e in enumerate(es):
        wo += gamma * np.outer(e / np.linalg.norm(e), common.audio_pair_direction(100 + j, d).astype(np.float64))
    wo16 = _f16(wo)
    over[last + ".weight"] = wo16
    over[last + ".bias"] = _f16(bo - (wo16.astype(np.float64) - w0) @ np.asarray(att_ref, dtype=np.float64))   # cancels the response to att_ref
    return over


def detect_calibrate(cfg, tk, means):
    """(att_ref, gamma) from the clips' mean encoder outputs, as common.audio_calibrate does it: gamma = VOTE * POS_RMS /
    (|E[c0] - E[c1]| * s_rms)"""
    spec = dict(peak_logit=PEAK, pos_rms=POS_RMS, pairs=[[tk.en + CAND[0], tk.en + CAND[1], 100]])
    common.audio_calibrate(cfg, means, spec, vote=VOTE)
    return np.asarray(spec["att_ref"], dtype=np.float64), spec["gamma"]


class _Fixture:
    pass


@pytest.fixture(scope="module")
def fx():
    """the model, the lockstep reference of the ten clips (computed once, never modified) and the overrides it was built from"""
    fx = _Fixture()
    fx.cfg, fx.tk = config.preset(NAME), common.tokens_for(NAME)
    fx.langs = _lang_tokens(fx.tk)
    zeros = np.zeros(fx.cfg.d_model)
    hm = common.build_hip(fx.cfg, fx.tk, overrides=detect_overrides(fx.cfg, fx.tk, zeros, 0.0), max_batch=N, lang=-1)
    fx.clips = np.stack([synth.synth_pcm(k) for k in range(N)])
    hm.logmel_array(fx.clips); hm.encode()
    means = [hm.encoder_output(b, S=1500).mean(0, keepdims=True) for b in range(N)]   # calibrated on the HIP encoder's outputs
    fx.att_ref, fx.gamma = detect_calibrate(fx.cfg, fx.tk, means)
    fx.over = detect_overrides(fx.cfg, fx.tk, fx.att_ref, fx.gamma)
    lastp = f"model.decoder.layers.{fx.cfg.decoder_layers - 1}.encoder_attn.out_proj"
    for leaf in (".weight", ".bias"):
        hm.load_tensor(lastp + leaf, fx.over[lastp + leaf].astype(np.float16))
    fx.hm = hm
    fx.lang, fx.probs = hm.detect_language(fx.langs)
    fx.want = hm.decode_greedy(max_new_tokens=MAXNEW)
    yield fx
    hm.close()


def _pool_ctx(fx, max_batch, graphs=True):
    hip = _hip()
    hp = hip.HipWhisper(fx.cfg, device=0, max_batch=max_batch, share_with=fx.hm)
    hp.set_tokens(fx.tk, -1, fx.tk.transcribe)
    if not graphs:
        hp.set_option(hip.NH_OPT_DECODE_GRAPHS, 0)
    return hp


def _encode_into(hp, clips):
    def encode(first, n, row0, must=True):
        hp.logmel_array_rows(np.ascontiguousarray(clips[first:first + n]), row0)
        hp.encode_rows(row0, n)
    return encode


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_detected(got, want, lang, probs, order=None):
    """pool results `got` (clip order `order`) against the lockstep decode, the detected tokens and the probability bits"""
    order = list(range(len(got))) if order is None else order
    bad = []
    for g, k in zip(got, order):
        ok = (_same(g, want[k]) and g["language"] == lang[k] == g["tokens"][1]
              and np.array_equal(_bits(g["language_probs"]), _bits(probs[k])))
        if not ok:
            bad.append(k)
    assert len(got) == len(order) and not bad, bad


def test_the_audio_decides_the_language_in_the_lockstep_reference(fx):
    """guards the fixture, not the feature: at least 3 distinct languages, no two clips with equal probability vectors"""
    assert len(set(fx.lang)) >= 3, fx.lang
    assert all(t - fx.tk.en in CAND for t in fx.lang), fx.lang
    assert len({_bits(p).tobytes() for p in fx.probs}) == N
    assert [w["tokens"][1] for w in fx.want] == fx.lang and all(w["tokens"][0] == fx.tk.sot and w["tokens"][2] == fx.tk.transcribe for w in fx.want)


@pytest.mark.parametrize("rows,staging,check_every,graphs", [(3, 4, 1, True), (5, 4, 16, True), (3, 4, 1, False)])
def test_pool_detects_bit_for_bit_what_the_lockstep_path_detects(fx, rows, staging, check_every, graphs):
    """check_every = 1: position 0 is a one-step graph; 16: it is the first of an 8-step graph whose second step already
    embeds the detected token; graphs off: the eager launches"""
    hp = _pool_ctx(fx, rows + staging, graphs)
    dp = pool.DecodePool(hp, rows=rows, staging=staging, max_new_tokens=MAXNEW, check_every=check_every, detect_languages=fx.langs)
    got = dp.run(N, _encode_into(hp, fx.clips))
    _check_detected(got, fx.want, fx.lang, fx.probs)
    order = list(reversed(range(N)))                         # a second stream, other clip order: other rows, other neighbours
    got2 = pool.DecodePool(hp, rows=rows, staging=staging, max_new_tokens=MAXNEW, check_every=check_every,
                           detect_languages=fx.langs).run(N, _encode_into(hp, fx.clips[order]))
    _check_detected(got2, fx.want, fx.lang, fx.probs, order)
    hp.close()


def test_staggered_admissions_by_hand(fx):
    """Rows join while others are at positions 5, 13 and later; a row's position 0 is the first step of a one-step graph
    (pool_step(5), pool_step(1)) and of an 8-step graph (pool_step(8), pool_step(16)) whose next step reads the token.
    pool_languages: refused before the row's first step, right one step later while it runs and after pool_collect, refused
    again once the row is refilled."""
    hip = _hip()
    R = 4
    hp = _pool_ctx(fx, R + N)
    hp.pool_begin(R, MAXNEW, True)
    hp.pool_detect_languages(fx.langs)
    _encode_into(hp, fx.clips)(0, N, R)
    owner, results = {}, {}

    def admit(c, r):
        hp.pool_admit(R + c, r, hip.NH_LANG_DETECT)
        owner[r] = c

    def refused(rows):
        with pytest.raises(hip.HipError) as e:
            hp.pool_languages(rows)
        assert e.value.code == STATE, str(e.value)

    def languages_ok(rows):
        toks, probs = hp.pool_languages(rows)
        for i, r in enumerate(rows):
            assert toks[i] == fx.lang[owner[r]] and np.array_equal(_bits(probs[i]), _bits(fx.probs[owner[r]])), (r, owner[r])
        assert hp.pool_languages(rows, want_probs=False) == (toks, None)

    def collect(flags):
        fin = [r for r in sorted(owner) if flags[r] in (1, 2)]
        if fin:
            for r, res in zip(fin, hp.pool_collect(fin)):
                results[owner[r]] = res
            languages_ok(fin)                                # after pool_collect it still answers
            for r in fin:
                del owner[r]
        return fin

    admit(0, 0)
    refused([0])
    flags = hp.pool_step(5)
    assert flags[0] == 0
    languages_ok([0])                                        # while the row is still running
    admit(1, 1)
    refused([0, 1])                                          # one row of the list has not stepped
    flags = hp.pool_step(8)                                  # clip 1 at position 0 beside clip 0 at position 5
    assert flags[:2].tolist() == [0, 0]
    languages_ok([0, 1])
    admit(2, 2); admit(3, 3)
    refused([2]); refused([3])
    flags = hp.pool_step(16)                                 # clips 2, 3 at position 0 beside positions 13 and 8
    assert flags[2] == 0 and flags[3] == 0
    languages_ok([1, 2, 3])
    assert collect(flags) == [0]                             # clip 0 has had 29 steps: finished
    owner_was = dict(owner)
    admit(4, 0)                                              # refilled
    refused([0])
    flags = hp.pool_step(1)                                  # one step later
    assert flags[0] == 0
    languages_ok([0])
    assert owner == {**owner_was, 0: 4}
    nxt = 5
    for _ in range(200):
        collect(flags)
        for r in range(R):
            if r not in owner and nxt < N:
                admit(nxt, r); nxt += 1
        if not owner:
            break
        flags = hp.pool_step(8)
    assert sorted(results) == list(range(N))
    bad = [c for c in range(N) if not (_same(results[c], fx.want[c]) and results[c]["tokens"][1] == fx.lang[c])]
    assert not bad, bad
    hp.close()


def test_given_and_detected_languages_in_one_pool(fx):
    tk = fx.tk
    # every other clip is given a language that detection would NOT pick
    given = [None if c % 2 == 0 else tk.en + (fx.lang[c] - tk.en + 5) % 99 for c in range(N)]
    mix = [fx.lang[c] if given[c] is None else given[c] for c in range(N)]
    assert all(given[c] != fx.lang[c] for c in range(N))
    fx.hm.set_languages(mix)
    want = fx.hm.decode_greedy(max_new_tokens=MAXNEW)
    assert [w["tokens"][1] for w in want] == mix
    hp = _pool_ctx(fx, 4 + 3)
    got = pool.DecodePool(hp, rows=4, staging=3, max_new_tokens=MAXNEW, check_every=8, detect_languages=fx.langs).run(
        N, _encode_into(hp, fx.clips), langs=given)
    bad = [c for c in range(N) if not (_same(got[c], want[c]) and got[c]["language"] == mix[c])]
    assert not bad, bad
    for c in range(N):
        if given[c] is None:
            assert np.array_equal(_bits(got[c]["language_probs"]), _bits(fx.probs[c])), c
        else:
            assert "language_probs" not in got[c]
    hp.close()


def test_fed_pool_detects_without_the_encoder_contexts_detecting(fx):
    hip = _hip()
    rows, batch = 6, 4
    hp = _pool_ctx(fx, rows + 1)
    encs = [_pool_ctx(fx, batch) for _ in range(2)]
    detect_calls = []
    for h in encs:                                           # an encoder context that detected would show here
        h.detect_language = lambda *a, **k: detect_calls.append(1)

    def encode(i, first, n):
        encs[i].logmel_array(np.ascontiguousarray(fx.clips[first:first + n])); encs[i].encode()
    fp = pool.FedDecodePool(hp, encs, rows=rows, batch=batch, max_new_tokens=MAXNEW, check_every=3, detect_languages=fx.langs)
    got = fp.run(N, encode)
    _check_detected(got, fx.want, fx.lang, fx.probs)
    assert not detect_calls and fp.encodes == -(-N // batch)
    hp.close()
    for h in encs:
        h.close()
    assert hip.NH_LANG_DETECT == -2


@pytest.mark.parametrize("n", [1, 64, 65, 99, 256])
def test_table_sizes_at_the_lane_boundaries(fx, n):
    """the softmax is one 64-lane wave with 4 entries per lane: n = 64 fills one entry of every lane, 65 starts the second,
    256 fills all; token ids spread over the whole vocabulary.  Token and probabilities == nh_detect_language, same table."""
    hip = _hip()
    V = fx.cfg.vocab_size
    table = [int((i * (V // n) + 17) % V) for i in range(n)]
    assert len(set(table)) == n and (n == 1 or max(table) >= V - 2 * (V // n))   # distinct ids, up to the end of the vocabulary
    ref_lang, ref_probs = fx.hm.detect_language(table)
    K, R = 4, 5
    hp = _pool_ctx(fx, R + K)
    hp.pool_begin(R, MAXNEW, True)
    hp.pool_detect_languages(table)
    _encode_into(hp, fx.clips)(0, K, R)
    for c in range(K):
        hp.pool_admit(R + c, c + 1, hip.NH_LANG_DETECT)      # rows 1 .. 4: row != clip
    hp.pool_step(1)
    toks, probs = hp.pool_languages(list(range(1, K + 1)))
    assert toks == ref_lang[:K]
    assert probs.shape == (K, n) and np.array_equal(_bits(probs), _bits(ref_probs[:K]))
    assert all(t in table for t in toks)
    hp.close()


def test_a_row_that_the_no_speech_probe_ends_has_a_language_too(fx):
    """position 0 also carries the no-speech token: p > 0.6, the row finishes with flag 2 in its first step -- and was detected
    in that step, as the reference detects before it decodes"""
    tk = fx.tk
    over = detect_overrides(fx.cfg, tk, fx.att_ref, fx.gamma, no_speech=4.0)
    hm = common.build_hip(fx.cfg, tk, overrides=over, max_batch=N, lang=-1)
    hm.logmel_array(fx.clips); hm.encode()
    lang, probs = hm.detect_language(fx.langs)
    want = hm.decode_greedy(max_new_tokens=MAXNEW)
    assert all(w["no_speech_exit"] and w["no_speech_prob"] > 0.6 and w["tokens"] == [tk.sot, lang[c], tk.transcribe] for c, w in enumerate(want))
    assert len(set(lang)) >= 2, lang
    hip = _hip()
    hp = hip.HipWhisper(fx.cfg, device=0, max_batch=3 + 4, share_with=hm)
    hp.set_tokens(tk, -1, tk.transcribe)
    hp.pool_begin(3, MAXNEW, True)
    hp.pool_detect_languages(fx.langs)
    _encode_into(hp, fx.clips)(0, 4, 3)
    hp.pool_admit(3, 0, hip.NH_LANG_DETECT)
    assert hp.pool_step(1).tolist() == [2, 3, 3]             # ended by the probe in its first step
    got = pool.DecodePool(hp, rows=3, staging=4, max_new_tokens=MAXNEW, check_every=2, detect_languages=fx.langs).run(
        N, _encode_into(hp, fx.clips))
    _check_detected(got, want, lang, probs)
    hm.close(); hp.close()


def test_fallback_keeps_the_language_of_the_greedy_attempt(fx):
    """DecodePool(fallback=True, detect_languages=...) against model.rs:175-190 evaluated on lockstep decodes after
    nh_detect_language: nh_decode_greedy, then nh_decode_sampled at 0.2 .. 1.0 (the construction of
    tests/test_gpu_pool_fallback.py).  A retried clip's prompt keeps the token its t = 0 attempt detected."""
    from test_gpu_pool_fallback import _assert_fallback_results, _median_threshold, _policy
    seed, clip0, T = 0xD37EC7, 500, pool.TEMPERATURES
    lang, _ = fx.hm.detect_language(fx.langs)                # the prompts of the lockstep attempts
    assert lang == fx.lang
    attempts = [fx.hm.decode_greedy(max_new_tokens=MAXNEW)] + [fx.hm.decode_sampled(T[a], seed, clip0, a, max_new_tokens=MAXNEW)
                                                             for a in range(1, len(T))]
    assert all(_same(a, w) for a, w in zip(attempts[0], fx.want))
    thr = _median_threshold(attempts[0])
    want = _policy(attempts, T, thr)
    hp = _pool_ctx(fx, 4 + 3)
    dp = pool.DecodePool(hp, rows=4, staging=3, max_new_tokens=MAXNEW, check_every=8, fallback=True, seed=seed, clip0=clip0,
                         logprob_threshold=thr, detect_languages=fx.langs)
    got = dp.run(N, _encode_into(hp, fx.clips))
    _assert_fallback_results(got, want)
    retried = [c for c in range(N) if want[c]["attempt"] > 0]
    assert retried and dp.retries == sum(w["attempt"] for w in want)
    for c in range(N):
        assert got[c]["tokens"][1] == got[c]["language"] == fx.lang[c], c
        assert np.array_equal(_bits(got[c]["language_probs"]), _bits(fx.probs[c])), c
    hp.close()


def test_pool_detection_against_the_oracle(fx):
    from oracle import oracle as O
    K = 4
    om = common.build_oracle(fx.cfg, fx.tk, overrides=fx.over, lang=-1)
    filt = assets_io.mel_filters(fx.cfg.num_mel_bins)
    hp = _pool_ctx(fx, 2 + K)
    got = pool.DecodePool(hp, rows=2, staging=K, max_new_tokens=4, check_every=4, detect_languages=fx.langs).run(
        K, _encode_into(hp, fx.clips))
    for c in range(K):
        xa = om.encoder_forward(O.pcm_to_mel(fx.clips[c], filt)[:, :3000])
        ref, rp = om.detect_language(xa, fx.langs)
        assert got[c]["language"] == ref, (c, got[c]["language"], ref)
        assert np.abs(got[c]["language_probs"] - rp).max() <= 2e-3 * rp.max() + 1e-6, c
    om.close(); hp.close()


def test_refusals_leave_the_pool_usable(fx):
    hip = _hip()
    tk, R, DET = fx.tk, 3, hip.NH_LANG_DETECT
    hp = _pool_ctx(fx, R + 4)

    def refused(code, fn, *args):
        with pytest.raises(hip.HipError) as e:
            fn(*args)
        assert e.value.code == code, str(e.value)

    refused(STATE, hp.pool_detect_languages, fx.langs)                   # no pool
    refused(STATE, hp.pool_languages, [0])
    hp.pool_begin(R, MAXNEW, False)
    _encode_into(hp, fx.clips)(0, 4, R)
    refused(INVALID, hp.pool_detect_languages, fx.langs)                 # pool begun without per-clip languages
    refused(INVALID, hp.pool_admit, R + 0, 0, DET)
    hp.pool_begin(R, MAXNEW, True)
    _encode_into(hp, fx.clips)(0, 4, R)
    refused(STATE, hp.pool_admit, R + 0, 0, DET)                         # no table yet
    refused(INVALID, hp.pool_detect_languages, [])                       # n out of range
    refused(INVALID, hp.pool_detect_languages, [tk.en] * 257)
    refused(INVALID, hp.pool_detect_languages, [tk.en, fx.cfg.vocab_size])   # a token id outside the vocabulary
    refused(INVALID, hp.pool_detect_languages, [-1, tk.en])
    refused(STATE, hp.pool_admit, R + 0, 0, DET)                         # the refused tables did not become the table
    hp.pool_detect_languages(fx.langs)
    refused(INVALID, hp.pool_languages, [R])                             # row outside the pool
    refused(INVALID, hp.pool_languages, [-1])
    refused(STATE, hp.pool_languages, [0])                               # never admitted
    hp.pool_admit(R + 0, 0, DET)
    refused(STATE, hp.pool_detect_languages, fx.langs)                   # a row is busy
    refused(STATE, hp.pool_languages, [0])                               # admitted, not stepped
    given = tk.en + (fx.lang[1] - tk.en + 5) % 99
    hp.pool_admit(R + 1, 1, given)
    refused(STATE, hp.detect_language, fx.langs)                         # the lockstep probe stays refused on a pooled context
    hp.pool_step(2)
    refused(STATE, hp.pool_languages, [1])                               # stepped, but its language was given
    refused(STATE, hp.pool_languages, [0, 2])
    refused(STATE, hp.pool_detect_languages, fx.langs[:5])
    assert hp.pool_languages([0], want_probs=False)[0] == [fx.lang[0]]
    for _ in range(100):
        flags = hp.pool_step(8)
        if all(flags[r] in (1, 2) for r in (0, 1)):
            break
    got = hp.pool_collect([0, 1])
    fx.hm.set_languages([fx.lang[0], given] + fx.lang[2:])
    want1 = fx.hm.decode_greedy(max_new_tokens=MAXNEW)[1]
    assert _same(got[0], fx.want[0]) and _same(got[1], want1) and got[1]["tokens"][1] == given
    # a new table once no row is busy: the step graphs are captured again for its size, rows detected under the old one are forgotten
    sub = fx.langs[:50]
    ref_lang, ref_probs = fx.hm.detect_language(sub)
    hp.pool_detect_languages(sub)
    refused(STATE, hp.pool_languages, [0])
    hp.pool_admit(R + 2, 2, DET)
    hp.pool_step(8)
    toks, probs = hp.pool_languages([2])
    assert toks == [ref_lang[2]] and np.array_equal(_bits(probs[0]), _bits(ref_probs[2]))
    hp.pool_begin(R, MAXNEW, True)                                       # nh_pool_begin clears the table
    _encode_into(hp, fx.clips)(0, 1, R)
    refused(STATE, hp.pool_admit, R + 0, 0, DET)
    hp.close()
