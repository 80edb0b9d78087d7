"""GPU: beam search (nh_decode_beam).

References: tests/beam_ref.py -- step_ref for the selection / merge view (decided steps exact on tokens, parents, state and
finished records, scores within the bound the reference derives from the kernel's f32 arithmetic), search_ref driven by the
CPU oracle for whole decodes (tokens identical: tests/test_beam_cpu.py asserts the fixtures' cut gaps at ten times the measured
device error; avg_logprob within 5e-3, the bar of the greedy parity tests).
K = 1 against nh_decode_greedy: tokens, n_tokens, no_speech_exit and the no_speech_prob bits identical; avg_logprob within 1e-5
-- that bar, not bit equality, applies: the selection kernel sums the softmax in another order than logit_step_kernel."""
import functools

import numpy as np
import pytest

import beam_fixture as F
import beam_ref
import common
from norma_amd import assets_io, hip, host, synth

pytestmark = pytest.mark.gpu

NH_ERR_INVALID, NH_ERR_STATE = 1, 3
NAME = "test-d128"


def _oracle():
    from oracle import oracle as O
    return O


def _clips(n=3):
    return F.clips(n)      # three clips of different lengths


# ---------------------------------------------------------------------------------------------- selection + merge view
def _sup_array(cfg, tk):
    sup = np.zeros(cfg.vocab_size, dtype=bool)
    sup[np.asarray(cfg.suppress_tokens, dtype=np.int64)] = True
    sup[tk.no_timestamps] = True
    return sup


NEAR_TIE = 2047 + 300     # this token and the next one carry logits one ulp apart in every row of _view_case


def _view_case(cfg, tk, K, B, seed, max_new, prompt_len=3):
    """Rows in every rule state: first token, after two timestamps, after text + timestamp, after text with the timestamp mass
    above and below the best text, dead rows, a row at cap - 1 and one at max_new_tokens - 1.  Near-ties and exact ties sit on
    the boundaries of the sweep (thread t owns tokens t, t + 1024, ..; waves are 64 threads): neighbours across a wave, the
    same thread's consecutive tokens, the last tokens of the row."""
    rng = np.random.default_rng(seed)
    V, Cn, NT, Z = cfg.vocab_size, cfg.max_target_positions, tk.no_timestamps, tk.zero_sec
    R = K * B
    toks = np.zeros((R, Cn), dtype=np.int32)
    nt, hl, lt, live = (np.zeros(R, dtype=np.int32) for _ in range(4))
    score = -rng.uniform(0.0, 3.0, R)
    lg = (1.5 * rng.standard_normal((R, V))).astype(np.float32)
    text = lambda: int(rng.integers(300, 40000))
    for r in range(R):
        kind = (r + seed) % 8
        seq = [tk.sot, tk.en, tk.transcribe]
        live[r] = 1
        if kind == 0:
            pass                                                       # first generated token: the window
        elif kind == 1:
            seq += [Z, text(), Z + 30, Z + 34]; hl[r], lt[r] = 1, Z + 34   # two timestamps: text only
        elif kind == 2:
            seq += [Z, text(), Z + 50]; hl[r], lt[r] = 1, Z + 50          # text + timestamp: timestamps only
        elif kind == 3:
            seq += [Z, text(), text()]; hl[r], lt[r] = 1, Z              # text, loud timestamps: sum_ts >= max_text
            lg[r, Z + 10:Z + 200] += 6.0
        elif kind == 4:
            seq += [Z, text(), text()]; hl[r], lt[r] = 1, Z              # text, a loud text token: past timestamps only
            lg[r, [text(), text(), tk.eot]] += [14.0, 13.0, 13.5]
            lg[r, Z - 5:Z + 1] += 12.0                                   # timestamps <= last_ts stay masked
        elif kind == 5:
            live[r] = 0                                                  # dead
            seq += [Z, text()]; hl[r], lt[r] = 1, Z
        elif kind == 6:
            seq += [Z] + [text() for _ in range(Cn - 2 - 4)]; hl[r], lt[r] = 1, Z   # cap - 1 tokens: the next one is the last
            lg[r, text()] += 14.0
        else:
            seq += [Z] + [text() for _ in range(max_new - 2)]; hl[r], lt[r] = 1, Z   # max_new_tokens - 1 generated
            lg[r, text()] += 14.0
        # ties on the sweep's boundaries, among tokens the row's rule allows (where it allows them)
        for a, c in ((63, 64), (1023 + 300, 1024 + 300), (V - 2, V - 1), (NT + 70, NT + 70 + 1024 - 1)):
            v = np.float32(lg[r].max() + 1.0)
            lg[r, a], lg[r, c] = v, v
        a = NEAR_TIE
        lg[r, a] = lg[r].max() + np.float32(0.5); lg[r, a + 1] = np.nextafter(lg[r, a], np.float32(0))   # one ulp apart
        nt[r] = len(seq)
        toks[r, :len(seq)] = seq
    return lg, dict(tokens=toks, n_tokens=nt, have_last=hl, last_ts=lt, live=live, score=score)


@functools.lru_cache(maxsize=None)
def _view_ctx(name):
    cfg, tk = common.make_config(name), common.tokens_for(name)
    hm = hip.HipWhisper(cfg, device=0, max_batch=16)
    hm.set_tokens(tk, tk.en, tk.transcribe)
    return cfg, tk, hm


@pytest.mark.parametrize("name", [NAME, "test-d256-mel128"])   # V = 51864 (EnV1) and 51866 (V2)
@pytest.mark.parametrize("K,B", [(1, 1), (2, 3), (5, 3), (8, 2)])
def test_selection_view_matches_the_step_reference(name, K, B):
    cfg, tk, hm = _view_ctx(name)
    sup, Cn, max_new = _sup_array(cfg, tk), cfg.max_target_positions, 40
    compared = exact_ties = near_pairs = 0
    for seed in range(3):
        lg, st = _view_case(cfg, tk, K, B, seed, max_new)
        nf_in = [(b + seed) % K for b in range(B)]    # some clips hold finished hypotheses already; a full list cannot occur (the clip is done)
        ref = beam_ref.step_ref(lg, st, K, B, nf_in, sup, tk, Cn - 1, max_new=max_new, prompt_len=3)
        got = hm.beam_step(K, B, lg, st, nf_in, max_new_tokens=max_new, prompt_len=3)
        for b in range(B):
            rows = [j * B + b for j in range(K)]
            for r in rows:
                if not st["live"][r] and not got["live"][r]:     # dead rows come back bit-identical
                    assert np.array_equal(got["tokens"][r], st["tokens"][r]) and got["n_tokens"][r] == st["n_tokens"][r]
                    assert got["have_last"][r] == st["have_last"][r] and got["last_ts"][r] == st["last_ts"][r]
                    assert got["score"][r] == st["score"][r]
            if not ref["decided"][b]:
                continue
            compared += 1
            exact_ties += ref["exact_ties"][b] > 0
            kids = {(int(ref["parent"][r]), int(ref["tokens"][r, ref["n_tokens"][r] - 1])) for r in rows if ref["live"][r]}
            near_pairs += any((p, NEAR_TIE) in kids and (p, NEAR_TIE + 1) in kids for p, _ in kids)
            for r in rows:
                assert got["live"][r] == ref["live"][r], (seed, b, r)
                assert got["parent"][r] == ref["parent"][r], (seed, b, r)
                if not ref["live"][r]:
                    continue
                n = ref["n_tokens"][r]
                assert got["n_tokens"][r] == n and np.array_equal(got["tokens"][r, :n], ref["tokens"][r, :n]), (seed, b, r)
                assert got["have_last"][r] == ref["have_last"][r] and got["last_ts"][r] == ref["last_ts"][r], (seed, b, r)
                assert abs(got["score"][r] - ref["score"][r]) <= ref["score_bound"], (seed, b, r, got["score"][r], ref["score"][r])
            assert got["n_finished"][b] == ref["n_finished"][b], (seed, b)
            assert [t for t, _ in got["finished"][b]] == [t for t, _ in ref["finished"][b]], (seed, b)
            for (_, s), (_, s2) in zip(got["finished"][b], ref["finished"][b]):
                assert abs(s - s2) <= ref["score_bound"]
    # The reference decides every clip of these cases (its verdict depends on the inputs alone, not on the device), so every
    # clip is compared; in each case some compared clip had equal candidates of one row inside the walked list and, at K > 1,
    # some compared clip took both tokens of one row's one-ulp pair as children.
    assert compared == 3 * B, compared
    assert exact_ties >= 1, exact_ties
    assert near_pairs >= (1 if K > 1 else 0), near_pairs


def test_selection_view_all_masked_row_ends_the_clip():
    cfg, tk, hm = _view_ctx(NAME)
    V, Cn = cfg.vocab_size, cfg.max_target_positions
    toks = np.zeros((2, Cn), dtype=np.int32)
    seq = [tk.sot, tk.en, tk.transcribe, tk.zero_sec, 500, V - 1]      # text + the last timestamp: nothing later is left
    toks[0, :len(seq)] = seq
    st = dict(tokens=toks, n_tokens=[len(seq), 0], have_last=[1, 0], last_ts=[V - 1, 0], live=[1, 0], score=[-2.0, 0.0])
    lg = np.random.default_rng(0).standard_normal((2, V)).astype(np.float32)
    got = hm.beam_step(2, 1, lg, st, [0])
    assert got["live"].tolist() == [0, 0] and got["n_finished"].tolist() == [0] and got["parent"].tolist() == [-1, -1]
    ft, fn, fs = got["fin_raw"]
    assert ft[0, 0, :fn[0, 0]].tolist() == seq + [V - 1] and fs[0, 0] == -np.inf     # the greedy step's all-masked convention


def test_merge_moves_hypothesis_state_under_a_cycle_and_a_chain():
    """Scores chosen so that the parent map of clip 0 is the 3-cycle 0 <- 1 <- 2 <- 0 (beam 3 stays) and that of clip 1 the
    chain 0 <- 1 <- 2 <- 3 with beam 3 feeding two rows.  Every row holds a history of its own length and its own last
    timestamp, and one text token far above the rest (q within 1e-6 of 1), so a child's score is its parent's and the
    ranking is the parents': token history, n_tokens, have_last and last_ts must arrive with the hypothesis."""
    cfg, tk, hm = _view_ctx(NAME)
    sup, V, Cn, Z = _sup_array(cfg, tk), cfg.vocab_size, cfg.max_target_positions, tk.zero_sec
    K, B = 4, 2
    R = K * B
    free = [v for v in range(300, 600) if not sup[v]][:64]
    lg = np.random.default_rng(7).standard_normal((R, V)).astype(np.float32)
    toks = np.zeros((R, Cn), dtype=np.int32)
    nt, lt = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
    score = np.zeros(R)
    by_clip = {0: [-3.0, -1.0, -2.0, -4.0], 1: [-9.0, -1.0, -2.0, -3.0]}
    loud = {}
    for j in range(K):
        for b in range(B):
            r = j * B + b
            seq = [tk.sot, tk.en, tk.transcribe, Z] + [free[(3 * r + i) % 64] for i in range(1 + r)] + [Z + 10 + r, Z + 20 + 2 * r]
            toks[r, :len(seq)], nt[r], lt[r], score[r] = seq, len(seq), seq[-1], by_clip[b][j]    # two timestamps: text only
            loud[r] = free[10 + r]
            lg[r, loud[r]] = 25.0
    lg[3 * B + 1, free[40]] = 25.0        # clip 1, beam 3: two equal tokens, the higher id first
    st = dict(tokens=toks, n_tokens=nt, have_last=np.ones(R, dtype=np.int32), last_ts=lt, live=np.ones(R, dtype=np.int32), score=score)
    ref = beam_ref.step_ref(lg, st, K, B, [0, 0], sup, tk, Cn - 1)
    got = hm.beam_step(K, B, lg, st, [0, 0])
    row = lambda j, b: j * B + b
    want = {0: [1, 2, 0, 3], 1: [1, 2, 3, 3]}
    last = {0: [loud[row(1, 0)], loud[row(2, 0)], loud[row(0, 0)], loud[row(3, 0)]], 1: [loud[row(1, 1)], loud[row(2, 1)], free[40], loud[row(3, 1)]]}
    assert ref["decided"] == [True, True]
    for b in range(B):
        for j in range(K):
            r, q = row(j, b), row(want[b][j], b)
            assert ref["parent"][r] == q and got["parent"][r] == q, (b, j, got["parent"].tolist())
            n = int(nt[q]) + 1
            assert got["live"][r] == 1 and got["n_tokens"][r] == n
            assert got["tokens"][r, :n].tolist() == toks[q, :n - 1].tolist() + [last[b][j]], (b, j)
            assert got["have_last"][r] == 1 and got["last_ts"][r] == lt[q], (b, j)
            assert abs(got["score"][r] - ref["score"][r]) <= ref["score_bound"]
        assert got["n_finished"][b] == 0


# ---------------------------------------------------------------------------------------------------- cache reorder
@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("layer", (0, 1))
def test_cache_reorder_under_every_kind_of_parent_map(layer, which):
    cfg, tk, hm = _view_ctx(NAME)
    K, B, H, Cn, n_pos = 4, 3, cfg.decoder_attention_heads, cfg.max_target_positions, 13    # 13: no multiple of 8
    R = K * B
    rng = np.random.default_rng(layer * 2 + which)
    row = lambda j, b: j * B + b
    maps = {
        "identity": list(range(R)),
        "swap": [row(1, b) if j == 0 else row(0, b) if j == 1 else row(j, b) for j in range(K) for b in range(B)],
        "cycle3": [row((j + 1) % 3, b) if j < 3 else row(j, b) for j in range(K) for b in range(B)],
        "fanout": [row(2, b) for j in range(K) for b in range(B)],
        # clip 0: chain 0 <- 1 <- 2 <- 3; clip 1: swap + fan-out; clip 2: dead rows and a foreign parent (ignored)
        "mixed": [[row(1, 0), row(2, 0), row(3, 0), row(3, 0)][j] if b == 0 else [row(1, 1), row(0, 1), row(0, 1), row(1, 1)][j] if b == 1
                  else [-1, row(0, 2), row(1, 0), -1][j] for j in range(K) for b in range(B)],
    }
    for kind, parent in maps.items():
        cache = rng.standard_normal((R, H, Cn, 64)).astype(np.float16)
        got = hm.beam_reorder(K, B, parent, n_pos, layer, which, cache)
        want = cache.copy()
        for r in range(R):
            q = parent[r]
            if q >= 0 and q != r and q % B == r % B:
                want[r, :, :n_pos] = cache[q, :, :n_pos]
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), kind


# ------------------------------------------------------------------------------------------------------- end to end
def _fixture(fx, name=NAME, lang=None):
    return _fixture_cached(fx, name, lang)


@functools.lru_cache(maxsize=None)
def _fixture_cached(fx, name, lang, n_clips=3):
    """One oracle and one context (max_batch 16) on the fixture's weights, the clips encoded on the oracle."""
    O = _oracle()
    cfg, tk = common.make_config(name), common.tokens_for(name)
    P = 2 if lang == -1 else 3
    steps = F.FIXTURES[fx](tk)
    over = F.weighted_overrides(cfg, tk, steps, prompt_len=P)
    om, (hm,) = common.build_together(cfg, tk, overrides=over, batches=(16,), lang=lang)
    return cfg, tk, steps, om, hm, _clips(n_clips), F.oracle_encodings(om, cfg, n_clips)


def _reference(fx, K, b, name=NAME, lang=None):
    return _reference_cached(fx, K, b, name, lang)


@functools.lru_cache(maxsize=None)
def _reference_cached(fx, K, b, name, lang):
    cfg, tk, steps, om, hm, clips, xas = _fixture(fx, name, lang)
    prompt = [tk.sot, tk.transcribe] if lang == -1 else [tk.sot, tk.en, tk.transcribe]
    return beam_ref.search_ref(F.oracle_step(om, xas[b]), prompt, K, tk, cfg.max_target_positions - 1, max_new=len(steps))


def _check_against_reference(fx, K, name=NAME, lang=None):
    cfg, tk, steps, om, hm, clips, xas = _fixture(fx, name, lang)
    hm.logmel(clips); hm.encode()
    got = hm.decode_beam(K, max_new_tokens=len(steps))
    worst = 0.0
    for b in range(len(clips)):
        ref = _reference(fx, K, b, name, lang)
        print(fx, K, b, "cut gap", ref["min_gap"], "winner", ref["tokens"])
        assert got[b]["tokens"] == ref["tokens"], (b, got[b]["tokens"], ref["tokens"])
        assert len(got[b]["tokens"]) == ref["n_tokens"]
        assert [t for t, _ in got[b]["hypotheses"]] == [t for t, _ in ref["finished"]], b
        assert abs(got[b]["avg_logprob"] - ref["avg_logprob"]) <= 5e-3, (b, got[b]["avg_logprob"], ref["avg_logprob"])
        for (_, s), (_, s2) in zip(got[b]["hypotheses"], ref["finished"]):
            worst = max(worst, abs(s - s2))
    print(fx, K, "largest |device - reference| cumulative score", worst)
    return got, worst


@pytest.mark.parametrize("K", (1, 2, 4, 5))
@pytest.mark.parametrize("fx", sorted(F.FIXTURES))
def test_beam_decode_matches_the_reference_search(fx, K):
    got, worst = _check_against_reference(fx, K)
    assert worst <= F.G / 2, worst    # two scores off by less than G / 2 each cannot flip a cut whose gap is at least G
    if fx == "fork" and K == 2:
        cfg, tk, steps, om, hm, clips, xas = _fixture(fx)
        greedy = hm.decode_greedy(max_new_tokens=len(steps))
        assert any(g["tokens"] != r["tokens"] for g, r in zip(greedy, got))     # the beam winner is not greedy's


def test_beam_decode_on_d256_mel128():
    _check_against_reference("fork", 2, name="test-d256-mel128")


def test_beam_decode_without_a_language_token():
    _check_against_reference("fork", 2, lang=-1)      # P = 2


# ------------------------------------------------------------------------------------------- against the other decodes
def _strip(results):
    return [{k: v for k, v in r.items() if k != "hypotheses"} for r in results]


@pytest.mark.parametrize("fx", sorted(F.FIXTURES))
def test_k1_equals_greedy(fx):
    cfg, tk, steps, om, hm, clips, xas = _fixture(fx)
    hm.logmel(clips); hm.encode()
    for max_new in (len(steps), 0):          # 0: on past the script to the length cap (forced eot there)
        g = hm.decode_greedy(max_new_tokens=max_new)
        k1 = hm.decode_beam(1, max_new_tokens=max_new)
        for a, c in zip(g, k1):
            assert a["tokens"] == c["tokens"] and a["no_speech_exit"] == c["no_speech_exit"]
            assert a["no_speech_prob"] == c["no_speech_prob"]
            assert abs(a["avg_logprob"] - c["avg_logprob"]) <= 1e-5, (a["avg_logprob"], c["avg_logprob"])


def test_batch_independence():
    cfg, tk, steps, om, hm, clips, xas = _fixture("swap")
    hm.logmel(clips); hm.encode()
    in_batch = hm.decode_beam(4, max_new_tokens=len(steps))[1]
    hm.logmel(clips[1:2]); hm.encode()
    alone = hm.decode_beam(4, max_new_tokens=len(steps))[0]
    assert alone == in_batch       # winner and finished list, tokens and scores: the same bits


def test_side_effect_freedom():
    cfg, tk, steps, om, hm, clips, xas = _fixture("closing")
    hm.logmel(clips); hm.encode()
    n = len(steps)
    g0 = hm.decode_greedy(max_new_tokens=n)
    s0 = hm.decode_sampled(0.6, seed=11, clip0=5, attempt=2, max_new_tokens=n)
    hm.decode_beam(5, max_new_tokens=n)
    assert hm.decode_greedy(max_new_tokens=n) == g0
    hm.decode_beam(4, max_new_tokens=n)
    assert hm.decode_sampled(0.6, seed=11, clip0=5, attempt=2, max_new_tokens=n) == s0
    # kept queries are not reordered with their hypotheses: nh_align_decoded serves a greedy decode and refuses after a beam decode
    hm.align_capture([(0, 0)])
    try:
        hm.decode_greedy(max_new_tokens=n)
        hm.align_decoded()
        hm.decode_beam(2, max_new_tokens=n)
        with pytest.raises(hip.HipError) as e:
            hm.align_decoded()
        assert e.value.code == NH_ERR_STATE
    finally:
        hm.align_capture([])
    assert hm.decode_greedy(max_new_tokens=n) == g0


def test_beam_decode_under_a_prefix():
    """A 4-token prefix (the one-pass prefill) and K = 2 against the reference search on the prefixed prompt."""
    name, NP = NAME, 4
    cfg, tk = common.make_config(name), common.tokens_for(name)
    steps = F.FIXTURES["fork"](tk)
    over = F.weighted_overrides(cfg, tk, steps, n_prefix=NP)
    om, (hm,) = common.build_together(cfg, tk, overrides=over, batches=(16,))
    O = _oracle()
    filt = assets_io.mel_filters(cfg.num_mel_bins)
    clips = _clips(2)
    pre = [[tk.no_speech - 1, 500 + b, 600, 700] for b in range(2)]
    hm.logmel(clips); hm.encode()
    hm.set_prompts(pre)
    got = hm.decode_beam(2, max_new_tokens=len(steps))
    greedy = hm.decode_greedy(max_new_tokens=len(steps))
    for b in range(2):
        xa = om.encoder_forward(O.pcm_to_mel(clips[b], filt)[:, :3000])
        ref = beam_ref.search_ref(F.oracle_step(om, xa), pre[b] + [tk.sot, tk.en, tk.transcribe], 2, tk, cfg.max_target_positions - 1,
                                  max_new=len(steps), n_skip=NP)
        assert got[b]["tokens"] == ref["tokens"] and got[b]["tokens"][0] == tk.sot
        assert [t for t, _ in got[b]["hypotheses"]] == [t for t, _ in ref["finished"]]
        assert abs(got[b]["avg_logprob"] - ref["avg_logprob"]) <= 5e-3
        assert got[b]["tokens"] != greedy[b]["tokens"]
    hm.close(); om.close()


def test_no_speech_exit_of_one_clip():
    """Loud cross-attention and a no-speech pull at position 0 sized so that the probe ends clip 2 alone (oracle: 0.55 / 0.39 /
    0.65): that clip returns what greedy returns, the others search on."""
    cfg, tk = common.make_config(NAME), common.tokens_for(NAME)
    steps = F.FIXTURES["fork"](tk)
    over = F.weighted_overrides(cfg, tk, steps)
    emb, pos = over["model.decoder.embed_tokens.weight"], over["model.decoder.embed_positions.weight"].copy()
    pos[0] += np.float32(3.45) * emb[tk.no_speech]
    over["model.decoder.embed_positions.weight"] = pos.astype(np.float16).astype(np.float32)
    for n in ("model.encoder.conv1.weight", "model.encoder.conv2.weight"):
        over[n] = (synth.synth_tensor_by_name(cfg, n, 0) * np.float32(4)).astype(np.float16).astype(np.float32)
    for l in range(cfg.decoder_layers):
        for w in ("v_proj", "out_proj"):
            key = f"model.decoder.layers.{l}.encoder_attn.{w}.weight"
            over[key] = (synth.synth_tensor_by_name(cfg, key, 0) * np.float32(2)).astype(np.float16).astype(np.float32)
    hm = common.build_hip(cfg, tk, overrides=over, max_batch=16)
    clips = [synth.synth_pcm(0, 480000), np.zeros(200000, np.float32), synth.synth_pcm(2, 300000)]
    hm.logmel(clips); hm.encode()
    g = hm.decode_greedy(max_new_tokens=len(steps))
    k = hm.decode_beam(4, max_new_tokens=len(steps))
    assert [r["no_speech_exit"] for r in g] == [False, False, True]
    assert _strip(k)[2] == g[2] and k[2]["hypotheses"] == []
    k1 = hm.decode_beam(1, max_new_tokens=len(steps))
    for b in range(2):
        assert not k[b]["no_speech_exit"] and len(k[b]["hypotheses"]) == 4 and k[b]["no_speech_prob"] == g[b]["no_speech_prob"]
        assert k1[b]["tokens"] == g[b]["tokens"]
    hm.close()


def test_refusals_leave_outputs_and_the_next_decode_untouched():
    cfg, tk, steps, om, hm, clips, xas = _fixture("fork")
    n = len(steps)
    hm.logmel(clips); hm.encode()
    g0 = hm.decode_greedy(max_new_tokens=n)
    Cn = cfg.max_target_positions

    def refused(code, K=2, fragment=None, null=False):
        toks = np.full((3, Cn), -7, dtype=np.int32)
        res = (hip.NhDecodeResult * 3)()
        rc = hm.L.nh_decode_beam(hm._h, K, None if null else hip._ip(toks), res, n)
        assert rc == code, (rc, code)
        assert (toks == -7).all() and all(res[b].n_tokens == 0 for b in range(3))
        if fragment:
            msg = hm.L.nh_last_error(hm._h).decode()
            assert all(f in msg for f in fragment), msg
        assert hm.decode_greedy(max_new_tokens=n) == g0

    refused(NH_ERR_INVALID, K=0)
    refused(NH_ERR_INVALID, K=9)
    refused(NH_ERR_INVALID, K=6, fragment=("3", "6", "16"))     # 3 clips x 6 beams > max_batch 16: the message names both
    refused(NH_ERR_INVALID, null=True)
    def state_refusal(h, rows, why):
        """NH_ERR_STATE with the outputs untouched, and for the reason meant: the message says which check refused."""
        toks = np.full((rows, Cn), -7, dtype=np.int32)
        res = (hip.NhDecodeResult * rows)()
        assert h.L.nh_decode_beam(h._h, 2, hip._ip(toks), res, n) == NH_ERR_STATE
        assert (toks == -7).all() and all(res[b].n_tokens == 0 for b in range(rows))
        msg = h.L.nh_last_error(h._h).decode()
        assert why in msg, msg

    hm.set_option(3, 1)                                        # NH_OPT_ABSORBED_XATTN
    try:
        state_refusal(hm, 3, "NH_OPT_ABSORBED_XATTN")
    finally:
        hm.set_option(3, 0)
    assert hm.decode_greedy(max_new_tokens=n) == g0
    # a prefix set for another batch
    hm.set_prompts([[tk.no_speech - 1, 500]] * 3)
    hm.logmel_array_rows(np.stack([synth.synth_pcm(3)]), 3); hm.encode_rows(3, 1)
    state_refusal(hm, 4, "prefix was set for another batch")
    # no encoder output / no tokens / a running pool: a fresh context on the same weights, taken through the three states.
    # decode_refusals looks at the encoder output first, so the later checks are reached only with something encoded.
    h2 = hip.HipWhisper(cfg, device=0, max_batch=4, share_with=hm)
    state_refusal(h2, 1, "call nh_encode first")               # nothing encoded (and no tokens either)
    h2.logmel(clips[:1]); h2.encode()
    state_refusal(h2, 1, "call nh_set_tokens first")           # encoded, no tokens
    h2.set_tokens(tk, tk.en, tk.transcribe)
    h2.pool_begin(2)
    h2.logmel_array_rows(np.stack([synth.synth_pcm(3)]), 2); h2.encode_rows(2, 1)    # a staging row: the pool has encoder output
    state_refusal(h2, 3, "decode pool")                        # a running pool
    h2.logmel(clips[:1]); h2.encode()                          # a fresh batch ends the pool: the context decodes again
    assert h2.decode_greedy(max_new_tokens=n)[0]["tokens"] == g0[0]["tokens"]
    h2.close()
    hm.logmel(clips); hm.encode()
    assert hm.decode_greedy(max_new_tokens=n) == g0


# ------------------------------------------------------------------------------------------------------- host layer
def test_host_model_beam_size():
    """Model.set_beam_size(2) through transcribe returns the fork fixture's beam text; set_beam_size(1) is what it was."""
    cfg, tk = common.make_config(NAME), common.tokens_for(NAME)
    steps = F.FIXTURES["fork"](tk)
    over = F.weighted_overrides(cfg, tk, steps)
    om = common.build_oracle(cfg, tk, overrides=over)
    d = host.Definition(host.ModelType.TinyEn, host.SelectedDevice.Rocm(0))
    model = d.blocking_try_to_model(cfg, tk, tk.en, tk.transcribe, ((n, a.astype(np.float16)) for n, a in synth.synth_weights(cfg, 0, over)))
    model.set_temperature_fallback(False)
    pcm = synth.synth_pcm(0)
    O = _oracle()
    xa = om.encoder_forward(O.pcm_to_mel(pcm, assets_io.mel_filters(cfg.num_mel_bins))[:, :3000])
    # transcribe decodes without max_new_tokens: past the script the search runs on, and ends when two hypotheses have finished
    ref = {K: beam_ref.search_ref(F.oracle_step(om, xa), [tk.sot, tk.en, tk.transcribe], K, tk, cfg.max_target_positions - 1) for K in (1, 2)}
    text = lambda toks: [t for t in toks[3:] if t < tk.eot]
    assert text(ref[1]["tokens"]) != text(ref[2]["tokens"]) and ref[2]["min_gap"] >= F.G
    segs1 = model.transcribe(pcm, final_chunk=True)
    last1 = model.last_result()
    model.set_beam_size(1)
    assert model.transcribe(pcm, final_chunk=True) == segs1 and model.last_result() == last1
    model.set_beam_size(2)
    segs2 = model.transcribe(pcm, final_chunk=True)
    assert [t for s in segs2 for t in s] == text(ref[2]["tokens"]) and segs2 != segs1
    assert abs(model.last_result()["avg_logprob"] - ref[2]["avg_logprob"]) <= 5e-3
    model.set_beam_size(1)        # the context of two rows decodes one as the context of one row did: the same bits
    assert model.transcribe(pcm, final_chunk=True) == segs1 and model.last_result() == last1
    with pytest.raises(host.WhisperError):
        model.set_beam_size(9)
    model.close(); om.close()
