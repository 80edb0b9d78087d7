"""GPU: a prompt prefix per row of the decode pool (nh_pool_prefix), prefilled in one ragged pass.

The yardstick is the one the pool already answers to: tokens, avg_logprob and no_speech_prob of a pooled clip are, bit for
bit, those of the lockstep decode of that clip -- here nh_set_prompts + nh_decode_greedy / nh_decode_sampled on a B = 1
context of the same weights.  Prefix lengths sit at the edges of the route and of prefill_attn_kernel: 0 (none), 1 (below
NH_PREFILL_MIN_PREFIX = 4: through the steps), 4 (the threshold), 17 (one wave against two), 65 (one key block against two),
223 (the longest).  The oracle-backed reference of prompted decodes (tests/prompt_ref.py) is asked once more on the tiny.en
fixture, within the 1e-3 of the existing decode tests."""
import numpy as np
import pytest

import common
import prompt_ref as R
from norma_amd import assets_io, hip, synth

pytestmark = pytest.mark.gpu

NH_ERR_INVALID, NH_ERR_STATE = 1, 3
NAME = "test-d128"
LENGTHS = (0, 1, 4, 17, 65, 223)
ROWS, STAGING = 6, 6


def _oracle():
    from oracle import oracle as O
    return O


@pytest.fixture(scope="module")
def pair():
    """one pool context (6 rows + 6 staging rows) and one B = 1 lockstep context on the scripted weights of
    test_a_clip_is_bit_identical_alone_and_in_a_batch; six clips; the lockstep results, computed once per (clip, prefix, how)"""
    cfg, tk = common.make_config(NAME), common.tokens_for(NAME)
    over = common.scripted_overrides(cfg, tk, R.long_script(tk))
    _, (hp, h1) = common.build_together(cfg, tk, overrides=over, batches=(ROWS + STAGING, 1), with_oracle=False)
    clips = np.stack([synth.synth_pcm(k) for k in range(6)])
    refs = {}

    def lockstep(c, prefix, stepwise=0, max_new=0, sampled=None, guard=None):
        key = (c, tuple(prefix), stepwise, max_new, sampled, None if guard is None else tuple(sorted(guard.items())))
        if key not in refs:
            h1.set_option(hip.NH_OPT_PROMPT_STEPWISE, stepwise)
            h1.set_guard(**guard) if guard else h1.set_guard(None)
            h1.logmel_array(np.ascontiguousarray(clips[c:c + 1])); h1.encode()
            h1.set_prompts([list(prefix)] if len(prefix) else None)
            if sampled is None:
                res = h1.decode_greedy(max_new_tokens=max_new)[0]
            else:
                t, seed, clip, attempt = sampled
                res = h1.decode_sampled(t, seed=seed, clip0=clip, attempt=attempt, max_new_tokens=max_new)[0]
            if guard:
                res = dict(res, loop_exit=int(h1.guard_report()[0]))
            refs[key] = res
        return refs[key]
    yield cfg, tk, hp, h1, clips, lockstep
    hp.close(); h1.close()


def _fresh(hp, clips, graphs=1, stepwise=0, max_new=0, rows=ROWS, per_clip_language=False, guard=None, n_staged=6):
    """a fresh pool on hp, clips 0 .. n_staged - 1 encoded into its staging rows"""
    hp.set_option(hip.NH_OPT_DECODE_GRAPHS, graphs)
    hp.set_option(hip.NH_OPT_PROMPT_STEPWISE, stepwise)
    hp.pool_begin(rows, max_new, per_clip_language)
    hp.set_guard(**guard) if guard else hp.set_guard(None)
    hp.logmel_array_rows(np.ascontiguousarray(clips[:n_staged]), rows)
    hp.encode_rows(rows, n_staged)


def _drain(hp, rows, step=8):
    """steps until every row of `rows` has finished; {row: its collected result}"""
    for _ in range(80):
        flags = hp.pool_step(step)
        if all(flags[r] in (1, 2) for r in rows):
            return dict(zip(rows, hp.pool_collect(list(rows))))
    raise AssertionError(f"rows {rows} did not finish: {flags}")


# ------------------------------------------------------------------------------------------------ bit identity
@pytest.mark.parametrize("graphs", (1, 0))
@pytest.mark.parametrize("stepwise", (0, 1))
def test_prefixed_rows_are_bit_identical_to_the_prompted_lockstep_decode(pair, graphs, stepwise):
    """six clips, six prefix lengths, all admitted before the first step into a permuted row order: on the default route ONE
    ragged pass over the clips of 4, 17, 65 and 223 ids (packed offsets 0, 4, 21, 86 in admission order: off the multiples of
    16), the clip of 1 id through the steps, the clip of none as ever"""
    cfg, tk, hp, h1, clips, lockstep = pair
    _fresh(hp, clips, graphs, stepwise)
    row_of = (3, 5, 0, 4, 1, 2)
    pre = [R.prefix_tokens(tk, n, c) if n else [] for c, n in enumerate(LENGTHS)]
    for c in range(6):
        hp.pool_prefix(row_of[c], pre[c])
        hp.pool_admit(ROWS + c, row_of[c])
    got = _drain(hp, list(range(ROWS)))
    for c, n in enumerate(LENGTHS):
        want = lockstep(c, pre[c], stepwise)
        print(n, graphs, stepwise, len(want["tokens"]), want["avg_logprob"], want["no_speech_prob"])
        assert got[row_of[c]] == want, (n, got[row_of[c]], want)          # tokens, avg_logprob, no_speech_prob: the same bits
        assert got[row_of[c]]["tokens"][:3] == [tk.sot, tk.en, tk.transcribe] and len(got[row_of[c]]["tokens"]) > 4, n
    # the prefixes' contents matter to the result: another clip's ids give other numbers
    assert lockstep(3, pre[3], stepwise) != lockstep(3, R.prefix_tokens(tk, 17, 0), stepwise)


def _same(got, want, tol=1e-3):
    assert got["tokens"] == want["tokens"]
    assert abs(got["avg_logprob"] - want["avg_logprob"]) <= tol and abs(got["no_speech_prob"] - want["no_speech_prob"]) <= tol
    assert got["no_speech_exit"] == want["no_speech_exit"]


def test_prefixed_rows_match_the_reference_on_the_scripted_tiny_en_fixture():
    cfg, tk, over, om, xas, mels = R.scripted_fixture()
    rows = 2 * len(R.PREFIX_LENGTHS)
    # the decoding context never encodes (nh_pool_admit_from): the ragged pass runs in workspaces no encoder of its own ever
    # wrote; the encoder context takes the oracle's own mels
    hp = common.build_hip(cfg, tk, overrides=over, max_batch=rows + 1)
    enc = hip.HipWhisper(cfg, device=0, max_batch=2, share_with=hp)
    enc.set_tokens(tk, tk.en, tk.transcribe)
    enc.set_mel(mels); enc.encode()
    hp.pool_begin(rows)
    jobs = [(n, b) for n in R.PREFIX_LENGTHS for b in range(2)]
    for r, (n, b) in enumerate(jobs):
        hp.pool_prefix(r, R.prefix_tokens(tk, n, b))
        hp.pool_admit_from(enc, b, r)
    got = _drain(hp, list(range(rows)))
    for r, (n, b) in enumerate(jobs):
        want = R.prompted_decode(om, xas[b], R.prefix_tokens(tk, n, b))
        print(n, b, got[r]["avg_logprob"] - want["avg_logprob"], got[r]["no_speech_prob"] - want["no_speech_prob"])
        _same(got[r], want)
        assert got[r]["tokens"][:3] == [tk.sot, tk.en, tk.transcribe]
    enc.close(); hp.close()


@pytest.mark.parametrize("n", (33,))
def test_the_ragged_pass_leaves_every_prefix_in_its_own_rows_cache(n):
    """the loud-self-attention weights of test_the_one_pass_leaves_the_prefix_in_the_self_cache: the no-speech probability,
    read right behind the prefix, moves with the prefix's CONTENTS.  Four copies of one clip, four prefixes, rows permuted:
    a prefix whose K/V landed in another row's cache, or nowhere, cannot give the lockstep bits."""
    O = _oracle()
    cfg, tk = common.make_config(NAME), common.tokens_for(NAME)
    over = {}
    for l in range(cfg.decoder_layers):
        for w in ("v_proj", "out_proj"):
            key = f"model.decoder.layers.{l}.self_attn.{w}.weight"
            over[key] = (synth.synth_tensor_by_name(cfg, key, 0) * np.float32(4)).astype(np.float16).astype(np.float32)
    om, (hp, h4) = common.build_together(cfg, tk, overrides=over, batches=(5, 4))
    clip = synth.synth_pcm(0)
    xa = om.encoder_forward(O.pcm_to_mel(clip, assets_io.mel_filters(cfg.num_mel_bins))[:, :3000])
    pre = [R.prefix_tokens(tk, n, c) for c in range(4)]
    sigma = max(float(om.final_linear(om.decoder_forward(p + [tk.sot], xa, True)[-1])[0].std()) for p in pre)
    tol = 2 * 4e-3 * max(sigma, 0.1)                       # that test's bar
    h4.logmel([clip] * 4); h4.encode()
    h4.set_prompts(pre)
    want = [r["no_speech_prob"] for r in h4.decode_greedy(max_new_tokens=1)]
    hp.pool_begin(4, 1)
    hp.logmel_array_rows(clip[None, :], 4); hp.encode_rows(4, 1)
    row_of = (2, 0, 3, 1)
    for c in range(4):
        hp.pool_prefix(row_of[c], pre[c])
        hp.pool_admit(4, row_of[c])
    got = _drain(hp, [0, 1, 2, 3])
    logs = [float(np.log(w)) for w in want]
    print("want", want, "spread", max(logs) - min(logs), "tol", tol)
    assert max(logs) - min(logs) >= 10 * tol
    assert [got[row_of[c]]["no_speech_prob"] for c in range(4)] == want
    hp.close(); h4.close(); om.close()


# ------------------------------------------------------------------------------------------------ neighbours
def test_a_running_unprefixed_row_is_untouched_by_a_prefill_in_mid_flight(pair):
    cfg, tk, hp, h1, clips, lockstep = pair
    _fresh(hp, clips)
    long_pre = R.prefix_tokens(tk, 65, 3)                  # clip 3 under 65 ids decodes for some 160 steps: still running below
    hp.pool_prefix(0, long_pre)
    hp.pool_admit(ROWS + 3, 0)
    hp.pool_admit(ROWS + 0, 1)                             # unprefixed, a short transcript
    assert list(hp.pool_step(3))[:2] == [0, 0]            # both in mid-flight, off a multiple of the graph's 8 steps
    p223 = R.prefix_tokens(tk, 223, 5)
    hp.pool_prefix(2, p223)
    hp.pool_admit(ROWS + 5, 2)                             # ... prefilled at the head of the next step
    got = _drain(hp, [0, 1, 2])
    assert got[1] == lockstep(0, []) and got[0] == lockstep(3, long_pre) and got[2] == lockstep(5, p223)


def test_staged_clips_wait_unharmed_while_a_prefix_is_prefilled_and_stepped(pair):
    """of three staged clips one is admitted under a prefix and stepped -- the ragged pass runs in the encoder's workspaces --
    before the other two are admitted from their staging rows"""
    cfg, tk, hp, h1, clips, lockstep = pair
    _fresh(hp, clips, n_staged=3)
    p = R.prefix_tokens(tk, 223, 1)
    hp.pool_prefix(4, p)
    hp.pool_admit(ROWS + 1, 4)
    hp.pool_step(5)
    hp.pool_admit(ROWS + 0, 2)
    p2 = R.prefix_tokens(tk, 17, 2)
    hp.pool_prefix(0, p2)
    hp.pool_admit(ROWS + 2, 0)
    got = _drain(hp, [0, 2, 4])
    assert got[4] == lockstep(1, p) and got[2] == lockstep(0, []) and got[0] == lockstep(2, p2)


def test_the_one_pass_saves_the_prefixs_steps(pair):
    """deterministic: 223 ids, two new tokens.  One pass: the row stands at sot after it and is through in 4 steps.  Stepwise:
    after 8 steps it is still inside its prefix."""
    cfg, tk, hp, h1, clips, lockstep = pair
    p = R.prefix_tokens(tk, 223, 0)
    flags = {}
    for stepwise in (0, 1):
        _fresh(hp, clips, stepwise=stepwise, max_new=2, n_staged=1)
        hp.pool_prefix(0, p)
        hp.pool_admit(ROWS, 0)
        flags[stepwise] = int(hp.pool_step(8)[0])
        if stepwise == 0:
            assert hp.pool_collect([0])[0] == lockstep(0, p, 0, max_new=2)
    assert flags == {0: 1, 1: 0}


# ------------------------------------------------------------------------------------------------ retry, guard, cap
@pytest.mark.parametrize("n,stepwise", ((5, 1), (223, 0)))
def test_a_retry_restarts_behind_the_prefix_with_the_lockstep_sampled_bits(pair, n, stepwise):
    cfg, tk, hp, h1, clips, lockstep = pair
    _fresh(hp, clips, stepwise=stepwise, max_new=12)
    p = R.prefix_tokens(tk, n, 2)
    hp.pool_prefix(3, p)
    hp.pool_admit(ROWS + 2, 3)
    hp.pool_admit(ROWS + 1, 0)                             # a greedy neighbour
    got = _drain(hp, [0, 3])
    assert got[3] == lockstep(2, p, stepwise, max_new=12)
    seed, clip, attempt = 0x1234_5678_9ABC, 40, 2
    hp.pool_retry(3, 0.6, seed, clip, attempt)
    again = _drain(hp, [3])[3]
    want = lockstep(2, p, stepwise, max_new=12, sampled=(0.6, seed, clip, attempt))
    print(n, "greedy", got[3]["tokens"][3:], "sampled", again["tokens"][3:])
    assert again == want, (again, want)


def test_guard_and_max_new_tokens_count_from_behind_the_prefix(pair):
    cfg, tk, hp, h1, clips, lockstep = pair
    guard = dict(no_repeat_ngram=3, loop_period=4, loop_repeats=3)
    _fresh(hp, clips, max_new=8, guard=guard)
    # 65 ids: generation starts among the script's fillers, a repetition the guard acts on
    jobs = [(0, 0, []), (1, 65, R.prefix_tokens(tk, 65, 1)), (2, 223, R.prefix_tokens(tk, 223, 2)), (3, 1, R.prefix_tokens(tk, 1, 3))]
    for c, n, p in jobs:
        hp.pool_prefix(c, p)
        hp.pool_admit(ROWS + c, c)
    got = _drain(hp, [0, 1, 2, 3])
    rep = hp.guard_report([0, 1, 2, 3])
    plain = lockstep(1, jobs[1][2], 0, max_new=8)
    for c, n, p in jobs:
        want = lockstep(c, p, 0, max_new=8, guard=guard)
        assert dict(got[c], loop_exit=int(rep[c])) == want, (n, got[c], rep[c], want)
        assert len(want["tokens"]) <= 3 + 8 + 1
    assert lockstep(1, jobs[1][2], 0, max_new=8, guard=guard)["tokens"] != plain["tokens"]   # the guard did act under the prefix
    hp.set_guard(None); h1.set_guard(None)


def test_the_length_cap_counts_the_physical_sequence():
    """the weights of R.scripted_fixture(endless_from=223), made here without that fixture's oracle: a segment that never
    closes behind 223 ids ends at physical length C, and what comes back counts from sot"""
    cfg, tk = common.make_config("tiny.en"), common.tokens_for("tiny.en")
    over = common.scripted_overrides(cfg, tk, R.long_script(tk, 223))
    _, (hp, h1) = common.build_together(cfg, tk, overrides=over, batches=(3, 1), with_oracle=False)
    C, n = cfg.max_target_positions, 223
    p = R.prefix_tokens(tk, n, 0)
    clip = synth.synth_pcm(0)
    h1.logmel([clip]); h1.encode(); h1.set_prompts([p])
    want = h1.decode_greedy()[0]
    hp.pool_begin(2)
    hp.logmel_array_rows(clip[None, :], 2); hp.encode_rows(2, 1)
    hp.pool_prefix(1, p)
    hp.pool_admit(2, 1)
    got = _drain(hp, [1], step=16)[1]
    t = got["tokens"]
    assert len(t) == C - n and t[-1] == tk.eot and tk.eot not in t[:-1] and t[:4] == [tk.sot, tk.en, tk.transcribe, tk.zero_sec]
    assert got == want
    hp.close(); h1.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_pending_prefixes_and_rows_as_they_were(pair):
    cfg, tk, hp, h1, clips, lockstep = pair
    L, h = hp.L, hp._h
    C = cfg.max_target_positions
    p5, p17 = R.prefix_tokens(tk, 5, 0), R.prefix_tokens(tk, 17, 1)
    a5 = np.ascontiguousarray(p5, dtype=np.int32)
    # no pool: a context that runs none
    assert L.nh_pool_prefix(h1._h, 0, hip._ip(a5), 5) == NH_ERR_STATE
    _fresh(hp, clips, per_clip_language=True)
    hp.pool_detect_languages([tk.en])
    hp.align_capture([(0, 0), (1, 1)])
    hp.pool_prefix(1, p17)
    hp.pool_admit(ROWS + 1, 1, tk.en)                      # row 1 is busy from here on
    big = np.zeros(C, dtype=np.int32)
    refusals = [(ROWS, a5, 5), (-1, a5, 5), (1, a5, 5),    # outside the pool (a staging row, a negative one), a busy row
                (0, big, C // 2), (0, a5, -1)]             # one past the longest prefix, a negative length
    for bad in (-1, cfg.vocab_size):
        t = a5.copy(); t[3] = bad
        refusals.append((0, t, 5))                         # a token id outside the vocabulary
    for row, arr, n in refusals:
        hp.pool_prefix(0, p5)
        assert L.nh_pool_prefix(h, row, hip._ip(arr), n) == NH_ERR_INVALID, (row, n)
        hp.pool_admit(ROWS + 0, 0, tk.en)
        assert _drain(hp, [0])[0] == lockstep(0, p5), (row, n)   # the prefix pending before the refusal is the one consumed
    # a detecting admission into a row with a pending prefix, and an admission refused for another reason: still pending
    hp.pool_prefix(0, p5)
    assert L.nh_pool_admit(h, ROWS + 0, 0, hip.NH_LANG_DETECT) == NH_ERR_INVALID
    assert L.nh_pool_admit(h, 0, 0, tk.en) != 0           # src_row is no staging row
    assert L.nh_pool_admit(h, ROWS + 0, 1, tk.en) == NH_ERR_INVALID   # dst_row busy
    a = np.ascontiguousarray([p5], dtype=np.int32)
    assert L.nh_set_prompts(h, hip._ip(a), 5, 5, 1) == NH_ERR_STATE   # a pool takes no batch prefix
    hp.pool_admit(ROWS + 0, 0, tk.en)
    got = _drain(hp, [0, 1])
    assert got[0] == lockstep(0, p5) and got[1] == lockstep(1, p17)   # keeping the queries changes no bit; row 1 saw nothing
    # one-shot, and cleared by hand and by pool_begin
    hp.pool_admit(ROWS + 0, 0, tk.en)
    hp.pool_prefix(2, p5); hp.pool_prefix(2, None)
    hp.pool_admit(ROWS + 0, 2, tk.en)
    hp.pool_prefix(3, p5); hp.pool_prefix(3, [])
    hp.pool_admit(ROWS + 0, 3, tk.en)
    got = _drain(hp, [0, 2, 3])
    assert got[0] == got[2] == got[3] == lockstep(0, [])
    # align_decoded: refused on the row whose last decode had a prefix, working on an unprefixed row of the same pool
    hp.pool_prefix(4, p5)
    hp.pool_admit(ROWS + 0, 4, tk.en)
    assert _drain(hp, [4])[4] == lockstep(0, p5)
    with pytest.raises(hip.HipError) as e:
        hp.align_decoded([4])
    assert e.value.code == NH_ERR_STATE
    first, last = hp.align_decoded([0])
    assert len(first) == len(last) == 1
    hp.pool_prefix(5, p5)
    hp.align_capture([])
    _fresh(hp, clips)                                      # nh_pool_begin clears every pending prefix
    hp.pool_admit(ROWS + 0, 5)
    assert _drain(hp, [5])[5] == lockstep(0, [])
