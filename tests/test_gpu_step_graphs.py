"""GPU: one context walked through every transition of its captured decode-step graphs.

A context keeps two pairs of step graphs (greedy steps, lockstep or pool; pool steps with a sampled row busy) under a key of
everything the captured kernels take by value.  The other pool tests cover each path on its own; here ONE context goes
lockstep -> pool -> pool with a retry -> all greedy again -> retry again -> new tokens -> new pool -> LayerNorm option ->
lockstep -> another max_new_tokens, and a second context does the same with NH_OPT_DECODE_GRAPHS = 0, where the same step is
launched eagerly.  Every result must be == between the two and == what the clip gives in a lockstep batch of a third
context (nh_decode_greedy, nh_decode_sampled).  No tolerance anywhere."""
import numpy as np
import pytest

import common
from norma_amd import config, synth
from test_gpu_pool import _same, _varlen_weights

pytestmark = pytest.mark.gpu

NAME, N, R = "test-d128", 8, 4          # 8 clips; pools of 4 rows, staging rows 4 .. 11
SEED, CLIP0 = 0x5EED_0123_4567_89AB, 1000
(T1, A1), (T2, A2) = (0.4, 1), (1.0, 5)


def _round(h, clips, admits=(), retries=()):
    """admits: (clip, row) -- encoded into the staging rows and admitted; retries: (row, t, attempt, clip the row holds).
    Steps three at a time and collects every row as it finishes; returns {row: result}."""
    for row, t, attempt, c in retries:
        h.pool_retry(row, t, SEED, CLIP0 + c, attempt)
    if admits:
        h.logmel_array_rows(np.ascontiguousarray(clips[[c for c, _ in admits]]), R)
        h.encode_rows(R, len(admits))
        for i, (_, row) in enumerate(admits):
            h.pool_admit(R + i, row)
    busy = {row for _, row in admits} | {r[0] for r in retries}
    out = {}
    for _ in range(2000):
        flags = h.pool_step(3)
        fin = [r for r in sorted(busy) if flags[r] in (1, 2)]
        if fin:
            out.update(zip(fin, h.pool_collect(fin)))
            busy -= set(fin)
        if not busy:
            return out
    raise AssertionError(f"rows {sorted(busy)} did not finish")


def _script(hip, h, tk, clips):
    """[(what the result must equal: ("g", clip) | (attempt, clip) | ("g5", clip), result)] in the order of the walk"""
    got = []

    def greedy_round(order):
        res = _round(h, clips, admits=[(c, row) for row, c in enumerate(order)])
        got.extend((("g", c), res[row]) for row, c in enumerate(order))

    def retry_round(row, t, attempt, c, admits=()):
        res = _round(h, clips, admits=admits, retries=[(row, t, attempt, c)])
        got.append(((attempt, c), res[row]))
        got.extend((("g", c2), res[row2]) for c2, row2 in admits)

    h.logmel_array(np.ascontiguousarray(clips[:4])); h.encode()                 # 1: lockstep
    got.extend((("g", c), r) for c, r in enumerate(h.decode_greedy()))
    h.pool_begin(R, 0, False)                                                   # 2: the pool's greedy graphs replace them
    greedy_round([0, 1, 2, 3])
    retry_round(0, T1, A1, 0, admits=[(4, 1), (5, 2), (6, 3)])                  # 3: the sampled pair, beside greedy rows
    greedy_round([7, 0, 1, 2])                                                  # 4: back to the greedy pair (row 0: greedy again)
    retry_round(1, T2, A2, 0)                                                   # 5: the sampled pair once more
    h.set_tokens(tk, tk.en, tk.transcribe)                                      # 6: drops every graph
    h.pool_begin(R, 0, False)
    greedy_round([3, 4, 5, 6])
    retry_round(2, T1, A1, 5)
    h.set_option(hip.NH_OPT_FUSE_DECODE_LAYERNORM, 0)                           # 7: drops every graph; the bits stay
    greedy_round([0, 1, 2, 3])
    h.logmel_array(clips); h.encode()                                           # 8: a batch at row 0 ends the pool
    got.extend((("g", c), r) for c, r in enumerate(h.decode_greedy()))
    got.extend((("g5", c), r) for c, r in enumerate(h.decode_greedy(5)))        # another max_new_tokens: another key
    return got


def test_one_context_through_every_step_graph_transition_matches_eager_steps_and_the_lockstep_batch():
    from norma_amd import hip
    cfg, tk = config.preset(NAME), common.tokens_for(NAME)
    hm = _varlen_weights(cfg, tk, eot_steps=[2, 5, 9, 14, 22], text_steps=40, n_calib=8, max_batch=N)
    clips = np.stack([synth.synth_pcm(k) for k in range(N)])
    hm.logmel_array(clips); hm.encode()
    want = {"g": hm.decode_greedy(), "g5": hm.decode_greedy(5),
            A1: hm.decode_sampled(T1, SEED, CLIP0, A1), A2: hm.decode_sampled(T2, SEED, CLIP0, A2)}
    assert len({len(r["tokens"]) for r in want["g"]}) >= 3, [len(r["tokens"]) for r in want["g"]]
    for a, c in ((A1, 0), (A2, 0), (A1, 5)):                                    # the retries of the walk are not the greedy results
        assert not _same(want[a][c], want["g"][c]), (a, c)
    hp = hip.HipWhisper(cfg, device=0, max_batch=12, share_with=hm)
    hq = hip.HipWhisper(cfg, device=0, max_batch=12, share_with=hm)
    for h in (hp, hq):
        h.set_tokens(tk, tk.en, tk.transcribe)
    hq.set_option(hip.NH_OPT_DECODE_GRAPHS, 0)
    gp, gq = _script(hip, hp, tk, clips), _script(hip, hq, tk, clips)
    assert [k for k, _ in gp] == [k for k, _ in gq] and len(gp) == 4 + 4 + 4 + 4 + 1 + 4 + 1 + 4 + 8 + 8
    assert not [(i, k) for i, ((k, a), (_, b)) in enumerate(zip(gp, gq)) if not _same(a, b)]
    for name, got in (("graphs", gp), ("eager", gq)):
        bad = [(name, i, kind, c) for i, ((kind, c), r) in enumerate(got) if not _same(r, want[kind][c])]
        assert not bad, bad
    hm.close(); hp.close(); hq.close()
