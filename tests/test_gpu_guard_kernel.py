"""GPU: the repetition guard's kernel through its parity view (nh_guard_apply) against tests/guard_ref.py, BIT for bit:
every operation of the contract is one IEEE f32 multiply, divide or add, or an assignment, so there is no tolerance.
The view returns the device rows whole: the pad columns (uploaded as all-ones patterns) and the rows that are not edited
must come back as they went in."""
import functools

import numpy as np
import pytest

import common
import guard_ref as G
from norma_amd import hip

pytestmark = pytest.mark.gpu

NAMES = ["test-d128", "test-d256-mel128"]   # V = 51864 and 51866: neither a multiple of 64, the second none of 4 either
A, B_, C_, D_, E_ = 1000, 2000, 3000, 4000, 5000


@functools.lru_cache(maxsize=None)
def _ctx(name):
    cfg, tk = common.make_config(name), common.tokens_for(name)
    hm = hip.HipWhisper(cfg, device=0, max_batch=16)
    hm.set_tokens(tk, tk.en, tk.transcribe)
    return cfg, tk, hm


def _logits(cfg, tk, rows, seed):
    """random logits; the tokens of every row's sequence carry planted values: 0.0, -0.0, negatives, positives"""
    rng = np.random.default_rng(seed)
    lg = (3.0 * rng.standard_normal((len(rows), cfg.vocab_size))).astype(np.float32)
    planted = np.array([0.0, -0.0, -2.5, 3.25, -1e-3, 7.0, -11.0, 0.5], dtype=np.float32)
    for r, (toks, _, _) in enumerate(rows):
        for i, t in enumerate(dict.fromkeys(toks)):
            if i % 3 != 2:     # a third keeps its random value
                lg[r, t] = planted[(i + r) % len(planted)]
    return lg


def _run(name, p, rows, prompt_len, seed=0):
    """rows: [(tokens, active, bias dict | None)].  Asserts the view equals the reference on every row; returns the flags."""
    cfg, tk, hm = _ctx(name)
    V = cfg.vocab_size
    ld = (V + 63) & ~63
    lg = _logits(cfg, tk, rows, seed)
    for r, (_, _, bias) in enumerate(rows):
        hm.guard_bias(r, bias)
    hm.set_guard(p.no_repeat_ngram, p.repetition_penalty, p.loop_period, p.loop_repeats, p.bias)
    out, flags = hm.guard_apply(lg, [t for t, _, _ in rows], prompt_len=prompt_len, active=[int(a) for _, a, _ in rows],
                                bias_rows=[r if b else -1 for r, (_, _, b) in enumerate(rows)])
    hm.set_guard(None)
    for r in range(len(rows)):
        hm.guard_bias(r, None)
    assert out.shape == (len(rows), ld)
    assert np.all(out[:, V:].view(np.uint32) == 0xFFFFFFFF), "pad columns were written"
    for r, (toks, active, bias) in enumerate(rows):
        if active:
            want, ex = G.edit(lg[r], toks, len(toks), prompt_len, p, bias, tk)
        else:
            want, ex = lg[r], 0
        bad = np.nonzero(out[r, :V].view(np.uint32) != want.view(np.uint32))[0]
        assert bad.size == 0, (r, bad[:8].tolist(), out[r, bad[:8]].tolist(), want[bad[:8]].tolist())
        assert flags[r] == ex, (r, flags[r], ex)
    return flags


def _prompt(tk):
    return [tk.sot, tk.en, tk.transcribe]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("N", (1, 2, 3, 5))
def test_ngram_and_penalty_on_short_histories(name, N):
    """m = 0, N - 2, N - 1, N, N + 1 and histories with duplicates, under the ban alone, the penalty alone and both"""
    cfg, tk, hm = _ctx(name)
    Z, P = tk.zero_sec, _prompt(tk)
    cyc = [A, B_, C_, A, B_, D_, A, B_, C_, C_, A, B_]
    rows = [(P + [Z] + cyc[:m], True, None) for m in sorted({0, max(N - 2, 0), N - 1, N, N + 1})]
    rows += [(P + [Z] + cyc, True, None), (P + [Z] + [A] * 7, True, None), (P + [Z, A, B_, Z + 5, Z + 9] + cyc[2:], True, None)]
    for p in (G.params(no_repeat_ngram=N), G.params(repetition_penalty=1.3), G.params(no_repeat_ngram=N, repetition_penalty=0.75)):
        _run(name, p, rows, 3, seed=N)


@pytest.mark.parametrize("name", NAMES)
def test_long_histories_around_one_workgroup_and_at_the_cap(name):
    """255, 256 and 257 text tokens (the workgroup's width: the compaction's second round), 445 (all a row can hold), drawn
    from few ids so that bigrams recur; timestamps in between; prompt_len = 1 so that 445 fit"""
    cfg, tk, hm = _ctx(name)
    Z = tk.zero_sec
    rng = np.random.default_rng(5)
    rows = []
    for m in (255, 256, 257, 445):
        rows.append(([tk.sot] + [int(v) for v in rng.choice([A, B_, C_, D_, E_, 600, 700], m)], True, None))
    # the same with timestamp pairs every 37 tokens: physical length 446 at the most
    text = [int(v) for v in rng.choice([A, B_, C_, D_], 400)]
    seq = [tk.sot]
    for i, v in enumerate(text):
        if i % 37 == 0:
            seq += [Z + i, Z + i + 1]
        seq.append(v)
    rows.append((seq[:446], True, None))
    assert len(rows[3][0]) == cfg.max_target_positions - 2
    for p in (G.params(no_repeat_ngram=2, repetition_penalty=1.2), G.params(no_repeat_ngram=3), G.params(repetition_penalty=2.0),
              G.params(no_repeat_ngram=16, repetition_penalty=1.1, loop_period=64, loop_repeats=7)):
        _run(name, p, rows, 1, seed=3)


@pytest.mark.parametrize("name", NAMES)
def test_ngram_spans_a_timestamp_and_ignores_the_prefix(name):
    cfg, tk, hm = _ctx(name)
    Z = tk.zero_sec
    p = G.params(no_repeat_ngram=3)
    # a b | ts ts | c ... a b: h = a b c a b, the trigram a b c spans the timestamps: c is banned
    rows = [(_prompt(tk) + [Z, A, B_, Z + 5, Z + 6, C_, A, B_], True, None)]
    flags = _run(name, p, rows, 3)
    x, _ = G.edit(np.zeros(cfg.vocab_size, dtype=np.float32), rows[0][0], len(rows[0][0]), 3, p, None, tk)
    assert x[C_] == -np.inf and np.isfinite(x[D_])
    # a prefix in front of the prompt (prompt_len = 7) holds a b c: not history, so a b bans nothing ...
    pre = [50, A, B_, C_]
    rows = [(pre + _prompt(tk) + [Z, A, B_], True, None), (pre + _prompt(tk) + [Z, A, B_, D_, A, B_], True, None)]
    _run(name, p, rows, 7)
    x, _ = G.edit(np.zeros(cfg.vocab_size, dtype=np.float32), rows[0][0], len(rows[0][0]), 7, p, None, tk)
    assert np.isfinite(x[C_])
    x, _ = G.edit(np.zeros(cfg.vocab_size, dtype=np.float32), rows[1][0], len(rows[1][0]), 7, p, None, tk)
    assert np.isfinite(x[C_]) and x[D_] == -np.inf     # ... and in the second row only what was generated does
    assert flags.tolist() == [0]


@pytest.mark.parametrize("name", NAMES)
def test_bias(name):
    """finite biases, -inf, a bias on a token the n-gram bans, on a penalised token, on timestamps and the last id; a row whose
    list is not used; 256 entries"""
    cfg, tk, hm = _ctx(name)
    Z, V = tk.zero_sec, cfg.vocab_size
    seq = _prompt(tk) + [Z, A, B_, C_, A, B_]
    big = {int(300 + 7 * i): float(np.float32(0.01 * i - 1.0)) for i in range(hip.NH_GUARD_MAX_BIAS)}
    rows = [(seq, True, {C_: 5.0, D_: -np.inf, A: 2.5, V - 1: -3.0, 0: 1e4, Z + 3: -0.5}),
            (seq, True, None), (seq, True, big), (seq, False, {C_: 5.0})]
    for p in (G.params(bias=True), G.params(bias=True, no_repeat_ngram=3, repetition_penalty=1.5), G.params(no_repeat_ngram=3)):
        _run(name, p, rows, 3, seed=9)
    x, _ = G.edit(np.zeros(V, dtype=np.float32), seq, len(seq), 3, G.params(bias=True, no_repeat_ngram=3), rows[0][2], tk)
    assert x[C_] == -np.inf and x[D_] == -np.inf and x[A] == 2.5


@pytest.mark.parametrize("name", NAMES)
def test_loop_exit(name):
    cfg, tk, hm = _ctx(name)
    Z, P = tk.zero_sec, _prompt(tk)
    blk = [A, B_, C_, D_]
    p = G.params(loop_period=4, loop_repeats=3)
    rows = [
        (P + [Z] + [A] * 3, True, None),                      # 0: p = 1, p * R == m, last token text: taken
        (P + [Z] + [A] * 2, True, None),                      # 1: one copy short: not taken
        (P + [Z] + blk * 3, True, None),                      # 2: p = Pmax, p * R == m: taken
        (P + [Z, E_] + blk * 3, True, None),                  # 3: p * R one short of m: taken
        (P + [Z] + blk[1:] + blk * 2, True, None),            # 4: m one short of p * R: not taken
        (P + [Z] + blk * 3 + [Z + 9], True, None),            # 5: text then a timestamp (timestamps only): deferred
        (P + [Z] + blk * 3 + [Z + 9, Z + 9], True, None),     # 6: two timestamps (text only): taken
        (P + blk * 3, True, None),                            # 7: no timestamp generated yet (first-token rule): deferred
        (P + [Z] + [A, B_] * 3 + [A, C_] + [A, B_] * 2, True, None),   # 8: the copies must be the LAST tokens: 2 only, not taken
        (P + [Z, A, B_, Z + 4, Z + 5, A, B_, Z + 9, Z + 11, A, B_], True, None),   # 9: copies with different timestamps: taken
        (P + [Z] + [A] * 3, False, None),                     # 10: finished row: untouched, no flag
        (P + [Z] + [A, B_, C_, D_, E_] * 3, True, None),      # 11: period 5 > Pmax: not taken
    ]
    flags = _run(name, p, rows, 3, seed=2)
    assert flags.tolist() == [1, 0, 1, 1, 0, 0, 1, 0, 0, 1, 0, 0]
    # with the other components on: the exit is the last edit, eot keeps what penalty and bias left it (eot is never in h)
    rows[0] = (rows[0][0], True, {tk.eot: 1.5, A: -np.inf})
    flags = _run(name, G.params(loop_period=4, loop_repeats=3, no_repeat_ngram=2, repetition_penalty=1.2, bias=True), rows, 3, seed=4)
    assert flags.tolist() == [1, 0, 1, 1, 0, 0, 1, 0, 0, 1, 0, 0]
    # p = 1 with R at its largest, Pmax at its largest
    rows = [(P + [Z] + [A] * 16, True, None), (P + [Z] + [A] * 15, True, None), (P + [Z] + list(range(300, 364)) * 2, True, None)]
    assert _run(name, G.params(loop_period=1, loop_repeats=16), rows, 3).tolist() == [1, 0, 0]
    assert _run(name, G.params(loop_period=64, loop_repeats=2), rows, 3).tolist() == [1, 1, 1]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("R", (1, 3, 16))
def test_row_counts_and_untouched_rows(name, R):
    cfg, tk, hm = _ctx(name)
    Z, P = tk.zero_sec, _prompt(tk)
    rng = np.random.default_rng(R)
    rows = []
    for r in range(R):
        m = int(rng.integers(0, 40))
        seq = P + [Z] + [int(v) for v in rng.choice([A, B_, C_, D_], m)] + ([A] * 4 if r % 4 == 1 else [])
        rows.append((seq, r % 3 != 2 or R == 1, {E_: -np.inf, A: 0.25} if r % 2 else None))
    p = G.params(no_repeat_ngram=2, repetition_penalty=1.25, loop_period=2, loop_repeats=4, bias=True)
    flags = _run(name, p, rows, 3, seed=R)
    if R == 16:
        assert flags.sum() >= 1 and any(not a for _, a, _ in rows)
