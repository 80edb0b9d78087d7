"""The beam search contract (tests/beam_ref.py) on hand-made probability tables, and the three fixtures of
tests/beam_fixture.py on the CPU oracle: decidable (every cut gap >= G) before any GPU run.  No GPU."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest

import beam_fixture as F
import beam_ref
import common

# a toy vocabulary: text 0 .. 4, eot 5, specials 6 .. 8 (no_timestamps 8), timestamps 9 .. 11
TK = SimpleNamespace(eot=5, no_timestamps=8, zero_sec=9, one_sec=10, sot=6)
V = 12


def table_step(table, default=None):
    """step callback from {tuple(tokens after the prompt): {token: probability}}."""
    def step(tokens, last_ts):
        row = table.get(tuple(tokens[1:]), default)
        q = np.zeros(V)
        for t, p in (row or {}).items():
            q[t] = p
        return q
    return step


def search(table, K, cap=20, max_new=0, default=None):
    return beam_ref.search_ref(table_step(table, default), [TK.sot], K, TK, cap, max_new=max_new)


def test_eot_fork_changes_the_winner_at_k2():
    # greedy walks on with 0.55 and then pays 0.3 twice; the early eot (0.45) has the better average
    table = {(): {0: 1.0}, (0,): {1: 0.55, TK.eot: 0.45}, (0, 1): {2: 0.3, 3: 0.25}, (0, 1, 2): {TK.eot: 0.3, 4: 0.2},
             (0, 1, 3): {TK.eot: 0.9}, (0, 1, 2, 4): {TK.eot: 1.0}}
    r1, r2 = search(table, 1), search(table, 2)
    assert r1["tokens"] == [TK.sot, 0, 1, 2, TK.eot]
    assert r2["tokens"] == [TK.sot, 0, TK.eot]
    assert r2["avg_logprob"] == pytest.approx(math.log(0.45) / 3)
    assert [t for t, _ in r2["finished"]][0] == [TK.sot, 0, TK.eot]          # finishing order: the early eot first
    assert r2["parents"][1] == [0] and r2["parents"][0] == [0]               # one live child while the eot took a slot... of the list


def test_finished_list_overflow_drops_the_later_eot():
    # step 2 offers eot from both live hypotheses; with one finished already only one more fits at K = 2
    table = {(): {0: 0.6, TK.eot: 0.4}, (0,): {1: 0.5, 2: 0.3, TK.eot: 0.2}, (0, 1): {TK.eot: 0.6, 3: 0.4}, (0, 2): {TK.eot: 0.9, 3: 0.1}}
    r = search(table, 2)
    fins = [t for t, _ in r["finished"]]
    assert fins == [[TK.sot, TK.eot], [TK.sot, 0, 1, TK.eot]] or fins == [[TK.sot, TK.eot], [TK.sot, 0, 2, TK.eot]]
    assert len(fins) == 2
    # scores: 0.5 * 0.6 = 0.30 * 0.6 against 0.3 * 0.6 = 0.18 * 0.9 = 0.162 < 0.18: [0, 1, eot] is admitted, [0, 2, eot] dropped
    assert fins[1] == [TK.sot, 0, 1, TK.eot]
    assert math.isfinite(r["min_gap"])


def test_forced_eot_at_max_new_tokens_and_at_the_cap():
    table = {}
    loop = {0: 0.7, 1: 0.3}
    r = search(table, 2, max_new=3, default=loop)
    for t, s in r["finished"]:
        assert len(t) == 1 + 3 + 1 and t[-1] == TK.eot
    assert r["finished"][0][0] == [TK.sot, 0, 0, 0, TK.eot]
    assert r["finished"][0][1] == pytest.approx(3 * math.log(0.7))           # the forced eot adds no log-probability
    r = search(table, 1, cap=6, default=loop)
    assert r["finished"][0][0] == [TK.sot, 0, 0, 0, 0, 0, TK.eot]            # 6 tokens reach the cap, eot is pushed behind them
    assert r["finished"][0][1] == pytest.approx(5 * math.log(0.7))


def test_all_masked_row_ends_the_clip_without_a_finished_hypothesis():
    table = {(): {0: 1.0}, (0,): {}}
    r = search(table, 2)
    assert r["tokens"] is None and r["finished"] == []


def test_tie_orders():
    # equal scores everywhere: lower parent beam first, then the higher token id
    table = {(): {0: 0.5, 1: 0.5}, (1,): {2: 0.5, 3: 0.5}, (0,): {2: 0.5, 3: 0.5}}
    r = beam_ref.search_ref(table_step(table), [TK.sot], 2, TK, 20, max_new=2)
    # step 1: tokens 1 then 0 (higher id first); step 2: both children of beam 0 (= token 1), 3 before 2
    assert r["parents"] == [[0, 0], []] or r["parents"][0] == [0, 0]
    assert [t for t, _ in r["finished"]] == [[TK.sot, 1, 3, TK.eot], [TK.sot, 1, 2, TK.eot]]
    # the final ranking: equal averages, the earliest finished wins
    assert r["winner"] == 0


def test_step_ref_rules_and_state_travel():
    """One step of the single-step reference on a toy layout: a closing-timestamp row may only take later timestamps, and
    the child inherits the parent's last_ts when it appends text."""
    tk = SimpleNamespace(eot=5, no_timestamps=8, zero_sec=9, one_sec=10, sot=6)
    sup = np.zeros(V, dtype=bool)
    sup[[6, 7, 8]] = True
    K, B, Cn = 2, 1, 16
    toks = np.zeros((2, Cn), dtype=np.int32)
    toks[0, :4] = [6, 9, 0, 10]      # text then a timestamp: timestamps > 10 only
    toks[1, :4] = [6, 9, 0, 1]       # text: decided by the masses
    state = dict(tokens=toks, n_tokens=[4, 4], have_last=[1, 1], last_ts=[10, 9], live=[1, 1], score=[-1.0, -1.2])
    lg = np.full((2, V), -5.0, dtype=np.float32)
    lg[0, [2, 11, 9]] = [4.0, 3.5, 3.0]     # text 2 and timestamp 9 are illegal for row 0: 11 is all it may take
    lg[1, [3, 4]] = [3.0, 2.0]
    r = beam_ref.step_ref(lg, state, K, B, [0], sup, tk, cap=Cn - 1)
    assert r["decided"] == [True]
    assert r["parent"].tolist() == [1, 0]      # -1.2 + log 0.72 (row 1, token 3) ahead of -1.0 + log 0.31 (row 0, token 11)
    kids = {int(r["tokens"][j, 4]): j for j in range(2)}
    assert 11 in kids and r["last_ts"][kids[11]] == 11
    assert 3 in kids and r["last_ts"][kids[3]] == 9 and r["n_tokens"][kids[3]] == 5


# ---- the fixtures on the CPU oracle ---------------------------------------------------------------------------------------
NAME = "test-d128"
KS = (1, 2, 4, 5)


@functools.lru_cache(maxsize=None)
def fixture_model(fx, name=NAME, lang=None):
    cfg, tk = common.make_config(name), common.tokens_for(name)
    steps = F.FIXTURES[fx](tk)
    om = common.build_oracle(cfg, tk, overrides=F.weighted_overrides(cfg, tk, steps, prompt_len=2 if lang == -1 else 3), lang=lang)
    return cfg, tk, steps, om, F.oracle_encodings(om, cfg)


@functools.lru_cache(maxsize=None)
def fixture_search(fx, K, b=0, name=NAME, lang=None):
    cfg, tk, steps, om, xas = fixture_model(fx, name, lang)
    prompt = [tk.sot, tk.transcribe] if lang == -1 else [tk.sot, tk.en, tk.transcribe]
    return beam_ref.search_ref(F.oracle_step(om, xas[b]), prompt, K, tk, cfg.max_target_positions - 1, max_new=len(steps))


@pytest.mark.parametrize("fx", sorted(F.FIXTURES))
def test_k1_reproduces_the_oracle_decode(fx):
    cfg, tk, steps, om, xas = fixture_model(fx)
    g = om.decode(xas[0], max_new_tokens=len(steps))
    r = fixture_search(fx, 1)
    assert r["tokens"] == g["tokens"]
    assert abs(r["avg_logprob"] - g["avg_logprob"]) < 2e-5     # the reference sums in fp64, the oracle in f32


@pytest.mark.parametrize("fx", sorted(F.FIXTURES))
def test_fixture_cut_gaps_are_at_least_G(fx):
    """Every case tests/test_gpu_beam.py decodes against the reference search: the three clips, K in 1, 2, 4, 5."""
    gaps = {(K, b): fixture_search(fx, K, b)["min_gap"] for K in KS for b in range(3)}
    print(fx, "cut gaps", gaps, "G", F.G)
    assert min(gaps.values()) >= F.G, gaps


@pytest.mark.parametrize("name,lang", [("test-d256-mel128", None), (NAME, -1)])
def test_fork_fixture_cut_gaps_on_the_other_configurations(name, lang):
    gaps = {b: fixture_search("fork", 2, b, name, lang)["min_gap"] for b in range(3)}
    print(name, lang, "cut gaps", gaps, "G", F.G)
    assert min(gaps.values()) >= F.G, gaps


def test_fork_fixture_beam_winner_differs_from_greedy():
    assert fixture_search("fork", 2)["tokens"] != fixture_search("fork", 1)["tokens"]
    assert fixture_search("fork", 2)["tokens"][-1] == common.tokens_for(NAME).eot


def test_closing_fixture_keeps_both_closing_timestamps_alive():
    cfg, tk, steps, om, xas = fixture_model("closing")
    r = fixture_search("closing", 4)
    Z = tk.zero_sec
    # the step after the fork: children of the T1 hypothesis (beam 0) and of the T2 hypothesis (beam 1) side by side; the
    # steered timestamp Z + 60 lies between them and is legal for T1 alone
    assert set(r["parents"][4]) >= {0, 1}
    assert any(t[3 + 3:3 + 5] == [Z + 40, Z + 60] for t, _ in r["finished"])
    assert not any(t[3 + 3:3 + 5] == [Z + 80, Z + 60] for t, _ in r["finished"])


def test_swap_fixture_parent_map_events():
    maps = [p for K in (4, 5) for p in fixture_search("swap", K)["parents"]]
    swap = any(any(p[i] == j and p[j] == i for i in range(len(p)) for j in range(i + 1, len(p))) for p in maps)
    fan = any(len(p) >= 2 and len(set(p)) < len(p) for p in maps)
    assert swap, maps
    assert fan, maps
