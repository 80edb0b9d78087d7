"""GPU: the token-selection kernels of k_token.hip -- logit_step_kernel (greedy step, no-speech probe, decode-pool phases),
pool_admit_kernel, sample_step_kernel, lang_detect_kernel -- called through tools/kref.hip and compared with the fp64
restatement of model.rs:212-277, 293-370 in tests/kref.py.

Tokens are discrete, so each step carries a margin derived from the kernel's arithmetic (kref.py, "token selection"): on a
decided step the kernel must produce exactly the reference's token and bookkeeping; an undecided step accepts either candidate
(and a multi-launch row with one is not compared further).  Log-probabilities, no_speech and the language probabilities are
compared within derived bounds.  Done rows must come back bit-identical, and the tickets must be zero after every run.

Out of scope: NaN or +-inf inside the logits themselves (the product's logits come from a finite GEMV); only the pad columns
V..ldl-1 hold NaN here, and the kernels must never read them."""
import collections

import numpy as np
import pytest

import kref as K

pytestmark = pytest.mark.gpu

LAYOUTS = K.token_layouts()
COUNTS = collections.Counter()


def run_logit_step(c, logits=None):
    L = K.lib()
    st = c.state()
    pos = st["pos"]
    tickets = np.zeros(c.B, np.uint32)
    partials = np.zeros((c.B, 64), np.float32)
    lg = np.ascontiguousarray(c.logits if logits is None else logits, dtype=np.float32)
    sup = c.sup.astype(np.uint8)                  # held: a temporary's buffer would be freed before the call
    rc = L.kref_logit_step(K.ptr(lg), c.K, c.V, c.B, c.ctx, c.cap, c.max_new, c.prompt_len, K.ptr(c.modes), K.ptr(c.use_pos),
                           K.ptr(c.tk), K.ptr(sup), K.ptr(st["tokens"]), K.ptr(st["n_tokens"]),
                           K.ptr(st["done"]), K.ptr(st["have_last"]), K.ptr(st["last_ts"]), K.ptr(st["sum_logprob"]),
                           K.ptr(st["no_speech"]), K.ptr(pos), K.ptr(c.admits if len(c.admits) else None), len(c.admits),
                           K.ptr(tickets), K.ptr(partials))
    K.check_rc(rc, f"launch_logit_step {c.name}")
    assert not tickets.any(), f"{c.name}: tickets left armed {tickets}"
    return st


def run_sample_step(c):
    L = K.lib()
    st = c.state()
    lg, sup = np.ascontiguousarray(c.logits, dtype=np.float32), c.sup.astype(np.uint8)
    rc = L.kref_sample_step(K.ptr(lg), c.K, c.V, c.B, c.ctx, c.cap, c.max_new, c.prompt_len,
                            c.inv_t, c.seed, c.clip0, c.attempt, K.ptr(c.tk), K.ptr(sup),
                            K.ptr(st["tokens"]), K.ptr(st["n_tokens"]), K.ptr(st["done"]), K.ptr(st["have_last"]),
                            K.ptr(st["last_ts"]), K.ptr(st["sum_logprob"]), K.ptr(st["no_speech"]))
    K.check_rc(rc, f"launch_sample_step {c.name}")
    return st


def _idle(c, b):
    return bool(c.done[b]) and not any(a[1] == b for a in c.admits)


def compare(c, got, ref, info, counted=True):
    """exact state on decided rows, acceptable tokens on undecided single steps, bounds on the continuous outputs"""
    init = c.state()
    for b in range(c.B):
        what = f"{c.name} row {b} ({c.labels[b]})"
        if _idle(c, b):                       # a done row is left exactly as it was, pos included
            for k in ("tokens", "n_tokens", "done", "have_last", "last_ts", "pos"):
                if init[k] is not None:
                    assert np.array_equal(got[k][b], init[k][b]), f"{what}: done row's {k} touched"
            for k in ("sum_logprob", "no_speech"):
                assert got[k][b].tobytes() == init[k][b].tobytes(), f"{what}: done row's {k} touched"
            continue
        steps = info[b]["steps"]
        if counted:
            for s in steps:
                COUNTS[(c.name.split("/")[0], s.state, s.decided)] += 1
        if not info[b]["decided"]:
            if len(steps) == 1:
                n0 = int(init["n_tokens"][b])
                assert int(got["tokens"][b, n0]) in steps[0].ok, f"{what}: {got['tokens'][b, n0]} not in {steps[0].ok}"
            continue
        n = int(ref["n_tokens"][b])
        assert int(got["n_tokens"][b]) == n, f"{what}: n_tokens {got['n_tokens'][b]} != {n}"
        assert np.array_equal(got["tokens"][b, :n], ref["tokens"][b, :n]), \
            f"{what}: tokens {got['tokens'][b, :n].tolist()} != {ref['tokens'][b, :n].tolist()}"
        for k in ("done", "have_last", "last_ts"):
            if k == "done" and not info[b].get("ns_decided", True):
                continue
            assert int(got[k][b]) == int(ref[k][b]), f"{what}: {k} {got[k][b]} != {ref[k][b]}"
        if ref["pos"] is not None and got["pos"] is not None:
            assert int(got["pos"][b]) == int(ref["pos"][b]), f"{what}: pos {got['pos'][b]} != {ref['pos'][b]}"
        lp, lr = got["sum_logprob"][b], ref["sum_logprob"][b]
        if np.isnan(lr):
            assert np.isnan(lp), f"{what}: sum_logprob {lp}, the reference's ln(-inf) is NaN"
        elif np.isfinite(info[b]["lp_bound"]):
            assert abs(lp - lr) <= info[b]["lp_bound"], f"{what}: sum_logprob {lp} vs {lr} (bound {info[b]['lp_bound']})"
        if "ns_bound" in info[b] and ref["no_speech"][b] != 0:
            assert abs(got["no_speech"][b] - ref["no_speech"][b]) <= info[b]["ns_bound"], \
                f"{what}: no_speech {got['no_speech'][b]} vs {ref['no_speech'][b]}"


@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_logit_step_matches_the_fp64_rules_in_every_state(layout):
    cases = K.greedy_cases(layout)
    for c in cases:
        for cc in [c] + ([c.extra] if c.extra is not None else []):
            ref, info = K.logit_step_ref(cc)
            compare(cc, run_logit_step(cc), ref, info)
    name = layout[0]
    got = {s: COUNTS[(name, s, True)] for s in K.RULE_STATES}
    print(f"\n{name}: decided steps per rule state {got}; undecided "
          f"{ {s: COUNTS[(name, s, False)] for s in K.RULE_STATES} }")
    for s in K.RULE_STATES:
        assert got[s] >= 20, f"{name}: only {got[s]} decided cases in state {s}"


@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_logit_step_sequences_pool_phases_and_probe(layout):
    """K = 24 launches on one state (cap, eot, max_new; the tickets re-arm themselves), the decode pool in mode 2 with rows
    admitted by launch_pool_admit in mixed phases (P = 2, 3), and the no-speech probe"""
    decided = collections.Counter()
    for c in K.sequence_cases(layout):
        ref, info = K.logit_step_ref(c)
        got = run_logit_step(c)
        compare(c, got, ref, info, counted=False)
        kind = c.name.split("/")[1].split("_")[0]
        decided[kind] += sum(1 for b in range(c.B) if not _idle(c, b) and info[b]["decided"] and info[b]["ns_decided"])
        if kind == "probe":
            assert np.array_equal(got["n_tokens"], c.n_tokens), "the probe adds no token"
            live = ~c.done.astype(bool)
            assert np.array_equal(got["pos"][live], np.ones(live.sum(), np.int32)), "the probe advances pos once"
        if kind == "seq":
            fin = got["done"][~c.done.astype(bool)]
            assert fin.any(), f"{c.name}: no row finished in {c.K} launches"
    print(f"\n{layout[0]}: decided rows {dict(decided)}")
    assert decided["seq"] >= 12 and decided["pool"] >= 8 and decided["probe"] >= 40, dict(decided)


@pytest.mark.parametrize("layout", LAYOUTS[2:4], ids=[l[0] for l in LAYOUTS[2:4]])
def test_logit_step_never_reads_the_pad_columns(layout):
    c = K.greedy_cases(layout)[1]
    assert K.ldl_of(c.V) > c.V or c.V == K.NH_MAX_VOCAB
    nan = run_logit_step(c)
    zero = c.logits.copy()
    zero[..., c.V:] = 0.0
    z = run_logit_step(c, zero)
    big = c.logits.copy()
    big[..., c.V:] = 1e30
    g = run_logit_step(c, big)
    for k in nan:
        if nan[k] is not None:
            assert nan[k].tobytes() == z[k].tobytes() == g[k].tobytes(), k


@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_sample_step_matches_the_fp64_cdf_draw(layout):
    decided = collections.Counter()
    for c in K.sample_cases(layout):
        ref, info = K.sample_step_ref(c)
        got = run_sample_step(c)
        compare(c, got, ref, info, counted=False)
        for b in range(c.B):
            if _idle(c, b):
                continue
            for s in info[b]["steps"]:
                decided[(s.state, s.decided)] += 1
        b = c.labels.index("NON_TS@all_masked")     # everything masked: eot pushed, done, sum_logprob unchanged
        n0 = int(c.n_tokens[b])
        assert got["done"][b] == 1 and got["n_tokens"][b] == n0 + 1 and got["tokens"][b, n0] == c.tk[1]
        assert got["sum_logprob"][b] == 0.0
    print(f"\n{layout[0]}: sampled steps {dict(decided)}")
    for s in K.RULE_STATES:
        assert decided[(s, True)] >= 5, (s, dict(decided))


@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_lang_detect_takes_the_first_maximum(layout):
    name, V, tk, _ = layout
    rng = np.random.default_rng(K.zlib_key(name, "lang"))
    L = K.lib()
    ndec = 0
    for n in (1, 99, 100, 256):
        base = np.arange(tk.en, tk.en + n) if n <= 100 else rng.choice(V, n, replace=False)
        lt = rng.permutation(base).astype(np.int32)
        B = 7
        lg = np.full((B, K.ldl_of(V)), np.nan, np.float32)
        lg[:, :V] = rng.standard_normal((B, V)) * 2
        if n > 1:
            lg[1, lt[n // 2]] = lg[1, lt[n - 1]] = lg[1, lt].max() + 1    # an exact tie: the earlier index wins
            lg[2, lt] = 0.0                                                   # flat: the first language
        probs = np.zeros((B, n), np.float32)
        out = np.zeros(B, np.int32)
        K.check_rc(L.kref_lang_detect(K.ptr(lg), V, B, K.ptr(lt), n, K.ptr(probs), K.ptr(out)), f"lang_detect n={n}")
        for b in range(B):
            p, pb, w, ok, dec = K.lang_ref(lg[b, :V], lt)
            K.within(probs[b], p, pb + 1e-300, f"{name} n={n} row {b} language probabilities")
            assert int(out[b]) in ok, (name, n, b, int(out[b]), ok)
            if dec:
                ndec += 1
                assert int(out[b]) == w
        if n > 1:
            assert out[1] == lt[n // 2] and out[2] == lt[0]
    assert ndec >= 24, ndec
