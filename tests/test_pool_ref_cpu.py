"""CPU checks of tests/pool_ref.py, the fp64 reference of a decode pool's token step: it agrees with kref.logit_step_ref where
the two overlap, every plausible bug of the phase logic changes a decided outcome of the GPU suite's own cases, the cases
reach what the suite claims to cover (counted from the reference alone).  That the wrapper library builds is checked in tests/test_kref_cpu.py."""
import numpy as np
import pytest

import kref as K
import pool_ref as PR

LAYOUTS = K.token_layouts()
SMALL = [l for l in LAYOUTS if l[0] == "small"][0]


@pytest.mark.parametrize("layout", [l for l in LAYOUTS if l[0] in ("V2", "small")], ids=["V2", "small"])
def test_pool_reference_equals_the_logit_step_reference_on_its_pool_cases(layout):
    """no prefix, no sampling, no detection, no guard: pool_step_ref is logit_step_ref, exactly"""
    n = 0
    for tc in K.sequence_cases(layout):
        if "/pool_" not in tc.name:
            continue
        want, winfo = K.logit_step_ref(tc)
        got, ginfo = PR.pool_step_ref(PR.from_token_case(tc))
        for key in ("tokens", "n_tokens", "done", "have_last", "last_ts", "pos"):
            assert np.array_equal(got[key], want[key]), (tc.name, key)
        for key in ("sum_logprob", "no_speech"):
            assert got[key].tobytes() == want[key].tobytes(), (tc.name, key)
        for b in range(tc.B):
            for key in ("decided", "ns_decided", "lp_bound", "ns_bound"):
                assert ginfo[b][key] == winfo[b][key], (tc.name, b, key)
            assert [s.next for s in winfo[b]["steps"]] == [s[2].next for s in ginfo[b]["steps"] if s[1] == "generate"]
        n += 1
    assert n == 2


def _outcome(c, st, b):
    return (st["tokens"][b, :c.ctx].tobytes(), int(st["n_tokens"][b]), int(st["done"][b]), int(st["have_last"][b]), int(st["last_ts"][b]),
            int(st["pos"][b]), int(st["lang_out"][b]), int(st["loop_exit"][b]), int(st["detect_flag"][b]),
            st["logits"][:, b, :c.V].tobytes())


def test_pool_mutations_change_a_decided_outcome_of_the_suite():
    """each plausible bug of PR.MUTATIONS, applied to the reference, changes the outcome of at least one decided row of the
    cases tests/test_gpu_pool_kernel.py runs, so a kernel with that bug fails the suite.  sum_logprob counts as changed when
    it moves by more than twice the row's bound."""
    caught = {m: [] for m in PR.MUTATIONS}
    for sec in PR.SECTIONS:
        for c, (ref, info) in zip(PR.cases(SMALL, sec), PR.refs(SMALL, sec)):
            for m in PR.MUTATIONS:
                mst, _ = PR.pool_step_ref(c, mut=(m,))
                for b in range(c.B):
                    if not PR.row_decided(info[b]):
                        continue
                    dlp = abs(mst["sum_logprob"][b] - ref["sum_logprob"][b])
                    if _outcome(c, ref, b) != _outcome(c, mst, b) or dlp > 2 * info[b]["lp_bound"] + 1e-9:
                        caught[m].append((c.name, b))
    print("mutations caught (decided rows changed):", {m: len(v) for m, v in caught.items()})
    missed = [m for m, v in caught.items() if not v]
    assert not missed, f"no decided row of the suite distinguishes {missed}"
    # each where it belongs: the sections exist for these bugs
    assert any("/guard_ngram" in n for n, _ in caught["guard_hist_pfx"]) and any("/guard_loop" in n for n, _ in caught["guard_hist_pfx"])
    assert any("/detect_" in n for n, _ in caught["detect_any_pos"]) and any("/detect_" in n for n, _ in caught["detect_slot0"])
    assert any("/retry_" in n for n, _ in caught["retry_pos0"]) and any("/retry_" in n for n, _ in caught["retry_keeps_lp"])
    assert any("/sampled_" in n for n, _ in caught["handled_ignored"]) and any("/sampled_" in n for n, _ in caught["sampler_in_prompt"])
    assert any("/phase_" in n for n, _ in caught["probe_at_0"]) and any("/phase_" in n for n, _ in caught["phase_no_pfx"])
    assert any("/phase_" in n for n, _ in caught["max_new_pfx"])


@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_pool_cases_reach_what_the_suite_covers(layout):
    """conditions on the cases, from the reference alone: >= 8 rows in every (phase, prefix route) cell, >= 5 sampled steps in
    every rule state, >= 24 detections -- counted over the steps the GPU test compares exactly (before a row's first undecided
    one) -- and what each section is about holds on the reference's own final state"""
    cells, sampled, detect = PR.check_coverage(layout)
    print(f"\n{layout[0]}: cells {dict(cells)}; sampled steps {dict(sampled)}; detections {detect}")
    seen = {}
    for c, (st, info) in zip(PR.cases(layout, "phase"), PR.refs(layout, "phase")):
        for k, v in PR.phase_properties(c, st, info).items():
            seen[k] = seen.get(k, 0) + v
    assert seen["ended"] >= 3 and seen["max_new"] >= 8 and seen["cap"] >= 1 and seen["prompt"] >= 1, seen
    for c, (st, info) in zip(PR.cases(layout, "detect"), PR.refs(layout, "detect")):
        PR.detect_properties(c, st, info)
    for c, (st, info) in zip(PR.cases(layout, "guard"), PR.refs(layout, "guard")):
        PR.guard_properties(c, st, info)
    for sec in PR.SECTIONS:
        for c in PR.cases(layout, sec):
            assert c.B <= 16 and c.K <= 24 and np.isnan(c.logits[..., c.V:]).all()
    # retried rows sample with the physical token count and probe again behind their prefix
    n_retry = 0
    for c, (st, info) in zip(PR.cases(layout, "retry"), PR.refs(layout, "retry")):
        for e in c.events:
            if e[0] != "retry" or e[1] >= c.K - c.P:
                continue
            b, k = e[2], e[1]
            steps = [s for s in info[b]["steps"] if s[0] >= k]
            assert steps[0][:2] == (k, "probe") and steps[c.P - 1][:2] == (k + c.P - 1, "generate") and k + c.P - 1 in info[b]["sampled"]
            n_retry += 1
    assert n_retry >= 6, n_retry


def test_embed_ragged_reference_and_its_mutations():
    ec = PR.embed_ragged_case()
    ref, covered = PR.embed_ragged_ref(ec)
    assert sorted(int(c[1]) for c in ec["clips"]) == sorted(PR.EMBED_T) and covered.sum() == sum(PR.EMBED_T)
    assert not covered[-1] and np.all(ref[~covered] == 777.0)
    toks = np.concatenate([ec["tokens"][r, :T] for r, T, _, _ in ec["clips"]])
    assert 0 in toks and ec["V"] - 1 in toks
    z = int(np.argmax(ec["clips"][:, 1] == 17))
    row, T, off, _ = ec["clips"][z]
    assert np.array_equal(ref[off + 5], K.d64(ec["E"])[ec["tokens"][row, 5]] + K.d64(ec["P"])[5])
    bound = K.U32 * np.abs(ref) + 1e-300
    K.discriminates(ref, bound, {m: PR.embed_ragged_ref(ec, m)[0] for m in ("table_row", "packed_pos")})
