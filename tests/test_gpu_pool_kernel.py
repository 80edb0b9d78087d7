"""GPU: what a decode pool's token step launches after the logits -- pool_lang_detect_kernel, guard_kernel's pos / pfx gate,
pool_sample_step_kernel, logit_step_kernel's handled and pfx arms, pool_admit_kernel's pfx / pos0 / detect arms,
pool_retry_kernel (k_token.hip, k_guard.hip) -- and embed_ragged_kernel (k_elem.hip), called through tools/kref_pool.hip in the
order of emit_token_step and compared with the fp64 restatement in tests/pool_ref.py.

Every case runs twice: all K steps in one call (one stream, the tickets re-arming between launches), compared with the
reference's final state; and step by step, the state carried from call to call, compared with the reference after EVERY step.
A row is compared exactly -- tokens (the whole row: nothing beyond n_tokens may move), books, positions, flags, the guard's
logits bit for bit -- up to its first undecided step (kref.py, "token selection"), where either candidate is accepted and the
row is left alone from then on; sum_logprob, no_speech and the language probabilities stay within kref's bounds.  Rows
nobody may touch come back bit-identical through the same comparison: the reference leaves them as they were.  The tickets
are zero after every call.

Out of scope: NaN or infinities in the logits themselves (only the pad columns hold NaN), detection under a prefix (refused)."""
import collections
import functools

import numpy as np
import pytest

import kref as K
import pool_ref as PR

pytestmark = pytest.mark.gpu

LAYOUTS = K.token_layouts()
IDS = [l[0] for l in LAYOUTS]
EXACT = ("n_tokens", "done", "have_last", "last_ts", "pos", "pfx", "seed", "clip", "attempt", "handled", "detect_flag", "lang_out",
         "loop_exit")


def compare_row(c, b, got, want, bounds, what):
    """row b of the state `got` against the reference's row `want` (values of PR.ROW_KEYS); bounds: lp_bound, ns_bound, probs_bound"""
    assert np.array_equal(got["tokens"][b], want["tokens"][:c.ctx]), \
        f"{what}: tokens {got['tokens'][b].tolist()} != {np.asarray(want['tokens'][:c.ctx]).tolist()}"
    for k in EXACT:
        assert int(got[k][b]) == int(want[k]), f"{what}: {k} {got[k][b]} != {want[k]}"
    assert np.float32(got["inv_t"][b]).tobytes() == np.float32(want["inv_t"]).tobytes(), f"{what}: inv_t"
    lp, lr = float(got["sum_logprob"][b]), float(want["sum_logprob"])
    if np.isnan(lr):
        assert np.isnan(lp), f"{what}: sum_logprob {lp}, the reference's ln(-inf) is NaN"
    elif np.isfinite(bounds["lp_bound"]):
        assert abs(lp - lr) <= bounds["lp_bound"], f"{what}: sum_logprob {lp} vs {lr} (bound {bounds['lp_bound']})"
    assert abs(float(got["no_speech"][b]) - float(want["no_speech"])) <= bounds["ns_bound"], \
        f"{what}: no_speech {got['no_speech'][b]} vs {want['no_speech']} (bound {bounds['ns_bound']})"
    K.within(got["probs"][b], want["probs"], bounds["probs_bound"], f"{what}: language probabilities")


def compare_logits(c, b, k, got, ref, what):
    bad = np.nonzero(got["logits"][k, b].view(np.uint32) != ref["logits"][k, b].view(np.uint32))[0]
    assert bad.size == 0, f"{what}: logits of step {k} differ at {bad[:8].tolist()}: {got['logits'][k, b, bad[:8]].tolist()} " \
                          f"!= {ref['logits'][k, b, bad[:8]].tolist()}"


def lockstep_sample_row(c, before, k, b):
    """launch_sample_step (the lockstep kernel) on row b alone as it stood before step k, with the row's own sampling arguments"""
    lg = np.ascontiguousarray(before["logits"][k, b][None, None, :])
    row = {key: np.ascontiguousarray(before[key][b:b + 1]).copy() for key in ("tokens", "n_tokens", "done", "have_last", "last_ts",
                                                                             "sum_logprob", "no_speech")}
    sup = c.sup.astype(np.uint8)
    rc = K.lib().kref_sample_step(K.ptr(lg), 1, c.V, 1, c.ctx, c.cap, c.max_new, c.P + int(before["pfx"][b]), float(before["inv_t"][b]),
                                  int(before["seed"][b]), int(before["clip"][b]), int(before["attempt"][b]), K.ptr(c.tk), K.ptr(sup),
                                  K.ptr(row["tokens"]), K.ptr(row["n_tokens"]), K.ptr(row["done"]), K.ptr(row["have_last"]),
                                  K.ptr(row["last_ts"]), K.ptr(row["sum_logprob"]), K.ptr(row["no_speech"]))
    K.check_rc(rc, f"launch_sample_step {c.name} row {b} step {k}")
    return row


def check_case(c, ref, info, sample_identity=False):
    """both runs of the case against the reference.  Returns (final state of the one-call run, counters of what was compared)."""
    counts = dict(cells=collections.Counter(), sampled=collections.Counter(), detect=0, identical=0)
    # ---- all K steps in one call ----
    rc, full = PR.run(c)
    K.check_rc(rc, f"kref_pool_steps {c.name}")
    assert not full["tickets"].any(), f"{c.name}: tickets left armed {full['tickets']}"
    for b in range(c.B):
        what = f"{c.name} row {b} ({c.labels[b]}), one call"
        for k in range(min(info[b]["good"] + 1, c.K)):
            compare_logits(c, b, k, full, ref, what)
        if info[b]["good"] == c.K:
            compare_row(c, b, full, {key: ref[key][b] for key in PR.ROW_KEYS},
                        dict(lp_bound=info[b]["lp_bound"], ns_bound=info[b]["ns_bound"], probs_bound=ref["probs_bound"][b]), what)
    assert np.isnan(full["logits"][..., c.V:]).all(), f"{c.name}: pad columns written"
    # ---- step by step ----
    st = c.state()
    for k in range(c.K):
        before = {key: st[key].copy() for key in PR.STATE_KEYS} if sample_identity else None
        rc, st = PR.run(c, st, step=k)
        K.check_rc(rc, f"kref_pool_steps {c.name} step {k}")
        assert not st["tickets"].any(), f"{c.name} step {k}: tickets left armed {st['tickets']}"
        for b in range(c.B):
            i = info[b]
            what = f"{c.name} row {b} ({c.labels[b]}), after step {k}"
            if k <= i["good"]:
                compare_logits(c, b, k, st, ref, what)
            took = [s for s in i["steps"] if s[0] == k]
            if k < i["good"]:
                compare_row(c, b, st, i["snap"][k], i["snap"][k], what)
                for _, ph, s in took:
                    if k in i["sampled"]:
                        counts["sampled"][s.state] += 1
                counts["detect"] += sum(1 for d in i["detect"] if d["k"] == k)
            elif k == i["good"]:
                for _, ph, s in took:
                    if s is not None and not s.decided:
                        assert int(st["tokens"][b, i["slot"][k]]) in s.ok, f"{what}: {st['tokens'][b, i['slot'][k]]} not in {s.ok}"
            if sample_identity and st["handled"][b] == 1 and c.sampled[k]:
                # the kernel's comment: "the bits are the lockstep path's" -- whatever the margins say
                row = lockstep_sample_row(c, before, k, b)
                for key in row:
                    assert row[key].tobytes() == st[key][b:b + 1].tobytes(), f"{what}: {key} {st[key][b]} is not the lockstep kernel's {row[key][0]}"
                assert st["pos"][b] == before["pos"][b] + 1
                counts["identical"] += 1
    # a row counts once per cell
    cells = collections.Counter()
    for b in range(c.B):
        for ph in PR.PHASES:
            if any(s[1] == ph and s[0] < info[b]["good"] for s in info[b]["steps"]):
                cells[(ph, c.routes[b])] += 1
    counts["cells"] = cells
    return full, counts


@functools.lru_cache(maxsize=None)
def _section(lname, sec):
    """every case of one section on the GPU, once per process; [(case, final state, info, counts)]"""
    layout = [l for l in LAYOUTS if l[0] == lname][0]
    out = []
    for c, (ref, info) in zip(PR.cases(layout, sec), PR.refs(layout, sec)):
        full, counts = check_case(c, ref, info, sample_identity=sec in ("sampled", "retry"))
        out.append((c, full, info, counts))
    return out


@pytest.mark.parametrize("layout", LAYOUTS, ids=IDS)
def test_prefix_phases(layout):
    """n_prefix in {0, 1, 4, 17} and one that nearly fills ctx, consumed by the steps (pos0 = 0) or in one pass (pos0 =
    n_prefix), P in {2, 3}; rows admitted mid-run beside rows in other phases"""
    seen = collections.Counter()
    for c, full, info, _ in _section(layout[0], "phase"):
        seen.update(PR.phase_properties(c, full, info))
    print(f"\n{layout[0]}: rows {dict(seen)}")
    assert seen["ended"] >= 3 and seen["max_new"] >= 8 and seen["cap"] >= 1 and seen["prompt"] >= 1, dict(seen)


@pytest.mark.parametrize("layout", LAYOUTS, ids=IDS)
def test_sampled_rows_beside_greedy_rows(layout):
    """rows on a retry at generation positions, rows on a retry still at their probe or prompt position (served by the greedy
    kernel with handled == 0), greedy rows and finished rows in one pool; every sampled step bit-identical to the lockstep
    kernel's on the same one-row state"""
    n = 0
    for c, full, info, counts in _section(layout[0], "sampled"):
        n += counts["identical"]
        fin = [b for b in range(c.B) if c.labels[b].startswith("finished pfx")]
        assert len(fin) == 2
        for b in fin:                                    # finished rows with sampling arguments: bit-identical, pos included
            for key in PR.ROW_KEYS:
                if key != "handled":
                    assert full[key][b].tobytes() == getattr(c, key)[b].tobytes(), (c.name, b, key)
        served = [b for b in range(c.B) if c.labels[b].startswith("finished, retried")]
        assert served and all(full["no_speech"][b] != 0.0 for b in served), "a retried row's probe is the greedy kernel's"
    assert n >= 25, n


@pytest.mark.parametrize("layout", LAYOUTS, ids=IDS)
def test_retry_resets_the_row_behind_its_prefix(layout):
    n_reset = 0
    for c, full, info, counts in _section(layout[0], "retry"):
        for e in c.events:
            if e[0] != "retry" or e[1] != c.K:
                continue
            _, _, b, inv_t, seed, clip, attempt = e      # retried after the last step: what comes back is the reset itself
            n = c.npfx[b]
            assert (full["n_tokens"][b], full["pos"][b], full["done"][b], full["have_last"][b], full["last_ts"][b]) == (n + c.P, n, 0, 0, 0)
            assert full["sum_logprob"][b] == 0.0 and full["no_speech"][b] == 0.0 and full["detect_flag"][b] == 0 and full["pfx"][b] == n
            assert (float(full["inv_t"][b]), int(full["seed"][b]), int(full["clip"][b]), int(full["attempt"][b])) == (inv_t, seed, clip, attempt)
            assert np.array_equal(full["tokens"][b], c.tokens[b]), "a retry leaves every token where it is"
            n_reset += 1
        assert counts["identical"] >= 10, counts
    assert n_reset >= 3


@pytest.mark.parametrize("layout", LAYOUTS, ids=IDS)
def test_detection_in_the_step_at_position_zero(layout):
    """table sizes 1, 64, 65, 256; the token in slot 1, lang_out and probs of flagged rows at pos == 0 -- one of them ended by
    the probe in the same step --, an exact tie to the earlier index; canaries on every other row"""
    for c, full, info, _ in _section(layout[0], "detect"):
        PR.detect_properties(c, full, info)


@pytest.mark.parametrize("layout", LAYOUTS, ids=IDS)
def test_guard_gate_counts_the_prompt_from_behind_the_prefix(layout):
    """no-repeat n-gram with penalty, and the loop exit, with the n-gram and the loop inside the prefix ids"""
    for c, full, info, _ in _section(layout[0], "guard"):
        PR.guard_properties(c, full, info)
        edited = sum(len(i["guard"]) for i in info)
        assert edited >= 8, (c.name, edited)


@pytest.mark.parametrize("layout", LAYOUTS, ids=IDS)
def test_compared_steps_reach_the_counts(layout):
    """the counts tests/test_pool_ref_cpu.py derives from the reference, here over what was compared on the GPU"""
    cells, sampled, detect = collections.Counter(), collections.Counter(), 0
    for sec in PR.SECTIONS:
        for _, _, _, counts in _section(layout[0], sec):
            cells.update(counts["cells"])
            sampled.update(counts["sampled"])
            detect += counts["detect"]
    print(f"\n{layout[0]}: cells {dict(cells)}; sampled steps {dict(sampled)}; detections {detect}")
    assert (cells, sampled, detect) == PR.coverage(layout)
    PR.check_coverage(layout)


@pytest.mark.parametrize("layout", [l for l in LAYOUTS if l[0] in ("V2", "small")], ids=["V2", "small"])
def test_pool_steps_without_a_prefix_array(layout):
    """pfx == nullptr (a pool that never saw nh_pool_prefix): kref.sequence_cases' pool cases through the pool step"""
    n = 0
    for tc in K.sequence_cases(layout):
        if "/pool_" in tc.name:
            c = PR.from_token_case(tc)
            ref, info = PR.pool_step_ref(c)
            check_case(c, ref, info)
            n += sum(1 for i in info if i["good"] == c.K and i["steps"])
    assert n >= 8, n


def test_embed_ragged_matches_fp64():
    ec = PR.embed_ragged_case()
    ref, covered = PR.embed_ragged_ref(ec)
    rc, x = PR.run_embed_ragged(ec)
    K.check_rc(rc, "launch_embed_ragged")
    assert np.all(x[~covered] == 777.0), "rows no clip covers were written"
    bound = K.U32 * np.abs(ref) + 1e-300
    K.within(x[covered], ref[covered], bound[covered], "embed_ragged")
    K.discriminates(ref, bound, {m: PR.embed_ragged_ref(ec, m)[0] for m in ("table_row", "packed_pos")})


def _unchanged(before, after):
    return all(before[k].tobytes() == after[k].tobytes() for k in before)


def test_refusals_leave_every_output_untouched():
    small = [l for l in LAYOUTS if l[0] == "small"][0]
    c = PR.cases(small, "detect")[-1]                     # n = 256, rows with and without a prefix
    rc, _ = PR.run(c)
    assert rc == 0
    ev = c.event_table()

    def refused(what, st=None, events=None, n_lang=None):
        st = c.state() if st is None else st
        before = {k: v.copy() for k, v in st.items()}
        cc = c
        if n_lang is not None:
            import copy
            cc = copy.copy(c)
            cc.n_lang = n_lang
        rc, after = PR.run(cc, st, events=events)
        assert rc == -1, f"{what}: returned {rc}"
        assert _unchanged(before, after), f"{what}: refused, yet something was written"

    for row in (-1, c.B):
        e = ev.copy(); e[0, 2] = row
        refused(f"an event on row {row}", events=e)
    e = ev.copy(); e[0, 7] = e[0, 8] = c.cap - c.P; e[0, 6] = 0
    refused("n_prefix + P == cap", events=e)
    e = ev.copy()
    i = int(np.argmax(e[:, 6] == 1))
    e[i, 7] = 4
    refused("detection under a prefix", events=e)
    st = c.state()
    b = int(np.argmax(st["done"] == 0))
    st["n_tokens"][b] = c.cap
    refused("a live row with n_tokens == cap", st=st)
    st = c.state()
    st["tokens"][c.B - 1, c.ctx - 1] = c.V
    refused("a token id outside the vocabulary", st=st)
    e = ev.copy(); e[0, 8] = 1
    refused("pos0 neither 0 nor n_prefix", events=e)
    e = ev.copy(); e[0, 0] = c.K
    refused("events out of order", events=e)
    e = ev.copy(); e[0, 1] = 2
    refused("an event of no kind", events=e)
    refused("an empty language table", n_lang=0)
    refused("a language table of 257", n_lang=257)
    # the ragged embedding: a token row outside the buffer, rows past x, overlapping clips
    ec = PR.embed_ragged_case()
    for what, z, col, val in (("token row", 0, 0, ec["tokens"].shape[0]), ("rows past x", 1, 2, ec["m_rows"] - 1),
                              ("T beyond the positions", 2, 1, ec["n_pos"] + 1), ("overlap", 3, 2, int(ec["clips"][4, 2]))):
        clips = ec["clips"].copy()
        clips[z, col] = val
        rc, x = PR.run_embed_ragged(ec, clips=clips)
        assert rc == -1 and np.all(x == 777.0), what
    ec["tokens"] = ec["tokens"].copy()
    ec["tokens"][ec["clips"][0, 0], 0] = ec["V"]
    rc, x = PR.run_embed_ragged(ec)
    assert rc == -1 and np.all(x == 777.0), "a token id outside the table"
