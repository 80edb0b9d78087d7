"""fp64 reference of what a decode pool's token step launches after the logits (emit_token_step, norma_amd/csrc/nh_decode.hip):
launch_pool_lang_detect, launch_guard(pos, pfx), launch_pool_sample_step, launch_logit_step(mode 2, handled, pfx), with
launch_pool_admit and launch_pool_retry around them; the loader of tools/bin/libnh_kref_pool.so (tools/kref_pool.hip); and the
cases tests/test_gpu_pool_kernel.py runs and tests/test_pool_ref_cpu.py counts.

pool_step_ref generalises kref.logit_step_ref per step and per row, in stream order.  Nothing numeric is new here: a greedy
token is kref.step_ref under PATHS["logit_step"], a sampled one kref.sample_ref under kref.sample_path, a language
kref.lang_ref under PATHS["lang"], and the guard's edit is guard_ref.edit, bit for bit.  What this file adds is the phase
logic: who acts on a row in a step, at which position, counted from where.

A logit the guard set to -inf enters the fp64 softmax as (row maximum - 200): its f32 mass is exactly 0 and its fp64 mass is
below 1e-86, so it can neither win nor move a sum by an ulp, and the margins of kref.step_ref stay finite."""
import ctypes as C
import functools
import os

import numpy as np

import guard_ref as G
import kref as K

LIB_PATH = os.path.join(K.ROOT, "tools", "bin", "libnh_kref_pool.so")
WRAPPERS = ["kref_pool_steps", "kref_embed_ragged"]
EV_ADMIT, EV_RETRY = 0, 1
PHASES = ("probe", "prompt", "generate")
ROUTES = ("none", "stepwise", "onepass")
# plausible bugs of the phase logic; each changes a decided outcome of the suite's own cases (tests/test_pool_ref_cpu.py)
MUTATIONS = ("probe_at_0", "phase_no_pfx", "max_new_pfx", "sampler_in_prompt", "handled_ignored", "retry_pos0", "retry_keeps_lp",
             "detect_any_pos", "detect_slot0", "guard_hist_pfx", "guard_in_prompt", "step_no_pfx")
_lib = None


def lib():
    """The wrapper library; a GPU run without it FAILS (pytest.fail): a vacuous pass is not a pass."""
    global _lib
    if _lib is None:
        import pytest
        if not os.path.exists(LIB_PATH):
            pytest.fail(f"{LIB_PATH} is not built (python -c 'import __graft_entry__ as g; g.build()')")
        L = C.CDLL(LIB_PATH)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        L.kref_pool_steps.argtypes = [vp, i, i, i, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, vp, vp, vp, vp, vp, vp, vp,
                                      vp, vp, i, vp, i, vp, vp, vp, i, i, f, i, i, vp]
        L.kref_embed_ragged.argtypes = [vp, i, i, vp, i, vp, i, vp, i, vp, i, i]
        for n in WRAPPERS:
            getattr(L, n).restype = C.c_int
        _lib = L
    return _lib


# ---- a case --------------------------------------------------------------------------------------------------------------
STATE_KEYS = ("logits", "tokens", "n_tokens", "done", "have_last", "last_ts", "sum_logprob", "no_speech", "pos", "pfx", "tickets",
              "partials", "inv_t", "seed", "clip", "attempt", "handled", "detect_flag", "lang_out", "probs", "loop_exit")


class PoolCase:
    """K pool steps on one state of B rows.  logits f32 [K][B][ldl] (pad columns NaN); events: ("admit", k, row, t0, t1, t2,
    detect, n_prefix, pos0) and ("retry", k, row, inv_t, seed, clip, attempt), k ascending, applied ahead of step k (k = K:
    after the last); sampled i32 [K]; lang_tokens i32 [n] or None; guard: guard_ref.params() or None.  routes[b]: how the
    row's prefix is consumed ("none", "stepwise", "onepass"), for the coverage counts only."""

    def __init__(self, name, layout, B, K_, ctx, P, max_new=0, use_pfx=True):
        self.name, self.layout = name, layout
        self.lname, self.V, self.tko, sl = layout
        self.tk = K.tk_array(self.tko)
        self.sup = K.sup_array(self.V, sl, self.tko.no_timestamps).astype(bool)
        self.B, self.K, self.ctx, self.cap, self.P, self.max_new, self.use_pfx = B, K_, ctx, ctx - 1, P, max_new, use_pfx
        ldl = K.ldl_of(self.V)
        self.logits = np.full((K_, B, ldl), np.nan, np.float32)
        self.tokens = np.full((B, ctx), 7, np.int32)            # 7: a canary id no case generates on purpose
        self.n_tokens = np.full(B, P, np.int32)
        self.done = np.ones(B, np.int32)
        self.have_last = np.zeros(B, np.int32)
        self.last_ts = np.zeros(B, np.int32)
        self.sum_logprob = np.zeros(B)
        self.no_speech = np.zeros(B)
        self.pos = np.zeros(B, np.int32)
        self.pfx = np.zeros(B, np.int32)
        self.tickets = np.zeros(B, np.uint32)
        self.partials = np.zeros((B, 64), np.float32)
        self.inv_t = np.zeros(B, np.float32)
        self.seed = np.zeros(B, np.uint64)
        self.clip = np.zeros(B, np.uint32)
        self.attempt = np.zeros(B, np.uint32)
        self.handled = np.full(B, -3, np.int32)
        self.sampled = np.zeros(K_, np.int32)
        self.events = []
        self.lang_tokens = None
        self.detect_flag = np.zeros(B, np.int32)
        self.lang_out = np.full(B, -7, np.int32)
        self.probs = np.full((B, 256), 123.0, np.float32)
        self.guard = None
        self.loop_exit = np.zeros(B, np.int32)
        self.labels = ["idle"] * B
        self.routes = ["none"] * B

    def state(self):
        return {k: getattr(self, k).copy() for k in STATE_KEYS}

    def event_table(self):
        ev = np.zeros((len(self.events), 9), np.int32)
        for i, e in enumerate(self.events):
            if e[0] == "admit":
                ev[i] = [e[1], EV_ADMIT] + list(e[2:])
            else:
                _, k, row, inv_t, seed, clip, attempt = e
                ev[i, :3] = [k, EV_RETRY, row]
                ev[i, 3:4].view(np.float32)[0] = inv_t
                ev[i, 4:6].view(np.uint32)[:] = [seed & 0xFFFFFFFF, seed >> 32]
                ev[i, 6:8].view(np.uint32)[:] = [clip, attempt]
        return ev


def run(c, st=None, step=None, events=None):
    """kref_pool_steps on the case, or on the state `st` of it; step = k: step k alone, with the events ahead of it, on
    st["logits"][k] (what the guard edits lands there); events: another table.  Returns (rc, state)."""
    L = lib()
    st = c.state() if st is None else st
    ev = c.event_table() if events is None else events
    K_, logits, sampled = c.K, st["logits"], c.sampled
    if step is not None:
        ev = np.ascontiguousarray(ev[ev[:, 0] == step])
        ev[:, 0] = 0
        K_, logits, sampled = 1, st["logits"][step:step + 1], np.ascontiguousarray(c.sampled[step:step + 1])
    sup = c.sup.astype(np.uint8)
    g = c.guard
    lt = None if c.lang_tokens is None else np.ascontiguousarray(c.lang_tokens, np.int32)
    rc = L.kref_pool_steps(K.ptr(logits), K_, c.V, c.B, c.ctx, c.cap, c.max_new, c.P, K.ptr(c.tk), K.ptr(sup), K.ptr(st["tokens"]),
                           K.ptr(st["n_tokens"]), K.ptr(st["done"]), K.ptr(st["have_last"]), K.ptr(st["last_ts"]), K.ptr(st["sum_logprob"]),
                           K.ptr(st["no_speech"]), K.ptr(st["pos"]), K.ptr(st["pfx"]), int(c.use_pfx), K.ptr(st["tickets"]),
                           K.ptr(st["partials"]), K.ptr(st["inv_t"]), K.ptr(st["seed"]), K.ptr(st["clip"]), K.ptr(st["attempt"]),
                           K.ptr(st["handled"]), K.ptr(sampled), K.ptr(ev if len(ev) else None), len(ev), K.ptr(lt),
                           0 if lt is None else getattr(c, "n_lang", len(lt)), K.ptr(st["detect_flag"]), K.ptr(st["lang_out"]), K.ptr(st["probs"]),
                           int(g is not None), g.no_repeat_ngram if g else 0, float(g.repetition_penalty) if g else 1.0,
                           g.loop_period if g else 0, g.loop_repeats if g else 0, K.ptr(st["loop_exit"]))
    return rc, st


# ---- the reference ---------------------------------------------------------------------------------------------------------
def _finite(l):
    """f32 logits for kref.step_ref: the guard's -inf as (maximum - 200), see the module's docstring"""
    if np.isfinite(l).all():
        return l
    out = l.copy()
    out[np.isneginf(l)] = np.float32(l[np.isfinite(l)].max() - 200.0)
    return out


def _sample_row(c, st, k, b, l, PL, mut, info):
    """one row of pool_sample_step_kernel: kref.sample_step_ref's body with the row's own seed, clip, attempt and inv_t"""
    path = K.sample_path(c.V)
    tk = c.tk
    n = int(st["n_tokens"][b])
    info["slot"][k] = n
    t = 1.0 / float(st["inv_t"][b])
    lf = _finite(l)
    s = K.step_ref(lf, list(st["tokens"][b, :n]), int(st["have_last"][b]), int(st["last_ts"][b]), c.sup, tk, path)
    p, x = s.p, K.softmax64(lf)[1]
    allowed = K._allowed_final(s.state, c.V, c.sup, tk, int(st["last_ts"][b]), (), int(tk[5]))
    q = np.where(allowed, p, -np.inf)
    rel = K._rel(K._eps_se(p, x, path, c.V), x)
    step = n - (int(st["pfx"][b]) if c.use_pfx and "step_no_pfx" in mut else 0)
    u = K._philox_u(int(st["seed"][b]), int(st["clip"][b]), step, int(st["attempt"][b]))
    j, ok, dec = K.sample_ref(q, rel, t, u)
    s.ok = ok if s.decided else (s.ok | ok)
    s.decided = s.decided and dec
    info["decided"] &= s.decided
    if j < 0:
        st["tokens"][b, n] = tk[1]; st["n_tokens"][b] = n + 1; st["done"][b] = 1
        s.next = -1
        return s
    s.next = j
    info["lp_bound"] += rel[j] + 2.0 ** -50 if x[j] > -80 else np.inf
    K._bookkeep(st, b, j, np.log(p[j]), tk, c.cap, c.max_new, PL, ())
    return s


def pool_step_ref(c, mut=(), upto=None):
    """the reference of the case's K steps (of its first `upto`, with the events ahead of them).  Returns (state, info):
    info[b] = dict(decided, ns_decided, lp_bound, ns_bound, steps = [(k, phase, Step | None)], sampled = [k of every sampled
    step], detect = [dict(k, ok, decided, p, bound, w)], guard = [k of every edit], good = the steps the row went through
    before its first undecided one (K: all), slot = {k: the slot step k's token went to}, snap = [after step k: the row's ROW_KEYS, the bounds so far])"""
    st = c.state()
    B, V, P, tk = c.B, c.V, c.P, c.tk
    st["tokens"] = np.concatenate([st["tokens"], np.zeros((B, 2 * c.K + 4), np.int32)], axis=1)   # room for a mutant's overrun
    st["probs"] = st["probs"].astype(np.float64)
    st["probs_bound"] = np.zeros((B, 256))
    info = [dict(decided=True, ns_decided=True, lp_bound=0.0, ns_bound=0.0, steps=[], sampled=[], detect=[], guard=[], good=c.K, snap=[], slot={})
            for _ in range(B)]
    path = K.PATHS["logit_step"]
    Kn = c.K if upto is None else upto
    nl = 0 if c.lang_tokens is None else len(c.lang_tokens)

    def npfx(b):
        return int(st["pfx"][b]) if c.use_pfx else 0

    for k in range(Kn + 1):
        for e in [e for e in c.events if e[1] == k]:
            row = e[2]
            if e[0] == "admit":                                                        # pool_admit_kernel
                _, _, _, t0, t1, t2, detect, n_prefix, pos0 = e
                st["tokens"][row, n_prefix:n_prefix + P] = [t0, t1, t2][:P]
                n0, p0 = n_prefix + P, pos0
                st["detect_flag"][row] = detect
                if c.use_pfx:
                    st["pfx"][row] = n_prefix
            else:                                                                      # pool_retry_kernel
                _, _, _, inv_t, seed, clip, attempt = e
                n0 = npfx(row) + P
                p0 = 0 if "retry_pos0" in mut else npfx(row)
                st["inv_t"][row], st["seed"][row], st["clip"][row], st["attempt"][row] = inv_t, seed, clip, attempt
                st["detect_flag"][row] = 0
            st["n_tokens"][row], st["done"][row], st["have_last"][row], st["last_ts"][row] = n0, 0, 0, 0
            if not (e[0] == "retry" and "retry_keeps_lp" in mut):
                st["sum_logprob"][row] = 0.0
            st["no_speech"][row] = 0.0
            st["pos"][row] = p0
            st["tickets"][row] = 0
        if k == Kn:
            break
        for b in range(B):
            l = st["logits"][k, b, :V]                                                 # a view: the guard's edit lands in the state
            PL = P + npfx(b)
            # ---- pool_lang_detect_kernel ----
            if nl and st["detect_flag"][b] and not st["done"][b] and (st["pos"][b] == 0 or "detect_any_pos" in mut):
                p, pb, w, ok, dec = K.lang_ref(l, c.lang_tokens)
                st["tokens"][b, 0 if "detect_slot0" in mut else 1] = w
                st["lang_out"][b] = w
                st["probs"][b, :nl], st["probs_bound"][b, :nl] = p, pb
                info[b]["detect"].append(dict(k=k, ok=ok, decided=dec, p=p, bound=pb, w=w))
                info[b]["decided"] &= dec
            # ---- guard_kernel ----
            if c.guard is not None and not st["done"][b]:
                hist_pl = P if "guard_hist_pfx" in mut else PL
                n = int(st["n_tokens"][b])
                if (st["pos"][b] >= PL - 1 or "guard_in_prompt" in mut) and n >= hist_pl:
                    if n == hist_pl:
                        st["loop_exit"][b] = 0
                    if not mut:
                        assert bool(st["have_last"][b]) == G.have_last(st["tokens"][b], n, PL, c.tko), "the case's state is not a decode's"
                    x, ex = G.edit(l, st["tokens"][b], n, hist_pl, c.guard, None, c.tko)
                    l[:] = x
                    if ex:
                        st["loop_exit"][b] = 1
                    info[b]["guard"].append(k)
            # ---- pool_sample_step_kernel ----
            taken = 0
            if c.sampled[k]:
                mine = bool(st["inv_t"][b] > 0 and not st["done"][b] and (st["pos"][b] >= PL - 1 or "sampler_in_prompt" in mut))
                st["handled"][b] = int(mine)
                if mine:
                    s = _sample_row(c, st, k, b, l, P if "max_new_pfx" in mut else PL, mut, info[b])
                    st["pos"][b] += 1
                    info[b]["steps"].append((k, "generate", s))
                    info[b]["sampled"].append(k)
                taken = int(mine) and "handled_ignored" not in mut
            # ---- logit_step_kernel, mode 2 ----
            if st["done"][b] or taken:
                continue
            mp = int(st["pos"][b])
            if mp == (0 if "probe_at_0" in mut else npfx(b)):                          # model.rs:293-315
                p, x = K.softmax64(_finite(l))
                ns = int(tk[4])
                rel = K._rel(K._eps_se(p, x, path, V), x[ns])
                st["no_speech"][b] = p[ns]
                info[b]["ns_bound"] = p[ns] * rel
                info[b]["ns_decided"] &= bool(abs(p[ns] - 0.6) > p[ns] * rel)
                if p[ns] > 0.6:
                    st["done"][b] = 2
                st["pos"][b] = mp + 1
                info[b]["steps"].append((k, "probe", None))
            elif mp < (P if "phase_no_pfx" in mut else PL) - 1:                        # a prompt or stepwise-prefix position
                st["pos"][b] = mp + 1
                info[b]["steps"].append((k, "prompt", None))
            else:
                n = int(st["n_tokens"][b])
                info[b]["slot"][k] = n
                s = K.step_ref(_finite(l), list(st["tokens"][b, :n]), int(st["have_last"][b]), int(st["last_ts"][b]), c.sup, tk, path)
                info[b]["decided"] &= s.decided
                info[b]["lp_bound"] += s.lp_bound
                K._bookkeep(st, b, s.next, s.lp, tk, c.cap, c.max_new, P if "max_new_pfx" in mut else PL, ())
                st["pos"][b] = mp + 1
                info[b]["steps"].append((k, "generate", s))
        for b in range(B):
            i = info[b]
            if not row_decided(i):
                i["good"] = min(i["good"], k)
            snap = {key: st[key][b].copy() for key in ROW_KEYS}
            snap["tokens"] = snap["tokens"][:c.ctx]
            snap.update(lp_bound=i["lp_bound"], ns_bound=i["ns_bound"], probs_bound=st["probs_bound"][b].copy())
            i["snap"].append(snap)
    st["tokens"] = st["tokens"][:, :c.ctx]
    return st, info


# what of the state belongs to one row (the logits of a step aside)
ROW_KEYS = ("tokens", "n_tokens", "done", "have_last", "last_ts", "sum_logprob", "no_speech", "pos", "pfx", "inv_t", "seed", "clip",
            "attempt", "handled", "detect_flag", "lang_out", "probs", "loop_exit")


def row_decided(i):
    return i["decided"] and i["ns_decided"]


def from_token_case(tc):
    """a mode-2 kref.TokenCase (kref.sequence_cases' "pool" cases) as a PoolCase without prefix, sampling, detection or guard"""
    layout = [l for l in K.token_layouts() if tc.name.startswith(l[0] + "/")][0]
    c = PoolCase(tc.name, layout, tc.B, tc.K, tc.ctx, tc.prompt_len, tc.max_new, use_pfx=False)
    assert c.cap == tc.cap and np.array_equal(c.sup, tc.sup) and np.array_equal(c.tk, tc.tk) and (tc.modes == 2).all() and tc.use_pos.all()
    c.logits = tc.logits.copy()
    for k in ("tokens", "n_tokens", "done", "have_last", "last_ts", "sum_logprob", "no_speech", "pos"):
        setattr(c, k, getattr(tc, k).copy())
    c.events = [("admit", int(a[0]), int(a[1]), int(a[2]), int(a[3]), int(a[4]), 0, 0, 0) for a in tc.admits]
    assert all(a[5] == tc.prompt_len for a in tc.admits)
    return c


# ---- the suite's cases -----------------------------------------------------------------------------------------------------
# A row is described by where it starts (k, position) -- at an admission, a retry, or from a planted state at step 0 -- and by
# its prefix length; from those its position at every step follows (one per step while it lives), and with it what the step's
# logits are FOR: at the probe position p(no_speech) is the row's own value; at prompt and stepwise-prefix positions nothing
# may read them, so they carry p(no_speech) = 0.9 and a peak (a probe or a generation step that lands there by an off-by-one
# ends the row or appends a token); at generation positions they are kref.sequence_cases' peaks, which move a row through the
# rule states.  Idle and finished rows get the traps too.
def _peaks(rng, V, tk, p_eot=0.0):
    NT = tk.no_timestamps
    bg = rng.standard_normal(V)
    r = rng.random()
    if r < p_eot:
        bg[tk.eot] = bg.max() + 6
    elif r < 0.5:
        bg[int(rng.integers(NT + 1, V))] = bg.max() + 6 + rng.random()
    else:
        bg[int(rng.integers(0, tk.eot))] = bg.max() + 9 + rng.random()
    return bg


def _set_no_speech(bg, tk, t):
    so = np.exp(np.delete(bg, tk.no_speech).astype(np.float32).astype(np.float64)).sum()
    bg[tk.no_speech] = np.log(t * so / (1 - t))


class _Rows:
    """builds a PoolCase row by row and plants its logits"""

    def __init__(self, name, layout, B, K_, ctx, P, max_new, seed, use_pfx=True):
        self.c = PoolCase(name, layout, B, K_, ctx, P, max_new, use_pfx)
        self.rng = np.random.default_rng(K.zlib_key(name, seed))
        self.starts = [[] for _ in range(B)]           # (k, position, p(no_speech) at its probe) of every start of the row
        self.npfx = [0] * B
        self.script = {}                                # (k, b) -> a token whose logit is the row's largest at step k
        self.b = 0

    def prompt(self):
        tk = self.c.tko
        return [tk.sot, tk.en, tk.transcribe] if self.c.P == 3 else [tk.sot, tk.transcribe]

    def prefix(self, b, n, ids=None):
        tk, c = self.c.tko, self.c
        ids = [int(v) for v in self.rng.integers(20, tk.eot, n)] if ids is None else list(ids)
        assert len(ids) == n
        c.tokens[b, :n] = ids
        self.npfx[b] = n

    def _next(self, label, route):
        b = self.b
        self.b += 1
        self.c.labels[b], self.c.routes[b] = label, route
        return b

    def idle(self):
        return self._next("idle", "none")

    def admit(self, k, n_prefix=0, onepass=False, probe_p=None, detect=0, ids=None):
        c, tk = self.c, self.c.tko
        route = "none" if n_prefix == 0 else ("onepass" if onepass else "stepwise")
        b = self._next(f"admit@{k} pfx {n_prefix} {route}", route)
        self.prefix(b, n_prefix, ids)
        pos0 = n_prefix if onepass else 0
        pr = self.prompt()
        c.events.append(("admit", k, b, pr[0], pr[1], pr[-1], detect, n_prefix, pos0))
        self.starts[b].append((k, pos0, float(self.rng.uniform(0.05, 0.5)) if probe_p is None else probe_p))
        return b

    def live(self, hist, have_last, last_ts, n_prefix=0, done=0, ids=None, label="live"):
        """a row planted at its next generation position with the generated tokens `hist`"""
        c = self.c
        b = self._next(f"{label} pfx {n_prefix}", "none" if n_prefix == 0 else "onepass")
        self.prefix(b, n_prefix, ids)
        seq = self.prompt() + list(hist)
        n = n_prefix + len(seq)
        c.tokens[b, n_prefix:n] = seq
        c.n_tokens[b], c.have_last[b], c.last_ts[b], c.done[b], c.pos[b], c.pfx[b] = n, have_last, last_ts, done, n - 1, n_prefix
        if not done:
            self.starts[b].append((0, n - 1, 0.9))
        return b

    def retry(self, b, k, t, seed, clip, attempt):
        c = self.c
        c.events.append(("retry", k, b, float(np.float32(1.0) / np.float32(t)), seed, clip, attempt))
        self.starts[b].append((k, self.npfx[b], float(self.rng.uniform(0.05, 0.5))))

    def finish(self):
        c, tk, rng = self.c, self.c.tko, self.rng
        c.events.sort(key=lambda e: e[1])
        for k in range(c.K):
            for b in range(c.B):
                st = [s for s in self.starts[b] if s[0] <= k]
                bg = _peaks(rng, c.V, tk)
                phase = "trap"
                if st:
                    pos = st[-1][1] + k - st[-1][0]
                    phase = "probe" if pos == self.npfx[b] else ("trap" if pos < self.npfx[b] + c.P - 1 else "generate")
                if (k, b) in self.script:
                    bg[self.script[(k, b)]] = bg.max() + 6
                if phase == "probe":
                    _set_no_speech(bg, tk, st[-1][2])
                elif phase == "trap":
                    _set_no_speech(bg, tk, 0.9)
                c.logits[k, b, :c.V] = bg
        c.starts, c.npfx, c.script = self.starts, self.npfx, dict(self.script)
        return c


def phase_cases(layout):
    """Prefix phases: n_prefix in {0, 1, 4, 17} on both routes and one prefix that nearly fills ctx; rows the probe ends; rows
    admitted mid-run beside rows in other phases; max_new = 5 counted from behind the prefix; the cap on the physical sequence"""
    name, V, tk, _ = layout
    small = name == "small"
    out = []
    for P in ((2, 3) if small else (3,)):
        K_ = 24 if small else 12
        r = _Rows(f"{name}/phase_P{P}", layout, 16, K_, 64, P, 5, 1)
        long_n = r.c.cap - P - 2
        r.admit(0)
        r.admit(0, 1)
        r.admit(0, 1, True)
        r.admit(0, 4)
        r.admit(0, 4, True)
        r.admit(0, 17 if small else 4)
        r.admit(0, 17, True)
        r.admit(0, long_n, True)
        r.admit(0, probe_p=0.8)                           # the probe ends these two
        r.admit(0, 4, True, probe_p=0.75)
        ts0 = tk.zero_sec + 3
        r.live([ts0, 11], 1, ts0, 4)                      # generating from step 0 on
        r.admit(K_ - 2)                                   # P = 3: still at a prompt position when the run ends
        r.admit(2)                                        # mid-run, beside rows in other phases
        r.admit(3, 4)
        r.admit(5, 17, True)
        r.admit(1, 1, probe_p=0.7)
        out.append(r.finish())
    return out


def _plant_states(r, k_states, pfx_cycle, sampler=None):
    """live rows in the rule states `k_states`, prefixes cycling; sampler(b, i): sets the row's sampling arguments"""
    tk = r.c.tko
    for i, state in enumerate(k_states):
        toks, hl, lt = K._hist(state, tk, r.rng, r.c.V)
        b = r.live(toks[3:], hl, lt, pfx_cycle[i % len(pfx_cycle)], label=f"live {state}")
        if sampler:
            sampler(b, i)


def sampled_cases(layout):
    """Sampled rows beside greedy rows: rows planted in every rule state with inv_t > 0, finished rows sent on a retry (still at
    their probe or prompt position in the first steps: the greedy kernel serves them, handled == 0), greedy rows in mixed
    phases, finished rows (sampling arguments set: still nobody's)"""
    name, V, tk, _ = layout
    small = name == "small"
    out = []
    for P in ((2, 3) if small else (3,)):
        K_ = 12 if small else 8
        r = _Rows(f"{name}/sampled_P{P}", layout, 16, K_, 64, P, 6, 2)
        c = r.c
        ts = (0.2, 0.6, 1.0)

        def sampler(b, i):
            c.inv_t[b] = np.float32(1.0) / np.float32(ts[i % 3])
            c.seed[b], c.clip[b], c.attempt[b] = 0x1234_5678_9abc + 17 * i, 3 + i, 1 + i % 4

        _plant_states(r, (K.FIRST, K.FIRST, K.SUP_TS, K.NON_TS, "TEXT", "TEXT", "TEXT"), (0, 4, 17, 1), sampler)
        ts0 = tk.zero_sec + 5
        for i, n_prefix in enumerate((0, 4, 1)):          # finished rows, retried
            b = r.live([ts0, 11, 12, tk.eot], 1, ts0, n_prefix, done=1, label="finished, retried")
            c.sum_logprob[b], c.no_speech[b] = -3.5 - i, 0.25
            r.retry(b, (0, 1, 3)[i], ts[i], 0xfeed_0000_0001 + i, 40 + i, 2 + i)
        r.admit(0, 4)                                     # greedy rows
        r.admit(1, 1, True)
        _plant_states(r, (K.SUP_TS, "TEXT"), (4, 0))
        for i, d in enumerate((1, 2)):                    # finished rows with sampling arguments: bit-identical, pos included
            b = r.live([ts0, 13, tk.eot], 1, ts0, 4 * i, done=d, label="finished")
            sampler(b, i)
            c.sum_logprob[b], c.pos[b] = -1.25, 9
        c.sampled[:] = 1
        c.sampled[0 if P == 3 else 1] = 0                 # one step without the sampler: handled is not read
        out.append(r.finish())
    return out


def retry_cases(layout):
    """Retry on finished rows with and without a prefix: at k = K (the reset itself is what comes back), at k = 0 and mid-run
    (the row probes again at pos == pfx, then samples with step = the physical token count); a row that finishes in the run"""
    name, V, tk, _ = layout
    small = name == "small"
    out = []
    for P in ((2, 3) if small else (3,)):
        K_ = 10 if small else 8
        r = _Rows(f"{name}/retry_P{P}", layout, 16, K_, 64, P, 4, 3)
        c = r.c
        ts0 = tk.zero_sec + 7
        spec = [(0, 0), (4, 0), (17, 0), (1, 0), (0, 2), (4, 2), (17, 3), (0, K_), (4, K_), (17, K_), (1, 1), (4, 1)]
        for i, (n_prefix, k) in enumerate(spec):
            b = r.live([ts0, 11, 12, 13, tk.eot], 1, ts0, n_prefix, done=1 + (i % 2), label=f"finished, retry@{k}")
            c.sum_logprob[b], c.no_speech[b], c.detect_flag[b], c.loop_exit[b] = -2.5 - i, 0.125, 1, 1
            c.inv_t[b], c.seed[b], c.clip[b], c.attempt[b] = 9.0, 5, 6, 7      # what the retry must overwrite
            r.retry(b, k, (0.2, 0.6, 1.0)[i % 3], 0xabcd_0000_0000_0100 + i, 70 + i, 1 + i % 5)
        b = r.admit(0, 4, True)                           # finishes at max_new = 4 (step 6), retried at step 7
        r.retry(b, 7, 0.6, 0x77, 90, 2)
        b = r.admit(0, probe_p=0.8)                       # ended by the probe, retried: probes again with another p
        r.retry(b, 2, 1.0, 0x78, 91, 3)
        r.admit(1, 1)                                     # a greedy row beside them
        r.idle()
        c.sampled[:] = 1
        out.append(r.finish())
    return out


DETECT_SIZES = (1, 64, 65, 256)


def detect_cases(layout):
    """Detection: table sizes 1, 64, 65 and 256; rows admitted with the flag (at step 0 and mid-run), one of them ended by the
    probe in the same step, one with an exact tie, one flat; rows that have the flag but pos != 0, finished rows with the flag,
    rows without the flag: their slot 1, lang_out and probs keep the canaries"""
    name, V, tk, _ = layout
    out = []
    for n in DETECT_SIZES:
        r = _Rows(f"{name}/detect_n{n}", layout, 16, 4, 64, 3, 0, 4)
        c = r.c
        base = np.arange(tk.en, tk.en + n) if n <= tk.n_languages else r.rng.choice(np.delete(np.arange(V), tk.no_speech), n, replace=False)
        lt = r.rng.permutation(base).astype(np.int32)
        c.lang_tokens = lt
        rows = [r.admit(0, detect=1) for _ in range(4)]
        ended = r.admit(0, detect=1, probe_p=0.85)        # detected although the probe ends it in this very step
        tie, flat = r.admit(0, detect=1), r.admit(0, detect=1)
        late = [r.admit(1, detect=1), r.admit(2, detect=1)]
        r.admit(0, detect=0)                              # no flag
        r.admit(0, 1, detect=0)
        r.admit(1, 4, True, detect=0)
        ts0 = tk.zero_sec + 2
        b = r.live([ts0, 11], 1, ts0)                     # the flag, but not at position 0
        c.detect_flag[b] = 1
        b = r.live([], 0, 0, done=1, label="finished")    # the flag and position 0, but finished
        c.detect_flag[b], c.pos[b] = 1, 0
        b = r.live([], 0, 0)                              # at its first generation position with the flag (P - 1 != 0)
        c.detect_flag[b] = 1
        r.idle()
        r.finish()
        if n > 1:
            top = float(np.nanmax(c.logits[0, tie, lt]))
            c.logits[0, tie, lt[n // 2]] = c.logits[0, tie, lt[n - 1]] = top + 1.0     # an exact tie: the earlier index
            c.logits[0, flat, lt] = 0.0
            for b in (tie, flat):                         # the probe's p(no_speech) moved with them: put it back
                bg = c.logits[0, b, :V].astype(np.float64)
                _set_no_speech(bg, tk, 0.2)
                c.logits[0, b, :V] = bg
        c.tie_row, c.flat_row, c.ended_row, c.flag_rows, c.late_rows = tie, flat, ended, rows, late
        out.append(c)
    return out


A_, B_, C_, D_ = 100, 200, 300, 400


def guard_cases(layout):
    """The guard's gate.  Prefix ids that contain the n-gram (a b c ...) and the loop (a b a b ...): with the right prompt_len
    the generated history a b bans nothing and closes no loop, with a prompt_len that forgets the prefix it bans c / fires the
    exit.  Rows without a prefix whose generated tokens really hold the n-gram / the loop; rows at their probe or prompt
    positions and finished rows (logits bit-identical, loop_exit canary 1 kept); rows at their first generation position
    (loop_exit cleared)."""
    name, V, tk, _ = layout
    small = name == "small"
    out = []
    for gname, g in (("ngram", G.params(no_repeat_ngram=3, repetition_penalty=1.3)), ("loop", G.params(loop_period=2, loop_repeats=3))):
        for P in ((2, 3) if small else (3,)):
            r = _Rows(f"{name}/guard_{gname}_P{P}", layout, 16, 5, 64, P, 0, 5)
            c = r.c
            c.guard = g
            Z = tk.zero_sec + 1
            if gname == "ngram":
                pre, hist_pfx, hist_real, want = [A_, B_, C_], [Z, A_, B_], [Z, A_, B_, C_, D_, A_, B_], C_
            else:
                pre, hist_pfx, hist_real, want = [A_, B_], [Z, A_, B_], [Z, A_, B_, A_, B_, A_, B_], D_
            for n_prefix in (8, 17, 9):
                ids = [pre[i % len(pre)] for i in range(n_prefix)]
                b = r.live(hist_pfx, 1, Z, n_prefix, ids=ids, label=f"{gname} in the prefix only")
                r.script[(0, b)] = want
            for _ in range(3):
                b = r.live(hist_real, 1, Z, label=f"{gname} generated")
                r.script[(0, b)] = want
            b = r.live([Z, A_, B_, Z + 4, Z + 4], 1, Z + 4, 4, label="after two timestamps")
            for n_prefix, one in ((0, False), (4, False), (17, False), (8, True)):       # probe and prompt positions
                ids = [pre[i % len(pre)] for i in range(n_prefix)]
                b = r.admit(0, n_prefix, one, ids=ids)
                c.loop_exit[b] = 1
            b = r.live([], 0, 0, 8, ids=[pre[i % len(pre)] for i in range(8)], label="first generation position")
            c.loop_exit[b] = 1
            b = r.live([], 0, 0, label="first generation position")
            c.loop_exit[b] = 1
            b = r.live(hist_real + [tk.eot], 1, Z, done=1, label="finished")
            c.loop_exit[b] = 1
            r.script[(0, b)] = want
            r.admit(0, 1, ids=pre[:1])
            r.idle()
            out.append(r.finish())
    return out


# ---- what the sections are about, stated on a final state (the reference's on the CPU, the kernels' on the GPU) --------------
def _admitted_once(c, b):
    return len(c.starts[b]) == 1 and any(e[0] == "admit" and e[2] == b for e in c.events)


def phase_properties(c, st, info):
    """Prefix phases, on the rows admitted once whose run is decided: the probe read the logits of the step at pos == n_prefix
    and no other (every other step before generation carries p(no_speech) = 0.9); p > 0.6 ends the row with flag 2 and nothing
    else moves; positions before generation move pos only; the first generated token sits in slot n_prefix + P and obeys the
    first-token rule; max_new counts from behind the prefix; the cap counts the physical sequence.  Returns the rows seen."""
    tk, P = c.tko, c.P
    seen = {"ended": 0, "prompt": 0, "max_new": 0, "cap": 0, "generating": 0}
    for b in range(c.B):
        if not _admitted_once(c, b) or not row_decided(info[b]):
            continue
        k0, pos0, probe_p = c.starts[b][0]
        n_prefix, PL = c.npfx[b], c.npfx[b] + P
        what = f"{c.name} row {b} ({c.labels[b]})"
        assert st["pfx"][b] == n_prefix, what
        steps = c.K - k0
        assert np.array_equal(st["tokens"][b, :n_prefix], c.tokens[b, :n_prefix]), f"{what}: prefix ids touched"
        if pos0 + steps <= n_prefix:                       # never reached its probe
            assert st["no_speech"][b] == 0.0 and st["done"][b] == 0 and st["pos"][b] == pos0 + steps, what
            continue
        assert abs(st["no_speech"][b] - probe_p) < 1e-5, f"{what}: no_speech {st['no_speech'][b]}, the probe step carries {probe_p}"
        n = int(st["n_tokens"][b])
        if probe_p > 0.6:
            assert st["done"][b] == 2 and st["pos"][b] == n_prefix + 1 and n == PL, what
            seen["ended"] += 1
        if n == PL:                                        # nothing generated: only pos moved
            assert np.all(st["tokens"][b, PL:] == 7) and st["sum_logprob"][b] == 0.0 and st["have_last"][b] == 0, what
            if st["done"][b] == 0:
                assert st["pos"][b] == pos0 + steps <= PL - 1, what
                seen["prompt"] += 1
            continue
        first = int(st["tokens"][b, PL])
        assert tk.zero_sec <= first <= tk.one_sec, f"{what}: first generated token {first} in slot {PL}"
        if st["done"][b] == 1 and n == c.ctx:              # the cap: cap - 1 tokens, then eot
            assert st["tokens"][b, n - 1] == tk.eot and n - 1 - PL < c.max_new, what
            seen["cap"] += 1
        elif st["done"][b] == 1:                           # max_new tokens behind the prompt, then eot
            assert n == PL + c.max_new + 1 and st["tokens"][b, n - 1] == tk.eot, f"{what}: n_tokens {n} with max_new {c.max_new}"
            seen["max_new"] += 1
        else:
            assert n - PL < c.max_new and st["pos"][b] == n - 1, what
            seen["generating"] += 1
    return seen


def detect_properties(c, st, info):
    """Detection: rows admitted with the flag hold the detected token in slot 1 and lang_out, probabilities in probs[:n]; the
    exact tie goes to the earlier table index, flat logits to the first; every other row keeps its canaries"""
    lt, n = c.lang_tokens, len(c.lang_tokens)
    detected = set(c.flag_rows + c.late_rows + [c.tie_row, c.flat_row, c.ended_row])
    for b in range(c.B):
        what = f"{c.name} row {b} ({c.labels[b]})"
        if b in detected:
            assert st["lang_out"][b] in lt and st["tokens"][b, 1] == st["lang_out"][b], what
            assert abs(float(st["probs"][b, :n].sum()) - 1.0) < 1e-4 and np.all(st["probs"][b, n:] == 123.0), what
            assert st["tokens"][b, 0] == c.tko.sot, what
        else:
            assert st["lang_out"][b] == -7 and np.all(st["probs"][b] == 123.0), f"{what}: canary gone"
            ev = [e for e in c.events if e[0] == "admit" and e[2] == b]
            want1 = ev[0][4 if c.npfx[b] == 0 else 3] if ev else c.tokens[b, 1]
            if c.npfx[b] == 0 or not ev:
                assert st["tokens"][b, 1] == want1, f"{what}: slot 1 written"
    if n > 1:
        assert st["lang_out"][c.tie_row] == lt[n // 2] and st["lang_out"][c.flat_row] == lt[0]
    assert st["done"][c.ended_row] == 2, "the probe ends the row in the step that detects its language"


def guard_properties(c, st, info):
    """The guard's gate: a row whose prefix alone holds the n-gram / the loop picks the token the logits favour (nothing is
    banned, no exit); a row that generated them does not (ngram: the banned token is passed over; loop: eot, loop_exit 1)"""
    tk = c.tko
    n_pfx = n_gen = 0
    for (k, b), want in c.script.items():
        if c.done[b] or not row_decided(info[b]):
            continue
        got = int(st["tokens"][b, c.n_tokens[b]])
        if "in the prefix only" in c.labels[b]:
            assert got == want and st["loop_exit"][b] == 0, f"{c.name} row {b}: picked {got}, not {want}: the prefix is in the guard's history"
            n_pfx += 1
        elif c.guard.loop_period:
            assert got == tk.eot and st["loop_exit"][b] == 1 and st["done"][b] == 1, (c.name, b, got)
            n_gen += 1
        else:
            assert got != want, (c.name, b, got)
            n_gen += 1
    assert n_pfx >= 3 and n_gen >= 3, (c.name, n_pfx, n_gen)


SECTIONS = {"phase": phase_cases, "sampled": sampled_cases, "retry": retry_cases, "detect": detect_cases, "guard": guard_cases}


@functools.lru_cache(maxsize=None)
def _cases(lname, section):
    layout = [l for l in K.token_layouts() if l[0] == lname][0]
    return tuple(SECTIONS[section](layout))


def cases(layout, section):
    """the cases of one section for one layout, built once; a test copies what it changes (PoolCase.state())"""
    return _cases(layout[0], section)


@functools.lru_cache(maxsize=None)
def _refs(lname, section):
    return tuple(pool_step_ref(c) for c in _cases(lname, section))


def refs(layout, section):
    """(state, info) of every case of the section, computed once"""
    return _refs(layout[0], section)


# ---- coverage, from the reference alone ------------------------------------------------------------------------------------
def coverage(layout):
    """what the suite's cases of one layout reach, counted over the steps a row takes before its first undecided one (the GPU
    test compares the row after every one of those): cells[(phase, route)] = rows that took a step of that phase on that
    route, sampled[rule state] = sampled steps, detect = detections"""
    import collections
    cells, sampled = collections.Counter(), collections.Counter()
    detect = 0
    for sec in SECTIONS:
        for c, (st, info) in zip(cases(layout, sec), refs(layout, sec)):
            for b in range(c.B):
                i = info[b]
                for ph in {s[1] for s in i["steps"] if s[0] < i["good"]}:
                    cells[(ph, c.routes[b])] += 1
                for k, ph, s in i["steps"]:
                    if k in i["sampled"] and k < i["good"]:
                        sampled[s.state] += 1
                detect += sum(1 for d in i["detect"] if d["k"] < i["good"])
    return cells, sampled, detect


def check_coverage(layout):
    cells, sampled, detect = coverage(layout)
    for ph in PHASES:
        for route in ROUTES:
            assert cells[(ph, route)] >= 8, f"{layout[0]}: only {cells[(ph, route)]} decided rows in ({ph}, {route}): {dict(cells)}"
    for s in K.RULE_STATES:
        assert sampled[s] >= 5, f"{layout[0]}: only {sampled[s]} decided sampled steps in state {s}: {dict(sampled)}"
    assert detect >= 24, f"{layout[0]}: only {detect} decided detections"
    return cells, sampled, detect


# ---- embed_ragged_kernel ---------------------------------------------------------------------------------------------------
EMBED_T = (1, 4, 17, 65, 223)


def embed_ragged_case(seed=0):
    """clips of T in EMBED_T packed at offsets off the multiples of 16, the table permuted against the token rows, canary rows
    between the clips and past the last.  Returns dict(tokens, E, P, x, clips, V, d, n_pos)."""
    rng = np.random.default_rng(K.zlib_key("embed_ragged", seed))
    V, d, n_pos, stride = 1000, 128, 448, 224
    E, P = K.f16(rng.standard_normal((V, d))), K.f16(rng.standard_normal((n_pos, d)) * 0.5)
    rows = [3, 0, 5, 1, 4]                                 # token row of table entry z: not z
    tokens = rng.integers(0, V, (6, stride)).astype(np.int32)
    clips = np.zeros((len(EMBED_T), 4), np.int32)
    off = 3
    for z in np.argsort(rng.random(len(EMBED_T))):         # packed in yet another order
        T = EMBED_T[z]
        off += off % 16 == 0                               # never on a multiple of 16
        clips[z] = [rows[z], T, off, 0]
        off += T + 2                                       # two canary rows between clips
    assert all(int(c[2]) % 16 for c in clips)
    tokens[rows[0], 0], tokens[rows[4], 0], tokens[rows[4], EMBED_T[4] - 1] = 0, V - 1, 0
    tokens[rows[2], 16], tokens[rows[3], 64] = V - 1, V - 1
    m_rows = off + 1
    x = np.full((m_rows, d), 777.0, np.float32)
    return dict(tokens=tokens, E=E, P=P, x=x, clips=clips, V=V, d=d, n_pos=n_pos, m_rows=m_rows)


def embed_ragged_ref(ec, mut=None):
    """x[off_z + i] = E[tokens[row_z][i]] + P[i] in fp64; rows no clip covers keep what x held.  mut "table_row": clip z reads
    token row z, not c.row; "packed_pos": position off + i, not i"""
    x = K.d64(ec["x"]).copy()
    E, P = K.d64(ec["E"]), K.d64(ec["P"])
    covered = np.zeros(len(x), bool)
    for z, (row, T, off, _) in enumerate(ec["clips"]):
        src = z if mut == "table_row" else row
        for i in range(T):
            x[off + i] = E[ec["tokens"][src, i]] + P[off + i if mut == "packed_pos" else i]
        covered[off:off + T] = True
    return x, covered


def run_embed_ragged(ec, clips=None, x=None):
    x = ec["x"].copy() if x is None else x
    clips = np.ascontiguousarray(ec["clips"] if clips is None else clips, np.int32)
    t = ec["tokens"]
    rc = lib().kref_embed_ragged(K.ptr(t), t.shape[1], t.shape[0], K.ptr(ec["E"]), ec["V"], K.ptr(ec["P"]), ec["n_pos"], K.ptr(x),
                                 len(x), K.ptr(clips), len(clips), ec["d"])
    return rc, x
