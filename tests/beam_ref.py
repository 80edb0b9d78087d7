"""The beam search contract of include/norma_hip.h (nh_decode_beam) in plain Python, in two forms:

  step_ref     one step over given logits and hypothesis state, fp64 with norma's logit rules; it reports for every decision
               (text-vs-timestamp, merge order, candidate underflow) whether the gap exceeds what the kernel's f32 arithmetic
               can blur, per clip: an undecided clip accepts either outcome and is not compared further
  search_ref   the whole search driven by a step(tokens, last_ts) -> masked probabilities callback: winner, finished list,
               every step's parent map and the smallest score gap at any cut

Rows are beam-major: hypothesis j of clip b is row j * B + b.
"""
import math

import numpy as np

# |log q_device - log q_exact| of one candidate for logits within 30 of the row maximum: the f32 softmax sum over <= 65536
# fast-exp terms (argument rounding (l - m) * log2(e) <= 1.3e-6 relative per term, <= 64 serial + 10 tree additions of
# 6e-8 each) is within 6e-6 relative; the winner's expf(l - m) within 1.1e-6 (argument rounding at |l - m| <= 30 plus one
# ulp), the division 6e-8.  Twice their sum, as the bound every comparison below uses.
LOGQ_BOUND = 2e-5
# sum_ts >= max_text compares two f32 probabilities built from those sums: relative blur of the same size on each side
RULE_REL_BOUND = 4e-5
# Two candidates of ONE row share the row's maximum m and sum, so only their own expf(l - m) differ.  The kernel picks a
# row's candidates by logit, which is exact, but the merge orders them by s + log((double)q_f32): two distinct logits
# whose f32 q round to one value tie there and fall to the higher token id, whatever their logits say.  Relative error
# of one q against its neighbour's: l - m and its product with log2(e) round once each (6e-8 of |l - m| each), exp2 and
# the division one ulp each (1.2e-7 + 6e-8).
def same_row_blur(d):
    """d = |l - m| of a candidate"""
    return 2e-7 + 1.2e-7 * d


def rule_of(tokens, n, have_last, tk):
    """0 first token, 1 text only, 2 timestamps only, 3 'last token is text' (decided by the masses)."""
    NT = tk.no_timestamps
    if not have_last:
        return 0
    if tokens[n - 1] > NT:
        return 1 if (n >= 2 and tokens[n - 2] >= tk.eot) else 2
    return 3


def masked_probs(l, tokens, n, have_last, last_ts, sup, tk):
    """fp64 rule-masked probabilities of one row (masked: 0.0) and whether the text-vs-timestamp choice was decided."""
    V = len(l)
    NT = tk.no_timestamps
    l = np.asarray(l, dtype=np.float64)
    e = np.exp(l - l.max())
    p = e / e.sum()
    idx = np.arange(V)
    sup = np.asarray(sup, dtype=bool)
    rule = rule_of(tokens, n, have_last, tk)
    decided = True
    if rule == 3:
        ts_sup = bool(sup[NT + 1:].any())
        sum_ts = -math.inf if ts_sup else float(p[NT + 1:].sum())
        text = np.where(~sup[:NT], p[:NT], -math.inf)
        max_text = float(text.max()) if NT > 0 else -math.inf
        rule = 2 if sum_ts >= max_text else 3
        if math.isfinite(sum_ts) and math.isfinite(max_text):
            decided = abs(sum_ts - max_text) > RULE_REL_BOUND * max(sum_ts, max_text)
        branch = 2 if rule == 2 else 4
    else:
        branch = rule
    if branch == 0:
        m = (idx < tk.zero_sec) | (idx > tk.one_sec)
    elif branch == 1:
        m = sup | (idx > NT)
    elif branch == 2:
        m = sup | (idx <= NT) | (idx <= last_ts)
    else:
        m = sup | ((idx > NT) & (idx <= last_ts))
    return np.where(m, 0.0, p), decided


def top_candidates(q, K1):
    """The K1 best tokens by q, higher id first on equal q; q == 0 is no candidate."""
    order = np.lexsort((np.arange(len(q)), q))[::-1][:K1]
    return [int(v) for v in order if q[v] > 0.0]


def merge(live, K, n_fin, tk, cap, max_new, prompt_len, bound=0.0, info=None):
    """live: [(beam, tokens list, last_ts or -1, score, [(token, q)...])] of ONE clip.  Returns children [(parent beam, tokens,
    last_ts, score)], newly finished [(tokens, score)], the smallest score gap at a cut, and whether every comparison that
    shaped the outcome exceeded `bound`.  info (a dict, optional) receives exact_ties: how many neighbouring pairs of the
    walked list were equal candidates of one row, ordered by token id alone (unequal ones that f32 may merge: step_ref)."""
    cands = []
    for j, toks, lts, s, cq in live:
        for v, q in cq:
            cands.append((s + math.log(q), j, v))
    cands.sort(key=lambda c: (-c[0], c[1], -c[2]))
    by_beam = {j: (toks, lts) for j, toks, lts, s, cq in live}
    children, fin, gap, decided = [], [], math.inf, True
    last_used, last_live_s, last_fin_s = -1, None, None
    dropped_eot = None
    for i, (s, j, v) in enumerate(cands):
        if len(children) == K:
            gap = min(gap, last_live_s - s)   # the K-th live candidate against the first one left out
            break
        toks, lts = by_beam[j]
        t2 = list(toks) + [v]
        done, forced = v == tk.eot, False
        if len(t2) >= cap:
            done, forced = True, True
        elif not done and max_new > 0 and len(t2) - prompt_len >= max_new:
            done, forced = True, True
        if done:
            if n_fin + len(fin) < K:
                fin.append((t2 + ([tk.eot] if forced else []), s))
                last_fin_s = s
            elif dropped_eot is None:
                dropped_eot = s
                if last_fin_s is not None:
                    gap = min(gap, last_fin_s - s)    # an eot admitted against one dropped
        else:
            children.append((j, t2, v if v > tk.no_timestamps else lts, s))
            last_live_s = s
        last_used = i
    # order blur: neighbours from different rows up to the first candidate left out, within `bound`.  From one row: equal q
    # is an exact tie here and there (higher token id first)
    upto = min(len(cands), last_used + 2)
    exact_ties = 0
    for a, c in zip(cands[:upto], cands[1:upto]):
        if a[1] != c[1]:
            if abs(a[0] - c[0]) <= bound:
                decided = False
        elif a[0] == c[0]:
            exact_ties += 1
    if info is not None:
        info["exact_ties"] = exact_ties
    if n_fin + len(fin) >= K:
        children = []
    return children, fin, gap, decided


def step_ref(logits, state, K, B, n_finished, sup, tk, cap, max_new=0, prompt_len=3):
    """One step of the contract on logits [K*B][V] and state dict(tokens [K*B][C], n_tokens, have_last, last_ts, live, score).
    Returns dict(state arrays after the step, parent, n_finished, finished per clip, decided per clip, exact_ties per clip
    (equal candidates of one row inside the walked list), score_bound)."""
    R = K * B
    toks = np.array(state["tokens"], dtype=np.int32).copy()
    nt, hl, lt = (np.array(state[k], dtype=np.int32).reshape(R).copy() for k in ("n_tokens", "have_last", "last_ts"))
    lv = np.array(state["live"], dtype=np.int32).reshape(R).copy()
    sc = np.array(state["score"], dtype=np.float64).reshape(R).copy()
    out = dict(tokens=toks.copy(), n_tokens=nt.copy(), have_last=hl.copy(), last_ts=lt.copy(), live=lv.copy(), score=sc.copy(),
               parent=np.full(R, -1, dtype=np.int32), n_finished=np.array(n_finished, dtype=np.int32).copy(), finished=[], decided=[],
               exact_ties=[])
    V = logits.shape[1]
    for b in range(B):
        live, decided = [], True
        for j in range(K):
            r = j * B + b
            if not lv[r]:
                continue
            q, d = masked_probs(logits[r], toks[r], int(nt[r]), int(hl[r]), int(lt[r]), sup, tk)
            decided = decided and d
            top = top_candidates(q, K + 1)
            if any(q[v] < 1e-30 for v in top):
                decided = False    # the f32 probability may have underflowed to 0, which is no candidate
            lr = np.asarray(logits[r], dtype=np.float64)
            for v, w in zip(top, top[1:]):     # neighbours of one row that f32 may merge into a tie, which token id then orders
                gap = math.log(q[v]) - math.log(q[w])
                if 0.0 < gap <= same_row_blur(lr.max() - lr[v]) + same_row_blur(lr.max() - lr[w]):
                    decided = False
            live.append((j, toks[r, :nt[r]].tolist(), int(lt[r]) if hl[r] else -1, float(sc[r]), [(v, float(q[v])) for v in top]))
        if not live:
            out["finished"].append([]); out["decided"].append(True); out["exact_ties"].append(0)
            continue
        info = {}
        children, fin, _, d2 = merge(live, K, int(n_finished[b]), tk, cap, max_new, prompt_len, bound=2 * LOGQ_BOUND, info=info)
        out["exact_ties"].append(info["exact_ties"])
        if not children and not fin and int(n_finished[b]) == 0 and all(not c[4] for c in live):
            # everything masked: the clip's best prefix + the last index, log-prob -inf, left in record 0 (count stays 0)
            bj = max(live, key=lambda c: (c[3], -c[0]))
            fin_dead = [(bj[1] + [V - 1], -math.inf)]
        else:
            fin_dead = None
        for j in range(K):
            r = j * B + b
            if j < len(children):
                pj, t2, lts, s = children[j]
                out["tokens"][r, :len(t2)] = t2
                out["n_tokens"][r] = len(t2)
                is_ts = t2[-1] > tk.no_timestamps
                out["have_last"][r] = 1 if is_ts else hl[pj * B + b]
                out["last_ts"][r] = t2[-1] if is_ts else lt[pj * B + b]
                out["score"][r] = s
                out["live"][r] = 1
                out["parent"][r] = pj * B + b
            else:
                out["live"][r] = 0
        out["n_finished"][b] = int(n_finished[b]) + len(fin)
        out["finished"].append(fin)
        out["decided"].append(decided and d2)
        out.setdefault("dead_end", {})[b] = fin_dead
    out["score_bound"] = LOGQ_BOUND
    return out


def winner_of(finished, n_skip=0):
    """Index of the finished hypothesis with the greatest sum_logprob / n, the earliest on ties."""
    best = 0
    for f in range(1, len(finished)):
        if finished[f][1] / (len(finished[f][0]) - n_skip) > finished[best][1] / (len(finished[best][0]) - n_skip):
            best = f
    return best


def trim(tokens, no_timestamps):
    """finish_sequence's trailing-timestamp trim (model.rs:375-381)."""
    t = list(tokens)
    while len(t) >= 2 and t[-2] > no_timestamps:
        t[-2] = t[-1]
        t.pop()
    return t


def search_ref(step, prompt, K, tk, cap, max_new=0, n_skip=0):
    """The full search of one clip.  step(tokens, last_ts) -> masked probabilities (masked entries <= 0 or -inf); prompt: the
    physical prompt (prefix included, n_skip of it).  Returns dict(winner tokens (trimmed, from sot on), avg_logprob, n_tokens,
    finished [(tokens from sot on, score)], parents [per step: parent beam of every live slot], min_gap)."""
    live = [(list(prompt), -1, 0.0)]
    fin, parents, min_gap, gaps = [], [], math.inf, []
    prompt_len = len(prompt)
    while live and len(fin) < K:
        rows = []
        for j, (t, lts, s) in enumerate(live):
            q = np.asarray(step(t, lts), dtype=np.float64)
            q = np.where(np.isfinite(q) & (q > 0), q, 0.0)
            rows.append((j, t, lts, s, [(v, float(q[v])) for v in top_candidates(q, K + 1)]))
        children, f, gap, _ = merge(rows, K, len(fin), tk, cap, max_new, prompt_len)
        min_gap = min(min_gap, gap)
        gaps.append(gap)
        fin += f
        parents.append([c[0] for c in children])
        live = [(t2, lts, s) for _, t2, lts, s in children]
    if not fin:
        return dict(tokens=None, finished=[], parents=parents, min_gap=min_gap)
    w = winner_of(fin, n_skip)
    ratios = sorted((s / (len(t) - n_skip) for t, s in fin), reverse=True)
    if len(ratios) > 1:
        min_gap = min(min_gap, (ratios[0] - ratios[1]) * (len(fin[w][0]) - n_skip))   # the final ranking, in score units
    wt = trim(fin[w][0][n_skip:], tk.no_timestamps)
    return dict(tokens=wt, n_tokens=len(wt), avg_logprob=fin[w][1] / (len(fin[w][0]) - n_skip), winner=w,
                finished=[(t[n_skip:], s) for t, s in fin], parents=parents, min_gap=min_gap, step_gaps=gaps)
