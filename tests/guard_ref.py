"""The repetition guard's contract (include/norma_hip.h: nh_set_guard) in numpy:

  edit        the four edits of one row's f32 logits, bit for bit what the kernel must give: every operation is one IEEE f32
              multiply, divide or add, or an assignment
  greedy_ref  a whole greedy decode of one clip driven by a tokens -> logits callback: the edit, an fp64 softmax, the logit
              rules of tests/beam_ref.py, the greedy step's bookkeeping.  It reports the smallest margin between the chosen
              token and the runner-up at any step, in log-probability.
"""
import math
from types import SimpleNamespace

import numpy as np

import beam_ref

OFF = dict(no_repeat_ngram=0, repetition_penalty=1.0, loop_period=0, loop_repeats=0, bias=False)


def params(**kw):
    p = dict(OFF)
    p.update(kw)
    return SimpleNamespace(**p)


def history(tokens, n, prompt_len, tk):
    """h: the generated ids below eot, in order"""
    return [int(t) for t in tokens[prompt_len:n] if t < tk.eot]


def have_last(tokens, n, prompt_len, tk):
    """the decode's have_last: a timestamp has been generated"""
    return any(t > tk.no_timestamps for t in tokens[prompt_len:n])


def loop_found(h, pmax, R):
    m = len(h)
    for p in range(1, pmax + 1):
        if p * R <= m and all(h[m - 1 - i] == h[m - 1 - i - p] for i in range(p * (R - 1))):
            return True
    return False


def edit(logits, tokens, n, prompt_len, p, bias, tk):
    """logits: f32 [V] of a running row at a generation position; tokens[:n] its tokens, prompt_len the physical prompt; p:
    params(); bias: {token: beta} or None.  Returns (edited f32 [V], loop_exit 0 | 1)."""
    x = np.array(logits, dtype=np.float32).copy()
    h = history(tokens, n, prompt_len, tk)
    m = len(h)
    r = np.float32(p.repetition_penalty)
    if r != np.float32(1.0):
        with np.errstate(all="ignore"):
            for v in dict.fromkeys(h):
                x[v] = x[v] * r if x[v] < 0 else x[v] / r
    if p.bias and bias:
        with np.errstate(all="ignore"):
            for v, beta in bias.items():
                x[v] = x[v] + np.float32(beta)
    N = p.no_repeat_ngram
    if N > 0 and m >= N - 1:
        s = h[m - N + 1:]
        for i in range(0, m - N + 1):
            if h[i:i + N - 1] == s:
                x[h[i + N - 1]] = -np.inf
    exit_ = 0
    if p.loop_period > 0 and loop_found(h, p.loop_period, p.loop_repeats):
        rule = beam_ref.rule_of(tokens, n, have_last(tokens, n, prompt_len, tk), tk)
        if rule in (1, 3):   # text only / last token is text: eot is not masked there
            keep = x[tk.eot]
            x[:] = -np.inf
            x[tk.eot] = keep
            exit_ = 1
    return x, exit_


def rule_margin(x, tokens, n, hl, sup, tk):
    """|log sum_ts - log max_text| where the step's rule is decided by the masses (last token text); inf elsewhere"""
    if beam_ref.rule_of(tokens, n, hl, tk) != 3:
        return math.inf
    NT = tk.no_timestamps
    l = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore"):
        e = np.exp(l - l.max())
    sup = np.asarray(sup, dtype=bool)
    if sup[NT + 1:].any():
        return math.inf
    sum_ts, text = float(e[NT + 1:].sum()), np.where(~sup[:NT], e[:NT], 0.0)
    if sum_ts <= 0.0 or text.max() <= 0.0:
        return math.inf
    return abs(math.log(sum_ts) - math.log(float(text.max())))


def greedy_ref(step_logits, prompt, p, bias, tk, sup, cap, max_new=0, n_skip=0):
    """step_logits(tokens) -> logits [V] for the next token.  prompt: the physical prompt (n_skip of it a prefix).  Returns
    dict(tokens from sot on, trimmed; n_tokens; avg_logprob; loop_exit; raw (untrimmed, physical); min_margin)."""
    toks = list(prompt)
    PL = len(prompt)
    last_ts, hl, slp, loop_exit, min_margin = 0, False, 0.0, 0, math.inf
    while True:
        n = len(toks)
        lg = np.asarray(step_logits(toks), dtype=np.float32)
        if n == PL:
            loop_exit = 0
        x, ex = edit(lg, toks, n, PL, p, bias, tk)
        loop_exit = max(loop_exit, ex)
        q, _ = beam_ref.masked_probs(x, toks, n, hl, last_ts, sup, tk)
        min_margin = min(min_margin, rule_margin(x, toks, n, hl, sup, tk))
        order = np.lexsort((np.arange(len(q)), q))[::-1]
        nxt, second = int(order[0]), int(order[1])
        if q[nxt] > 0:
            if q[second] > 0:
                min_margin = min(min_margin, math.log(q[nxt]) - math.log(q[second]))
            slp += math.log(q[nxt])
        else:               # everything masked: the greedy step's convention, the last index at log-probability -inf
            nxt, slp = len(q) - 1, -math.inf
        if nxt > tk.no_timestamps:
            last_ts, hl = nxt, True
        toks.append(nxt)
        if len(toks) >= cap:
            toks.append(tk.eot)
            break
        if nxt == tk.eot:
            break
        if max_new > 0 and len(toks) - PL >= max_new:
            toks.append(tk.eot)
            break
    out = toks[n_skip:]
    trimmed = beam_ref.trim(out, tk.no_timestamps)
    return dict(tokens=trimmed, n_tokens=len(trimmed), avg_logprob=slp / len(out), loop_exit=loop_exit, raw=toks, min_margin=min_margin)
