"""Reference for prompted decodes (nh_set_prompts): Model::decode (model.rs:279-389) composed from the oracle's primitives
with a prefix in front of [sot, lang?, task], and a pure-Python model of host.Model's prompt history.

The oracle's own decode (whisper_oracle.c, wo_decode_t) always starts from the bare prompt, and the oracle is a yardstick
that stays as it is; so the loop is restated here, step for step, on decoder_forward / final_linear / apply_rules /
sample_token.  Every step runs the whole sequence again (the oracle's Python view has no incremental form): the decodes
the tests ask for are a few dozen tokens long.

What a prefix means (include/norma_hip.h, nh_set_prompts): positions 0 .. n-1 consume it, sot sits at position n and the
no-speech probe reads ITS logits, the rules see the physical sequence, the length cap counts the physical sequence, the
sampling counter is the physical token count; what comes back starts at sot, and avg_logprob is divided by that length.
"""
import numpy as np

NO_SPEECH_THRESHOLD = 0.6   # model.rs:308
LOGIT_BAR = 4e-3            # the project's logit bar: |d logit| <= 4e-3 * max(sigma, 0.1) (tests/test_gpu_parity.py)


def softmax_f32(logits: np.ndarray) -> np.ndarray:
    """whisper_oracle.c softmax_row: f32 throughout, the sum taken in index order (cumsum is sequential).  expf is taken as
    the correctly rounded exponential (numpy's f32 exp is a vector routine that may be an ulp off the C library's)."""
    x = np.ascontiguousarray(logits, dtype=np.float32)
    e = np.exp((x - x.max()).astype(np.float64)).astype(np.float32)
    s = np.cumsum(e, dtype=np.float32)[-1]
    return (e / s).astype(np.float32)


def argmax_total(p: np.ndarray) -> int:
    """Iterator::max_by(f32::total_cmp): the LAST maximum wins, a positive NaN beats everything (wo_argmax_total)"""
    b = np.ascontiguousarray(p, dtype=np.float32).view(np.int32)
    key = b ^ ((b >> 31).view(np.uint32) >> np.uint32(1)).view(np.int32)
    return int(len(key) - 1 - np.argmax(key[::-1]))


def prompted_decode(om, xa, prefix, max_new_tokens=0, temperature=0.0, seed=0, clip=0, attempt=0):
    """-> dict(tokens (from sot on, after the trailing-timestamp trim), avg_logprob, no_speech_prob, no_speech_exit,
    physical_len (prefix included, before the trim), min_gap (the smallest top-2 gap of the logits among the tokens the
    rules allow, over all generated steps, in units of max(sigma, 0.1) of that step's logits; inf when nothing was generated))"""
    from oracle import oracle as O
    tk, cfg = om.tok, om.cfg
    V, cap = cfg.vocab_size, cfg.max_target_positions - 1
    prefix = [int(t) for t in prefix]
    NP = len(prefix)
    tokens = prefix + [tk.sot] + ([tk.lang] if tk.lang >= 0 else []) + [tk.task]
    first_mask = om.mask(3)
    ys = om.decoder_forward(tokens, xa, True)                      # :293-305, flush = true
    p = softmax_f32(om.final_linear(ys[NP])[0])                    # the logits at sot's position
    nsp = float(p[tk.no_speech])
    out = dict(no_speech_prob=nsp, no_speech_exit=False, min_gap=float("inf"))
    if nsp > NO_SPEECH_THRESHOLD:                                  # :308-315
        out.update(tokens=tokens[NP:], avg_logprob=0.0, no_speech_exit=True, physical_len=len(tokens))
        return out
    have_last, last_ts, new_tokens, sum_lp = False, 0, 0, 0.0
    while tokens[-1] != tk.eot:                                    # :317
        ys = om.decoder_forward(tokens, xa, False)
        logits = om.final_linear(ys[-1])[0]
        p = softmax_f32(logits)                                    # :331
        p = om.apply_rules(p, tokens, last_ts) if have_last else (p + first_mask).astype(np.float32)   # :333-338
        if temperature > 0.0:                                      # :340-348, step = the physical token count
            nxt = O.sample_token(p, temperature, seed, clip, len(tokens), attempt)
            if nxt < 0:
                tokens.append(tk.eot)
                break
        else:
            nxt = argmax_total(p)                                  # :350-356
        allowed = np.sort(logits[p > -np.inf])
        if len(allowed) >= 2:
            out["min_gap"] = min(out["min_gap"], float(allowed[-1] - allowed[-2]) / max(float(logits.std()), 0.1))
        if nxt > tk.no_timestamps:                                 # :359-361
            last_ts, have_last = nxt, True
        tokens.append(nxt)
        new_tokens += 1
        sum_lp += float(np.log(np.float64(p[nxt])))                # :364-365
        if len(tokens) >= cap:                                     # :367-370, the PHYSICAL length
            tokens.append(tk.eot)
            break
        if max_new_tokens > 0 and new_tokens >= max_new_tokens and tokens[-1] != tk.eot:
            tokens.append(tk.eot)
            break
    seq = tokens[NP:]
    n = len(seq)
    out["physical_len"] = len(tokens)
    out["avg_logprob"] = sum_lp / n                                # :373, over the sequence from sot on
    while n >= 2 and seq[n - 2] > tk.no_timestamps:                # :375-381
        seq[n - 2] = seq[n - 1]
        n -= 1
    out["tokens"] = seq[:n]
    return out


# ---- host.Model's prompt history (include/norma_host.h: set_prompt_tokens, set_condition_on_previous) ----------------------
class PromptHistory:
    """What Model::transcribe keeps between slices.  prefix(): what the next slice decodes under; accept(): a decoded
    slice's text tokens join the history, unless it was accepted at a temperature above 0.5 (the history is dropped);
    final_chunk(): dropped, where the reference clears its language state."""

    def __init__(self, startofprev: int, max_target_positions: int, initial=(), condition_on_previous=False):
        self.sop, self.room = int(startofprev), max_target_positions // 2 - 2
        self.initial, self.cond, self.history = [int(t) for t in initial], bool(condition_on_previous), []

    def prefix(self):
        body = self.initial + (self.history if self.cond else [])
        if not body:
            return []
        return [self.sop] + body[-self.room:]

    def accept(self, text_tokens, temperature=0.0):
        if not self.cond:
            return
        if temperature > 0.5:
            self.history = []
        else:
            self.history += [int(t) for t in text_tokens]

    def final_chunk(self):
        self.history = []


# ---- the shared fixture: scripted weights whose greedy decode under a prefix of n tokens is known --------------------------
# common.scripted_overrides steers the token emitted after position p towards script[p - 2]; under a prefix of n tokens and
# the 3-token prompt, generation starts after position n + 2, i.e. at script[n].  So ONE script serves several prefix
# lengths when a well-formed transcript starts at each of them and ends (eot) before the next begins.
PREFIX_LENGTHS = (1, 5, 223)
FILLER = 1000


def long_script(tk, endless_from=None, C=448):
    """transcripts at script[1], script[5] and script[223]; endless_from = n: from script[n] on a segment that never closes
    (the decode runs into the length cap)"""
    import common
    s = [FILLER] * max(C, 448)
    s[1:5] = [tk.zero_sec, 777, 778, tk.eot]   # one open segment (the rules allow eot after text only: model.rs:216-223)
    t5 = common.transcript_script(tk, n_segments=2, words_per_segment=4, seed=5)
    s[5:5 + len(t5)] = t5
    t223 = common.transcript_script(tk, n_segments=1, words_per_segment=3, seed=7)
    s[223:223 + len(t223)] = t223
    if endless_from is not None:
        rng = np.random.default_rng(17)
        s[endless_from] = tk.zero_sec
        for i in range(endless_from + 1, len(s)):
            s[i] = int(rng.integers(300, 40000))
        sup = set(common.vocab.default_suppress_tokens("EnV1"))
        s = [t + 1 if (i > (endless_from or 0) and t in sup) else t for i, t in enumerate(s)]
    return s[:C] if C < 448 else s


def prefix_tokens(tk, n, clip=0):
    """n ids: <|startofprev|> (EnV1: no_speech - 1), then words that differ from clip to clip"""
    rng = np.random.default_rng([41, n, clip])
    return [tk.no_speech - 1] + [int(t) for t in rng.integers(300, 40000, size=n - 1)]


_FIXTURES = {}


def scripted_fixture(name="tiny.en", endless_from=None, n_clips=2):
    """(cfg, tk, overrides, oracle, [xa per clip], mels) for the scripted weights above, built once per process"""
    key = (name, endless_from, n_clips)
    if key not in _FIXTURES:
        import common
        from norma_amd import assets_io, synth
        from oracle import oracle as O
        cfg, tk = common.make_config(name), common.tokens_for(name)
        over = common.scripted_overrides(cfg, tk, long_script(tk, endless_from))
        om = common.build_oracle(cfg, tk, overrides=over)
        filt = assets_io.mel_filters(cfg.num_mel_bins)
        mels = np.stack([O.pcm_to_mel(synth.synth_pcm(k), filt)[:, :3000] for k in range(n_clips)])
        xas = [om.encoder_forward(m) for m in mels]
        _FIXTURES[key] = (cfg, tk, over, om, xas, mels)
    return _FIXTURES[key]
