"""Fixtures of the beam search tests: synthetic weights whose decode is steered position by position, like
common.scripted_overrides, but a position may steer towards SEVERAL tokens with weights (pos[p] += gain * w * E[token]), so
that hypotheses fork, finish early and overtake each other with margins a trained model would show.

Every position up to the end is scripted and max_new_tokens is the script's length: a hypothesis that walked past the script
into unsteered positions would run to the length cap on near-flat distributions, where cut gaps are ~3e-5.
"""
import numpy as np

import common
from norma_amd import synth

# The cut-gap bar.  Measured on the MI355X over the three fixtures (K in 1, 2, 4, 5; three clips each; plus the fork fixture on
# test-d256-mel128 and without a language token): the largest |device - reference| difference of any finished hypothesis's
# cumulative score, through nh_beam_hypotheses, was 1.351e-3 (fork, K = 5: the fp16 decoder against the f32 oracle over nine
# tokens); G is ten times that.  The smallest cut gap of any of those cases is 0.0257.  tests/test_beam_cpu.py asserts every
# case's smallest cut gap is at least G on the oracle alone.
G_MEASURED = 1.36e-3
G = 10 * G_MEASURED

X = [1000, 2000, 3000, 4000, 5000, 6000, 7000, 8000, 9000]


TAIL = [11000, 12000, 13000, 14000, 15000, 16000]


def _tail(step, ts0=None, w0=0.36, dw=0.06):
    """The step plus a tail of further tokens with distinct, falling weights: with K = 5 a row offers six candidates, and the
    ones behind the steered few must not be a flat crowd of near-ties.  ts0: the tail is timestamps from ts0 on."""
    have = {t for t, _ in step}
    pool = [t for t in (range(ts0, ts0 + 12, 2) if ts0 is not None else TAIL) if t not in have]
    return list(step) + [(t, w0 - dw * i) for i, t in enumerate(pool[:6 - len(step)])]


def fork(tk):
    """A text-vs-eot fork followed by flatter positions: the early eot has the better average at K >= 2, greedy walks on."""
    Z = tk.zero_sec
    return [[(Z, 1.0)], _tail([(X[0], 1.0)]), _tail([(X[1], 1.0)]),
            _tail([(X[2], 0.72), (tk.eot, 0.71)]),
            _tail([(X[3], 0.66), (X[4], 0.58), (X[5], 0.50)], w0=0.40, dw=0.08), _tail([(X[6], 0.66), (X[3], 0.58), (X[8], 0.50)], w0=0.40, dw=0.08),
            _tail([(Z + 100, 1.0)], ts0=Z + 110), _tail([(Z + 101, 1.0)], ts0=Z + 110), [(tk.eot, 1.0)]]


def closing(tk):
    """Two candidate closing timestamps T1 < T2, then a position steered to a timestamp between them: legal only for the
    hypothesis that holds T1, so last_ts must travel with its hypothesis."""
    Z = tk.zero_sec
    return [[(Z, 1.0)], _tail([(X[0], 1.0)]), _tail([(X[1], 1.0)]),
            _tail([(Z + 40, 0.72), (Z + 80, 0.68)], ts0=Z + 90),
            _tail([(Z + 60, 1.0)], ts0=Z + 90), _tail([(X[2], 1.0)]), _tail([(X[3], 1.0)]), [(tk.eot, 1.0)]]


def swap(tk):
    """Two live hypotheses that fork almost evenly and overtake each other a step later (the parent map holds a swap), and
    steps where one parent feeds two rows."""
    Z = tk.zero_sec
    return [[(Z, 1.0)], _tail([(X[0], 0.70), (X[1], 0.69)]),
            _tail([(X[2], 0.9)]), _tail([(X[3], 0.66), (X[4], 0.60)]), _tail([(X[5], 0.9)]),
            _tail([(Z + 50, 1.0)], ts0=Z + 60), _tail([(Z + 51, 1.0)], ts0=Z + 60), [(tk.eot, 1.0)]]


# Every weight below 1.0 is moved by a seeded amount in [-0.03, 0.03]: the seeds were searched on the CPU oracle (a few dozen
# each) for the largest smallest cut gap over K in 1, 2, 4, 5 that keeps the fixture's events; tests/test_beam_cpu.py checks
# both on every run.
JITTER_SEED = {"fork": 58, "closing": 18, "swap": 14}
JITTER = 0.03


def jittered(steps, seed):
    if not seed:
        return steps
    rng = np.random.default_rng(seed)
    return [[(t, w if w >= 1.0 else float(np.float32(w + rng.uniform(-JITTER, JITTER)))) for t, w in st] for st in steps]


def _fixture(fn, key):
    return lambda tk, seed=None: jittered(fn(tk), JITTER_SEED[key] if seed is None else seed)


FIXTURES = {"fork": _fixture(fork, "fork"), "closing": _fixture(closing, "closing"), "swap": _fixture(swap, "swap")}


def weighted_overrides(cfg, tk, steps, pos_rms=1.2, seed=0, peak_logit=14.0, prompt_len=3, n_prefix=0):
    """embed_tokens scaled as in common.scripted_overrides; embed_positions[n_prefix + prompt_len - 1 + i] steers step i towards
    steps[i] = [(token, weight), ...]."""
    emb = synth.synth_tensor_by_name(cfg, "model.decoder.embed_tokens.weight", seed)
    scale = max(1.0, peak_logit / (cfg.d_model * 0.02))
    emb = (emb * np.float32(scale)).astype(np.float16).astype(np.float32)
    gain = pos_rms / (0.02 * scale)
    pos = (0.02 * np.random.default_rng(991).standard_normal((cfg.max_target_positions, cfg.d_model))).astype(np.float32)
    for i, st in enumerate(steps):
        for t, w in st:
            pos[n_prefix + prompt_len - 1 + i] += np.float32(gain * w) * emb[t]
    return {"model.decoder.embed_tokens.weight": emb,
            "model.decoder.embed_positions.weight": pos.astype(np.float16).astype(np.float32)}


def oracle_step(om, xa):
    """search_ref's callback on the CPU oracle: decoder forward, final linear, fp64 softmax, the oracle's own rules."""
    def step(tokens, last_ts):
        h = om.decoder_forward(tokens, xa, True)
        lg = om.final_linear(h[-1:])[0].astype(np.float64)
        p = np.exp(lg - lg.max())
        p /= p.sum()
        return om.apply_rules(p.astype(np.float32), tokens, last_ts)
    return step


CLIP_SAMPLES = (480000, 200000, 300000)   # the three clips of the tests, of different lengths


def clips(n=3):
    return [synth.synth_pcm(k, CLIP_SAMPLES[k]) for k in range(n)]


def oracle_encodings(om, cfg, n=3):
    """the oracle's encoder output of every clip: what the GPU tests' reference searches and the CPU gap test both decode on"""
    from oracle import oracle as O
    from norma_amd import assets_io
    filt = assets_io.mel_filters(cfg.num_mel_bins)
    return [om.encoder_forward(O.pcm_to_mel(c, filt)[:, :3000]) for c in clips(n)]
