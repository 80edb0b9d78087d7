"""Fixtures of the repetition-guard tests: scripted weights (beam_fixture.weighted_overrides) whose decode walks into a loop --
the text block X0 X1 X2 again and again, with a pair of timestamps between the copies, as a looping Whisper window does.
Every text position also steers, with less weight, towards a runner-up of its own and a tail of further tokens, so that the
token a ban or a penalty hands the step to is decided with a margin too.

Every position is scripted and max_new_tokens is the script's length (see beam_fixture).
"""
import beam_fixture as F
import guard_ref as G

X = [1000, 2000, 3000]
RUNNERS = [4000, 5000, 6000, 7000, 8000, 9000, 1500, 2500, 3500, 4500, 5500, 6500]
THIRD = [11000, 12500, 13000]
COPIES = 4
RUNNER_W, THIRD_W = 0.75, 0.50

# The margin bar: every decision of every case must be at least this far (in log-probability) from its runner-up on the CPU
# oracle.  It is the beam fixtures' cut-gap bar (beam_fixture.G: ten times the largest device-vs-oracle difference of a
# cumulative score measured over those fixtures), which bounds a single step's difference a fortiori.
MARGIN = F.G


def loop_script(tk, copies=COPIES):
    Z = tk.zero_sec
    steps = [[(Z, 1.0)]]
    for c in range(copies):
        for k in range(3):
            steps.append([(X[k], 1.0), (RUNNERS[3 * c + k], RUNNER_W), (THIRD[k], THIRD_W)])
        if c + 1 < copies:
            steps.append(F._tail([(Z + 100 * (c + 1), 1.0)], ts0=Z + 100 * (c + 1) + 10))
            steps.append(F._tail([(Z + 100 * (c + 1) + 1, 1.0)], ts0=Z + 100 * (c + 1) + 10))
    steps.append([(tk.eot, 1.0)])
    return steps


# the guards of the decode tests: each component alone, and all together
BIAS = {X[1]: -6.0, RUNNERS[0]: 1.0, 12000: -float("inf")}
CASES = {
    "off": (G.params(), None),
    "ngram": (G.params(no_repeat_ngram=3), None),
    "penalty": (G.params(repetition_penalty=1.6), None),
    "bias": (G.params(bias=True), BIAS),
    "exit": (G.params(loop_period=3, loop_repeats=2), None),
    "all": (G.params(no_repeat_ngram=6, repetition_penalty=1.05, loop_period=4, loop_repeats=3, bias=True), {12000: -float("inf"), RUNNERS[1]: -1.0}),
}


PEAK_LOGIT = 22.0   # more peaked than the beam fixtures' 14: the runner-up of a banned text token must beat the timestamp mass


def overrides(cfg, tk, steps, **kw):
    return F.weighted_overrides(cfg, tk, steps, peak_logit=PEAK_LOGIT, **kw)


def oracle_logits(om, xa):
    """greedy_ref's callback on the CPU oracle"""
    def step(tokens):
        h = om.decoder_forward(tokens, xa, True)
        return om.final_linear(h[-1:])[0]
    return step
