"""What a decoder prompt costs ("Cost"): distil-large-v3 with the seed-0 synthetic weights, 32 clips in lockstep
(the bench shape: every sequence runs to the length cap), prefixes of 8, 32 and 223 tokens by default.

    python tools/dbg/prompt_cost.py [--reps 5] [--prefixes 8 32 223] [--out profiles/prompt_cost.json]

Per prefix length n, alternating the variants inside one process:
  prefix_ms_onepass / prefix_ms_stepwise   the prefix alone: decode_ms of a decode cut to ONE generated token under the prefix
                                           (one pass; NH_OPT_PROMPT_STEPWISE = 1: the decode step once per position, which
                                           is what the code before this feature would have had to do) minus the decode_ms
                                           of the same decode with no prefix
  decode_ms_prompted_*                     a whole prompted decode, to the cap: n prefix positions + the positions from sot on
  decode_ms_unprompted                     a decode with no prefix, to the cap: the same physical length, every position a step
decode_ms is the HIP-event time of nh_decode_* (from the reset of the decode state to the last step), medians of --reps runs
after one warm-up run of every variant.  A decode under another prefix length than the one before captures its step graphs
again, inside decode_ms (about 0.5 ms), so every timed run follows an untimed run of the same variant.  Prints one JSON line
and, with --out, writes it to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

MODEL = "distil-large-v3"
PREFIXES = (8, 32, 223)


def main(reps, out_path, prefixes=PREFIXES, B=32):
    import common
    from norma_amd import config, hip, synth
    if hip.device_count() < 1:
        raise SystemExit("prompt_cost: no MI355X visible; there is nothing to measure without one")
    cfg, tk = config.preset(MODEL), common.tokens_for(MODEL)
    hm = common.build_hip(cfg, tk, max_batch=B)
    hm.logmel_array(np.stack([synth.synth_pcm(k) for k in range(B)]))
    hm.encode()
    rng = np.random.default_rng(5)

    def run(n, stepwise, max_new):
        hm.set_option(hip.NH_OPT_PROMPT_STEPWISE, stepwise)
        hm.set_prompts(None if n == 0 else [[tk.no_speech - 1] + [int(t) for t in rng.integers(300, 40000, size=n - 1)] for _ in range(B)])
        res = hm.decode_greedy(max_new)
        t = hm.timings()
        return t["decode_ms"], t["decode_steps"], sorted({len(r["tokens"]) for r in res})

    out = {"tool": "prompt_cost", "model": MODEL, "batch": B, "reps": reps, "prefixes": {}}
    for n in prefixes:
        variants = {"base1": (0, 0, 1), "onepass1": (n, 0, 1), "stepwise1": (n, 1, 1),
                    "unprompted": (0, 0, 0), "prompted_onepass": (n, 0, 0), "prompted_stepwise": (n, 1, 0)}
        times = {k: [] for k in variants}
        shape = {}
        for rep in range(reps + 1):               # rep 0 warms every variant up
            for k, v in variants.items():         # alternating: drift of the clock hits every variant alike
                run(*v)                           # a new prefix length captures its step graphs inside decode_ms: not timed
                ms, steps, lens = run(*v)
                shape[k] = (steps, lens)
                if rep:
                    times[k].append(ms)
        m = {k: statistics.median(v) for k, v in times.items()}
        spread = {k: max(v) - min(v) for k, v in times.items()}
        out["prefixes"][str(n)] = {
            "prefix_ms_onepass": m["onepass1"] - m["base1"], "prefix_ms_stepwise": m["stepwise1"] - m["base1"],
            "stepwise_over_onepass": (m["stepwise1"] - m["base1"]) / max(m["onepass1"] - m["base1"], 1e-9),
            "decode_ms_unprompted": m["unprompted"], "decode_ms_prompted_onepass": m["prompted_onepass"],
            "decode_ms_prompted_stepwise": m["prompted_stepwise"],
            "medians_ms": m, "max_minus_min_ms": spread,
            "steps_and_returned_lengths": {k: shape[k] for k in ("unprompted", "prompted_onepass", "prompted_stepwise")}}
    hm.close()
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--prefixes", type=int, nargs="+", default=list(PREFIXES))
    a = ap.parse_args()
    main(a.reps, a.out, a.prefixes)
