"""What a prompt prefix per pool row costs ("Pool rows"): distil-large-v3 with the seed-0 synthetic weights, a decode
pool of 32 rows over 64 clips (staging 32), every clip under its own 223-token prefix (nh_pool_prefix).

    python tools/dbg/pool_prompt_cost.py [--reps 5] [--out profiles/pool_prompt_cost.json]

Variants, alternating inside one process, each timed run behind an untimed run of the same variant:
  onepass_64 / stepwise_64     max_new_tokens = 64: the default route (one ragged one-pass prefill per group of admissions)
                               against NH_OPT_PROMPT_STEPWISE = 1 (every prefix position a step of the pool)
  onepass_cap / stepwise_cap   the same to the length cap (the seed-0 weights never emit eot: 225 positions from sot on)
  plain_64 / plain_cap         no prefix: what the pool did before, for scale
Per variant: decode_wall_ms, the wall time of DecodePool.run minus the time inside its encode callback (log-mel + encoder of 32
clips, drained before the callback returns, the same work in every variant), median of --reps; and row_steps, the pool's
sum over steps of busy rows.  Prints one JSON line and, with --out, writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

MODEL = "distil-large-v3"


def main(reps, out_path, rows=32, n_clips=64, n_prefix=223):
    import common
    from norma_amd import config, hip, pool, synth
    if hip.device_count() < 1:
        raise SystemExit("pool_prompt_cost: no MI355X visible; there is nothing to measure without one")
    cfg, tk = config.preset(MODEL), common.tokens_for(MODEL)
    hm = common.build_hip(cfg, tk, max_batch=2 * rows)
    clips = np.stack([synth.synth_pcm(k % 8) for k in range(n_clips)])
    rng = np.random.default_rng(5)
    prefixes = [[tk.no_speech - 1] + [int(t) for t in rng.integers(300, 40000, size=n_prefix - 1)] for _ in range(n_clips)]

    def run(prefixed, stepwise, max_new):
        hm.set_option(hip.NH_OPT_PROMPT_STEPWISE, stepwise)
        spent = [0.0]

        def encode(first, n, row0, must=True):
            t0 = time.perf_counter()
            hm.logmel_array_rows(np.ascontiguousarray(clips[first:first + n]), row0)
            hm.encode_rows(row0, n)
            hm.synchronize()
            spent[0] += time.perf_counter() - t0
        dp = pool.DecodePool(hm, rows=rows, staging=rows, max_new_tokens=max_new, check_every=16,
                             prefix=(lambda c, prev: prefixes[c]) if prefixed else None)
        t0 = time.perf_counter()
        res = dp.run(n_clips, encode)
        wall = time.perf_counter() - t0
        return (wall - spent[0]) * 1e3, dp.row_steps, sorted({len(r["tokens"]) for r in res})

    variants = {"plain_64": (False, 0, 64), "onepass_64": (True, 0, 64), "stepwise_64": (True, 1, 64),
                "plain_cap": (False, 0, 0), "onepass_cap": (True, 0, 0), "stepwise_cap": (True, 1, 0)}
    times = {k: [] for k in variants}
    shape = {}
    for rep in range(reps):
        for k, v in variants.items():   # alternating: drift of the clock hits every variant alike
            run(*v)                     # untimed: the step graphs of this max_new_tokens are captured here
            ms, row_steps, lens = run(*v)
            times[k].append(ms)
            shape[k] = (row_steps, lens)
    hm.close()
    out = {"tool": "pool_prompt_cost", "model": MODEL, "rows": rows, "clips": n_clips, "n_prefix": n_prefix, "reps": reps,
           "variants": {k: {"decode_wall_ms": statistics.median(times[k]), "max_minus_min_ms": max(times[k]) - min(times[k]),
                            "row_steps": shape[k][0], "returned_lengths": shape[k][1]} for k in variants}}
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    main(a.reps, a.out)
