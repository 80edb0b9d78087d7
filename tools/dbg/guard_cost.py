"""What the repetition guard costs per decode step ("Measurements"): distil-large-v3 with the seed-0 synthetic
weights, max_new_tokens 128, eot suppressed so that every decode runs the same number of steps (tools/dbg/beam_cost.py has the
reasoning).

    python tools/dbg/guard_cost.py [--reps 5] [--rounds 3] [--parent-root DIR] [--out profiles/guard_cost.json]

Every measurement is a child process (one build per process), and the children alternate, so drift of the clock hits every
variant alike.  A child measures, alternating inside its process, after one warm-up of each:
  lockstep_off / lockstep_on     nh_decode_greedy of 32 clips (the headline's lockstep shape): decode_ms / decode_steps of
                                 nh_timings (HIP events), guard off / on
  pool_off / pool_on             64 pool rows all generating: wall time of nh_pool_step(96) / 96 (the call drains the stream)
  load_off / load_on             lockstep as above while two more contexts on the same weights decode in threads of their own
                                 (three batches in flight, as bench.py keeps them), all three with the guard off / on
"on" is no-repeat 3-gram + penalty 1.1 + loop exit (8, 3): all three stages that read the history, one launch per step.
With --parent-root (a built checkout of the parent commit) children that import THAT tree -- which has no guard and measures
the *_off variants only -- alternate with this commit's for --rounds rounds: the off path of this commit against
the parent, to be read against the spread of the parent's own rounds.
Prints one JSON line and, with --out, writes it to a file."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import threading
import time

# a child imports the tree it is told to measure (--parent-root); everything else this one
ROOT = os.environ.get("GUARD_COST_ROOT") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

MODEL = "distil-large-v3"
MAX_NEW, B, POOL_ROWS, POOL_STEPS = 128, 32, 64, 96
GUARD = dict(no_repeat_ngram=3, repetition_penalty=1.1, loop_period=8, loop_repeats=3)


def child(reps):
    import common
    from norma_amd import config, hip, synth
    if hip.device_count() < 1:
        raise SystemExit("guard_cost: no MI355X visible; there is nothing to measure without one")
    cfg, tk = config.preset(MODEL), common.tokens_for(MODEL)
    sup = list(cfg.suppress_tokens) + [tk.eot]
    hm = common.build_hip(cfg, tk, max_batch=B)
    hm.set_tokens(tk, tk.en, tk.transcribe, suppress=sup)
    has_guard = hasattr(hm, "set_guard")
    clips = np.stack([synth.synth_pcm(k % 8) for k in range(B)])
    hm.logmel_array(clips); hm.encode()
    others = []
    for _ in range(2):
        h = hip.HipWhisper(cfg, device=0, max_batch=B, share_with=hm)
        h.set_tokens(tk, tk.en, tk.transcribe, suppress=sup)
        h.logmel_array(clips); h.encode()
        others.append(h)
    hp = hip.HipWhisper(cfg, device=0, max_batch=POOL_ROWS + B, share_with=hm)
    hp.set_tokens(tk, tk.en, tk.transcribe, suppress=sup)

    def lockstep(on):
        if has_guard:
            hm.set_guard(**GUARD) if on else hm.set_guard(None)
        # a change of the guard moves the graph key: the next decode captures its steps again, on the host, between the two
        # events decode_ms is taken from.  That decode is not the measured one (the parent's children do the same two).
        hm.decode_greedy(MAX_NEW)
        hm.decode_greedy(MAX_NEW)
        t = hm.timings()
        return t["decode_ms"] / t["decode_steps"], t["decode_steps"]

    def pooled(on):
        hp.pool_begin(POOL_ROWS, 0, False)
        if has_guard:
            hp.set_guard(**GUARD) if on else hp.set_guard(None)
        for g in range(POOL_ROWS // B):
            hp.logmel_array_rows(clips, POOL_ROWS); hp.encode_rows(POOL_ROWS, B)
            for i in range(B):
                hp.pool_admit(POOL_ROWS + i, g * B + i)
        hp.pool_step(8)                      # probe and prompt behind every row: all 64 generate from here on
        hp.synchronize()
        t0 = time.perf_counter()
        hp.pool_step(POOL_STEPS)
        return (time.perf_counter() - t0) * 1e3 / POOL_STEPS, POOL_STEPS

    def spin(h, stop, flip):
        """decode until told to stop; the guard follows the measured context's (flip[0], read between decodes)"""
        on = None
        while not stop.is_set():
            if has_guard and flip[0] != on:
                on = flip[0]
                h.set_guard(**GUARD) if on else h.set_guard(None)
            h.decode_greedy(MAX_NEW)
        if has_guard:
            h.set_guard(None)

    kinds = [("lockstep", lockstep), ("pool", pooled)]
    variants = (False, True) if has_guard else (False,)
    times, steps = {}, {}
    for phase in ("", "load"):
        threads, stop, flip = [], threading.Event(), [False]
        if phase:
            threads = [threading.Thread(target=spin, args=(h, stop, flip)) for h in others]
            for th in threads:
                th.start()
        for rep in range(reps + 1):          # rep 0 warms every variant up (graph capture under its key)
            for name, fn in (kinds if not phase else kinds[:1]):
                for on in variants:
                    key = f"{phase or name}_{'on' if on else 'off'}"
                    if phase:
                        flip[0] = on         # the other two contexts switch over during the unmeasured decode of fn
                    ms, n = fn(on)
                    steps[key] = n
                    if rep:
                        times.setdefault(key, []).append(ms)
        stop.set()
        for th in threads:
            th.join()
    print(json.dumps({"has_guard": has_guard, "ms_per_step": times, "steps": steps}), flush=True)
    for h in others + [hp, hm]:
        h.close()


def run_child(root, reps):
    env = dict(os.environ)
    if root:
        env["GUARD_COST_ROOT"] = os.path.abspath(root)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)], env=env, capture_output=True,
                       text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("guard_cost child failed: " + (r.stderr or r.stdout)[-600:])
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main(reps, rounds, parent_root, out_path):
    runs = {"this": [], "parent": []}
    for _ in range(rounds if parent_root else 1):
        if parent_root:
            runs["parent"].append(run_child(parent_root, reps))
        runs["this"].append(run_child(None, reps))
    med = lambda v: statistics.median(v)
    out = {"tool": "guard_cost", "model": MODEL, "max_new_tokens": MAX_NEW, "lockstep_clips": B, "pool_rows": POOL_ROWS,
           "guard_on": GUARD, "reps": reps, "rounds": len(runs["this"]), "steps": runs["this"][0]["steps"]}
    for who in ("this", "parent"):
        if not runs[who]:
            continue
        keys = sorted(runs[who][0]["ms_per_step"])
        per_round = {k: [med(r["ms_per_step"][k]) for r in runs[who]] for k in keys}
        out[who] = {"ms_per_step_median_per_round": per_round, "ms_per_step": {k: med(v) for k, v in per_round.items()},
                    "spread_over_rounds": {k: max(v) - min(v) for k, v in per_round.items()},
                    "max_minus_min_within_a_round": {k: max(max(r["ms_per_step"][k]) - min(r["ms_per_step"][k]) for r in runs[who]) for k in keys}}
    t = out["this"]["ms_per_step"]
    out["guard_us_per_step"] = {k: (t[f"{k}_on"] - t[f"{k}_off"]) * 1e3 for k in ("lockstep", "pool", "load")}
    if runs["parent"]:
        p = out["parent"]["ms_per_step"]
        out["off_minus_parent_us_per_step"] = {k: (t[k] - p[k]) * 1e3 for k in p}
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.reps)
    else:
        main(a.reps, a.rounds, a.parent_root, a.out)
