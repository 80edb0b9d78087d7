"""What a beam step costs ("Cost"): distil-large-v3 with the seed-0 synthetic weights, max_new_tokens 128.
eot and every timestamp are put on the suppress list for this measurement: after the first token (a timestamp from the
window, which looks at no list) every row is in the "last token is text" state, the selection's longest path, and no
hypothesis ends before max_new_tokens.  So every decode runs the same number of steps, and from its second step on (the
first expands 16 hypotheses into 80) the beam decode has all 80 rows live in every step, as the greedy yardstick has.
Without that the flat synthetic distributions walk the timestamps to the last one within some thirty steps, where a beam
has nothing left to choose and its clip ends, most steps run at few live rows, and the beam step looks cheaper than it is.  The result says
whether that held: `steps_equal` (all decodes ran the same number of steps) and `beam_rows_live_throughout` (every clip
finished K hypotheses, all of the full length).

    python tools/dbg/beam_cost.py [--reps 5] [--kernel-split] [--out profiles/beam_cost.json]

Three decodes, alternating inside one process on one context of 80 rows:
  greedy_b16    nh_decode_greedy, 16 clips                 the search a beam replaces
  greedy_b80    nh_decode_greedy, 80 clips                 the yardstick: a greedy step at the beam's row count
  beam5_b16     nh_decode_beam, K = 5, 16 clips            80 rows; eager launches
ms per step = decode_ms / decode_steps, decode_ms the HIP-event time of the decode (state reset to last step), medians of
--reps runs after one warm-up of every variant; the greedy decodes replay captured graphs (the default), and
greedy_b80_eager repeats the yardstick with NH_OPT_DECODE_GRAPHS = 0, launch for launch what the beam loop does up to the logits.
--kernel-split: a run of its own under `rocprofv3 --kernel-trace --stats` (a child process that only does beam decodes) gives
the device time of the three beam kernels per call, one call of each per step: selection + merge, and the cache reorder.
Prints one JSON line and, with --out, writes it to a file."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

MODEL = "distil-large-v3"
MAX_NEW, K, B_SMALL, B_ROWS = 128, 5, 16, 80
NH_OPT_DECODE_GRAPHS = 0


def build(rows):
    import common
    from norma_amd import config, hip
    if hip.device_count() < 1:
        raise SystemExit("beam_cost: no MI355X visible; there is nothing to measure without one")
    cfg, tk = config.preset(MODEL), common.tokens_for(MODEL)
    hm = common.build_hip(cfg, tk, max_batch=rows)
    # nothing ends before max_new_tokens: no eot, and no timestamp to run out of
    hm.set_tokens(tk, tk.en, tk.transcribe, suppress=list(cfg.suppress_tokens) + [tk.eot] + list(range(tk.no_timestamps + 1, cfg.vocab_size)))
    return hm


def encode(hm, n):
    from norma_amd import synth
    hm.logmel_array(np.stack([synth.synth_pcm(k % 8) for k in range(n)]))
    hm.encode()


def child(reps):
    """beam decodes alone, for the kernel trace"""
    hm = build(B_ROWS)
    encode(hm, B_SMALL)
    steps = 0
    for _ in range(reps + 1):
        hm.decode_beam(K, MAX_NEW)
        steps = hm.timings()["decode_steps"]
    print(json.dumps({"decodes": reps + 1, "steps_per_decode": steps}), flush=True)
    hm.close()


def kernel_split(reps):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "beam", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {"error": (r.stderr or r.stdout)[-400:]}
        info = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no kernel_stats.csv written"}
        rows = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                rows[row["Name"]] = (int(row["Calls"]), float(row["TotalDurationNs"]))
        out = {"steps_per_decode": info["steps_per_decode"], "decodes": info["decodes"]}
        for key in ("beam_select_kernel", "beam_merge_kernel", "beam_reorder_kernel"):
            hit = [(c, ns) for n, (c, ns) in rows.items() if key in n]
            calls, ns = sum(c for c, _ in hit), sum(ns for _, ns in hit)
            out[key] = {"calls": calls, "us_per_call": ns / 1e3 / max(calls, 1)}
        out["beam_kernels_us_per_step"] = sum(out[k]["us_per_call"] for k in ("beam_select_kernel", "beam_merge_kernel", "beam_reorder_kernel"))
        return out


def main(reps, out_path, split):
    hm = build(B_ROWS)

    def run(kind):
        from norma_amd import hip
        hm.set_option(NH_OPT_DECODE_GRAPHS, 0 if kind.endswith("eager") else 1)
        encode(hm, B_ROWS if "b80" in kind else B_SMALL)
        res = hm.decode_beam(K, MAX_NEW) if kind.startswith("beam") else hm.decode_greedy(MAX_NEW)
        t = hm.timings()
        if kind.startswith("beam"):      # every hypothesis of every clip ran to max_new_tokens: K finished ones of one length
            full = {len(t) for r in res for t, _ in r["hypotheses"]}
            live_throughout.append(all(len(r["hypotheses"]) == K for r in res) and len(full) == 1)
        return t["decode_ms"], t["decode_steps"], sorted({len(r["tokens"]) for r in res})

    live_throughout = []
    kinds = ("greedy_b16", "greedy_b80", "greedy_b80_eager", "beam5_b16")
    times, shape = {k: [] for k in kinds}, {}
    for rep in range(reps + 1):          # rep 0 warms every variant up (graph capture, buffers)
        for k in kinds:                  # alternating: drift of the clock hits every variant alike
            if rep == 0:
                run(k)
            ms, steps, lens = run(k)
            shape[k] = (steps, lens)
            if rep:
                times[k].append(ms / steps)
    hm.set_option(NH_OPT_DECODE_GRAPHS, 1)
    hm.close()
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"tool": "beam_cost", "model": MODEL, "max_new_tokens": MAX_NEW, "beam_size": K, "reps": reps,
           "eot_and_timestamps_suppressed": True, "beam_live_rows": "16 in the first generation step, 80 in every later one",
           "steps_equal": len({steps for steps, _ in shape.values()}) == 1, "beam_rows_live_throughout": all(live_throughout),
           "ms_per_step": med, "max_minus_min_ms_per_step": {k: max(v) - min(v) for k, v in times.items()},
           "steps_and_returned_lengths": shape,
           "beam_over_greedy_at_equal_rows": med["beam5_b16"] / med["greedy_b80"],
           "beam_over_eager_greedy_at_equal_rows": med["beam5_b16"] / med["greedy_b80_eager"]}
    if split:
        out["kernel_split"] = kernel_split(2)
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-split", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.reps)
    else:
        main(a.reps, a.out, a.kernel_split)
