"""What scoring a transcript costs ("Cost"): distil-large-v3 with the seed-0 synthetic weights, 32 clips,
sequences of 128 tokens.  The protocol is tools/dbg/beam_cost.py's: eot and every timestamp are on the suppress list, so every
greedy decode runs to max_new_tokens = 124 and returns [sot, language, task] + 124 tokens + the forced eot = 128 tokens; nh_score
then scores exactly those sequences, i.e. the same 127 positions the decode stepped through.

    python tools/dbg/score_cost.py [--reps 5] [--kernel-split] [--out profiles/score_cost.json]

Two calls, alternating inside one process on one context, medians of --reps runs after one warm-up of each:
  decode   nh_decode_greedy (captured step graphs, the default)
  score    nh_score on what the decode returned
Both are timed with a host clock around the call -- each ends in a stream synchronise and a copy of its results --; the decode's
own HIP-event time (nh_timings.decode_ms) is reported beside it.  The condition of the design is score <= decode / 2.
--kernel-split: two runs of their own under `rocprofv3 --kernel-trace --stats` (a child process that encodes, decodes once and
scores 2 and 6 times) give, by difference, the device time per call of the two scoring kernels and of everything else the call
launches (the one-pass forward).
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
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

MODEL = "distil-large-v3"
B, MAX_NEW, N_TOKENS = 32, 124, 128


def build():
    import common
    from norma_amd import config, hip
    if hip.device_count() < 1:
        raise SystemExit("score_cost: no MI355X visible; there is nothing to measure without one")
    cfg, tk = config.preset(MODEL), common.tokens_for(MODEL)
    hm = common.build_hip(cfg, tk, max_batch=B)
    # nothing ends before max_new_tokens: no eot, and no timestamp to run out of
    hm.set_tokens(tk, tk.en, tk.transcribe, suppress=list(cfg.suppress_tokens) + [tk.eot] + list(range(tk.no_timestamps + 1, cfg.vocab_size)))
    from norma_amd import synth
    hm.logmel_array(np.stack([synth.synth_pcm(k % 8) for k in range(B)]))
    hm.encode()
    return cfg, hm


def flops(cfg, rows, T):
    """algorithmic FLOPs of one nh_score call on `rows` = B * T rows: the projection, and the decoder blocks of the forward"""
    d, V, S, L = cfg.d_model, cfg.vocab_size, cfg.max_source_positions, cfg.decoder_layers
    proj = 2.0 * rows * V * d
    gemms = 2.0 * rows * d * d * (3 + 1 + 1 + 1 + 4 + 4)          # qkv, o, cross q, cross o, fc1, fc2
    attn = 2.0 * 2.0 * rows * d * (T / 2.0 + S)                    # q.k and p.v over the causal half and the S cross keys
    return proj, L * (gemms + attn)


def child(reps):
    """scores alone, for the kernel trace"""
    cfg, hm = build()
    seqs = [r["tokens"] for r in hm.decode_greedy(MAX_NEW)]
    for _ in range(reps + 1):
        hm.score(seqs)
    print(json.dumps({"scores": reps + 1, "n_tokens": sorted({len(s) for s in seqs})}), flush=True)
    hm.close()


def traced(reps):
    """kernel name -> total ns of a child that scores reps + 1 times"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "score", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError((r.stderr or r.stdout)[-400:])
        info = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("no kernel_stats.csv written")
        with open(files[0]) as f:
            return info, {row["Name"]: float(row["TotalDurationNs"]) for row in csv.DictReader(f)}


def kernel_split(few=1, many=5):
    """The child also encodes and decodes once, with kernels the forward shares (GEMM, LayerNorm, embed): two traced runs that
    differ only in the number of scores, and per kernel the difference over the extra scores."""
    try:
        (info, a), (_, b) = traced(few), traced(many)
    except RuntimeError as e:
        return {"error": str(e)}
    extra = many - few
    per = {name: (b[name] - a.get(name, 0.0)) / 1e6 / extra for name in b}
    out = {"scores_traced": [few + 1, many + 1], "n_tokens": info["n_tokens"]}
    total = 0.0
    for key in ("score_logits_kernel", "score_merge_kernel"):
        out[key + "_ms"] = sum(ms for name, ms in per.items() if key in name)
        total += out[key + "_ms"]
    out["forward_ms"] = sum(ms for name, ms in per.items() if "score_" not in name)
    out["forward_largest"] = sorted(((round(ms, 4), name.split("(")[0][:48]) for name, ms in per.items() if "score_" not in name), reverse=True)[:5]
    out["all_kernels_ms"] = total + out["forward_ms"]
    return out


def main(reps, out_path, split):
    cfg, hm = build()
    times = {"decode_wall": [], "decode_event": [], "score_wall": []}
    seqs, steps = None, 0
    for rep in range(reps + 1):          # rep 0 warms both up (graph capture, the score buffers)
        t0 = time.perf_counter()
        res = hm.decode_greedy(MAX_NEW)
        t1 = time.perf_counter()
        tm = hm.timings()
        seqs, steps = [r["tokens"] for r in res], tm["decode_steps"]
        t2 = time.perf_counter()
        lp = hm.score(seqs)
        t3 = time.perf_counter()
        if rep:
            times["decode_wall"].append((t1 - t0) * 1e3)
            times["decode_event"].append(tm["decode_ms"])
            times["score_wall"].append((t3 - t2) * 1e3)
    hm.close()
    lens = sorted({len(s) for s in seqs})
    med = {k: statistics.median(v) for k, v in times.items()}
    proj, fwd = flops(cfg, B * (lens[-1] - 1), lens[-1] - 1)
    out = {"tool": "score_cost", "model": MODEL, "batch": B, "max_new_tokens": MAX_NEW, "reps": reps,
           "returned_lengths": lens, "sequences_are_128_tokens": lens == [N_TOKENS], "decode_steps": steps,
           "finite": bool(np.isfinite(lp).all()),
           "ms": med, "max_minus_min_ms": {k: max(v) - min(v) for k, v in times.items()},
           "score_over_decode": med["score_wall"] / med["decode_wall"],
           "condition_score_at_most_half_the_decode": med["score_wall"] <= 0.5 * med["decode_wall"],
           "flops": {"projection": proj, "forward": fwd}}
    if split:
        ks = kernel_split()
        out["kernel_split"] = ks
        if "score_logits_kernel_ms" in ks:
            out["projection_tflops_per_s"] = proj / (ks["score_logits_kernel_ms"] * 1e-3) / 1e12
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
