"""What token-level timestamps cost ("Cost"): distil-large-v3, 32 clips decoded to the cap, 6 alignment heads.

    python tools/dbg/align_cost.py lockstep    # nh_align against nh_align_decoded for the same batch; ms_per_step of
                                               # nh_decode_greedy with the capture on and off
    python tools/dbg/align_cost.py pool        # the varlen clips through one DecodePool, align_heads on and off

Prints one JSON line per part.  Times are host wall time around calls that return when the device is done (the align calls
copy their result back; decode_ms is the HIP-event time of the decode loop), medians of --reps runs after one warm-up."""
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
HEADS = [(0, 3), (0, 7), (1, 0), (1, 5), (1, 12), (1, 19)]


def med(f, reps):
    f()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def lockstep(reps, B=32):
    import common
    from norma_amd import config, hip, synth
    cfg, tk = config.preset(MODEL), common.tokens_for(MODEL)
    hm = common.build_hip(cfg, tk, max_batch=B)          # seed-0 weights: every sequence runs to the cap, as in bench.py b32
    hm.logmel_array(np.stack([synth.synth_pcm(k) for k in range(B)]))
    hm.encode()
    out = {"part": "lockstep", "model": MODEL, "batch": B, "heads": len(HEADS)}

    def decode_ms():
        res = hm.decode_greedy()
        t = hm.timings()
        return res, t["decode_ms"], t["decode_ms"] / t["decode_steps"]
    for name, heads in (("off", []), ("on", HEADS), ("off_again", [])):
        hm.align_capture(heads)
        decode_ms()
        runs = [decode_ms() for _ in range(reps)]
        out[f"decode_ms_capture_{name}"] = statistics.median(r[1] for r in runs)
        out[f"ms_per_step_capture_{name}"] = statistics.median(r[2] for r in runs)
    hm.align_capture(HEADS)
    res, _, _ = decode_ms()
    toks = [r["tokens"] for r in res]
    out["n_tokens"] = sorted({len(t) for t in toks})
    got = {}
    out["align_decoded_ms"] = med(lambda: got.__setitem__("d", hm.align_decoded()), reps)
    out["align_ms"] = med(lambda: got.__setitem__("a", hm.align(toks, prompt_len=3, heads=HEADS)), reps)
    out["same_times"] = bool(np.array_equal(got["d"][0], got["a"][0]) and np.array_equal(got["d"][1], got["a"][1]))
    hm.close()
    print(json.dumps(out), flush=True)


def pool_part(reps, rows=64, staging=32):
    import bench
    import common
    from norma_amd import assets_io, config, hip, pool, synth
    cfg, tk = config.preset(MODEL), common.tokens_for(MODEL)
    job = bench.WORKLOADS["varlen"][1]
    hm = hip.HipWhisper(cfg, device=0, max_batch=rows + staging)
    hm.set_mel_filters(assets_io.mel_filters(cfg.num_mel_bins))
    hm.set_tokens(tk, tk.en, tk.transcribe)
    spec = bench.varlen_spec(cfg, tk)                      # the varlen workload's weights, calibrated as bench.py does
    over0, _ = common.audio_overrides(cfg, tk, spec)
    for name, arr in synth.synth_weights(cfg, 0, over0):
        hm.load_tensor(name, arr.astype(np.float16))
    hm.logmel([synth.synth_pcm(k) for k in range(16)]); hm.encode()
    means = [hm.encoder_output(b).mean(0, keepdims=True) for b in range(16)]
    common.audio_calibrate(cfg, means, spec, vote=1.5)
    over, _ = common.audio_overrides(cfg, tk, spec)
    lastp = f"model.decoder.layers.{cfg.decoder_layers - 1}.encoder_attn.out_proj"
    for leaf in (".weight", ".bias"):
        hm.load_tensor(lastp + leaf, over[lastp + leaf].astype(np.float16))
    clips = np.stack([synth.synth_pcm(k) for k in range(job)])

    def encode(first, n, row0, must=True):
        hm.logmel_array_rows(np.ascontiguousarray(clips[first:first + n]), row0)
        hm.encode_rows(row0, n)
    out = {"part": "pool", "model": MODEL, "clips": job, "rows": rows, "staging": staging, "heads": len(HEADS)}
    last = {}
    for name, heads in (("off", None), ("on", HEADS), ("off_again", None)):
        if heads is None:
            hm.pool_begin(rows, 0, False); hm.align_capture([])

        def run():
            last[name] = pool.DecodePool(hm, rows=rows, staging=staging, align_heads=heads).run(job, encode)
        ms = med(run, reps)
        out[f"pool_ms_{name}"] = ms
        out[f"audio_s_per_s_{name}"] = job * 30.0 / (ms * 1e-3)
    out["same_tokens"] = all(a["tokens"] == b["tokens"] and a["avg_logprob"] == b["avg_logprob"] for a, b in zip(last["off"], last["on"]))
    out["timed_clips"] = sum(1 for r in last["on"] if "token_first" in r)
    hm.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["lockstep", "pool"])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    (lockstep if a.part == "lockstep" else pool_part)(a.reps)
