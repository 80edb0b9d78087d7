"""What mapping the speech of a long recording costs through the library ("Measured"), beside what it replaces, and
what it saves end to end:

    python tools/dbg/vad_cost.py [--seconds 600] [--reps 10] [--model test-d128] [--max-new-tokens 32] [--no-end-to-end]

  call         HipWhisper.vad_plan on a device-resident recording: host wall time around nh_vad_plan, which returns when the
               piece and chunk records and the counts are on the host (the launches alone, per stage, under HIP events:
               tools/bin/vadbench)
  alternative  the recording copied from the device to host memory, then tests/vad_ref.py in numpy (the same arithmetic)
  end to end   longform.transcribe_speech against longform.transcribe_recording on the same recording: wall time and chunks.
               Seed-0 synthetic weights (bench.py's), so every chunk decodes to --max-new-tokens: the time is per chunk, and
               the chunk ratio is the recording's speech fraction

Prints one JSON line; medians of --reps runs after one warm-up.  The signal: noise bursts of 0.2 - 1.2 s at 0.3, separated by
pauses at 1e-3 of 0.5 s or, one time in four, 3 s (the defaults bridge the short ones)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def med(f, reps):
    f()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def recording(seconds, seed=0):
    r = np.random.default_rng([2024, seed])
    n = int(seconds * 16000)
    x = np.zeros(n, dtype=np.float32)
    at = 0
    while at < n:
        b = int(r.integers(3200, 19201))
        x[at:at + b] = r.uniform(-0.3, 0.3, size=len(x[at:at + b]))
        at += b
        p = 48000 if r.uniform() < 0.25 else 8000
        x[at:at + p] = r.uniform(-1e-3, 1e-3, size=len(x[at:at + p]))
        at += p
    x[np.abs(x) < 2.0 ** -40] = 0.0
    return x


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--model", default="test-d128")
    ap.add_argument("--max-new-tokens", type=int, default=32)
    ap.add_argument("--max-batch", type=int, default=32)
    ap.add_argument("--no-end-to-end", action="store_true")
    a = ap.parse_args()
    import vad_ref as VR
    from norma_amd import assets_io, config, hip, longform, synth, vocab
    x = recording(a.seconds)
    cfg = config.preset(a.model)
    hm = hip.HipWhisper(cfg, device=0, max_batch=a.max_batch)
    dev = hip.DeviceBuffer(x)
    rt = hip.DeviceBuffer.runtime()
    back = np.empty_like(x)
    plans = {}

    def call():
        plans["device"] = hm.vad_plan(dev.ptr, len(x))

    def copy():
        assert rt.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(dev.ptr), x.nbytes, 2) == 0   # hipMemcpyDeviceToHost

    def host():
        p = VR.plan(back)
        plans["host"] = (p.piece_starts, p.piece_lens, p.chunk_first)

    out = {"seconds": a.seconds, "samples": len(x), "params": list(VR.DEFAULTS), "reps": a.reps, "call_ms": med(call, a.reps),
           "copy_to_host_ms": med(copy, a.reps), "vad_ref_numpy_ms": med(host, max(1, a.reps // 3))}
    out["alternative_ms"] = out["copy_to_host_ms"] + out["vad_ref_numpy_ms"]
    out["pieces"], out["chunks"] = len(plans["device"][0]), len(plans["device"][2]) - 1
    out["kept_fraction"] = float(plans["device"][1].sum()) / len(x)
    out["same_plan"] = bool(all(np.array_equal(d, h) for d, h in zip(plans["device"], plans["host"])))
    if not a.no_end_to_end:
        tk = vocab.VOCABS[config.preset_vocab(a.model)]
        hm.load_weights((n, w.astype(np.float16)) for n, w in synth.synth_weights(cfg, 0))
        hm.set_mel_filters(assets_io.mel_filters(cfg.num_mel_bins))
        hm.set_tokens(tk, tk.en, tk.transcribe)
        runs = {}

        def speech():
            runs["speech"] = longform.transcribe_speech(hm, (dev.ptr, len(x)), None, a.max_new_tokens)

        def whole():
            runs["recording"] = longform.transcribe_recording(hm, (dev.ptr, len(x)), None, a.max_new_tokens)

        reps = max(1, a.reps // 3)
        out.update(model=a.model, weights="seed-0 synthetic", max_new_tokens=a.max_new_tokens, max_batch=a.max_batch,
                   transcribe_recording_ms=med(whole, reps), transcribe_speech_ms=med(speech, reps),
                   transcribe_recording_ms_again=med(whole, reps), transcribe_speech_ms_again=med(speech, reps),
                   recording_chunks=len(runs["recording"]), speech_chunks=len(runs["speech"]))
    print(json.dumps(out), flush=True)
    dev.free()
    hm.close()
