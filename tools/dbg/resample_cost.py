"""What audio ingest on the device costs ("Cost"): 32 clips of 30 s, 48 000 Hz stereo i16 and 44 100 Hz stereo
f32, on a test-d128 context (nothing here depends on the model's size: the log-mel has 80 bins either way).

    python tools/dbg/resample_cost.py launch [--read-gbs R]   # the resample launch alone, device-resident frames, beside its
                                                               # byte floor at R GB/s (the read rate tools/bin/peaks attains)
    python tools/dbg/resample_cost.py logmel                   # logmel_resampled against logmel_device on pre-resampled PCM and
                                                               # logmel on host f32; the same batch as host native frames
    python tools/dbg/resample_cost.py samples                  # logmel_samples on 32 x 30 s of host mono i16 at 16 kHz (the
                                                               # conversion route: nothing to mix down or resample)
    python tools/dbg/resample_cost.py scipy                    # the host alternative: scipy.signal.resample_poly, 16 threads

Prints one JSON line per format.  Times are host wall time around calls followed by a stream synchronisation, medians of
--reps runs after one warm-up."""
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

B, SECONDS = 32, 30
FORMATS = (("48000 Hz stereo i16", 48000, np.int16), ("44100 Hz stereo f32", 44100, np.float32))


def med(f, reps):
    f()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def frames_of(src_hz, dtype):
    """[B][30 s][2]: a few tones per clip, the right channel a scaled copy (the content does not change the work)"""
    n = src_hz * SECONDS
    t = np.arange(n) / src_hz
    out = np.empty((B, n, 2), dtype=dtype)
    for b in range(B):
        x = 0.3 * np.sin(2 * np.pi * (200 + 37 * b) * t) + 0.2 * np.sin(2 * np.pi * (2100 + 91 * b) * t)
        st = np.stack([x, 0.7 * x], axis=1)
        out[b] = st.astype(np.float32) if dtype == np.float32 else np.round(st * 32767).astype(np.int16)
    return out


def context():
    import common
    from norma_amd import config
    cfg, tk = config.preset("test-d128"), common.tokens_for("test-d128")
    return common.build_hip(cfg, tk, max_batch=B)


def launch_part(reps, read_gbs):
    from norma_amd import hip
    hm = context()
    for name, src_hz, dtype in FORMATS:
        fr = frames_of(src_hz, dtype)
        dev = hip.DeviceBuffer(fr)
        nf = np.full(B, fr.shape[1], dtype=np.int32)
        n_out = hm.L.nh_resample_len(src_hz, fr.shape[1])

        def run():
            hm._chk(hm.L.nh_resample(hm._h, C.c_void_p(dev.ptr), 1, hip.SAMPLE_DTYPES[np.dtype(dtype)], 2, src_hz,
                                     nf.ctypes.data_as(C.POINTER(C.c_int32)), fr.shape[1], B, None, None, None, 0))
            hm.synchronize()
        ms = med(run, reps)
        moved = fr.nbytes + 4.0 * B * n_out
        out = {"part": "launch", "format": name, "clips": B, "n_out": n_out, "taps": hm.resample_table(src_hz)[3], "ms": ms,
               "bytes_in": fr.nbytes, "bytes_out": 4 * B * n_out, "gb_per_s": moved / ms * 1e-6}
        if read_gbs:
            out["floor_ms"] = moved / read_gbs * 1e-6
            out["ratio_to_floor"] = ms / out["floor_ms"]
        print(json.dumps(out), flush=True)
        dev.free()
    hm.close()


def logmel_part(reps):
    from norma_amd import hip
    hm = context()
    for name, src_hz, dtype in FORMATS:
        fr = frames_of(src_hz, dtype)
        dev = hip.DeviceBuffer(fr)
        nf = [fr.shape[1]] * B
        pcm = np.stack(hm.resample(dev.ptr, src_hz, n_frames=nf, stride_frames=fr.shape[1], dtype=dtype, channels=2))
        pcm_dev = hip.DeviceBuffer(pcm)
        ns = [pcm.shape[1]] * B

        def sync(f):
            def g():
                f()
                hm.synchronize()
            return g
        out = {"part": "logmel", "format": name, "clips": B,
               "logmel_resampled_device_frames_ms": med(sync(lambda: hm.logmel_resampled(dev.ptr, src_hz, n_frames=nf, stride_frames=fr.shape[1], dtype=dtype, channels=2)), reps),
               "logmel_device_16k_pcm_ms": med(sync(lambda: hm.logmel_device(pcm_dev.ptr, ns, pcm.shape[1])), reps),
               "logmel_host_16k_f32_ms": med(sync(lambda: hm.logmel_array(pcm)), reps),
               "logmel_resampled_host_frames_ms": med(sync(lambda: hm.logmel_resampled(fr, src_hz)), reps),
               "host_frames_mb": fr.nbytes / 1e6, "host_16k_f32_mb": pcm.nbytes / 1e6}
        print(json.dumps(out), flush=True)
        dev.free(); pcm_dev.free()
    hm.close()


def samples_part(reps):
    hm = context()
    t = np.arange(16000 * SECONDS) / 16000.0
    pcm = np.stack([np.round(32767 * (0.3 * np.sin(2 * np.pi * (200 + 37 * b) * t) + 0.2 * np.sin(2 * np.pi * (2100 + 91 * b) * t)))
                    for b in range(B)]).astype(np.int16)

    def run():
        hm.logmel_samples(pcm)
        hm.synchronize()
    print(json.dumps({"part": "samples", "format": "16000 Hz mono i16", "clips": B, "logmel_samples_host_ms": med(run, reps),
                      "host_samples_mb": pcm.nbytes / 1e6}), flush=True)
    hm.close()


def scipy_part(reps, threads=16):
    from concurrent.futures import ThreadPoolExecutor
    import resample_ref as RR
    try:
        from scipy.signal import resample_poly
    except ImportError:
        print(json.dumps({"part": "scipy", "error": "scipy is not installed"}), flush=True)
        return
    for name, src_hz, dtype in FORMATS:
        fr = frames_of(src_hz, dtype)
        L, M = RR.design(src_hz)[:2]
        scale = np.float32(1.0 if dtype == np.float32 else 1.0 / 32768.0)

        def one(b):
            return resample_poly((fr[b].astype(np.float32) * scale).mean(axis=1), L, M).astype(np.float32)

        def run():
            with ThreadPoolExecutor(threads) as ex:
                list(ex.map(one, range(B)))
        print(json.dumps({"part": "scipy", "format": name, "clips": B, "threads": threads, "ms": med(run, reps)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["launch", "logmel", "samples", "scipy"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--read-gbs", type=float, default=0.0, help="read rate of tools/bin/peaks on this device, GB/s")
    a = ap.parse_args()
    if a.part == "launch":
        launch_part(a.reps, a.read_gbs)
    elif a.part == "logmel":
        logmel_part(a.reps)
    elif a.part == "samples":
        samples_part(a.reps)
    else:
        scipy_part(a.reps)
