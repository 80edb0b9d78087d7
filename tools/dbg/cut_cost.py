"""What planning the cuts of a long recording costs through the library ("Measured"), beside what it replaces:

    python tools/dbg/cut_cost.py [--seconds 600] [--reps 10]

  call         HipWhisper.cut_plan on a device-resident recording: host wall time around nh_cut_plan, which returns when
               starts, lens and the count are on the host (the launches alone, under HIP events: tools/bin/cutbench)
  alternative  the recording copied from the device to host memory, then tests/cut_ref.py in numpy (the same arithmetic)

Prints one JSON line; medians of --reps runs after one warm-up.  A test-d128 context without weights: a plan needs none."""
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


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import cut_ref as CR
    from norma_amd import config, hip
    x, _ = CR.bursts(0, a.seconds)
    hm = hip.HipWhisper(config.preset("test-d128"), device=0, max_batch=1)
    dev = hip.DeviceBuffer(x)
    rt = hip.DeviceBuffer.runtime()
    back = np.empty_like(x)
    plans = {}

    def call():
        plans["device"] = hm.cut_plan(dev.ptr, len(x))

    def copy():
        assert rt.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(dev.ptr), x.nbytes, 2) == 0   # hipMemcpyDeviceToHost

    def host():
        plans["host"] = CR.plan(back)[:2]

    out = {"seconds": a.seconds, "samples": len(x), "params": list(CR.DEFAULTS), "reps": a.reps, "call_ms": med(call, a.reps),
           "copy_to_host_ms": med(copy, a.reps), "cut_ref_numpy_ms": med(host, max(1, a.reps // 3))}
    out["alternative_ms"] = out["copy_to_host_ms"] + out["cut_ref_numpy_ms"]
    out["chunks"] = len(plans["device"][0])
    out["same_plan"] = bool(np.array_equal(plans["device"][0], plans["host"][0]) and np.array_equal(plans["device"][1], plans["host"][1]))
    print(json.dumps(out), flush=True)
    dev.free()
    hm.close()
