"""tools/busvcf_timing.py — what the bus filters cost against a plain copy of their rows (notes/r19.md).

In one process, after a warm-up, alternating round by round, per shape (buses x 2 channels x 48 000 samples):
  A   a device-to-device copy of the rows into a second buffer (hipMemcpyAsync): the bytes an out-of-place filter call moves, less the CV;
  B   srack_buses_filter out of place and in place, each with a CV row per bus and without.
Each figure is a window of HIP events on the null stream around enough repetitions to last 0.2 s or more, divided by the repetitions;
`--rounds` (at least six) windows each, the median and the spread (min .. max) reported, and the ratio of every filter median to the
copy's.  No bar is fixed in advance; the reading (notes/r19.md): a lane is a row and a row is serial in time, so up to a wave on every
SIMD (1 024 waves: 32 768 stereo buses) the time should be flat in the buses and set by one row's chain — time that grows with the
buses at small counts means the rows are not spread over the CUs; a time at 32 768 buses far above copy + chain means the tile traffic
is not coalesced or not overlapped.

    python tools/busvcf_timing.py [--rounds 6] [--shapes 64,4096,32768] [--out profiles/r19_busvcf.json]
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import srack_pkg  # noqa: E402
from bus_reverb_timing import Events, device_buffer  # noqa: E402
from master_timing import fill, repetitions  # noqa: E402

T = 48000


def shape(S, ev, NB, rounds):
    p = S.Patch(48000, 1024, 2)
    S.build_p1(p)
    p.configure_voices(1)
    p.set_buses(NB)
    rng = np.random.default_rng(NB)
    params = np.stack([rng.uniform(0.05, 0.8, NB), rng.uniform(0.0, 1.0, NB), rng.uniform(-0.5, 0.5, NB)], axis=1).astype(np.float32)
    p.set_bus_filter(params, rng.integers(0, 3, NB).astype(np.intc))
    nbytes, cvbytes = NB * 2 * T * 4, NB * T * 4
    d_rows, d_out, d_cv = device_buffer(S, nbytes), device_buffer(S, nbytes), device_buffer(S, cvbytes)
    fill(S, d_rows, nbytes, rng)
    fill(S, d_cv, cvbytes, rng)
    ev.hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]

    def copy():
        assert ev.hip.hipMemcpyAsync(d_out, d_rows, nbytes, 3, None) == 0  # hipMemcpyDeviceToDevice

    runs = {"copy": copy,
            "filter": lambda: p.bus_filter_raw(T, d_rows, 2, None, d_out),
            "filter_cv": lambda: p.bus_filter_raw(T, d_rows, 2, d_cv, d_out),
            "filter_in_place": lambda: p.bus_filter_raw(T, d_rows, 2, None, d_rows),
            "filter_in_place_cv": lambda: p.bus_filter_raw(T, d_rows, 2, d_cv, d_rows)}
    reps = {k: repetitions(ev, f) for k, f in runs.items()}
    ms = {k: [] for k in runs}
    for _ in range(rounds):  # alternating
        for k, f in runs.items():
            def window(f=f, n=reps[k]):
                for _ in range(n):
                    f()
            ms[k].append(ev.time(window) / reps[k])
    info = p.info()
    for d in (d_rows, d_out, d_cv):
        S.lib.srack_device_free(d)
    out = {"buses": NB, "samples": T, "row_bytes": nbytes, "cv_bytes": cvbytes, "info": re.search(r"busvcf=\d+\[\d+ waves\]", info).group(0)}
    for k in runs:
        med = statistics.median(ms[k])
        out[k] = {"median_ms": round(med, 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4), "repetitions_per_window": reps[k]}
        if k != "copy":
            out[k]["over_copy"] = round(med / out["copy"]["median_ms"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--shapes", default="64,4096,32768")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 6, "at least six rounds"
    S = srack_pkg.load()
    ev = Events()
    results = []
    for NB in (int(x) for x in args.shapes.split(",")):
        results.append(shape(S, ev, NB, args.rounds))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/busvcf_timing.py", "rounds": args.rounds, "window_ms": 200.0, "shapes": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
