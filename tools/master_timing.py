"""tools/master_timing.py — what the master section costs against a plain copy of its input (notes/r17.md).

In one process, after a warm-up, alternating round by round:
  A   a device-to-device copy of the rows into a second buffer (hipMemcpyAsync): it moves twice the bytes the master must read;
  B   srack_buses_master on the same rows with statistics NULL;
  B'  the same with statistics on.
Each figure is a window of HIP events on the null stream around enough repetitions to last 0.2 s or more, divided by the repetitions;
`--rounds` (at least six) windows each, the median and the spread (min .. max) reported.  The read rate is the bytes of the rows —
from the shapes — over the time.  The bar (the issue's): at the two large shapes the master's median is no longer than the copy's.

    python tools/master_timing.py [--rounds 6] [--out profiles/r17_master.json]
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

# (buses, samples, does the bar apply)
SHAPES = [(4096, 48000, True), (65536, 4096, True), (64, 48000, False), (4096, 1024, False)]
WINDOW_MS = 200.0


def fill(S, d, nbytes, rng):
    """seeded noise, a 64 MiB block of it repeated (what the values are does not change what is timed)"""
    block = (rng.random(min(nbytes, 64 << 20) // 4, dtype=np.float32) * np.float32(2) - np.float32(1))
    for at in range(0, nbytes, block.nbytes):
        n = min(block.nbytes, nbytes - at)
        S._check(S.lib.srack_device_from_host(d.value + at, block.ctypes.data_as(C.c_void_p), n, None))
    S._check(S.lib.srack_device_sync(None))


def repetitions(ev, fn):
    """how many make a window of WINDOW_MS, from one timed call after a warm-up"""
    fn()
    one = max(ev.time(fn), 1e-3)
    return max(3, int(np.ceil(WINDOW_MS * 1.25 / one)))


def shape(S, ev, NB, T, bar, rounds):
    p = S.Patch(48000, 1024, 2)
    S.build_p1(p)
    p.configure_voices(1)
    p.set_buses(NB)
    rng = np.random.default_rng(NB + T)
    p.set_master(rng.uniform(-2, 2, (NB, 2)).astype(np.float32))
    nbytes = NB * 2 * T * 4
    d_rows, d_copy = device_buffer(S, nbytes), device_buffer(S, nbytes)
    d_master, d_stats = device_buffer(S, 2 * T * 4), device_buffer(S, 2 * 6 * 8, np.zeros((2, 6)))
    fill(S, d_rows, nbytes, rng)
    ev.hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]

    def copy():
        assert ev.hip.hipMemcpyAsync(d_copy, d_rows, nbytes, 3, None) == 0  # hipMemcpyDeviceToDevice

    runs = {"copy": copy, "master": lambda: p.master_raw(T, d_rows, 2, d_master), "master_stats": lambda: p.master_raw(T, d_rows, 2, d_master, d_stats)}
    reps = {k: repetitions(ev, f) for k, f in runs.items()}
    ms = {k: [] for k in runs}
    for _ in range(rounds):  # A, B, B' alternating
        for k, f in runs.items():
            def window(f=f, n=reps[k]):
                for _ in range(n):
                    f()
            ms[k].append(ev.time(window) / reps[k])
    info = p.info()
    for d in (d_rows, d_copy, d_master, d_stats):
        S.lib.srack_device_free(d)
    out = {"buses": NB, "samples": T, "input_bytes": nbytes, "bar_applies": bar, "info": re.search(r"master=\d+\[\d+ runs\]", info).group(0)}
    for k in runs:
        med = statistics.median(ms[k])
        out[k] = {"median_ms": round(med, 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4), "repetitions_per_window": reps[k],
                  "rows_read_GB_per_s": round(nbytes / med / 1e6, 1)}
    if bar:
        out["bar_met"] = out["master"]["median_ms"] <= out["copy"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 6, "at least six rounds"
    S = srack_pkg.load()
    ev = Events()
    results = []
    for NB, T, bar in SHAPES:
        results.append(shape(S, ev, NB, T, bar, args.rounds))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/master_timing.py", "rounds": args.rounds, "window_ms": WINDOW_MS, "shapes": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
