"""tools/sends_timing.py — what the bus sends cost against a plain copy of their input (notes/r18.md).

The table: 4 096 buses, buses 0 .. 3 aux, every other bus b sends to aux b % 4, through gains 1 — S = 4 092 sends, 1 023 into each aux
bus.  In one process, after a warm-up, alternating round by round:
  A   a device-to-device copy of the rows into a second buffer (hipMemcpyAsync): it moves 2 N row-bytes;
  B   srack_buses_send on the same rows: it reads N + S rows and writes N, 1.5 x the copy's traffic.
Each figure is a window of HIP events on the null stream around enough repetitions to last 0.25 s or more, divided by the repetitions;
`--rounds` (at least six) windows each, the median and the spread (min .. max) reported.  The bar (the issue's), at 48 000 samples:
the send's median no longer than 1.5 x the copy's.  The same table x 1 024 samples is the ticked host: no bar, the time and the
launches per call.

    python tools/sends_timing.py [--rounds 6] [--out profiles/r18_sends.json]
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
from master_timing import fill  # noqa: E402

NB, AUX = 4096, 4
# (samples, does the bar apply)
SHAPES = [(48000, True), (1024, False)]
WINDOW_MS = 250.0
BAR = 1.5


def repetitions(ev, fn):
    """how many make a window of WINDOW_MS, from one timed call after a warm-up"""
    fn()
    one = max(ev.time(fn), 1e-3)
    return max(3, int(np.ceil(WINDOW_MS * 1.1 / one)))


def shape(S, ev, T, bar, rounds):
    p = S.Patch(48000, 1024, 2)
    S.build_p1(p)
    p.configure_voices(1)
    p.set_buses(NB)
    src = np.arange(AUX, NB, dtype=np.intc)
    p.set_sends(src, src % AUX)
    n_terms, _, n_runs = p.send_plan()
    multi = int((n_terms > 64).sum())
    rng = np.random.default_rng(NB + T)
    nbytes = NB * 2 * T * 4
    d_rows, d_copy, d_out = device_buffer(S, nbytes), device_buffer(S, nbytes), device_buffer(S, nbytes)
    fill(S, d_rows, nbytes, rng)
    ev.hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]

    def copy():
        assert ev.hip.hipMemcpyAsync(d_copy, d_rows, nbytes, 3, None) == 0  # hipMemcpyDeviceToDevice

    runs = {"copy": copy, "send": lambda: p.send_raw(T, d_rows, 2, d_out)}
    reps = {k: repetitions(ev, f) for k, f in runs.items()}
    ms = {k: [] for k in runs}
    for _ in range(rounds):  # A, B alternating
        for k, f in runs.items():
            def window(f=f, n=reps[k]):
                for _ in range(n):
                    f()
            ms[k].append(ev.time(window) / reps[k])
    info = p.info()
    for d in (d_rows, d_copy, d_out):
        S.lib.srack_device_free(d)
    row_bytes = 2 * T * 4
    out = {"buses": NB, "samples": T, "sends": len(src), "runs": n_runs, "launches_per_call": 1 + (1 if multi else 0), "input_bytes": nbytes,
           "copy_traffic_bytes": 2 * nbytes, "send_traffic_bytes": (2 * NB + len(src)) * row_bytes, "bar_applies": bar,
           "info": re.search(r"sends=\d+\[\d+ runs\]", info).group(0)}
    for k in runs:
        med = statistics.median(ms[k])
        out[k] = {"median_ms": round(med, 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4), "repetitions_per_window": reps[k]}
    out["copy"]["traffic_GB_per_s"] = round(out["copy_traffic_bytes"] / out["copy"]["median_ms"] / 1e6, 1)
    out["send"]["traffic_GB_per_s"] = round(out["send_traffic_bytes"] / out["send"]["median_ms"] / 1e6, 1)
    out["send_over_copy"] = round(out["send"]["median_ms"] / out["copy"]["median_ms"], 3)
    if bar:
        out["bar"] = BAR
        out["bar_met"] = out["send"]["median_ms"] <= BAR * out["copy"]["median_ms"]
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
    for T, bar in SHAPES:
        results.append(shape(S, ev, T, bar, args.rounds))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/sends_timing.py", "rounds": args.rounds, "window_ms": WINDOW_MS, "shapes": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
