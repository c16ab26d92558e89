"""tools/busmeter_timing.py — what the bus meters cost against a plain copy of their rows and against the master section (notes/r25.md).

In one process, after a warm-up, alternating round by round, per shape (buses x 2 channels x 48 000 samples):
  copy       a device-to-device copy of the rows into a second buffer (hipMemcpyAsync): twice the bytes a meter call reads;
  master     srack_buses_master on the same rows, with its statistics: the other call that reads every row once;
  levels     srack_buses_meter, d_levels only, window 480 (100 records per call);
  totals     d_totals only;
  both       d_levels (window 480) and d_totals;
  window_64  both, window 64, the shortest: a record stored and the next one loaded every tile (750 records per call).
Each figure is a window of HIP events on the null stream around enough repetitions to last 0.25 s or more, divided by the repetitions;
`--rounds` (at least six) windows each, the median and the spread (min .. max) reported, the ratio of every median to the copy's and to
the master's, the bytes the call reads over its median and the picoseconds per metered sample.  The rows are noise in [-1, 1].  Every
meter call is handed stream position 0 again, so the records keep adding up: the sums grow, the work per sample does not.
No bar is fixed in advance; the reading is in notes/r25.md.

    python tools/busmeter_timing.py [--rounds 6] [--shapes 64,4096,32768] [--runs REGEX] [--out profiles/r25_busmeter.json]

`--runs`: only the variants whose name matches, beside the copy (for comparing builds of the kernel).
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import srack_pkg  # noqa: E402
from bus_reverb_timing import Events, device_buffer  # noqa: E402
from busvca_timing import repetitions  # noqa: E402
from master_timing import fill  # noqa: E402

T = 48000
WINDOW_MS = 250.0
WINDOW, SHORT = 480, 64


def zeroed(S, hip, nbytes):
    d = device_buffer(S, nbytes)
    assert hip.hipMemset(d, 0, nbytes) == 0
    return d


def shape(S, ev, NB, rounds, only=None):
    rng = np.random.default_rng(NB)
    p = S.Patch(48000, 1024, 2)
    S.build_p1(p)
    p.configure_voices(1)
    p.set_buses(NB)
    nbytes, frame = NB * 2 * T * 4, S.STAT_COUNT * NB * 2 * 8
    n_win, n_short = -(-T // WINDOW), -(-T // SHORT)
    ev.hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    ev.hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    d_rows, d_out = device_buffer(S, nbytes), device_buffer(S, nbytes)
    d_lv, d_short, d_tt = zeroed(S, ev.hip, n_win * frame), zeroed(S, ev.hip, n_short * frame), zeroed(S, ev.hip, frame)
    d_master, d_stats = device_buffer(S, 2 * T * 4), zeroed(S, ev.hip, 2 * S.STAT_COUNT * 8)
    fill(S, d_rows, nbytes, rng)

    def copy():
        assert ev.hip.hipMemcpyAsync(d_out, d_rows, nbytes, 3, None) == 0  # hipMemcpyDeviceToDevice

    # (bytes the call reads and writes, for the TB/s: the records are read and written once each)
    runs = {"copy": (copy, 2 * nbytes),
            "master": (lambda: p.master_raw(T, d_rows, 2, d_master, d_stats), nbytes),
            "levels": (lambda: p.bus_meter_raw(0, T, d_rows, 2, WINDOW, d_lv, n_win, None), nbytes + 2 * n_win * frame),
            "totals": (lambda: p.bus_meter_raw(0, T, d_rows, 2, 0, None, 0, d_tt), nbytes + 2 * frame),
            "both": (lambda: p.bus_meter_raw(0, T, d_rows, 2, WINDOW, d_lv, n_win, d_tt), nbytes + 2 * (n_win + 1) * frame),
            "window_64": (lambda: p.bus_meter_raw(0, T, d_rows, 2, SHORT, d_short, n_short, d_tt), nbytes + 2 * (n_short + 1) * frame)}
    if only:
        runs = {k: v for k, v in runs.items() if k == "copy" or re.search(only, k)}
    reps = {k: repetitions(ev, fn) for k, (fn, _) in runs.items()}
    ms = {k: [] for k in runs}
    for _ in range(rounds):  # alternating
        for k, (fn, _) in runs.items():
            def window(fn=fn, n=reps[k]):
                for _ in range(n):
                    fn()
            ms[k].append(ev.time(window) / reps[k])
    note = re.search(r"meter=\d+\[w[-\d]+\]", p.info())
    for d in (d_rows, d_out, d_lv, d_short, d_tt, d_master, d_stats):
        S.lib.srack_device_free(d)
    out = {"buses": NB, "samples": T, "row_bytes": nbytes, "frame_bytes": frame, "records": {"levels": n_win, "window_64": n_short}, "info": note.group(0) if note else ""}
    for k, (_, moved) in runs.items():
        med = statistics.median(ms[k])
        out[k] = {"median_ms": round(med, 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4), "repetitions_per_window": reps[k],
                  "bytes_moved": moved, "tb_per_s": round(moved / med / 1e9, 3)}
        if k != "copy":
            out[k]["over_copy"] = round(med / out["copy"]["median_ms"], 2)
            if "master" in out and k != "master":
                out[k]["over_master"] = round(med / out["master"]["median_ms"], 2)
            out[k]["ps_per_sample"] = round(med * 1e9 / (NB * 2 * T), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--shapes", default="64,4096,32768")
    ap.add_argument("--runs", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 6, "at least six rounds"
    S = srack_pkg.load()
    ev = Events()
    results = []
    for NB in (int(x) for x in args.shapes.split(",")):
        results.append(shape(S, ev, NB, args.rounds, args.runs))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/busmeter_timing.py", "rounds": args.rounds, "window_ms": WINDOW_MS, "shapes": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
