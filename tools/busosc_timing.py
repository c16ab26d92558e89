"""tools/busosc_timing.py — what the bus oscillators cost (notes/r32.md): against the bus filters on as many rows, and against the only
other way such rows get onto the device, a copy from pinned host memory.

In one process, after a warm-up, alternating round by round, per shape (buses x 48 000 samples, one second of audio at 48 kHz):
  osc_<port>_<rows>  srack_buses_osc, every bus enabled with that port (sine, square, saw; antialiasing on), LFO pitches (VAL -8 .. -4:
                     1.7 to 27 Hz): without rows, with a CV row (noise in [-1, 1]: the increment is recomputed every sample, the worst
                     case), with CV and sync (square gates of 0 / 1, a period of 9 600 samples);
  filter             srack_buses_filter without a CV on the same number of rows (row_channels 1, every bus enabled): the same kernel
                     shape, one row's chain;
  upload             hipMemcpyAsync of f32 [buses][48 000] from pinned host memory to the device: a floor on the host's route — the host
                     has not even computed anything;
  oracle_s           (once, on the CPU, shapes up to --oracle-buses) the seconds the CPU oracle needs to compute those rows.
Each figure is one call between two HIP events on the null stream; `--rounds` (three by default) of them, the median and the spread
(min .. max) reported, and every oscillator run's ratio to the filter's and to the upload's median.  No bar is fixed here; the reading is
in notes/r32.md.

    python tools/busosc_timing.py [--rounds 3] [--shapes 64,4096,32768] [--runs REGEX] [--oracle-buses 64] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import srack_pkg  # noqa: E402
from bus_reverb_timing import Events, device_buffer  # noqa: E402
from busvca_timing import fill_gates  # noqa: E402
from master_timing import fill  # noqa: E402

T = 48000
PORTS = (("sine", 0), ("square", 1), ("saw", 2))


def handle(S, NB, params, port):
    p = S.Patch(48000, 1024, 2)
    S.build_p1(p)
    p.configure_voices(1)
    p.set_buses(NB)
    p.set_bus_osc(params, np.full(NB, port, dtype=np.intc))
    return p


def shape(S, ev, NB, rounds, only, oracle_buses):
    rng = np.random.default_rng(NB)
    params = np.stack([rng.uniform(-8.0, -4.0, NB), rng.uniform(0.1, 1.0, NB), rng.uniform(-0.5, 0.5, NB)], axis=1).astype(np.float32)
    rowbytes = NB * T * 4
    d_cv, d_sync, d_out = device_buffer(S, rowbytes), device_buffer(S, rowbytes), device_buffer(S, rowbytes)
    fill(S, d_cv, rowbytes, rng)
    fill_gates(S, d_sync, rowbytes)
    hip = ev.hip
    hip.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    hip.hipHostFree.argtypes = [C.c_void_p]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    pinned = C.c_void_p()
    assert hip.hipHostMalloc(C.byref(pinned), rowbytes, 0) == 0
    C.memset(pinned, 0, rowbytes)  # (touched: the pages exist before the first copy is timed)

    def upload():
        assert hip.hipMemcpyAsync(d_out, pinned, rowbytes, 1, None) == 0  # hipMemcpyHostToDevice

    f = handle(S, NB, params, 0)
    f.set_bus_filter(np.stack([rng.uniform(0.05, 0.8, NB), rng.uniform(0.0, 1.0, NB), rng.uniform(-0.5, 0.5, NB)], axis=1).astype(np.float32),
                     rng.integers(0, 3, NB).astype(np.intc))
    runs = {"upload": upload, "filter": lambda: f.bus_filter_raw(T, d_cv, 1, None, d_out)}
    handles = {}
    for name, port in PORTS:
        p = handles[name] = handle(S, NB, params, port)
        runs[f"osc_{name}_none"] = lambda p=p: p.bus_osc_raw(T, None, None, d_out)
        runs[f"osc_{name}_cv"] = lambda p=p: p.bus_osc_raw(T, d_cv, None, d_out)
        runs[f"osc_{name}_cv_sync"] = lambda p=p: p.bus_osc_raw(T, d_cv, d_sync, d_out)
    if only:
        runs = {k: v for k, v in runs.items() if k in ("upload", "filter") or re.search(only, k)}
    for fn in runs.values():  # the warm-up: tables, state and events exist
        fn()
    S._check(S.lib.srack_device_sync(None))
    ms = {k: [] for k in runs}
    for _ in range(rounds):  # alternating
        for k, fn in runs.items():
            ms[k].append(ev.time(fn))
    out = {"buses": NB, "samples": T, "row_bytes": rowbytes, "info": re.search(r"busosc=\d+\[[^\]]*\]", handles["sine"].info()).group(0)}
    for k in runs:
        out[k] = {"median_ms": round(statistics.median(ms[k]), 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4)}
    for k in runs:
        if k.startswith("osc_"):
            out[k]["over_filter"] = round(out[k]["median_ms"] / out["filter"]["median_ms"], 3)
            out[k]["over_upload"] = round(out[k]["median_ms"] / out["upload"]["median_ms"], 3)
    out["upload"]["gb_per_s"] = round(rowbytes / out["upload"]["median_ms"] / 1e6, 2)
    if NB <= oracle_buses:
        from tests import busosc_ref as R
        t0 = time.perf_counter()
        R.bus_osc(None, None, params, np.zeros(NB, dtype=np.intc), None, None, 48000, n=T)
        out["oracle_s"] = round(time.perf_counter() - t0, 3)
    for d in (d_cv, d_sync, d_out):
        S.lib.srack_device_free(d)
    assert hip.hipHostFree(pinned) == 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="64,4096,32768")
    ap.add_argument("--runs", default=None)
    ap.add_argument("--oracle-buses", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 3, "at least three rounds"
    S = srack_pkg.load()
    ev = Events()
    results = []
    for NB in (int(x) for x in args.shapes.split(",")):
        results.append(shape(S, ev, NB, args.rounds, args.runs, args.oracle_buses))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"tool": "tools/busosc_timing.py", "rounds": args.rounds, "shapes": results}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
