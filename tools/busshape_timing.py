"""tools/busshape_timing.py — what the bus shapers cost against a plain copy of their rows (notes/r24.md).

In one process, after a warm-up, alternating round by round, per shape (buses x 2 channels x 48 000 samples):
  copy            a device-to-device copy of the rows into a second buffer (hipMemcpyAsync): the bytes an out-of-place call moves, less the CV rows;
  const           srack_buses_shaper, every bus CONST, out of place;
  cv              every bus CV with a CV row, out of place;
  const_in_place  every bus CONST, in place;
  half_off        alternating buses OFF and CONST, out of place: the OFF half is a word copy.
Each figure is a window of HIP events on the null stream around enough repetitions to last 0.25 s or more, divided by the repetitions;
`--rounds` (at least six) windows each, the median and the spread (min .. max) reported, the ratio of every median to the copy's, the
bytes the call moves over its median and the picoseconds per processed sample.  The rows are noise in [-1, 1], the drives random in
[0.25, 4], the exponents in [0.5, 2], the CV rows in [0.5, 2].  The in-place run shapes its own output again and again, so its constants are 1, 1, 1: the power takes the same instructions for any exponent, and
powf(x, 1) is x, which keeps the rows where they are instead of walking them to 0 or 1 and into the cold path within a window.
No bar is fixed in advance; the reading is in notes/r24.md.

    python tools/busshape_timing.py [--rounds 6] [--shapes 64,4096,32768] [--runs REGEX] [--out profiles/r24_busshape.json]

`--runs`: only the variants whose name matches, beside the copy (for comparing builds of the kernel).
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
from busvca_timing import repetitions  # noqa: E402
from master_timing import fill  # noqa: E402

T = 48000
WINDOW_MS = 250.0


def fill_cv(S, d, nbytes, rng):
    """exponents in [0.5, 2], a 64 MiB block of them repeated"""
    block = (rng.random(min(nbytes, 64 << 20) // 4, dtype=np.float32) * np.float32(1.5) + np.float32(0.5))
    for at in range(0, nbytes, block.nbytes):
        n = min(block.nbytes, nbytes - at)
        S._check(S.lib.srack_device_from_host(d.value + at, block.ctypes.data_as(C.c_void_p), n, None))
    S._check(S.lib.srack_device_sync(None))


def shape(S, ev, NB, rounds, only=None):
    rng = np.random.default_rng(NB)
    params = np.stack([rng.uniform(0.25, 4.0, NB), rng.uniform(0.5, 2.0, NB), rng.uniform(0.25, 2.0, NB)], axis=1).astype(np.float32)
    unit = np.ones_like(params)
    handles = {}
    for name, par, mode in (("const", params, np.full(NB, S.BUS_SHAPER_CONST)), ("cv", params, np.full(NB, S.BUS_SHAPER_CV)),
                            ("in_place", unit, np.full(NB, S.BUS_SHAPER_CONST)),
                            ("half_off", params, np.where(np.arange(NB) % 2, S.BUS_SHAPER_CONST, S.BUS_SHAPER_OFF))):
        p = S.Patch(48000, 1024, 2)
        S.build_p1(p)
        p.configure_voices(1)
        p.set_buses(NB)
        p.set_bus_shaper(par, mode.astype(np.intc))
        handles[name] = p
    nbytes, rowbytes = NB * 2 * T * 4, NB * T * 4
    d_rows, d_out, d_cv = device_buffer(S, nbytes), device_buffer(S, nbytes), device_buffer(S, rowbytes)
    fill(S, d_rows, nbytes, rng)
    fill_cv(S, d_cv, rowbytes, rng)
    ev.hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]

    def copy():
        assert ev.hip.hipMemcpyAsync(d_out, d_rows, nbytes, 3, None) == 0  # hipMemcpyDeviceToDevice

    # (processed samples per call, for the ps per sample: half_off processes half of them)
    runs = {"copy": (copy, 2 * nbytes, 0),
            "const": (lambda: handles["const"].bus_shaper_raw(T, d_rows, 2, None, d_out), 2 * nbytes, NB * 2 * T),
            "cv": (lambda: handles["cv"].bus_shaper_raw(T, d_rows, 2, d_cv, d_out), 2 * nbytes + rowbytes, NB * 2 * T),
            "const_in_place": (lambda: handles["in_place"].bus_shaper_raw(T, d_out, 2, None, d_out), 2 * nbytes, NB * 2 * T),
            "half_off": (lambda: handles["half_off"].bus_shaper_raw(T, d_rows, 2, None, d_out), 2 * nbytes, (NB // 2) * 2 * T)}
    if only:
        runs = {k: v for k, v in runs.items() if k == "copy" or re.search(only, k)}
    copy()  # (const_in_place starts from the rows)
    reps = {k: repetitions(ev, fn) for k, (fn, _, _) in runs.items()}
    ms = {k: [] for k in runs}
    for _ in range(rounds):  # alternating
        for k, (fn, _, _) in runs.items():
            if k == "const_in_place":
                copy()
            def window(fn=fn, n=reps[k]):
                for _ in range(n):
                    fn()
            ms[k].append(ev.time(window) / reps[k])
    info = handles["cv"].info() if "cv" in runs else next(iter(handles.values())).info()
    for d in (d_rows, d_out, d_cv):
        S.lib.srack_device_free(d)
    note = re.search(r"busshp=\d+\[\d+ cv\]", info)
    out = {"buses": NB, "samples": T, "row_bytes": nbytes, "cv_bytes": rowbytes, "info": note.group(0) if note else ""}
    for k, (_, moved, processed) in runs.items():
        med = statistics.median(ms[k])
        out[k] = {"median_ms": round(med, 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4), "repetitions_per_window": reps[k],
                  "bytes_moved": moved, "tb_per_s": round(moved / med / 1e9, 3)}
        if k != "copy":
            out[k]["over_copy"] = round(med / out["copy"]["median_ms"], 2)
            out[k]["ps_per_processed_sample"] = round(med * 1e9 / processed, 2)
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
            json.dump({"tool": "tools/busshape_timing.py", "rounds": args.rounds, "window_ms": WINDOW_MS, "shapes": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
