"""tools/busvca_timing.py — what the bus VCAs cost against a plain copy of their rows, beside the bus filters and the sends (notes/r20.md).

In one process, after a warm-up, alternating round by round, per shape (buses x 2 channels x 48 000 samples):
  copy      a device-to-device copy of the rows into a second buffer (hipMemcpyAsync): the bytes an out-of-place call moves, less the control rows;
  vca_*     srack_buses_vca: every bus CV; every bus GATE; half and half (alternating buses: every workgroup has gated buses); every bus GATE
            with d_env; every bus GATE in place;
  filter    srack_buses_filter without a CV, every bus enabled (tools/busvcf_timing.py's first variant);
  send      srack_buses_send, four aux buses fed by all others (tools/sends_timing.py's list).
Each figure is a window of HIP events on the null stream around enough repetitions to last 0.25 s or more, divided by the repetitions;
`--rounds` (at least six) windows each, the median and the spread (min .. max) reported, the ratio of every median to the copy's and the
bytes the call moves over its median.  The gates are square waves of 0 / 1 with a period of 9 600 samples, the CVs noise in [-1, 1], the
sliders random in [0.001, 0.3] s.  No bar is fixed in advance; the reading is in notes/r20.md.

    python tools/busvca_timing.py [--rounds 6] [--shapes 64,4096,32768] [--runs REGEX] [--out profiles/r20_busvca.json]

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
from master_timing import fill  # noqa: E402

T = 48000
WINDOW_MS = 250.0
GATE_PERIOD = 9600
AUX = 4


def repetitions(ev, fn):
    """how many make a window of WINDOW_MS, from one timed call after a warm-up"""
    fn()
    one = max(ev.time(fn), 1e-3)
    return max(3, int(np.ceil(WINDOW_MS * 1.1 / one)))


def fill_gates(S, d, nbytes):
    """square waves of 0 / 1, a 64 MiB block of them repeated"""
    n = min(nbytes, 64 << 20) // 4
    block = ((np.arange(n) % GATE_PERIOD) < GATE_PERIOD // 2).astype(np.float32)
    for at in range(0, nbytes, block.nbytes):
        k = min(block.nbytes, nbytes - at)
        S._check(S.lib.srack_device_from_host(d.value + at, block.ctypes.data_as(C.c_void_p), k, None))
    S._check(S.lib.srack_device_sync(None))


def shape(S, ev, NB, rounds, only=None):
    rng = np.random.default_rng(NB)
    sliders = np.stack([rng.uniform(0.001, 0.3, NB), rng.uniform(0.001, 0.3, NB), rng.uniform(0.0, 1.0, NB), rng.uniform(0.001, 0.3, NB)], axis=1).astype(np.float32)
    handles = {}
    for name, mode in (("cv", np.full(NB, S.BUS_VCA_CV)), ("gate", np.full(NB, S.BUS_VCA_GATE)), ("half", np.where(np.arange(NB) % 2, S.BUS_VCA_CV, S.BUS_VCA_GATE))):
        p = S.Patch(48000, 1024, 2)
        S.build_p1(p)
        p.configure_voices(1)
        p.set_buses(NB)
        p.set_bus_vca(sliders, mode.astype(np.intc))
        handles[name] = p
    f = handles["cv"]   # the filters and the sends, for comparison, hang off one of the handles
    f.set_bus_filter(np.stack([rng.uniform(0.05, 0.8, NB), rng.uniform(0.0, 1.0, NB), rng.uniform(-0.5, 0.5, NB)], axis=1).astype(np.float32),
                     rng.integers(0, 3, NB).astype(np.intc))
    src = np.arange(AUX, NB, dtype=np.intc)
    f.set_sends(src, src % AUX)
    nbytes, rowbytes = NB * 2 * T * 4, NB * T * 4
    d_rows, d_out = device_buffer(S, nbytes), device_buffer(S, nbytes)
    d_gate, d_cv, d_env = device_buffer(S, rowbytes), device_buffer(S, rowbytes), device_buffer(S, rowbytes)
    fill(S, d_rows, nbytes, rng)
    fill(S, d_cv, rowbytes, rng)
    fill_gates(S, d_gate, rowbytes)
    ev.hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]

    def copy():
        assert ev.hip.hipMemcpyAsync(d_out, d_rows, nbytes, 3, None) == 0  # hipMemcpyDeviceToDevice

    runs = {"copy": (copy, 2 * nbytes),
            "vca_cv": (lambda: handles["cv"].bus_vca_raw(T, d_rows, 2, d_cv, d_out), 2 * nbytes + rowbytes),
            "vca_gate": (lambda: handles["gate"].bus_vca_raw(T, d_rows, 2, d_gate, d_out), 2 * nbytes + rowbytes),
            "vca_half": (lambda: handles["half"].bus_vca_raw(T, d_rows, 2, d_gate, d_out), 2 * nbytes + rowbytes),
            "vca_gate_env": (lambda: handles["gate"].bus_vca_raw(T, d_rows, 2, d_gate, d_out, d_env), 2 * nbytes + 2 * rowbytes),
            "vca_gate_in_place": (lambda: handles["gate"].bus_vca_raw(T, d_out, 2, d_gate, d_out), 2 * nbytes + rowbytes),
            "filter": (lambda: f.bus_filter_raw(T, d_rows, 2, None, d_out), 2 * nbytes),
            "send": (lambda: f.send_raw(T, d_rows, 2, d_out), 2 * nbytes)}
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
    info = handles["gate"].info()
    for d in (d_rows, d_out, d_gate, d_cv, d_env):
        S.lib.srack_device_free(d)
    out = {"buses": NB, "samples": T, "row_bytes": nbytes, "ctl_bytes": rowbytes, "info": re.search(r"busvca=\d+\[\d+ gated\]", info).group(0)}
    for k, (_, moved) in runs.items():
        med = statistics.median(ms[k])
        out[k] = {"median_ms": round(med, 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4), "repetitions_per_window": reps[k],
                  "bytes_moved": moved, "tb_per_s": round(moved / med / 1e9, 3)}
        if k != "copy":
            out[k]["over_copy"] = round(med / out["copy"]["median_ms"], 2)
    if "vca_gate" in out:
        out["vca_gate"]["ns_per_sample"] = round(out["vca_gate"]["median_ms"] * 1e6 / T, 2)
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
            json.dump({"tool": "tools/busvca_timing.py", "rounds": args.rounds, "window_ms": WINDOW_MS, "shapes": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
