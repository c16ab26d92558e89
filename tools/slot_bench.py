"""tools/slot_bench.py — what voice bus slots (srack_voices_set_bus_slots) cost against the mix table that was there before, in ms per
second of audio.  A sibling of tools/bus_bench.py: one process, one GPU, the modes alternate round by round, the first round of each
is a warm-up that is not kept, and every round of every mode is printed so that the spread can be read next to the medians.

    python tools/slot_bench.py [--workload cfg3] [--voices V] [--buses 4096] [--samples 48000] [--rounds R] [--reps N]

Modes (frames and mix are written in all of them, as in bus_bench's mode 2, so that the differences are the folds'):
    r  srack_render alone: what every other mode pays as well
    a  srack_voices_set_buses, contiguous buses, one gain per voice: the two kernels that were there before (bus_fold_tiles / _sum)
    b  srack_voices_set_bus_slots, K = 1, the same buses, distinct Left / Right gains (equal-power pan): bus_slot_fold_tiles / _sum
    c  K = 2: slot 0 as in b, slot 1 one of four aux buses (v mod 4) with a send amount per voice
Prints one JSON line: per mode the median and all rounds, and per fold the median of the round-by-round differences from r."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--voices", type=int, default=262144)
    ap.add_argument("--buses", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed window")
    args = ap.parse_args()
    import torch
    import srack_pkg
    S = srack_pkg.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    V, NB, T, AUX = args.voices, args.buses, args.samples, 4
    B, build, overrides = S.bench_workload(args.workload, V)
    rng = np.random.default_rng(1)
    group = (np.arange(V) // (V // NB)).astype(np.intc)
    theta = rng.uniform(0, np.pi / 2, V)
    pan = np.stack([np.cos(theta), np.sin(theta)], axis=1).astype(np.float32)
    send = rng.uniform(0, 1, (V, 1, 2)).astype(np.float32)
    tables = {
        "r": None,
        "a": lambda p: p.set_buses(NB, group, pan[:, 0]),
        "b": lambda p: p.set_bus_slots(NB, group[:, None], pan[:, None, :]),
        "c": lambda p: p.set_bus_slots(NB + AUX, np.stack([group, NB + np.arange(V) % AUX], axis=1), np.concatenate([pan[:, None, :], send], axis=1)),
    }
    patches = {}
    for m, table in tables.items():  # a handle per mode: nothing is uploaded or re-planned inside the timed calls
        p = S.Patch(48000, B, 2)
        ids = build(p)
        p.configure_voices(V)
        for mod, f, v in overrides(ids):
            p.set_voice_field(mod, f, v)
        if table:
            table(p)
        patches[m] = p
    P, _ = patches["r"].planes()
    frames = torch.empty((P, T, V), dtype=torch.float32, device=dev)
    mix = torch.empty((2, T), dtype=torch.float32, device=dev)
    bus_mix = torch.empty((NB + AUX, 2, T), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def run(m):
        p = patches[m]
        if m == "r":
            p.render_raw(T, frames.data_ptr(), mix.data_ptr(), 0, st)
        else:
            p.render_buses_raw(T, bus_mix.data_ptr(), frames.data_ptr(), mix.data_ptr(), None, 0, st)

    times = {m: [] for m in tables}
    for r in range(args.rounds + 1):
        for m in tables:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.reps):
                run(m)
            torch.cuda.synchronize(dev)
            if r > 0:
                times[m].append((time.perf_counter() - t0) * 1e3 / (args.reps * T / 48000.0))
    out = {"workload": args.workload, "voices": V, "buses": NB, "aux": AUX, "samples": T, "planes": P, "rounds": args.rounds, "reps": args.reps}
    for m in tables:
        out[f"{m}_ms_per_s"] = round(float(np.median(times[m])), 3)
        out[f"{m}_all"] = [round(x, 3) for x in times[m]]
        if m != "r":
            d = np.array(times[m]) - np.array(times["r"])
            out[f"{m}_fold_ms_per_s"] = round(float(np.median(d)), 3)
            out[f"{m}_fold_min_max"] = [round(float(d.min()), 3), round(float(d.max()), 3)]
            seg, _ = patches[m].bus_plan()
            out[f"{m}_segments"], out[f"{m}_partials"] = int(len(seg)), int((seg[:, 2] >= 0).sum())
            out[f"{m}_info"] = patches[m].info().split(" buses=")[1].split()[0]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
