"""tools/bus_bench.py — what mix buses (srack_voices_set_buses / srack_render_buses) cost, in ms per second of audio, against the route a
host has without them (frames, then the same weighted, grouped sum over them in torch).  One process, one GPU; the modes alternate round
by round and the first round of each is a warm-up that is not kept.

    python tools/bus_bench.py [--workload cfg3 ...] [--buses 4096] [--rounds R] [--samples T] [--chunk C]

Tables: `contiguous` (bus = v // (V / buses)) and `mod` (bus = v mod buses), every gain drawn from [-1, 1).
Modes:  1 frames + mix (srack_render, as today)      2 frames + mix + buses      3 buses only (frames in library scratch)
        4 today's route: frames of a chunk of C samples, then torch — a reshape-and-sum for the contiguous table, index_add_ for `mod`
Prints one JSON line per workload and table."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VOICES = {"cfg3": 262144, "cfg3_poly": 262144, "p3": 262144, "p4": 131072, "cfg2": 4096, "cfg4": 65536, "cfg4_b1024": 65536}  # (bench.py's sizes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="append", default=None, help="cfg3 cfg3_poly cfg4 p4 ... (repeatable; default cfg3)")
    ap.add_argument("--table", action="append", default=None, help="contiguous | mod (repeatable; default both)")
    ap.add_argument("--voices", type=int, default=0)
    ap.add_argument("--buses", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--chunk", type=int, default=4096, help="mode 4: samples per frames chunk")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", default="1234")
    args = ap.parse_args()
    import torch
    import srack_pkg
    S = srack_pkg.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for w in args.workload or ["cfg3"]:
        V = args.voices or VOICES[w]
        NB = args.buses
        B, build, overrides = S.bench_workload(w, V)
        p = S.Patch(48000, B, 2)
        ids = build(p)
        p.configure_voices(V)
        for m, f, v in overrides(ids):
            p.set_voice_field(m, f, v)
        T, C = args.samples, min(args.chunk, args.samples)
        P, _ = p.planes()
        frames = torch.empty((P, T, V), dtype=torch.float32, device=dev)
        mix = torch.empty((2, T), dtype=torch.float32, device=dev)
        bus_mix = torch.empty((NB, 2, T), dtype=torch.float32, device=dev)
        chunk = torch.empty((P, C, V), dtype=torch.float32, device=dev)
        mix_c = torch.empty((2, C), dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        p.reserve(T, want_mix=True)
        gain = np.random.default_rng(1).uniform(-1, 1, V).astype(np.float32)
        g_dev = torch.from_numpy(gain).to(dev)
        for table in args.table or ["contiguous", "mod"]:
            per = V // NB
            bus = (np.arange(V) // per if table == "contiguous" else np.arange(V) % NB).astype(np.intc)
            p.set_buses(NB, bus, gain)
            b_dev = torch.from_numpy(bus.astype(np.int64)).to(dev)

            def today():
                out = torch.empty((P, T, NB), dtype=torch.float32, device=dev)
                for t in range(0, T, C):
                    n = min(C, T - t)
                    p.render_raw(n, chunk.data_ptr(), mix_c.data_ptr(), 0, st)
                    x = chunk[:, :n] * g_dev
                    if table == "contiguous":
                        out[:, t:t + n] = x.view(P, n, NB, per).sum(-1)
                    else:
                        out[:, t:t + n] = torch.zeros((P, n, NB), dtype=torch.float32, device=dev).index_add_(2, b_dev, x)
                    del x
                return out

            modes = {
                1: lambda: p.render_raw(T, frames.data_ptr(), mix.data_ptr(), 0, st),
                2: lambda: p.render_buses_raw(T, bus_mix.data_ptr(), frames.data_ptr(), mix.data_ptr(), None, 0, st),
                3: lambda: p.render_buses_raw(T, bus_mix.data_ptr(), None, None, None, 0, st),
                4: today,
            }
            modes = {m: fn for m, fn in modes.items() if str(m) in args.modes}
            times = {m: [] for m in modes}
            for r in range(args.rounds + 1):
                for m, fn in modes.items():
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize(dev)
                    if r > 0:
                        times[m].append((time.perf_counter() - t0) * 1e3 / (T / 48000.0))
            seg, _ = p.bus_plan()
            out = {"workload": w, "table": table, "voices": V, "buses": NB, "samples": T, "chunk_mode4": C, "planes": P,
                   "segments": int(len(seg)), "partials": int((seg[:, 2] >= 0).sum()), "kernel": p.info().split("kernel=")[-1].split()[0]}
            for m in modes:
                v = sorted(times[m])
                out[f"mode{m}_ms_per_s"] = round(v[len(v) // 2], 3) if v else None  # (--rounds 0: the warm-up only, for a profiler)
                out[f"mode{m}_all"] = [round(x, 3) for x in times[m]]
            print(json.dumps(out), flush=True)
        del frames, mix, bus_mix, chunk, mix_c, p
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
