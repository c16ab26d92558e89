"""tools/stats_bench.py — what per-voice output statistics (srack_render_stats) cost, in ms per second of audio, against the route a host
has without them (frames, then a second pass over them).  One process, one GPU; the modes alternate round by round and the first round of
each is a warm-up that is not kept.

    python tools/stats_bench.py [--workload cfg3 ...] [--rounds R] [--samples T] [--chunk C]

Modes:  1 frames + mix (srack_render, as today)      2 frames + mix + stats      3 mix + stats      4 stats only
        5 today's route: frames of a chunk of C samples, then a torch pass over them that computes the same six statistics (f64)
A workload whose kernel does not carry statistics reports modes 2 - 4 as unsupported.  Prints one JSON line per workload."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VOICES = {"cfg3": 262144, "cfg3_poly": 262144, "p3": 262144, "p4": 131072, "cfg2": 4096, "cfg4": 65536, "cfg4_b1024": 65536}  # (bench.py's sizes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="append", default=None, help="cfg3 cfg3_poly cfg4 cfg4_b1024 p4 ... (repeatable; default cfg3)")
    ap.add_argument("--voices", type=int, default=0)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--chunk", type=int, default=4096, help="mode 5: samples per frames chunk")
    ap.add_argument("--rounds", type=int, default=4)
    args = ap.parse_args()
    import torch
    import srack_pkg
    S = srack_pkg.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for w in args.workload or ["cfg3"]:
        V = args.voices or VOICES[w]
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
        stats = torch.zeros((P, 6, V), dtype=torch.float64, device=dev)
        chunk = torch.empty((P, C, V), dtype=torch.float32, device=dev)
        mix_c = torch.empty((2, C), dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        p.reserve(T, want_mix=True)

        def today():
            s = torch.zeros((P, 6, V), dtype=torch.float64, device=dev)
            for t in range(0, T, C):
                n = min(C, T - t)
                p.render_raw(n, chunk.data_ptr(), mix_c.data_ptr(), 0, st)
                x = chunk[:, :n].double()
                fin = torch.isfinite(x)
                xs = torch.where(fin, x, torch.zeros((), dtype=x.dtype, device=dev))
                s[:, 0] += xs.sum(1)
                s[:, 1] += (xs * xs).sum(1)
                s[:, 2] = torch.maximum(s[:, 2], xs.amax(1))
                s[:, 3] = torch.maximum(s[:, 3], (-xs).amax(1))
                s[:, 4] += (~fin).sum(1)
                s[:, 5] += (fin & (xs.abs() > 1)).sum(1)
                del x, fin, xs
            return s

        modes = {
            1: lambda: p.render_raw(T, frames.data_ptr(), mix.data_ptr(), 0, st),
            2: lambda: p.render_raw(T, frames.data_ptr(), mix.data_ptr(), 0, st, stats.data_ptr()),
            3: lambda: p.render_raw(T, None, mix.data_ptr(), 0, st, stats.data_ptr()),
            4: lambda: p.render_raw(T, None, None, 0, st, stats.data_ptr()),
            5: today,
        }
        times = {m: [] for m in modes}
        unsupported = {}
        for r in range(args.rounds + 1):
            for m, fn in modes.items():
                if m in unsupported:
                    continue
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                try:
                    fn()
                except S.SrackError as e:
                    unsupported[m] = str(e)
                    continue
                torch.cuda.synchronize(dev)
                if r > 0:
                    times[m].append((time.perf_counter() - t0) * 1e3 / (T / 48000.0))
        out = {"workload": w, "voices": V, "samples": T, "chunk_mode5": C, "kernel": p.info().split("kernel=")[-1].split()[0]}
        for m in modes:
            if m in unsupported:
                out[f"mode{m}"] = "unsupported"
            else:
                v = sorted(times[m])
                out[f"mode{m}_ms_per_s"] = round(v[len(v) // 2], 3)
                out[f"mode{m}_all"] = [round(x, 3) for x in times[m]]
        print(json.dumps(out), flush=True)
        del frames, mix, stats, chunk, mix_c, p
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
