"""tools/bank_bench.py — what a wave per voice costs the sample player, on ONE box (boxes differ by a few percent: legs are only comparable
within a run).  Not bench.py: P4's patch at 131 072 voices x 48 000 samples with a 48 000-frame wave (never staged in LDS), frames and mix
as bench.py asks for them, in four legs that alternate for three rounds, each leg a fresh process:

    a  another build of the library (--parent path/to/libsrack_hip.so: the parent commit's), one wave shared by every voice   the yardstick
    b  this tree's library, the same call                                                                                      must tie with a
    c  this tree, a bank of 1024 distinct 48 000-frame waves, voice v plays wave v % 1024, plain gather (SRACK_JIT_SMP_WINDOW=0)
    d  c with the windowed read of the bank (the default)

    python tools/bank_bench.py --parent tools/ab_libs/libsrack_hip_parent.so [--rounds 3] [--steps 3] [--voices 131072] [--samples 48000]

Prints one JSON line per leg and round ({"leg", "round", "ms_per_step": [...], "kernel"}), then a summary with c / a — the price of
per-voice waves — and whether d beats c in every round by more than four times the larger round-to-round spread (notes/r10.md's bar).
The library is driven through ctypes directly (the binding in s-rack_amd/ loads one fixed path); the patch comes from workloads.py.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_BANK = 1024


class Raw:
    """the few calls build_p4 makes, on a library loaded from any path"""

    def __init__(self, path, sample_rate=48000, buffer_size=1024, channels=2):
        self.L = L = C.CDLL(path)
        vp, i32, u32, fp, ip = C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_int)
        L.srack_last_error.restype = C.c_char_p
        L.srack_patch_create.argtypes = [u32, u32, u32, C.POINTER(vp)]
        L.srack_patch_destroy.argtypes = [vp]
        L.srack_patch_add_module.argtypes = [vp, i32]
        L.srack_patch_set_field.argtypes = [vp, i32, i32, C.c_double]
        L.srack_patch_set_wave.argtypes = [vp, i32, fp, u32, C.c_float]
        L.srack_patch_connect.argtypes = [vp, i32, i32, i32, i32]
        L.srack_voices_configure.argtypes = [vp, u32]
        L.srack_voices_set_field_f32.argtypes = [vp, i32, i32, fp]
        L.srack_render.argtypes = [vp, u32, vp, vp, u32, vp]
        L.srack_render_info.argtypes = [vp, C.c_char_p, C.c_size_t]
        L.srack_device_alloc.argtypes = [C.POINTER(vp), C.c_size_t]
        L.srack_device_free.argtypes = [vp]
        L.srack_device_sync.argtypes = [vp]
        if hasattr(L, "srack_voices_set_waves"):
            L.srack_patch_set_wave_bank.argtypes = [vp, i32, fp, ip, fp, u32]
            L.srack_voices_set_waves.argtypes = [vp, i32, ip]
        self.h = vp()
        self.ok(L.srack_patch_create(sample_rate, buffer_size, channels, C.byref(self.h)))

    def ok(self, rc):
        if rc < 0:
            raise RuntimeError("srack error %d: %s" % (rc, self.L.srack_last_error().decode(errors="replace")))
        return rc

    def add_module(self, t):
        return self.ok(self.L.srack_patch_add_module(self.h, t))

    def set_field(self, m, f, v):
        self.ok(self.L.srack_patch_set_field(self.h, m, f, float(v)))

    def set_wave(self, m, samples, rate):
        a = np.ascontiguousarray(samples, dtype=np.float32)
        self.ok(self.L.srack_patch_set_wave(self.h, m, a.ctypes.data_as(C.POINTER(C.c_float)), a.size, float(rate)))

    def connect(self, a, ap, b, bp):
        self.ok(self.L.srack_patch_connect(self.h, a, ap, b, bp))

    def info(self):
        buf = C.create_string_buffer(4096)
        self.ok(self.L.srack_render_info(self.h, buf, 4096))
        return buf.value.decode()


def worker(args):
    import srack_pkg
    W = srack_pkg.load_workloads()
    V, T = args.voices, args.samples
    p = Raw(args.lib)
    ids = W.build_p4(p, wave=W.p4_wave(48000))
    p.ok(p.L.srack_voices_configure(p.h, V))
    depth, expo = W.p4_voice_params(V)
    for m, f, vals in ((ids["depth"], W.MATH_CONSTANT, depth), (ids["shaper"], W.NONLIN_CONSTANT, expo)):
        a = np.ascontiguousarray(vals, dtype=np.float32)
        p.ok(p.L.srack_voices_set_field_f32(p.h, m, f, a.ctypes.data_as(C.POINTER(C.c_float))))
    if args.bank:
        rng = np.random.default_rng(7)
        flat = rng.uniform(-1, 1, N_BANK * 48000).astype(np.float32)
        lengths, rates = np.full(N_BANK, 48000, dtype=np.intc), np.full(N_BANK, 44100.0, dtype=np.float32)
        p.ok(p.L.srack_patch_set_wave_bank(p.h, ids["smp"], flat.ctypes.data_as(C.POINTER(C.c_float)), lengths.ctypes.data_as(C.POINTER(C.c_int)),
                                           rates.ctypes.data_as(C.POINTER(C.c_float)), N_BANK))
        idx = (np.arange(V) % N_BANK).astype(np.intc)
        p.ok(p.L.srack_voices_set_waves(p.h, ids["smp"], idx.ctypes.data_as(C.POINTER(C.c_int))))
    d_fr, d_mx = C.c_void_p(), C.c_void_p()
    p.ok(p.L.srack_device_alloc(C.byref(d_fr), 2 * T * V * 4))
    p.ok(p.L.srack_device_alloc(C.byref(d_mx), 2 * T * 4))
    ms = []
    for step in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        p.ok(p.L.srack_render(p.h, T, d_fr, d_mx, 0, None))
        p.ok(p.L.srack_device_sync(None))
        if step >= args.warmup:
            ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    info = p.info()
    p.L.srack_device_free(d_fr)
    p.L.srack_device_free(d_mx)
    print(json.dumps({"ms_per_step": ms, "kernel": info.split("kernel=")[-1], "waves": ("waves=" in info) and info.split("waves=")[1].split()[0]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the other build of the library (leg a)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--voices", type=int, default=131072)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--legs", default="abcd")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per leg")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", help=argparse.SUPPRESS)
    ap.add_argument("--bank", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    tree = os.path.join(ROOT, "s-rack_amd", "libsrack_hip.so")
    legs = {"a": (args.parent, False, {}), "b": (tree, False, {}), "c": (tree, True, {"SRACK_JIT_SMP_WINDOW": "0"}), "d": (tree, True, {})}
    if "a" in args.legs and not args.parent:
        ap.error("leg a needs --parent")
    best = {leg: [] for leg in args.legs}
    for rnd in range(args.rounds):
        for leg in args.legs:
            lib, bank, env = legs[leg]
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--lib", os.path.abspath(lib), "--steps", str(args.steps), "--warmup", str(args.warmup),
                   "--voices", str(args.voices), "--samples", str(args.samples)] + (["--bank"] if bank else [])
            r = subprocess.run(cmd, env={**os.environ, **env}, capture_output=True, text=True, timeout=args.timeout)
            if r.returncode != 0:  # a leg that fails ends the run: nothing more is started on the device
                print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
                sys.exit("leg %s failed (exit %d)" % (leg, r.returncode))
            out = json.loads(r.stdout.strip().splitlines()[-1])
            best[leg].append(min(out["ms_per_step"]))
            print(json.dumps({"leg": leg, "round": rnd, **out}), flush=True)
    spread = {leg: max(v) - min(v) for leg, v in best.items()}
    summary = {"best_ms_per_round": best, "spread_ms": spread}
    if "a" in best and "c" in best:
        summary["c_over_a"] = round(float(np.median(best["c"]) / np.median(best["a"])), 4)
    if "a" in best and "b" in best:
        summary["b_minus_a_ms"] = [round(b - a, 3) for a, b in zip(best["a"], best["b"])]
    if "c" in best and "d" in best:
        bar = 4 * max(spread["c"], spread["d"])
        summary["d_minus_c_ms"] = [round(d - c, 3) for c, d in zip(best["c"], best["d"])]
        summary["window_bar_ms"] = round(bar, 3)
        summary["window_wins"] = all(c - d > bar for c, d in zip(best["c"], best["d"]))
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
