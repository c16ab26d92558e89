"""tools/seq_bank_bench.py — what a sequence per voice costs the sequencers, on ONE box (boxes differ by a few percent: legs are only
comparable within a run).  Not bench.py: P3's patch at 262 144 voices x 48 000 samples, frames and mix as bench.py asks for them, in four
legs that alternate for three rounds, each leg a fresh process under its own time limit:

    a  another build of the library (--parent path/to/libsrack_hip.so: the parent commit's), a per-voice clock pitch: the sequencers are
       per voice already, on the module's one sequence                                                                the yardstick
    b  this tree's library, the same call                                                                              must tie with a
    c  this tree, a bank of 1024 distinct sequences per sequencer, voice v plays v % 1024: the per-lane gather
    e  c on the shared clock (no per-voice clock pitch: the sequencers are per voice only because of the assignment)        "c'"
(Legs d and f were c and e with a step-major LDS tile per sequencer, behind an environment knob; the tile lost — notes/r12.md R12.2 —
and went, the knob with it.)

    python tools/seq_bank_bench.py --parent path/to/parent/libsrack_hip.so [--rounds 3] [--steps 3] [--voices 262144] [--samples 48000]

Prints one JSON line per leg and round ({"leg", "round", "ms_per_step": [...], "kernel", "sequences"}), then a summary with c / a — the
price of per-voice sequences.  The library is driven through ctypes directly (the binding in s-rack_amd/ loads one fixed path); the patch
comes from workloads.py.
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
    """the few calls build_p3 makes, on a library loaded from any path"""

    def __init__(self, path, sample_rate=48000, buffer_size=1024, channels=2):
        self.L = L = C.CDLL(path)
        vp, i32, u32, fp, ip = C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_int)
        L.srack_last_error.restype = C.c_char_p
        L.srack_patch_create.argtypes = [u32, u32, u32, C.POINTER(vp)]
        L.srack_patch_destroy.argtypes = [vp]
        L.srack_patch_add_module.argtypes = [vp, i32]
        L.srack_patch_set_field.argtypes = [vp, i32, i32, C.c_double]
        L.srack_patch_set_step.argtypes = [vp, i32, i32, i32, i32, i32]
        L.srack_patch_connect.argtypes = [vp, i32, i32, i32, i32]
        L.srack_voices_configure.argtypes = [vp, u32]
        L.srack_voices_set_field_f32.argtypes = [vp, i32, i32, fp]
        L.srack_render.argtypes = [vp, u32, vp, vp, u32, vp]
        L.srack_render_info.argtypes = [vp, C.c_char_p, C.c_size_t]
        L.srack_device_alloc.argtypes = [C.POINTER(vp), C.c_size_t]
        L.srack_device_free.argtypes = [vp]
        L.srack_device_sync.argtypes = [vp]
        if hasattr(L, "srack_voices_set_sequences"):
            L.srack_patch_set_sequence_bank.argtypes = [vp, i32, vp, vp, ip, u32]
            L.srack_voices_set_sequences.argtypes = [vp, i32, ip]
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

    def set_step(self, m, channel, step, state, value=0):
        self.ok(self.L.srack_patch_set_step(self.h, m, channel, step, state, value))

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
    _, build, overrides = W.bench_workload("p3", V)
    p = Raw(args.lib)
    ids = build(p)
    p.ok(p.L.srack_voices_configure(p.h, V))
    per_voice = list(overrides(ids))
    if not args.shared_clock:   # a clock pitch per voice, +-0.1 octave around the patch's own: every lane steps on its own samples
        per_voice.append((ids["clock"], W.OSC_VAL, -4.0 + np.linspace(-0.1, 0.1, V)))
    for m, f, vals in per_voice:
        a = np.ascontiguousarray(vals, dtype=np.float32)
        p.ok(p.L.srack_voices_set_field_f32(p.h, m, f, a.ctypes.data_as(C.POINTER(C.c_float))))
    if args.bank:
        rng = np.random.default_rng(7)
        lengths = rng.integers(1, 65, N_BANK).astype(np.intc)
        idx = (np.arange(V) % N_BANK).astype(np.intc)
        for module, channels in ((ids["grid"], 1), (ids["pat"], 8)):
            states = rng.integers(0, 3, (N_BANK, channels, 64)).astype(np.uint8)
            values = rng.integers(0, 25, (N_BANK, 64)).astype(np.uint16)   # two octaves of notes, as P3's own
            p.ok(p.L.srack_patch_set_sequence_bank(p.h, module, states.ctypes.data, values.ctypes.data, lengths.ctypes.data_as(C.POINTER(C.c_int)), N_BANK))
            p.ok(p.L.srack_voices_set_sequences(p.h, module, idx.ctypes.data_as(C.POINTER(C.c_int))))
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
    print(json.dumps({"ms_per_step": ms, "kernel": info.split("kernel=")[-1], "sequences": ("sequences=" in info) and info.split("sequences=")[1].split()[0]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the other build of the library (leg a)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--voices", type=int, default=262144)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--legs", default="abce")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per leg")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", help=argparse.SUPPRESS)
    ap.add_argument("--bank", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--shared-clock", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    tree = os.path.join(ROOT, "s-rack_amd", "libsrack_hip.so")
    legs = {"a": (args.parent, False, False, {}), "b": (tree, False, False, {}), "c": (tree, True, False, {}), "e": (tree, True, True, {})}
    if "a" in args.legs and not args.parent:
        ap.error("leg a needs --parent")
    best = {leg: [] for leg in args.legs}
    for rnd in range(args.rounds):
        for leg in args.legs:
            lib, bank, shared, env = legs[leg]
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--lib", os.path.abspath(lib), "--steps", str(args.steps), "--warmup", str(args.warmup),
                   "--voices", str(args.voices), "--samples", str(args.samples)] + (["--bank"] if bank else []) + (["--shared-clock"] if shared else [])
            r = subprocess.run(cmd, env={**os.environ, **env}, capture_output=True, text=True, timeout=args.timeout)
            if r.returncode != 0:  # a leg that fails ends the run: nothing more is started on the device
                print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
                sys.exit("leg %s failed (exit %d)" % (leg, r.returncode))
            out = json.loads(r.stdout.strip().splitlines()[-1])
            best[leg].append(min(out["ms_per_step"]))
            print(json.dumps({"leg": leg, "round": rnd, **out}), flush=True)
    spread = {leg: max(v) - min(v) for leg, v in best.items()}
    summary = {"best_ms_per_round": best, "spread_ms": spread}
    for leg in "ce":
        if "a" in best and leg in best:
            summary[leg + "_over_a"] = round(float(np.median(best[leg]) / np.median(best["a"])), 4)
    if "a" in best and "b" in best:
        summary["b_minus_a_ms"] = [round(b - a, 3) for a, b in zip(best["a"], best["b"])]
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
