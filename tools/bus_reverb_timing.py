"""tools/bus_reverb_timing.py — what a stereo reverb costs per second of audio, two ways (notes/r14.md):

  --per-voice N   what the library offered before the bus reverbs: an N-voice patch of two oscillators through a FreeverbModule with
                  a per-voice detune, so that every voice has a reverb of its own (tile_freeverb, one lane per reverb); one render of
                  48 000 samples.  Needs nothing of the bus reverbs: runs against an older build of the library as well.
  --buses N ...   srack_buses_reverb for N enabled buses over 48 000 samples at 48 kHz: one call, and a tick session of 1024-sample calls.

Timed with HIP events on the null stream around the call(s) alone, after one untimed pass (allocations, first launch); `--rounds` timed
passes each.  One JSON line per configuration, ms per second of audio.

    python tools/bus_reverb_timing.py --per-voice 64 --buses 1 64 1024
"""
import argparse
import ctypes as C
import json
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import srack_pkg  # noqa: E402

SR, T, TICK = 48000, 48000, 1024


class Events:
    """hipEvent pairs through the HIP runtime the library itself is linked against"""

    def __init__(self):
        srack_pkg.load()  # (the library first: the runtime found below is the one it brought in)
        with open("/proc/self/maps") as f:
            paths = sorted({ln.split()[-1] for ln in f if "libamdhip64.so" in ln})
        assert len(paths) == 1, paths
        self.hip = C.CDLL(paths[0])
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [C.c_void_p]
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def time(self, fn):
        assert self.hip.hipEventRecord(self.a, None) == 0
        fn()
        assert self.hip.hipEventRecord(self.b, None) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return float(ms.value)


def device_buffer(S, nbytes, src=None):
    d = C.c_void_p()
    S._check(S.lib.srack_device_alloc(C.byref(d), nbytes))
    if src is not None:
        S._check(S.lib.srack_device_from_host(d, src.ctypes.data_as(C.c_void_p), src.nbytes, None))
    return d


def per_voice(S, ev, V, rounds):
    p = S.Patch(SR, 1024, 2)
    osc, osc2, fv, out = p.add_module(S.MOD_OSCILLATOR), p.add_module(S.MOD_OSCILLATOR), p.add_module(S.MOD_FREEVERB), p.add_module(S.MOD_OUTPUT)
    p.set_field(osc2, S.OSC_VAL, 0.37)
    p.connect(osc, S.OSC_OUT_SAW, fv, 0)
    p.connect(osc2, S.OSC_OUT_SQUARE, fv, 1)
    p.connect(fv, 0, out, 0)
    p.connect(fv, 1, out, 1)
    p.configure_voices(V)
    p.set_voice_field(osc, S.OSC_VAL, np.linspace(-2.0, 1.0, V).astype(np.float32))
    n_planes, _ = p.planes()
    d_fr, d_mx = device_buffer(S, n_planes * T * V * 4), device_buffer(S, 2 * T * 4)
    ms = []
    for k in range(rounds + 1):
        x = ev.time(lambda: p.render_raw(T, d_fr, d_mx))
        if k:
            ms.append(x)
    info = p.info()
    for d in (d_fr, d_mx):
        S.lib.srack_device_free(d)
    return {"what": "per-voice FreeverbModule", "reverbs": V, "kernel": info.split("kernel=")[-1], "ms_per_second_of_audio": [round(x, 3) for x in ms]}


def buses(S, ev, NB, rounds):
    p = S.Patch(SR, 1024, 2)
    S.build_p1(p)
    p.configure_voices(1)
    p.set_buses(NB)
    rng = np.random.default_rng(NB)
    p.set_bus_reverbs(np.column_stack([rng.uniform(0, 2, NB), np.zeros(NB), rng.uniform(0.2, 1, NB), rng.uniform(0, 1, NB), rng.uniform(0, 1, NB), rng.uniform(0, 1, NB)]))
    x = rng.random((NB, 2, T), dtype=np.float32) * np.float32(2) - np.float32(1)  # noise in bursts of 1000 samples, 30 % of the time
    x *= (rng.random((NB, 2, T // 1000)) < 0.3).astype(np.float32).repeat(1000, axis=2)
    d_in, d_out = device_buffer(S, x.nbytes, x), device_buffer(S, x.nbytes)
    one, ticked = [], []
    for k in range(rounds + 1):
        a = ev.time(lambda: p.bus_reverb_raw(T, d_in, d_out))
        if k:
            one.append(a)

    def session():  # (a tick session hands the library one 1024-sample slice of every bus per call: the slices are laid out call by call)
        for c in range(len(cuts)):
            p.bus_reverb_raw(cuts[c], d_tin[c], d_tout[c])

    cuts = [TICK] * (T // TICK) + ([T % TICK] if T % TICK else [])
    at = np.concatenate(([0], np.cumsum(cuts)))
    tin = [np.ascontiguousarray(x[:, :, at[c]:at[c + 1]]) for c in range(len(cuts))]
    d_tin = [device_buffer(S, a.nbytes, a) for a in tin]
    d_tout = [device_buffer(S, a.nbytes) for a in tin]
    for k in range(rounds + 1):
        a = ev.time(session)
        if k:
            ticked.append(a)
    info = p.info()
    for d in [d_in, d_out] + d_tin + d_tout:
        S.lib.srack_device_free(d)
    return {"what": "srack_buses_reverb", "reverbs": NB, "info": re.search(r"busfx=\d+\[block \d+\]", info).group(0),
            "ms_per_second_of_audio_one_call": [round(v, 3) for v in one], "ms_per_second_of_audio_calls_of_1024": [round(v, 3) for v in ticked]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-voice", type=int, default=0)
    ap.add_argument("--buses", type=int, nargs="*", default=[])
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    S = srack_pkg.load()
    ev = Events()
    if args.per_voice:
        print(json.dumps(per_voice(S, ev, args.per_voice, args.rounds)), flush=True)
    for nb in args.buses:
        print(json.dumps(buses(S, ev, nb, args.rounds)), flush=True)


if __name__ == "__main__":
    main()
