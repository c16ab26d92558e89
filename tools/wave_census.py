#!/usr/bin/env python3
"""tools/wave_census.py — where and when the waves of the flagship kernel (render_voice_chain_track) run, launch by launch.

The census is a tools-only build of the library: lane 0 of every wave stamps the 100 MHz constant clock at entry and at exit, with its
XCC / SE / CU / SIMD (fused.hip.h, SRK_WAVE_CENSUS).  The default library has none of it.  Build the variant beside the real one:

    make -C s-rack_amd/csrc EXTRA=-DSRK_WAVE_CENSUS BUILD=build_census OUT=../libsrack_hip_census.so
    python tools/wave_census.py --lib s-rack_amd/libsrack_hip_census.so [--json census.json]

It renders config 3 (bench.py's default workload: P1, 262 144 voices, calls of 48 000 samples) `--warmup` times unrecorded, then one call
recorded, and reports per launch and over the call's full-length launches:
  * voice waves per SIMD (over the launch, and the most resident at one time),
  * the spread of the SIMDs' last end times and the spread of end times within a SIMD, in % of the launch,
  * when the control block ends, relative to the launch and to the last voice wave,
  * wave lifetime / launch length (the counters' SQ_WAVE_CYCLES x 4 / SQ_WAVES over GRBM_GUI_ACTIVE / 8: 0.771 in profiles/r06_summary.json),
  * the pacing groups (wave.hip.h pace_key: a SIMD's voice waves): how many keys have exactly four members, and — a paced launch records
    them — the steps each wave took and the largest lead any wave saw.
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import shutil
import sys
import tempfile
from collections import Counter, defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "s-rack_amd")


def load_variant(lib_path):
    """The package's Python files beside a copy of the variant library, imported as module `srack_amd` (the binding loads the
    libsrack_hip.so next to its own file)."""
    tmp = tempfile.mkdtemp(prefix="srack_census_")
    for f in os.listdir(PKG_DIR):
        if f.endswith(".py"):
            shutil.copy(os.path.join(PKG_DIR, f), tmp)
    shutil.copy(lib_path, os.path.join(tmp, "libsrack_hip.so"))
    spec = importlib.util.spec_from_file_location("srack_amd", os.path.join(tmp, "__init__.py"), submodule_search_locations=[tmp])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["srack_amd"] = mod
    spec.loader.exec_module(mod)
    if not hasattr(mod.lib, "srack_census_begin"):
        raise SystemExit(f"{lib_path} is not a census build (make EXTRA=-DSRK_WAVE_CENSUS ...)")
    return mod, tmp


def pct(x, span):
    return round(100.0 * float(x) / span, 2)


def pace_key(hw, xcc):
    """wave.hip.h pace_key: XCC (3 bits), HW_ID's CU / SH / SE bits 8 .. 15, the SIMD — not the pipe, not the wave slot."""
    hw, xcc = np.asarray(hw, np.int64), np.asarray(xcc, np.int64)
    return ((xcc & 7) << 10) | (((hw >> 8) & 0xFF) << 2) | ((hw >> 4) & 3)


def pace_groups(rec):
    """The pacing groups of one launch's records: the voice waves by pace key.  Word [6] of a paced wave: 4 = paced, bits 3 .. 15 the key
    the wave used, bits 16 .. 23 the largest lead it saw (steps summed over the group's other waves), bits 24 .. 31 the steps it took."""
    rec = np.asarray(rec, np.uint32).reshape(-1, 8)
    flags = rec[:, 6]
    voice = ((flags & 1) != 0) & ((flags & 2) == 0)
    if not voice.any():
        return None
    key = pace_key(rec[:, 4], rec[:, 5])
    members = Counter(int(k) for k in key[voice])
    sizes = Counter(members.values())
    out = {"keys": len(members), "keys_with_four": int(sizes.get(4, 0)), "members_per_key": {str(k): v for k, v in sorted(sizes.items())}}
    paced = voice & ((flags & 4) != 0)
    out["paced_waves"] = int(paced.sum())
    if paced.any():
        f = flags[paced].astype(np.int64)
        out["key_mismatches"] = int((((f >> 3) & 0x1FFF) != key[paced]).sum())   # the key the wave used against the decode of its HW_ID here
        out["largest_lead"] = int(((f >> 16) & 0xFF).max())
        steps = (f >> 24) & 0xFF
        out["steps"] = {"min": int(steps.min()), "max": int(steps.max())}
    return out


def analyse(rec):
    """rec: [slots][8] uint32 of one launch (fused.hip.h census_begin)."""
    flags = rec[:, 6]
    have = (flags & 1) != 0
    if not have.any():
        return None
    t0 = rec[:, 0].astype(np.int64) | (rec[:, 1].astype(np.int64) << 32)
    t1 = rec[:, 2].astype(np.int64) | (rec[:, 3].astype(np.int64) << 32)
    ctl = have & ((flags & 2) != 0)
    voice = have & ~ctl
    if (t1[have] == 0).any():
        return {"incomplete": int((t1[have] == 0).sum())}
    begin, end = t0[have].min(), t1[have].max()
    span = float(end - begin)
    hw, xcc = rec[:, 4], rec[:, 5] & 0xF
    simd = (hw >> 4) & 3
    cu_key = (xcc.astype(np.int64) << 8) | ((hw >> 8) & 0xFF)   # XCC, then HW_ID's CU / SH / SE bits: one CU
    simd_key = (cu_key << 2) | simd
    se = (hw >> 13) & 3
    out = {"span_ticks_10ns": int(span), "voice_waves": int(voice.sum()), "control_block": bool(ctl.any())}
    # waves per SIMD: over the launch, and the most resident at one time
    per_simd = defaultdict(list)
    for i in np.nonzero(voice)[0]:
        per_simd[int(simd_key[i])].append((int(t0[i]), int(t1[i])))
    counts = Counter(len(v) for v in per_simd.values())
    peak = Counter()
    last_end, spread_in = [], []
    for v in per_simd.values():
        ev = sorted([(a, 1) for a, _ in v] + [(b, -1) for _, b in v], key=lambda e: (e[0], e[1]))
        cur = best = 0
        for _, d in ev:
            cur += d
            best = max(best, cur)
        peak[best] += 1
        ends = [b for _, b in v]
        last_end.append(max(ends) - begin)
        spread_in.append(max(ends) - min(ends))
    last_end, spread_in = np.array(last_end, np.float64), np.array(spread_in, np.float64)
    out["simds"] = len(per_simd)
    out["cus"] = len(set(int(k) >> 2 for k in per_simd))
    out["xccs"] = sorted(set(int(x) for x in xcc[voice]))
    out["ses_per_xcc"] = len(set(int(s) for s in se[voice]))
    out["waves_per_simd"] = {str(k): v for k, v in sorted(counts.items())}
    out["peak_resident_per_simd"] = {str(k): v for k, v in sorted(peak.items())}
    out["simd_last_end_pct"] = {q: pct(np.percentile(last_end, p), span) for q, p in (("min", 0), ("p10", 10), ("p50", 50), ("p90", 90), ("max", 100))}
    out["simd_last_end_spread_pct"] = pct(last_end.max() - last_end.min(), span)
    out["end_spread_within_simd_pct"] = {q: pct(np.percentile(spread_in, p), span) for q, p in (("p50", 50), ("p90", 90), ("max", 100))}
    vs = t0[voice] - begin
    out["voice_start_spread_pct"] = {q: pct(np.percentile(vs, p), span) for q, p in (("p50", 50), ("p90", 90), ("max", 100))}
    life = (t1[voice] - t0[voice]).astype(np.float64)
    out["voice_lifetime_over_launch"] = round(float(life.mean()) / span, 4)
    all_life = (t1[have] - t0[have]).astype(np.float64)
    out["wave_lifetime_over_launch_all"] = round(float(all_life.mean()) / span, 4)   # the counters' ratio: every wave, the control block's too
    if ctl.any():
        i = int(np.nonzero(ctl)[0][0])
        out["control"] = {"start_pct": pct(t0[i] - begin, span), "end_pct": pct(t1[i] - begin, span),
                          "end_minus_last_voice_pct": pct(t1[i] - t1[voice].max(), span), "xcc": int(xcc[i]), "simd": int(simd[i]),
                          "voice_waves_on_its_simd": len(per_simd.get(int(simd_key[i]), []))}
    out["pace"] = pace_groups(rec)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--lib", required=True, help="the census build of libsrack_hip.so")
    ap.add_argument("--voices", type=int, default=262144)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--warmup", type=int, default=3, help="unrecorded calls first")
    ap.add_argument("--flags", type=int, default=0, help="render flags (1: exact mode)")
    ap.add_argument("--json", help="write the per-launch records' summary here")
    args = ap.parse_args()
    S, tmp = load_variant(os.path.abspath(args.lib))
    try:
        L = S.lib
        L.srack_census_begin.argtypes = [C.c_uint32, C.c_uint32]
        L.srack_census_read.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32]
        V, T = args.voices, args.samples
        B, build, overrides = S.bench_workload("cfg3", V)
        p = S.Patch(48000, B, 2)
        ids = build(p)
        p.configure_voices(V)
        for m, f, v in overrides(ids):
            p.set_voice_field(m, f, v)
        n_planes, _ = p.planes()
        d_fr, d_mx = C.c_void_p(), C.c_void_p()
        S._check(L.srack_device_alloc(C.byref(d_fr), n_planes * T * V * 4))
        S._check(L.srack_device_alloc(C.byref(d_mx), 2 * T * 4))
        for _ in range(args.warmup):
            p.render_raw(T, d_fr.value, d_mx.value, args.flags, None)
        S._check(L.srack_device_sync(None))
        max_launches = 256
        slots = (V + 63) // 64 + 1
        max_slots = slots * max_launches
        S._check(L.srack_census_begin(max_slots, max_launches))
        p.render_raw(T, d_fr.value, d_mx.value, args.flags, None)
        buf = np.zeros(max_slots * 8, np.uint32)
        per = np.zeros(max_launches, np.uint32)
        n = S._check(L.srack_census_read(buf.ctypes.data_as(C.POINTER(C.c_uint32)), max_slots, per.ctypes.data_as(C.POINTER(C.c_uint32)), max_launches))
        info = p.info()
        L.srack_device_free(d_fr)
        L.srack_device_free(d_mx)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    launches, off = [], 0
    for k in range(n):
        rec = buf[off * 8:(off + int(per[k])) * 8].reshape(-1, 8)
        off += int(per[k])
        launches.append(analyse(rec))
    full = [x for x in launches if x and "span_ticks_10ns" in x]
    # the call's full-length launches: all but the shorter last one
    body = full[:-1] if len(full) > 1 else full

    def med(key, sub=None):
        vals = [x[key] if sub is None else x[key][sub] for x in body if key in x]
        return round(float(np.median(vals)), 4) if vals else None

    summary = {"lib": os.path.basename(args.lib), "voices": V, "samples": T, "flags": args.flags, "launches": n, "info": info,
               "median_over_full_launches": {
                   "span_ms": round(med("span_ticks_10ns") * 1e-5, 4),
                   "voice_lifetime_over_launch": med("voice_lifetime_over_launch"),
                   "wave_lifetime_over_launch_all": med("wave_lifetime_over_launch_all"),
                   "simd_last_end_spread_pct": med("simd_last_end_spread_pct"),
                   "end_spread_within_simd_p50_pct": med("end_spread_within_simd_pct", "p50"),
                   "end_spread_within_simd_max_pct": med("end_spread_within_simd_pct", "max"),
                   "simd_last_end_min_pct": med("simd_last_end_pct", "min"),
                   "voice_start_spread_max_pct": med("voice_start_spread_pct", "max"),
                   "control_end_pct": med("control", "end_pct") if all("control" in x for x in body) else None,
               },
               "waves_per_simd_all_launches": dict(sum((Counter(x["waves_per_simd"]) for x in full), Counter())),
               "peak_resident_per_simd_all_launches": dict(sum((Counter(x["peak_resident_per_simd"]) for x in full), Counter())),
               "per_launch": launches}
    text = json.dumps(summary, indent=1)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")
    s = dict(summary)
    s.pop("per_launch")
    print(json.dumps(s, indent=1))
    for k, x in enumerate(launches):
        if x and "span_ticks_10ns" in x:
            print(f"launch {k:2d}: {x['span_ticks_10ns'] / 1e5:.3f} ms  waves/SIMD {x['waves_per_simd']}  peak {x['peak_resident_per_simd']}  "
                  f"life/launch {x['voice_lifetime_over_launch']:.3f}  SIMD last-end spread {x['simd_last_end_spread_pct']} %  "
                  f"within-SIMD max {x['end_spread_within_simd_pct']['max']} %  ctl end {x.get('control', {}).get('end_pct')} %  "
                  f"pace keys with four {x['pace']['keys_with_four']} / {x['pace']['keys']}  largest lead {x['pace'].get('largest_lead')}")
        else:
            print(f"launch {k:2d}: {x}")


if __name__ == "__main__":
    main()
