"""One envelope kind of tests/test_gpu_flagship_tile_uniform.py in a process of its own (the library reads SRACK_TILE_PLAIN once): P1 with
per-voice detune and cutoff through the flagship kernel, in both modes (flags 0 and 1), at every voice count and call shape of the
suite, with everything rendered and the voice state read back afterwards written to an .npz.  The test compares the .npz of
SRACK_TILE_PLAIN=1 with that of SRACK_TILE_PLAIN=0 bit for bit and holds the renders to the oracle.

    python tests/tile_uniform_driver.py <kind> <out.npz>
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import srack_pkg  # noqa: E402

# (One voice alone has nothing voice-invariant to hoist: its envelope is no track, and it renders through render_voice_chain.  It stays in
# the suite as the library renders it; two voices are the fewest the flagship kernel takes.)
VOICES = (1, 2, 63, 64, 65, 200)
# One patch per voice count, its calls in this order, each continuing the one before: single calls of 1, 31, 32, 33, 95 and 4 103 samples
# (less than a tile, one short of a tile, a tile, a tile and one, three tiles short of one, several chunks and a 7-sample tail), then a
# session of 7, 243, 1 024 and 33, which starts every later call's track at a sample offset that is no multiple of 8.
CALLS = (1, 31, 32, 33, 95, 4103, 7, 243, 1024, 33)
MODES = ("fm", "f", "m")   # call c of voice count j renders MODES[(c + j) % 3]: every mode meets every call shape
STATS_VOICES = (65, 200)   # the statistics variant of the kernel: frames and mix decided at run time
STATS_CALLS = (95, 4103, 7, 1024, 33)
LFO_VAL = -1.0             # the gate's LFO at 220 Hz: an edge every 109 samples

# kind -> (ADSR fields, VCA negative: None, a value for every voice, or "some")
KINDS = {
    # the suite's finite ADSR: 0.0 until the gate first opens, > 0 from there
    "finite": (dict(a=0.01, d=0.1, s=0.5, r=0.2), None),
    # a decay of 48 samples to a sustain of 0.0: the envelope reaches exactly 0.0 in the middle of a gate, again and again
    "sustain0": (dict(a=0.0005, d=0.001, s=0.0, r=0.0005), None),
    # a sustain below zero: the decay crosses 0.0 and the envelope stays negative, which the VCA passes only with `negative` set
    "negative": (dict(a=0.0005, d=0.001, s=-0.4, r=0.0005), 1),
    "negative_some": (dict(a=0.0005, d=0.001, s=-0.4, r=0.0005), "some"),
}


def mode_of(j, c):
    return MODES[(c + j) % 3]


def build(g, S, kind, V):
    """The kind's patch on `g` (a product Patch or an OraclePatch) -> (ids, per-voice overrides)."""
    adsr, neg = KINDS[kind]
    ids = S.build_p1(g, adsr="finite", lfo_val=LFO_VAL)
    g.set_field(ids["adsr"], S.ADSR_A_SEC, adsr["a"])
    g.set_field(ids["adsr"], S.ADSR_D_SEC, adsr["d"])
    g.set_field(ids["adsr"], S.ADSR_S_VAL, adsr["s"])
    g.set_field(ids["adsr"], S.ADSR_R_SEC, adsr["r"])
    det, cut = S.p1_voice_params(V)
    over = [(ids["osc_a"], S.OSC_VAL, det), (ids["vcf"], S.VCF_FREQ, cut)]
    if neg == "some":
        over.append((ids["vca"], S.VCA_NEGATIVE, (np.arange(V) % 3 == 0).astype(np.float32)))
    elif neg is not None:
        g.set_field(ids["vca"], S.VCA_NEGATIVE, neg)
    return ids, over


def gpu_patch(S, kind, V):
    p = S.Patch(48000, 1024, 2)
    ids, over = build(p, S, kind, V)
    p.configure_voices(V)
    for m, f, v in over:
        p.set_voice_field(m, f, v)
    return p, ids


def state(S, p, ids, out, tag):
    out[f"{tag}_osc_pos"] = p.get_voice_field(ids["osc_a"], S.OSC_POS)
    for name in ("F", "P", "Q", "B0", "B1", "B2", "B3", "B4"):
        out[f"{tag}_vcf_{name}"] = p.get_voice_field(ids["vcf"], getattr(S, "VCF_ST_" + name))


def main():
    kind, out_path = sys.argv[1], sys.argv[2]
    S = srack_pkg.load()
    out = {}
    for flags in (0, 1):
        for j, V in enumerate(VOICES):
            p, ids = gpu_patch(S, kind, V)
            infos = []
            for c, n in enumerate(CALLS):
                what = mode_of(j, c)
                fr, mx = p.render(n, frames="f" in what, mix="m" in what, flags=flags)
                if fr is not None:
                    out[f"x{flags}_v{V}_c{c}_fr"] = fr[0]
                if mx is not None:
                    out[f"x{flags}_v{V}_c{c}_mx"] = mx
                infos.append(p.info())
            state(S, p, ids, out, f"x{flags}_v{V}")
            out[f"x{flags}_v{V}_infos"] = np.array(infos)
        for V in STATS_VOICES:
            p, ids = gpu_patch(S, kind, V)
            infos = []
            for c, n in enumerate(STATS_CALLS):
                fr, mx, st = p.render_stats(n, frames=True, mix=True, flags=flags)
                out[f"x{flags}_s{V}_c{c}_fr"] = fr[0]
                out[f"x{flags}_s{V}_c{c}_mx"] = mx
                out[f"x{flags}_s{V}_c{c}_st"] = st
                infos.append(p.info())
            state(S, p, ids, out, f"x{flags}_s{V}")
            out[f"x{flags}_s{V}_infos"] = np.array(infos)
    np.savez(out_path, **out)


if __name__ == "__main__":
    main()
