"""Every case of tests/test_gpu_vcf_b4.py in a process of its own (the library reads SRACK_VCF_B4 once): P1 through the flagship kernel with
per-voice cutoffs, resonances and starting states on both sides of the ladder's vote on its clamp behind the cubic (csrc/modules.hip.h,
vcf_b4_bounded; notes/r30.md), at every voice count, call shape and output mode of the suite, with everything rendered and the voice state
read back afterwards written to an .npz.  The test compares the .npz of SRACK_VCF_B4=1 with that of SRACK_VCF_B4=0 bit for bit and holds
the renders to the oracle.

    python tests/vcf_b4_driver.py <out.npz>
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import srack_pkg  # noqa: E402

VOICES = (2, 63, 64, 65, 200)
# One patch per voice count, its calls in this order, each continuing the one before (as tests/tile_uniform_driver.py)
CALLS = (1, 31, 32, 33, 95, 4103, 7, 243, 1024, 33)
MODES = ("fm", "f", "m")   # call c of voice count j renders MODES[(c + j) % 3]
STATS_VOICES = (65, 200)
STATS_CALLS = (95, 4103, 7, 1024, 33)
LFO_VAL = -1.0             # the gate's LFO at 220 Hz

# case -> the render flags it runs under.  Resonance 1 at these cutoffs is beyond the flattener's error budget (csrc/approx.cpp, module by
# module, which RENDER_KEEP_DEFAULT does not waive): flags 0 then renders the exact sources through the general path, and the flagship's
# default-mode vote never meets such a lane — b_half is the mixed wave it does meet.
CASES = {
    "a": (0, 1),                    # cfg3's draw, cutoffs U(0.05, 0.6): every wave votes yes
    "b": (0, 1),                    # cutoffs 0.88, 0.894, 0.897, 0.9 with resonance 0 and 1 inside every wave: the wave votes no
    "b_half": (0, 1),               # the same with resonance 0 and 0.5: within the budget, so flags 0 is the flagship's default mode
    "c90": (0, 1),                  # one voice per wave of case (a) warm: cutoff 0.9, b0 ... b3 = 1, b4 = -1, phase 0.99 — the clamp acts on the first sample
    "c89": (0, 1),                  # the same at cutoff 0.89 and resonance 0: the coefficients alone pass the vote, the state does not
    "c89_soft": (0, 1),             # cutoff 0.89, b4 = -0.95: passes the fourth stage's bound taken alone, 2p + |f| 0.95 <= 2.83, and the clamp acts
}
# the warm cases once more with a first call of full tiles: a first call of one sample runs the short tile's loop, which keeps every clamp,
# and leaves b4 = -1 behind — the tile copies without the clamp would never meet the state the case is about
LONG_CALLS = (4103, 33)
WARM = {"c90": (0.9, -1.0, 0.5), "c89": (0.89, -1.0, 0.0), "c89_soft": (0.89, -0.95, 0.5)}   # case -> (cutoff, b4, resonance) of the warm voice


def mode_of(j, c):
    return MODES[(c + j) % 3]


def hot_voices(V):
    """the warm voice of every wave of 64 (the last wave's, where it is partial, its last voice)"""
    return sorted({min(w * 64 + 37, V - 1) for w in range(-(-V // 64))})


def params(S, case, V):
    """-> [(module key, field, values[V])]: the per-voice overrides of the case, state fields included (f64 for the phase)"""
    f = np.float32
    det, cut = S.p1_voice_params(V)
    v = np.arange(V)
    if case == "a":
        return [("osc_a", S.OSC_VAL, det), ("vcf", S.VCF_FREQ, cut)]
    if case in ("b", "b_half"):
        cut = np.array([0.88, 0.894, 0.897, 0.9], f)[v % 4]
        res = np.where((v // 4) % 2 == 1, f(1.0 if case == "b" else 0.5), f(0.0)).astype(f)
        return [("osc_a", S.OSC_VAL, det), ("vcf", S.VCF_FREQ, cut), ("vcf", S.VCF_RES, res)]
    hot_cut, hot_b4, hot_res = WARM[case]
    hot = hot_voices(V)
    cut = cut.copy()
    cut[hot] = f(hot_cut)
    b = np.zeros(V, f)
    b[hot] = f(1.0)
    b4 = np.zeros(V, f)
    b4[hot] = f(hot_b4)
    pos = np.zeros(V, np.float64)
    pos[hot] = 0.99
    res = np.full(V, 0.5, f)   # the patch's own resonance everywhere but in the warm voice
    res[hot] = f(hot_res)
    return [("osc_a", S.OSC_VAL, det), ("vcf", S.VCF_FREQ, cut), ("vcf", S.VCF_RES, res), ("osc_a", S.OSC_POS, pos), ("vcf", S.VCF_ST_B0, b),
            ("vcf", S.VCF_ST_B1, b), ("vcf", S.VCF_ST_B2, b), ("vcf", S.VCF_ST_B3, b), ("vcf", S.VCF_ST_B4, b4)]


def build(g, S):
    return S.build_p1(g, adsr="finite", lfo_val=LFO_VAL)


def overrides(S, ids, case, V):
    return [(ids[k], fld, vals) for k, fld, vals in params(S, case, V)]


def gpu_patch(S, case, V):
    p = S.Patch(48000, 1024, 2)
    ids = build(p, S)
    p.configure_voices(V)
    for m, fld, vals in overrides(S, ids, case, V):
        p.set_voice_field(m, fld, vals)
    return p, ids


def state(S, p, ids, out, tag):
    out[f"{tag}_osc_pos"] = p.get_voice_field(ids["osc_a"], S.OSC_POS)
    for name in ("F", "P", "Q", "B0", "B1", "B2", "B3", "B4"):
        out[f"{tag}_vcf_{name}"] = p.get_voice_field(ids["vcf"], getattr(S, "VCF_ST_" + name))


def main():
    out_path = sys.argv[1]
    S = srack_pkg.load()
    out = {}
    for case, flag_list in CASES.items():
        for flags in flag_list:
            for j, V in enumerate(VOICES):
                p, ids = gpu_patch(S, case, V)
                infos = []
                for c, n in enumerate(CALLS):
                    what = mode_of(j, c)
                    fr, mx = p.render(n, frames="f" in what, mix="m" in what, flags=flags)
                    if fr is not None:
                        out[f"{case}_x{flags}_v{V}_c{c}_fr"] = fr[0]
                    if mx is not None:
                        out[f"{case}_x{flags}_v{V}_c{c}_mx"] = mx
                    infos.append(p.info())
                state(S, p, ids, out, f"{case}_x{flags}_v{V}")
                out[f"{case}_x{flags}_v{V}_infos"] = np.array(infos)
            for V in VOICES if case in WARM else ():
                p, ids = gpu_patch(S, case, V)
                infos = []
                for c, n in enumerate(LONG_CALLS):
                    fr, mx = p.render(n, frames=True, mix=True, flags=flags)
                    out[f"{case}_x{flags}_l{V}_c{c}_fr"] = fr[0]
                    out[f"{case}_x{flags}_l{V}_c{c}_mx"] = mx
                    infos.append(p.info())
                state(S, p, ids, out, f"{case}_x{flags}_l{V}")
                out[f"{case}_x{flags}_l{V}_infos"] = np.array(infos)
            for V in STATS_VOICES:
                p, ids = gpu_patch(S, case, V)
                infos = []
                for c, n in enumerate(STATS_CALLS):
                    fr, mx, st = p.render_stats(n, frames=True, mix=True, flags=flags)
                    out[f"{case}_x{flags}_s{V}_c{c}_fr"] = fr[0]
                    out[f"{case}_x{flags}_s{V}_c{c}_mx"] = mx
                    out[f"{case}_x{flags}_s{V}_c{c}_st"] = st
                    infos.append(p.info())
                state(S, p, ids, out, f"{case}_x{flags}_s{V}")
                out[f"{case}_x{flags}_s{V}_infos"] = np.array(infos)
    np.savez(out_path, **out)


if __name__ == "__main__":
    main()
