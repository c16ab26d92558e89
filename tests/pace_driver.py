"""One case of tests/test_gpu_pace.py in a process of its own (the library reads SRACK_PACE once): P1 as tests/test_gpu_flagship_shapes.py
builds it, rendered through the flagship kernel, with everything rendered and the voice state read back afterwards written to an .npz.
The test compares the .npz of SRACK_PACE=1 with that of SRACK_PACE=0 bit for bit and holds the frames to the oracle.

    python tests/pace_driver.py <case> <flags> <out.npz>
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import srack_pkg  # noqa: E402

# case -> (voice counts of its patches, samples per call, calls per patch)
CASES = {
    "small": ((64,), 100, 1),                    # four 16-voice waves, and not one pace step
    "chunks": ((257,), 3 * 4096 + 100, 2),       # a partial wave, several chunks, a last launch shorter than a pace interval, the table reused
    "grid": ((4097 * 64 + 5,), 4500, 1),         # more than four waves per SIMD: late joiners
    "stats": ((257,), 9000, 1),                  # the statistics variant of the kernel
    "two": ((100, 192), 5000, 2),                # two handles on one device, rendered alternately
}
GRID_PICK_SEED = 7


def grid_pick(V):
    """The sampled voices of test_gpu_flagship_shapes.test_full_grid_and_a_partial_wave."""
    return np.unique(np.array([0, 1, 63, 64, 255, 256, 4095 * 64 - 1, 4096 * 64 - 1, 4096 * 64, 4097 * 64 - 1, 4097 * 64, V - 2, V - 1]
                              + list(np.random.default_rng(GRID_PICK_SEED).integers(0, V, 19))))


def p1(g, S, V):
    ids = S.build_p1(g, adsr="finite", lfo_val=-4.0)
    det, cut = S.p1_voice_params(V)
    return ids, [(ids["osc_a"], S.OSC_VAL, det), (ids["vcf"], S.VCF_FREQ, cut)]


def state(S, p, ids, out, tag):
    out[f"{tag}_osc_pos"] = p.get_voice_field(ids["osc_a"], S.OSC_POS)
    for name in ("F", "P", "Q", "B0", "B1", "B2", "B3", "B4"):
        out[f"{tag}_vcf_{name}"] = p.get_voice_field(ids["vcf"], getattr(S, "VCF_ST_" + name))


def main():
    case, flags, out_path = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    S = srack_pkg.load()
    voices, T, calls = CASES[case]
    patches = []
    for V in voices:
        p = S.Patch(48000, 1024, 2)
        ids, over = p1(p, S, V)
        p.configure_voices(V)
        for m, f, v in over:
            p.set_voice_field(m, f, v)
        patches.append((p, ids, V))
    out, infos = {}, []
    if case == "grid":
        from tests.test_gpu_parity import read_plane
        p, ids, V = patches[0]
        mix = np.empty((2, T), np.float32)
        with S.DeviceScope() as dev:
            d_fr, d_mx = dev.alloc(T * V * 4), dev.alloc(mix.nbytes)
            p.render_raw(T, d_fr, d_mx, flags, None)
            assert S.lib.srack_device_sync(None) == 0
            got, own, scale = read_plane(S, d_fr, T, V, grid_pick(V))
            dev.download(mix, d_mx)
        out.update(p0_fr0=got, p0_own0=own, p0_scale0=scale, p0_mx0=mix)
        infos.append(p.info())
    else:
        for c in range(calls):
            for k, (p, ids, V) in enumerate(patches):   # (two patches: alternately)
                if case == "stats":
                    fr, mx, st = p.render_stats(T, frames=True, mix=True, flags=flags)
                    out[f"p{k}_st{c}"] = st
                else:
                    fr, mx = p.render(T, flags=flags)
                out[f"p{k}_fr{c}"] = fr[0]
                out[f"p{k}_mx{c}"] = mx
                infos.append(p.info())
    for k, (p, ids, V) in enumerate(patches):
        state(S, p, ids, out, f"p{k}")
    out["infos"] = np.array(infos)
    np.savez(out_path, **out)


if __name__ == "__main__":
    main()
