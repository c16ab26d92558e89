"""Differential fuzzing with settings beyond the sliders: random_wide_patch (tests/fuzz_patches.py) on the GPU against the CPU oracle.

Nothing in the library clamps a field — pitches of 0.03 Hz and of 4.7 cycles per sample, increments that underflow an f32, cutoffs and
resonances outside 0 ... 1, negative envelope times, gains of +-12, 0 or 65535 steps per octave, a wave at 3 MHz, and (the special cases)
infinities, NaNs and subnormals among the settings — and three parts of it decide by exactly these values: the flattener's error bound,
the kernels' range-dependent forms, the planner's choice of kernel.  tests/test_wide_fuzz_host.py holds the conditions on the inputs and
the emulated forms; what the kernels themselves do — which kernel a patch gets, hoisting, control units across lanes, the staging of a
wave — only shows here.  Shaped like tests/test_gpu_fuzz.py: the exact modes bit for bit, the default modes within the contract."""
import numpy as np
import pytest

import srack_pkg

pytestmark = pytest.mark.gpu

from tests import wide_ref as R  # noqa: E402

EXACT_FLAGS, EXACT_SPECIAL = (1, 3, 5, 7, 9, 11), (35, 39)   # exact oscillator x {fused, interpreter} x {hoisted, per voice}; specialised at run time
DEFAULT_FLAGS, DEFAULT_SPECIAL = (0, 2, 4), (34,)           # what bench.py times; the specialised kernels on every third seed (each is a compilation)
KNOWN_CHAOTIC = {
    # (family, seed): reason — a strict xfail of the default modes.  An entry needs the CPU evidence that the REFERENCE is chaotic there (the
    # oracle against the oracle with one input moved by an ulp), and none may cover an envelope with a negative time, an increment that
    # underflows or 0 steps per octave: those were wrong bounds (notes/r28.md), not chaos.  Empty.
}


def _cases():
    out = []
    for family, seed in R.CASES:   # a case's two modes side by side: they share one reference
        out.append(pytest.param(family, seed, "exact"))
        why = KNOWN_CHAOTIC.get((family, seed))
        out.append(pytest.param(family, seed, "default", marks=pytest.mark.xfail(strict=True, reason=why)) if why else pytest.param(family, seed, "default"))
    return out


def _same_f32(a, b):
    a, b = np.float32(a), np.float32(b)
    return bool(a.view(np.uint32) == b.view(np.uint32) or (np.isnan(a) and np.isnan(b)))


@pytest.mark.parametrize("family,seed,mode", _cases())
def test_wide_patch_matches_oracle(family, seed, mode, oracle, monkeypatch):
    S = srack_pkg.load()
    if seed % 2:  # odd seeds: the full 64-lane waves large renders use, with a ragged last wave
        monkeypatch.setenv("SRACK_WANT_WAVES", "1")
    B, build, _ = R.draw(family, seed)
    V, T, ov, ref, plan = R.reference(family, seed)
    exact = mode == "exact"
    flag_sets = (EXACT_FLAGS + (EXACT_SPECIAL if seed % 3 == 0 else ())) if exact else (DEFAULT_FLAGS + (DEFAULT_SPECIAL if seed % 3 == 0 else ()))
    bad = []
    for flags in flag_sets:
        p = S.Patch(48000, B, 2)
        build(p)
        p.configure_voices(V)
        for m, f, vals in ov:
            p.set_voice_field(m, f, vals)
        assert p.plan() == plan
        if flags == flag_sets[0]:   # before the first render of the case: the voice table holds every override, an infinity or a NaN included
            for m, f, vals in ov:
                got = p.get_voice_field(m, f)
                for v in (0, 63, 64, V - 1):
                    assert _same_f32(got[v], vals[v]), f"{family} {seed}: module {m} field {f} voice {v}: {got[v]!r}, set {vals[v]!r}"
        if flags & 32:
            try:
                p.kernel_source(flags)
            except S.SrackError as e:
                assert e.code == S.ERR_UNSUPPORTED  # a reverb: the interpreter's (covered by the other flags)
                continue
        fr = p.render_channels(T, flags)
        info = p.info()
        if flags & 32:
            assert "render_specialized" in info
        why = R.check(fr, ref, bits=exact)
        print(f"WIDE {family} {seed} flags {flags}: {'bits' if exact else '%.2e' % R.worst(fr, ref)} {'ok' if why is None else why} | {info}")
        if why is not None:
            bad.append(f"flags {flags}: {why}; {info}")
    assert not bad, f"{family} {seed} ({mode}): " + " | ".join(bad)
