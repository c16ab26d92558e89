"""Differential fuzzing of the whole render path: random patches, GPU (several render modes) against the CPU oracle.

Patches are random graphs over the module types whose GPU arithmetic is bit-exact in exact-oscillator mode (oscillator
saw / square ports, ladder filter, ADSR, VCA, mixer, math, both sequencers, the sample player, and — in a second family of
patches — the noise source), wired at random — cycles included, so the
planner's broken edges become delay rings — with random parameters and random per-voice overrides.  What this is after
is the host side: planning, dead-code elimination, uniform hoisting, control units, wire-slot reuse, rings, tiles.

What a lane READS per voice — a wave per voice for the sample players, a sequence per voice for the sequencers — is a family of its own,
random_banked_patch, with a reference of its own: tests/test_gpu_banked_fuzz.py.  random_patch draws neither, so the seeds here keep
their patches.
"""
import numpy as np
import pytest

import srack_pkg

pytestmark = pytest.mark.gpu

from tests.fuzz_patches import random_patch  # noqa: E402


# seeds past 159: found by tools/fuzz_soak.py — patches whose oscillators take an audio-rate pitch CV inside a feedback loop, where one
# last-bit difference in 2^cv (ocml's pow against the host libm's) used to grow into different samples (780, 867, 944: fixed by
# exp2_cr in round 2), patches that overflow into NaNs (707, 774, 1000, 1157), and the three the default modes' soak found chaotic in
# round 3 (725: a loop through a sync input, 1459: a filter <-> mixer loop with a gain above 1, 1473: a loop through a pitch): 725 and
# 1473 parted from the oracle in exact mode too, at one of the arguments where the libm's pow is not the correctly rounded 2^e — since
# round 4 the exact mode evaluates 2^cv with the libm's own algorithm (modules.hip.h, exp2_libm) and they are bit-identical
@pytest.mark.parametrize("seed,noise", [(s, False) for s in list(range(160)) + [707, 725, 774, 780, 867, 944, 1000, 1157, 1459, 1473, 2691, 4386, 10901, 16340, 28336, 40214, 40913, 66697, 72223]] + [(s, True) for s in list(range(40)) + [2127, 2197, 2203, 2360]])
def test_random_patch_matches_oracle(seed, noise, oracle, monkeypatch):
    S = srack_pkg.load()
    if seed % 2:  # few voices normally run as quarter-filled waves (more waves, same cost); odd seeds force the full,
        monkeypatch.setenv("SRACK_WANT_WAVES", "1")  # 64-lane waves large renders use — with a ragged last wave
    B, build, overrides = random_patch(seed, noise)
    V, T = (67, 1300) if B < 1024 else (131, 2300)  # past the first control chunk (1024) and, at B = 1024, past two ring periods
    o = oracle.OraclePatch(48000, B, 2)
    ids = build(o)
    ov = [(ids[m], f, fn(V)) for m, f, fn in overrides]
    ref, _ = o.render_batch(V, T, ov, threads=8)
    # exact oscillator x {fused, interpreter} x {hoisted (pipelined / one control unit), everything per voice}, then the kernels
    # specialised at run time (32 | 2: hoisted / per voice) for the patches the generator covers (a third of the seeds: each is a compilation)
    for flags in (1, 3, 5, 7, 9, 11) + ((35, 39) if seed % 3 == 0 else ()):
        p = S.Patch(48000, B, 2)
        ids = build(p)
        p.configure_voices(V)
        for m, f, vals in ov:
            p.set_voice_field(m, f, vals)
        assert p.plan() == o.plan()
        if flags & 32:
            try:
                p.kernel_source(flags)
            except S.SrackError as e:
                assert e.code == S.ERR_UNSUPPORTED  # a reverb: the interpreter's (covered above)
                continue
        fr = p.render_channels(T, flags)
        if flags & 32:
            assert "render_specialized" in p.info()
        assert np.isfinite(fr).all() == np.isfinite(ref).all()
        # (a NaN is a NaN: x86's default NaN is 0xffc00000, the GPU's 0x7fc00000 — seeds 707, 774, 1000, 1157 blow up and hold thousands)
        same = (fr.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(fr) & np.isnan(ref))
        # everything in these patches is bit-exact in exact-oscillator mode (tools/fuzz_stats.py: 960 of 960 renders)
        assert same.all(), f"seed {seed} flags {flags}: {1 - same.mean():.5f} of the samples differ; {p.info()}"


@pytest.mark.parametrize("seed", list(range(2000, 2030)))
def test_random_patch_with_waveshapers_matches_oracle(seed, oracle, monkeypatch):
    """The NonLinear family (FUZZ_NONLIN: half the MathModules become sign-preserving waveshapers, exponents 0.3 ... 3 per voice) in the exact modes, bit
    for bit — possible since round 6, when `a.powf(b)` became the host libm's powf operation for operation (modules.hip.h, powf_libm_plain); until then
    the fuzzer's exact-mode family had no waveshaper because the power was an f32 ulp off now and then.  (tools/fuzz_soak.py with FUZZ_NONLIN=1: 2 100
    renders past these seeds, 300 of them through the specialised kernels, 0 not bit-identical.)"""
    monkeypatch.setenv("FUZZ_NONLIN", "1")
    S = srack_pkg.load()
    if seed % 2:
        monkeypatch.setenv("SRACK_WANT_WAVES", "1")
    B, build, overrides = random_patch(seed, False)
    V, T = (67, 1300) if B < 1024 else (131, 2300)
    o = oracle.OraclePatch(48000, B, 2)
    ids = build(o)
    ov = [(ids[m], f, fn(V)) for m, f, fn in overrides]
    ref, _ = o.render_batch(V, T, ov, threads=8)
    for flags in (1, 3, 5) + ((35,) if seed % 3 == 0 else ()):
        p = S.Patch(48000, B, 2)
        build(p)
        p.configure_voices(V)
        for m, f, vals in ov:
            p.set_voice_field(m, f, vals)
        assert p.plan() == o.plan()
        if flags & 32:
            try:
                p.kernel_source(flags)
            except S.SrackError as e:
                assert e.code == S.ERR_UNSUPPORTED
                continue
        fr = p.render_channels(T, flags)
        same = (fr.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(fr) & np.isnan(ref))
        assert same.all(), f"seed {seed} flags {flags}: {1 - same.mean():.5f} of the samples differ; {p.info()}"


# ---- the DEFAULT (approximating) render modes — what bench.py times — over the same patches ----------------------------------------
# Contract: |gpu - ref| <= 1e-5 * max(|ref|, 1) per sample, NaN / inf at the oracle's positions (BASELINE.json north_star; SURVEY 7 gives
# the denominator).  Default arithmetic is 1e-7-accurate, not bit-identical: the f32 PolyBLEP, the fma-contracted ladder, the polynomial
# 2^cv and sine.  A patch that ITERATES such a value — feedback through a pitch or a sync input, a sample-player read index that truncates
# the other way, a ladder at resonance > 0.9 inside a loop — is chaotic: any 1e-7 grows without bound, and no implementation that is
# not bit-identical to the host libm stays within 1e-5 on it (notes/ has the soaks).  The flattener's error bound (csrc/approx.cpp)
# finds those structures as unbounded gains and evaluates what sits behind them exactly — single oscillators as a whole, producers one by
# one, the whole patch where its values have no bound; a patch that still leaves the band would be listed in KNOWN_CHAOTIC as a strict xfail.
DEFAULT_FLAGS = (0, 2, 4)          # fused / general path (interpreter at this size) / everything per voice
DEFAULT_SPECIAL = 34               # the general path through a kernel specialised at run time (a compilation: every third seed)
KNOWN_CHAOTIC = {
    # (seed, noise): reason.  Empty since round 4.  The seeds pinned below are the soaks' finds of rounds 3 - 5 (725, 1459, 1473: cycles
    # through event inputs, amplifying cycles with a filter in them, a loop through a pitch; 2691: a bandpass into a gate; 4386: two mixers
    # amplifying each other; 10901: producers into a cutoff behind a highpass; 16340: a pitch above one cycle per sample; 28336: a square on a
    # cutoff; 40214 / 40913: a ladder in a cycle, an integrator; the noise family's 2127 ... 2360: white noise on a cutoff; 66697: a hard-synced
    # LFO on a cutoff; 72223: a filter's lowpass, fed from a chaotic loop, on a cutoff) — each had a rule of its own in flatten.cpp until round 5 and is now whatever the bound makes of it.
}


def _default_cases():
    cases = []
    for s, noise in [(s, False) for s in list(range(160)) + [707, 725, 774, 780, 867, 944, 1000, 1157, 1459, 1473, 2691, 4386, 10901, 16340, 28336, 40214, 40913, 66697, 72223]] + [(s, True) for s in list(range(40)) + [2127, 2197, 2203, 2360]]:
        why = KNOWN_CHAOTIC.get((s, noise))
        cases.append(pytest.param(s, noise, marks=pytest.mark.xfail(strict=True, reason=why)) if why else pytest.param(s, noise))
    return cases


@pytest.mark.parametrize("seed,noise", _default_cases())
def test_random_patch_default_modes_within_tolerance(seed, noise, oracle, monkeypatch):
    S = srack_pkg.load()
    if seed % 2:
        monkeypatch.setenv("SRACK_WANT_WAVES", "1")
    B, build, overrides = random_patch(seed, noise)
    V, T = (67, 1300) if B < 1024 else (131, 2300)
    o = oracle.OraclePatch(48000, B, 2)
    ids = build(o)
    ov = [(ids[m], f, fn(V)) for m, f, fn in overrides]
    ref, _ = o.render_batch(V, T, ov, threads=8)
    r64 = ref.astype(np.float64)
    bad = []
    for flags in DEFAULT_FLAGS + ((DEFAULT_SPECIAL,) if seed % 3 == 0 or seed == 72223 else ()):   # (72223: found through the specialised kernels)
        p = S.Patch(48000, B, 2)
        build(p)
        p.configure_voices(V)
        for m, f, vals in ov:
            p.set_voice_field(m, f, vals)
        if flags & 32:
            try:
                p.kernel_source(flags)
            except S.SrackError as e:
                assert e.code == S.ERR_UNSUPPORTED  # a reverb: the interpreter's (covered above)
                continue
        fr = p.render_channels(T, flags)
        if flags & 32:
            assert "render_specialized" in p.info()
        masks = (np.isnan(fr) == np.isnan(ref)).all() and (np.isinf(fr) == np.isinf(ref)).all() and (np.sign(fr[np.isinf(fr)]) == np.sign(ref[np.isinf(ref)])).all()
        ok = np.isfinite(r64) & np.isfinite(fr)
        err = np.abs(fr.astype(np.float64)[ok] - r64[ok]) / np.maximum(np.abs(r64[ok]), 1.0)
        e = float(err.max()) if err.size else 0.0
        if e > 1e-5 or not masks:
            bad.append(f"flags {flags}: max rel err {e:.2e}, {float((err > 1e-5).mean()):.5f} of the samples outside, non-finite positions equal: {masks}; {p.info()}")
    assert not bad, f"seed {seed} noise {noise}: " + " | ".join(bad)


@pytest.mark.parametrize("seed,noise,more", [(104123, False, True), (105055, False, True), (123042, True, False)])
def test_soak_finds_at_two_hundred_voices(seed, noise, more, oracle, monkeypatch):
    """Round 5's later soaks, at their 200 voices x 6 000 samples.  With resonances, amounts, envelope times and initial phases as per-voice arrays
    too (FUZZ_MORE_OV): 104123 — an audio-rate SINE on a cutoff whose filter feeds another cutoff (5.2e-4 before the motion classes handed a
    filter's own cutoff's motion on) — and 105055 — a ladder, already literal, behind a mix of magnitude 4 and with an audio-rate saw on its
    cutoff, that turned a 4.8e-7 disturbance of its input into 6.9e-5.  The noise family: 123042 — a ladder behind a reverb, 1.0e-4.  The last two
    are the OVERDRIVEN ladder (tools/ladder_calib.c `amp`: chaotic from an input of ~1.9 up where the cutoff is high): no bound is claimed for
    such a filter, nor for one whose cutoff moves at audio rate — everything in front exact, and all three bit-identical to the oracle."""
    if more:
        monkeypatch.setenv("FUZZ_MORE_OV", "1")
    S = srack_pkg.load()
    B, build, overrides = random_patch(seed, noise)
    V, T = 200, 6000
    o = oracle.OraclePatch(48000, B, 2)
    ids = build(o)
    ov = [(ids[m], f, fn(V)) for m, f, fn in overrides]
    ref, _ = o.render_batch(V, T, ov, threads=8)
    r64 = ref.astype(np.float64)
    assert np.isfinite(r64).all()
    for flags in DEFAULT_FLAGS:
        p = S.Patch(48000, B, 2)
        build(p)
        p.configure_voices(V)
        for m, f, vals in ov:
            p.set_voice_field(m, f, vals)
        fr = p.render_channels(T, flags).astype(np.float64)
        err = float((np.abs(fr - r64) / np.maximum(np.abs(r64), 1.0)).max())
        assert err <= 1e-5, f"seed {seed} flags {flags}: {err:.2e}; {p.info()}"
        assert "approx[bound" in p.info() and "exact osc" in p.info(), p.info()


@pytest.mark.parametrize("seed,noise,env", [(251484, False, ("FUZZ_MORE_OV",)), (277445, True, ("FUZZ_MORE_OV",)), (235484, True, ()), (227662, True, ()), (239367, True, ()),
                                            (226856, True, ()), (405576, False, ("FUZZ_NONLIN",))])
def test_cpu_soak_finds_on_the_gpu(seed, noise, env, oracle, monkeypatch):
    """The patches round 5's CPU soak (tools/cpu_soak.py on tests/cpp/forms_emu.c — an EMULATION of the kernels' forms) found above their own
    derived bound, here through the kernels themselves, at the soak's 200 voices x 6 000 samples and its draw (notes/r05.md R5.8: 251484 a
    literal ladder behind an f32 square; 277445 noise on an envelope's gate, the envelope on a cutoff: 9.98e-6 with every form taken; 235484 /
    227662 / 239367 noise on a contracted ladder's input: 7.0 - 7.7e-6; 226856 / 405576 hard-synced saws — raw jumps at audio rate — into
    contracted ladders, the second from the NonLinear family — a waveshaper inside a loop of unbounded gain, which the emulation rendered with the
    host's powf and the kernels, until round 6, with a power of their own an f32 ulp away now and then: 1.97 on the GPU; since the port of the libm's
    powf, modules.hip.h powf_libm_plain, the same render).  Each is held to the CONTRACT and to its OWN bound as srack_render_info states
    it, plus three f32 ulps (the feed-forward roundings behind a form, which the bound does not count)."""
    for e in env:
        monkeypatch.setenv(e, "1")
    S = srack_pkg.load()
    B, build, overrides = random_patch(seed, noise)
    V, T = 200, 6000
    o = oracle.OraclePatch(48000, B, 2)
    ids = build(o)
    ov = [(ids[m], f, fn(V)) for m, f, fn in overrides]
    ref, _ = o.render_batch(V, T, ov, threads=8)
    r64 = ref.astype(np.float64)
    assert np.isfinite(r64).all() and np.abs(r64).max() > 0.01
    for flags in DEFAULT_FLAGS + (DEFAULT_SPECIAL,):
        p = S.Patch(48000, B, 2)
        build(p)
        p.configure_voices(V)
        for m, f, vals in ov:
            p.set_voice_field(m, f, vals)
        if flags & 32:
            try:
                p.kernel_source(flags)
            except S.SrackError as e:
                assert e.code == S.ERR_UNSUPPORTED
                continue
        fr = p.render_channels(T, flags).astype(np.float64)
        info = p.info()
        err = float((np.abs(fr - r64) / np.maximum(np.abs(r64), 1.0)).max())
        bound = 0.0 if "approx[exact" in info else float(info.split("approx[bound ")[1].split(";")[0].split("]")[0])
        assert err <= 1e-5 and err <= bound * 1.05 + 3.6e-7, f"seed {seed} flags {flags}: {err:.2e} against its bound {bound:.1e}; {info}"


@pytest.mark.parametrize("seed", [30111, 31051, 7, 23])
def test_random_patch_default_modes_over_a_whole_second(seed, oracle):
    """The default contract over 48 000 samples (the other cases render 1 300 - 2 300): what grows with time.  30111: a held pitch CV's
    polynomial increment was a one-way phase drift (now the reference's own increment per held value); 31051: the same through a CV that
    is flagged as sweeping and sits still (a filter rendering silence; now the polynomial of degree 10, 3e-16) — each 4e-5 on the edges
    of an oscillator two pitch inputs downstream after one second."""
    S = srack_pkg.load()
    B, build, overrides = random_patch(seed, False)
    V, T = 16, 48000
    o = oracle.OraclePatch(48000, B, 2)
    ids = build(o)
    ov = [(ids[m], f, fn(V)) for m, f, fn in overrides]
    ref, _ = o.render_batch(V, T, ov, threads=8)
    r64 = ref.astype(np.float64)
    for flags in DEFAULT_FLAGS:
        p = S.Patch(48000, B, 2)
        build(p)
        p.configure_voices(V)
        for m, f, vals in ov:
            p.set_voice_field(m, f, vals)
        fr = p.render_channels(T, flags)
        assert (np.isnan(fr) == np.isnan(ref)).all() and (np.isinf(fr) == np.isinf(ref)).all()
        ok = np.isfinite(r64) & np.isfinite(fr)
        err = np.abs(fr.astype(np.float64)[ok] - r64[ok]) / np.maximum(np.abs(r64[ok]), 1.0)
        assert not err.size or float(err.max()) <= 1e-5, f"seed {seed} flags {flags}: max rel err {float(err.max()):.2e}; {p.info()}"


@pytest.mark.parametrize("seed,noise", [(s, False) for s in range(60)] + [(s, True) for s in range(20)])
def test_random_patch_renders_continue_across_calls(seed, noise):
    """State carries over between calls in every mode, default (approximating) modes included: render(T) equals
    render(a) ++ render(b) ++ render(c) bit for bit, whatever kernels, tiles, chunks and control units the patch got."""
    S = srack_pkg.load()
    B, build, overrides = random_patch(seed, noise)
    rng = np.random.default_rng(1000 + seed)
    V, T = 70, 2600
    cuts = sorted(int(c) for c in rng.choice(np.arange(1, T), size=2, replace=False))
    values = [(m, f, fn(V)) for m, f, fn in overrides]  # drawn once: the generators are stateful
    for flags in (0, 2, 4, 1) + ((34, 39) if seed % 4 == 0 else ()):  # ... and through the specialised kernels (the interpreter renders what they do not cover)
        if flags & 32:
            p = S.Patch(48000, B, 2)
            ids = build(p)
            p.configure_voices(V)
            for m, f, vals in values:
                p.set_voice_field(ids[m], f, vals)
            try:
                p.kernel_source(flags)
            except S.SrackError as e:
                assert e.code == S.ERR_UNSUPPORTED
                continue
        outs = []
        for parts in ([T], [cuts[0], cuts[1] - cuts[0], T - cuts[1]]):
            p = S.Patch(48000, B, 2)
            ids = build(p)
            p.configure_voices(V)
            for m, f, vals in values:
                p.set_voice_field(ids[m], f, vals)
            outs.append(np.concatenate([p.render_channels(n, flags) for n in parts], axis=1))
        same = outs[0].view(np.uint32) == outs[1].view(np.uint32)
        assert same.all(), f"seed {seed} flags {flags} cuts {cuts}: {1 - same.mean():.5f} of the samples differ"
