"""Differential fuzzing with a wave and a sequence per voice: the banked family of random patches (tests/fuzz_patches.py,
random_banked_patch), every render mode against the reference of tests/banked_ref.py.  Needs a real MI355X (-m gpu).

tests/test_gpu_wave_bank.py and tests/test_gpu_sequence_bank.py hold the two features to the oracle on one graph each.  Here the graph is
random: two or three banked players in one patch, players and sequencers sharing one table, banked modules inside delay rings, behind
control units, beside an unassigned sequencer, as dead code, with a constant assignment, with a bank louder and higher than the module's
own data.  tests/test_banked_fuzz_host.py asserts on the reference alone that the seed list reaches all of that."""
import numpy as np
import pytest

import srack_pkg
from tests import banked_ref as R
from tests.test_gpu_voice_stats import assert_stats_equal, ref_stats

pytestmark = pytest.mark.gpu

EXACT_FLAGS = (1, 3, 5, 17)        # exact oscillator x {fused, general path, everything per voice, the interpreter}
EXACT_SPECIAL = (33, 37)           # ... through kernels specialised at run time (a compilation each: every third seed, and R.MIXED_STAGING)
DEFAULT_FLAGS = (0, 2, 4)
DEFAULT_SPECIAL = 34
TOL = 1e-5                         # the project's contract: |gpu - ref| <= 1e-5 max(|ref|, 1) per sample (BASELINE.json north_star)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    """bit for bit; a NaN is a NaN (x86's default NaN is 0xffc00000, the GPU's 0x7fc00000)"""
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def first_difference(fr, ref):
    bad = ~same(fr, ref)
    v = int(np.flatnonzero(bad.any(axis=(0, 1)))[0])
    t = int(np.flatnonzero(bad[:, :, v].any(axis=0))[0])
    c = int(np.flatnonzero(bad[:, t, v])[0])
    return f"first difference: voice {v} sample {t} channel {c}: {fr[c, t, v]!r} against {ref[c, t, v]!r}"


_DRAW, _REF = {}, {}


def drawn(seed):
    if seed not in _DRAW:
        _DRAW[seed] = R.draw(seed)
    return _DRAW[seed]


def reference(oracle, seed):
    """frames [2][T][V] of the seed at the fuzz's sizes: computed once, shared by the tests, never written to"""
    if seed not in _REF:
        B, build, ov, banks, idx = drawn(seed)
        V, T = R.sizes(B)
        _REF[seed] = R.reference(oracle, B, build, ov, banks, idx, V, T)
        _REF[seed].setflags(write=False)
    return _REF[seed]


def gpu_patch(S, B, build, ov, banks, idx, V):
    p = S.Patch(48000, B, 2)
    ids = build(p)
    p.configure_voices(V)
    for m, f, vals in ov:
        p.set_voice_field(ids[m], f, vals)
    R.install(p, ids, build, banks, idx)
    return p, ids


def specialisable(S, p, flags):
    if not flags & 32:
        return True
    try:
        p.kernel_source(flags)
    except S.SrackError as e:
        assert e.code == S.ERR_UNSUPPORTED
        return False
    return True


def check_info(info, facts, flags):
    """waves= / sequences= name the banks of the assigned modules that render, and nothing where none does"""
    if flags & 32:
        assert "render_specialized" in info, info
    for name, n in (("waves", facts["live_waves"]), ("sequences", facts["live_sequences"])):
        assert (" %s=%d[" % (name, n) in info) if n else (" %s=" % name not in info), (name, n, info)


@pytest.mark.parametrize("seed", R.SEEDS)
def test_banked_patch_matches_reference(seed, oracle, monkeypatch):
    S = srack_pkg.load()
    if seed % 2:  # few voices normally run as quarter-filled waves; odd seeds force the full 64-lane waves — with a ragged last wave
        monkeypatch.setenv("SRACK_WANT_WAVES", "1")
    B, build, ov, banks, idx = drawn(seed)
    V, T = R.sizes(B)
    ref = reference(oracle, seed)
    facts = R.graph_facts(build, ov, banks, idx)
    o = oracle.OraclePatch(48000, B, 2)
    build(o)
    for flags in EXACT_FLAGS + (EXACT_SPECIAL if seed % 3 == 0 or seed in R.MIXED_STAGING else ()):
        p, ids = gpu_patch(S, B, build, ov, banks, idx, V)
        assert p.plan() == o.plan()
        if not specialisable(S, p, flags):
            continue
        fr = p.render_channels(T, flags)
        info = p.info()
        check_info(info, facts, flags)
        ok = same(fr, ref)
        assert ok.all(), f"seed {seed} flags {flags}: {1 - ok.mean():.5f} of the samples differ; {first_difference(fr, ref)}; {info}"


def contract(fr, ref):
    """-> (max error relative to max(|ref|, 1), share of the samples outside, non-finite positions and signs equal)"""
    r64 = ref.astype(np.float64)
    masks = bool((np.isnan(fr) == np.isnan(ref)).all() and (np.isinf(fr) == np.isinf(ref)).all() and (np.sign(fr[np.isinf(fr)]) == np.sign(ref[np.isinf(ref)])).all())
    ok = np.isfinite(r64) & np.isfinite(fr)
    err = np.abs(fr.astype(np.float64)[ok] - r64[ok]) / np.maximum(np.abs(r64[ok]), 1.0)
    return (float(err.max()) if err.size else 0.0), (float((err > TOL).mean()) if err.size else 0.0), masks


@pytest.mark.parametrize("seed", R.SEEDS)
def test_banked_patch_default_modes_within_tolerance(seed, oracle, monkeypatch):
    """the approximating modes: the contract per sample, and bit equality where the flattener's bound (csrc/approx.cpp) — which has to
    look at the loudest sample and the highest note of the whole bank — sends the patch to the exact arithmetic"""
    S = srack_pkg.load()
    if seed % 2:
        monkeypatch.setenv("SRACK_WANT_WAVES", "1")
    B, build, ov, banks, idx = drawn(seed)
    V, T = R.sizes(B)
    ref = reference(oracle, seed)
    facts = R.graph_facts(build, ov, banks, idx)
    bad = []
    for flags in DEFAULT_FLAGS + ((DEFAULT_SPECIAL,) if seed % 3 == 0 or seed in R.MIXED_STAGING else ()):
        p, ids = gpu_patch(S, B, build, ov, banks, idx, V)
        if not specialisable(S, p, flags):
            continue
        fr = p.render_channels(T, flags)
        info = p.info()
        check_info(info, facts, flags)
        e, outside, masks = contract(fr, ref)
        print(f"seed {seed} flags {flags}: max rel err {e:.2e}; {info}")
        if "approx[exact:" in info:
            if not same(fr, ref).all():
                bad.append(f"flags {flags}: exact by its own word, {1 - same(fr, ref).mean():.5f} of the samples differ; {first_difference(fr, ref)}; {info}")
        elif e > TOL or not masks:
            bad.append(f"flags {flags}: max rel err {e:.2e}, {outside:.5f} of the samples outside, non-finite positions equal: {masks}; {info}")
    assert not bad, f"seed {seed}: " + " | ".join(bad)


@pytest.mark.parametrize("seed", R.SEEDS[::3])
def test_banked_patch_renders_continue_across_calls(seed):
    """render(T) equals render(a) ++ render(b) ++ render(c) bit for bit in every mode, the approximating ones included"""
    S = srack_pkg.load()
    V, T = 70, 2600
    B, build, ov, banks, idx = R.draw(seed, V)
    rng = np.random.default_rng(1000 + seed)
    cuts = sorted(int(c) for c in rng.choice(np.arange(1, T), size=2, replace=False))
    for flags in (0, 2, 4, 1) + ((34,) if seed % 4 == 0 else ()):
        if not specialisable(S, gpu_patch(S, B, build, ov, banks, idx, V)[0], flags):
            continue
        outs = []
        for parts in ([T], [cuts[0], cuts[1] - cuts[0], T - cuts[1]]):
            p, ids = gpu_patch(S, B, build, ov, banks, idx, V)
            outs.append(np.concatenate([p.render_channels(n, flags) for n in parts], axis=1))
        ok = bits(outs[0]) == bits(outs[1])
        assert ok.all(), f"seed {seed} flags {flags} cuts {cuts}: {1 - ok.mean():.5f} of the samples differ"


@pytest.mark.parametrize("seed", R.EDIT_SEEDS)
def test_a_new_assignment_under_keep_state(seed, oracle):
    """render, give one assigned module a fresh assignment, render: a wave load for every voice of a player (pos = 0, playing = false),
    an edit of cells for a sequencer (step, detectors and held CV go on; a step past the new length wraps on the next sample) — and
    every other module, banked ones included, runs on.  The cut is a whole number of ticks of the oracle."""
    S = srack_pkg.load()
    B, build, ov, banks, idx = R.draw(seed)
    V = R.sizes(B)[0]
    T1, T2 = (B * max(1, 600 // B), B * max(1, 700 // B)) if B < 1024 else (1024, 2048)
    m = R.edit_module(seed)
    idx2 = R.random_banked_patch(seed)[4][m](V, 1)
    assert (idx2 != idx[m]).any()
    ref, ref_state = R.reference_edits(oracle, B, build, ov, banks, [(idx, T1), ({m: idx2}, T2)], V)
    for flags in (1, 3) + ((33,) if R.EDIT_SEEDS.index(seed) % 3 == 0 else ()):
        p, ids = gpu_patch(S, B, build, ov, banks, idx, V)
        if not specialisable(S, p, flags):
            continue
        p.keep_state(True)
        first = p.render_channels(T1, flags)
        (p.set_voice_waves if build.types[m] == R.SMP else p.set_voice_sequences)(ids[m], idx2)
        second = p.render_channels(T2, flags)
        fr = np.concatenate([first, second], axis=1)
        ok = same(fr, ref)
        assert ok.all(), f"seed {seed} flags {flags} module {m}: {1 - ok.mean():.5f} of the samples differ; {first_difference(fr, ref)}; {p.info()}"
        for b in banks:
            state = np.stack([p.get_voice_field(ids[b["m"]], f) for f in R.state_fields(b)])
            np.testing.assert_array_equal(state, ref_state[b["m"]], err_msg=f"seed {seed} flags {flags}: state of module {b['m']} {R.STATE[b['type']]}")
        for mm, a in {**idx, m: idx2}.items():
            got = (p.get_voice_waves if build.types[mm] == R.SMP else p.get_voice_sequences)(ids[mm])
            assert (got == a).all(), (seed, mm)


@pytest.mark.parametrize("seed", R.WIDE_SEEDS)
def test_wide_render(seed, oracle):
    """4 160 voices (65 waves of lanes), flags 0 but for the exact oscillator: the dispatcher makes its own choice of kernel.  The
    reference renders the voices of each tuple of items as one batch."""
    S = srack_pkg.load()
    V, T = 4160, 96
    B, build, ov, banks, idx = R.draw(seed, V)
    ref = R.reference(oracle, B, build, ov, banks, idx, V, T)
    p, ids = gpu_patch(S, B, build, ov, banks, idx, V)
    fr = p.render_channels(T, 1)
    info = p.info()
    print(f"seed {seed}: {info}")
    check_info(info, R.graph_facts(build, ov, banks, idx), 0)
    assert np.abs(ref).max() > 0.01
    ok = same(fr, ref)
    assert ok.all(), f"seed {seed}: {1 - ok.mean():.5f} of the samples differ; {first_difference(fr, ref)}; {info}"


@pytest.mark.parametrize("seed", R.SEEDS[::8])
def test_statistics_of_a_banked_patch(seed, oracle):
    """srack_render_stats in exact mode: the sequential f64 loop over the reference's frames, bit for bit"""
    S = srack_pkg.load()
    B, build, ov, banks, idx = drawn(seed)
    V, T = R.sizes(B)
    ref = reference(oracle, seed)
    p, ids = gpu_patch(S, B, build, ov, banks, idx, V)
    n_planes, cp = p.planes()
    assert n_planes > 0
    _, _, st = p.render_stats(T, flags=1)
    planes = np.stack([ref[cp.index(k)] for k in range(n_planes)])
    assert_stats_equal(st, ref_stats(planes))
