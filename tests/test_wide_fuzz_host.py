"""The wide family without a GPU: conditions on the inputs of tests/test_gpu_wide_fuzz.py, met by the reference alone — the two restatements
agree on it, it is neither all silence nor all NaN, every class of wide value is heard — and the default mode's error bound held on the CPU:
every case through csrc/approx.cpp's analysis and the emulated forms (tests/cpp/forms_emu.c) the way tools/cpu_soak.py runs them."""
import os
import sys

import numpy as np
import pytest

from tests import wide_ref as R
from tests.npgraph import NumpyGraph
from tests.test_approx import CSRC, ROOT, _build

sys.path.insert(0, os.path.join(ROOT, "tools"))


def bits(a):
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).copy()
    a[(a & 0x7fffffff) > 0x7f800000] = 0x7fc00000   # a NaN for a NaN
    return a


# ---- the restatements agree ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,seed", R.CASES)
def test_wide_patches_c_equals_numpy(oracle, family, seed):
    """like test_random_patches_c_equals_numpy: the C oracle and the NumPy twin bit for bit, with voice 3's overrides"""
    B, build, overrides = R.draw(family, seed)
    T = 500 if B < 1024 else 1300
    g = oracle.OraclePatch(48000, B, 2)
    ids = build(g)
    ng = NumpyGraph(48000, B, 2)
    build(ng)
    for m, f, fn in overrides:
        v = float(fn(8)[3])
        g.set_field(ids[m], f, v)
        ng.set_field(ids[m], f, v)
    assert g.plan() == ng.plan()[0]
    with np.errstate(all="ignore"):
        a, b = g.render(T), ng.render(T)
    np.testing.assert_array_equal(bits(a), bits(b))


# ---- not all silence, not all NaN -----------------------------------------------------------------------------------------------------------
def test_the_plain_seeds_are_mostly_finite_audio(oracle):
    audible = [s for s in R.FAMILIES["plain"] if np.isfinite(R.voice0("plain", s)).all() and np.abs(R.voice0("plain", s)).max() > 1e-2]
    blown = [s for s in R.FAMILIES["plain"] if (~np.isfinite(R.voice0("plain", s))).mean() > 0.5]
    assert len(audible) >= 36 and len(blown) <= 6, (audible, blown)


def test_the_special_seeds_hold_non_finite_samples_and_not_only_those(oracle):
    """(over every voice of the device case: a special in one voice of an override is a special)"""
    hold = [s for s in R.FAMILIES["special"] if not np.isfinite(R.reference("special", s)[3]).all()]
    assert len(hold) >= 10 and len(R.FAMILIES["special"]) - len(hold) >= 10, hold


# ---- every class is heard ----------------------------------------------------------------------------------------------------------------------
def heard(kind):
    """the cases where clamping this kind of wide value back into today's range changes voice 0's render by more than 1e-2"""
    return [c for c in R.CASES if kind in R.draw(*c)[1].kinds and R.differs(R.voice0(*c), R.voice0(c[0], c[1], (kind,)))]


@pytest.mark.parametrize("kind", R.KINDS)
def test_every_class_of_wide_value_is_heard(oracle, kind):
    """each row of the table, the negative envelope times alone, the underflowing pitches alone, STEPS_PER_OCTAVE 0 alone (notes/r28.md lists the seeds)"""
    cases = heard(kind)
    assert len(cases) >= 3, (kind, cases)


# ---- the bound, on the CPU ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    srcs = [os.path.join(ROOT, "tests", "cpp", "approx_probe.cpp"), os.path.join(CSRC, "graph.cpp"), os.path.join(CSRC, "approx.cpp"),
            os.path.join(CSRC, "approx.hpp"), os.path.join(CSRC, "graph.hpp"), os.path.join(CSRC, "flatten.hpp"), os.path.join(ROOT, "include", "srack_hip.h")]
    return _build(os.path.join(ROOT, "tests", "cpp", "approx_probe"), srcs, ["-std=c++17", "-Wall"])


# tools/cpu_soak.py --family wide over seeds 0 - 5999 of each sub-family, on the analysis as it was before this family existed: 104 / 102 / 92 / 92
# seeds (plain / noise / NonLinear / special) outside the contract, none on the analysis as it is.  Pinned, beside plain 37 and special 33
# of the lists above: an oscillator whose f32 increment underflows — a NaN where the reference is finite (noise 952, on a patch whose bound
# said 0), a ramp missing altogether (plain 233 and 1253, NonLinear 3664: 1.0; noise 279: 2.0; special 2202: 1.0 in half the samples) —
# and an envelope with a negative time whose ramp overflows behind forms the analysis had granted (noise 1421, NonLinear 4037 and 4821,
# special 2966: these four alone stay red with the envelope's fix taken out again).  They run at the soak's 6 000 samples: two of the four
# ramps need more than 3 000 to overflow.
SOAK_FINDS = [("plain", 233), ("plain", 1253), ("noise", 279), ("noise", 952), ("noise", 1421), ("nonlin", 3664), ("nonlin", 4037), ("nonlin", 4821),
              ("special", 2202), ("special", 2966)]


@pytest.mark.parametrize("family,seed,T", [c + (3000,) for c in R.CASES] + [c + (6000,) for c in SOAK_FINDS])
def test_emulated_forms_stay_inside_the_contract(oracle, probe, family, seed, T):
    """V = 16, T = 3 000 (the soak's finds: 6 000), per-voice overrides passed to the analysis and to both renders; what the analysis grants, rendered by the
    emulation, stays within |emu - ref| <= 1e-5 max(|ref|, 1), non-finite positions and the signs of infinities equal."""
    import cpu_soak
    from tests import forms_emu
    forms_emu.lib()
    B, build, overrides = R.draw(family, seed)
    V = 16
    g = cpu_soak.Both(48000, B, 2)
    ids = build(g)
    ov = [(ids[m], f, fn(V)) for m, f, fn in overrides]
    for m, f, vals in ov:
        g.rec.override(m, f, vals)
    plan = g.rec.run(probe)
    if plan["exact_patch"] or not g.b.apply_plan(g.types, plan, False, per_voice={m for m, _, _ in ov}):
        return   # nothing approximated: the exact modes' business (tests/test_gpu_wide_fuzz.py)
    ref, _ = g.a.render_batch(V, T, ov, threads=1)
    emu, _ = g.b.render_batch(V, T, ov, threads=1)
    why = R.check(emu, ref, bits=False)
    assert why is None, f"{family} {seed}: {why}; bound {plan['bound']:.1e}"


# ---- the voice table, on the host's side ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,seed", R.CASES)
def test_the_voice_table_holds_every_override_before_a_render(family, seed):
    """srack_voices_get_field's "nothing rendered yet" branch: every overridden setting bit for bit at voices 0, 63, 64 and V - 1 — a NaN, an
    infinity, a subnormal and -0.0 included (the device test reads it again where a device holds it)"""
    import srack_pkg
    S = srack_pkg.load()
    B, build, overrides = R.draw(family, seed)
    V, _ = R.sizes(B)
    p = S.Patch(48000, B, 2)
    ids = build(p)
    p.configure_voices(V)
    for m, f, fn in overrides:
        p.set_voice_field(ids[m], f, fn(V))
    for m, f, fn in overrides:
        got, vals = p.get_voice_field(ids[m], f).astype(np.float32), fn(V)
        for v in (0, 63, 64, V - 1):
            assert bits(got[v:v + 1]) == bits(vals[v:v + 1]), (family, seed, m, f, v, got[v], vals[v])


# ---- the checker ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_the_checker_refuses_the_clamped_render(oracle, kind):
    """handed the clamped-to-slider render in place of the wide one it fails, in bit mode and in contract mode"""
    for family, seed in heard(kind)[:3]:
        wide, clamped = R.voice0(family, seed), R.voice0(family, seed, (kind,))
        assert R.check(wide, wide, bits=True) is None and R.check(wide, wide, bits=False) is None
        assert R.check(clamped, wide, bits=True) is not None and R.check(clamped, wide, bits=False) is not None, (kind, family, seed)


def test_the_checker_tells_one_ulp_and_the_sign_of_an_infinity():
    ref = np.array([[0.5, -1.25, np.inf, np.nan, 3e38]], dtype=np.float32)
    ulp = ref.copy()
    ulp[0, 0] = np.nextafter(np.float32(0.5), np.float32(1.0))
    assert R.check(ulp, ref, bits=True) is not None and R.check(ulp, ref, bits=False) is None
    nan = ref.copy()
    nan.view(np.uint32)[0, 3] = 0xffc00000   # a NaN of the other sign is a NaN
    assert R.check(nan, ref, bits=True) is None and R.check(nan, ref, bits=False) is None
    for wrong in (np.float32(-np.inf), np.float32(3e38), np.float32(np.nan)):
        other = ref.copy()
        other[0, 2] = wrong
        assert R.check(other, ref, bits=True) is not None and R.check(other, ref, bits=False) is not None
    moved = ref.copy()
    moved[0, 1] = np.inf
    assert R.check(moved, ref, bits=False) is not None
    far = ref.copy()
    far[0, 1] = np.float32(-1.25 - 2e-5)
    assert R.check(far, ref, bits=False) is not None
