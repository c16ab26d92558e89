"""Warm starts (notes/r27.md): every kernel family starts a render from "the state stored in the patch" — the state fields of every module
and, for the sink of a broken feedback edge, the source port's saved block (srack_patch_set_output_buffer, or a loaded .srk), which goes
into ring rows of the voice table or into FlatProgram::ring_init — and almost every other test starts from zeros, where a wrong ring id, a
wrong row or a dropped block cannot show.  Here random racks (tests/fuzz_patches.py: the plain, the noise and the NonLinear family) and the
named patches of tests/handoff_ref.py are resumed from a starting point the oracle made (tests/warm_ref.py: a warm-up, a harvest of every
field and every port, applied to a fresh patch) and rendered in every mode:

  exact modes     flags 1, 3, 5, 7, 9, 11 (35 and 39 on every third seed): bit for bit the reference's, a NaN equal to a NaN; the plans equal
  default modes   flags 0, 2, 4 (34 on every third seed): |gpu - ref| <= 1e-5 * max(|ref|, 1), non-finite positions and signs equal

on two state routes (the voices diverge from one running rack / a state per voice) and two delivery routes (even seeds: the graph API; odd
seeds: a rack file loaded twice).  Before the first render the voices hold what was loaded (srack_voices_get_field at voices 0, 63, 64,
V - 1).  tests/test_warm_host.py holds the guards: the harvest is complete, a cold start and ignored blocks would show."""
import numpy as np
import pytest

import srack_pkg
from tests import handoff_ref as H
from tests import warm_ref as WR

pytestmark = pytest.mark.gpu

KNOWN_CHAOTIC = {
    # (family, seed, route): reason — a default-mode miss caused by a chaotic structure, as tests/test_gpu_fuzz.py lists them: a strict
    # xfail.  At most 3 may stand here; more means something is wrong.
}
assert len(KNOWN_CHAOTIC) <= 3


@pytest.fixture(scope="module")
def S():
    S = srack_pkg.load()
    assert S.device_count() > 0, "no GPU visible: the render path has no CPU fallback"
    return S


def _params(chaotic=False):
    out = []
    for family, seed in WR.CASES:
        for route in WR.ROUTES:
            why = KNOWN_CHAOTIC.get((family, seed, route)) if chaotic else None
            out.append(pytest.param(family, seed, route, id=f"{family}-{seed}-{route}", marks=[pytest.mark.xfail(strict=True, reason=why)] if why else []))
    return out


def _setup(monkeypatch, family, seed, route):
    if family == "nonlin":
        monkeypatch.setenv("FUZZ_NONLIN", "1")
    if seed % 2:   # few voices normally run as quarter-filled waves; odd seeds force the full 64-lane waves, with a ragged last one
        monkeypatch.setenv("SRACK_WANT_WAVES", "1")
    w = WR.fuzz_case(family, seed, route)
    return w, WR.reference(w)


def _loaded(S, w, seed, flags):
    """-> the patch, or None where the generated kernels do not cover it (a reverb: the interpreter's)"""
    p = WR.make_patch(S, w, via_file=seed % 2 == 1)
    if flags & 32:
        try:
            p.kernel_source(flags)
        except S.SrackError as e:
            assert e.code == S.ERR_UNSUPPORTED
            return None
    return p


def _holds_what_was_loaded(p, w):
    """srack_voices_get_field, "nothing rendered yet: the initial table\""""
    for m, f, vals in WR.loaded_state(w):
        got = p.get_voice_field(m, f)
        for v in WR.FIRST_VOICES + (w.V - 1,):
            assert H.same_bits(np.float64(got[v]), np.float64(vals[v])).all(), f"{w.name}: module {m} field {f} voice {v}: {got[v]!r}, loaded {vals[v]!r}"


@pytest.mark.parametrize("family,seed,route", _params())
def test_a_random_rack_resumes_bit_for_bit_in_the_exact_modes(S, oracle, monkeypatch, family, seed, route):
    w, ref = _setup(monkeypatch, family, seed, route)
    plan = WR.fresh_oracle(w).plan()
    for k, flags in enumerate(WR.EXACT_FLAGS + (WR.EXACT_SPECIAL if seed % 3 == 0 else ())):
        p = _loaded(S, w, seed, flags)
        if p is None:
            continue
        assert p.plan() == plan
        if k == 0:
            _holds_what_was_loaded(p, w)
        fr = p.render_channels(w.T, flags)
        if flags & 32:
            assert "render_specialized" in p.info()
        WR.check(fr, ref, True, f"{w.name} flags {flags}; {p.info()}")


@pytest.mark.parametrize("family,seed,route", _params(chaotic=True))
def test_a_random_rack_resumes_within_the_contract_in_the_default_modes(S, oracle, monkeypatch, family, seed, route):
    w, ref = _setup(monkeypatch, family, seed, route)
    bad, worst = [], 0.0
    for k, flags in enumerate(WR.DEFAULT_FLAGS + (WR.DEFAULT_SPECIAL if seed % 3 == 0 else ())):
        p = _loaded(S, w, seed, flags)
        if p is None:
            continue
        if k == 0:
            _holds_what_was_loaded(p, w)
        fr = p.render_channels(w.T, flags)
        if flags & 32:
            assert "render_specialized" in p.info()
        err, masks = WR.contract_error(fr, ref)
        worst = max(worst, err)
        if err > WR.TOL or not masks:
            bad.append(f"flags {flags}: max rel err {err:.2e}, non-finite positions and signs equal: {masks}; {p.info()}")
    print(f"warm {w.name} | default modes | max rel err {worst:.2e}")
    assert not bad, f"{w.name}: " + " | ".join(bad)


def _check_state(S, p, w, ids, patch, flags):
    """The hand-off checker's rule (tests/test_gpu_handoff.py): behind an exact render every state field of every module is the oracle's bit
    for bit; behind a default-mode render that took no other flattening, the phase of the FM pair's exact-by-default modulator"""
    exact = bool(flags & H.EXACT)
    if not exact and not (patch == "p2" and not flags & H.REFLATTEN):
        return
    for (m, f), per_voice in sorted(WR.final_state(w, H.SAMPLED).items()):
        if not exact and (m, f) != (ids.get("osc_m"), S.OSC_POS):
            continue
        got = p.get_voice_field(m, f)
        for v, want in per_voice.items():
            assert H.same_bits(np.float64(got[v]), np.float64(want)).all(), f"{w.name} flags {flags}: module {m} field {f} voice {v}: {got[v]!r}, the oracle holds {want!r}"


@pytest.mark.parametrize("patch,B,T,flags", WR.NAMED, ids=[f"{p}-B{B}-T{T}-f{f}" for p, B, T, f in WR.NAMED])
def test_a_named_patch_starts_warm_in_its_own_kernel(S, oracle, patch, B, T, flags):
    w, ids = WR.named_case(patch, B, T)
    ref = WR.reference(w)
    p = WR.make_patch(S, w, via_file=False)
    _holds_what_was_loaded(p, w)
    fr = p.render_channels(T, flags)
    name = p.info().split("kernel=")[-1]
    assert name == WR.named_kernel(patch, B, T, flags), p.info()
    err = WR.check(fr, ref, bool(flags & H.EXACT), f"{w.name} flags {flags}; {p.info()}")
    _check_state(S, p, w, ids, patch, flags)
    print(f"warm {w.name} flags {flags} | {name} | max rel err {err:.2e}")
