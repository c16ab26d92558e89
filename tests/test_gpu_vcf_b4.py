"""The flagship's vote on the ladder's clamp behind the cubic (render_voice_chain_track, csrc/fused.hip.h; vcf_b4_bounded, csrc/modules.hip.h;
notes/r30.md): a default-mode wave whose every lane passes the bound runs its tiles without `s.b4 = clamp1(s.b4)`, which is meant to change
no bit.  Needs a real MI355X (-m gpu).

tests/vcf_b4_driver.py renders every case in two processes, one after the other, SRACK_VCF_B4=1 (the default) and SRACK_VCF_B4=0 (the vote
fails everywhere), and the two .npz files must agree bit for bit: frames and mix as uint32, the statistics, the voice state read back.  The
renders are also held to the CPU oracle — exact mode bit for bit, default mode at the suite's 1e-5 — so that "both wrong alike" does not
pass.  Voices 2, 63, 64, 65, 200; calls of 1, 31, 32, 33, 95 and 4 103 samples, then 7, 243, 1 024 and 33, continuing; frames + mix,
frames, mix in turn, and the statistics variant; default and exact mode.  The warm starts also with a first call of 4 103 samples: after a
first call of one sample — the short tile's loop, which keeps every clamp — the state the case is about is gone.

    a          cfg3's draw, cutoffs U(0.05, 0.6): every wave votes yes
    b          cutoffs 0.88, 0.894, 0.897, 0.9 with resonance 0 and 1 inside every wave: the wave votes no.  (Resonance 1 at these cutoffs is
               beyond the flattener's error budget, so default mode renders it from the exact sources through render_interp — the
               flagship's default-mode code never meets such a lane, under no flag; its exact mode does.)
    b_half     the same with resonance 0 and 0.5: within the budget, the flagship in default mode
    c90        a warm start: one voice per wave of (a) at cutoff 0.9 with b0 ... b3 = 1, b4 = -1, phase 0.99 — the oracle's fifth clamp acts
               on the first sample (the cubic leaves at about -1.1)
    c89        the same at cutoff 0.89 and resonance 0, whose coefficients alone pass (2p + |f| 0.95 = 2.826 <= 2.83: the same voice with a
               zero state votes yes) and whose state does not (|b4| = 1: 2.873): the vote has to look at the state.  At the patch's
               resonance of 0.5 the coefficients fail by themselves (3.27), as they do in c90 and c89_soft
    c89_soft   cutoff 0.89 with b4 = -0.95: 2p + |f| 0.95 <= 2.83, the bound of the fourth stage taken alone, PASSES this voice, and the clamp
               acts all the same — the stage sees the step's own b3 unclamped and the resonance feedback with it

The guards come from the oracle's ladder alone (P1 without the VCA: the low-pass port IS b4 behind its clamp, which has acted exactly where
it reads +-1.0) and from the vote's formula in numpy, before any GPU result is read.

Against a library from before the change SRACK_VCF_B4 is an unknown variable that nothing reads: the two processes then run the same code,
and the comparison passes trivially.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import srack_pkg
from tests.test_gpu_flagship_shapes import check_frames, check_mix

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vcf_b4_driver as D  # noqa: E402

TOTAL = sum(D.CALLS)
CASE_FLAGS = [(case, flags) for case, fl in D.CASES.items() for flags in fl]
PRE_MAX, BOUND = 2.83, 0.95   # modules.hip.h: kVcfB4PreMax, kVcfB4Bound


@pytest.fixture(scope="module")
def S():
    S = srack_pkg.load()
    assert S.device_count() > 0, "no GPU visible: the render path has no CPU fallback"
    return S


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


@functools.lru_cache(maxsize=None)
def rendered(knob, tmp):
    """Every case's renders from a child process with SRACK_VCF_B4=knob (once per module)"""
    out = os.path.join(tmp, f"b4_{knob}.npz")
    env = dict(os.environ, SRACK_VCF_B4=str(knob))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "vcf_b4_driver.py"), out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(out)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("vcf_b4"))


@functools.lru_cache(maxsize=None)
def reference(case, V):
    """The oracle's frames [T][V] of the case's patch (computed once, never written to)"""
    from oracle import oracle as O
    S = srack_pkg.load()
    o = O.OraclePatch(48000, 1024, 2)
    ids = D.build(o, S)
    ref, _ = o.render_batch(V, TOTAL, D.overrides(S, ids, case, V), threads=8)
    ref[0].setflags(write=False)
    return ref[0]


@functools.lru_cache(maxsize=None)
def lowpass(case, V):
    """The oracle's ladder alone: the case's oscillator and filter with the low-pass port on the output — b4 behind its clamp, [T][V]"""
    from oracle import oracle as O
    S = srack_pkg.load()
    o = O.OraclePatch(48000, 1024, 2)
    osc, vcf, out = o.add_module(S.MOD_OSCILLATOR), o.add_module(S.MOD_MOOG_FILTER), o.add_module(S.MOD_OUTPUT)
    o.set_field(osc, S.OSC_VAL, 0.0)
    o.set_field(vcf, S.VCF_FREQ, 0.2)
    o.set_field(vcf, S.VCF_RES, 0.5)
    o.set_field(vcf, S.VCF_EXP_AMT, 0.5)
    o.connect(osc, S.OSC_OUT_SAW, vcf, 0)
    o.connect(vcf, S.VCF_OUT_LOWPASS, out, 0)
    o.connect(vcf, S.VCF_OUT_LOWPASS, out, 1)
    ids = dict(osc_a=osc, vcf=vcf)
    lp, _ = o.render_batch(V, TOTAL, D.overrides(S, ids, case, V), threads=8)
    return lp[0]


def vote(S, case, V):
    """vcf_b4_bounded_lane for every voice of the case at its first launch, in f64 from the f32 parameters (no voice of these cases
    sits within an f32 rounding of the threshold: 0.892 at resonance 0)"""
    par = {(k, fld): np.asarray(vals, np.float64) for k, fld, vals in D.params(S, case, V)}
    cut = par[("vcf", S.VCF_FREQ)]
    res = par.get(("vcf", S.VCF_RES), np.full(V, 0.5))
    b = [par.get(("vcf", getattr(S, f"VCF_ST_B{i}")), np.zeros(V)) for i in range(5)]
    q0 = 1.0 - cut
    p = cut + 0.8 * cut * q0
    f = 2.0 * p - 1.0
    q = res * (1.0 + 0.5 * q0 * (1.0 - q0 + 5.6 * q0 * q0))
    m = np.maximum(np.abs(b[4]), BOUND)
    pre = p ** 4 * 2.0 + (p ** 3 + p ** 2 + p) * np.abs(1.0 - f) + (np.abs(f) + p ** 4 * np.abs(q)) * m
    stage_only = 2.0 * p + np.abs(f) * m
    cold = p ** 4 * 2.0 + (p ** 3 + p ** 2 + p) * np.abs(1.0 - f) + (np.abs(f) + p ** 4 * np.abs(q)) * BOUND   # the same voice, zero state
    return (pre <= PRE_MAX) & np.all([np.abs(x) <= 1.0 for x in b], axis=0), stage_only <= PRE_MAX, cold <= PRE_MAX


@pytest.mark.parametrize("case", sorted(D.CASES))
def test_the_cases_are_what_they_say(oracle, S, case):
    """What the cases below rest on, from the oracle's ladder and the vote's formula alone (no GPU work, but of no use without the cases)."""
    for V in D.VOICES:
        lp = lowpass(case, V)
        acted = np.abs(lp) == 1.0   # the clamp has acted exactly where b4 reads +-1.0
        yes, stage_only, cold = vote(S, case, V)
        hot = D.hot_voices(V)
        print(case, V, "max |b4|", float(np.abs(lp).max()), "samples at the clamp", int(acted.sum()), "voices voting yes", int(yes.sum()), "of", V)
        if case == "a":
            assert not acted.any() and np.abs(lp).max() <= BOUND and np.abs(lp).max() > 0.3
            assert yes.all()
        elif case in ("b", "b_half"):
            assert yes.any() and not yes.all()
            for w in range(0, V, 64):   # both sides inside every wave of eight voices or more (65 voices: the second wave is one voice, which votes yes)
                if len(yes[w:w + 64]) >= 8:
                    assert yes[w:w + 64].any() and not yes[w:w + 64].all()
        else:
            assert acted[0, hot].all(), lp[0, hot]
            assert not yes[hot].any() and yes[np.setdiff1d(np.arange(V), hot)].all()
            assert stage_only[hot].all() == (case == "c89_soft")   # ... which the fourth stage's own bound would have let through
            # c89 alone: the warm voice's coefficients pass, so it is its state that makes the vote fail (a vote on f, p, q alone says yes)
            assert cold[hot].all() == (case == "c89") and (cold[hot].any() == cold[hot].all())


def check_against_oracle(got_fr, got_mx, ref, exact):
    scale = np.abs(ref.astype(np.float64)).sum(axis=1)
    if got_fr is not None:
        assert got_fr.shape == ref.shape
        check_frames(got_fr, ref, exact)
    if got_mx is not None:
        for ch in range(got_mx.shape[0]):
            check_mix(got_mx[ch], ref.astype(np.float64).sum(axis=1), scale)
            if got_fr is not None:
                check_mix(got_mx[ch], got_fr.astype(np.float64).sum(axis=1), scale)


@pytest.mark.parametrize("case,flags", CASE_FLAGS, ids=[f"{c}-{('default', 'exact')[f]}" for c, f in CASE_FLAGS])
def test_no_clamp_changes_no_bit(S, oracle, tmp, case, flags):
    # the guards first, from the oracle alone
    for V in D.VOICES:
        lp = lowpass(case, V)
        if case == "a":
            assert not (np.abs(lp) == 1.0).any()
        elif case in D.WARM:
            assert (np.abs(lp[0, D.hot_voices(V)]) == 1.0).all()
        else:
            yes = vote(S, case, V)[0]
            assert yes.any() and not yes.all()
    on, off = rendered(1, tmp), rendered(0, tmp)
    assert sorted(on.files) == sorted(off.files)
    mine = [k for k in on.files if k.startswith(f"{case}_x{flags}_")]
    n_state = 9 * (len(D.VOICES) * (2 if case in D.WARM else 1) + len(D.STATS_VOICES))
    assert len([k for k in mine if "_osc_pos" in k or "_vcf_" in k]) == n_state
    for k in mine:
        if not k.endswith("_infos"):
            np.testing.assert_array_equal(bits(on[k]), bits(off[k]), err_msg=k)
    # resonance 1 in default mode: the exact sources through the general path (csrc/approx.cpp); everything else is the flagship's
    # (two voices of case b are both of resonance 0)
    def want(k):
        general = (case, flags) == ("b", 0) and int(k.split("_")[-2][1:]) > 4
        return "kernel=render_interp" if general else "kernel=render_voice_chain_track"
    for d, v in ((on, 1), (off, 0)):
        for k in mine:
            if k.endswith("_infos"):
                assert len(d[k]) in (len(D.CALLS), len(D.STATS_CALLS), len(D.LONG_CALLS)) and all(str(i).endswith(want(k)) for i in d[k]), (k, d[k])
                assert all(f"SRACK_VCF_B4={v}" in str(i) for i in d[k])   # each child did carry the knob it was given
    for j, V in enumerate(D.VOICES):
        ref, at = reference(case, V), 0
        assert np.abs(ref).max() > 0.05, "oracle render is silent"
        for c, n in enumerate(D.CALLS):
            what = D.mode_of(j, c)
            fr = on[f"{case}_x{flags}_v{V}_c{c}_fr"] if "f" in what else None
            mx = on[f"{case}_x{flags}_v{V}_c{c}_mx"] if "m" in what else None
            assert (f"{case}_x{flags}_v{V}_c{c}_fr" in on.files) == ("f" in what) and (f"{case}_x{flags}_v{V}_c{c}_mx" in on.files) == ("m" in what)
            check_against_oracle(fr, mx, ref[at:at + n], flags & 1)
            at += n
        assert np.unique(on[f"{case}_x{flags}_v{V}_osc_pos"]).size > V // 2 and np.abs(on[f"{case}_x{flags}_v{V}_vcf_B0"]).max() > 0, "the voices did not run"
    for V in D.VOICES if case in D.WARM else ():   # the warm start met by full tiles
        ref, at = reference(case, V), 0
        for c, n in enumerate(D.LONG_CALLS):
            check_against_oracle(on[f"{case}_x{flags}_l{V}_c{c}_fr"], on[f"{case}_x{flags}_l{V}_c{c}_mx"], ref[at:at + n], flags & 1)
            at += n
    for V in D.STATS_VOICES:
        ref, at = reference(case, V), 0
        for c, n in enumerate(D.STATS_CALLS):
            fr, st = on[f"{case}_x{flags}_s{V}_c{c}_fr"], on[f"{case}_x{flags}_s{V}_c{c}_st"]
            check_against_oracle(fr, on[f"{case}_x{flags}_s{V}_c{c}_mx"], ref[at:at + n], flags & 1)
            assert st.shape == (1, S.STAT_COUNT, V)
            np.testing.assert_array_equal(st[0, S.STAT_PEAK_POS], np.maximum(fr.max(axis=0), 0.0).astype(np.float64))
            at += n
