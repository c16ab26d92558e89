"""The hand-written chain kernels through every port instantiation.  Needs a real MI355X (-m gpu).

render_voice_chain_track, render_voice_chain (csrc/fused.hip.h) and render_voice_chain_seq (csrc/seq.hip.h) are templates over the output
port of the audio oscillator and of the filter, and the instantiations of one oscillator port are a translation unit of their own
(csrc/chain_saw.hip, chain_square.hip, chain_sine.hip; launch_fused and launch_seq pick by the port the patch is wired with).  The rest of the
suite renders saw / low-pass nearly everywhere: a ladder wired to the wrong port would build and pass it.  Here every port pair renders
against the CPU oracle — P1 (finite ADSR, the cfg3 draw of detune and cutoff) through both chain kernels in default and exact mode, P3
through the sequencer chain — at 65 voices (a full wave and one lane of the next) and 100 samples (three full tiles and a 4-sample tail).

Per case: the kernel's name; the frames against the oracle, bit for bit in exact mode and within the suite's 1e-5 contract in default mode;
a render that is not silent.  Exact mode has two instantiations per port pair (the compile-time frames + mix, and the one that decides at
run time): frames only and mix only must give the bits of frames + mix.

The gate LFO keeps its square port: a saw or sine gate may move an edge of the envelope by a sample in default mode.  The filter's
resonance is 0.3: at build_p1's 0.5 the flattener's error budget (csrc/approx.cpp, 5e-6 per channel) denies the f32 PolyBLEP and the
contracted ladder to saw / band-pass, saw / high-pass and square / band-pass over this draw of cutoffs (bound 5.0e-6 and above), and a
default-mode program with an exact source is the general path's (render_interp) — those instantiations would never run.  At 0.3 all nine
wirings keep the default forms (bounds 1.9e-6 ... 4.9e-6, tests/cpp/approx_probe)."""
import functools
import re

import numpy as np
import pytest

import srack_pkg
from tests.patch_makers import bits
from tests.test_gpu_parity import assert_close

pytestmark = pytest.mark.gpu

EXACT, NO_HOIST = 1, 4
V, T = 65, 100
OSC_PORTS = ["saw", "square", "sine"]
VCF_PORTS = ["lp", "bp", "hp"]


@pytest.fixture(scope="module")
def S():
    S = srack_pkg.load()
    assert S.device_count() > 0, "no GPU visible: the render path has no CPU fallback"
    return S


def osc_port(S, name):
    return {"saw": S.OSC_OUT_SAW, "square": S.OSC_OUT_SQUARE, "sine": S.OSC_OUT_SINE}[name]


def vcf_port(S, name):
    return {"lp": S.VCF_OUT_LOWPASS, "bp": S.VCF_OUT_BANDPASS, "hp": S.VCF_OUT_HIGHPASS}[name]


def p1(S, g, osc, vcf):
    """P1 with the gate LFO at 27.5 Hz, started in its high half, the audio oscillator's `osc` port into the filter and the filter's `vcf` port into the VCA."""
    ids = S.build_p1(g, adsr="finite", lfo_val=-4.0)
    g.set_field(ids["osc_lfo"], S.OSC_POS, 0.75)  # the gate is high from the first sample: the attack fills the 100 samples
    g.set_field(ids["vcf"], S.VCF_RES, 0.3)  # (see the module's docstring: every wiring keeps the default mode's forms)
    g.disconnect(ids["vcf"], 0)
    g.connect(ids["osc_a"], osc_port(S, osc), ids["vcf"], 0)
    g.disconnect(ids["vca"], 0)
    g.connect(ids["vcf"], vcf_port(S, vcf), ids["vca"], 0)
    det, cut = S.p1_voice_params(V)
    return [(ids["osc_a"], S.OSC_VAL, det), (ids["vcf"], S.VCF_FREQ, cut)]


def p3(S, g, osc):
    """bench.py's P3 with the oscillator's `osc` port into the filter."""
    _, build, overrides = S.bench_workload("p3", V)
    ids = build(g)
    g.set_field(ids["clock"], S.OSC_POS, 0.75)  # the first step fires at the first sample
    g.disconnect(ids["vcf"], 0)
    g.connect(ids["osc"], osc_port(S, osc), ids["vcf"], 0)
    return overrides(ids)


@functools.lru_cache(maxsize=None)
def reference(patch, *ports):
    """The oracle's frames of one wiring, rendered once: plane 0, [T][V].  (The oracle has no render modes: one reference per wiring.)"""
    from oracle import oracle as O
    O.build()
    S = srack_pkg.load()
    o = O.OraclePatch(48000, 1024, 2)
    over = (p1 if patch == "p1" else p3)(S, o, *ports)
    ref, _ = o.render_batch(V, T, over, threads=8)
    ref = np.array(ref[0], dtype=np.float32)
    ref.setflags(write=False)
    return ref


def gpu_patch(S, patch, *ports):
    p = S.Patch(48000, 1024, 2)
    over = (p1 if patch == "p1" else p3)(S, p, *ports)
    p.configure_voices(V)
    for m, f, v in over:
        p.set_voice_field(m, f, v)
    return p


def kernel_of(p):
    return re.search(r"kernel=(\w+)", p.info()).group(1)


def check(S, patch, ports, flags, kernel):
    ref = reference(patch, *ports)
    p = gpu_patch(S, patch, *ports)
    fr, mix = p.render(T, flags=flags)
    # (another kernel here means the flattener's error budget, csrc/approx.cpp, no longer leaves this wiring its default forms: the docstring)
    assert kernel_of(p) == kernel, p.info()
    assert fr[0].shape == (T, V)
    print("%s %s flags=%d: max |ref| %.4f, max |gpu - ref| %.3e" % (kernel, "/".join(ports), flags, np.abs(ref).max(), np.abs(fr[0].astype(np.float64) - ref).max()))
    if flags & EXACT:
        np.testing.assert_array_equal(bits(fr[0]), bits(ref))
    else:
        assert_close(fr[0], ref)
    # not silent, no voice of it: the envelope is a fifth of the way up its 480-sample attack (P3: through its 96-sample one), and the oracle's
    # quietest voice of any wiring (saw / high-pass) peaks at 5.8e-3
    assert np.abs(ref).max(axis=0).min() > 1e-3 and np.abs(fr[0]).max(axis=0).min() > 1e-3
    if flags & EXACT:  # frames + mix is the compile-time output mode; frames only and mix only take the instantiation that decides at run time
        q = gpu_patch(S, patch, *ports)
        fr1, none = q.render(T, mix=False, flags=flags)
        assert none is None and kernel_of(q) == kernel, q.info()
        np.testing.assert_array_equal(bits(fr1), bits(fr))
        q = gpu_patch(S, patch, *ports)
        none, mix2 = q.render(T, frames=False, flags=flags)
        assert none is None and kernel_of(q) == kernel, q.info()
        np.testing.assert_array_equal(bits(mix2), bits(mix))


@pytest.mark.parametrize("flags", [0, EXACT], ids=["default", "exact"])
@pytest.mark.parametrize("vcf", VCF_PORTS)
@pytest.mark.parametrize("osc", OSC_PORTS)
def test_voice_chain_track_ports(S, osc, vcf, flags):
    check(S, "p1", (osc, vcf), flags, "render_voice_chain_track")


@pytest.mark.parametrize("flags", [NO_HOIST, NO_HOIST | EXACT], ids=["default", "exact"])
@pytest.mark.parametrize("vcf", VCF_PORTS)
@pytest.mark.parametrize("osc", OSC_PORTS)
def test_voice_chain_ports(S, osc, vcf, flags):
    check(S, "p1", (osc, vcf), flags, "render_voice_chain")


@pytest.mark.parametrize("osc", OSC_PORTS)
def test_voice_chain_seq_ports(S, osc):
    check(S, "p3", (osc,), 0, "render_voice_chain_seq")
