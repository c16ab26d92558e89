"""The flagship kernel (render_voice_chain_track, csrc/fused.hip.h) at the edges of its launch shape: one-wave workgroups whose priority
falls 2 -> 1 -> 0 over a launch (the waves of a SIMD kept in step), the control block at priority 3 computing the NEXT chunk's track.
Needs a real MI355X (-m gpu).

What the shape could get wrong, and what holds it here against the CPU oracle:
  * a last wave with fewer than its lanes' voices (shadow lanes), waves of 16 or 32 voices at small voice counts, a grid one wave past
    four per SIMD: voice counts 64, 100, 192, 255, 257 and 4 097 x 64 + 5;
  * chunks shorter than a tile or than the ramp's steps, one-chunk and multi-chunk calls, a tick session of 1024-sample calls;
  * the control block's track where it ends after the voice waves: the launch of a call's short last chunk (100 samples) carries the next
    call's first full chunk (a 4096-sample latency chain);
  * exact mode bit for bit (the reference's arithmetic), default mode within the suite's tolerance, the mix against the frames.
"""

import numpy as np
import pytest

import srack_pkg
from tests.test_gpu_parity import read_plane

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def S():
    S = srack_pkg.load()
    assert S.device_count() > 0, "no GPU visible: the render path has no CPU fallback"
    return S


def p1(g, S, V, adsr="finite", lfo_val=-4.0):
    """P1 with the gate LFO at 27.5 Hz (the envelope moves inside every chunk) and the cfg3 draw of detune / cutoff."""
    ids = S.build_p1(g, adsr=adsr, lfo_val=lfo_val)
    det, cut = S.p1_voice_params(V)
    return ids, [(ids["osc_a"], S.OSC_VAL, det), (ids["vcf"], S.VCF_FREQ, cut)]


def gpu_patch(S, V):
    p = S.Patch(48000, 1024, 2)
    ids, over = p1(p, S, V)
    p.configure_voices(V)
    for m, f, v in over:
        p.set_voice_field(m, f, v)
    return p


def check_frames(got, want, exact):
    assert np.isfinite(got).all()
    if exact:
        np.testing.assert_array_equal(np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32))
    else:
        err = np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1.0)
        assert err.max() <= TOL, f"max rel err {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"


def check_mix(mix, frames_sum, frames_abs_sum):
    assert (np.abs(mix.astype(np.float64) - frames_sum) <= 2e-5 * np.maximum(frames_abs_sum, 1.0)).all()


@pytest.mark.parametrize("flags", [0, 1], ids=["default", "exact"])
@pytest.mark.parametrize("T", [3000, 9000], ids=["one-chunk", "multi-chunk"])
@pytest.mark.parametrize("V", [64, 100, 192, 255, 257])
def test_partial_waves_against_the_oracle(S, oracle, V, T, flags):
    p = gpu_patch(S, V)
    fr, mix = p.render(T, flags=flags)
    assert "kernel=render_voice_chain_track" in p.info(), p.info()
    o = oracle.OraclePatch(48000, 1024, 2)
    _, over = p1(o, S, V)
    ref, ref_mix = o.render_batch(V, T, over, mix=True, threads=8)
    assert np.abs(ref[0]).max() > 0.05, "oracle render is silent"
    check_frames(fr[0], ref[0], flags & 1)
    scale = np.abs(ref[0].astype(np.float64)).sum(axis=1)
    assert (np.abs(mix[0] - ref_mix[0]) <= 2e-5 * np.maximum(scale, 1.0)).all()
    check_mix(mix[0], fr[0].astype(np.float64).sum(axis=1), scale)


@pytest.mark.parametrize("flags", [0, 1], ids=["default", "exact"])
def test_control_track_when_the_control_block_ends_last(S, oracle, flags):
    """64 voices (four 16-voice waves), calls of three full chunks and a 100-sample one: the last launch's control block runs a
    4096-sample chain beside 100 samples of voices."""
    V, T = 64, 3 * 4096 + 100
    p = gpu_patch(S, V)
    o = oracle.OraclePatch(48000, 1024, 2)
    _, over = p1(o, S, V)
    ref, _ = o.render_batch(V, 2 * T, over, threads=8)
    for c in range(2):   # the second call continues the tick session: its first chunk's track came from the first call's last launch
        fr, _ = p.render(T, flags=flags)
        check_frames(fr[0], ref[0][c * T:(c + 1) * T], flags & 1)


@pytest.mark.parametrize("flags", [0, 1], ids=["default", "exact"])
@pytest.mark.parametrize("V", [100, 257])
def test_tick_session_of_1024_sample_calls(S, oracle, V, flags):
    n_calls, L = 10, 1024
    p = gpu_patch(S, V)
    got = [p.render(L, flags=flags)[0][0] for _ in range(n_calls)]
    assert "kernel=render_voice_chain_track" in p.info(), p.info()
    o = oracle.OraclePatch(48000, 1024, 2)
    _, over = p1(o, S, V)
    ref, _ = o.render_batch(V, n_calls * L, over, threads=8)
    check_frames(np.concatenate(got, axis=0), ref[0], flags & 1)


@pytest.mark.parametrize("flags", [0, 1], ids=["default", "exact"])
def test_full_grid_and_a_partial_wave(S, oracle, flags):
    """4 097 x 64 + 5 voices: four full waves per SIMD and two more, the second with 5 voices.  Sampled voices (the first and last of
    every region the grid distinguishes) against the oracle; the mix against the f64 sum of all voices' frames."""
    V, T = 4097 * 64 + 5, 4500
    p = gpu_patch(S, V)
    n_planes, _ = p.planes()
    assert n_planes == 1
    mix = np.empty((2, T), np.float32)
    with S.DeviceScope() as dev:
        d_fr, d_mx = dev.alloc(T * V * 4), dev.alloc(mix.nbytes)
        p.render_raw(T, d_fr, d_mx, flags, None)
        assert S.lib.srack_device_sync(None) == 0
        assert "kernel=render_voice_chain_track" in p.info(), p.info()
        pick = np.unique(np.array([0, 1, 63, 64, 255, 256, 4095 * 64 - 1, 4096 * 64 - 1, 4096 * 64, 4097 * 64 - 1, 4097 * 64, V - 2, V - 1]
                                  + list(np.random.default_rng(7).integers(0, V, 19))))
        got, own, scale = read_plane(S, d_fr, T, V, pick)
        dev.download(mix, d_mx)
    o = oracle.OraclePatch(48000, 1024, 2)
    ids = S.build_p1(o, adsr="finite", lfo_val=-4.0)
    det, cut = S.p1_voice_params(V)
    ref, _ = o.render_batch(len(pick), T, [(ids["osc_a"], S.OSC_VAL, det[pick]), (ids["vcf"], S.VCF_FREQ, cut[pick])], threads=8)
    assert np.abs(ref[0]).max() > 0.05
    check_frames(got, ref[0], flags & 1)
    check_mix(mix[0], own, scale)
