"""A wave per voice for the sample player (srack_patch_set_wave_bank / srack_voices_set_waves) against the CPU oracle, through the C ABI.
Needs a real MI355X (-m gpu).

The contract: voice v renders what a ONE-voice patch renders after srack_patch_set_wave(bank wave wave[v], its rate).  The oracle knows no
bank: it renders one voice at a time, each after a set_wave of its own.  The reference is computed once per bank and shared.

The patch is P4's shape: CLOCK (square, a per-voice pitch: every voice retriggers at its own samples) -> player gate; LFO (sine) through
a Multiply by 1.5 -> player CV (steps of 2^+-1.5 times the rate ratio: below and above one sample); player -> NonLinear -> channel 0,
player -> channel 1.  buffer_size 100, so that every render length here is whole ticks of the oracle.
"""
import numpy as np
import pytest

import srack_pkg

pytestmark = pytest.mark.gpu
TOL = 1e-5
B = 100
V, T1, T2 = 70, 300, 400            # one full and one ragged wave of lanes; 700 samples: a ragged last tile, rendered in two calls
OWN_LEN, OWN_RATE = 60, 32000.0
RATES = (8000.0, 44100.0, 48000.0)
LENGTHS = {"staged": [0, 1, 3, 255, 256, 257, 1200],                    # own + bank = 2032 frames <= 2048: one copy in LDS
           "global": [0, 1, 3, 255, 256, 257, 1200, 2049, 5000]}        # > 2048: gathered through the global pointer
OVERRIDE_OWN, OVERRIDE_BANKED = 22050.0, 12345.0


@pytest.fixture(scope="module")
def S():
    S = srack_pkg.load()
    assert S.device_count() > 0, "no GPU visible: the render path has no CPU fallback"
    return S


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def own_wave():
    return np.random.default_rng(11).uniform(-1, 1, OWN_LEN).astype(np.float32)


def bank(kind):
    rng = np.random.default_rng(len(LENGTHS[kind]))
    return [rng.uniform(-1, 1, n).astype(np.float32) for n in LENGTHS[kind]], [RATES[k % 3] for k in range(len(LENGTHS[kind]))]


def assignment(n_waves, n_voices, shift=0):
    """SRACK_WAVE_OWN and every wave in turn; each further wave of 64 lanes starts five cases on, so that the ragged last wave of lanes
    (six voices at 70) holds the own wave, the empty wave and the longest ones too."""
    v = np.arange(n_voices)
    return ((v + 5 * (v // 64) + shift) % (n_waves + 1) - 1).astype(np.intc)


def clock_vals(n_voices):
    return np.linspace(-1.5, 1.0, n_voices).astype(np.float32)   # 155 ... 880 Hz: a retrigger every 54 ... 310 samples


def build(g, S):
    ids = S.build_p4(g, wave=own_wave(), wave_rate=OWN_RATE, clock_val=-1.0)
    g.set_field(ids["lfo"], S.OSC_VAL, -1.0)          # 220 Hz: three cycles of vibrato in 700 samples
    g.set_field(ids["depth"], S.MATH_CONSTANT, 1.5)
    return ids


def rate_overrides(S, idx):
    """a per-voice wave_sample_rate: one on a voice that plays the own wave, one on a banked voice (which must be ignored)"""
    own_v, banked_v = int(np.flatnonzero(idx == S.WAVE_OWN)[1]), int(np.flatnonzero(idx == 3)[0])
    r = np.full(len(idx), OWN_RATE, dtype=np.float32)
    r[own_v], r[banked_v] = OVERRIDE_OWN, OVERRIDE_BANKED
    return r, own_v


def oracle_voice(S, oracle, v, clock, segments):
    """one voice: segments = [(wave index or WAVE_OWN, waves, rates, own rate, samples)]: set_wave, then render, per segment"""
    o = oracle.OraclePatch(48000, B, 2)
    ids = build(o, S)
    o.set_field(ids["clock"], S.OSC_VAL, clock)
    out = []
    for w, waves, rates, own_rate, n in segments:
        if w >= 0:
            o.set_wave(ids["smp"], waves[w], rates[w])
        else:
            o.set_wave(ids["smp"], own_wave(), own_rate)
        out.append(o.render(n))
    return np.concatenate(out, axis=1), o.get_field(ids["smp"], S.SAMPLE_POS), o.get_field(ids["smp"], S.SAMPLE_PLAYING)


_REF = {}


def reference(S, oracle, kind):
    """[2][T1 + T2][V] frames, pos [V], playing [V]: computed once per bank, never written to"""
    if kind not in _REF:
        waves, rates = bank(kind)
        idx = assignment(len(waves), V)
        own_rate, own_v = rate_overrides(S, idx)
        clock = clock_vals(V)
        fr, pos, playing = np.empty((2, T1 + T2, V), dtype=np.float32), np.empty(V), np.empty(V)
        for v in range(V):
            fr[:, :, v], pos[v], playing[v] = oracle_voice(S, oracle, v, clock[v], [(idx[v], waves, rates, own_rate[v], T1 + T2)])
        for a in (fr, pos, playing):
            a.setflags(write=False)
        _REF[kind] = (fr, pos, playing)
    return _REF[kind]


def gpu_patch(S, kind, n_voices=V, assign=True, with_bank=True):
    waves, rates = bank(kind)
    idx = assignment(len(waves), n_voices)
    p = S.Patch(48000, B, 2)
    ids = build(p, S)
    p.configure_voices(n_voices)
    p.set_voice_field(ids["clock"], S.OSC_VAL, clock_vals(n_voices))
    if n_voices == V:
        p.set_voice_field(ids["smp"], S.SAMPLE_WAVE_SAMPLE_RATE, rate_overrides(S, idx)[0])
    if with_bank:
        p.set_wave_bank(ids["smp"], waves, rates)
    if assign:
        p.set_voice_waves(ids["smp"], idx)
    return p, ids, idx


def test_the_assignment_covers_every_case_in_every_wave_of_lanes(S):
    for kind in LENGTHS:
        idx = assignment(len(LENGTHS[kind]), V)
        assert set(idx[:64].tolist()) == set(range(-1, len(LENGTHS[kind])))
        tail = set(idx[64:].tolist())
        assert S.WAVE_OWN in tail and 0 in tail and max(tail) >= 6   # the own wave, the empty wave, a long one


@pytest.mark.parametrize("exact", [pytest.param(1, id="exact"), pytest.param(0, id="default")])
@pytest.mark.parametrize("flags", [pytest.param(16, id="interpreter"), pytest.param(32, id="specialised"), pytest.param(0, id="dispatcher")])
@pytest.mark.parametrize("kind", ["staged", "global"])
def test_every_voice_plays_its_own_wave(S, oracle, kind, flags, exact):
    ref, ref_pos, ref_playing = reference(S, oracle, kind)
    p, ids, idx = gpu_patch(S, kind)
    assert p.planes() == (2, [0, 1])
    parts = [p.render(n, mix=False, flags=flags | exact)[0] for n in (T1, T2)]   # two calls: the second continues the first
    fr = np.concatenate(parts, axis=1)
    info = p.info()
    n_waves = len(LENGTHS[kind])
    if flags == 32:
        assert info.endswith("kernel=render_specialized") and "waves=%d[%s]" % (n_waves, "lds" if kind == "staged" else "global") in info, info
    else:
        assert info.endswith("kernel=render_interp") and "waves=%d[global]" % n_waves in info, info
    pos, playing = p.get_voice_field(ids["smp"], S.SAMPLE_POS), p.get_voice_field(ids["smp"], S.SAMPLE_PLAYING)
    raw_same = (bits(fr[1]) == bits(ref[1])).mean()
    err = np.abs(fr.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1.0)
    print(f"{kind} flags {flags | exact}: raw plane equal bits {raw_same:.6f}, max rel err {err.max():.3e}, pos equal {(pos == ref_pos).mean():.4f}; {info}")
    assert np.abs(ref[1]).max() > 0.3 and len(np.unique(ref_pos)) > 10 and 0 < ref_playing.sum() < V   # the reference is not trivial
    if exact or "approx[exact:" in info:
        np.testing.assert_array_equal(bits(fr[1]), bits(ref[1]))   # the raw player: wave values
        np.testing.assert_array_equal(bits(fr[0]), bits(ref[0]))   # through the waveshaper
        np.testing.assert_array_equal(pos, ref_pos)
        np.testing.assert_array_equal(playing, ref_playing)
    else:
        assert np.isfinite(fr).all() and err.max() <= TOL, f"max rel err {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"
    # a voice that plays the empty wave is silent; the banked voice ignored its wave_sample_rate override (or it would not match)
    assert not fr[1][:, idx == 0].any()


@pytest.mark.parametrize("kind", ["staged", "global"])
def test_wide_render_takes_the_specialised_kernel_by_itself(S, oracle, kind):
    """4160 voices (65 waves of lanes), flags 0 but for the exact oscillator: the dispatcher picks the specialised kernel.  The oracle
    renders the voices of each wave as one batch, after one set_wave."""
    n, T = 4160, 96
    p, ids, idx = gpu_patch(S, kind, n_voices=n)
    fr, _ = p.render(T, mix=False, flags=1)
    assert p.info().endswith("kernel=render_specialized"), p.info()
    waves, rates = bank(kind)
    clock = clock_vals(n)
    ref = np.empty((2, T, n), dtype=np.float32)
    for w in range(-1, len(waves)):
        o = oracle.OraclePatch(48000, B, 2)
        build(o, S)
        if w >= 0:
            o.set_wave(ids["smp"], waves[w], rates[w])
        who = np.flatnonzero(idx == w)
        ref[:, :, who] = o.render_batch(len(who), T, [(ids["clock"], S.OSC_VAL, clock[who])], threads=8)[0]
    np.testing.assert_array_equal(bits(fr[1]), bits(ref[1]))
    np.testing.assert_array_equal(bits(fr[0]), bits(ref[0]))


@pytest.mark.parametrize("flags", [pytest.param(1, id="exact"), pytest.param(33, id="special-exact")])
def test_a_new_assignment_under_keep_state_is_a_wave_load(S, oracle, flags):
    """render, change the assignment, render: every voice of the player starts its new wave at pos = 0, playing = false (wavebox.new),
    everything else — the clock's and the LFO's phases, the gate detector — runs on.  The oracle per voice: render, set_wave, render."""
    kind, n = "global", 200
    waves, rates = bank(kind)
    p, ids, idx = gpu_patch(S, kind)
    p.keep_state(True)
    first, _ = p.render(n, mix=False, flags=flags)
    idx2 = assignment(len(waves), V, shift=4)
    assert (idx2 != idx).any()
    p.set_voice_waves(ids["smp"], idx2)
    second, _ = p.render(n, mix=False, flags=flags)
    fr = np.concatenate([first, second], axis=1)
    own_rate, _ = rate_overrides(S, idx)
    clock = clock_vals(V)
    for v in range(V):
        ref, pos, playing = oracle_voice(S, oracle, v, clock[v], [(idx[v], waves, rates, own_rate[v], n), (idx2[v], waves, rates, own_rate[v], n)])
        np.testing.assert_array_equal(bits(fr[:, :, v]), bits(ref), err_msg=f"voice {v}: wave {idx[v]} -> {idx2[v]}")
    assert (p.get_voice_waves(ids["smp"]) == idx2).all()


@pytest.mark.parametrize("flags", [pytest.param(16, id="interpreter"), pytest.param(32, id="specialised")])
def test_a_bank_without_an_assignment_changes_nothing(S, flags):
    a, _, _ = gpu_patch(S, "global", assign=False, with_bank=False)
    b, _, _ = gpu_patch(S, "global", assign=False, with_bank=True)
    fa, ma = a.render(T1, flags=flags)
    fb, mb = b.render(T1, flags=flags)
    assert np.abs(fa).max() > 0.3
    np.testing.assert_array_equal(bits(fa), bits(fb))
    np.testing.assert_array_equal(bits(ma), bits(mb))
    assert "waves=" not in b.info() and a.info().split(" jit=")[0] == b.info().split(" jit=")[0]


# ---- the per-lane window on a bank in global memory (modules.hip.h, SmpWindow) -------------------------------------------------------
W_LENGTHS, W_RATES = [2049, 2049, 2049, 100], [48000.0, 44100.0, 8000.0, 48000.0]
_W_REF = {}


def _window_build(g, S):
    """the CV swings +-3 octaves (steps of 1/8 ... 8 samples at 48 kHz, 0.02 ... 1.3 at 8 kHz: within a group of four, into the next one
    and past it) and the gate retriggers every 37 samples (48000 / 37 Hz: val = log2(1297.3 / 440)): the window is served from, shifted,
    missed and re-centred; the 100-frame wave runs out and wraps before the retrigger"""
    ids = S.build_p4(g, wave=own_wave(), wave_rate=OWN_RATE, clock_val=float(np.log2(48000.0 / 37.0 / 440.0)))
    g.set_field(ids["lfo"], S.OSC_VAL, 0.0)           # 440 Hz: the CV crosses its whole range every 109 samples
    g.set_field(ids["depth"], S.MATH_CONSTANT, 3.0)
    return ids


def _window_bank():
    rng = np.random.default_rng(37)    # white noise: a group served one step late reads other bits
    return [rng.uniform(-1, 1, n).astype(np.float32) for n in W_LENGTHS]


@pytest.mark.parametrize("flags", [pytest.param(33, id="special-exact"), pytest.param(32, id="special-default")])
def test_the_window_never_serves_a_stale_group(S, oracle, flags):
    T, lfo_vals = T1 + T2, np.linspace(-0.5, 0.5, V).astype(np.float32)   # a vibrato rate per voice: every lane's steps its own
    waves = _window_bank()
    idx = assignment(len(waves), V)
    if not _W_REF:
        ref = np.empty((2, T, V), dtype=np.float32)
        for v in range(V):
            o = oracle.OraclePatch(48000, B, 2)
            ids = _window_build(o, S)
            o.set_field(ids["lfo"], S.OSC_VAL, lfo_vals[v])
            if idx[v] >= 0:
                o.set_wave(ids["smp"], waves[idx[v]], W_RATES[idx[v]])
            ref[:, :, v] = o.render(T)
        ref.setflags(write=False)
        _W_REF["ref"] = ref
    ref = _W_REF["ref"]
    p = S.Patch(48000, B, 2)
    ids = _window_build(p, S)
    p.configure_voices(V)
    p.set_voice_field(ids["lfo"], S.OSC_VAL, lfo_vals)
    p.set_wave_bank(ids["smp"], waves, W_RATES)
    p.set_voice_waves(ids["smp"], idx)
    assert "smp_window_read(" in p.kernel_source(flags)
    fr, _ = p.render(T, mix=False, flags=flags)
    info = p.info()
    assert info.endswith("kernel=render_specialized") and "waves=4[global]" in info, info
    # the reference does what the case is about: steps below and above a group of four, retriggers, a wave that runs out
    raw = ref[1][:, idx == 0]
    assert len(np.unique(raw)) > 100 and (ref[1][:, idx == 3] == waves[3][0]).mean() > 0.2   # (a wave that has run out reads its first sample)
    same = (bits(fr[1]) == bits(ref[1])).mean()
    err = np.abs(fr.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1.0)
    print(f"window flags {flags}: raw plane equal bits {same:.6f}, max rel err {err.max():.3e}; {info}")
    if (flags & 1) or "approx[exact:" in info:
        np.testing.assert_array_equal(bits(fr[1]), bits(ref[1]))
        np.testing.assert_array_equal(bits(fr[0]), bits(ref[0]))
    else:
        assert np.isfinite(fr).all() and err.max() <= TOL, f"max rel err {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"
