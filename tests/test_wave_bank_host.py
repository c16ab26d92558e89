"""The sample player's wave bank (srack_patch_set_wave_bank / srack_voices_set_waves): the C ABI surface, the bindings, the argument
checks, and what the flattener and the kernel generator make of an assignment — read from srack_render_info and from the generated
source, without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import srack_pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["srack_patch_set_wave_bank", "srack_patch_get_wave_bank", "srack_patch_get_wave_bank_samples", "srack_voices_set_waves", "srack_voices_get_waves"]


@pytest.fixture(scope="module")
def S():
    return srack_pkg.load()


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _bank(lengths, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, n).astype(np.float32) for n in lengths]


def test_symbols_and_bindings(S):
    hdr = open(os.path.join(ROOT, "include", "srack_hip.h")).read()
    L = ctypes.CDLL(S.LIB_PATH)
    assert L.srack_abi_version() == 2
    assert re.search(r"#define SRACK_WAVE_OWN\s+\(-1\)", hdr) and S.WAVE_OWN == -1
    src = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hpp = open(os.path.join(ROOT, "include", "srack.hpp")).read()
    for name in NAMES:
        assert name in S.ABI_SYMBOLS and hasattr(L, name), name
        assert getattr(S.lib, name).argtypes is not None, name
        assert re.search(r"pub fn %s\(" % name, src), name
        assert "ffi::%s(" % name in src, name
        assert name in doc, name
        assert name + "(" in hpp, name
    assert "pub const WAVE_OWN: i32 = -1;" in src
    for wrapper in ("set_wave_bank", "get_wave_bank", "set_voice_waves", "get_voice_waves"):
        assert hasattr(S.Patch, wrapper), wrapper


def test_round_trips(S):
    p = S.Patch(48000, 1024, 2)
    ids = S.build_p4(p)
    smp = ids["smp"]
    own, own_rate = p.get_wave(smp)
    assert p.get_wave_bank(smp)[0] == [] and p.get_voice_waves(smp) is None
    odd = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -3.5], dtype=np.float32)   # any f32 is accepted
    waves = _bank([0, 1, 3, 255]) + [odd]
    rates = [8000.0, 44100.0, 48000.0, 22050.5, 1.0]
    p.set_wave_bank(smp, waves, rates)
    got, sr = p.get_wave_bank(smp)
    assert len(got) == 5 and (sr == np.array(rates, dtype=np.float32)).all()
    for a, b in zip(got, waves):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    # the bank is copied, and the module's own wave and rate stay what they were
    waves[3][:] = 9.0
    assert not (p.get_wave_bank(smp)[0][3] == 9.0).any()
    w2, r2 = p.get_wave(smp)
    assert r2 == own_rate and np.array_equal(w2, own) and p.get_field(smp, S.SAMPLE_WAVE_SAMPLE_RATE) == own_rate
    # short reads
    lengths = np.full(5, 77, dtype=np.intc)
    assert S.lib.srack_patch_get_wave_bank(p.h, smp, _ip(lengths), None, 2) == 5
    assert lengths.tolist() == [0, 1, 77, 77, 77]
    buf = np.full(8, 5.0, dtype=np.float32)
    assert S.lib.srack_patch_get_wave_bank_samples(p.h, smp, 3, _fp(buf), 4) == 255 and (buf[4:] == 5.0).all() and (buf[:4] != 5.0).all()
    # the assignment
    V = 10
    p.configure_voices(V)
    idx = (np.arange(V) % 6 - 1).astype(np.intc)   # OWN and every wave
    p.set_voice_waves(smp, idx)
    assert (p.get_voice_waves(smp) == idx).all()
    short = np.full(V, 99, dtype=np.intc)
    assert S.lib.srack_voices_get_waves(p.h, smp, _ip(short), 3) == V and short.tolist() == idx[:3].tolist() + [99] * 7
    p.set_voice_waves(smp, None)
    assert p.get_voice_waves(smp) is None
    # n_waves == 0 removes the bank
    p.set_wave_bank(smp, [], [])
    assert p.get_wave_bank(smp)[0] == []


def test_errors_and_what_drops_an_assignment(S):
    V = 6
    p = S.Patch(48000, 1024, 2)
    ids = S.build_p4(p)
    smp, osc = ids["smp"], ids["clock"]
    waves, rates = _bank([4, 0, 9]), [8000.0, 44100.0, 48000.0]
    flat = np.concatenate(waves)
    lengths, sr = np.array([4, 0, 9], dtype=np.intc), np.array(rates, dtype=np.float32)
    idx = np.array([0, 1, 2, -1, 2, 0], dtype=np.intc)
    # a null handle, a module that is no sample player, pointers that must be given
    assert S.lib.srack_patch_set_wave_bank(None, smp, _fp(flat), _ip(lengths), _fp(sr), 3) == S.ERR_INVALID
    assert S.lib.srack_voices_set_waves(None, smp, _ip(idx)) == S.ERR_INVALID
    for m in (osc, -1, 99):
        assert S.lib.srack_patch_set_wave_bank(p.h, m, _fp(flat), _ip(lengths), _fp(sr), 3) == S.ERR_INVALID
        assert S.lib.srack_patch_get_wave_bank(p.h, m, None, None, 0) == S.ERR_INVALID
        assert S.lib.srack_patch_get_wave_bank_samples(p.h, m, 0, None, 0) == S.ERR_INVALID
        assert S.lib.srack_voices_set_waves(p.h, m, _ip(idx)) == S.ERR_INVALID
        assert S.lib.srack_voices_get_waves(p.h, m, None, 0) == S.ERR_INVALID
    assert S.lib.srack_patch_set_wave_bank(p.h, smp, None, _ip(lengths), _fp(sr), 3) == S.ERR_INVALID
    assert S.lib.srack_patch_set_wave_bank(p.h, smp, _fp(flat), None, _fp(sr), 3) == S.ERR_INVALID
    assert S.lib.srack_patch_set_wave_bank(p.h, smp, _fp(flat), _ip(lengths), None, 3) == S.ERR_INVALID
    assert S.lib.srack_patch_set_wave_bank(p.h, smp, _fp(flat), _ip(np.array([4, -1, 9], dtype=np.intc)), _fp(sr), 3) == S.ERR_INVALID
    assert p.get_wave_bank(smp)[0] == []
    # before the voices are configured
    assert S.lib.srack_voices_set_waves(p.h, smp, _ip(idx)) == S.ERR_STATE
    assert "voices_configure" in S.lib.srack_last_error().decode()
    p.configure_voices(V)
    # an index >= 0 with no bank set
    assert S.lib.srack_voices_set_waves(p.h, smp, _ip(idx)) == S.ERR_INVALID
    p.set_voice_waves(smp, np.full(V, S.WAVE_OWN, dtype=np.intc))   # (OWN needs no bank)
    p.set_voice_waves(smp, None)
    p.set_wave_bank(smp, waves, rates)
    assert S.lib.srack_patch_get_wave_bank_samples(p.h, smp, 3, None, 0) == S.ERR_INVALID
    assert S.lib.srack_patch_get_wave_bank_samples(p.h, smp, -1, None, 0) == S.ERR_INVALID
    p.set_voice_waves(smp, idx)
    # an index outside [-1, n_waves): the earlier assignment stays
    for bad in (3, -2, 1 << 20):
        b = idx.copy()
        b[4] = bad
        assert S.lib.srack_voices_set_waves(p.h, smp, _ip(b)) == S.ERR_INVALID, bad
        assert (p.get_voice_waves(smp) == idx).all()
    # setting a bank drops the assignment; so does configure
    p.set_wave_bank(smp, waves, rates)
    assert p.get_voice_waves(smp) is None
    p.set_voice_waves(smp, idx)
    p.configure_voices(V)
    assert p.get_voice_waves(smp) is None and len(p.get_wave_bank(smp)[0]) == 3
    # rack files carry neither
    p.set_voice_waves(smp, idx)
    q = S.Patch.load_srk(p.save_srk(), 48000, 1024, 2)
    players = [m for m in range(q.num_modules()) if S.lib.srack_patch_module_type(q.h, m) == S.MOD_SAMPLE]   # (a load reverses the list)
    assert len(players) == 1 and q.get_wave_bank(players[0])[0] == [] and len(q.get_wave(players[0])[0]) == 1500


def test_source_is_the_same_until_voices_are_assigned(S):
    V = 64
    p = S.Patch(48000, 1024, 2)
    ids = S.build_p4(p)
    smp = ids["smp"]
    p.configure_voices(V)
    depth, expo = S.p4_voice_params(V)
    p.set_voice_field(ids["depth"], S.MATH_CONSTANT, depth)
    p.set_voice_field(ids["shaper"], S.NONLIN_CONSTANT, expo)
    plain = p.kernel_source(S.RENDER_SPECIALIZE)
    info = p.info()
    assert "waves=" not in info
    p.set_wave_bank(smp, _bank([10, 300]), [8000.0, 48000.0])
    assert p.kernel_source(S.RENDER_SPECIALIZE) == plain and "waves=" not in p.info()
    p.set_voice_waves(smp, np.arange(V, dtype=np.intc) % 3 - 1)
    banked = p.kernel_source(S.RENDER_SPECIALIZE)
    assert banked != plain and "_base" in banked and "waves=2[" in p.info()
    p.set_voice_waves(smp, None)
    assert p.kernel_source(S.RENDER_SPECIALIZE) == plain and "waves=" not in p.info()


def test_staging_choice_is_in_the_source(S):
    V = 64
    for bank_len, staged in ((400, True), (2049 - 1500 + 1, False), (5000, False)):   # own wave: 1500 frames; 1500 + 400 <= 2048 < 1500 + 550
        p = S.Patch(48000, 1024, 2)
        ids = S.build_p4(p)
        p.configure_voices(V)
        p.set_wave_bank(ids["smp"], _bank([bank_len]), [44100.0])
        p.set_voice_waves(ids["smp"], np.arange(V, dtype=np.intc) % 2 - 1)
        src = p.kernel_source(S.RENDER_SPECIALIZE)
        assert ("_bank_lds[2048]" in src) == staged, bank_len
        assert ("smp_window_read(" in src) == (not staged), bank_len   # global memory: the per-lane window
        p.kernel_compile(S.RENDER_SPECIALIZE)   # hiprtc, gfx950: no GPU needed


def test_three_players_share_the_lds_budget(S):
    """Three players with an 8 KB wave each: every one of them fits the kernel's LDS share alone (20 KB less tables and a mix tile at two
    waves per SIMD), all three do not — the copies are counted together."""
    p = S.Patch(48000, 1024, 4)
    clock, out = p.add_module(S.MOD_OSCILLATOR), p.add_module(S.MOD_OUTPUT)
    wave = _bank([2048])[0]
    for c in range(3):
        smp = p.add_module(S.MOD_SAMPLE)
        p.set_wave(smp, wave, 44100.0)
        p.connect(clock, S.OSC_OUT_SQUARE, smp, 0)
        p.connect(smp, 0, out, c)
    p.configure_voices(64)
    p.set_voice_field(clock, S.OSC_VAL, np.linspace(-3, -2, 64).astype(np.float32))
    src = p.kernel_source(S.RENDER_SPECIALIZE)
    staged = re.findall(r"__shared__ uint32_t \w*_wave_lds\[(\d+)\]", src)
    share = 160 * 1024 // (4 * 2) - 1024 - 8704
    assert staged and all(n == "2048" for n in staged)
    assert 4 * 2048 * len(staged) <= share < 4 * 2048 * 3, staged
    p.kernel_compile(S.RENDER_SPECIALIZE)


def test_an_assigned_player_is_never_hoisted(S):
    """A player without overrides whose gate and CV come from voice-invariant modules is evaluated once, by the control program — until
    its voices are assigned waves."""
    V = 128
    p = S.Patch(48000, 1024, 2)
    clock, lfo, smp, gain, out = (p.add_module(t) for t in (S.MOD_OSCILLATOR, S.MOD_OSCILLATOR, S.MOD_SAMPLE, S.MOD_MATH, S.MOD_OUTPUT))
    p.set_field(clock, S.OSC_VAL, -3.0)
    p.set_field(lfo, S.OSC_VAL, -5.0)
    p.set_field(gain, S.MATH_OPERATION, S.MATH_MULTIPLY)
    p.set_wave(smp, S.p4_wave(), 44100.0)
    p.connect(clock, S.OSC_OUT_SQUARE, smp, 0)
    p.connect(lfo, S.OSC_OUT_SINE, smp, 1)
    p.connect(smp, 0, gain, 0)
    p.connect(gain, 0, out, 0)
    p.configure_voices(V)
    p.set_voice_field(gain, S.MATH_CONSTANT, np.linspace(0.1, 1, V).astype(np.float32))

    def voice_ops():
        return int(re.search(r"voice\[ops=(\d+)", p.info()).group(1))

    assert voice_ops() == 2 and " + ctl[" in p.info()            # the gain and the output; the player is the control program's
    p.set_wave_bank(smp, _bank([100, 7]), [8000.0, 48000.0])
    assert voice_ops() == 2
    p.set_voice_waves(smp, np.arange(V, dtype=np.intc) % 3 - 1)
    assert voice_ops() == 3 and " + ctl[" in p.info() and "waves=2[" in p.info()   # the player per voice; clock and LFO stay shared
    src = p.kernel_source(S.RENDER_SPECIALIZE)
    assert "_base" in src
    p.set_voice_waves(smp, None)
    assert voice_ops() == 2
