"""A sequence per voice for both sequencers (srack_patch_set_sequence_bank / srack_voices_set_sequences) against the CPU oracle, through
the C ABI.  Needs a real MI355X (-m gpu).

The contract: voice v renders what a ONE-voice patch renders whose sequencer holds bank sequence seq[v]'s cells (srack_patch_set_step) and
length (*_LENGTH).  The oracle knows no bank: it renders one voice at a time, each after its own set_step / set_field calls.  A reference
is computed once per clocking and assignment and shared.

The patch is P3's shape (workloads.build_p3): CLOCK (square) steps a grid and a pattern sequencer; the grid's CV plays the oscillator through
a transpose, its gate fires the amplitude envelope, its sync output re-syncs the pattern; pattern channel 1 gates the filter envelope and
pattern channel 5 is output channel 1 as it is.  buffer_size 100, so that every render length here is whole ticks of the oracle.  The
grid's steps_per_octave is 16384 here: note 65535 is four octaves up, and the voice that plays it stays finite audio."""
import numpy as np
import pytest

import srack_pkg

pytestmark = pytest.mark.gpu
TOL = 1e-5
B = 100
V, T1, T2 = 70, 300, 700            # one full and one ragged wave of lanes; 1 000 samples, rendered in two calls
T = T1 + T2
SPO, LAST0 = 16384.0, 0.25          # steps_per_octave; the CV the grid holds before its first note (all-rests voices keep it)
NONE, ON, HOLD = 0, 1, 2
# lengths of the bank sequences; grid sequence 5 is all rests, 6 all HOLD; pattern sequence 4 is all rests, 6 all HOLD
GRID_LEN = [1, 2, 7, 63, 64, 5, 6]
PAT_LEN = [1, 2, 7, 63, 5, 64, 6, 3]
CLOCKINGS = ["shared", "per_voice"]


@pytest.fixture(scope="module")
def S():
    S = srack_pkg.load()
    assert S.device_count() > 0, "no GPU visible: the render path has no CPU fallback"
    return S


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def grid_bank():
    """-> states u8 [7][64], values u16 [7][64] (cells past a sequence's length are set too: the bank must ignore them), lengths"""
    rng = np.random.default_rng(5)
    n = len(GRID_LEN)
    st = rng.integers(0, 3, (n, 64)).astype(np.uint8)
    vals = rng.integers(0, 65536, (n, 64)).astype(np.uint16)
    st[0, 0], st[1, :2] = ON, (ON, HOLD)
    st[5, :], st[6, :] = NONE, HOLD
    st[4, 9], vals[4, 9] = ON, 65535        # the highest note there is, and the lowest
    st[4, 10], vals[4, 10] = HOLD, 0
    return st, vals, np.array(GRID_LEN, dtype=np.intc)


def pat_bank():
    """-> states u8 [8][8][64], lengths: all eight channels random; channel 5 (the raw output) is distinct per sequence and, like the
    patch's own channel 5, holds rests and HOLDs only: output channel 1 is then 0.0 / 1.0 by sequencer arithmetic alone (an ON gate
    passes the clock's band-limited square through, which the default mode computes to its own rounding)"""
    rng = np.random.default_rng(6)
    n = len(PAT_LEN)
    st = rng.integers(0, 3, (n, 8, 64)).astype(np.uint8)
    st[:, 5, :] = HOLD * rng.integers(0, 2, (n, 64)).astype(np.uint8)
    st[4], st[6] = NONE, HOLD
    st[0, 5, 0], st[1, 5, :2], st[7, 5, :3] = HOLD, (HOLD, NONE), (NONE, NONE, HOLD)
    for a in range(n):
        for b in range(a):
            La, Lb = PAT_LEN[a], PAT_LEN[b]
            assert La != Lb or (st[a, 5, :La] != st[b, 5, :Lb]).any(), (a, b)
    return st, np.array(PAT_LEN, dtype=np.intc)


def assignment(n_sequences, n_voices, shift=0):
    """SRACK_SEQ_OWN and every sequence in turn; each further wave of 64 lanes starts five cases on, so that the ragged last wave of lanes
    (six voices at 70) holds the own sequence, a length-1 and a length-64 sequence too."""
    v = np.arange(n_voices)
    return ((v + 5 * (v // 64) + shift) % (n_sequences + 1) - 1).astype(np.intc)


def initial_steps(n_voices):
    return (63 - np.arange(n_voices) % 11).astype(np.float32)   # 53 ... 63: at or past every length but 63 / 64, which wrap within 11 steps


def clock_vals(clocking, n_voices):
    if clocking == "shared":   # every lane on the same step: a period of 15 samples, 66 steps in 1 000 samples
        return np.full(n_voices, np.log2(48000.0 / 15.0 / 440.0), dtype=np.float32)
    periods = np.linspace(14.0, 55.0, n_voices)   # lanes step on different samples; the slowest makes 18 steps
    return np.log2(48000.0 / periods / 440.0).astype(np.float32)


def build(g, S):
    ids = S.build_p3(g)
    g.set_field(ids["grid"], S.GRIDSEQ_STEPS_PER_OCTAVE, SPO)
    g.set_field(ids["grid"], S.GRIDSEQ_LAST, LAST0)
    return ids


def own_cells(S):
    """what build_p3 leaves in the two sequencers: (grid states [64], grid values [64], grid length, pattern states [8][64], pattern length)"""
    p = S.Patch(48000, B, 2)
    ids = build(p, S)
    g = np.array([p.get_step(ids["grid"], 0, i) for i in range(64)])
    ps = np.array([[p.get_step(ids["pat"], c, i)[0] for i in range(64)] for c in range(8)])
    return g[:, 0], g[:, 1], int(p.get_field(ids["grid"], S.GRIDSEQ_LENGTH)), ps, int(p.get_field(ids["pat"], S.PATSEQ_LENGTH))


def oracle_write(S, o, ids, own, gseq, pseq):
    """the voice's cells and lengths, the way a host without a bank would set them"""
    gst, gvals, glen = grid_bank()
    pst, plen = pat_bank()
    g_states, g_values, g_len = (own[0], own[1], own[2]) if gseq < 0 else (gst[gseq], gvals[gseq], int(glen[gseq]))
    p_states, p_len = (own[3], own[4]) if pseq < 0 else (pst[pseq], int(plen[pseq]))
    for i in range(64):
        inside = gseq < 0 or i < g_len
        o.set_step(ids["grid"], 0, i, int(g_states[i]) if inside else NONE, int(g_values[i]) if inside and g_states[i] != NONE else 0)
        for c in range(8):
            o.set_step(ids["pat"], c, i, int(p_states[c][i]) if (pseq < 0 or i < p_len) else NONE)
    o.set_field(ids["grid"], S.GRIDSEQ_LENGTH, g_len)
    o.set_field(ids["pat"], S.PATSEQ_LENGTH, p_len)


STATE = ["GRIDSEQ_CURRENT_STEP", "GRIDSEQ_STEP_LAST", "GRIDSEQ_SYNC_LAST", "GRIDSEQ_LAST", "PATSEQ_CURRENT_STEP", "PATSEQ_STEP_LAST", "PATSEQ_SYNC_LAST"]


def state_of(S, read, ids):
    """[7][...]: read(module, field) of every state field the two sequencers have"""
    return np.stack([np.asarray(read(ids["grid" if n.startswith("GRID") else "pat"], getattr(S, n)), dtype=np.float64) for n in STATE])


_REF = {}


def reference(S, oracle, clocking, segments):
    """segments: ((shift of the assignment or None for no assignment, samples), ...): per voice, write the cells, render, write, render.
    -> frames [2][sum of samples][V], state [7][V]; computed once, never written to"""
    key = (clocking, segments)
    if key not in _REF:
        own = own_cells(S)
        clock, init = clock_vals(clocking, V), initial_steps(V)
        n = sum(s[1] for s in segments)
        fr, state = np.empty((2, n, V), dtype=np.float32), np.empty((len(STATE), V))
        for v in range(V):
            o = oracle.OraclePatch(48000, B, 2)
            ids = build(o, S)
            o.set_field(ids["clock"], S.OSC_VAL, float(clock[v]))
            o.set_field(ids["grid"], S.GRIDSEQ_CURRENT_STEP, float(init[v]))
            o.set_field(ids["pat"], S.PATSEQ_CURRENT_STEP, float(init[(v + 3) % V]))
            out = []
            for shift, samples in segments:
                if shift is not None:
                    oracle_write(S, o, ids, own, int(assignment(len(GRID_LEN), V, shift)[v]), int(assignment(len(PAT_LEN), V, shift)[v]))
                out.append(o.render(samples))
            fr[:, :, v] = np.concatenate(out, axis=1)
            state[:, v] = state_of(S, o.get_field, ids)
        fr.setflags(write=False)
        state.setflags(write=False)
        _REF[key] = (fr, state)
    return _REF[key]


def gpu_patch(S, clocking, shift=0, with_bank=True):
    p = S.Patch(48000, B, 2)
    ids = build(p, S)
    p.configure_voices(V)
    if clocking == "shared":   # the clock stays one oscillator of the control program: the sequencers are per voice because of the assignment
        p.set_field(ids["clock"], S.OSC_VAL, float(clock_vals(clocking, V)[0]))
    else:
        p.set_voice_field(ids["clock"], S.OSC_VAL, clock_vals(clocking, V))
    p.set_voice_field(ids["grid"], S.GRIDSEQ_CURRENT_STEP, initial_steps(V))
    p.set_voice_field(ids["pat"], S.PATSEQ_CURRENT_STEP, np.roll(initial_steps(V), -3))
    if with_bank:
        gst, gvals, glen = grid_bank()
        pst, plen = pat_bank()
        p.set_sequence_bank(ids["grid"], gst, gvals, glen)
        p.set_sequence_bank(ids["pat"], pst, None, plen)
    if shift is not None:
        assign(S, p, ids, shift)
    return p, ids


def assign(S, p, ids, shift):
    p.set_voice_sequences(ids["grid"], assignment(len(GRID_LEN), V, shift))
    p.set_voice_sequences(ids["pat"], assignment(len(PAT_LEN), V, shift))


N_SEQ = len(GRID_LEN) + len(PAT_LEN)


def test_the_assignment_covers_every_case_in_every_wave_of_lanes(S):
    for lengths in (GRID_LEN, PAT_LEN):
        idx = assignment(len(lengths), V)
        assert set(idx[:64].tolist()) == set(range(-1, len(lengths)))
        tail = set(idx[64:].tolist())
        assert S.SEQ_OWN in tail and lengths.index(1) in tail and lengths.index(64) in tail   # the own sequence, a length-1 and a length-64 one
    init = initial_steps(V)
    assert init.max() == 63 and (init >= 53).all()   # at or past every length below 63: the wrap at sample 0


def check(S, p, ids, fr, ref, ref_state, exact, what):
    info = p.info()
    state = state_of(S, p.get_voice_field, ids)
    raw_same = (bits(fr[1]) == bits(ref[1])).mean()
    err = np.abs(fr.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1.0)
    print(f"{what}: raw plane equal bits {raw_same:.6f}, max rel err {err.max():.3e}, state equal {(state == ref_state).mean():.4f}; {info}")
    # the reference is not trivial: sound, a raw gate that is neither stuck low nor high, voices on many different steps
    assert np.abs(ref[0]).max() > 0.05 and 0.05 < (ref[1] != 0).mean() < 0.95 and len(np.unique(ref_state[0])) > 5
    np.testing.assert_array_equal(bits(fr[1]), bits(ref[1]))   # the raw pattern gate: sequencer arithmetic only, in every mode
    if exact or "approx[exact:" in info:
        np.testing.assert_array_equal(bits(fr[0]), bits(ref[0]))
    else:
        assert np.isfinite(fr).all() and err.max() <= TOL, f"max rel err {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"
    np.testing.assert_array_equal(state, ref_state)


@pytest.mark.parametrize("exact", [pytest.param(1, id="exact"), pytest.param(0, id="default")])
@pytest.mark.parametrize("flags", [pytest.param(16, id="interpreter"), pytest.param(32, id="specialised"), pytest.param(0, id="dispatcher")])
@pytest.mark.parametrize("clocking", CLOCKINGS)
def test_every_voice_plays_its_own_sequence(S, oracle, clocking, flags, exact):
    ref, ref_state = reference(S, oracle, clocking, ((0, T),))
    p, ids = gpu_patch(S, clocking)
    assert p.planes() == (2, [0, 1])
    fr = np.concatenate([p.render(n, mix=False, flags=flags | exact)[0] for n in (T1, T2)], axis=1)   # the second call continues the first
    info = p.info()
    # one form ships — the per-lane gather from seqtab (the step-major LDS tile lost its measurement: notes/r12.md) — in every kernel
    assert info.endswith("kernel=render_specialized" if flags == 32 else "kernel=render_interp") and "sequences=%d[global]" % N_SEQ in info, info
    check(S, p, ids, fr, ref, ref_state, exact, f"{clocking} flags {flags | exact}")


@pytest.mark.parametrize("clocking", CLOCKINGS)
def test_the_specialised_kernel_with_the_mix_down_on(S, oracle, clocking):
    """frames and mix from one launch (the kernel's other output mode): the same frames and state, bit for bit"""
    ref, ref_state = reference(S, oracle, clocking, ((0, T),))
    p, ids = gpu_patch(S, clocking)
    parts = [p.render(n, mix=True, flags=33) for n in (T1, T2)]
    fr, mix = np.concatenate([a for a, _ in parts], axis=1), np.concatenate([m for _, m in parts], axis=1)
    info = p.info()
    assert info.endswith("kernel=render_specialized") and "sequences=%d[global]" % N_SEQ in info, info
    check(S, p, ids, fr, ref, ref_state, 1, f"{clocking} flags 33 with mix")
    want = ref.astype(np.float64).sum(axis=2)   # both channels are planes of their own here
    assert np.abs(mix - want).max() <= (V + 1) * 2.0 ** -24 * np.abs(ref).astype(np.float64).sum(axis=2).max()


@pytest.mark.parametrize("flags", [pytest.param(17, id="interpreter-exact"), pytest.param(33, id="special-exact")])
@pytest.mark.parametrize("clocking", CLOCKINGS)
def test_a_new_assignment_under_keep_state_is_an_edit_of_cells(S, oracle, clocking, flags):
    """render, change the assignment, render: every voice goes on from its step, its detectors and its held CV; a step at or past the new
    length wraps to 0 on the next sample.  The oracle per voice: render, rewrite cells and length, render."""
    ref, ref_state = reference(S, oracle, clocking, ((0, T1), (4, T2)))
    p, ids = gpu_patch(S, clocking)
    p.keep_state(True)
    first, _ = p.render(T1, mix=False, flags=flags)
    assert (assignment(len(GRID_LEN), V, 4) != assignment(len(GRID_LEN), V)).any()
    assign(S, p, ids, 4)
    second, _ = p.render(T2, mix=False, flags=flags)
    check(S, p, ids, np.concatenate([first, second], axis=1), ref, ref_state, 1, f"keep_state {clocking} flags {flags}")
    assert (p.get_voice_sequences(ids["grid"]) == assignment(len(GRID_LEN), V, 4)).all()


def test_a_new_assignment_without_keep_state_restarts_the_voices(S, oracle):
    ref, ref_state = reference(S, oracle, "per_voice", ((4, T2),))
    p, ids = gpu_patch(S, "per_voice")
    p.render(T1, mix=False, flags=33)
    assign(S, p, ids, 4)
    second, _ = p.render(T2, mix=False, flags=33)
    check(S, p, ids, second, ref, ref_state, 1, "no keep_state")


@pytest.mark.parametrize("flags", [pytest.param(16, id="interpreter"), pytest.param(32, id="specialised")])
def test_a_bank_without_an_assignment_changes_nothing(S, flags):
    a, _ = gpu_patch(S, "per_voice", shift=None, with_bank=False)
    b, _ = gpu_patch(S, "per_voice", shift=None, with_bank=True)
    fa, ma = a.render(T1, flags=flags)
    fb, mb = b.render(T1, flags=flags)
    assert np.abs(fa).max() > 0.05
    np.testing.assert_array_equal(bits(fa), bits(fb))
    np.testing.assert_array_equal(bits(ma), bits(mb))
    assert "sequences=" not in b.info() and a.info().split(" jit=")[0] == b.info().split(" jit=")[0]


@pytest.mark.parametrize("flags", [pytest.param(17, id="interpreter-exact"), pytest.param(33, id="special-exact")])
def test_buses_and_statistics_of_an_assigned_patch(S, oracle, flags):
    """srack_render_buses on the assigned patch: the frames are the plain render's bit for bit, every bus is the weighted f32 sum of its
    voices' frames (any order of summation: |bus - sum| <= (n + 1) 2^-24 sum |gain x| for n voices — one rounding per product, n - 1 per
    fold, second-order terms), and the per-voice peaks are the frames' own."""
    ref, ref_state = reference(S, oracle, "per_voice", ((0, T),))
    p, ids = gpu_patch(S, "per_voice")
    rng = np.random.default_rng(9)
    n_buses = 5
    bus, gain = rng.integers(-1, n_buses, V).astype(np.intc), rng.uniform(-2, 2, V).astype(np.float32)
    p.set_buses(n_buses, bus, gain)
    fr, _, st, bm = p.render_buses(T, frames=True, stats=True, flags=flags)
    check(S, p, ids, fr, ref, ref_state, 1, f"buses flags {flags}")
    assert "buses=%d[fold]" % n_buses in p.info() and bm.shape == (n_buses, 2, T)
    n_planes, cp = p.planes()
    for b in range(n_buses):
        who = np.flatnonzero(bus == b)
        assert len(who) > 3
        for c in range(2):
            prod = fr[cp[c]][:, who].astype(np.float64) * gain[who].astype(np.float64)
            lim = (len(who) + 1) * 2.0 ** -24 * np.abs(prod).sum(axis=1) + len(who) * 2.0 ** -149
            assert (np.abs(bm[b, c] - prod.sum(axis=1)) <= lim).all(), (b, c)
    assert np.abs(bm).max() > 0.05
    np.testing.assert_array_equal(st[:, S.STAT_PEAK_POS, :], np.maximum(fr.max(axis=1), 0).astype(np.float64))
    np.testing.assert_array_equal(st[:, S.STAT_PEAK_NEG, :], np.maximum((-fr).max(axis=1), 0).astype(np.float64))
    np.testing.assert_array_equal(st[:, S.STAT_SUM, :], fr.astype(np.float64).cumsum(axis=1)[:, -1, :])   # (the sequential f64 loop)
    assert not st[:, S.STAT_NONFINITE, :].any()
