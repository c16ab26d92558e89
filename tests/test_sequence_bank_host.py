"""The sequencers' sequence bank (srack_patch_set_sequence_bank / srack_voices_set_sequences): the C ABI surface, the bindings, the
argument checks, and what the flattener, the error bound and the kernel generator make of an assignment — read from srack_render_info and
from the generated source, without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import srack_pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["srack_patch_set_sequence_bank", "srack_patch_get_sequence_bank", "srack_voices_set_sequences", "srack_voices_get_sequences"]
NONE, ON, HOLD = 0, 1, 2


@pytest.fixture(scope="module")
def S():
    return srack_pkg.load()


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _p3(S, n_voices=0):
    p = S.Patch(48000, 1024, 2)
    ids = S.build_p3(p)
    if n_voices:
        p.configure_voices(n_voices)
    return p, ids


def _grid_bank(n=3, seed=3):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 3, (n, 64)).astype(np.uint8), rng.integers(0, 65536, (n, 64)).astype(np.uint16), rng.integers(1, 65, n).astype(np.intc)


def _own(p, module, channels):
    return [[p.get_step(module, c, i) for i in range(64)] for c in range(channels)]


def test_symbols_and_bindings(S):
    hdr = open(os.path.join(ROOT, "include", "srack_hip.h")).read()
    L = ctypes.CDLL(S.LIB_PATH)
    assert L.srack_abi_version() == 2
    assert re.search(r"#define SRACK_SEQ_OWN\s+\(-1\)", hdr) and S.SEQ_OWN == -1
    assert re.search(r"#define SRACK_MAX_SEQUENCES\s+65536", hdr) and S.MAX_SEQUENCES == 65536
    src = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hpp = open(os.path.join(ROOT, "include", "srack.hpp")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in S.ABI_SYMBOLS and hasattr(L, name), name
        assert getattr(S.lib, name).argtypes is not None, name
        assert re.search(r"pub fn %s\(" % name, src), name
        assert "ffi::%s(" % name in src, name
        assert name in doc, name
        assert name + "(" in hpp, name
    assert "pub const SEQ_OWN: i32 = -1;" in src
    for wrapper in ("set_sequence_bank", "get_sequence_bank", "set_voice_sequences", "get_voice_sequences"):
        assert hasattr(S.Patch, wrapper), wrapper
        assert "pub fn %s(" % wrapper in src and " %s(" % wrapper in hpp, wrapper


def test_round_trips_of_a_grid_sequencer(S):
    p, ids = _p3(S)
    grid = ids["grid"]
    own, own_len = _own(p, grid, 1), p.get_field(grid, S.GRIDSEQ_LENGTH)
    st, vals, ln = p.get_sequence_bank(grid)
    assert st.shape == (0, 1, 64) and vals.shape == (0, 64) and len(ln) == 0 and p.get_voice_sequences(grid) is None
    st = np.tile(np.array([NONE, ON, HOLD, ON], dtype=np.uint8), (4, 16))       # every state
    vals = np.tile(np.array([7, 0, 65535, 1234], dtype=np.uint16), (4, 16))     # note values 0 and 65535
    lengths = np.array([1, 64, 7, 63], dtype=np.intc)                           # lengths 1 and 64
    p.set_sequence_bank(grid, st, vals, lengths)
    got_st, got_vals, got_len = p.get_sequence_bank(grid)
    assert got_len.tolist() == lengths.tolist()
    for k, n in enumerate(lengths):
        assert got_st[k, 0, :n].tolist() == st[k, :n].tolist()
        assert got_vals[k, :n].tolist() == np.where(st[k, :n] != NONE, vals[k, :n], 0).tolist()   # (a rest has no note)
        assert not got_st[k, 0, n:].any() and not got_vals[k, n:].any()                            # a sequence ends at its length
    # the bank is copied, and the module's own cells and length stay what they were
    st[:], vals[:] = HOLD, 9
    assert p.get_sequence_bank(grid)[0][1, 0, :4].tolist() == [NONE, ON, HOLD, ON] and p.get_sequence_bank(grid)[1][1, 2] == 65535
    assert _own(p, grid, 1) == own and p.get_field(grid, S.GRIDSEQ_LENGTH) == own_len
    # values = NULL: all notes 0
    p.set_sequence_bank(grid, np.full((2, 64), ON, dtype=np.uint8), None, [64, 2])
    st2, vals2, len2 = p.get_sequence_bank(grid)
    assert len2.tolist() == [64, 2] and st2[0].all() and not vals2.any()
    # short reads
    p.set_sequence_bank(grid, np.tile(np.array([NONE, ON, HOLD, ON], dtype=np.uint8), (4, 16)), vals, lengths)
    short_len, short_st = np.full(4, 77, dtype=np.intc), np.full((4, 64), 9, dtype=np.uint8)
    assert S.lib.srack_patch_get_sequence_bank(p.h, grid, short_st.ctypes.data, None, _ip(short_len), 2) == 4
    assert short_len.tolist() == [1, 64, 77, 77] and (short_st[2:] == 9).all() and short_st[1, :4].tolist() == [NONE, ON, HOLD, ON]
    # the assignment
    V = 10
    p.configure_voices(V)
    idx = (np.arange(V) % 5 - 1).astype(np.intc)   # OWN and every sequence
    p.set_voice_sequences(grid, idx)
    assert (p.get_voice_sequences(grid) == idx).all()
    short = np.full(V, 99, dtype=np.intc)
    assert S.lib.srack_voices_get_sequences(p.h, grid, _ip(short), 3) == V and short.tolist() == idx[:3].tolist() + [99] * 7
    p.set_voice_sequences(grid, None)
    assert p.get_voice_sequences(grid) is None
    # n_sequences == 0 removes the bank
    p.set_sequence_bank(grid, np.zeros((0, 64), dtype=np.uint8))
    assert len(p.get_sequence_bank(grid)[2]) == 0
    assert S.lib.srack_patch_set_sequence_bank(p.h, grid, None, None, None, 0) == S.OK


def test_round_trips_of_a_pattern_sequencer(S):
    p, ids = _p3(S)
    pat = ids["pat"]
    own, own_len = _own(p, pat, 8), p.get_field(pat, S.PATSEQ_LENGTH)
    rng = np.random.default_rng(8)
    st = rng.integers(0, 3, (3, 8, 64)).astype(np.uint8)
    st[0, :, 0] = [NONE, ON, HOLD, NONE, ON, HOLD, NONE, ON]   # every state, on every channel
    lengths = np.array([1, 64, 33], dtype=np.intc)
    p.set_sequence_bank(pat, st, np.full((3, 64), 5, dtype=np.uint16), lengths)   # (values are ignored)
    got_st, got_vals, got_len = p.get_sequence_bank(pat, 8)
    assert got_len.tolist() == lengths.tolist() and not got_vals.any()
    for k, n in enumerate(lengths):
        assert (got_st[k, :, :n] == st[k, :, :n]).all() and not got_st[k, :, n:].any()
    p.set_sequence_bank(pat, st, None, lengths)   # values may be NULL
    st[:] = ON
    assert (p.get_sequence_bank(pat, 8)[0][0, :, 0] == [NONE, ON, HOLD, NONE, ON, HOLD, NONE, ON]).all()
    assert _own(p, pat, 8) == own and p.get_field(pat, S.PATSEQ_LENGTH) == own_len
    p.configure_voices(5)
    idx = np.array([2, -1, 0, 1, 2], dtype=np.intc)
    p.set_voice_sequences(pat, idx)
    assert (p.get_voice_sequences(pat) == idx).all() and p.get_voice_sequences(ids["grid"]) is None
    p.set_sequence_bank(pat, np.zeros((0, 8, 64), dtype=np.uint8))
    assert len(p.get_sequence_bank(pat, 8)[2]) == 0 and p.get_voice_sequences(pat) is None


def test_errors_and_what_drops_an_assignment(S):
    V = 6
    p, ids = _p3(S)
    grid, pat, osc = ids["grid"], ids["pat"], ids["clock"]
    st, vals, lengths = _grid_bank(3)
    idx = np.array([0, 1, 2, -1, 2, 0], dtype=np.intc)

    def set_bank(h, m, states=st, values=vals, lens=lengths, n=3):
        return S.lib.srack_patch_set_sequence_bank(h, m, None if states is None else states.ctypes.data, None if values is None else values.ctypes.data,
                                                   None if lens is None else _ip(lens), n)

    # a null handle, a module that is no sequencer, pointers that must be given
    assert set_bank(None, grid) == S.ERR_INVALID
    assert S.lib.srack_voices_set_sequences(None, grid, _ip(idx)) == S.ERR_INVALID
    for m in (osc, -1, 99):
        assert set_bank(p.h, m) == S.ERR_INVALID
        assert S.lib.srack_patch_get_sequence_bank(p.h, m, None, None, None, 0) == S.ERR_INVALID
        assert S.lib.srack_voices_set_sequences(p.h, m, _ip(idx)) == S.ERR_INVALID
        assert S.lib.srack_voices_get_sequences(p.h, m, None, 0) == S.ERR_INVALID
    assert set_bank(p.h, grid, states=None) == S.ERR_INVALID
    assert set_bank(p.h, grid, lens=None) == S.ERR_INVALID
    assert len(p.get_sequence_bank(grid)[2]) == 0
    # before the voices are configured
    assert S.lib.srack_voices_set_sequences(p.h, grid, _ip(idx)) == S.ERR_STATE
    assert "voices_configure" in S.lib.srack_last_error().decode()
    p.configure_voices(V)
    # an index >= 0 with no bank set
    assert S.lib.srack_voices_set_sequences(p.h, grid, _ip(idx)) == S.ERR_INVALID
    p.set_voice_sequences(grid, np.full(V, S.SEQ_OWN, dtype=np.intc))   # (OWN needs no bank)
    p.set_voice_sequences(grid, None)
    p.set_sequence_bank(grid, st, vals, lengths)
    p.set_voice_sequences(grid, idx)
    before = [a.copy() for a in p.get_sequence_bank(grid)]

    def unchanged():
        return all((a == b).all() for a, b in zip(p.get_sequence_bank(grid), before)) and (p.get_voice_sequences(grid) == idx).all()

    # a state outside 0..2, a length outside 1..64, too many sequences: the earlier bank and assignment stay
    bad_st = st.copy()
    bad_st[2, 63] = 3      # (also past that sequence's length: every state of the array is checked)
    assert set_bank(p.h, grid, states=bad_st) == S.ERR_INVALID and unchanged()
    for bad_len in (0, 65, -1):
        ln = lengths.copy()
        ln[1] = bad_len
        assert set_bank(p.h, grid, lens=ln) == S.ERR_INVALID and unchanged(), bad_len
    assert set_bank(p.h, grid, n=S.MAX_SEQUENCES + 1) == S.ERR_INVALID and unchanged()   # (refused before anything is read)
    # an index outside [-1, n_sequences): the earlier assignment stays
    for bad in (3, -2, 1 << 20):
        b = idx.copy()
        b[4] = bad
        assert S.lib.srack_voices_set_sequences(p.h, grid, _ip(b)) == S.ERR_INVALID, bad
        assert unchanged()
    # setting a bank drops the assignment (the other sequencer's stays); so does configure
    pst = np.zeros((2, 8, 64), dtype=np.uint8)
    p.set_sequence_bank(pat, pst, None, [3, 4])
    p.set_voice_sequences(pat, np.array([0, 1, -1, 0, 1, -1], dtype=np.intc))
    p.set_sequence_bank(grid, st, vals, lengths)
    assert p.get_voice_sequences(grid) is None and p.get_voice_sequences(pat) is not None
    p.set_voice_sequences(grid, idx)
    p.configure_voices(V)
    assert p.get_voice_sequences(grid) is None and p.get_voice_sequences(pat) is None and len(p.get_sequence_bank(grid)[2]) == 3
    # the largest bank there may be is accepted
    big = np.zeros((S.MAX_SEQUENCES, 64), dtype=np.uint8)
    assert set_bank(p.h, grid, states=big, values=None, lens=np.full(S.MAX_SEQUENCES, 64, dtype=np.intc), n=S.MAX_SEQUENCES) == S.OK
    p.set_sequence_bank(grid, st, vals, lengths)
    # rack files carry neither
    p.set_voice_sequences(grid, idx)
    q = S.Patch.load_srk(p.save_srk(), 48000, 1024, 2)
    grids = [m for m in range(q.num_modules()) if S.lib.srack_patch_module_type(q.h, m) == S.MOD_GRID_SEQUENCER]
    assert len(grids) == 1 and len(q.get_sequence_bank(grids[0])[2]) == 0 and _own(q, grids[0], 1) == _own(p, grid, 1)


def _program(info):
    return info.split(" jit=")[0].split(" sequences=")[0]


def test_a_bank_is_inert_until_voices_are_assigned(S):
    V = 64
    p, ids = _p3(S, V)
    p.set_voice_field(ids["transpose"], S.MATH_CONSTANT, np.linspace(-1, 1, V).astype(np.float32))
    plain, info = p.kernel_source(S.RENDER_SPECIALIZE), p.info()
    assert "sequences=" not in info and "srk_ctl0" in plain      # the sequencers belong to the control program
    st, vals, lengths = _grid_bank(5)
    p.set_sequence_bank(ids["grid"], st, vals, lengths)
    p.set_sequence_bank(ids["pat"], np.ones((2, 8, 64), dtype=np.uint8), None, [3, 64])
    assert p.kernel_source(S.RENDER_SPECIALIZE) == plain and p.info() == info
    p.set_voice_sequences(ids["grid"], np.arange(V, dtype=np.intc) % 6 - 1)
    banked = p.kernel_source(S.RENDER_SPECIALIZE)
    assert banked != plain and "this lane's sequence" in banked and "sequences=5[" in p.info()
    p.set_voice_sequences(ids["grid"], None)
    assert p.kernel_source(S.RENDER_SPECIALIZE) == plain and p.info() == info


def test_an_assigned_sequencer_is_never_hoisted(S):
    """P3 with a per-voice transpose only: both sequencers, the clock and both envelopes are the control program's, and the voice program
    is the fused sequencer chain — until voices are assigned sequences.  Then that sequencer and what hangs off it are per voice, the
    general path renders, and the other sequencer stays where it was."""
    V = 128
    p, ids = _p3(S, V)
    p.set_voice_field(ids["transpose"], S.MATH_CONSTANT, np.linspace(-1, 1, V).astype(np.float32))

    def voice(info):
        m = re.search(r"voice\[ops=(\d+) .*? fused=(\d+)\]", info)
        return int(m.group(1)), int(m.group(2))

    assert voice(p.info()) == (6, 5) and " + ctl[" in p.info()            # transpose, oscillator, filter, VCA, two outputs: FUSED_VOICE_CHAIN_SEQ
    st, vals, lengths = _grid_bank(4)
    p.set_sequence_bank(ids["grid"], st, vals, lengths)
    assert voice(p.info()) == (6, 5)
    p.set_voice_sequences(ids["grid"], np.arange(V, dtype=np.intc) % 5 - 1)
    info = p.info()
    n_ops, fused = voice(info)
    assert fused == 0 and n_ops > 6 and " + ctl[" in info and "sequences=4[" in info, info   # the clock is still shared
    src = p.kernel_source(S.RENDER_SPECIALIZE)
    assert len(re.findall(r"_len = row\(\d+\);", src)) == 1 and len(re.findall(r"_len = \(uint32_t\)a\.ops\[\d+\]\.seq_len;", src)) == 1   # the grid per lane; the pattern (re-synced by the grid: per voice too) on its own cells
    p.kernel_compile(S.RENDER_SPECIALIZE)   # hiprtc, gfx950: no GPU needed
    p.set_voice_sequences(ids["pat"], np.full(V, S.SEQ_OWN, dtype=np.intc))   # OWN everywhere is an assignment too
    src = p.kernel_source(S.RENDER_SPECIALIZE)
    assert len(re.findall(r"_len = row\(\d+\);", src)) == 2 and "sequences=4[" in p.info()
    p.kernel_compile(S.RENDER_SPECIALIZE)
    p.set_voice_sequences(ids["grid"], None)
    p.set_voice_sequences(ids["pat"], None)
    assert voice(p.info()) == (6, 5)


def _approx(info):
    m = re.search(r"approx\[(.*?)\]", info)
    return m.group(1) if m else None


def test_the_bound_sees_the_bank(S):
    """A grid whose own notes are <= 12 with a bank sequence that holds note 6000 (500 octaves at 12 steps per octave), against a patch
    whose OWN cells hold note 6000: once voices are assigned the analysis gives both the same result; without an assignment the first
    patch gets what it gets with no bank."""
    V = 64

    def patch():
        p, ids = _p3(S, V)
        p.set_voice_field(ids["transpose"], S.MATH_CONSTANT, np.linspace(-1, 1, V).astype(np.float32))
        return p, ids

    a, ids = patch()
    no_bank = _approx(a.info())
    st, vals = np.zeros((2, 64), dtype=np.uint8), np.zeros((2, 64), dtype=np.uint16)
    st[:, :4], vals[0, :4], vals[1, :4] = ON, (1, 2, 3, 4), (5, 6000, 7, 8)
    a.set_sequence_bank(ids["grid"], st, vals, [4, 4])
    assert _approx(a.info()) == no_bank
    b, ids_b = patch()
    b.set_step(ids_b["grid"], 0, 1, S.STEP_ON, 6000)
    high = _approx(b.info())
    assert high is not None and high != no_bank, (high, no_bank)   # (or the comparison below would show nothing)
    # every voice on the OWN cells is an assignment: the bank counts, whoever plays it
    a.set_voice_sequences(ids["grid"], np.full(V, S.SEQ_OWN, dtype=np.intc))
    b.set_voice_sequences(ids_b["grid"], np.full(V, S.SEQ_OWN, dtype=np.intc))   # (the same program shape on both sides)
    assert _approx(a.info()) == _approx(b.info()) and _approx(a.info()) is not None
    a.set_voice_sequences(ids["grid"], np.arange(V, dtype=np.intc) % 3 - 1)
    assert _approx(a.info()) == _approx(b.info())
    # a pattern sequencer has no notes: its bank changes no bound
    c, ids_c = patch()
    c.set_voice_sequences(ids_c["pat"], np.full(V, S.SEQ_OWN, dtype=np.intc))
    low = _approx(c.info())
    c.set_sequence_bank(ids_c["pat"], np.full((1, 8, 64), HOLD, dtype=np.uint8), None, [64])
    c.set_voice_sequences(ids_c["pat"], np.zeros(V, dtype=np.intc))
    assert _approx(c.info()) == low and low is not None
