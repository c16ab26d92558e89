"""Bus VCAs (srack_buses_set_vca / _get_vca / _reset_vca / _vca_state / srack_buses_vca): the C ABI surface, the bindings, the argument
and lifetime rules without a GPU — and tests/busvca_ref.py, the reference the GPU tests compare with, held to the oracle's ADSRModule
and VCAModule bit for bit."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import srack_pkg
from oracle import oracle as O
from tests import busvca_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["srack_buses_set_vca", "srack_buses_get_vca", "srack_buses_reset_vca", "srack_buses_vca_state", "srack_buses_vca"]

_CTYPES = {"srack_patch*": ctypes.c_void_p, "const srack_patch*": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int,
           "const int*": ctypes.POINTER(ctypes.c_int), "int*": ctypes.POINTER(ctypes.c_int), "const float*": ctypes.POINTER(ctypes.c_float),
           "float*": ctypes.POINTER(ctypes.c_float), "void*": ctypes.c_void_p}
_DEVICE_POINTERS = {"d_rows", "d_ctl", "d_out", "d_env"}  # (device addresses travel as integers: c_void_p)
DEFAULTS = [0.0, 0.5, 0.25, 0.5]
FRESH = [0.0, 4.0, 0.0, 0.0, 48000.0, 1.0]


@pytest.fixture(scope="module")
def S():
    return srack_pkg.load()


def _prototype(hdr, name):
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    args = re.search(r"int %s\((.*?)\);" % name, hdr, flags=re.S).group(1)
    out = []
    for a in [x.strip() for x in args.replace("\n", " ").split(",")]:
        m = re.match(r"(.*?)(\w+)$", a)
        out.append((re.sub(r"\s+", " ", m.group(1)).strip().replace(" *", "*"), m.group(2)))
    return out


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _patch(S, channels=2, voices=6, n_buses=3, rate=48000):
    p = S.Patch(rate, 64, channels)
    p.ids = S.build_p1(p)
    if voices:
        p.configure_voices(voices)
        if n_buses:
            p.set_buses(n_buses, np.arange(voices, dtype=np.intc) % n_buses)
    return p


def test_symbols_prototypes_and_argtypes(S):
    hdr = open(os.path.join(ROOT, "include", "srack_hip.h")).read()
    L = ctypes.CDLL(S.LIB_PATH)
    assert L.srack_abi_version() == 2 and S.lib.srack_abi_version() == 2
    assert re.search(r"#define SRACK_ABI_VERSION 2\b", hdr)
    assert re.search(r"#define SRACK_BUS_VCA_NPARAMS 4\b", hdr) and re.search(r"#define SRACK_BUS_VCA_NSTATE\s+6\b", hdr)
    assert re.search(r"enum \{ SRACK_BUS_VCA_OFF = 0, SRACK_BUS_VCA_CV = 1, SRACK_BUS_VCA_GATE = 2 \};", hdr)
    assert len(set(S.ABI_SYMBOLS)) == len(S.ABI_SYMBOLS)
    for name in NAMES:
        assert name in S.ABI_SYMBOLS and hasattr(L, name), name
        proto = _prototype(hdr, name)
        argtypes = getattr(S.lib, name).argtypes
        assert len(argtypes) == len(proto), name
        for (ctype, pname), at in zip(proto, argtypes):
            want = ctypes.c_void_p if pname in _DEVICE_POINTERS else _CTYPES[ctype]
            assert at is want, f"{name}: {pname} is {at}, the header says {ctype}"
    assert [n for _, n in _prototype(hdr, "srack_buses_set_vca")] == ["p", "params", "mode", "negative"]
    assert [n for _, n in _prototype(hdr, "srack_buses_get_vca")] == ["p", "params", "mode", "negative", "cap"]
    assert [n for _, n in _prototype(hdr, "srack_buses_reset_vca")] == ["p"]
    assert [n for _, n in _prototype(hdr, "srack_buses_vca_state")] == ["p", "state", "cap"]
    assert [n for _, n in _prototype(hdr, "srack_buses_vca")] == ["p", "n_samples", "d_rows", "row_channels", "d_ctl", "d_out", "d_env", "stream"]


def test_python_wrappers_and_constants(S):
    assert list(inspect.signature(S.Patch.set_bus_vca).parameters) == ["self", "params", "mode", "negative"]
    assert list(inspect.signature(S.Patch.get_bus_vca).parameters) == ["self"]
    assert list(inspect.signature(S.Patch.reset_bus_vca).parameters) == ["self"]
    assert list(inspect.signature(S.Patch.bus_vca_state).parameters) == ["self"]
    assert list(inspect.signature(S.Patch.bus_vca_raw).parameters) == ["self", "n_samples", "d_rows", "row_channels", "d_ctl", "d_out", "d_env", "stream"]
    assert list(inspect.signature(S.Patch.bus_vca).parameters) == ["self", "rows", "ctl", "in_place", "want_env"]
    assert (S.BUS_VCA_NPARAMS, S.BUS_VCA_NSTATE) == (4, 6) and tuple(S.BUS_VCA_DEFAULTS) == tuple(DEFAULTS) == tuple(R.DEFAULTS)
    assert (S.BUS_VCA_OFF, S.BUS_VCA_CV, S.BUS_VCA_GATE) == (0, 1, 2) == (R.OFF, R.CV, R.GATE)
    assert S.BUS_VCA_NPARAMS == S.ADSR_R_SEC - S.ADSR_A_SEC + 1 and S.BUS_VCA_NSTATE == R.NSTATE == S.ADSR_GATE_LAST - S.ADSR_PHASE + 1
    assert (S.ADSR_MODE_ATTACK, S.ADSR_MODE_DECAY, S.ADSR_MODE_SUSTAIN, S.ADSR_MODE_RELEASE, S.ADSR_MODE_NONE) == (R.ATTACK, R.DECAY, R.SUSTAIN, R.RELEASE, R.NONE)


def test_rust_and_cpp_bindings_and_documents():
    src = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hpp = open(os.path.join(ROOT, "include", "srack.hpp")).read()
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, src), name
        assert "ffi::%s(" % name in src, name
        assert name in doc, name
        assert name + "(" in hpp, name
    for fn in ("set_bus_vca", "get_bus_vca", "reset_bus_vca", "bus_vca_state", "bus_vca"):
        assert re.search(r"pub fn %s\(" % fn, src), fn
        assert re.search(r"\b%s\(" % fn, hpp), fn
    for path, what in (("README.md", "srack_buses_vca"), ("DESIGN.md", "busvca.hip.h"), ("NOTES.md", "notes/r20.md"), ("tools/README.md", "busvca_timing.py"),
                       ("profiles/README.md", "r20_busvca.json"), ("notes/r20.md", "srack_buses_vca")):
        assert what in open(os.path.join(ROOT, path)).read(), (path, what)


def test_error_codes_in_their_order_without_a_device(S):
    par = np.tile(np.array(DEFAULTS, dtype=np.float32), (3, 1))
    mo, ng = np.full(3, 2, dtype=np.intc), np.zeros(3, dtype=np.intc)
    st = np.zeros((3, 6), dtype=np.float32)
    calls = {
        "set": lambda h: S.lib.srack_buses_set_vca(h, _fp(par), _ip(mo), _ip(ng)),
        "get": lambda h: S.lib.srack_buses_get_vca(h, None, None, None, 0),
        "reset": lambda h: S.lib.srack_buses_reset_vca(h),
        "state": lambda h: S.lib.srack_buses_vca_state(h, _fp(st), 3),
        "run": lambda h: S.lib.srack_buses_vca(h, 16, 4096, 2, None, 8192, None, None),
    }
    for name, call in calls.items():  # a null handle
        assert call(None) == S.ERR_INVALID, name
    p = _patch(S, voices=0)
    for name, call in calls.items():  # before srack_voices_configure
        assert call(p.h) == S.ERR_STATE, name
        assert "voices_configure" in S.lib.srack_last_error().decode(), name
    p.configure_voices(6)
    for name, call in calls.items():  # before a bus table exists
        assert call(p.h) == S.ERR_STATE, name
        assert "set_buses" in S.lib.srack_last_error().decode(), name
    p.set_buses(3, np.arange(6, dtype=np.intc) % 3)
    assert calls["get"](p.h) == 0  # none set
    assert p.get_bus_vca() == (0, None, None, None)
    for name in ("run", "reset", "state"):  # without VCAs set — before any look at the call's own arguments
        assert calls[name](p.h) == S.ERR_STATE, name
        assert "set_vca" in S.lib.srack_last_error().decode(), name
    assert S.lib.srack_buses_vca(p.h, 0, None, 2, None, None, None, None) == S.ERR_STATE
    assert S.lib.srack_buses_vca(p.h, 16, None, 99, None, None, None, None) == S.ERR_STATE
    assert calls["set"](p.h) == S.OK
    assert calls["get"](p.h) == 3
    assert calls["reset"](p.h) == S.OK
    st[:] = 7
    assert calls["state"](p.h) == 3 and st.tolist() == [FRESH] * 3  # nothing ran: every envelope is fresh — which is not all zeros
    # srack_buses_vca's own arguments, refused before anything reaches the device (this host has none); zero samples is nothing to do
    assert S.lib.srack_buses_vca(p.h, 0, None, 99, None, None, None, None) == S.OK
    assert S.lib.srack_buses_vca(p.h, 16, None, 2, None, 8192, None, None) == S.ERR_INVALID
    assert S.lib.srack_buses_vca(p.h, 16, 4096, 2, None, None, None, None) == S.ERR_INVALID
    for rc in (0, 9, 1 << 20):
        assert S.lib.srack_buses_vca(p.h, 16, 4096, rc, None, 1 << 20, None, None) == S.ERR_INVALID, rc
        assert "row_channels" in S.lib.srack_last_error().decode()
    nbytes, rowbytes, base, far, farther = 3 * 2 * 16 * 4, 3 * 16 * 4, 1 << 20, 1 << 24, 1 << 25
    for d_in, d_out in ((base, base + 4), (base, base + nbytes - 4), (base + nbytes - 4, base), (base + 64, base)):  # a partial overlap
        assert S.lib.srack_buses_vca(p.h, 16, d_in, 2, None, d_out, None, None) == S.ERR_INVALID, (d_in, d_out)
        assert "overlaps d_rows in part" in S.lib.srack_last_error().decode()
    for d_x in (base, base + nbytes - 4, base - rowbytes + 4):  # d_ctl or d_env on d_out, in place and out of place
        for d_in in (base, far):
            assert S.lib.srack_buses_vca(p.h, 16, d_in, 2, d_x, base, None, None) == S.ERR_INVALID, (d_x, d_in)
            assert "d_ctl overlaps d_out" in S.lib.srack_last_error().decode()
            assert S.lib.srack_buses_vca(p.h, 16, d_in, 2, None, base, d_x, None) == S.ERR_INVALID, (d_x, d_in)
            assert "d_env overlaps d_out" in S.lib.srack_last_error().decode()
        # d_env on d_rows, out of place; d_env on d_ctl
        assert S.lib.srack_buses_vca(p.h, 16, base, 2, None, far, d_x, None) == S.ERR_INVALID, d_x
        assert "d_env overlaps d_rows" in S.lib.srack_last_error().decode()
    for d_env in (farther, farther + rowbytes - 4, farther - rowbytes + 4):
        assert S.lib.srack_buses_vca(p.h, 16, base, 2, farther, far, d_env, None) == S.ERR_INVALID, d_env
        assert "d_env overlaps d_ctl" in S.lib.srack_last_error().decode()
    # ... and such calls leave the setting in place and add nothing to the description
    n, a, m, g = p.get_bus_vca()
    assert n == 3 and (a == par).all() and (m == 2).all() and (g == 0).all()
    assert "busvca" not in p.info()


def test_round_trip_defaults_odd_values_and_a_bad_mode(S):
    p = _patch(S, n_buses=4, voices=8)
    p.set_bus_vca()  # NULL, NULL, NULL: the module's defaults, every bus GATE, negative off
    n, a, m, g = p.get_bus_vca()
    assert n == 4 and a.tolist() == np.array([DEFAULTS] * 4, dtype=np.float32).tolist() and m.tolist() == [2] * 4 and g.tolist() == [0] * 4
    odd = np.array([[0.1, 1.0, 0.25, 0.0], [np.nan, -0.0, np.inf, 1.0], [-np.inf, 1e-45, 3.4028235e38, -1.0], [-np.nan, 1.7, -3.0, 5e-324]], dtype=np.float32)
    odd.view(np.uint32)[3, 0] = 0xFFC12345  # a NaN with a payload
    mo, ng = np.array([2, 1, 0, 2], dtype=np.intc), np.array([1, 0, 5, -2], dtype=np.intc)
    p.set_bus_vca(odd, mo, ng)
    n, a, m, g = p.get_bus_vca()
    assert n == 4 and m.tolist() == [2, 1, 0, 2] and g.tolist() == [1, 0, 1, 1]
    np.testing.assert_array_equal(a.view(np.uint32), odd.view(np.uint32))  # bit for bit, NaN payloads and signed zeros included
    # the raw call with NULL mode and negative keeps params; a short read copies `cap` buses
    assert S.lib.srack_buses_set_vca(p.h, _fp(odd), None, None) == S.OK
    a2, m2, g2 = np.full((4, 4), 77.0, dtype=np.float32), np.full(4, 77, dtype=np.intc), np.full(4, 77, dtype=np.intc)
    assert S.lib.srack_buses_get_vca(p.h, _fp(a2), _ip(m2), _ip(g2), 2) == 4
    np.testing.assert_array_equal(a2[:2].view(np.uint32), odd[:2].view(np.uint32))
    assert (a2[2:] == 77.0).all() and m2.tolist() == [2, 2, 77, 77] and g2.tolist() == [0, 0, 77, 77]
    # a mode outside 0..2 is refused and leaves the earlier setting in place
    p.set_bus_vca(odd, mo, ng)
    for bad in (3, -1, 1 << 30):
        bm = mo.copy()
        bm[2] = bad
        assert S.lib.srack_buses_set_vca(p.h, None, _ip(bm), None) == S.ERR_INVALID, bad
        assert "mode" in S.lib.srack_last_error().decode()
    n, a, m, g = p.get_bus_vca()
    np.testing.assert_array_equal(a.view(np.uint32), odd.view(np.uint32))
    assert m.tolist() == [2, 1, 0, 2] and g.tolist() == [1, 0, 1, 1]
    # the state of every bus reads fresh, whatever its mode; the rate slot is the patch's f32 rate
    assert p.bus_vca_state().tolist() == [FRESH] * 4
    q = _patch(S, rate=44100)
    q.set_bus_vca()
    assert q.bus_vca_state().tolist() == [[0.0, 4.0, 0.0, 0.0, 44100.0, 1.0]] * 3
    assert q.get_field(q.ids["adsr"], S.ADSR_SAMPLE_RATE) == 44100.0   # what a fresh ADSR module of that patch carries


def test_lifetime_with_the_bus_table_and_the_voices(S):
    p = _patch(S, n_buses=3, voices=6)
    par = (np.arange(12, dtype=np.float32).reshape(3, 4) / 70).astype(np.float32)
    p.set_bus_vca(par, [2, 1, 0], [1, 0, 1])
    info = p.info()
    assert "busvca" not in info  # no call has run
    twin = _patch(S, n_buses=3, voices=6)
    assert twin.info() == info   # a handle that never heard of VCAs says the same
    # the same n_buses, another table: the VCAs stay
    p.set_buses(3, np.array([2, 2, 1, 1, 0, -1], dtype=np.intc), np.linspace(0, 1, 6).astype(np.float32))
    n, a, m, g = p.get_bus_vca()
    assert n == 3 and (a == par).all() and m.tolist() == [2, 1, 0] and g.tolist() == [1, 0, 1]
    # not part of the program: the description of the patch is what it was, a field edit keeps them
    assert p.info() == info
    p.set_field(p.ids["vcf"], S.VCF_RES, 0.3)
    assert p.get_bus_vca()[0] == 3
    # a bad table is refused and drops nothing
    assert S.lib.srack_voices_set_buses(p.h, 2, _ip(np.full(6, 5, dtype=np.intc)), None) == S.ERR_INVALID
    assert p.get_bus_vca()[0] == 3
    # the filters and the VCAs do not know of each other
    p.set_bus_filter()
    assert p.get_bus_vca()[0] == 3 and p.get_bus_filter()[0] == 3
    # another n_buses drops them
    p.set_buses(4, np.arange(6, dtype=np.intc) % 4)
    assert p.get_bus_vca() == (0, None, None, None)
    assert S.lib.srack_buses_vca(p.h, 16, 4096, 2, None, 1 << 20, None, None) == S.ERR_STATE
    p.set_bus_vca()
    assert p.get_bus_vca()[0] == 4
    # srack_voices_configure drops the table and with it the VCAs
    p.configure_voices(6)
    assert S.lib.srack_buses_get_vca(p.h, None, None, None, 0) == S.ERR_STATE
    p.set_buses(4, np.arange(6, dtype=np.intc) % 4)
    assert p.get_bus_vca() == (0, None, None, None)


# ---- tests/busvca_ref.py against the oracle's ADSRModule and VCAModule, bit for bit -----------------------------------------------------
BUF, NBUF = 37, 108
T = BUF * NBUF   # 3 996: the oracle renders buffer by buffer, so its state belongs to a sample count only at a buffer's end

# (a, d, s, r; the LFO's OSC_VAL; negative) and what the case is there for: the fewest samples any of the five modes holds, and the
# retriggers the gate causes from inside Attack, Decay, Sustain, Release — guards on the ORACLE's output, counted by R.retriggers
CASES = [
    ((0.0, 0.5, 0.25, 0.5), -2.87, False, None, {}),
    ((0.004, 0.003, 0.6, 0.004), -3.2, False, 579, {}),
    ((0.01, 0.003, 0.6, 0.004), -0.87, False, None, {R.ATTACK: 19}),
    ((0.0005, 0.01, 0.5, 0.01), -1.14, False, None, {R.DECAY: 16}),
    ((0.0005, 0.0005, 0.5, 0.02), -1.87, False, None, {R.RELEASE: 9}),
    ((0.0005, 0.0005, 0.5, 0.02), -1.87, True, None, {R.RELEASE: 9}),
    ((0.002, 0.002, -0.5, 0.0), -3.2, True, None, {}),
    ((0.002, 0.002, -0.5, 0.002), -3.2, False, None, {}),
]


def _oracle_pair(S, adsr, lfo_val, negative, gate=True, cuts=(NBUF,)):
    """square LFO -> ADSRModule -> VCAModule's CV, a saw on its Audio; 4 output channels: the VCA's out, the envelope, the gate, the saw.
    cuts: buffers per render.  -> (out [4][T], the ADSR's six state values after every render)"""
    o = O.OraclePatch(48000, BUF, 4)
    lfo, osc, env, amp, out = (o.add_module(m) for m in (S.MOD_OSCILLATOR, S.MOD_OSCILLATOR, S.MOD_ADSR, S.MOD_VCA, S.MOD_OUTPUT))
    o.set_field(lfo, S.OSC_VAL, lfo_val)
    o.set_field(osc, S.OSC_VAL, -1.0)
    for f, v in zip((S.ADSR_A_SEC, S.ADSR_D_SEC, S.ADSR_S_VAL, S.ADSR_R_SEC), adsr):
        o.set_field(env, f, v)
    o.set_field(amp, S.VCA_NEGATIVE, 1.0 if negative else 0.0)
    if gate:
        o.connect(lfo, S.OSC_OUT_SQUARE, env, 0)
    o.connect(osc, S.OSC_OUT_SAW, amp, 0)
    o.connect(env, 0, amp, 1)
    o.connect(amp, 0, out, 0)
    o.connect(env, 0, out, 1)
    o.connect(lfo, S.OSC_OUT_SQUARE, out, 2)
    o.connect(osc, S.OSC_OUT_SAW, out, 3)
    parts, states = [], []
    for n in cuts:
        parts.append(o.render(n * BUF))
        states.append(np.array([o.get_field(env, S.ADSR_PHASE + k) for k in range(R.NSTATE)], dtype=np.float32))
    return np.concatenate(parts, axis=1), states


def _assert_bits(got, ref, what):
    ok = R.same_bits(got, ref)
    assert ok.all(), f"{what}: {np.count_nonzero(~ok)} of {ok.size} differ, first at {tuple(np.argwhere(~ok)[0])}"


@pytest.mark.parametrize("adsr,lfo_val,negative,floor,retrig", CASES)
def test_busvca_ref_is_the_oracles_modules(S, adsr, lfo_val, negative, floor, retrig):
    out, states = _oracle_pair(S, adsr, lfo_val, negative)
    y, e, gate, saw = out
    assert out.shape == (4, T) and np.isfinite(out).all() and np.abs(saw).max() > 0.5 and (gate > 0).any() and (gate <= 0).any()
    env, st, track = R.envelope(gate[None, :], np.array([adsr], dtype=np.float32), 48000)
    # the guards, on the oracle's own output: the envelope moves, and the case visits what it is there for
    assert np.count_nonzero(e) > T // 10 and len(np.unique(e)) > 10
    counts = R.retriggers(track, gate[None, :])
    if floor is not None:
        held = [int(np.count_nonzero(track == m)) for m in range(5)]
        assert min(held) >= floor, held
    for m, k in retrig.items():
        assert counts[m] == k, counts
    if adsr[2] < 0 and negative:     # a negative sustain through an open VCA; a release of one sample (r_sec = 0)
        rel = np.flatnonzero(track[0] == R.RELEASE)
        assert np.count_nonzero((e < 0) & (y != 0)) > 100 and len(rel) == 3 and (track[0][rel - 1] == R.SUSTAIN).all() and (track[0][rel + 1] == R.NONE).all()
    if adsr[2] < 0 and not negative:  # ... and through a closed one: the output is zero on 3 361 samples, 3 360 of them for want of a positive CV
        assert np.count_nonzero(y == 0) == 3361 and np.count_nonzero(~(e > 0)) == 3360 and np.count_nonzero(saw == 0) == 4
    _assert_bits(env[0], e, "envelope")
    _assert_bits(st[0], states[0], "state")
    _assert_bits(R.vca(saw[None, :], env, [negative])[0], y, "VCA")
    other = R.vca(saw[None, :], env, [not negative])[0]
    if adsr[2] < 0:
        assert not R.same_bits(other, y).all(), "negative on and off are meant to differ"
    # ... and through the bus layout the GPU tests call
    rows = np.stack([saw, saw])[None]
    bo, be, bs, bt = R.bus_vca(rows, gate[None, :], [adsr], [R.GATE], [negative], 48000)
    _assert_bits(bo[0, 0], y, "bus_vca, channel 0")
    _assert_bits(bo[0, 1], y, "bus_vca, channel 1")
    _assert_bits(be[0], e, "bus_vca, envelope")
    _assert_bits(bs[0], states[0], "bus_vca, state")
    assert (bt == track).all()


def test_busvca_ref_with_the_gate_disconnected(S):
    """gate_in_buf is None: a fresh envelope stays in None; the state the oracle reports is the fresh one, last still true"""
    out, states = _oracle_pair(S, (0.002, 0.002, 0.5, 0.002), -3.2, True, gate=False)
    assert (out[0] == 0).all() and (out[1] == 0).all() and np.abs(out[3]).max() > 0.5
    env, st, track = R.envelope(None, np.array([[0.002, 0.002, 0.5, 0.002]], dtype=np.float32), 48000, n=T)
    _assert_bits(env[0], out[1], "envelope")
    _assert_bits(st[0], states[0], "state")
    assert (track == R.NONE).all() and st[0].tolist() == [0.0, 4.0, 0.0, 0.0, 48000.0, 0.0]   # (is_transition(&0.0) has cleared `last`)
    # from Sustain, no gate means Release: the reference's `gate_in_buf.is_none() ||`
    sus = np.array([[0.0, R.SUSTAIN, 0.5, 0.0, 48000.0, 1.0]], dtype=np.float32)
    env, st, track = R.envelope(None, np.array([[0.002, 0.002, 0.5, 0.002]], dtype=np.float32), 48000, state=sus, n=200)
    assert track[0, 0] == R.RELEASE and track[0, -1] == R.NONE and env[0, 0] == 0.5 and (np.diff(env[0, :90]) < 0).all()
    # a CV bus without a control row writes +0.0, whatever `negative` says
    rows = np.stack([out[3], out[3]])[None, :, :64]
    bo, be, bs, _ = R.bus_vca(rows, None, [R.DEFAULTS], [R.CV], [True], 48000)
    assert (bo.view(np.uint32) == 0).all() and (be.view(np.uint32) == 0).all() and bs[0].tolist() == FRESH


def test_busvca_ref_carries_the_state_as_the_oracle_does(S):
    adsr, cuts = (0.004, 0.003, 0.6, 0.004), (11, 10)
    out, states = _oracle_pair(S, adsr, -3.2, False, cuts=cuts)
    one, states_one = _oracle_pair(S, adsr, -3.2, False, cuts=(21,))
    _assert_bits(out, one, "the oracle itself, cut and uncut")
    gate, par = out[2:3], np.array([adsr], dtype=np.float32)
    n1 = cuts[0] * BUF
    e1, s1, _ = R.envelope(gate[:, :n1], par, 48000)
    _assert_bits(s1[0], states[0], "state after the first render")
    e2, s2, _ = R.envelope(gate[:, n1:], par, 48000, s1)
    _assert_bits(np.concatenate([e1, e2], axis=1)[0], out[1], "envelope over two renders")
    _assert_bits(s2[0], states[1], "state after the second render")
    _assert_bits(s2[0], states_one[0], "state, cut and uncut")
    assert not R.same_bits(s1[0], R.fresh(1, 48000)[0]).all() and not R.same_bits(s1[0], s2[0]).all()
