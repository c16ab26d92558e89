"""Bus oscillators (srack_buses_set_osc / _get_osc / _reset_osc / _osc_state / srack_buses_osc): the C ABI surface, the bindings, the
argument and lifetime rules without a GPU — and tests/busosc_ref.py, the reference the GPU tests compare with, held to the reference's own
unit test and to a planned render of the same three modules."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import srack_pkg
from oracle import oracle as O
from tests import busosc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["srack_buses_set_osc", "srack_buses_get_osc", "srack_buses_reset_osc", "srack_buses_osc_state", "srack_buses_osc"]

_CTYPES = {"srack_patch*": ctypes.c_void_p, "const srack_patch*": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int,
           "const int*": ctypes.POINTER(ctypes.c_int), "int*": ctypes.POINTER(ctypes.c_int), "const float*": ctypes.POINTER(ctypes.c_float),
           "float*": ctypes.POINTER(ctypes.c_float), "const double*": ctypes.POINTER(ctypes.c_double), "double*": ctypes.POINTER(ctypes.c_double),
           "void*": ctypes.c_void_p}
_DEVICE_POINTERS = {"d_cv", "d_sync", "d_out"}  # (device addresses travel as integers: c_void_p)
DEFAULTS = [0.0, 1.0, 0.0]
FRESH = [0.0, 1.0]


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


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _patch(S, channels=2, voices=6, n_buses=3, rate=48000):
    p = S.Patch(rate, 64, channels)
    p.ids = S.build_p1(p)
    if voices:
        p.configure_voices(voices)
        if n_buses:
            p.set_buses(n_buses, np.arange(voices, dtype=np.intc) % n_buses)
    return p


def _assert_bits(got, ref, what):
    ok = R.same_bits(got, ref)
    assert ok.all(), f"{what}: {np.count_nonzero(~ok)} of {ok.size} differ, first at {tuple(np.argwhere(~ok)[0])}"


def test_symbols_prototypes_and_argtypes(S):
    hdr = open(os.path.join(ROOT, "include", "srack_hip.h")).read()
    L = ctypes.CDLL(S.LIB_PATH)
    assert L.srack_abi_version() == 2 and S.lib.srack_abi_version() == 2
    assert re.search(r"#define SRACK_ABI_VERSION 2\b", hdr)
    assert re.search(r"#define SRACK_BUS_OSC_NPARAMS 3\b", hdr) and re.search(r"#define SRACK_BUS_OSC_NSTATE\s+2\b", hdr)
    assert re.search(r"enum \{ SRACK_BUS_OSC_VAL = 0, SRACK_BUS_OSC_DEPTH = 1, SRACK_BUS_OSC_OFFSET = 2 \};", hdr)
    assert "comes out as +0.0" in hdr  # the Math operations always run: said in the header
    assert len(set(S.ABI_SYMBOLS)) == len(S.ABI_SYMBOLS)
    for name in NAMES:
        assert name in S.ABI_SYMBOLS and hasattr(L, name), name
        proto = _prototype(hdr, name)
        argtypes = getattr(S.lib, name).argtypes
        assert len(argtypes) == len(proto), name
        for (ctype, pname), at in zip(proto, argtypes):
            want = ctypes.c_void_p if pname in _DEVICE_POINTERS else _CTYPES[ctype]
            assert at is want, f"{name}: {pname} is {at}, the header says {ctype}"
    assert [n for _, n in _prototype(hdr, "srack_buses_set_osc")] == ["p", "params", "port", "antialiasing", "enabled"]
    assert [n for _, n in _prototype(hdr, "srack_buses_get_osc")] == ["p", "params", "port", "antialiasing", "enabled", "cap"]
    assert [n for _, n in _prototype(hdr, "srack_buses_reset_osc")] == ["p", "pos"]
    assert [n for _, n in _prototype(hdr, "srack_buses_osc_state")] == ["p", "state", "cap"]
    assert [n for _, n in _prototype(hdr, "srack_buses_osc")] == ["p", "n_samples", "d_cv", "d_sync", "d_out", "stream"]


def test_python_wrappers_and_constants(S):
    assert list(inspect.signature(S.Patch.set_bus_osc).parameters) == ["self", "params", "port", "antialiasing", "enabled"]
    assert list(inspect.signature(S.Patch.get_bus_osc).parameters) == ["self"]
    assert list(inspect.signature(S.Patch.reset_bus_osc).parameters) == ["self", "pos"]
    assert list(inspect.signature(S.Patch.bus_osc_state).parameters) == ["self"]
    assert list(inspect.signature(S.Patch.bus_osc_raw).parameters) == ["self", "n_samples", "d_cv", "d_sync", "d_out", "stream"]
    assert list(inspect.signature(S.Patch.bus_osc).parameters) == ["self", "n_samples", "cv", "sync"]
    assert (S.BUS_OSC_NPARAMS, S.BUS_OSC_NSTATE) == (3, 2) == (R.NPARAMS, R.NSTATE)
    assert tuple(S.BUS_OSC_DEFAULTS) == tuple(DEFAULTS) == tuple(R.DEFAULTS)
    assert (S.BUS_OSC_VAL, S.BUS_OSC_DEPTH, S.BUS_OSC_OFFSET) == (0, 1, 2)
    assert (S.OSC_OUT_SINE, S.OSC_OUT_SQUARE, S.OSC_OUT_SAW) == (R.SINE, R.SQUARE, R.SAW)
    assert S.BUS_OSC_NSTATE == S.OSC_SYNC_LAST - S.OSC_POS + 1


def test_rust_and_cpp_bindings_and_documents():
    src = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hpp = open(os.path.join(ROOT, "include", "srack.hpp")).read()
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, src), name
        assert "ffi::%s(" % name in src, name
        assert name in doc, name
        assert name + "(" in hpp, name
    for fn in ("set_bus_osc", "get_bus_osc", "reset_bus_osc", "bus_osc_state", "bus_osc"):
        assert re.search(r"pub fn %s\(" % fn, src), fn
        assert re.search(r"\b%s\(" % fn, hpp), fn
    for path, what in (("README.md", "srack_buses_osc"), ("DESIGN.md", "busosc.hip.h"), ("NOTES.md", "notes/r32.md"), ("tools/README.md", "busosc_timing.py"),
                       ("notes/r32.md", "srack_buses_osc"), ("s-rack_amd/csrc/Makefile", "busosc.hip")):
        assert what in open(os.path.join(ROOT, path)).read(), (path, what)
    assert os.path.exists(os.path.join(ROOT, "tools", "busosc_timing.py"))


def test_error_codes_in_their_order_without_a_device(S):
    par = np.tile(np.array(DEFAULTS, dtype=np.float32), (3, 1))
    po, aa, en = np.zeros(3, dtype=np.intc), np.ones(3, dtype=np.intc), np.ones(3, dtype=np.intc)
    st = np.zeros((3, 2), dtype=np.float64)
    calls = {
        "set": lambda h: S.lib.srack_buses_set_osc(h, _fp(par), _ip(po), _ip(aa), _ip(en)),
        "get": lambda h: S.lib.srack_buses_get_osc(h, None, None, None, None, 0),
        "reset": lambda h: S.lib.srack_buses_reset_osc(h, None),
        "state": lambda h: S.lib.srack_buses_osc_state(h, _dp(st), 3),
        "run": lambda h: S.lib.srack_buses_osc(h, 16, None, None, 8192, None),
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
    assert p.get_bus_osc() == (0, None, None, None, None)
    for name in ("run", "reset", "state"):  # without oscillators set — before any look at the call's own arguments
        assert calls[name](p.h) == S.ERR_STATE, name
        assert "set_osc" in S.lib.srack_last_error().decode(), name
    assert S.lib.srack_buses_osc(p.h, 0, None, None, None, None) == S.ERR_STATE
    assert S.lib.srack_buses_osc(p.h, 16, None, None, None, None) == S.ERR_STATE
    bad = np.array([0.0, np.nan, 0.5])
    assert S.lib.srack_buses_reset_osc(p.h, _dp(bad)) == S.ERR_STATE  # (not INVALID: the order)
    assert calls["set"](p.h) == S.OK
    assert calls["get"](p.h) == 3
    assert calls["reset"](p.h) == S.OK
    st[:] = 7
    assert calls["state"](p.h) == 3 and st.tolist() == [FRESH] * 3  # nothing ran: every oscillator is fresh — which is not all zeros
    # srack_buses_osc's own arguments, refused before anything reaches the device (this host has none); zero samples is nothing to do
    assert S.lib.srack_buses_osc(p.h, 0, None, None, None, None) == S.OK
    assert S.lib.srack_buses_osc(p.h, 0, 4096, 4096, 4096, None) == S.OK
    assert S.lib.srack_buses_osc(p.h, 16, None, None, None, None) == S.ERR_INVALID
    assert "d_out" in S.lib.srack_last_error().decode()
    assert S.lib.srack_buses_osc(p.h, 16, 4096, 8192, None, None) == S.ERR_INVALID
    rowbytes, base, far = 3 * 16 * 4, 1 << 20, 1 << 24
    for d_x in (base, base + rowbytes - 4, base - rowbytes + 4):  # d_cv or d_sync on d_out
        assert S.lib.srack_buses_osc(p.h, 16, d_x, None, base, None) == S.ERR_INVALID, d_x
        assert "d_cv overlaps d_out" in S.lib.srack_last_error().decode()
        assert S.lib.srack_buses_osc(p.h, 16, None, d_x, base, None) == S.ERR_INVALID, d_x
        assert "d_sync overlaps d_out" in S.lib.srack_last_error().decode()
        assert S.lib.srack_buses_osc(p.h, 16, far, d_x, base, None) == S.ERR_INVALID, d_x
        assert "d_sync overlaps d_out" in S.lib.srack_last_error().decode()
    # ... and such calls leave the setting in place and add nothing to the description
    n, a, m, g, e = p.get_bus_osc()
    assert n == 3 and (a == par).all() and (m == 0).all() and (g == 1).all() and (e == 1).all()
    assert "busosc" not in p.info()


def test_round_trip_defaults_odd_values_and_a_bad_port(S):
    p = _patch(S, n_buses=4, voices=8)
    p.set_bus_osc()  # NULL x 4: 0, 1, 0; sine; antialiasing on; every bus
    n, a, po, aa, en = p.get_bus_osc()
    assert n == 4 and a.tolist() == np.array([DEFAULTS] * 4, dtype=np.float32).tolist()
    assert po.tolist() == [0] * 4 and aa.tolist() == [1] * 4 and en.tolist() == [1] * 4
    odd = np.array([[0.1, 1.0, 0.25], [np.nan, -0.0, np.inf], [-np.inf, 1e-45, 3.4028235e38], [-np.nan, 2000.0, -3.0]], dtype=np.float32)
    odd.view(np.uint32)[3, 0] = 0xFFC12345  # a NaN with a payload
    ports, flags, on = np.array([2, 1, 0, 2], dtype=np.intc), np.array([1, 0, 5, -2], dtype=np.intc), np.array([7, 1, 0, -1], dtype=np.intc)
    p.set_bus_osc(odd, ports, flags, on)
    n, a, po, aa, en = p.get_bus_osc()
    assert n == 4 and po.tolist() == [2, 1, 0, 2] and aa.tolist() == [1, 0, 1, 1] and en.tolist() == [1, 1, 0, 1]
    np.testing.assert_array_equal(a.view(np.uint32), odd.view(np.uint32))  # bit for bit, NaN payloads and signed zeros included
    # the raw call with NULL port, flags and enabled keeps params; a short read copies `cap` buses
    assert S.lib.srack_buses_set_osc(p.h, _fp(odd), None, None, None) == S.OK
    a2, x2, y2, z2 = np.full((4, 3), 77.0, dtype=np.float32), np.full(4, 77, dtype=np.intc), np.full(4, 77, dtype=np.intc), np.full(4, 77, dtype=np.intc)
    assert S.lib.srack_buses_get_osc(p.h, _fp(a2), _ip(x2), _ip(y2), _ip(z2), 2) == 4
    np.testing.assert_array_equal(a2[:2].view(np.uint32), odd[:2].view(np.uint32))
    assert (a2[2:] == 77.0).all() and x2.tolist() == [0, 0, 77, 77] and y2.tolist() == [1, 1, 77, 77] and z2.tolist() == [1, 1, 77, 77]
    # a port outside 0..2 is refused and leaves the earlier setting in place
    p.set_bus_osc(odd, ports, flags, on)
    for bad in (3, -1, 1 << 30):
        bp = ports.copy()
        bp[2] = bad
        assert S.lib.srack_buses_set_osc(p.h, None, _ip(bp), None, None) == S.ERR_INVALID, bad
        assert "port" in S.lib.srack_last_error().decode()
    n, a, po, aa, en = p.get_bus_osc()
    np.testing.assert_array_equal(a.view(np.uint32), odd.view(np.uint32))
    assert po.tolist() == [2, 1, 0, 2] and aa.tolist() == [1, 0, 1, 1] and en.tolist() == [1, 1, 0, 1]
    # the state of every bus reads fresh, enabled or not
    assert p.bus_osc_state().tolist() == [FRESH] * 4


def test_reset_takes_phases_in_0_1_and_nothing_else(S):
    p = _patch(S, n_buses=4, voices=8)
    p.set_bus_osc(enabled=[1, 1, 0, 1])
    good = np.array([0.0, 0.25, 0.75, 1.0 - 2.0 ** -53])
    p.reset_bus_osc(good)
    st = p.bus_osc_state()
    assert st[:, 0].tolist() == [0.0, 0.25, 0.0, 1.0 - 2.0 ** -53]  # (the disabled bus holds the fresh state)
    assert st[:, 1].tolist() == [1.0] * 4                          # last is true, as after new()
    # 1.0, a negative number, -0.0 (no `pos %= 1.0` of non-negative numbers makes one, and its wrap is not +0.0's), NaN, 2.5, +-inf: refused,
    # on a disabled bus as well, and nothing is reset
    for bad in (1.0, -1e-300, -0.0, np.nan, 2.5, np.inf, -np.inf):
        for at in (0, 2, 3):
            ph = np.array([0.5, 0.5, 0.5, 0.5])
            ph[at] = bad
            assert S.lib.srack_buses_reset_osc(p.h, _dp(ph)) == S.ERR_INVALID, (bad, at)
            assert "phase" in S.lib.srack_last_error().decode()
            assert R.same_state(p.bus_osc_state(), st).all(), (bad, at)
    # the sliders keep the phases; a bus that becomes enabled starts fresh, one that leaves drops its phase
    p.set_bus_osc(np.tile(np.array([-8.0, 2.0, 1.0], dtype=np.float32), (4, 1)), [1, 1, 1, 1], [0, 0, 0, 0], [1, 0, 1, 1])
    assert p.bus_osc_state()[:, 0].tolist() == [0.0, 0.0, 0.0, 1.0 - 2.0 ** -53]
    p.set_bus_osc()
    assert p.bus_osc_state()[:, 0].tolist() == [0.0, 0.0, 0.0, 1.0 - 2.0 ** -53]
    p.reset_bus_osc()
    assert p.bus_osc_state().tolist() == [FRESH] * 4


def test_lifetime_with_the_bus_table_and_the_voices(S):
    p = _patch(S, n_buses=3, voices=6)
    par = (np.arange(9, dtype=np.float32).reshape(3, 3) / 7).astype(np.float32)
    p.set_bus_osc(par, [2, 1, 0], [1, 0, 1], [1, 1, 0])
    p.reset_bus_osc([0.125, 0.5, 0.25])
    info = p.info()
    assert "busosc" not in info  # no call has run
    twin = _patch(S, n_buses=3, voices=6)
    assert twin.info() == info   # a handle that never heard of the stage says the same
    # the same n_buses, another table: the oscillators stay, phases included
    p.set_buses(3, np.array([2, 2, 1, 1, 0, -1], dtype=np.intc), np.linspace(0, 1, 6).astype(np.float32))
    n, a, po, aa, en = p.get_bus_osc()
    assert n == 3 and (a == par).all() and po.tolist() == [2, 1, 0] and aa.tolist() == [1, 0, 1] and en.tolist() == [1, 1, 0]
    assert p.bus_osc_state().tolist() == [[0.125, 1.0], [0.5, 1.0], [0.0, 1.0]]
    # not part of the program: the description of the patch is what it was, a field edit keeps them
    assert p.info() == info
    p.set_field(p.ids["vcf"], S.VCF_RES, 0.3)
    assert p.get_bus_osc()[0] == 3 and p.bus_osc_state()[0].tolist() == [0.125, 1.0]
    # a bad table is refused and drops nothing
    assert S.lib.srack_voices_set_buses(p.h, 2, _ip(np.full(6, 5, dtype=np.intc)), None) == S.ERR_INVALID
    assert p.get_bus_osc()[0] == 3
    # the stages do not know of each other
    p.set_bus_vca()
    p.set_bus_filter()
    assert p.get_bus_osc()[0] == 3 and p.get_bus_vca()[0] == 3 and p.get_bus_filter()[0] == 3
    # another n_buses drops them
    p.set_buses(4, np.arange(6, dtype=np.intc) % 4)
    assert p.get_bus_osc() == (0, None, None, None, None)
    assert S.lib.srack_buses_osc(p.h, 16, None, None, 1 << 20, None) == S.ERR_STATE
    p.set_bus_osc()
    assert p.get_bus_osc()[0] == 4 and p.bus_osc_state().tolist() == [FRESH] * 4
    # srack_voices_configure drops the table and with it the oscillators
    p.configure_voices(6)
    assert S.lib.srack_buses_get_osc(p.h, None, None, None, None, 0) == S.ERR_STATE
    p.set_buses(4, np.arange(6, dtype=np.intc) % 4)
    assert p.get_bus_osc() == (0, None, None, None, None)


# ---- tests/busosc_ref.py held to the reference ---------------------------------------------------------------------------------------
def test_busosc_ref_reproduces_the_references_produces_440():
    """oscillator.rs's own unit test: rate 1760, val 0 -> a 440 Hz sine is 0, ~1, ~0, ~-1 per buffer of 4, and carries on smoothly"""
    par = np.array([DEFAULTS], dtype=np.float32)
    out, st = R.bus_osc(None, None, par, [R.SINE], None, None, 1760, n=4)
    assert out[0, 0] == 0.0 and abs(out[0, 1] - 1.0) < 1e-6 and abs(out[0, 2]) < 1e-6 and abs(out[0, 3] + 1.0) < 1e-6
    out2, st2 = R.bus_osc(None, None, par, [R.SINE], None, None, 1760, state=st, n=4)
    assert abs(out2[0, 0]) < 1e-6 and abs(out2[0, 1] - 1.0) < 1e-6 and abs(out2[0, 2]) < 1e-6 and abs(out2[0, 3] + 1.0) < 1e-6
    assert st[0].tolist() == [0.0, 0.0] and st2[0].tolist() == [0.0, 0.0]   # four quarter steps wrap exactly; no sync: `last` fell


def _planned(S, rate, buf, n_buf, val, depth, offset, port, aa, cuts=None):
    """the same three modules wired as a patch and rendered through plan_execution: -> (row [T], the oscillator's (pos, last) per render)"""
    o = O.OraclePatch(rate, buf, 1)
    osc, mul, add, out = (o.add_module(m) for m in (S.MOD_OSCILLATOR, S.MOD_MATH, S.MOD_MATH, S.MOD_OUTPUT))
    o.set_field(osc, S.OSC_VAL, val)
    o.set_field(osc, S.OSC_ANTIALIASING, 1.0 if aa else 0.0)
    o.set_field(mul, S.MATH_OPERATION, S.MATH_MULTIPLY)
    o.set_field(mul, S.MATH_CONSTANT, depth)
    o.set_field(add, S.MATH_OPERATION, S.MATH_ADD)
    o.set_field(add, S.MATH_CONSTANT, offset)
    o.connect(osc, port, mul, 0)
    o.connect(mul, 0, add, 0)
    o.connect(add, 0, out, 0)
    parts, states = [], []
    for n in cuts or (n_buf,):
        parts.append(o.render(n * buf)[0])
        states.append((o.get_field(osc, S.OSC_POS), o.get_field(osc, S.OSC_SYNC_LAST)))
    return np.concatenate(parts), states


@pytest.mark.parametrize("port", [R.SINE, R.SQUARE, R.SAW])
@pytest.mark.parametrize("aa", [True, False])
def test_busosc_ref_is_a_planned_render_of_the_three_modules(S, port, aa):
    rate, buf, n_buf, val, depth, offset = 48000, 37, 27, 1.37, 0.3, -0.125
    row, states = _planned(S, rate, buf, n_buf, val, depth, offset, port, aa)
    assert np.isfinite(row).all() and len(np.unique(row)) > (1 if port == R.SQUARE and not aa else 50)
    out, st = R.bus_osc(None, None, [[val, depth, offset]], [port], [aa], None, rate, n=buf * n_buf)
    _assert_bits(out[0], row, "row")
    assert R.same_state(st[0], states[0]).all(), (st, states)
    assert 0.0 < st[0, 0] < 1.0 and st[0, 1] == 0.0
    # ... and it is the same cut and uncut, the oracle's and this file's
    cut_row, cut_states = _planned(S, rate, buf, n_buf, val, depth, offset, port, aa, cuts=(11, 16))
    _assert_bits(cut_row, row, "the oracle itself, cut and uncut")
    n1 = 11 * buf
    o1, s1 = R.bus_osc(None, None, [[val, depth, offset]], [port], [aa], None, rate, n=n1)
    o2, s2 = R.bus_osc(None, None, [[val, depth, offset]], [port], [aa], None, rate, state=s1, n=buf * n_buf - n1)
    _assert_bits(np.concatenate([o1, o2], axis=1)[0], row, "cut")
    assert R.same_state(s1[0], cut_states[0]).all() and R.same_state(s2[0], cut_states[1]).all() and R.same_state(s2, st).all()


def test_busosc_ref_rows_ports_and_the_disabled(S):
    """CV and sync rows reach the oscillator; a row of +0.0 is the unconnected CV port bit for bit; defaults turn -0.0 into +0.0"""
    T, rate = 200, 48000
    rng = np.random.default_rng(5)
    cv = np.repeat(rng.uniform(-1, 1, (3, T // 20)).astype(np.float32), 20, axis=1)
    sync = (np.arange(T)[None, :] % np.array([[50], [37], [64]]) < 9).astype(np.float32)
    par = np.array([[1.5, 1.0, 0.0], [1.0, 0.5, 0.25], [2.0, -2.0, 1.0]], dtype=np.float32)
    out, st = R.bus_osc(cv, sync, par, [R.SINE, R.SQUARE, R.SAW], [1, 1, 0], [1, 0, 1], rate)
    assert (out[1].view(np.uint32) == 0).all() and st[1].tolist() == FRESH
    assert len(np.unique(out[0])) > 50 and len(np.unique(out[2])) > 50
    free, _ = R.bus_osc(cv, None, par, [R.SINE, R.SQUARE, R.SAW], [1, 1, 0], [1, 0, 1], rate)
    assert not R.same_bits(free[0], out[0]).all() and R.same_bits(free[0, :50], out[0, :50]).all()  # the first gate is high at sample 0: no reset until 50
    flat, _ = R.bus_osc(None, sync, par, [R.SINE, R.SQUARE, R.SAW], [1, 1, 0], [1, 0, 1], rate)
    zero, _ = R.bus_osc(np.zeros_like(cv), sync, par, [R.SINE, R.SQUARE, R.SAW], [1, 1, 0], [1, 0, 1], rate)
    _assert_bits(flat, zero, "CV unconnected against a row of +0.0")
    assert not R.same_bits(flat[0], out[0]).all()
    # the Math operations always run: a standing phase's sine, +0.0, times -1 is -0.0; plus OFFSET +0.0 it is +0.0, plus -0.0 it stays -0.0
    neg, _ = R.bus_osc(None, None, [[-2000.0, -1.0, 0.0], [-2000.0, -1.0, -0.0]], [R.SINE, R.SINE], None, None, rate, n=4)
    assert (neg[0].view(np.uint32) == 0).all() and (neg[1].view(np.uint32) == 0x80000000).all()
