"""Bus filters (srack_buses_set_filter / _get_filter / _reset_filter / _filter_state / srack_buses_filter): the C ABI surface, the
bindings, the argument and lifetime rules without a GPU — and tests/busvcf_ref.py, the reference the GPU tests compare with, held to the
oracle's MoogFilterModule bit for bit."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import srack_pkg
from oracle import oracle as O
from tests import busvcf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["srack_buses_set_filter", "srack_buses_get_filter", "srack_buses_reset_filter", "srack_buses_filter_state", "srack_buses_filter"]

_CTYPES = {"srack_patch*": ctypes.c_void_p, "const srack_patch*": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int,
           "const int*": ctypes.POINTER(ctypes.c_int), "int*": ctypes.POINTER(ctypes.c_int), "const float*": ctypes.POINTER(ctypes.c_float),
           "float*": ctypes.POINTER(ctypes.c_float), "void*": ctypes.c_void_p}
_DEVICE_POINTERS = {"d_rows", "d_cv", "d_out"}  # (device addresses travel as integers: c_void_p)
DEFAULTS = [0.2, 0.5, 0.5]


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


def _patch(S, channels=2, voices=6, n_buses=3):
    p = S.Patch(48000, 64, channels)
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
    assert re.search(r"#define SRACK_BUS_FILTER_NPARAMS 3\b", hdr) and re.search(r"#define SRACK_BUS_FILTER_NSTATE\s+10\b", hdr)
    assert len(set(S.ABI_SYMBOLS)) == len(S.ABI_SYMBOLS)
    for name in NAMES:
        assert name in S.ABI_SYMBOLS and hasattr(L, name), name
        proto = _prototype(hdr, name)
        argtypes = getattr(S.lib, name).argtypes
        assert len(argtypes) == len(proto), name
        for (ctype, pname), at in zip(proto, argtypes):
            want = ctypes.c_void_p if pname in _DEVICE_POINTERS else _CTYPES[ctype]
            assert at is want, f"{name}: {pname} is {at}, the header says {ctype}"
    assert [n for _, n in _prototype(hdr, "srack_buses_set_filter")] == ["p", "params", "port", "enabled"]
    assert [n for _, n in _prototype(hdr, "srack_buses_get_filter")] == ["p", "params", "port", "enabled", "cap"]
    assert [n for _, n in _prototype(hdr, "srack_buses_reset_filter")] == ["p"]
    assert [n for _, n in _prototype(hdr, "srack_buses_filter_state")] == ["p", "state", "cap"]
    assert [n for _, n in _prototype(hdr, "srack_buses_filter")] == ["p", "n_samples", "d_rows", "row_channels", "d_cv", "d_out", "stream"]


def test_python_wrappers_and_constants(S):
    assert list(inspect.signature(S.Patch.set_bus_filter).parameters) == ["self", "params", "port", "enabled"]
    assert list(inspect.signature(S.Patch.get_bus_filter).parameters) == ["self"]
    assert list(inspect.signature(S.Patch.reset_bus_filter).parameters) == ["self"]
    assert list(inspect.signature(S.Patch.bus_filter_state).parameters) == ["self"]
    assert list(inspect.signature(S.Patch.bus_filter_raw).parameters) == ["self", "n_samples", "d_rows", "row_channels", "d_cv", "d_out", "stream"]
    assert list(inspect.signature(S.Patch.bus_filter).parameters) == ["self", "rows", "cv", "in_place"]
    assert (S.BUS_FILTER_NPARAMS, S.BUS_FILTER_NSTATE) == (3, 10) and tuple(S.BUS_FILTER_DEFAULTS) == tuple(DEFAULTS)
    assert S.BUS_FILTER_NSTATE == R.NSTATE == S.VCF_ST_RES - S.VCF_ST_F + 1


def test_rust_and_cpp_bindings_and_documents():
    src = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hpp = open(os.path.join(ROOT, "include", "srack.hpp")).read()
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, src), name
        assert "ffi::%s(" % name in src, name
        assert name in doc, name
        assert name + "(" in hpp, name
    for fn in ("set_bus_filter", "get_bus_filter", "reset_bus_filter", "bus_filter_state", "bus_filter"):
        assert re.search(r"pub fn %s\(" % fn, src), fn
        assert re.search(r"\b%s\(" % fn, hpp), fn


def test_error_codes_in_their_order_without_a_device(S):
    par = np.tile(np.array(DEFAULTS, dtype=np.float32), (3, 1))
    po, en = np.zeros(3, dtype=np.intc), np.ones(3, dtype=np.intc)
    st = np.zeros((3, 2, 10), dtype=np.float32)
    calls = {
        "set": lambda h: S.lib.srack_buses_set_filter(h, _fp(par), _ip(po), _ip(en)),
        "get": lambda h: S.lib.srack_buses_get_filter(h, None, None, None, 0),
        "reset": lambda h: S.lib.srack_buses_reset_filter(h),
        "state": lambda h: S.lib.srack_buses_filter_state(h, _fp(st), 3),
        "run": lambda h: S.lib.srack_buses_filter(h, 16, 4096, 2, None, 8192, None),
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
    assert p.get_bus_filter() == (0, None, None, None)
    for name in ("run", "reset", "state"):  # without filters set — before any look at the call's own arguments
        assert calls[name](p.h) == S.ERR_STATE, name
        assert "set_filter" in S.lib.srack_last_error().decode(), name
    assert S.lib.srack_buses_filter(p.h, 0, None, 2, None, None, None) == S.ERR_STATE
    assert S.lib.srack_buses_filter(p.h, 16, None, 99, None, None, None) == S.ERR_STATE
    assert calls["set"](p.h) == S.OK
    assert calls["get"](p.h) == 3
    assert calls["reset"](p.h) == S.OK
    st[:] = 7
    assert calls["state"](p.h) == 3 and (st == 0).all()  # nothing ran: every filter is at Default
    # srack_buses_filter's own arguments, refused before anything reaches the device (this host has none); zero samples is nothing to do
    assert S.lib.srack_buses_filter(p.h, 0, None, 99, None, None, None) == S.OK
    assert S.lib.srack_buses_filter(p.h, 16, None, 2, None, 8192, None) == S.ERR_INVALID
    assert S.lib.srack_buses_filter(p.h, 16, 4096, 2, None, None, None) == S.ERR_INVALID
    for rc in (0, 9, 1 << 20):
        assert S.lib.srack_buses_filter(p.h, 16, 4096, rc, None, 1 << 20, None) == S.ERR_INVALID, rc
        assert "row_channels" in S.lib.srack_last_error().decode()
    nbytes, cvbytes, base = 3 * 2 * 16 * 4, 3 * 16 * 4, 1 << 20
    for d_in, d_out in ((base, base + 4), (base, base + nbytes - 4), (base + nbytes - 4, base), (base + 64, base)):  # a partial overlap
        assert S.lib.srack_buses_filter(p.h, 16, d_in, 2, None, d_out, None) == S.ERR_INVALID, (d_in, d_out)
        assert "overlap" in S.lib.srack_last_error().decode()
    for d_cv in (base, base + nbytes - 4, base - cvbytes + 4):  # d_cv on d_out, in place and out of place
        for d_in in (base, 1 << 24):
            assert S.lib.srack_buses_filter(p.h, 16, d_in, 2, d_cv, base, None) == S.ERR_INVALID, (d_cv, d_in)
            assert "d_cv overlaps d_out" in S.lib.srack_last_error().decode()
    # ... and such calls leave the setting in place and add nothing to the description
    n, a, o, e = p.get_bus_filter()
    assert n == 3 and (a == par).all() and (o == 0).all() and (e == 1).all()
    assert "busvcf" not in p.info()


def test_round_trip_defaults_odd_values_and_a_bad_port(S):
    p = _patch(S, n_buses=4, voices=8)
    p.set_bus_filter()  # NULL, NULL, NULL: the module's defaults, lowpass, every bus enabled
    n, a, o, e = p.get_bus_filter()
    assert n == 4 and a.tolist() == np.array([DEFAULTS] * 4, dtype=np.float32).tolist() and o.tolist() == [0] * 4 and e.tolist() == [1] * 4
    odd = np.array([[0.1, 1.0, 0.25], [np.nan, -0.0, np.inf], [-np.inf, 1e-45, 3.4028235e38], [-np.nan, 1.7, -3.0]], dtype=np.float32)
    odd.view(np.uint32)[3, 0] = 0xFFC12345  # a NaN with a payload
    po, en = np.array([2, 1, 0, 2], dtype=np.intc), np.array([1, 0, 5, -2], dtype=np.intc)
    p.set_bus_filter(odd, po, en)
    n, a, o, e = p.get_bus_filter()
    assert n == 4 and o.tolist() == [2, 1, 0, 2] and e.tolist() == [1, 0, 1, 1]
    np.testing.assert_array_equal(a.view(np.uint32), odd.view(np.uint32))  # bit for bit, NaN payloads and signed zeros included
    # the raw call with NULL port and enabled keeps params; a short read copies `cap` buses
    assert S.lib.srack_buses_set_filter(p.h, _fp(odd), None, None) == S.OK
    a2, o2, e2 = np.full((4, 3), 77.0, dtype=np.float32), np.full(4, 77, dtype=np.intc), np.full(4, 77, dtype=np.intc)
    assert S.lib.srack_buses_get_filter(p.h, _fp(a2), _ip(o2), _ip(e2), 2) == 4
    np.testing.assert_array_equal(a2[:2].view(np.uint32), odd[:2].view(np.uint32))
    assert (a2[2:] == 77.0).all() and o2.tolist() == [0, 0, 77, 77] and e2.tolist() == [1, 1, 77, 77]
    # a port outside 0..2 is refused and leaves the earlier setting in place
    p.set_bus_filter(odd, po, en)
    for bad in (3, -1, 1 << 30):
        bp = po.copy()
        bp[2] = bad
        assert S.lib.srack_buses_set_filter(p.h, None, _ip(bp), None) == S.ERR_INVALID, bad
        assert "port" in S.lib.srack_last_error().decode()
    n, a, o, e = p.get_bus_filter()
    np.testing.assert_array_equal(a.view(np.uint32), odd.view(np.uint32))
    assert o.tolist() == [2, 1, 0, 2] and e.tolist() == [1, 0, 1, 1]


def test_lifetime_with_the_bus_table_and_the_voices(S):
    p = _patch(S, n_buses=3, voices=6)
    par = (np.arange(9, dtype=np.float32).reshape(3, 3) / 7).astype(np.float32)
    p.set_bus_filter(par, [0, 1, 2], [1, 0, 1])
    info = p.info()
    assert "busvcf" not in info  # no call has run
    twin = _patch(S, n_buses=3, voices=6)
    assert twin.info() == info   # a handle that never heard of filters says the same
    # the same n_buses, another table: the filters stay
    p.set_buses(3, np.array([2, 2, 1, 1, 0, -1], dtype=np.intc), np.linspace(0, 1, 6).astype(np.float32))
    n, a, o, e = p.get_bus_filter()
    assert n == 3 and (a == par).all() and o.tolist() == [0, 1, 2] and e.tolist() == [1, 0, 1]
    # not part of the program: the description of the patch is what it was, a field edit keeps them
    assert p.info() == info
    p.set_field(p.ids["vcf"], S.VCF_RES, 0.3)
    assert p.get_bus_filter()[0] == 3
    # a bad table is refused and drops nothing
    assert S.lib.srack_voices_set_buses(p.h, 2, _ip(np.full(6, 5, dtype=np.intc)), None) == S.ERR_INVALID
    assert p.get_bus_filter()[0] == 3
    # another n_buses drops them
    p.set_buses(4, np.arange(6, dtype=np.intc) % 4)
    assert p.get_bus_filter() == (0, None, None, None)
    assert S.lib.srack_buses_filter(p.h, 16, 4096, 2, None, 1 << 20, None) == S.ERR_STATE
    p.set_bus_filter()
    assert p.get_bus_filter()[0] == 4
    # srack_voices_configure drops the table and with it the filters
    p.configure_voices(6)
    assert S.lib.srack_buses_get_filter(p.h, None, None, None, 0) == S.ERR_STATE
    p.set_buses(4, np.arange(6, dtype=np.intc) % 4)
    assert p.get_bus_filter() == (0, None, None, None)


# ---- tests/busvcf_ref.py against the oracle's MoogFilterModule, bit for bit -------------------------------------------------------------
T, BUF = 777, 37   # 21 whole buffers: the oracle renders buffer by buffer, so its state belongs to a sample count only at their ends


def _oracle_filter(S, freq, res, exp_amt, with_cv, cuts=(T,)):
    """saw oscillator -> Math x 3 -> MoogFilterModule, an LFO's sine on its CV port (or nothing); 8 output channels: the three ports, the
    filter's input, the CV.  -> (out [8][sum(cuts)], the module's ten state values after every cut)"""
    o = O.OraclePatch(48000, BUF, 8)
    osc, lfo, gain, vcf, out = (o.add_module(m) for m in (S.MOD_OSCILLATOR, S.MOD_OSCILLATOR, S.MOD_MATH, S.MOD_MOOG_FILTER, S.MOD_OUTPUT))
    o.set_field(osc, S.OSC_VAL, -1.0)
    o.set_field(lfo, S.OSC_VAL, -2.5)
    o.set_field(gain, S.MATH_OPERATION, S.MATH_MULTIPLY)
    o.set_field(gain, S.MATH_CONSTANT, 3.0)
    for f, v in ((S.VCF_FREQ, freq), (S.VCF_RES, res), (S.VCF_EXP_AMT, exp_amt)):
        o.set_field(vcf, f, v)
    o.connect(osc, S.OSC_OUT_SAW, gain, 0)
    o.connect(gain, 0, vcf, 0)
    if with_cv:
        o.connect(lfo, S.OSC_OUT_SINE, vcf, 1)
    for port in range(3):
        o.connect(vcf, port, out, port)
    o.connect(gain, 0, out, 3)
    o.connect(lfo, S.OSC_OUT_SINE, out, 4)
    parts, states = [], []
    for n in cuts:
        parts.append(o.render(n))
        states.append(np.array([o.get_field(vcf, S.VCF_ST_F + k) for k in range(R.NSTATE)], dtype=np.float32))
    return np.concatenate(parts, axis=1), states


def _assert_bits(got, ref, what):
    ok = R.same_bits(got, ref)
    assert ok.all(), f"{what}: {np.count_nonzero(~ok)} of {ok.size} differ, first at {tuple(np.argwhere(~ok)[0])}"


@pytest.mark.parametrize("with_cv", [True, False])
@pytest.mark.parametrize("freq,res,exp_amt", [(0.2, 0.5, 0.5), (0.45, 1.7, 2.0), (0.0, 0.0, 0.5)])
def test_busvcf_ref_is_the_oracles_module(S, freq, res, exp_amt, with_cv):
    out, states = _oracle_filter(S, freq, res, exp_amt, with_cv)
    x, cv = out[3], out[4]
    assert np.isfinite(out).all() and np.count_nonzero(np.abs(x) > 1) > T // 3, "the input is meant to drive the clamps"
    assert np.abs(cv).max() > 0.5
    if (freq, res, exp_amt) == (0.45, 1.7, 2.0) and with_cv:  # the cutoff leaves [0, 0.9] on both sides, the resonance its own range
        sweep = np.float32(freq) + cv * np.float32(exp_amt)
        assert sweep.min() < 0 and sweep.max() > 0.9
    rows = np.tile(x, (3, 1))
    y, st = R.ladder(rows, np.tile(cv, (3, 1)) if with_cv else None, freq, res, exp_amt, [0, 1, 2])
    for port in range(3):
        _assert_bits(y[port], out[port], f"port {port}")
        _assert_bits(st[port], states[0], f"state, port {port}")
    if freq == 0.0 and res == 0.0 and not with_cv:
        # the reference's quirk: a fresh filter at (0, 0) never computes its coefficients — p = f = q = 0, nothing passes
        assert (out[0] == 0).all() and (out[2] == x).all() and (states[0][:3] == 0).all()
    else:
        assert np.abs(out[0]).max() > 1e-3 and not (out[0] == out[1]).all() and not (out[1] == out[2]).all() and not (out[0] == x).all()


def test_busvcf_ref_carries_the_state_as_the_oracle_does(S):
    cuts = (11 * BUF, 10 * BUF)
    out, states = _oracle_filter(S, 0.3, 0.8, 0.7, True, cuts)
    one, states_one = _oracle_filter(S, 0.3, 0.8, 0.7, True)
    _assert_bits(out, one, "the oracle itself, cut and uncut")
    x, cv = out[3:4], out[4:5]
    y1, s1 = R.ladder(x[:, :cuts[0]], cv[:, :cuts[0]], 0.3, 0.8, 0.7, 1)
    _assert_bits(s1[0], states[0], "state after the first render")
    y2, s2 = R.ladder(x[:, cuts[0]:], cv[:, cuts[0]:], 0.3, 0.8, 0.7, 1, s1)
    _assert_bits(np.concatenate([y1, y2], axis=1)[0], out[1], "bandpass over two renders")
    _assert_bits(s2[0], states[1], "state after the second render")
    _assert_bits(s2[0], states_one[0], "state, cut and uncut")
    assert np.abs(s2[0, 3:8]).max() > 1e-3 and s2[0, 8] != 0 and s2[0, 9] == np.float32(0.8)


def test_busvcf_ref_bus_layout():
    """bus_filter (what the GPU tests call): rows of disabled buses pass, further channels are zero, a disabled bus's state reads zero"""
    rng = np.random.default_rng(5)
    rows = rng.uniform(-2, 2, (3, 3, 40)).astype(np.float32)
    rows[1, 0, 3] = -0.0
    par = np.array([[0.3, 0.6, 0.5]] * 3, dtype=np.float32)
    out, st = R.bus_filter(rows, None, par, [0, 1, 2], [1, 0, 1])
    assert R.same_bits(out[1, :2], rows[1, :2]).all() and (out[:, 2] == 0).all() and (st[1] == 0).all() and (st[[0, 2]] != 0).any()
    y, s = R.ladder(rows[[0, 2], 1], None, 0.3, 0.6, 0.5, [0, 2])
    assert R.same_bits(out[[0, 2], 1], y).all() and R.same_bits(st[[0, 2], 1], s).all()
