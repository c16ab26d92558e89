"""Bus reverbs (srack_buses_set_reverb / _get_reverb / _reset_reverb / _reverb_plan / srack_buses_reverb): the C ABI surface, the
bindings, the argument and lifetime rules and the plan, without a GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import srack_pkg
from oracle.srack_numpy import _Freeverb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["srack_buses_set_reverb", "srack_buses_get_reverb", "srack_buses_reset_reverb", "srack_buses_reverb_plan", "srack_buses_reverb"]

_CTYPES = {"srack_patch*": ctypes.c_void_p, "const srack_patch*": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int,
           "const int*": ctypes.POINTER(ctypes.c_int), "int*": ctypes.POINTER(ctypes.c_int), "const double*": ctypes.POINTER(ctypes.c_double),
           "double*": ctypes.POINTER(ctypes.c_double), "void*": ctypes.c_void_p}
_DEVICE_POINTERS = {"d_bus_mix", "d_bus_fx"}  # (device addresses travel as integers: c_void_p)
DEFAULTS = [0.5, 0.0, 1.0, 0.5, 0.5, 0.0]


@pytest.fixture(scope="module")
def S():
    return srack_pkg.load()


def _prototype(hdr, name):
    args = re.search(r"int %s\((.*?)\);" % name, hdr, flags=re.S).group(1)
    out = []
    for a in [x.strip() for x in args.replace("\n", " ").split(",")]:
        m = re.match(r"(.*?)(\w+)$", a)
        out.append((re.sub(r"\s+", " ", m.group(1)).strip().replace(" *", "*"), m.group(2)))
    return out


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _patch(S, sample_rate=48000, channels=2, voices=6, n_buses=3):
    p = S.Patch(sample_rate, 64, channels)
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
    for name in NAMES:
        assert name in S.ABI_SYMBOLS and hasattr(L, name), name
        proto = _prototype(hdr, name)
        argtypes = getattr(S.lib, name).argtypes
        assert len(argtypes) == len(proto), name
        for (ctype, pname), at in zip(proto, argtypes):
            want = ctypes.c_void_p if pname in _DEVICE_POINTERS else _CTYPES[ctype]
            assert at is want, f"{name}: {pname} is {at}, the header says {ctype}"
    assert [n for _, n in _prototype(hdr, "srack_buses_set_reverb")] == ["p", "params", "enabled"]
    assert [n for _, n in _prototype(hdr, "srack_buses_get_reverb")] == ["p", "params", "enabled", "cap"]
    assert [n for _, n in _prototype(hdr, "srack_buses_reverb_plan")] == ["p", "line_lengths", "block"]
    assert [n for _, n in _prototype(hdr, "srack_buses_reverb")] == ["p", "n_samples", "d_bus_mix", "d_bus_fx", "stream"]
    # the rules the header states
    for text in ("ANY f64 is accepted", "FREEZE is zero or non-zero", "must not overlap d_bus_mix"):
        assert text in hdr, text


def test_python_wrappers(S):
    assert list(inspect.signature(S.Patch.set_bus_reverbs).parameters) == ["self", "params", "enabled"]
    assert list(inspect.signature(S.Patch.get_bus_reverbs).parameters) == ["self"]
    assert list(inspect.signature(S.Patch.reset_bus_reverbs).parameters) == ["self"]
    assert list(inspect.signature(S.Patch.bus_reverb_plan).parameters) == ["self"]
    assert list(inspect.signature(S.Patch.bus_reverb_raw).parameters) == ["self", "n_samples", "d_bus_mix", "d_bus_fx", "stream"]
    assert tuple(S.FREEVERB_DEFAULTS) == tuple(DEFAULTS)


def test_rust_and_cpp_bindings_and_documents():
    src = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hpp = open(os.path.join(ROOT, "include", "srack.hpp")).read()
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, src), name
        assert "ffi::%s(" % name in src, name
        assert name in doc, name
        assert name + "(" in hpp, name
    for fn in ("set_bus_reverbs", "get_bus_reverbs", "reset_bus_reverbs", "bus_reverb_plan", "bus_reverb"):
        assert re.search(r"pub fn %s\(" % fn, src), fn
    assert "reduce first, reverberate on the root" in doc and "srack_dist_reduce_mix" in doc


def test_error_codes_without_a_device(S):
    par = np.tile(np.array(DEFAULTS), (3, 1))
    en = np.ones(3, dtype=np.intc)
    ln, blk = np.zeros(24, dtype=np.intc), ctypes.c_int(0)
    calls = {
        "set": lambda h: S.lib.srack_buses_set_reverb(h, _dp(par), _ip(en)),
        "get": lambda h: S.lib.srack_buses_get_reverb(h, None, None, 0),
        "reset": lambda h: S.lib.srack_buses_reset_reverb(h),
        "plan": lambda h: S.lib.srack_buses_reverb_plan(h, _ip(ln), ctypes.byref(blk)),
        "run": lambda h: S.lib.srack_buses_reverb(h, 16, 4096, 8192, None),
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
    assert p.get_bus_reverbs() == (0, None, None)
    assert calls["plan"](p.h) == S.OK  # (the plan depends on the sample rate alone)
    for name in ("run", "reset"):  # without reverbs set
        assert calls[name](p.h) == S.ERR_STATE, name
        assert "set_reverb" in S.lib.srack_last_error().decode(), name
    assert calls["set"](p.h) == S.OK
    assert calls["get"](p.h) == 3
    assert calls["reset"](p.h) == S.OK
    # srack_buses_reverb's own arguments, refused before anything reaches the device (this host has none); zero samples is nothing to do
    assert S.lib.srack_buses_reverb(p.h, 0, None, None, None) == S.OK
    assert S.lib.srack_buses_reverb(p.h, 16, None, 8192, None) == S.ERR_INVALID
    assert S.lib.srack_buses_reverb(p.h, 16, 4096, None, None) == S.ERR_INVALID
    n_in, n_out = 3 * 2 * 16 * 4, 3 * 2 * 16 * 4
    for d_in, d_out in ((1 << 20, 1 << 20), (1 << 20, (1 << 20) + n_in - 4), ((1 << 20) + n_out - 4, 1 << 20), (1 << 20, (1 << 20) + 64)):
        assert S.lib.srack_buses_reverb(p.h, 16, d_in, d_out, None) == S.ERR_INVALID, (d_in, d_out)
        assert "overlap" in S.lib.srack_last_error().decode()
    # ... and such calls leave the setting in place
    n, a, e = p.get_bus_reverbs()
    assert n == 3 and (a == par).all() and (e == 1).all()


def test_round_trip_defaults_and_odd_values(S):
    p = _patch(S, n_buses=4, voices=8)
    p.set_bus_reverbs()  # NULL, NULL: the module's defaults, every bus enabled
    n, a, e = p.get_bus_reverbs()
    assert n == 4 and a.tolist() == [DEFAULTS] * 4 and e.tolist() == [1] * 4
    odd = np.array([[0.1, 1.0, 0.25, 1.0, 0.9, 0.5],
                    [np.nan, 0.0, np.inf, -np.inf, -0.0, 1e-310],
                    [2.0, -3.0, 1e300, -1e300, 5e-324, 1.7976931348623157e308],
                    [-np.nan, np.nan, 0.0, 0.5, 0.5, 7.0]])
    en = np.array([1, 0, 5, -2], dtype=np.intc)
    p.set_bus_reverbs(odd, en)
    n, a, e = p.get_bus_reverbs()
    assert n == 4 and e.tolist() == [1, 0, 1, 1]
    np.testing.assert_array_equal(a.view(np.uint64), odd.view(np.uint64))  # bit for bit, NaN payloads and signed zeros included
    # the raw call with NULL enabled keeps params, enables all; a short read copies `cap` buses
    assert S.lib.srack_buses_set_reverb(p.h, _dp(odd), None) == S.OK
    a2, e2 = np.full((4, 6), 77.0), np.full(4, 77, dtype=np.intc)
    assert S.lib.srack_buses_get_reverb(p.h, _dp(a2), _ip(e2), 2) == 4
    np.testing.assert_array_equal(a2[:2].view(np.uint64), odd[:2].view(np.uint64))
    assert (a2[2:] == 77.0).all() and e2.tolist() == [1, 1, 77, 77]
    # a bad call leaves the earlier setting in place
    assert S.lib.srack_buses_set_reverb(None, None, None) == S.ERR_INVALID
    assert S.lib.srack_buses_reverb(p.h, 8, 4096, 4096, None) == S.ERR_INVALID
    n, a, e = p.get_bus_reverbs()
    np.testing.assert_array_equal(a.view(np.uint64), odd.view(np.uint64))
    assert e.tolist() == [1, 1, 1, 1]


def test_lifetime_with_the_bus_table_and_the_voices(S):
    p = _patch(S, n_buses=3, voices=6)
    par = np.arange(18, dtype=np.float64).reshape(3, 6) / 7
    p.set_bus_reverbs(par, [1, 0, 1])
    info = p.info()
    assert "busfx" not in info  # no call has run
    # the same n_buses, another table: parameters stay
    p.set_buses(3, np.array([2, 2, 1, 1, 0, -1], dtype=np.intc), np.linspace(0, 1, 6).astype(np.float32))
    n, a, e = p.get_bus_reverbs()
    assert n == 3 and (a == par).all() and e.tolist() == [1, 0, 1]
    # not part of the program: the description of the patch is what it was, a field edit keeps them
    assert p.info() == info
    p.set_field(p.ids["vcf"], S.VCF_RES, 0.3)
    assert p.get_bus_reverbs()[0] == 3
    # a bad table is refused and drops nothing
    assert S.lib.srack_voices_set_buses(p.h, 2, _ip(np.full(6, 5, dtype=np.intc)), None) == S.ERR_INVALID
    assert p.get_bus_reverbs()[0] == 3
    # another n_buses drops parameters (and state)
    p.set_buses(4, np.arange(6, dtype=np.intc) % 4)
    assert p.get_bus_reverbs() == (0, None, None)
    assert S.lib.srack_buses_reverb(p.h, 16, 4096, 1 << 20, None) == S.ERR_STATE
    p.set_bus_reverbs()
    assert p.get_bus_reverbs()[0] == 4
    # srack_voices_configure drops the table and with it the reverbs
    p.configure_voices(6)
    assert S.lib.srack_buses_get_reverb(p.h, None, None, 0) == S.ERR_STATE
    p.set_buses(4, np.arange(6, dtype=np.intc) % 4)
    assert p.get_bus_reverbs() == (0, None, None)


def test_below_784_hz_is_unsupported(S):
    p = _patch(S, sample_rate=700)
    assert S.lib.srack_buses_set_reverb(p.h, None, None) == S.ERR_UNSUPPORTED
    assert "784" in S.lib.srack_last_error().decode()
    ln, blk = np.zeros(24, dtype=np.intc), ctypes.c_int(0)
    assert S.lib.srack_buses_reverb_plan(p.h, _ip(ln), ctypes.byref(blk)) == S.ERR_UNSUPPORTED
    assert S.lib.srack_buses_get_reverb(p.h, None, None, 0) == 0
    p = _patch(S, sample_rate=783)
    assert S.lib.srack_buses_set_reverb(p.h, None, None) == S.ERR_UNSUPPORTED


@pytest.mark.parametrize("sr", [784, 2000, 44100, 48000, 65535])
def test_plan_matches_the_reference_lines(S, sr):
    p = _patch(S, sample_rate=sr)
    ln, block = p.bus_reverb_plan()
    fv = _Freeverb(sr)
    want = [len(c.d.buf) for pair in fv.combs for c in pair] + [len(a.d.buf) for pair in fv.allpasses for a in pair]
    assert ln.tolist() == want  # line = 2 * unit + channel, combs then allpasses
    assert 1 <= block <= min(want)
    assert block == min(256, min(want))
    # either pointer may be NULL
    assert S.lib.srack_buses_reverb_plan(p.h, None, None) == S.OK
