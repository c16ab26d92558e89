"""Mix buses (srack_voices_set_buses / srack_voices_get_buses / srack_render_buses): the C ABI surface, the bindings, the argument
checks and the host-side layout of the table for the bus fold (csrc/buses.hpp), without a GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import srack_pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["srack_voices_set_buses", "srack_voices_get_buses", "srack_render_buses"]

_CTYPES = {"srack_patch*": ctypes.c_void_p, "const srack_patch*": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int,
           "const int*": ctypes.POINTER(ctypes.c_int), "int*": ctypes.POINTER(ctypes.c_int), "const float*": ctypes.POINTER(ctypes.c_float),
           "float*": ctypes.POINTER(ctypes.c_float), "void*": ctypes.c_void_p}
_DEVICE_POINTERS = {"d_frames", "d_mix", "d_stats", "d_bus_mix"}  # (device addresses travel as integers: c_void_p)


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


def test_symbols_prototypes_and_argtypes(S):
    hdr = open(os.path.join(ROOT, "include", "srack_hip.h")).read()
    L = ctypes.CDLL(S.LIB_PATH)
    assert L.srack_abi_version() == 2
    assert re.search(r"#define SRACK_MAX_BUSES 65536\b", hdr) and re.search(r"#define SRACK_BUS_NONE\s+\(-1\)", hdr)
    assert (S.MAX_BUSES, S.BUS_NONE) == (65536, -1)
    for name in NAMES + ["srack_voices_bus_plan"]:
        assert name in S.ABI_SYMBOLS and hasattr(L, name), name
        proto = _prototype(hdr, name)
        argtypes = getattr(S.lib, name).argtypes
        assert len(argtypes) == len(proto), name
        for (ctype, pname), at in zip(proto, argtypes):
            want = ctypes.c_void_p if pname in _DEVICE_POINTERS else _CTYPES[ctype]
            assert at is want, f"{name}: {pname} is {at}, the header says {ctype}"
    assert [n for _, n in _prototype(hdr, "srack_voices_set_buses")] == ["p", "n_buses", "bus", "gain"]
    assert [n for _, n in _prototype(hdr, "srack_voices_get_buses")] == ["p", "bus", "gain", "cap"]
    assert [n for _, n in _prototype(hdr, "srack_render_buses")] == ["p", "n_samples", "d_frames", "d_mix", "d_stats", "d_bus_mix", "flags", "stream"]


def test_python_wrappers(S):
    assert list(inspect.signature(S.Patch.set_buses).parameters) == ["self", "n_buses", "bus", "gain"]
    assert list(inspect.signature(S.Patch.get_buses).parameters) == ["self"]
    assert list(inspect.signature(S.Patch.render_buses).parameters) == ["self", "n_samples", "frames", "mix", "stats", "flags"]


def test_rust_and_cpp_bindings_and_documents():
    src = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hpp = open(os.path.join(ROOT, "include", "srack.hpp")).read()
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, src), name
        assert "ffi::%s(" % name in src, name
        assert name in doc, name
        assert name + "(" in hpp, name
    assert "srack_dist_reduce_mix" in doc and "n_buses * channels * n_samples" in doc


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def test_argument_checks_without_a_device(S):
    V = 10
    bus = np.arange(V, dtype=np.intc) % 3
    gain = np.linspace(-1, 1, V).astype(np.float32)
    # a null handle
    assert S.lib.srack_voices_set_buses(None, 3, _ip(bus), _fp(gain)) == S.ERR_INVALID
    assert S.lib.srack_voices_get_buses(None, None, None, 0) == S.ERR_INVALID
    assert S.lib.srack_render_buses(None, 16, None, None, None, None, 0, None) == S.ERR_INVALID
    p = S.Patch(48000, 1024, 2)
    S.build_p1(p)
    # before the voices are configured
    assert S.lib.srack_voices_set_buses(p.h, 3, _ip(bus), _fp(gain)) == S.ERR_STATE
    assert "voices_configure" in S.lib.srack_last_error().decode()
    assert S.lib.srack_render_buses(p.h, 16, None, None, None, 4096, 0, None) == S.ERR_STATE
    p.configure_voices(V)
    assert p.get_buses() == (0, None, None)
    # a render that asks for bus mixes with no table set: refused before anything reaches the device (this host has none)
    assert S.lib.srack_render_buses(p.h, 16, None, None, None, 4096, 0, None) == S.ERR_STATE
    assert "set_buses" in S.lib.srack_last_error().decode()
    with pytest.raises(S.SrackError) as e:
        p.render_buses(16)
    assert e.value.code == S.ERR_STATE
    # a table; bad tables leave it in place
    p.set_buses(3, bus, gain)
    for n_buses, b in ((0, bus), (S.MAX_BUSES + 1, bus), (2, bus), (3, np.where(bus == 1, -2, bus).astype(np.intc)), (3, np.where(bus == 1, 3, bus).astype(np.intc))):
        assert S.lib.srack_voices_set_buses(p.h, n_buses, _ip(b), _fp(gain)) == S.ERR_INVALID, (n_buses, b)
        n, b2, g2 = p.get_buses()
        assert n == 3 and (b2 == bus).all() and (g2 == gain).all()
    p.set_buses(S.MAX_BUSES, bus, gain)  # the largest count; buses may be empty
    assert p.get_buses()[0] == S.MAX_BUSES
    # defaults: NULL bus -> every voice in bus 0, NULL gain -> 1.0; BUS_NONE and any f32 gain round-trip
    p.set_buses(1)
    n, b2, g2 = p.get_buses()
    assert n == 1 and not b2.any() and (g2 == 1.0).all()
    odd = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -3.5, 2.0, 1e38, 1.0], dtype=np.float32)
    none = np.where(bus == 2, S.BUS_NONE, bus).astype(np.intc)
    p.set_buses(2, none, odd)
    n, b2, g2 = p.get_buses()
    assert n == 2 and (b2 == none).all()
    np.testing.assert_array_equal(g2.view(np.uint32), odd.view(np.uint32))
    # a short read
    b3 = np.full(V, 77, dtype=np.intc)
    assert S.lib.srack_voices_get_buses(p.h, _ip(b3), None, 4) == 2
    assert (b3[:4] == none[:4]).all() and (b3[4:] == 77).all()
    # setting a table is not an edit of the program: the description does not change, and configure drops the table
    p.configure_voices(V)
    assert p.get_buses() == (0, None, None)
    assert S.lib.srack_render_buses(p.h, 16, None, None, None, 4096, 0, None) == S.ERR_STATE


def _check_plan(S, V, n_buses, bus):
    """every voice with a bus in exactly one segment of its own tile; a bus's segments in ascending tile order, each with a row of its
    own unless it is the bus's only one; voices in no bus nowhere"""
    p = S.Patch(48000, 1024, 2)
    S.build_p1(p)
    p.configure_voices(V)
    p.set_buses(n_buses, bus)
    seg, order = p.bus_plan()
    bus = np.asarray(bus)
    assert sorted(order.tolist()) == np.flatnonzero(bus >= 0).tolist()
    at = 0
    rows = {}
    last = (-1, -1)
    for tile, b, row, n in seg.tolist():
        assert 1 <= n <= 64 and (tile, b) > last
        last = (tile, b)
        voices = order[at:at + n]
        at += n
        assert (voices // 64 == tile).all() and (bus[voices] == b).all() and (np.diff(voices) > 0).all()
        rows.setdefault(b, []).append((tile, row))
    assert at == len(order)
    used = []
    for b, lst in rows.items():
        assert [t for t, _ in lst] == sorted(t for t, _ in lst)
        if len(lst) == 1:
            assert lst[0][1] == -1
        else:
            r = [x for _, x in lst]
            assert r == list(range(r[0], r[0] + len(r)))  # consecutive, ascending with the tile
            used += r
    assert sorted(used) == list(range(len(used)))  # scratch rows: exactly the partials that exist
    return seg


def test_table_layout_for_the_fold(S):
    rng = np.random.default_rng(5)
    # contiguous buses of 64: one segment per tile, no scratch at all
    seg = _check_plan(S, 4096, 64, np.arange(4096) // 64)
    assert len(seg) == 64 and (seg[:, 2] == -1).all()
    # v mod n: every tile holds every bus once
    seg = _check_plan(S, 1000, 64, np.arange(1000) % 64)
    assert len(seg) == 1000
    _check_plan(S, 257, 7, np.arange(257) % 7)
    _check_plan(S, 1, 1, np.zeros(1, dtype=int))
    _check_plan(S, 20, 20, rng.permutation(20))
    # random, with voices in no bus and empty buses
    for V, n in ((4097, 64), (300, 1), (300, 300), (1000, 7)):
        b = rng.integers(0, max(1, n - n // 4), V)
        b[rng.random(V) < 0.2] = S.BUS_NONE
        _check_plan(S, V, n, b)
    # nobody in any bus
    seg = _check_plan(S, 100, 3, np.full(100, S.BUS_NONE))
    assert len(seg) == 0
