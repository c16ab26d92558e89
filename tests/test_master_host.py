"""The master section (srack_buses_set_master / _get_master / srack_buses_master): the C ABI surface, the bindings, the argument and
lifetime rules, and the NumPy reference checked against itself — without a GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import srack_pkg
from tests import master_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["srack_buses_set_master", "srack_buses_get_master", "srack_buses_master"]

_CTYPES = {"srack_patch*": ctypes.c_void_p, "const srack_patch*": ctypes.c_void_p, "uint32_t": ctypes.c_uint32,
           "const float*": ctypes.POINTER(ctypes.c_float), "float*": ctypes.POINTER(ctypes.c_float), "void*": ctypes.c_void_p}
_DEVICE_POINTERS = {"d_rows", "d_master", "d_master_stats"}  # (device addresses travel as integers: c_void_p)


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


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _patch(S, voices=6, n_buses=3):
    p = S.Patch(48000, 64, 2)
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
    assert re.search(r"#define SRACK_MASTER_RUN\s+64\b", hdr) and re.search(r"#define SRACK_MASTER_BLOCK\s+64\b", hdr)
    assert (S.MASTER_RUN, S.MASTER_BLOCK) == (64, 64) == (R.RUN, R.BLOCK)
    for name in NAMES:
        assert name in S.ABI_SYMBOLS and hasattr(L, name), name
        proto = _prototype(hdr, name)
        argtypes = getattr(S.lib, name).argtypes
        assert len(argtypes) == len(proto), name
        for (ctype, pname), at in zip(proto, argtypes):
            want = ctypes.c_void_p if pname in _DEVICE_POINTERS else _CTYPES[ctype]
            assert at is want, f"{name}: {pname} is {at}, the header says {ctype}"
    assert [n for _, n in _prototype(hdr, "srack_buses_set_master")] == ["p", "gain"]
    assert [n for _, n in _prototype(hdr, "srack_buses_get_master")] == ["p", "gain", "cap"]
    assert [n for _, n in _prototype(hdr, "srack_buses_master")] == ["p", "n_samples", "d_rows", "row_channels", "d_master", "d_master_stats", "stream"]
    for text in ("ANY f32 gain is accepted", "part of the ABI", "must not overlap d_rows", "No floating-point atomics"):
        assert text in hdr, text


def test_python_wrappers(S):
    assert list(inspect.signature(S.Patch.set_master).parameters) == ["self", "gain"]
    assert inspect.signature(S.Patch.set_master).parameters["gain"].default is None
    assert list(inspect.signature(S.Patch.get_master).parameters) == ["self"]
    sig = inspect.signature(S.Patch.master_raw)
    assert list(sig.parameters) == ["self", "n_samples", "d_rows", "row_channels", "d_master", "d_master_stats", "stream"]
    assert sig.parameters["d_master_stats"].default is None and sig.parameters["stream"].default is None
    sig = inspect.signature(S.Patch.master)
    assert list(sig.parameters) == ["self", "rows", "stats"] and sig.parameters["stats"].default is None


def test_rust_and_cpp_bindings_and_documents():
    src = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hpp = open(os.path.join(ROOT, "include", "srack.hpp")).read()
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, src), name
        assert "ffi::%s(" % name in src, name
        assert name in doc, name
        assert name + "(" in hpp, name
    for fn in ("set_master", "get_master", "master"):
        assert re.search(r"pub fn %s\(" % fn, src), fn
    assert "take the master there" in doc and "different association" in doc


def test_error_codes_and_their_order_without_a_device(S):
    g = np.ones((3, 2), dtype=np.float32)
    calls = {
        "set": lambda h: S.lib.srack_buses_set_master(h, _fp(g)),
        "get": lambda h: S.lib.srack_buses_get_master(h, None, 0),
        "run": lambda h: S.lib.srack_buses_master(h, 16, 4096, 2, 1 << 20, None, None),
    }
    # 1: a null handle — before anything else, whatever the other arguments
    for name, call in calls.items():
        assert call(None) == S.ERR_INVALID, name
    assert S.lib.srack_buses_master(None, 0, None, 0, None, None, None) == S.ERR_INVALID
    # 2: before srack_voices_configure, then before a mix table exists — before the arguments are looked at
    p = _patch(S, voices=0)
    for name, call in calls.items():
        assert call(p.h) == S.ERR_STATE, name
        assert "voices_configure" in S.lib.srack_last_error().decode(), name
    assert S.lib.srack_buses_master(p.h, 0, None, 0, None, None, None) == S.ERR_STATE
    p.configure_voices(6)
    for name, call in calls.items():
        assert call(p.h) == S.ERR_STATE, name
        assert "set_buses" in S.lib.srack_last_error().decode(), name
    assert S.lib.srack_buses_master(p.h, 16, None, 9, None, None, None) == S.ERR_STATE
    p.set_buses(3, np.arange(6, dtype=np.intc) % 3)
    assert calls["get"](p.h) == 0 and p.get_master() is None  # none set
    # 3: zero samples is nothing to do, whatever else is wrong
    assert S.lib.srack_buses_master(p.h, 0, None, 0, None, None, None) == S.OK
    assert S.lib.srack_buses_master(p.h, 0, 4096, 99, 4096, 4, None) == S.OK
    # 4: the call's own arguments, refused before anything reaches the device (this host has none)
    assert S.lib.srack_buses_master(p.h, 16, None, 2, 1 << 20, None, None) == S.ERR_INVALID
    assert S.lib.srack_buses_master(p.h, 16, 4096, 2, None, None, None) == S.ERR_INVALID
    for rc in (0, 9, 1 << 31):
        assert S.lib.srack_buses_master(p.h, 16, 4096, rc, 1 << 20, None, None) == S.ERR_INVALID, rc
        assert "row_channels" in S.lib.srack_last_error().decode()
    assert S.lib.srack_buses_master(p.h, 16, 4096, 2, 1 << 20, (1 << 21) + 4, None) == S.ERR_INVALID
    n_in, n_out = 3 * 2 * 16 * 4, 2 * 16 * 4
    for d_in, d_out in ((1 << 20, 1 << 20), (1 << 20, (1 << 20) + n_in - 4), ((1 << 20) + n_out - 4, 1 << 20), (1 << 20, (1 << 20) + 64)):
        assert S.lib.srack_buses_master(p.h, 16, d_in, 2, d_out, None, None) == S.ERR_INVALID, (d_in, d_out)
        assert "overlap" in S.lib.srack_last_error().decode()
    # (with three row channels the rows reach further: what did not overlap with two does now)
    assert S.lib.srack_buses_master(p.h, 16, 1 << 20, 3, (1 << 20) + n_in, None, None) == S.ERR_INVALID
    # nothing ran: no note, and no gains appeared
    assert "master=" not in p.info() and p.get_master() is None


def test_round_trip_of_any_bit_pattern(S):
    p = _patch(S, n_buses=4, voices=8)
    p.set_master()  # NULL: 1.0f everywhere
    g = p.get_master()
    assert g.shape == (4, 2) and g.dtype == np.float32 and (g == 1.0).all()
    odd = np.array([0x7FC00000, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x7F7FFFFF, 0x3F800000], dtype=np.uint32).view(np.float32).reshape(4, 2)
    p.set_master(odd)
    np.testing.assert_array_equal(p.get_master().view(np.uint32), odd.view(np.uint32))  # NaN payloads, infinities, -0.0, a subnormal
    # a short read copies `cap` buses and still returns n_buses
    g2 = np.full((4, 2), 77.0, dtype=np.float32)
    assert S.lib.srack_buses_get_master(p.h, _fp(g2), 2) == 4
    np.testing.assert_array_equal(g2[:2].view(np.uint32), odd[:2].view(np.uint32))
    assert (g2[2:] == 77.0).all()
    # failed calls leave the earlier gains in place
    assert S.lib.srack_buses_set_master(None, None) == S.ERR_INVALID
    assert S.lib.srack_buses_master(p.h, 8, 4096, 2, 4096, None, None) == S.ERR_INVALID
    np.testing.assert_array_equal(p.get_master().view(np.uint32), odd.view(np.uint32))
    # NULL again: back to 1.0f
    p.set_master(None)
    assert (p.get_master() == 1.0).all()


def test_lifetime_with_the_bus_table_and_the_voices(S):
    p = _patch(S, n_buses=3, voices=6)
    g = (np.arange(6, dtype=np.float32).reshape(3, 2) - 2.5) / 3
    info = p.info()
    p.set_master(g)
    assert p.info() == info  # not part of the program; and no call has run: no note
    # a field edit (a re-flatten) keeps the gains
    p.set_field(p.ids["vcf"], S.VCF_RES, 0.3)
    np.testing.assert_array_equal(p.get_master(), g)
    assert "master=" not in p.info()
    # the same n_buses, another table: kept
    p.set_buses(3, np.array([2, 2, 1, 1, 0, -1], dtype=np.intc), np.linspace(0, 1, 6).astype(np.float32))
    np.testing.assert_array_equal(p.get_master(), g)
    # a bad table is refused and drops nothing
    assert S.lib.srack_voices_set_buses(p.h, 2, np.full(6, 5, dtype=np.intc).ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None) == S.ERR_INVALID
    np.testing.assert_array_equal(p.get_master(), g)
    # the reverbs come and go without touching them
    p.set_bus_reverbs()
    np.testing.assert_array_equal(p.get_master(), g)
    # another n_buses drops them
    p.set_buses(4, np.arange(6, dtype=np.intc) % 4)
    assert p.get_master() is None
    p.set_master()
    assert p.get_master().shape == (4, 2)
    # srack_voices_configure drops the table and with it the gains
    p.configure_voices(6)
    assert S.lib.srack_buses_get_master(p.h, None, 0) == S.ERR_STATE
    p.set_buses(4, np.arange(6, dtype=np.intc) % 4)
    assert p.get_master() is None


@pytest.mark.parametrize("n_buses", [1, 2, 63, 64, 65])
def test_reference_is_the_sequential_sum_up_to_65_buses(n_buses):
    rows, gain = R.case_inputs(n_buses, 70)
    tree, seq = R.master_tree(rows, gain), R.master_sequential(rows, gain)
    assert tree.dtype == np.float32 and tree.shape == (2, 70)
    assert np.abs(tree).max() > 1e-3 and np.count_nonzero(tree) > tree.size // 2
    np.testing.assert_array_equal(tree.view(np.uint32), seq.view(np.uint32))


def test_reference_tree_differs_from_the_sequential_sum_at_129_buses():
    rows, gain = R.case_inputs(129, 70)
    tree, seq = R.master_tree(rows, gain), R.master_sequential(rows, gain)
    assert np.count_nonzero(tree.view(np.uint32) != seq.view(np.uint32)) > 70  # (most samples: the association matters)
    np.testing.assert_allclose(tree, seq, rtol=0, atol=1e-4)  # ... and nothing else does
    # by hand, channel 0 of sample 0: two full runs and a run of one bus, then one block, then the master
    p = [np.float32(gain[b, 0]) * np.float32(rows[b, 0, 0]) for b in range(129)]
    runs = []
    for r0 in (0, 64, 128):
        s = np.float32(0.0)
        for b in range(r0, min(129, r0 + 64)):
            s = np.float32(s + p[b])
        runs.append(s)
    blk = np.float32(0.0)
    for s in runs:
        blk = np.float32(blk + s)
    assert np.float32(np.float32(0.0) + blk).view(np.uint32) == tree[0, 0].view(np.uint32)


def test_reference_edges():
    # one row channel: channel 1 is +0.0 and takes no product (an inf gain there would make NaN)
    rows, gain = R.case_inputs(5, 9, row_channels=1)
    gain[:, 1] = np.inf
    m = R.master_tree(rows, gain)
    assert (m[1].view(np.uint32) == 0).all() and np.isfinite(m[0]).all() and m[0].any()
    # a third channel is ignored
    rows3, gain = R.case_inputs(5, 9, row_channels=3)
    other = rows3.copy()
    other[:, 2] = 7.0
    np.testing.assert_array_equal(R.master_tree(rows3, gain), R.master_tree(other, gain))
    # +0.0 + -0.0 is +0.0: a master of negative zeros is positive zero, as MonoMixerModule's is
    z = np.full((3, 2, 4), -0.0, dtype=np.float32)
    assert (R.master_tree(z).view(np.uint32) == 0).all()
    # 0 * inf is NaN
    assert np.isnan(R.master_tree(np.zeros((1, 2, 3), dtype=np.float32), np.full((1, 2), np.inf, dtype=np.float32))).all()
    # the statistics: non-finite samples count and do nothing else; the buffer is continued
    x = np.array([[0.5, -2.0, np.nan, np.inf, -0.0, 1.5], [0.0, 0.0, 0.0, 0.0, 0.0, -np.inf]], dtype=np.float32)
    st = R.stats_sequential(x)
    assert st[0].tolist() == [0.0, 0.25 + 4.0 + 2.25, 1.5, 2.0, 2.0, 2.0] and st[1].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    st2 = R.stats_sequential(x, st)
    assert st2[0].tolist() == [0.0, 13.0, 1.5, 2.0, 4.0, 4.0]
    st1 = R.stats_sequential(x, st, channels=1)
    assert st1[1].tolist() == st[1].tolist() and st1[0].tolist() == st2[0].tolist()
