"""The bus sends (srack_buses_set_sends / _get_sends / _send_plan / srack_buses_send): the C ABI surface, the bindings, the argument and
lifetime rules, the plan, and the NumPy reference checked against itself — without a GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import srack_pkg
from tests import master_ref as M
from tests import sends_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["srack_buses_set_sends", "srack_buses_get_sends", "srack_buses_send_plan", "srack_buses_send"]

_CTYPES = {"srack_patch*": ctypes.c_void_p, "const srack_patch*": ctypes.c_void_p, "uint32_t": ctypes.c_uint32,
           "const float*": ctypes.POINTER(ctypes.c_float), "float*": ctypes.POINTER(ctypes.c_float),
           "const int*": ctypes.POINTER(ctypes.c_int), "int*": ctypes.POINTER(ctypes.c_int), "void*": ctypes.c_void_p}
_DEVICE_POINTERS = {"d_rows", "d_out"}  # (device addresses travel as integers: c_void_p)


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


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


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


def _same_sends(got, src, dst, gain, through):
    assert got is not None
    np.testing.assert_array_equal(got[0], src)
    np.testing.assert_array_equal(got[1], dst)
    np.testing.assert_array_equal(got[2].view(np.uint32), np.asarray(gain, dtype=np.float32).view(np.uint32))
    np.testing.assert_array_equal(got[3].view(np.uint32), np.asarray(through, dtype=np.float32).view(np.uint32))


def test_symbols_prototypes_and_argtypes(S):
    hdr = open(os.path.join(ROOT, "include", "srack_hip.h")).read()
    L = ctypes.CDLL(S.LIB_PATH)
    assert L.srack_abi_version() == 2 and S.lib.srack_abi_version() == 2
    assert re.search(r"#define SRACK_ABI_VERSION 2\b", hdr)
    assert re.search(r"#define SRACK_MAX_SENDS\s+1048576\b", hdr) and S.MAX_SENDS == 1048576
    assert len(set(S.ABI_SYMBOLS)) == len(S.ABI_SYMBOLS)
    for name in NAMES:
        assert name in S.ABI_SYMBOLS and hasattr(L, name), name
        proto = _prototype(hdr, name)
        argtypes = getattr(S.lib, name).argtypes
        assert len(argtypes) == len(proto), name
        for (ctype, pname), at in zip(proto, argtypes):
            want = ctypes.c_void_p if pname in _DEVICE_POINTERS else _CTYPES[ctype]
            assert at is want, f"{name}: {pname} is {at}, the header says {ctype}"
    assert [n for _, n in _prototype(hdr, "srack_buses_set_sends")] == ["p", "n_sends", "src", "dst", "gain", "through"]
    assert [n for _, n in _prototype(hdr, "srack_buses_get_sends")] == ["p", "src", "dst", "gain", "cap", "through", "through_cap"]
    assert [n for _, n in _prototype(hdr, "srack_buses_send_plan")] == ["p", "n_terms", "bus_cap", "order", "order_cap"]
    assert [n for _, n in _prototype(hdr, "srack_buses_send")] == ["p", "n_samples", "d_rows", "row_channels", "d_out", "stream"]
    for text in ("a stable grouping", "part of the ABI", "never the output", "Must not overlap d_rows", "No floating-point atomics",
                 "sends on the root", "another association"):
        assert text in hdr, text


def test_python_wrappers(S):
    sig = inspect.signature(S.Patch.set_sends)
    assert list(sig.parameters) == ["self", "src", "dst", "gain", "through"]
    assert sig.parameters["gain"].default is None and sig.parameters["through"].default is None
    assert list(inspect.signature(S.Patch.get_sends).parameters) == ["self"]
    assert list(inspect.signature(S.Patch.send_plan).parameters) == ["self"]
    sig = inspect.signature(S.Patch.send_raw)
    assert list(sig.parameters) == ["self", "n_samples", "d_rows", "row_channels", "d_out", "stream"] and sig.parameters["stream"].default is None
    assert list(inspect.signature(S.Patch.send).parameters) == ["self", "rows"]


def test_rust_and_cpp_bindings_and_documents():
    src = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hpp = open(os.path.join(ROOT, "include", "srack.hpp")).read()
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, src), name
        assert "ffi::%s(" % name in src, name
        assert name in doc, name
        assert name + "(" in hpp, name
    for fn in ("set_sends", "get_sends", "send"):
        assert re.search(r"pub fn %s\(" % fn, src), fn
    assert "sends on the root" in doc and "another association" in doc


def test_error_codes_and_their_order_without_a_device(S):
    s1, d1 = np.array([1], dtype=np.intc), np.array([0], dtype=np.intc)
    calls = {
        "set": lambda h: S.lib.srack_buses_set_sends(h, 1, _ip(s1), _ip(d1), None, None),
        "get": lambda h: S.lib.srack_buses_get_sends(h, None, None, None, 0, None, 0),
        "plan": lambda h: S.lib.srack_buses_send_plan(h, None, 0, None, 0),
        "run": lambda h: S.lib.srack_buses_send(h, 16, 4096, 2, 1 << 20, None),
    }
    # 1: a null handle — before anything else, whatever the other arguments
    for name, call in calls.items():
        assert call(None) == S.ERR_INVALID, name
    assert S.lib.srack_buses_send(None, 0, None, 0, None, None) == S.ERR_INVALID
    # 2: before srack_voices_configure, then before a mix table exists — before the arguments are looked at
    p = _patch(S, voices=0)
    for name, call in calls.items():
        assert call(p.h) == S.ERR_STATE, name
        assert "voices_configure" in S.lib.srack_last_error().decode(), name
    assert S.lib.srack_buses_send(p.h, 0, None, 0, None, None) == S.ERR_STATE
    p.configure_voices(6)
    for name, call in calls.items():
        assert call(p.h) == S.ERR_STATE, name
        assert "set_buses" in S.lib.srack_last_error().decode(), name
    assert S.lib.srack_buses_send(p.h, 16, None, 9, None, None) == S.ERR_STATE
    p.set_buses(3, np.arange(6, dtype=np.intc) % 3)
    assert calls["get"](p.h) == 0 and p.get_sends() is None and calls["plan"](p.h) == 0 and p.send_plan() is None  # none set
    # 3: the send call before set_sends — before zero samples, before its arguments
    assert calls["run"](p.h) == S.ERR_STATE and "set_sends" in S.lib.srack_last_error().decode()
    assert S.lib.srack_buses_send(p.h, 0, None, 0, None, None) == S.ERR_STATE
    assert S.lib.srack_buses_send(p.h, 16, None, 9, None, None) == S.ERR_STATE
    assert calls["set"](p.h) == S.OK
    # 4: zero samples is nothing to do, whatever else is wrong
    assert S.lib.srack_buses_send(p.h, 0, None, 0, None, None) == S.OK
    assert S.lib.srack_buses_send(p.h, 0, 4096, 99, 4096, None) == S.OK
    # 5: the call's own arguments, refused before anything reaches the device (this host has none)
    assert S.lib.srack_buses_send(p.h, 16, None, 2, 1 << 20, None) == S.ERR_INVALID
    assert S.lib.srack_buses_send(p.h, 16, 4096, 2, None, None) == S.ERR_INVALID
    for rc in (0, 9, 1 << 31):
        assert S.lib.srack_buses_send(p.h, 16, 4096, rc, 1 << 20, None) == S.ERR_INVALID, rc
        assert "row_channels" in S.lib.srack_last_error().decode()
    n_bytes = 3 * 2 * 16 * 4
    for d_in, d_out in ((1 << 20, 1 << 20), (1 << 20, (1 << 20) + n_bytes - 4), ((1 << 20) + n_bytes - 4, 1 << 20), (1 << 20, (1 << 20) + 64)):
        assert S.lib.srack_buses_send(p.h, 16, d_in, 2, d_out, None) == S.ERR_INVALID, (d_in, d_out)
        assert "overlap" in S.lib.srack_last_error().decode()
    # (with three row channels the rows reach further: what did not overlap with two does now)
    assert S.lib.srack_buses_send(p.h, 16, 1 << 20, 3, (1 << 20) + n_bytes, None) == S.ERR_INVALID
    # nothing ran: no note, and the sends are what was set
    assert "sends=" not in p.info()
    _same_sends(p.get_sends(), s1, d1, np.ones((1, 2)), np.ones((3, 2)))


def test_refused_lists_leave_the_earlier_sends_in_place(S):
    p = _patch(S, n_buses=4, voices=8)
    src, dst = np.array([3, 1, 1], dtype=np.intc), np.array([0, 0, 2], dtype=np.intc)
    gain = np.array([[0.5, -0.25], [2.0, 3.0], [-1.0, 0.0]], dtype=np.float32)
    through = np.array([[1.0, 1.0], [0.0, 0.5], [-2.0, 2.0], [1.5, 1.25]], dtype=np.float32)
    p.set_sends(src, dst, gain, through)
    _same_sends(p.get_sends(), src, dst, gain, through)
    plan = p.send_plan()
    two = np.zeros(2, dtype=np.intc)
    refused = {
        "a null src": lambda: S.lib.srack_buses_set_sends(p.h, 2, None, _ip(two), None, None),
        "a null dst": lambda: S.lib.srack_buses_set_sends(p.h, 2, _ip(two), None, None, None),
        "a source past the buses": lambda: S.lib.srack_buses_set_sends(p.h, 2, _ip(np.array([0, 4], dtype=np.intc)), _ip(two), None, None),
        "a negative source": lambda: S.lib.srack_buses_set_sends(p.h, 2, _ip(np.array([-1, 0], dtype=np.intc)), _ip(two), None, None),
        "a destination past the buses": lambda: S.lib.srack_buses_set_sends(p.h, 2, _ip(two), _ip(np.array([0, 4], dtype=np.intc)), None, None),
        "a negative destination": lambda: S.lib.srack_buses_set_sends(p.h, 2, _ip(two), _ip(np.array([0, -1], dtype=np.intc)), None, None),
        "too many sends": lambda: S.lib.srack_buses_set_sends(p.h, S.MAX_SENDS + 1, _ip(two), _ip(two), None, None),
        "a null handle": lambda: S.lib.srack_buses_set_sends(None, 0, None, None, None, None),
        "a refused call": lambda: S.lib.srack_buses_send(p.h, 8, 4096, 2, 4096, None),
    }
    for what, call in refused.items():
        assert call() == S.ERR_INVALID, what
        assert S.lib.srack_last_error().decode(), what
        _same_sends(p.get_sends(), src, dst, gain, through)
        for a, b in zip(p.send_plan(), plan):
            np.testing.assert_array_equal(a, b, err_msg=what)


def test_round_trip_of_any_bit_pattern_and_removal(S):
    p = _patch(S, n_buses=4, voices=8)
    src, dst = np.array([1, 2, 3, 3], dtype=np.intc), np.array([0, 0, 0, 3], dtype=np.intc)
    p.set_sends(src, dst)  # NULL gains, NULL through: 1.0f everywhere
    _same_sends(p.get_sends(), src, dst, np.ones((4, 2)), np.ones((4, 2)))
    odd = np.array([0x7FC00000, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x7F7FFFFF, 0x3F800000], dtype=np.uint32).view(np.float32).reshape(4, 2)
    p.set_sends(src, dst, odd, odd[::-1])
    _same_sends(p.get_sends(), src, dst, odd, odd[::-1])  # NaN payloads, infinities, -0.0, a subnormal
    # a short read copies `cap` sends and `through_cap` buses and still returns n_sends
    s2, d2 = np.full(4, 77, dtype=np.intc), np.full(4, 77, dtype=np.intc)
    g2, t2 = np.full((4, 2), 77.0, dtype=np.float32), np.full((4, 2), 77.0, dtype=np.float32)
    assert S.lib.srack_buses_get_sends(p.h, _ip(s2), _ip(d2), _fp(g2), 2, _fp(t2), 1) == 4
    assert s2.tolist() == [1, 2, 77, 77] and d2.tolist() == [0, 0, 77, 77]
    np.testing.assert_array_equal(g2[:2].view(np.uint32), odd[:2].view(np.uint32))
    np.testing.assert_array_equal(t2[:1].view(np.uint32), odd[3:].view(np.uint32))
    assert (g2[2:] == 77.0).all() and (t2[1:] == 77.0).all()
    # only one of the two given
    p.set_sends(src, dst, None, odd)
    _same_sends(p.get_sends(), src, dst, np.ones((4, 2)), odd)
    p.set_sends(src, dst, odd, None)
    _same_sends(p.get_sends(), src, dst, odd, np.ones((4, 2)))
    # n_sends == 0 removes them: the pointers may be NULL and through is ignored
    assert S.lib.srack_buses_set_sends(p.h, 0, None, None, None, _fp(odd)) == S.OK
    assert p.get_sends() is None and p.send_plan() is None
    assert S.lib.srack_buses_send(p.h, 16, 4096, 2, 1 << 20, None) == S.ERR_STATE
    p.set_sends(src, dst)
    p.set_sends([], [])
    assert p.get_sends() is None


def test_the_limits(S):
    p = _patch(S, n_buses=32, voices=32)
    n = 65536
    src, dst = (np.arange(n) % 32).astype(np.intc), np.full(n, 7, dtype=np.intc)
    assert S.lib.srack_buses_set_sends(p.h, n - 1, _ip(src), _ip(dst), None, None) == S.OK  # 65 535 sends and the through term: 65 536 terms
    nt, order, runs = p.send_plan()
    assert nt[7] == 65536 and nt.sum() == 65535 + 32 and runs == 1024 + 31
    np.testing.assert_array_equal(order, np.arange(n - 1))
    assert S.lib.srack_buses_set_sends(p.h, n, _ip(src), _ip(dst), None, None) == S.ERR_INVALID  # one more is past the tree
    assert "65535" in S.lib.srack_last_error().decode()
    assert p.send_plan()[0][7] == 65536  # ... and the earlier list stays
    # the longest list, over 32 destinations, is taken; one more is not
    big = S.MAX_SENDS
    src, dst = (np.arange(big + 1) % 31).astype(np.intc), (np.arange(big + 1) % 32).astype(np.intc)
    assert S.lib.srack_buses_set_sends(p.h, big, _ip(src), _ip(dst), None, None) == S.OK
    nt, order, runs = p.send_plan()
    assert (nt == big // 32 + 1).all() and runs == 32 * ((big // 32 + 1 + 63) // 64)
    assert S.lib.srack_buses_get_sends(p.h, None, None, None, 0, None, 0) == big
    assert S.lib.srack_buses_set_sends(p.h, big + 1, _ip(src), _ip(dst), None, None) == S.ERR_INVALID
    assert S.lib.srack_buses_get_sends(p.h, None, None, None, 0, None, 0) == big


def test_lifetime_with_the_bus_table_and_the_voices(S):
    p = _patch(S, n_buses=3, voices=6)
    src, dst = np.array([2, 1], dtype=np.intc), np.array([0, 0], dtype=np.intc)
    gain = (np.arange(4, dtype=np.float32).reshape(2, 2) - 1.5) / 3
    through = (np.arange(6, dtype=np.float32).reshape(3, 2) - 2.5) / 3
    info = p.info()
    p.set_sends(src, dst, gain, through)
    assert p.info() == info  # not part of the program; and no call has run: no note
    # a field edit (a re-flatten) keeps the sends
    p.set_field(p.ids["vcf"], S.VCF_RES, 0.3)
    _same_sends(p.get_sends(), src, dst, gain, through)
    assert "sends=" not in p.info()
    # the same n_buses, another table: kept
    p.set_buses(3, np.array([2, 2, 1, 1, 0, -1], dtype=np.intc), np.linspace(0, 1, 6).astype(np.float32))
    _same_sends(p.get_sends(), src, dst, gain, through)
    # a bad table is refused and drops nothing
    assert S.lib.srack_voices_set_buses(p.h, 2, _ip(np.full(6, 5, dtype=np.intc)), None) == S.ERR_INVALID
    _same_sends(p.get_sends(), src, dst, gain, through)
    # the reverbs and the master's gains come and go without touching them, and they touch neither
    p.set_bus_reverbs()
    p.set_master()
    _same_sends(p.get_sends(), src, dst, gain, through)
    assert p.get_master() is not None and p.get_bus_reverbs()[0] == 3
    # another n_buses drops them
    p.set_buses(4, np.arange(6, dtype=np.intc) % 4)
    assert p.get_sends() is None and p.send_plan() is None
    p.set_sends(src, dst)
    assert p.get_sends()[3].shape == (4, 2)
    # srack_voices_configure drops the table and with it the sends
    p.configure_voices(6)
    assert S.lib.srack_buses_get_sends(p.h, None, None, None, 0, None, 0) == S.ERR_STATE
    p.set_buses(4, np.arange(6, dtype=np.intc) % 4)
    assert p.get_sends() is None


def test_plan_is_the_stable_grouping_of_an_unsorted_list(S):
    n_buses = 9
    rng = np.random.default_rng(18)
    src = rng.integers(0, n_buses, 300).astype(np.intc)
    dst = rng.choice([7, 2, 2, 5, 0], 300).astype(np.intc)  # unsorted, buses without sends, 2 fed most
    src[:40], dst[:40] = 3, 2                                # duplicate pairs
    src[40:50] = dst[40:50]                                  # src == dst
    dst[50:120] = 5                                          # more than one run
    p = _patch(S, n_buses=n_buses, voices=9)
    p.set_sends(src, dst)
    nt, order, runs = p.send_plan()
    want_nt, want_order = R.grouping(n_buses, dst)
    np.testing.assert_array_equal(nt, want_nt)
    np.testing.assert_array_equal(order, want_order)
    assert runs == R.n_runs(want_nt) and runs > n_buses and nt.min() == 1 and nt.max() > 64
    assert (np.diff(dst[order]) >= 0).all() and sorted(order.tolist()) == list(range(300))
    for d in range(n_buses):  # ascending i within a destination
        mine = order[dst[order] == d]
        assert (np.diff(mine) > 0).all() and len(mine) == nt[d] - 1
    # a short read
    nt2, o2 = np.full(n_buses, 77, dtype=np.intc), np.full(300, 77, dtype=np.intc)
    assert S.lib.srack_buses_send_plan(p.h, _ip(nt2), 2, _ip(o2), 5) == runs
    assert nt2[:2].tolist() == nt[:2].tolist() and (nt2[2:] == 77).all() and o2[:5].tolist() == order[:5].tolist() and (o2[5:] == 77).all()


@pytest.mark.parametrize("n_terms", [1, 2, 63, 64, 65])
def test_reference_is_the_sequential_sum_up_to_65_terms(n_terms):
    rows, gain = R.case_inputs(n_terms, 70)
    src, dst = R.all_to_one(n_terms)
    tree = R.send_tree(rows, src, dst, gain[1:], gain)
    seq = R.send_sequential(rows, src, dst, gain[1:], gain)
    assert tree.dtype == np.float32 and tree.shape == rows.shape
    assert np.abs(tree[0]).max() > 1e-3 and np.count_nonzero(tree[0]) > tree[0].size // 2
    np.testing.assert_array_equal(tree.view(np.uint32), seq.view(np.uint32))


def test_reference_tree_differs_from_the_sequential_sum_at_129_terms():
    rows, gain = R.case_inputs(129, 70)
    src, dst = R.all_to_one(129)
    tree = R.send_tree(rows, src, dst, gain[1:], gain)
    seq = R.send_sequential(rows, src, dst, gain[1:], gain)
    assert np.count_nonzero(tree[0].view(np.uint32) != seq[0].view(np.uint32)) > 70  # (most samples: the association matters)
    np.testing.assert_allclose(tree, seq, rtol=0, atol=1e-4)  # ... and nothing else does
    np.testing.assert_array_equal(tree[1:].view(np.uint32), seq[1:].view(np.uint32))  # (the buses without sends: one term each)


@pytest.mark.parametrize("n_buses", [5, 66, 129, 4097])
def test_reference_row_0_of_all_to_one_is_the_master_tree(n_buses):
    rows, gain = R.case_inputs(n_buses, 70)
    src, dst = R.all_to_one(n_buses)
    out = R.send_tree(rows, src, dst, gain[1:], gain, only=[0])
    np.testing.assert_array_equal(out[0].view(np.uint32), M.master_tree(rows, gain).view(np.uint32))
    assert np.abs(out[0]).max() > 1e-3


def test_reference_edges():
    rows, gain = R.case_inputs(4, 9)
    # a bus without sends is +0.0 + through * row: -0.0 becomes +0.0
    z = np.full((3, 2, 4), -0.0, dtype=np.float32)
    assert (R.send_tree(z, [1], [0]).view(np.uint32) == 0).all()
    # the input is read, not the output: 0 -> 1 and 1 -> 2 in one call moves nothing of bus 0 into bus 2
    out = R.send_tree(rows, [0, 1], [1, 2])
    np.testing.assert_array_equal(out[2], np.float32(0) + rows[2] + rows[1])
    np.testing.assert_array_equal(out[1], np.float32(0) + rows[1] + rows[0])
    # src == dst is a second gain on the own row; a duplicate pair adds twice
    out = R.send_tree(rows, [3, 3, 3], [3, 0, 0], np.array([[0.5, 0.5]] * 3, dtype=np.float32))
    np.testing.assert_array_equal(out[3], (np.float32(0) + rows[3]) + np.float32(0.5) * rows[3])
    np.testing.assert_array_equal(out[0], ((np.float32(0) + rows[0]) + np.float32(0.5) * rows[3]) + np.float32(0.5) * rows[3])
    # a third channel is neither read nor written; one row channel has one
    rows3, _ = R.case_inputs(4, 9, row_channels=3)
    out = R.send_tree(rows3, [1], [0])
    assert not out[:, 2].any() and out[:, :2].any()
    rows1, _ = R.case_inputs(4, 9, row_channels=1)
    assert R.send_tree(rows1, [1], [0]).shape == (4, 1, 9)
    # 0 * inf is NaN, and reaches the destination it is sent to only
    zero = np.zeros((3, 2, 3), dtype=np.float32)
    out = R.send_tree(zero, [1], [0], np.full((1, 2), np.inf, dtype=np.float32))
    assert np.isnan(out[0]).all() and not np.isnan(out[1:]).any()
