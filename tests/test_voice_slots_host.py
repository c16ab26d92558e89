"""Voice bus slots (srack_voices_set_bus_slots / srack_voices_get_bus_slots): the C ABI surface, the bindings, the argument checks, the
lifetime of the one mix table of a handle, the host-side plan over (tile, slot) groups (csrc/buses.hpp: bus_slot_plan_make) and the
bit-exact reference of tests/voice_slots_ref.py itself — all without a GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import srack_pkg
from tests import voice_slots_ref as VR
from tests.test_mix_buses_host import _CTYPES, _fp, _ip, _prototype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["srack_voices_set_bus_slots", "srack_voices_get_bus_slots"]


@pytest.fixture(scope="module")
def S():
    return srack_pkg.load()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def patch(S, V, channels=2):
    p = S.Patch(48000, 1024, channels)
    osc, out = p.add_module(S.MOD_OSCILLATOR), p.add_module(S.MOD_OUTPUT)
    for c in range(min(channels, 2)):
        p.connect(osc, S.OSC_OUT_SAW, out, c)
    if V:
        p.configure_voices(V)
    return p


def test_symbols_prototypes_and_argtypes(S):
    hdr = open(os.path.join(ROOT, "include", "srack_hip.h")).read()
    L = ctypes.CDLL(S.LIB_PATH)
    assert L.srack_abi_version() == 2
    assert re.search(r"#define SRACK_MAX_VOICE_SLOTS 4\b", hdr) and S.MAX_VOICE_SLOTS == 4
    for name in NAMES:
        assert name in S.ABI_SYMBOLS and hasattr(L, name), name
        proto = _prototype(hdr, name)
        argtypes = getattr(S.lib, name).argtypes
        assert len(argtypes) == len(proto), name
        for (ctype, pname), at in zip(proto, argtypes):
            assert at is _CTYPES[ctype], f"{name}: {pname} is {at}, the header says {ctype}"
    assert [n for _, n in _prototype(hdr, "srack_voices_set_bus_slots")] == ["p", "n_buses", "n_slots", "bus", "gain"]
    assert [n for _, n in _prototype(hdr, "srack_voices_get_bus_slots")] == ["p", "n_slots", "bus", "gain", "cap"]


def test_python_wrappers(S):
    assert list(inspect.signature(S.Patch.set_bus_slots).parameters) == ["self", "n_buses", "bus", "gain"]
    assert inspect.signature(S.Patch.set_bus_slots).parameters["gain"].default is None
    assert list(inspect.signature(S.Patch.get_bus_slots).parameters) == ["self"]


def test_rust_and_cpp_bindings_and_documents():
    src = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hpp = open(os.path.join(ROOT, "include", "srack.hpp")).read()
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, src), name
        assert "ffi::%s(" % name in src, name
        assert name in doc, name
        assert name + "(" in hpp, name
    assert "MAX_VOICE_SLOTS: u32 = 4" in src
    assert "srack_voices_set_bus_slots" in open(os.path.join(ROOT, "README.md")).read()
    assert "bus_slot_fold_tiles" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert os.path.exists(os.path.join(ROOT, "notes", "r31.md"))


def test_argument_checks_without_a_device(S):
    V, K, C = 10, 3, 2
    rng = np.random.default_rng(31)
    bus = rng.integers(-1, 5, (V, K)).astype(np.intc)
    bus[3, 1] = 4  # (the table needs all five buses)
    gain = VR.slot_gains((V, K, C), rng)
    u = ctypes.c_int(99)
    assert S.lib.srack_voices_set_bus_slots(None, 5, K, _ip(bus), _fp(gain)) == S.ERR_INVALID
    assert S.lib.srack_voices_get_bus_slots(None, ctypes.byref(u), None, None, 0) == S.ERR_INVALID
    p = patch(S, 0)
    assert S.lib.srack_voices_set_bus_slots(p.h, 5, K, _ip(bus), _fp(gain)) == S.ERR_STATE
    assert "voices_configure" in S.lib.srack_last_error().decode()
    p.configure_voices(V)
    assert p.get_bus_slots() == (0, None, None)
    assert S.lib.srack_voices_get_bus_slots(p.h, ctypes.byref(u), None, None, 0) == 0 and u.value == 0

    def bad_calls(check):
        b5 = bus.copy()
        b5[7, 2] = 5
        bm2 = bus.copy()
        bm2[0, 1] = -2
        for n_buses, k, b in ((0, K, bus), (S.MAX_BUSES + 1, K, bus), (5, 0, bus), (5, S.MAX_VOICE_SLOTS + 1, bus), (4, K, bus), (5, K, b5), (5, K, bm2)):
            big = np.zeros((V, max(k, K) + 2), dtype=np.intc)
            big[:, :K] = b
            arg = b if k == K else big  # (a bad count is refused before anything is read)
            assert S.lib.srack_voices_set_bus_slots(p.h, n_buses, k, _ip(np.ascontiguousarray(arg)), None) == S.ERR_INVALID, (n_buses, k)
            check()

    # a slot table; bad calls of either setter leave it in place
    p.set_bus_slots(5, bus, gain)

    def slot_table_stays():
        n, b2, g2 = p.get_bus_slots()
        assert n == 5 and (b2 == bus).all()
        np.testing.assert_array_equal(bits(g2), bits(gain))

    bad_calls(slot_table_stays)
    assert S.lib.srack_voices_set_buses(p.h, 2, _ip(np.full(V, 3, dtype=np.intc)), None) == S.ERR_INVALID
    slot_table_stays()
    assert S.lib.srack_voices_set_bus_slots(p.h, 5, 9, None, None) == S.ERR_INVALID and "n_slots" in S.lib.srack_last_error().decode()
    # srack_voices_get_buses on a slot table: n_buses, slot 0, channel 0
    n, b1, g1 = p.get_buses()
    assert n == 5 and (b1 == bus[:, 0]).all()
    np.testing.assert_array_equal(bits(g1), bits(gain[:, 0, 0]))
    # a short read counts voices
    b3, g3 = np.full((V, K), 77, dtype=np.intc), np.full((V, K, C), 7.0, dtype=np.float32)
    assert S.lib.srack_voices_get_bus_slots(p.h, ctypes.byref(u), _ip(b3), _fp(g3), 4) == 5 and u.value == K
    assert (b3[:4] == bus[:4]).all() and (b3[4:] == 77).all() and (g3[4:] == 7.0).all()
    np.testing.assert_array_equal(bits(g3[:4]), bits(gain[:4]))
    # an old-style table; bad calls of the new setter leave it in place; it reads back as one slot, the gain repeated per channel
    ob, og = (np.arange(V, dtype=np.intc) % 3), np.linspace(-1, 1, V).astype(np.float32)
    p.set_buses(3, ob, og)

    def old_table_stays():
        n, b2, g2 = p.get_buses()
        assert n == 3 and (b2 == ob).all() and (g2 == og).all()
        n, b2, g2 = p.get_bus_slots()
        assert n == 3 and b2.shape == (V, 1) and (b2[:, 0] == ob).all() and g2.shape == (V, 1, C)
        np.testing.assert_array_equal(bits(g2), bits(np.repeat(og, C).reshape(V, 1, C)))

    old_table_stays()
    bad_calls(old_table_stays)
    # defaults: NULL bus -> slot 0 is bus 0 and the other slots none; NULL gain -> 1.0
    assert S.lib.srack_voices_set_bus_slots(p.h, 2, 3, None, None) == S.OK
    n, b2, g2 = p.get_bus_slots()
    assert n == 2 and b2.shape == (V, 3) and (b2[:, 0] == 0).all() and (b2[:, 1:] == S.BUS_NONE).all() and (g2 == 1.0).all()
    p.set_bus_slots(S.MAX_BUSES, bus)  # the largest count; buses may be empty
    assert p.get_bus_slots()[0] == S.MAX_BUSES and p.n_buses() == S.MAX_BUSES
    # srack_voices_configure drops the table
    p.configure_voices(V)
    assert p.get_bus_slots() == (0, None, None) and p.get_buses() == (0, None, None)
    assert S.lib.srack_render_buses(p.h, 16, None, None, None, 4096, 0, None) == S.ERR_STATE


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_every_bit_pattern_of_the_gains_round_trips(S, channels):
    V, K = 37, 4
    rng = np.random.default_rng(channels)
    pat = rng.integers(0, 2 ** 32, (V, K, channels), dtype=np.uint64).astype(np.uint32)
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x00000001, 0x807FFFFF, 0x7F7FFFFF], dtype=np.uint32)
    pat.reshape(-1)[:len(special)] = special  # +-0, +-inf, quiet and signalling NaNs with payloads, subnormals, the largest finite
    p = patch(S, V, channels)
    bus = rng.integers(-1, 6, (V, K)).astype(np.intc)
    p.set_bus_slots(6, bus, pat.view(np.float32))
    n, b2, g2 = p.get_bus_slots()
    assert n == 6 and (b2 == bus).all() and g2.shape == (V, K, channels)
    np.testing.assert_array_equal(bits(g2), pat)
    np.testing.assert_array_equal(bits(p.get_buses()[2]), pat[:, 0, 0])


def test_the_console_goes_with_n_buses_and_stays_with_the_table_kind(S):
    V = 6
    p = patch(S, V)
    for name, call in (("master", lambda: S.lib.srack_buses_get_master(p.h, None, 0)), ("sends", lambda: S.lib.srack_buses_get_sends(p.h, None, None, None, 0, None, 0))):
        assert call() == S.ERR_STATE, name  # no mix table yet
    bus = np.array([[0, 2], [1, -1], [2, 2], [-1, -1], [0, 1], [1, 0]], dtype=np.intc)
    p.set_bus_slots(3, bus)  # every console call that needs "a mix table" accepts a slot table
    desc = p.info()
    g = np.arange(6, dtype=np.float32).reshape(3, 2)
    p.set_master(g)
    p.set_sends([0, 1], [2, 2])
    p.set_bus_reverbs()
    p.set_bus_filter()
    p.set_bus_vca()
    p.set_bus_shaper()
    np.testing.assert_array_equal(p.get_master(), g)

    def all_set():
        np.testing.assert_array_equal(p.get_master(), g)
        return p.get_sends() is not None and p.get_bus_reverbs()[0] == 3 and p.get_bus_filter()[0] == 3 and p.get_bus_vca()[0] == 3 and p.get_bus_shaper()[0] == 3

    # the same n_buses keeps the console, whichever setter and whichever kind the table was
    p.set_bus_slots(3, bus[:, ::-1].copy(), np.full((V, 2, 2), 0.5, np.float32))
    assert all_set()
    p.set_buses(3, bus[:, 0])
    assert all_set() and p.get_bus_slots()[1].shape == (V, 1)
    p.set_bus_slots(3, bus[:, :1])
    assert all_set()
    assert S.lib.srack_voices_set_bus_slots(p.h, 3, 5, None, None) == S.ERR_INVALID and all_set()  # a refused call drops nothing
    assert p.info() == desc  # not part of the program: the description does not change
    # another n_buses drops it, from either side
    p.set_bus_slots(4, bus)
    assert p.get_master() is None and p.get_sends() is None and p.get_bus_reverbs()[0] == 0
    p.set_master()
    p.set_buses(4, bus[:, 0])
    assert p.get_master() is not None
    p.set_buses(5, bus[:, 0])
    assert p.get_master() is None
    p.set_master()
    p.set_bus_slots(5, bus)
    assert p.get_master() is not None
    p.configure_voices(V)
    assert S.lib.srack_buses_get_master(p.h, None, 0) == S.ERR_STATE


def random_tables(rng):
    for V, n in ((1, 1), (64, 3), (65, 7), (130, 5), (300, 300), (1000, 7), (4097, 64)):
        b = rng.integers(0, max(1, n - n // 4), V)
        b[rng.random(V) < 0.2] = -1
        yield V, n, b


def test_one_slot_plans_like_set_buses(S):
    rng = np.random.default_rng(6)
    cases = list(random_tables(rng)) + [(4096, 64, np.arange(4096) // 64), (1000, 64, np.arange(1000) % 64), (100, 3, np.full(100, -1))]
    for V, n, b in cases:
        p, q = patch(S, V), patch(S, V)
        p.set_buses(n, b)
        q.set_bus_slots(n, np.asarray(b).reshape(V, 1))
        (seg, order), (seg1, order1) = p.bus_plan(), q.bus_plan()
        np.testing.assert_array_equal(seg1, seg)
        np.testing.assert_array_equal(order1, order)


def check_slot_plan(S, V, n_buses, bus):
    """segments in ascending (tile, slot, bus) order, i.e. ascending (group, bus); a bus's scratch rows ascend in that order; every (v, k)
    that is not NONE exactly once in `order`; a bus with one segment has no row"""
    K = bus.shape[1]
    p = patch(S, V)
    p.set_bus_slots(n_buses, bus)
    seg, order = p.bus_plan()
    at, last, rows, seen = 0, (-1, -1, -1), {}, set()
    for group, b, row, n in seg.tolist():
        tile, k = divmod(group, K)
        assert 1 <= n <= 64 and (tile, k, b) > last
        last = (tile, k, b)
        voices = order[at:at + n]
        at += n
        assert (voices // 64 == tile).all() and (bus[voices, k] == b).all() and (np.diff(voices) > 0).all()
        for v in voices.tolist():
            assert (v, k) not in seen
            seen.add((v, k))
        rows.setdefault(b, []).append(row)
    assert at == len(order)
    assert seen == {(int(v), int(k)) for v, k in zip(*np.nonzero(bus != S.BUS_NONE))}
    used = []
    for b, r in rows.items():
        if len(r) == 1:
            assert r == [-1]
        else:
            assert r == list(range(r[0], r[0] + len(r)))  # consecutive, ascending with (tile, slot)
            used += r
    assert sorted(used) == list(range(len(used)))
    # the groups of the reference are the segments of the plan
    want = [(tile * K + k, b, len(vs)) for tile, k, members in VR.groups(V, bus) for b, vs in sorted(members.items())]
    assert [(g, b, n) for g, b, _, n in seg.tolist()] == want
    return seg


@pytest.mark.parametrize("K", [2, 4])
def test_the_plan_over_groups(S, K):
    rng = np.random.default_rng(60 + K)
    for V, n in ((1, 2), (64, 3), (65, 7), (130, 5), (257, 300), (1000, 7)):
        bus = rng.integers(0, max(1, n - n // 4), (V, K))
        bus[rng.random((V, K)) < 0.3] = -1
        check_slot_plan(S, V, n, bus)
    # a voice naming one bus in every slot: as many terms; every voice of three tiles in one bus through every slot: 3 K rows
    V = 192
    seg = check_slot_plan(S, V, 2, np.ones((V, K), dtype=int))
    assert len(seg) == 3 * K and seg[:, 2].tolist() == list(range(3 * K)) and (seg[:, 3] == 64).all()
    # slot 0 all NONE in the first tile
    bus = rng.integers(0, 3, (130, K))
    bus[:64, 0] = -1
    seg = check_slot_plan(S, 130, 3, bus)
    assert (seg[:, 0] != 0).all()
    # nobody anywhere
    assert len(check_slot_plan(S, 100, 3, np.full((100, K), -1))) == 0


@pytest.mark.parametrize("K,cp", [(1, [0]), (2, [0, 0]), (4, [0, 1]), (4, [0, 1, -1])])
def test_the_reference_is_an_f32_sum_of_the_terms(K, cp):
    """the reference on synthetic frames against the f64 sum, inside the derived bound for an f32 sum of n rounded products"""
    V, T, n_buses = 130, 97, 6
    rng = np.random.default_rng(K + len(cp))
    fr = rng.uniform(-1, 1, (max(cp) + 1, T, V)).astype(np.float32)
    bus = rng.integers(-1, n_buses - 1, (V, K))  # (the last bus stays empty)
    bus[:64, 0] = 0  # many terms in one bus
    gain = VR.slot_gains((V, K, len(cp)), rng)
    got = VR.slot_reference(fr, cp, n_buses, bus, gain)
    ref, bound, n = VR.slot_sums_f64(fr, cp, n_buses, bus, gain)
    assert got.dtype == np.float32 and n.max() >= 64 and n[-1] == 0
    err = np.abs(got.astype(np.float64) - ref)
    print(f"K={K} cp={cp}: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()
    assert err.max() > 0, "an f32 sum of this many terms that is exact in f64 checks nothing"
    assert not got[-1].any() and not np.signbit(got[-1]).any()  # an empty bus is +0
    for c, plane in enumerate(cp):
        if plane < 0:
            assert not got[:, c].any() and not np.signbit(got[:, c]).any()
    # one term: the product itself, sign of zero included; the same bus twice: two terms
    one = VR.slot_reference(fr[:, :, :1], cp, 2, np.array([[1] + [-1] * (K - 1)]), np.full((1, K, len(cp)), -0.0, np.float32))
    np.testing.assert_array_equal(bits(one[1, 0]), bits(np.float32(-0.0) * fr[cp[0]][:, 0]))
    if K > 1:
        two = VR.slot_reference(fr[:, :, :1], cp, 1, np.zeros((1, K), dtype=int), np.ones((1, K, len(cp)), np.float32))
        acc = fr[cp[0]][:, 0]
        for _ in range(K - 1):
            acc = acc + fr[cp[0]][:, 0]
        np.testing.assert_array_equal(bits(two[0, 0]), bits(acc))
