"""Voice bus slots (srack_voices_set_bus_slots): each voice in up to four buses with a gain per channel, folded by bus_slot_fold_tiles /
bus_slot_fold_sum (folds.hip.h) from frames that each wave reads once.

Two yardsticks, neither with a tolerance: a twin patch's srack_voices_set_buses render (K = 1, the gain repeated per channel: the bits
of the fold that was there before), and the NumPy reference of tests/voice_slots_ref.py computed from the frames the same call
returned (f32 products, sequential f32 additions in the documented order).

The shapes are the smallest at which the fold can go wrong: 1, 64, 65 and 130 voices (a lone lane, a full tile, a ragged second tile,
a ragged third); 1, 63 and 65 samples (a ragged slab, a second slab of one row) and 4 100 (a second launch of four rows on the
flagship); 1, 2 and 4 slots; one channel, two on one plane, two on two planes (P3) and three with one unconnected."""
import os
import subprocess
import sys

import numpy as np
import pytest

import srack_pkg
from tests import master_ref as RM
from tests import sends_ref as RS
from tests import voice_slots_ref as VR
from tests.test_gpu_mix_buses import NO_FUSION, NO_SPEC, all_fields, assert_audible, bits, maker, mixed_gains

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def S():
    return srack_pkg.load()


def assert_same_bits(got, want, what=""):
    """equal bit for bit — the sign of a zero included —, or NaN where the reference is NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{what}: NaN where the reference has none, or the reverse")
    bad = (bits(got) != bits(want)) & ~nan
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} of {bad.size} samples differ; the first at {tuple(np.argwhere(bad)[0])}"


def saw_patch(S, V, channels, two_planes=False):
    """an oscillator per voice, pitches spread over three octaves: saw -> Left (and Right; with two_planes the sine -> Right)"""
    p = S.Patch(48000, 1024, channels)
    osc, out = p.add_module(S.MOD_OSCILLATOR), p.add_module(S.MOD_OUTPUT)
    p.connect(osc, S.OSC_OUT_SAW, out, 0)
    if channels > 1:
        p.connect(osc, S.OSC_OUT_SINE if two_planes else S.OSC_OUT_SAW, out, 1)
    p.configure_voices(V)
    p.set_voice_field(osc, S.OSC_VAL, np.linspace(-1.0, 2.0, V).astype(np.float32) if V > 1 else np.array([0.5], np.float32))
    return p


def special_table(V, K, C, n_buses, rng):
    """A random table (n_buses >= 5) with NONE slots and the last bus empty, and with what the plan has to get right: a voice names
    one bus twice; (from 65 voices on) the first tile's slot 0 is all NONE while its slot 1 is not; (from 130 on) every voice of the tiles behind the first
    sits in bus 2 through the first and the last slot (many partial rows); gains among 0, -0.0, negative and powers of two, one inf and one NaN."""
    bus = rng.integers(0, n_buses - 1, (V, K))
    bus[rng.random((V, K)) < 0.25] = VR.NONE
    gain = VR.slot_gains((V, K, C), rng)
    if K > 1 and V >= 65:
        bus[:64, 0] = VR.NONE
        bus[:64, 1] = rng.integers(0, n_buses - 1, 64)
    if V >= 130:
        bus[64:, 0] = bus[64:, K - 1] = 2  # (K == 2: each of these voices names bus 2 twice)
    elif K > 1:
        twice = 0 if V < 65 else 64
        bus[twice, 0] = bus[twice, 1] = 1
    # one inf and one NaN, each on one (voice, slot, channel) that is in a bus other than 0
    placed = [(v, k) for v in range(V) for k in range(K) if bus[v, k] > 0][:2]
    for (v, k), c, x in zip(placed, (0, C - 1), (np.inf, np.nan)):
        gain[v, k, c] = x
    return bus, gain


def render_and_compare(p, n_buses, bus, gain, T, flags=0, what=""):
    p.set_bus_slots(n_buses, bus, gain)
    fr, _, _, bm = p.render_buses(T, frames=True, flags=flags)
    K = np.shape(bus)[1]
    assert f" buses={n_buses}[fold slots={K}]" in p.info(), p.info()
    n_planes, cp = p.planes()
    want = VR.slot_reference(fr, cp, n_buses, bus, gain)
    assert_same_bits(bm, want, what)
    return fr, bm, want, cp


# ---- 1. today's bits: K = 1, the gain repeated per channel, against a twin's srack_voices_set_buses render --------------------------------------
FAMILIES = [
    ("cfg3", None, 1, 3000, 0, "render_voice_chain"),
    ("cfg3", None, 20, 5000, 0, "render_voice_chain_track"),
    ("p3", None, 257, 5000, 0, "render_voice_chain_seq"),
    ("cfg4", 1, 257, 5000, 0, "render_fm_pair_x"),
    ("cfg4", 1024, 100, 9000, 0, "render_fm_pair_block_x"),
    ("cfg2", None, 4096, 3000, 0, None),
    ("cfg3_poly", None, 4097, 2500, 0, "render_specialized"),
    ("cfg3", None, 257, 5000, NO_FUSION | NO_SPEC, "render_interp"),
]


@pytest.mark.parametrize("w,B,V,T,flags,kernel", FAMILIES)
def test_one_slot_has_the_bits_of_set_buses(S, w, B, V, T, flags, kernel):
    rng = np.random.default_rng(V + T)
    n_buses = 7
    bus = rng.integers(-1, n_buses - 1, V)
    gain = mixed_gains(V, rng)
    make = maker(S, w, V, B, nan_voices=(3, 17, 5, 9))
    p, q = make(), make()
    p.set_buses(n_buses, bus, gain)
    q.set_bus_slots(n_buses, bus[:, None], np.repeat(gain, 2).reshape(V, 1, 2))
    fr0, _, _, old = p.render_buses(T, frames=True, flags=flags)
    fr1, _, _, new = q.render_buses(T, frames=True, flags=flags)
    ip, iq = p.info(), q.info()
    assert f" buses={n_buses}[fold]" in ip and f" buses={n_buses}[fold slots=1]" in iq, (ip, iq)
    assert ip.split(" buses=")[0] == iq.split(" buses=")[0] and ip.split("kernel=")[-1] == iq.split("kernel=")[-1]  # (a jit= note may say where the kernel came from)
    assert ip.split("kernel=")[-1] == kernel if kernel else "kernel=" in ip, ip
    assert_audible(fr0)
    np.testing.assert_array_equal(bits(fr1), bits(fr0))
    np.testing.assert_array_equal(bits(new), bits(old))
    assert not new[n_buses - 1].any()  # the empty bus


# ---- 2. bit for bit against the reference ---------------------------------------------------------------------------------------------------------
# (patch, channels, V, T, K)
CASES = [
    ("saw", 1, 1, 1, 1), ("saw", 1, 64, 63, 2), ("saw", 1, 65, 65, 4), ("saw", 1, 130, 65, 2),
    ("saw", 2, 1, 63, 4), ("saw", 2, 64, 65, 4), ("saw", 2, 65, 1, 2), ("saw", 2, 130, 63, 4),
    ("two", 2, 65, 63, 2), ("two", 2, 130, 65, 4),
    ("saw", 3, 64, 1, 1), ("saw", 3, 65, 65, 2), ("saw", 3, 130, 63, 4),
    ("cfg3", 2, 130, 4100, 4), ("cfg3", 2, 65, 4100, 1), ("cfg3", 2, 64, 4100, 2),
    ("p3", 2, 130, 4100, 2), ("p3", 2, 65, 65, 4), ("p3", 2, 1, 63, 1),
]


@pytest.mark.parametrize("kind,C,V,T,K", CASES)
def test_bit_for_bit_against_the_reference(S, kind, C, V, T, K):
    rng = np.random.default_rng(1000 * V + 10 * T + K)
    n_buses = 6
    if kind in ("cfg3", "p3"):
        p = maker(S, kind, V, nan_voices=(3,) if kind == "cfg3" else ())()
    else:
        p = saw_patch(S, V, C, two_planes=kind == "two")
    bus, gain = special_table(V, K, C, n_buses, rng)
    fr, bm, want, cp = render_and_compare(p, n_buses, bus, gain, T, what=f"{kind} C={C} V={V} T={T} K={K}")
    n_planes = {"two": 2, "p3": 2}.get(kind, 1)
    assert (p.planes()[0], len(cp)) == (n_planes, C) and (C < 3 or cp[2] == -1)
    if T >= 4100 or (kind in ("saw", "two") and T >= 63):  # (P1 and P3 open their envelopes later than 65 samples)
        assert_audible(fr)
    # an empty bus and an unconnected channel are +0
    assert not bits(bm[n_buses - 1]).any()
    if C == 3:
        assert not bits(bm[:, 2]).any()
    # the non-finite gains (and cfg3's NaN voice) reach the buses and channels the reference says, and no others: the table has both kinds
    if V * K >= 8 and T >= 63:
        bad = ~np.isfinite(want).all(axis=2)
        np.testing.assert_array_equal(~np.isfinite(bm).all(axis=2), bad)
        assert bad.any() and not bad.all(), "the table no longer has a bus and channel of each kind"


def test_a_bus_named_twice_is_two_terms_and_many_rows_add_in_group_order(S):
    V, T, K = 130, 65, 4
    p = saw_patch(S, V, 2)
    gain = np.ones((V, K, 2), dtype=np.float32)
    gain[:, :, 1] = np.float32(1.0) / 3
    fr, bm, _, _ = render_and_compare(p, 1, np.zeros((V, K), dtype=int), gain, T, what="everything in one bus")
    seg, order = p.bus_plan()
    assert len(seg) == 3 * K and seg[:, 2].tolist() == list(range(3 * K)) and len(order) == V * K
    acc = None
    for tile in range(3):
        for k in range(K):
            s = None
            for v in range(tile * 64, min(V, tile * 64 + 64)):
                s = fr[0][:, v] if s is None else s + fr[0][:, v]
            acc = s if acc is None else acc + s
    assert_same_bits(bm[0, 0], acc, "Left, unit gains")


# ---- 3. pan costs no plane --------------------------------------------------------------------------------------------------------------------------
def test_pan_costs_no_plane(S):
    V, T = 130, 4100
    rng = np.random.default_rng(33)
    make = maker(S, "cfg3", V, nan_voices=(3,))
    plain = make()
    fr0, _ = plain.render(T, mix=False)
    p = make()
    bus = rng.permutation(V)
    theta = rng.uniform(0, np.pi / 2, V)
    gain = np.stack([np.cos(theta), np.sin(theta)], axis=1).astype(np.float32).reshape(V, 1, 2)  # equal-power pan
    assert (gain[:, 0, 0] != gain[:, 0, 1]).all()
    p.set_bus_slots(V, bus[:, None], gain)
    fr, _, _, bm = p.render_buses(T, frames=True)
    assert p.planes() == (1, [0, 0]) == plain.planes()
    assert p.info().split("kernel=")[-1] == plain.info().split("kernel=")[-1] == "render_voice_chain_track", p.info()
    assert "buses=" not in plain.info() and f" buses={V}[fold slots=1]" in p.info()
    assert_audible(fr)
    np.testing.assert_array_equal(bits(fr), bits(fr0))
    with np.errstate(all="ignore"):
        for c in range(2):
            want = (fr[0] * gain[None, :, 0, c]).T  # f32 products, [V][T]
            assert want.dtype == np.float32
            assert_same_bits(bm[bus, c], np.ascontiguousarray(want), f"channel {c}")
    assert (bm[bus[0], 0] != bm[bus[0], 1]).any()


# ---- 4. cuts ------------------------------------------------------------------------------------------------------------------------------------------
CUTS = (1, 63, 65)


@pytest.mark.parametrize("w,K", [("cfg3", 4), ("p3", 2), ("cfg4", 2)])
def test_however_the_render_is_cut(S, w, K):
    V, T, n_buses = 130, 4100 + 129, 6
    rng = np.random.default_rng(40 + K)
    bus, gain = special_table(V, K, 2, n_buses, rng)
    gain[~np.isfinite(gain)] = 0.5
    def make():
        p = maker(S, w, V)()
        p.set_bus_slots(n_buses, bus, gain)
        return p
    fr, _, _, whole = make().render_buses(T, frames=True)
    assert_audible(fr)
    assert_same_bits(whole, VR.slot_reference(fr, make().planes()[1], n_buses, bus, gain), f"{w}: one call")
    q = make()
    parts = [q.render_buses(n, frames=(i % 2 == 0), stats=(i == 1))[3] for i, n in enumerate(CUTS + (T - sum(CUTS),))]
    np.testing.assert_array_equal(bits(np.concatenate(parts, axis=2)), bits(whole))
    _, _, _, alone = make().render_buses(T)  # nothing else asked for: the frames go to the library's scratch
    np.testing.assert_array_equal(bits(alone), bits(whole))


def test_cuts_with_kept_state_and_an_edit_between_calls(S):
    V, K, n_buses = 130, 4, 6
    rng = np.random.default_rng(44)
    bus, gain = special_table(V, K, 2, n_buses, rng)
    gain[~np.isfinite(gain)] = -0.25
    rest = 4100
    def run(cuts, edit_after):
        p = maker(S, "cfg3", V)()
        p.keep_state(True)
        p.set_bus_slots(n_buses, bus, gain)
        frs, bms = [], []
        for i, n in enumerate(cuts):
            fr, _, _, bm = p.render_buses(n, frames=True)
            frs.append(fr), bms.append(bm)
            if i == edit_after:
                p.set_field(p.ids["vcf"], S.VCF_RES, 0.8)  # re-flattens; the voices carry on (srack_patch_keep_state)
        return np.concatenate(frs, axis=1), np.concatenate(bms, axis=2), p
    fr_a, bm_a, pa = run(CUTS + (rest,), 2)
    fr_b, bm_b, pb = run((sum(CUTS), rest), 0)
    fr_c, _, _ = run((sum(CUTS) + rest,), -1)  # no edit
    assert_audible(fr_a)
    np.testing.assert_array_equal(bits(fr_a), bits(fr_b))
    np.testing.assert_array_equal(bits(bm_a), bits(bm_b))
    assert (bits(fr_a[:, sum(CUTS):]) != bits(fr_c[:, sum(CUTS):])).any(), "the edit is not heard: the test checks nothing about it"
    np.testing.assert_array_equal(bits(fr_a[:, :sum(CUTS)]), bits(fr_c[:, :sum(CUTS)]))
    assert_same_bits(bm_a, VR.slot_reference(fr_a, pa.planes()[1], n_buses, bus, gain), "cuts with an edit")


def test_changing_the_slot_table_between_calls_moves_nothing(S):
    V, T = 130, 4100
    rng = np.random.default_rng(45)
    make = maker(S, "cfg3", V)
    plain = make()
    whole, _ = plain.render(T, mix=False)
    p = make()
    b1, g1 = special_table(V, 2, 2, 6, rng)
    b2, g2 = special_table(V, 4, 2, 9, rng)
    p.set_bus_slots(6, b1, g1)
    a, _, _, bm1 = p.render_buses(T // 2, frames=True)
    desc = p.info().split(" buses=")[0]
    p.set_bus_slots(9, b2, g2)
    assert p.info().split(" buses=")[0] == desc
    b, _, _, bm2 = p.render_buses(T - T // 2, frames=True)
    assert bm1.shape == (6, 2, T // 2) and bm2.shape == (9, 2, T - T // 2)
    np.testing.assert_array_equal(bits(np.concatenate([a, b], axis=1)), bits(whole))
    assert_same_bits(bm2, VR.slot_reference(b, p.planes()[1], 9, b2, g2), "the second table")
    want, got = all_fields(S, plain), all_fields(S, p)
    assert len(want) >= 8 and got.keys() == want.keys()
    for k in want:
        np.testing.assert_array_equal(got[k].view(np.uint64), want[k].view(np.uint64), err_msg=f"module {k[0]} field {k[1]}")


# ---- 5. downstream: the console on rows from a slot table ----------------------------------------------------------------------------------------------
def test_the_console_runs_on_rows_from_a_slot_table(S):
    V, T, K, NB = 130, 300, 2, 8
    rng = np.random.default_rng(50)
    group = np.arange(V) % 4                   # four group buses, four aux buses: each voice feeds its group and one aux bus by its own amount
    bus = np.stack([group, 4 + rng.integers(0, 4, V)], axis=1)
    gain = rng.uniform(0.1, 1.0, (V, K, 2)).astype(np.float32)
    mgain = rng.uniform(-2.0, 2.0, (NB, 2)).astype(np.float32)
    src, dst = np.arange(4, dtype=np.intc), (4 + (np.arange(4) + 1) % 4).astype(np.intc)
    sgain = rng.uniform(0.1, 0.6, (4, 2)).astype(np.float32)
    p = maker(S, "cfg3", V)()
    fr, bm, _, _ = render_and_compare(p, NB, bus, gain, T, what="the bus mixes")
    assert_audible(bm[4:])
    p.set_master(mgain)
    p.set_sends(src, dst, sgain)
    sent = p.send(bm)
    assert_same_bits(sent, RS.send_tree(bm, src, dst, sgain), "the sends of the bus mixes")
    m, _ = p.master(sent)
    assert_same_bits(m, RM.master_tree(sent, mgain), "the master of the sent rows")
    assert_audible(m)
    # a table of srack_voices_set_buses with the same n_buses in its place: the console's settings stay
    p.set_buses(NB, bus[:, 0], gain[:, 0, 0])
    np.testing.assert_array_equal(p.get_master(), mgain)
    assert p.get_sends() is not None
    _, _, _, bm_old = p.render_buses(T)
    assert "[fold]" in p.info()
    m2, _ = p.master(p.send(bm_old))
    assert_same_bits(m2, RM.master_tree(RS.send_tree(bm_old, src, dst, sgain), mgain), "the console behind the old table")
    # ... and back; another n_buses drops them
    p.set_bus_slots(NB, bus, gain)
    np.testing.assert_array_equal(p.get_master(), mgain)
    p.set_bus_slots(NB + 1, bus, gain)
    assert p.get_master() is None and p.get_sends() is None
    _, _, _, bm9 = p.render_buses(T)
    m3, _ = p.master(bm9)
    assert_same_bits(m3, RM.master_tree(bm9, None), "the master after the drop: unit gains")


# ---- 6. the caller's stream --------------------------------------------------------------------------------------------------------------------------------
def test_on_a_stream_with_the_default_stream_busy(S, tmp_path):
    path = str(tmp_path / "slots_stream.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "voice_slots_stream_driver.py"), path], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"the driver failed (rc {r.returncode}):\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    d = np.load(path)
    V, K, NB, CALLS, N = VR.STREAM_CASE
    (bus, gain), (bus2, gain2) = VR.stream_tables()
    print(f"stall {float(d['stall_ms']):.1f} ms; busy {d['busy'].tolist()}; still busy behind the calls that upload nothing {d['busy_after'].tolist()}")
    assert d["busy"].all() and len(d["busy"]) == CALLS, "the default stream was not busy when the calls began"
    assert f" buses={NB}[fold slots={K}]" in str(d["info"])
    # the same calls on the null stream of this process
    q = maker(S, "cfg3", V)()
    q.set_bus_slots(NB, bus, gain)
    for i in range(CALLS):
        if i == 2:
            q.set_bus_slots(NB, bus2, gain2)
        fr, _, _, bm = q.render_buses(N, frames=True)
        np.testing.assert_array_equal(bits(d["frames"][i]), bits(fr), err_msg=f"call {i}: frames")
        np.testing.assert_array_equal(bits(d["bus_mix"][i]), bits(bm), err_msg=f"call {i}: bus mixes")
        b, g = (bus, gain) if i < 2 else (bus2, gain2)
        assert_same_bits(d["bus_mix"][i], VR.slot_reference(d["frames"][i], q.planes()[1], NB, b, g), f"call {i} against the reference")
    assert_audible(d["frames"])
