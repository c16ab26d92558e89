"""The bus sends on the device (srack_buses_send, csrc/sends.hip.h): aux sends from bus to bus, per destination the master section's
three-level sum over its terms, in an order that is part of the ABI.

Rows are seeded f32 values fed straight into srack_buses_send; the reference is tests/sends_ref.py, the sum stated in NumPy (f32
arrays vectorised over time, Python loops over destinations, terms, runs and blocks).  The criterion is BIT EQUALITY (NaN matching
NaN) — derived, not measured: both sides perform the same single-rounded IEEE f32 products and additions in the same order (the
library is built with -ffp-contract=off).  No tolerance anywhere in this file.  Every case asserts that what it compares is not
silent, and from 66 terms on that the reference tree's bits differ from the plain sequential sum's: a kernel that adds in another
order cannot pass."""

import numpy as np
import pytest

import srack_pkg
from tests import master_ref as M
from tests import sends_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-54321.5)  # what d_out holds before a call, wherever the call must not write
GUARD = np.float32(12345.0)      # one float behind d_out


@pytest.fixture(scope="module")
def S():
    return srack_pkg.load()


def assert_same_bits(got, ref, what=""):
    got, ref = np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    ok = R.same_bits(got, ref)
    if not ok.all():
        at = np.argwhere(~ok)
        first = tuple(at[0])
        raise AssertionError(f"{what}: {len(at)} of {ok.size} samples differ, first at {first}: got {got[first]!r} "
                             f"({got.view(np.uint32)[first]:#010x}), reference {ref[first]!r} ({ref.view(np.uint32)[first]:#010x})")


def assert_audible(x, what=""):
    x = np.asarray(x)
    x = np.where(np.isfinite(x), x, 0)
    assert np.abs(x).max() > 1e-3 and np.count_nonzero(x) > x.size // 4, f"{what}: (nearly) silent — the comparison would show nothing"


def assert_tree_matters(seq_row, ref_row, what=""):
    """from 66 terms on the tree is not the sequential sum: a share of the destination's samples that no accident explains must differ
    (at 66 terms only the last two are added in another order; from 129 on nearly all samples differ)"""
    differ = np.count_nonzero(~R.same_bits(seq_row, ref_row))
    assert differ >= max(1, ref_row.size // 8), f"{what}: the tree and the sequential sum differ in {differ} of {ref_row.size} samples only"


def host(S, n_buses, channels=2):
    """a handle to hang the table on: an oscillator into every channel, one voice in bus 0 of n_buses (never rendered here)"""
    p = S.Patch(48000, 64, channels)
    osc, out = p.add_module(S.MOD_OSCILLATOR), p.add_module(S.MOD_OUTPUT)
    for c in range(channels):
        p.connect(osc, S.OSC_OUT_SINE, out, c)
    p.configure_voices(1)
    p.set_buses(n_buses)
    return p


def run_raw(S, p, rows, offset_in=0, offset_out=None):
    """as Patch.send, with d_rows and d_out `offset_in` / `offset_out` floats into their allocations, d_out holding SENTINEL beforehand
    (it comes back wherever the call did not write) and one guard float behind it"""
    lib = S.lib
    offset_out = offset_in if offset_out is None else offset_out
    x = np.ascontiguousarray(rows, dtype=np.float32)
    out = np.full(x.size + 1, SENTINEL, dtype=np.float32)
    out[-1] = GUARD
    with S.DeviceScope() as dev:
        a_in, a_out = dev.upload(x, offset_in), dev.upload(out, offset_out)
        p.send_raw(x.shape[2], a_in, x.shape[1], a_out, None)
        dev.download(out, a_out)
    assert out[-1] == GUARD, "the call wrote past d_out"
    return out[:-1].reshape(x.shape)


def run_cut(p, rows, cuts):
    """rows through srack_buses_send in calls of `cuts` samples"""
    assert sum(cuts) == rows.shape[2]
    out, at = [], 0
    for n in cuts:
        out.append(p.send(rows[:, :, at:at + n]))
        at += n
    return np.concatenate(out, axis=2)


# ---- the mixed table: 130 buses, four aux destinations with 1, 64, 65 and 129 terms, the rest through-only ------------------------
NB = 130
AUX = {3: 1, 50: 64, 77: 65, 129: 129}  # destination: terms, the through term included


def mixed_table(seed=7):
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for d, n in AUX.items():
        s = rng.integers(0, NB, n - 1)
        src += s.tolist()
        dst += [d] * (n - 1)
    src, dst = np.array(src, dtype=np.intc), np.array(dst, dtype=np.intc)
    at = {d: np.flatnonzero(dst == d) for d in AUX}
    src[at[50][:3]] = (129, 77, 3)        # sources that are aux buses themselves: the input is read, not the output
    src[at[129][:3]] = (50, 77, 129)      # ... the last of them src == dst
    src[at[77][:4]] = (77, 77, 12, 12)    # src == dst twice, and a duplicate pair
    src[at[129][60:70]] = 12              # ... ten more duplicates, across the first run's end
    order = rng.permutation(len(src))     # the list is not sorted by destination
    src, dst = src[order], dst[order]
    gain = rng.uniform(-2.0, 2.0, (len(src), 2)).astype(np.float32)
    through = rng.uniform(-2.0, 2.0, (NB, 2)).astype(np.float32)
    assert (np.diff(dst) < 0).any() and len(set(zip(src.tolist(), dst.tolist()))) < len(src) and (src == dst).any()
    return src, dst, gain, through


_MIXED = {}


def mixed_case(T=4099, rc=2):
    """rows, the table and the reference over T samples, computed once: a shorter call is the first samples of it (every sample is on
    its own)"""
    key = (T, rc)
    if key not in _MIXED:
        src, dst, gain, through = mixed_table()
        rows, _ = R.case_inputs(NB, T, seed=1800 + T, row_channels=rc)
        ref = R.send_tree(rows, src, dst, gain, through)
        seq = R.send_sequential(rows, src, dst, gain, through, only=list(AUX))
        for a in (rows, ref, seq):
            a.setflags(write=False)
        _MIXED[key] = (rows, src, dst, gain, through, ref, seq)
    return _MIXED[key]


def mixed_host(S):
    p = host(S, NB)
    p.set_sends(*mixed_table())
    return p


# ---- 1: the order of the additions --------------------------------------------------------------------------------
@pytest.mark.parametrize("n_terms,T", [(1, 70), (2, 70), (63, 70), (64, 70), (65, 70), (66, 70), (128, 70), (129, 70), (4096, 70), (4097, 70),
                                       (8193, 70), (65536, 64)])
def test_order_of_additions(S, n_terms, T):
    """bus 0 fed by every other bus: n_buses = the term count.  (One term cannot be had that way — a list without sends is no list —:
    there two buses, bus 0 sending to bus 1, and bus 0 is the destination of one term.)"""
    n_buses = max(2, n_terms)
    rows, g = R.case_inputs(n_buses, T)
    src, dst = R.all_to_one(n_buses) if n_terms > 1 else (np.array([0], dtype=np.intc), np.array([1], dtype=np.intc))
    gain, through = g[1:] if n_terms > 1 else g[:1], g
    ref = R.send_tree(rows, src, dst, gain, through)
    assert_audible(ref[0], f"{n_terms} terms")
    seq0 = R.send_sequential(rows, src, dst, gain, through, only=[0])[0]
    if n_terms <= 65:
        assert_same_bits(seq0, ref[0], "up to 65 terms the tree is the sequential sum")
    else:
        assert_tree_matters(seq0, ref[0], f"{n_terms} terms")
    p = host(S, n_buses)
    assert "sends=" not in p.info()
    p.set_sends(src, dst, gain, through)
    nt, order, runs = p.send_plan()
    assert nt[0] == n_terms and runs == (n_terms + 63) // 64 + n_buses - 1  # (every other bus is one run)
    got = p.send(rows)
    assert_same_bits(got, ref, f"{n_terms} terms")
    assert f" sends={len(src)}[{runs} runs]" in p.info()


# ---- 2: a mixed table ---------------------------------------------------------------------------------------------
def test_mixed_table(S):
    rows, src, dst, gain, through, ref, seq = mixed_case()
    rows, ref, seq = rows[:, :, :70], ref[:, :, :70], seq[:, :, :70]
    nt, order = R.grouping(NB, dst)
    runs = R.n_runs(nt)
    assert {d: int(nt[d]) for d in AUX} == AUX and nt.sum() == NB + len(src) and runs == NB - 4 + 1 + 1 + 2 + 3
    assert_audible(ref, "the mixed table")
    for d, n in AUX.items():
        if n <= 65:
            assert_same_bits(seq[d], ref[d], f"aux {d}: up to 65 terms the tree is the sequential sum")
        else:
            assert_tree_matters(seq[d], ref[d], f"aux {d}")
    # the sends out of aux buses carry the INPUT rows: a reference fed its own output for those sources gives other bits
    fed_back = rows.copy()
    fed_back[list(AUX)] = ref[list(AUX)]
    assert not R.same_bits(R.send_tree(fed_back, src, dst, gain, through, only=[50, 129])[[50, 129]], ref[[50, 129]]).all()
    p = mixed_host(S)
    got_nt, got_order, got_runs = p.send_plan()
    np.testing.assert_array_equal(got_nt, nt)
    np.testing.assert_array_equal(got_order, order)
    assert got_runs == runs
    got = run_raw(S, p, rows)
    assert_same_bits(got, ref, "the mixed table")
    assert f" sends={len(src)}[{runs} runs]" in p.info()


# ---- 3: lengths and alignment --------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("T", [1, 3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1026, 1027, 1028, 4099])
def test_lengths_and_alignment(S, T, offset):
    """the mixed table; offset 1 .. 3: rows and out that many floats into their allocations, so no row is 16-byte aligned.  With offset
    0 the lengths that are multiples of four take the four-samples-per-lane kernel, below, at and past one workgroup's 1 024 samples."""
    rows, src, dst, gain, through, ref, seq = mixed_case()
    rows, ref = np.ascontiguousarray(rows[:, :, :T]), ref[:, :, :T]
    if T >= 63:
        assert_audible(ref, f"T = {T}")
        assert_tree_matters(seq[129, :, :T], ref[129], f"T = {T}")
    else:
        assert np.abs(ref).max() > 1e-3
    p = mixed_host(S)
    got = run_raw(S, p, rows, offset)
    assert_same_bits(got, ref, f"T = {T}, offset {offset}")


@pytest.mark.parametrize("offset_in,offset_out", [(0, 1), (2, 0), (4, 8), (4, 3)])
def test_rows_and_out_aligned_apart(S, offset_in, offset_out):
    """T % 4 == 0 and only one of the two bases 16-byte aligned: one sample per lane; both 16 bytes in: four"""
    rows, src, dst, gain, through, ref, seq = mixed_case()
    rows, ref = np.ascontiguousarray(rows[:, :, :1028]), ref[:, :, :1028]
    got = run_raw(S, mixed_host(S), rows, offset_in, offset_out)
    assert_same_bits(got, ref, f"rows {offset_in} floats in, out {offset_out}")
    assert_audible(ref, "aligned apart")


# ---- 4: row channels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [130, 132])
@pytest.mark.parametrize("rc", [1, 2, 3])
def test_row_channels(S, rc, T):
    rows, src, dst, gain, through, ref, seq = mixed_case(132, rc)
    rows, ref, seq = np.ascontiguousarray(rows[:, :, :T]), ref[:, :, :T], seq[:, :, :T]
    used = min(rc, 2)
    assert_audible(ref[:, :used], f"{rc} row channels")
    assert_tree_matters(seq[129, :used], ref[129, :used], f"{rc} row channels")
    p = mixed_host(S)
    got = run_raw(S, p, rows)
    assert_same_bits(got[:, :used], ref[:, :used], f"{rc} row channels")
    if rc == 3:
        assert (got[:, 2] == SENTINEL).all(), "the third channel's rows of d_out were written"
        other = rows.copy()
        other[:, 2] = np.nan  # ... and the third channel's rows of d_rows are not read
        assert_same_bits(run_raw(S, p, other)[:, :2], ref[:, :2], "another third channel")
    assert (got[:, :used] != SENTINEL).all()


# ---- 5: cuts ----------------------------------------------------------------------------------------------------
def test_however_the_samples_are_cut(S):
    cuts = [1, 7, 63, 64, 65, 300, 524]
    rows, src, dst, gain, through, ref, seq = mixed_case()
    T = sum(cuts)
    rows, ref = np.ascontiguousarray(rows[:, :, :T]), ref[:, :, :T]
    p, q = mixed_host(S), mixed_host(S)
    one, cut = p.send(rows), run_cut(q, rows, cuts)
    assert_same_bits(cut, one, f"in calls of {cuts}")
    assert_same_bits(one, ref, "one call")
    assert_audible(one, "cutting")
    assert_tree_matters(seq[129, :, :T], ref[129], "cutting")


# ---- 6: non-finite values reach the destinations they are sent to ----------------------------------------------------
def test_nonfinite_values_reach_their_destinations_only(S):
    rows, src, dst, gain, through, ref, seq = mixed_case()
    T = 200
    rows, clean = rows[:, :, :T].copy(), ref[:, :, :T]
    p = mixed_host(S)
    assert_same_bits(p.send(rows), clean, "the finite case")
    assert np.isfinite(clean).all()
    assert_audible(clean, "non-finite")

    def reached(s):
        """the destinations bus s reaches: itself (its through term) and wherever it is sent"""
        return sorted({s} | set(dst[src == s].tolist()))

    # a NaN sample in bus 12 (sent to 77 twice and to 129): exactly that channel and sample of the buses it reaches
    assert set(reached(12)) >= {12, 77, 129}
    bad = rows.copy()
    bad[12, 1, 123] = np.nan
    got, want = p.send(bad), R.send_tree(bad, src, dst, gain, through)
    where = np.zeros(got.shape, dtype=bool)
    where[reached(12), 1, 123] = True
    assert np.isnan(got[where]).all() and np.isfinite(got[~where]).all() and (R.same_bits(got, clean) | where).all()
    assert_same_bits(got, want, "a NaN sample")
    # an inf row with gain 0: bus 5's row is inf, every gain on it 0 — through and sends: NaN (0 * inf) wherever it reaches, nowhere else
    g0, t0 = gain.copy(), through.copy()
    src5 = src.copy()
    src5[np.flatnonzero(dst == 50)[5]] = 5  # (bus 5 is sent to aux 50 for certain)
    g0[src5 == 5] = 0.0
    t0[5] = 0.0
    inf_rows = rows.copy()
    inf_rows[5] = np.inf
    p.set_sends(src5, dst, g0, t0)
    got, want = p.send(inf_rows), R.send_tree(inf_rows, src5, dst, g0, t0)
    nan_at = np.isnan(got).all(axis=(1, 2))
    assert sorted(np.flatnonzero(nan_at).tolist()) == sorted({5} | set(dst[src5 == 5].tolist())) and 50 in np.flatnonzero(nan_at)
    assert np.isfinite(got[~nan_at]).all()
    assert_same_bits(got, want, "an inf row with gain 0")
    # a NaN gain on channel 0 of one send: that destination's channel 0, nothing else
    gn = gain.copy()
    k = int(np.flatnonzero(dst == 129)[70])
    gn[k, 0] = np.nan
    p.set_sends(src, dst, gn, through)
    got = p.send(rows)
    where = np.zeros(got.shape, dtype=bool)
    where[129, 0] = True
    assert np.isnan(got[where]).all() and np.isfinite(got[~where]).all() and (R.same_bits(got, clean) | where).all()
    assert_same_bits(got, R.send_tree(rows, src, dst, gn, through), "a NaN gain")


# ---- 7: negative zeros, and the defaults -----------------------------------------------------------------------------
def test_negative_zero_rows_through_a_bus_without_sends(S):
    rows, src, dst, gain, through, ref, seq = mixed_case()
    rows = rows[:, :, :70].copy()
    rows[[10, 11]] = -0.0  # (neither is sent anywhere in a way that matters here: both are read through their own term)
    t1 = through.copy()
    t1[10], t1[11] = 1.0, -1.0  # -0.0 * 1 = -0.0, -0.0 * -1 = +0.0: +0.0 + either is +0.0
    p = host(S, NB)
    p.set_sends(src, dst, gain, t1)
    got = run_raw(S, p, rows)
    assert (got[[10, 11]].view(np.uint32) == 0).all(), "a row of -0.0 through a bus without sends must come out +0.0"
    assert_same_bits(got, R.send_tree(rows, src, dst, gain, t1), "negative zeros")
    assert_audible(got, "negative zeros")


@pytest.mark.parametrize("no_gain,no_through", [(True, True), (True, False), (False, True)])
def test_null_gain_and_null_through_are_ones(S, no_gain, no_through):
    rows, src, dst, gain, through, ref, seq = mixed_case()
    rows = np.ascontiguousarray(rows[:, :, :70])
    g, t = (None if no_gain else gain), (None if no_through else through)
    p = host(S, NB)
    p.set_sends(src, dst, g, t)
    want = R.send_tree(rows, src, dst, g, t)
    ones = R.send_tree(rows, src, dst, np.ones_like(gain) if no_gain else gain, np.ones_like(through) if no_through else through)
    assert_same_bits(want, ones, "the reference's defaults")
    assert not R.same_bits(want, ref[:, :, :70]).all()
    assert_same_bits(p.send(rows), want, f"gain NULL: {no_gain}, through NULL: {no_through}")
    assert_audible(want, "defaults")


# ---- 8: the all-to-one table is the master --------------------------------------------------------------------------
@pytest.mark.parametrize("n_buses", [66, 129, 4097])
def test_all_to_one_is_the_master(S, n_buses):
    rows, g = R.case_inputs(n_buses, 70, seed=81)
    src, dst = R.all_to_one(n_buses)
    p = host(S, n_buses)
    p.set_sends(src, dst, g[1:], g)
    p.set_master(g)
    sent, (master, _) = p.send(rows), p.master(rows)
    assert_audible(master, f"{n_buses} buses")
    assert_same_bits(sent[0], master, "row 0 of the sends against srack_buses_master")
    assert_same_bits(master, M.master_tree(rows, g), "... and the master against its reference")
    assert_tree_matters(M.master_sequential(rows, g), master, f"{n_buses} buses")
    info = p.info()
    assert info.index(" sends=") < info.index(" master=")


# ---- 9: the reference's mixer ---------------------------------------------------------------------------------------
def test_against_the_mixer_module(S, oracle):
    """four oscillators into a MonoMixerModule with four gains (the oracle) = four voices of one oscillator, a bus each at gain 1, buses
    1 .. 3 sent to bus 0 with the mixer's gains 1 .. 3 and bus 0's through gain the mixer's gain 0 — bit for bit, in the exact render mode"""
    T = 512
    vals = [-1.0, 0.37, 1.25, -2.5]
    gains = np.array([0.7, -1.3, 0.05, 1.9], dtype=np.float32)
    o = oracle.OraclePatch(48000, 64, 2)
    oscs = [o.add_module(S.MOD_OSCILLATOR) for _ in range(4)]
    mix, out = o.add_module(S.MOD_MONO_MIXER), o.add_module(S.MOD_OUTPUT)
    for k, (osc, v) in enumerate(zip(oscs, vals)):
        o.set_field(osc, S.OSC_VAL, v)
        o.connect(osc, S.OSC_OUT_SINE, mix, k)
        o.set_field(mix, S.MIX_GAIN0 + k, float(gains[k]))
    o.connect(mix, 0, out, 0)
    ref = np.asarray(o.render(T), dtype=np.float32)
    p = S.Patch(48000, 64, 2)
    osc, out = p.add_module(S.MOD_OSCILLATOR), p.add_module(S.MOD_OUTPUT)
    p.connect(osc, S.OSC_OUT_SINE, out, 0)
    p.configure_voices(4)
    p.set_voice_field(osc, S.OSC_VAL, np.array(vals, dtype=np.float32))
    p.set_buses(4, np.arange(4, dtype=np.intc), np.ones(4, dtype=np.float32))
    _, _, _, bm = p.render_buses(T, flags=S.RENDER_EXACT_OSC)
    src, dst = np.array([1, 2, 3], dtype=np.intc), np.zeros(3, dtype=np.intc)
    gain = np.stack([gains[1:], np.ones(3, dtype=np.float32)], axis=1)
    through = np.ones((4, 2), dtype=np.float32)
    through[0, 0] = gains[0]
    p.set_sends(src, dst, gain, through)
    got = p.send(bm)
    assert_audible(ref[0], "the mixer")
    assert_same_bits(got[0, 0], ref[0], "the sends against MonoMixerModule")
    assert_same_bits(got, R.send_tree(bm, src, dst, gain, through), "... and against the NumPy tree")
    assert not got[:, 1].any()  # (channel 1 is not wired)


# ---- 10: end to end, and nothing else moves -------------------------------------------------------------------------
def test_end_to_end_and_nothing_else_moves(S):
    """P1 at 2000 Hz, 140 voices in 70 buses — 68 group buses and two aux buses that carry the rooms —, 600 samples in two calls with
    another send list for the second: render_buses -> send -> reverb (the aux buses only) -> master, every stage against its reference
    on the previous stage's output; everything a render writes, the voice state and the kernel are what a twin handle gives that
    never heard of sends"""
    from tests.test_gpu_bus_reverb import ROOMS, DEFAULTS, new_reverb, tick
    from tests.test_gpu_mix_buses import all_fields
    sr, V, NBUS, n = 2000, 140, 70, 300
    aux = (68, 69)
    rng = np.random.default_rng(18)
    bus = (np.arange(V) % 68).astype(np.intc)  # (no voice sits in an aux bus: what the rooms hear is what is sent there)
    vgain = rng.uniform(0.2, 0.9, V).astype(np.float32)
    det = rng.uniform(-1.0, 1.0, V).astype(np.float32)
    params = np.tile(np.array(DEFAULTS), (NBUS, 1))
    params[68], params[69] = ROOMS[0], ROOMS[3]
    enabled = np.zeros(NBUS, dtype=np.intc)
    enabled[list(aux)] = 1
    mgain = rng.uniform(-2.0, 2.0, (NBUS, 2)).astype(np.float32)
    # every group bus sends to one aux bus, every fourth to both; the second list is shorter, in another order, with other gains
    lists = []
    for k in range(2):
        s = np.concatenate([np.arange(68), np.arange(0, 68, 4)]) if k == 0 else np.arange(67, 10, -1)
        d = np.concatenate([68 + np.arange(68) % 2, 69 - np.arange(0, 68, 4) % 2]) if k == 0 else 68 + (np.arange(67, 10, -1) // 3) % 2
        g = rng.uniform(0.1, 0.6, (len(s), 2)).astype(np.float32)
        t = rng.uniform(0.5, 1.0, (NBUS, 2)).astype(np.float32)
        lists.append((s.astype(np.intc), d.astype(np.intc), g, t))

    def make():
        p = S.Patch(sr, 64, 2)
        ids = S.build_p1(p, lfo_val=0.0)
        p.configure_voices(V)
        p.set_voice_field(ids["osc_a"], S.OSC_VAL, det)
        p.set_buses(NBUS, bus, vgain)
        p.set_bus_reverbs(params, enabled)
        p.set_master(mgain)
        return p

    p, q = make(), make()
    assert "sends=" not in p.info()
    bms, sents, fxs, masters = [], [], [], []
    for k in range(2):
        p.set_sends(*lists[k])
        rp = p.render_buses(n, frames=True, mix=True, stats=True)
        rq = q.render_buses(n, frames=True, mix=True, stats=True)
        for what, x, y in zip(("frames", "mix", "statistics", "bus mixes"), rp, rq):
            np.testing.assert_array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8), err_msg=f"call {k}: {what} moved")
        sent = p.send(rp[3])
        fx_p, fx_q = p.bus_reverb(sent), q.bus_reverb(rq[3])
        m, _ = p.master(fx_p)
        q.master(fx_q)
        ip, iq = p.info(), q.info()
        note = f" sends={len(lists[k][0])}[{NBUS} runs]"  # (at most 52 terms in any bus: a run each)
        assert "sends=" not in iq and note in ip and ip.replace(note, "") == iq
        assert ip.split(" sends=")[0] == iq.split(" busfx=")[0] and ip.split("kernel=")[-1] == iq.split("kernel=")[-1] and "kernel=" in ip
        assert ip.index(" buses=") < ip.index(" sends=") < ip.index(" busfx=") < ip.index(" master=") < ip.index(" kernel=")
        bms.append(rp[3]), sents.append(sent), fxs.append(fx_p), masters.append(m)
    want, got = all_fields(S, q), all_fields(S, p)
    assert len(want) >= 8 and got.keys() == want.keys()
    for key in want:
        np.testing.assert_array_equal(got[key].view(np.uint64), want[key].view(np.uint64), err_msg=f"module {key[0]} field {key[1]}")
    # stage by stage, each on the previous stage's output
    for k in range(2):
        assert_audible(bms[k][:68], f"call {k}: the bus mixes")
        assert not bms[k][68:].any()
        assert_same_bits(sents[k], R.send_tree(bms[k], *lists[k]), f"call {k}: the sends of the bus mixes")
        assert_audible(sents[k][68:], f"call {k}: what the aux buses hear")
        assert_same_bits(masters[k], M.master_tree(fxs[k], mgain), f"call {k}: the master of the fx rows")
        assert_audible(masters[k], f"call {k}: the master")
    sent, fx = np.concatenate(sents, axis=2), np.concatenate(fxs, axis=2)
    for b in range(NBUS):  # the rooms' tails carry on over the change of the list; a bus without a room is copied
        assert_same_bits(fx[b], tick(new_reverb(sr, params[b]), sent[b]) if enabled[b] else sent[b], f"bus {b} through the reverbs")
    assert_audible(fx[68:], "the rooms")


# ---- 11: determinism ------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(S):
    rows, src, dst, gain, through, ref, seq = mixed_case()
    rows = np.ascontiguousarray(rows[:, :, :1028])
    outs = [mixed_host(S).send(rows) for _ in range(2)]
    np.testing.assert_array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert_audible(outs[0], "determinism")
