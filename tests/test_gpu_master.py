"""The master section on the device (srack_buses_master, csrc/master.hip.h): a gain per bus and channel, the buses summed to one stereo
pair in an order that is part of the ABI, and the statistics of the result.

Rows are seeded f32 values fed straight into srack_buses_master; the reference is tests/master_ref.py, the three-level sum stated in
NumPy (f32 arrays vectorised over time, Python loops over buses, runs and blocks).  The criterion is BIT EQUALITY (NaN matching NaN)
— derived, not measured: both sides perform the same single-rounded IEEE f32 products and additions in the same order (the library
is built with -ffp-contract=off), and the statistics the same f64 operations in sample order.  No tolerance anywhere in this file.
Every case asserts that what it compares is not silent, and from 66 buses on that the reference tree's bits differ from the plain
sequential sum's: a kernel that adds in another order cannot pass."""

import numpy as np
import pytest

import srack_pkg
from tests import master_ref as R

pytestmark = pytest.mark.gpu


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


def assert_same_stats(got, ref, what=""):
    np.testing.assert_array_equal(np.asarray(got).view(np.uint64), np.asarray(ref).view(np.uint64), err_msg=what)


def assert_audible(x, what=""):
    x = np.asarray(x)
    x = np.where(np.isfinite(x), x, 0)
    assert np.abs(x).max() > 1e-3 and np.count_nonzero(x) > x.size // 4, f"{what}: (nearly) silent — the comparison would show nothing"


def assert_tree_matters(rows, gain, ref, what=""):
    """from 66 buses on the tree is not the sequential sum: a share of the samples that no accident explains must differ (at 66 buses
    only the last two buses are added in another order: about half the samples; from 129 on nearly all)"""
    used = min(rows.shape[1], 2)
    seq = R.master_sequential(rows, gain)
    differ = np.count_nonzero(~R.same_bits(seq[:used], ref[:used]))
    assert differ >= max(1, ref[:used].size // 8), f"{what}: the tree and the sequential sum differ in {differ} of {ref[:used].size} samples only"


def host(S, n_buses, channels=2):
    """a handle to hang the table on: an oscillator into every channel, one voice in bus 0 of n_buses (never rendered here)"""
    p = S.Patch(48000, 64, channels)
    osc, out = p.add_module(S.MOD_OSCILLATOR), p.add_module(S.MOD_OUTPUT)
    for c in range(channels):
        p.connect(osc, S.OSC_OUT_SINE, out, c)
    p.configure_voices(1)
    p.set_buses(n_buses)
    return p


def run_cut(p, rows, cuts, stats=None):
    """rows through srack_buses_master in calls of `cuts` samples, the statistics buffer carried from call to call"""
    assert sum(cuts) == rows.shape[2]
    out, at = [], 0
    for n in cuts:
        m, stats = p.master(rows[:, :, at:at + n], stats)
        out.append(m)
        at += n
    return np.concatenate(out, axis=1), stats


def run_offset(S, p, rows, offset, stats=None):
    """as Patch.master, with d_rows and d_master each `offset` floats into their allocations"""
    lib = S.lib
    x = np.ascontiguousarray(rows, dtype=np.float32)
    T = x.shape[2]
    buf = np.zeros(2 * T + 1, dtype=np.float32)
    buf[-1] = 12345.0  # one float behind the master: the call must not write it
    st = None if stats is None else np.array(stats, dtype=np.float64)
    with S.DeviceScope() as dev:
        a_in, a_out = dev.upload(x, offset), dev.upload(buf, offset)
        d_st = None if st is None else dev.upload(st)
        p.master_raw(T, a_in, x.shape[1], a_out, d_st, None)
        dev.download(buf, a_out)
        if st is not None:
            dev.download(st, d_st)
    assert buf[-1] == 12345.0, "the call wrote past d_master"
    return buf[:-1].reshape(2, T), st


START = np.array([[1.5, 2.25, 0.75, 0.125, 3.0, 2.0], [-0.5, 10.0, 0.0, 1.25, 0.0, 7.0]])  # a statistics buffer that is not zeros


# ---- 1: the order of the additions --------------------------------------------------------------------------------
@pytest.mark.parametrize("n_buses,T", [(1, 70), (2, 70), (63, 70), (64, 70), (65, 70), (66, 70), (128, 70), (129, 70), (4095, 70), (4096, 70),
                                       (4097, 70), (8193, 70), (61441, 67), (65536, 67)])
def test_order_of_additions(S, n_buses, T):
    rows, gain = R.case_inputs(n_buses, T)
    ref = R.master_tree(rows, gain)
    assert_audible(ref, f"{n_buses} buses")
    if n_buses <= 65:
        assert_same_bits(R.master_sequential(rows, gain), ref, "up to 65 buses the tree is the sequential sum")
    else:
        assert_tree_matters(rows, gain, ref, f"{n_buses} buses")
    p = host(S, n_buses)
    assert "master=" not in p.info()
    p.set_master(gain)
    got, st = p.master(rows, np.zeros((2, 6)))
    assert_same_bits(got, ref, f"{n_buses} buses")
    assert_same_stats(st, R.stats_sequential(ref), f"{n_buses} buses: statistics")
    assert f" master={n_buses}[{(n_buses + 63) // 64} runs]" in p.info()
    if n_buses <= 129:  # without gains set: 1.0f everywhere
        q = host(S, n_buses)
        got1, none = q.master(rows)
        assert none is None and q.get_master() is None
        assert_same_bits(got1, R.master_tree(rows), f"{n_buses} buses, no gains set")


# ---- 2: lengths and alignment --------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("T", [1, 3, 63, 64, 65, 255, 257, 1021, 4099])
def test_lengths_and_alignment(S, T, offset):
    """130 buses (two full runs and a run of two); offset 1: rows and master one float into their allocations, so no row is 16-byte aligned"""
    rows, gain = R.case_inputs(130, T, seed=1701 + T)
    ref = R.master_tree(rows, gain)
    assert_audible(ref, f"T = {T}")
    assert_tree_matters(rows, gain, ref, f"T = {T}")
    p = host(S, 130)
    p.set_master(gain)
    got, st = run_offset(S, p, rows, offset, START)
    assert_same_bits(got, ref, f"T = {T}, offset {offset}")
    assert_same_stats(st, R.stats_sequential(ref, START), f"T = {T}, offset {offset}: statistics")


@pytest.mark.parametrize("T", [64, 1024, 4100])
def test_aligned_rows_of_every_length_class(S, T):
    """n_samples % 4 == 0 from an aligned base: the four-samples-per-lane path, below, at and past one workgroup's 1 024 samples"""
    rows, gain = R.case_inputs(130, T, seed=9 + T)
    ref = R.master_tree(rows, gain)
    assert_tree_matters(rows, gain, ref, f"T = {T}")
    p = host(S, 130)
    p.set_master(gain)
    got, _ = run_offset(S, p, rows, 0)
    assert_same_bits(got, ref, f"T = {T}")
    got4, _ = run_offset(S, p, rows, 4)  # (16 bytes in: still aligned)
    assert_same_bits(got4, ref, f"T = {T}, four floats in")


# ---- 3: row channels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [1, 2, 3])
def test_row_channels(S, rc):
    n_buses, T = 70, 130
    rows, gain = R.case_inputs(n_buses, T, seed=30 + rc, row_channels=rc)
    if rc == 1:
        gain[:, 1] = np.inf  # no product is taken for channel 1: an inf gain there makes nothing NaN
    ref = R.master_tree(rows, gain)
    assert_audible(ref[:min(rc, 2)], f"{rc} row channels")
    assert_tree_matters(rows, gain, ref, f"{rc} row channels")
    p = host(S, n_buses)
    p.set_master(gain)
    got, st = p.master(rows, START)
    assert_same_bits(got, ref, f"{rc} row channels")
    assert_same_stats(st, R.stats_sequential(ref, START, channels=min(rc, 2)), f"{rc} row channels: statistics")
    if rc == 1:
        assert (got[1].view(np.uint32) == 0).all()  # +0.0 throughout
        assert_same_stats(st[1], START[1], "channel 1's statistics row is left alone")
        assert not np.array_equal(st[0], START[0])
    if rc == 3:
        other = rows.copy()
        other[:, 2] = np.random.default_rng(5).uniform(-1, 1, (n_buses, T)).astype(np.float32)
        got2, _ = p.master(other)
        assert_same_bits(got2, got, "another third channel")


# ---- 4: cuts ----------------------------------------------------------------------------------------------------
def test_however_the_samples_are_cut(S):
    cuts = [1, 7, 63, 64, 65, 300]
    rows, gain = R.case_inputs(130, sum(cuts), seed=44)
    rows[:, :, 5::37] *= np.float32(40.0)  # (some master samples above 1 in magnitude: CLIPPED moves)
    p, q = host(S, 130), host(S, 130)
    p.set_master(gain)
    q.set_master(gain)
    one, st_one = p.master(rows, START)
    cut, st_cut = run_cut(q, rows, cuts, START)
    assert_same_bits(cut, one, f"in calls of {cuts}")
    assert_same_stats(st_cut, st_one, f"statistics carried through calls of {cuts}")
    ref = R.master_tree(rows, gain)
    assert_same_bits(one, ref, "one call")
    assert_same_stats(st_one, R.stats_sequential(ref, START), "one call: statistics")
    assert st_one[0, R.STAT_CLIPPED] > START[0, R.STAT_CLIPPED]
    assert_audible(one, "cutting")
    assert_tree_matters(rows, gain, ref, "cutting")


# ---- 5: statistics -----------------------------------------------------------------------------------------------
def test_statistics_with_special_values(S):
    n_buses, T = 3, 300  # (gain 1 on three buses: the master holds the special values themselves)
    rng = np.random.default_rng(51)
    rows = np.zeros((n_buses, 2, T), dtype=np.float32)
    rows[0] = rng.uniform(-1.6, 1.6, (2, T)).astype(np.float32)
    rows[1, :, ::3] = rng.uniform(-0.2, 0.2, (2, (T + 2) // 3)).astype(np.float32)
    rows[0, 0, 10], rows[0, 0, 11], rows[0, 0, 12], rows[0, 1, 70] = np.nan, np.inf, -np.inf, np.nan
    rows[2, 0, 200], rows[2, 1, 201] = np.inf, -np.inf
    rows[:, :, 64] = -0.0
    rows[:, :, 299] = (np.float32(-3.0), np.float32(2.5))
    ref = R.master_tree(rows)
    assert np.isnan(ref[0, 10]) and ref[0, 11] == np.inf and ref[0, 12] == -np.inf and ref[0, 200] == np.inf and ref[1, 201] == -np.inf
    assert (ref[:, 64].view(np.uint32) == 0).all() and (np.abs(ref[np.isfinite(ref)]) > 1).sum() > 50
    want = R.stats_sequential(ref, START)
    assert want[0, R.STAT_NONFINITE] == START[0, R.STAT_NONFINITE] + 4 and want[1, R.STAT_NONFINITE] == START[1, R.STAT_NONFINITE] + 2
    assert want[0, R.STAT_PEAK_NEG] == 9.0 and want[1, R.STAT_PEAK_POS] == 7.5
    assert want[0, R.STAT_CLIPPED] > START[0, R.STAT_CLIPPED] + 50
    p = host(S, n_buses)
    got, st = p.master(rows, START)
    assert_same_bits(got, ref, "special values")
    assert_same_stats(st, want, "statistics of special values")
    # from zeros, and a call of statistics only moves what the statistics say: NULL statistics leave the master's bits alone
    got0, st0 = p.master(rows, np.zeros((2, 6)))
    assert_same_stats(st0, R.stats_sequential(ref), "from zeros")
    got_none, _ = p.master(rows)
    assert_same_bits(got0, got, "statistics on")
    assert_same_bits(got_none, got, "statistics off")


# ---- 6: non-finite values stay local --------------------------------------------------------------------------
def test_nonfinite_values_stay_local(S):
    n_buses, T = 130, 200
    rows, gain = R.case_inputs(n_buses, T, seed=66)
    rows[77, :, 40:60] = 0.0  # (zeros for the inf gain below)
    p = host(S, n_buses)
    p.set_master(gain)
    clean, _ = p.master(rows)
    assert_same_bits(clean, R.master_tree(rows, gain), "the finite case")
    assert np.isfinite(clean).all()
    # one NaN sample in one bus and channel: exactly that master sample
    bad = rows.copy()
    bad[100, 1, 123] = np.nan
    got, st = p.master(bad, np.zeros((2, 6)))
    where = np.zeros((2, T), dtype=bool)
    where[1, 123] = True
    assert np.isnan(got[where]).all() and (R.same_bits(got, clean) | where).all() and np.isfinite(got[~where]).all()
    assert st[0, R.STAT_NONFINITE] == 0 and st[1, R.STAT_NONFINITE] == 1
    # an inf gain on a bus whose row holds zeros: NaN at those zeros (0 * inf), inf elsewhere in that channel, the other channel as it was
    g2 = gain.copy()
    g2[77, 0] = np.inf
    p.set_master(g2)
    got, _ = p.master(rows)
    assert np.isnan(got[0, 40:60]).all() and np.isinf(got[0, :40]).all() and np.isinf(got[0, 60:]).all()
    assert_same_bits(got[1], clean[1], "the other channel")
    assert_same_bits(got, R.master_tree(rows, g2), "an inf gain")
    assert_audible(clean, "non-finite")


# ---- 7: the reference's mixer ---------------------------------------------------------------------------------------
def test_against_the_mixer_module(S, oracle):
    """four oscillators into a MonoMixerModule with four gains (the oracle) = four voices of one oscillator, a bus each at gain 1,
    through the master with the mixer's gains — bit for bit, in the exact render mode"""
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
    p.set_master(np.stack([gains, np.ones(4, dtype=np.float32)], axis=1))
    got, _ = p.master(bm)
    assert_audible(ref[0], "the mixer")
    assert_same_bits(got[0], ref[0], "the master against MonoMixerModule")
    assert_same_bits(got[0], R.master_tree(bm, p.get_master())[0], "... and against the NumPy tree")
    assert not got[1].any()  # (channel 1 is not wired)


# ---- 8: end to end, and nothing else moves -------------------------------------------------------------------------
def test_end_to_end_and_nothing_else_moves(S):
    """P1 at 2000 Hz, 130 voices in 66 buses, two of them with reverbs, 600 samples in two calls: render_buses -> reverb -> master is the
    NumPy chain on the returned bus mixes; everything a render or the reverbs write, the voice state and the kernel are what a twin
    handle gives that never heard of the master"""
    from tests.test_gpu_bus_reverb import ROOMS, DEFAULTS, new_reverb, tick
    from tests.test_gpu_mix_buses import all_fields
    sr, V, NB, n = 2000, 130, 66, 300
    rng = np.random.default_rng(88)
    bus = (np.arange(V) % NB).astype(np.intc)
    vgain = rng.uniform(0.2, 0.9, V).astype(np.float32)
    det = rng.uniform(-1.0, 1.0, V).astype(np.float32)
    params = np.tile(np.array(DEFAULTS), (NB, 1))
    params[3], params[65] = ROOMS[0], ROOMS[3]
    enabled = np.zeros(NB, dtype=np.intc)
    enabled[[3, 65]] = 1
    mgain = rng.uniform(-2.0, 2.0, (NB, 2)).astype(np.float32)

    def make():
        p = S.Patch(sr, 64, 2)
        ids = S.build_p1(p, lfo_val=0.0)
        p.configure_voices(V)
        p.set_voice_field(ids["osc_a"], S.OSC_VAL, det)
        p.set_buses(NB, bus, vgain)
        p.set_bus_reverbs(params, enabled)
        return p

    p, q = make(), make()
    masters, fxs = [], []
    stats = np.zeros((2, 6))
    for k in range(2):
        if k == 1:
            p.set_master(mgain)  # (the first call runs with 1.0f everywhere)
        rp = p.render_buses(n, frames=True, mix=True, stats=True)
        rq = q.render_buses(n, frames=True, mix=True, stats=True)
        fx_p, fx_q = p.bus_reverb(rp[3]), q.bus_reverb(rq[3])
        assert "master=" not in q.info() and ("master=" in p.info()) == (k == 1)
        m, stats = p.master(fx_p, stats)
        for what, x, y in zip(("frames", "mix", "statistics", "bus mixes", "fx"), rp + (fx_p,), rq + (fx_q,)):
            np.testing.assert_array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8), err_msg=f"call {k}: {what} moved")
        ip, iq = p.info(), q.info()
        assert ip.split("kernel=")[-1] == iq.split("kernel=")[-1] and "kernel=" in ip
        assert " master=66[2 runs]" in ip and ip.replace(" master=66[2 runs]", "") == iq
        assert ip.index(" busfx=") < ip.index(" master=") < ip.index(" kernel=")
        masters.append(m)
        fxs.append(fx_p)
    want, got = all_fields(S, q), all_fields(S, p)
    assert len(want) >= 8 and got.keys() == want.keys()
    for key in want:
        np.testing.assert_array_equal(got[key].view(np.uint64), want[key].view(np.uint64), err_msg=f"module {key[0]} field {key[1]}")
    # the NumPy chain: the reverbs of buses 3 and 65 ticked in Python on the returned bus mixes, the tree over the fx rows
    bm = np.concatenate([fxs[0], fxs[1]], axis=2)
    assert_audible(bm, "the fx rows")
    ref = np.concatenate([R.master_tree(fxs[0]), R.master_tree(fxs[1], mgain)], axis=1)
    got = np.concatenate(masters, axis=1)
    assert_same_bits(got, ref, "the master of the fx rows")
    assert_audible(got, "end to end")
    assert_tree_matters(fxs[1], mgain, ref[:, n:], "end to end")
    assert_same_stats(stats, R.stats_sequential(ref), "the master's statistics over both calls")
    # ... and the fx rows themselves are the reverb's (tests/test_gpu_bus_reverb.py holds every other bus): bus 65, the last run's
    rq2 = make()
    bm2 = np.concatenate([rq2.render_buses(n)[3] for _ in range(2)], axis=2)
    assert_same_bits(bm[65], tick(new_reverb(sr, params[65]), bm2[65]), "bus 65 through its reverb")


# ---- 9: determinism -------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(S):
    rows, gain = R.case_inputs(4097, 70)
    outs = []
    for _ in range(2):
        p = host(S, 4097)
        p.set_master(gain)
        outs.append(p.master(rows, START))
    np.testing.assert_array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))
    assert_same_stats(outs[0][1], outs[1][1])
    assert_audible(outs[0][0], "determinism")
