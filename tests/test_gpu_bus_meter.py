"""The bus meters on the device (srack_buses_meter, csrc/busmeter.hip.h): a lane per (bus, channel) row, tiles of 64 rows x 64 samples
through LDS, the open window's record and the totals in registers.

Rows are seeded f32 values fed straight into srack_buses_meter.  The reference is tests/busmeter_ref.py — master_ref.stats_sequential's
literal loop per row and window, continued from the buffers —, which tests/test_bus_meter_host.py holds to the per-voice definitions and
whose case inputs it shows to tell orders of addition apart.  The criterion is BIT EQUALITY OF EVERY f64 WORD — derived, not measured:
the device adds the same f64 values in the same order through wave.hip.h's stats_add, an f64 add and an exact-product fma per sample.
No tolerance anywhere in this file.  Every comparison is of WHOLE buffers, guard words behind them included: whatever a call must
not touch — records outside its windows, channel-1 entries of one-channel rows — holds a sentinel that the reference leaves alone."""
import ctypes as C
import functools

import numpy as np
import pytest

import srack_pkg
from tests import busmeter_ref as R
from tests import busshaper_ref as RSH
from tests import busvca_ref as RA
from tests import busvcf_ref as RF
from tests import console_ref as CR
from tests import sends_ref as RS
from tests.test_gpu_bus_reverb import copy_of, new_reverb, tick

pytestmark = pytest.mark.gpu

SENTINEL = -7.25       # what an output word holds where a call must not write (an f32 value: a peak is read back as f32)
GUARD = 12345.0        # four f64 words behind each output buffer
NB, T, WINDOW = 130, 777, 100   # 260 rows: four full waves and one of four rows; twelve tiles and a tail of nine; boundaries in mid-tile
SEEDS = (7, 8, 9)


@pytest.fixture(scope="module")
def S():
    return srack_pkg.load()


def assert_same_words(got, ref, what=""):
    got, ref = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    ok = R.same_bits64(got, ref)
    if not ok.all():
        at = np.argwhere(~ok)
        first = tuple(at[0])
        raise AssertionError(f"{what}: {len(at)} of {ok.size} words differ, first at {first}: got {got[first]!r} "
                             f"({got.view(np.uint64)[first]:#018x}), reference {ref[first]!r} ({ref.view(np.uint64)[first]:#018x})")


def host(S, n_buses, channels=2, rate=48000):
    """a handle to hang the table on: an oscillator into every channel, one voice in bus 0 of n_buses (never rendered here)"""
    p = S.Patch(rate, 64, channels)
    osc, out = p.add_module(S.MOD_OSCILLATOR), p.add_module(S.MOD_OUTPUT)
    for c in range(channels):
        p.connect(osc, S.OSC_OUT_SINE, out, c)
    p.configure_voices(1)
    p.set_buses(n_buses)
    return p


@functools.lru_cache(maxsize=None)
def case(n_buses, rc, n, seed):
    rows = R.case_rows(n_buses, n, seed, rc)
    rows.setflags(write=False)
    return rows


def start(n_windows, n_buses, seed, how):
    """what the buffers hold before the first call -> (levels [n_windows][6][n_buses][2], totals [6][n_buses][2]).  "zeros"; "sentinel":
    SENTINEL everywhere (a continuation from it is as good as any); "carried": sums and counts of an earlier stretch, and peaks of 5.0
    on every third entity, which no sample of the cases reaches"""
    shape = (n_windows, R.STAT_COUNT, n_buses, 2)
    if how == "zeros":
        return np.zeros(shape), np.zeros(shape[1:])
    if how == "sentinel":
        return np.full(shape, SENTINEL), np.full(shape[1:], SENTINEL)
    assert how == "carried", how
    rng = np.random.default_rng(seed + 100)
    both = np.empty((n_windows + 1,) + shape[1:])
    both[:, R.STAT_SUM] = rng.uniform(-3, 3, both[:, 0].shape) * np.exp2(rng.integers(-20, 1, both[:, 0].shape))
    both[:, R.STAT_SUM_SQ] = rng.uniform(0, 9, both[:, 0].shape)
    both[:, R.STAT_PEAK_POS] = rng.uniform(0, 1, both[:, 0].shape).astype(np.float32)
    both[:, R.STAT_PEAK_NEG] = rng.uniform(0, 1, both[:, 0].shape).astype(np.float32)
    high = (np.arange(n_buses * 2) % 3 == 0).reshape(n_buses, 2)
    both[:, R.STAT_PEAK_POS][:, high] = 5.0
    both[:, R.STAT_PEAK_NEG][:, high] = 5.0
    both[:, R.STAT_NONFINITE] = rng.integers(0, 50, both[:, 0].shape)
    both[:, R.STAT_CLIPPED] = rng.integers(0, 50, both[:, 0].shape)
    return both[:-1].copy(), both[-1].copy()


class Device:
    """buffers of a staging scope (S.DeviceScope, which frees them), sent and fetched at once, guard words behind them"""

    def __init__(self, S, scope):
        self.lib, self.alloc = S.lib, scope.alloc

    def up(self, d, a, stream=None):
        a = np.ascontiguousarray(a)
        if a.nbytes:
            assert self.lib.srack_device_from_host(d, a.ctypes.data_as(C.c_void_p), a.nbytes, stream) == 0
            assert self.lib.srack_device_sync(stream) == 0   # (the host array may go away)

    def down(self, d, shape, dtype=np.float32, stream=None):
        a = np.empty(shape, dtype=dtype)
        if a.nbytes:
            assert self.lib.srack_device_to_host(a.ctypes.data_as(C.c_void_p), d, a.nbytes, stream) == 0
        assert self.lib.srack_device_sync(stream) == 0
        return a

    def guarded(self, a):
        """`a` (f64) on the device with four GUARD words behind it -> the address"""
        d = self.alloc(a.nbytes + 32)
        self.up(d, np.concatenate([np.ascontiguousarray(a, dtype=np.float64).ravel(), np.full(4, GUARD)]))
        return d

    def back(self, d, shape):
        """the buffer as it came back; the guard words must be what they were"""
        a = self.down(d, int(np.prod(shape)) + 4, np.float64)
        assert (a[-4:].view(np.uint64) == np.full(4, GUARD).view(np.uint64)).all(), "a word behind the buffer was written"
        return a[:-4].reshape(shape)


def run(S, p, rows, window=None, first=0, levels=None, totals=None, cuts=None, off=0):
    """srack_buses_meter on `rows` in calls of `cuts` samples (None: one call), each call's rows an allocation of its own, `off` floats
    into it.  levels / totals: what the buffers hold beforehand, None: that output is not taken.  -> (levels, totals) as they came
    back.  Asserts that the rows come back unchanged and that the guard words behind both buffers stand."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    nb, rc, n = x.shape
    with S.DeviceScope() as scope:
        dev = Device(S, scope)
        d_lv = None if levels is None else dev.guarded(levels)
        d_tt = None if totals is None else dev.guarded(totals)
        at = 0
        for m in (cuts or [n]):
            piece = np.ascontiguousarray(x[:, :, at:at + m])
            d = dev.alloc(piece.nbytes + 4 * off + 4)
            dev.up(d, np.concatenate([np.full(off, 99.0, dtype=np.float32), piece.ravel(), np.full(1, 99.0, dtype=np.float32)]))
            p.bus_meter_raw(first + at, m, d + 4 * off, rc, window or 0, d_lv, 0 if levels is None else levels.shape[0], d_tt, None)
            held = dev.down(d, off + piece.size + 1)
            assert (held[off:-1].view(np.uint32) == piece.ravel().view(np.uint32)).all() and (held[:off] == 99.0).all() and held[-1] == 99.0, "the rows were written"
            at += m
        assert at == n
        return (None if levels is None else dev.back(d_lv, levels.shape)), (None if totals is None else dev.back(d_tt, totals.shape))


def check(S, rows, window, first, how, n_extra=0, what="", cuts=None, off=0, outputs="both", seed=0):
    """one case against the reference, whole buffers; -> (got levels, got totals)"""
    nb, rc, n = rows.shape
    n_windows = R.n_windows_for(first, n, window) + n_extra
    lv0, tt0 = start(n_windows, nb, seed, how)
    if outputs == "totals":
        lv0 = None
    if outputs == "levels":
        tt0 = None
    want_lv, want_tt = R.bus_meter(rows, window if lv0 is not None else None, first, lv0, False if tt0 is None else tt0)
    got_lv, got_tt = run(S, host(S, nb), rows, window, first, lv0, tt0, cuts, off)
    if lv0 is not None:
        assert_same_words(got_lv, want_lv, what + ": levels")
    if tt0 is not None:
        assert_same_words(got_tt, want_tt, what + ": totals")
    return got_lv, got_tt


# ---- 1. the case behind the guards of tests/test_bus_meter_host.py --------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 37])
@pytest.mark.parametrize("window", [100, 64, 65, 1024], ids=["w100", "w64", "w65", "one window"])
def test_the_case(S, window, first):
    rows = case(NB, 2, T, SEEDS[0])
    lv, tt = check(S, rows, window, first, "zeros", what=f"window {window}, first {first}")
    assert lv.shape[0] == (1 if window == 1024 else -(-(first + T) // window))
    assert np.count_nonzero(lv[:, R.STAT_CLIPPED]) > lv[:, 0].size // 2 and (tt[R.STAT_CLIPPED] > 0).all()


@pytest.mark.parametrize("seed", SEEDS[1:])
def test_the_case_other_seeds(S, seed):
    check(S, case(NB, 2, T, seed), WINDOW, 0, "zeros", what=f"seed {seed}")


# ---- 2. wave and channel shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [1, 2, 3])
@pytest.mark.parametrize("n_buses", [1, 32, 33, 64, 65])
def test_bus_counts_and_row_channels(S, n_buses, rc):
    """one row channel: every channel-1 entry keeps its sentinel (the whole-buffer comparison holds it, and it is asked again here);
    three: the third channel is all NaN and never read"""
    rows = case(n_buses, rc, 200, 21 + rc).copy()
    if rc == 3:
        rows[:, 2] = np.nan
    lv, tt = check(S, rows, 64, 37, "sentinel", n_extra=1, what=f"{n_buses} buses, {rc} row channels")
    if rc == 1:
        assert (lv[:, :, :, 1] == SENTINEL).all() and (tt[:, :, 1] == SENTINEL).all()
    assert (lv[-1] == SENTINEL).all()   # the record behind the call's last window
    assert (tt[R.STAT_NONFINITE, :, :min(rc, 2)] == SENTINEL).all()   # nothing non-finite was seen


# ---- 3. the outputs, and buffers that start non-zero -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", ["levels", "totals", "both"])
def test_outputs_and_continuation(S, outputs):
    rows = case(NB, 2, T, SEEDS[0])
    lv, tt = check(S, rows, WINDOW, 37, "carried", what=outputs, outputs=outputs, seed=3)
    high = (np.arange(NB * 2) % 3 == 0).reshape(NB, 2)   # a peak does not move down
    if lv is not None:
        assert (lv[:, R.STAT_PEAK_POS][:, high] == 5.0).all() and (lv[:, R.STAT_PEAK_NEG][:, high] == 5.0).all()
    if tt is not None:
        assert (tt[R.STAT_PEAK_POS][high] == 5.0).all() and (tt[R.STAT_PEAK_NEG][high] == 5.0).all()
    assert (lv is None) == (outputs == "totals") and (tt is None) == (outputs == "levels")


# ---- 4. rows that start 1, 2 and 3 floats into their allocation ------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [1, 2, 3])
def test_rows_need_four_byte_alignment_only(S, off):
    check(S, case(NB, 2, T, SEEDS[0]), WINDOW, 0, "zeros", what=f"{off} floats in", off=off)


# ---- 5. the cut into calls does not show -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 37])
def test_cut_into_calls(S, first):
    cuts = [1, 63, 64, 65, 300, T - 493]
    rows = case(NB, 2, T, SEEDS[0])
    lv, tt = check(S, rows, WINDOW, first, "zeros", what=f"cuts {cuts}, first {first}", cuts=cuts)
    one_lv, one_tt = run(S, host(S, NB), rows, WINDOW, first, np.zeros_like(lv), np.zeros_like(tt))
    assert_same_words(lv, one_lv, "cut against one call: levels")
    assert_same_words(tt, one_tt, "cut against one call: totals")


# ---- 6. special values -------------------------------------------------------------------------------------------------------------------------
def test_special_values_stay_in_their_rows(S):
    one_up = np.nextafter(np.float32(1), np.float32(2))
    specials = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, -1.0, one_up, -one_up, 1e-45, -1e-45, 1.1754942e-38, -5e-40], dtype=np.float32)
    rows = case(70, 2, 300, 31).copy()
    rng = np.random.default_rng(31)
    for b in (0, 5, 30, 31, 36, 63, 64, 69):   # scattered over the waves' ends and middles (rows 64 .. 127 are buses 32 .. 63)
        at = rng.random((2, 300)) < 0.3
        rows[b][at] = rng.choice(specials, int(at.sum()))
    rows[33] = np.nan                       # a bus that is all NaN, between two ordinary ones
    rows[6, 1] = np.inf
    lv, tt = check(S, rows, 64, 0, "zeros", what="special values")
    assert (tt[R.STAT_NONFINITE, 33] == 300).all() and (tt[:4, 33] == 0).all() and not np.signbit(tt[:4, 33]).any() and (tt[R.STAT_CLIPPED, 33] == 0).all()
    assert (lv[:, R.STAT_NONFINITE, 33].sum(axis=0) == 300).all() and tt[R.STAT_NONFINITE, 6].tolist() == [0.0, 300.0]
    clean = case(70, 2, 300, 31)
    _, clean_tt = R.bus_meter(clean)
    for b in (32, 34):                      # its neighbours are what they are without it
        assert_same_words(tt[:, b], clean_tt[:, b], f"bus {b}")


# ---- 7. what a call leaves alone ---------------------------------------------------------------------------------------------------------------
def test_records_outside_the_call_keep_their_sentinel(S):
    rows = case(NB, 2, 130, 41)
    first, n_windows = 250, 8           # windows 2 and 3 of eight
    lv0, tt0 = start(n_windows, NB, 0, "sentinel")
    want_lv, want_tt = R.bus_meter(rows, WINDOW, first, lv0, tt0)
    lv, tt = run(S, host(S, NB), rows, WINDOW, first, lv0, tt0)
    assert_same_words(lv, want_lv, "levels")
    assert_same_words(tt, want_tt, "totals")
    assert (lv[[0, 1, 4, 5, 6, 7]] == SENTINEL).all() and (lv[2:4, R.STAT_SUM_SQ] != SENTINEL).all()
    # a call that ends exactly on a boundary does not open the next record
    lv, _ = run(S, host(S, NB), rows[:, :, :50], WINDOW, first, lv0, None)
    assert (lv[[0, 1, 3, 4, 5, 6, 7]] == SENTINEL).all() and (lv[2, R.STAT_SUM_SQ] != SENTINEL).all()


# ---- 8. a tap: before and behind an in-place shaper on one stream ---------------------------------------------------------------------------------
def _stream():
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    st = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(st), 1) == 0   # hipStreamNonBlocking
    return hip, st


def test_taps_around_a_shaper_on_one_stream(S):
    n_buses, n = 70, 300
    rows = case(n_buses, 2, n, 51)
    rng = np.random.default_rng(51)
    params = np.stack([rng.uniform(0.25, 4.0, n_buses), rng.uniform(0.5, 2.0, n_buses), rng.uniform(0.25, 2.0, n_buses)], axis=1).astype(np.float32)
    mode = np.full(n_buses, RSH.CONST, dtype=np.intc)
    shaped = RSH.bus_shaper(rows, None, params, mode)
    assert np.count_nonzero(~RSH.same_bits(shaped, rows)) > rows.size // 2
    n_windows = R.n_windows_for(0, n, WINDOW)
    zl, zt = start(n_windows, n_buses, 0, "zeros")
    want = [R.bus_meter(rows, WINDOW, 0, zl, zt), R.bus_meter(shaped, WINDOW, 0, zl, zt)]
    assert np.count_nonzero(~R.same_bits64(want[0][0], want[1][0])) > zl.size // 2
    p = host(S, n_buses)
    p.set_bus_shaper(params, mode)
    hip, st = _stream()
    try:
        with S.DeviceScope() as scope:
            dev = Device(S, scope)
            d_rows = dev.alloc(rows.nbytes)
            dev.up(d_rows, rows, st)
            d = [(dev.guarded(zl), dev.guarded(zt)) for _ in range(2)]
            p.bus_meter_raw(0, n, d_rows, 2, WINDOW, d[0][0], n_windows, d[0][1], st)
            p.bus_shaper_raw(n, d_rows, 2, None, d_rows, st)
            p.bus_meter_raw(0, n, d_rows, 2, WINDOW, d[1][0], n_windows, d[1][1], st)
            assert S.lib.srack_device_sync(st) == 0
            for k, name in enumerate(("before the shaper", "behind the shaper")):
                assert_same_words(dev.back(d[k][0], zl.shape), want[k][0], name + ": levels")
                assert_same_words(dev.back(d[k][1], zt.shape), want[k][1], name + ": totals")
            assert RSH.same_bits(dev.down(d_rows, rows.shape), shaped).all()   # the shaper's bits are what they are without the taps
    finally:
        assert hip.hipStreamDestroy(st) == 0


# ---- 9. the chain of tests/console_ref.py's case, a tap behind every stage ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_reference(n_buses=20, T=260):
    """sends -> filter -> VCA -> shaper -> reverb on console_ref's case, each stage by the reference console_ref composes (the shaper by
    tests/busshaper_ref.py) -> (rows, ctl, settings, shaper params, [the five stage outputs])"""
    rows, ctl, s = CR.case(n_buses, 2, T, CR.SEED, 4)
    rng = np.random.default_rng(CR.SEED + 9)
    spar = np.stack([rng.uniform(0.5, 3.0, n_buses), rng.uniform(0.5, 2.0, n_buses), rng.uniform(0.5, 1.5, n_buses)], axis=1).astype(np.float32)
    sent = RS.send_tree(rows, s.send_src, s.send_dst, s.send_gain, s.through)
    vcf, _ = RF.bus_filter(sent, ctl, s.vcf_params, s.vcf_port, s.vcf_enabled)
    vca = RA.bus_vca(vcf, ctl, s.vca_params, s.vca_mode, s.vca_negative, s.rate)[0]
    shp = RSH.bus_shaper(vca, None, spar, np.full(n_buses, RSH.CONST, dtype=np.intc))
    fx = np.stack([tick(new_reverb(s.rate, tuple(float(v) for v in s.rv_params[b])), shp[b]) if s.rv_enabled[b] else copy_of(shp[b]) for b in range(n_buses)])
    return rows, ctl, s, spar, [np.ascontiguousarray(a, dtype=np.float32) for a in (sent, vcf, vca, shp, fx)]


def test_a_tap_behind_every_stage_of_the_chain(S):
    rows, ctl, s, spar, stages = chain_reference()
    nb, _, n = rows.shape
    names = ("sends", "filter", "VCA", "shaper", "reverb")
    for a, b, name in zip([rows] + stages[:-1], stages, names):   # every stage shows: the taps are not five views of one buffer
        assert np.count_nonzero(~CR.same_bits(a, b)) > 0, name
    window, first = 64, 37
    n_windows = R.n_windows_for(first, n, window)
    zl, zt = start(n_windows, nb, 0, "zeros")
    want = [R.bus_meter(x, window, first, zl, zt) for x in stages]
    p = CR.host(S, s)
    p.set_bus_shaper(spar, np.full(nb, RSH.CONST, dtype=np.intc))
    hip, st = _stream()
    try:
        with S.DeviceScope() as scope:
            dev = Device(S, scope)
            d_rows, d_buf, d_fx, d_ctl = dev.alloc(rows.nbytes), dev.alloc(rows.nbytes), dev.alloc(rows.nbytes), dev.alloc(ctl.nbytes)
            dev.up(d_rows, rows, st)
            dev.up(d_ctl, ctl, st)
            taps = [(dev.guarded(zl), dev.guarded(zt)) for _ in stages]
            tap = lambda k, d: p.bus_meter_raw(first, n, d, 2, window, taps[k][0], n_windows, taps[k][1], st)
            p.send_raw(n, d_rows, 2, d_buf, st)
            tap(0, d_buf)
            p.bus_filter_raw(n, d_buf, 2, d_ctl, d_buf, st)
            tap(1, d_buf)
            p.bus_vca_raw(n, d_buf, 2, d_ctl, d_buf, None, st)
            tap(2, d_buf)
            p.bus_shaper_raw(n, d_buf, 2, None, d_buf, st)
            tap(3, d_buf)
            p.bus_reverb_raw(n, d_buf, d_fx, st)
            tap(4, d_fx)
            assert S.lib.srack_device_sync(st) == 0
            assert CR.same_bits(dev.down(d_fx, rows.shape), stages[-1]).all(), "the chain itself"
            for k, name in enumerate(names):
                assert_same_words(dev.back(taps[k][0], zl.shape), want[k][0], f"behind the {name}: levels")
                assert_same_words(dev.back(taps[k][1], zt.shape), want[k][1], f"behind the {name}: totals")
    finally:
        assert hip.hipStreamDestroy(st) == 0


# ---- 10. the note, the convenience call, the lifecycle -----------------------------------------------------------------------------------------------
def test_the_note_and_the_convenience_call(S):
    n_buses, n = 5, 150
    rows = case(n_buses, 2, n, 61)
    p = host(S, n_buses)
    before = p.info()
    assert "meter" not in before
    lv, tt = p.bus_meter(rows, window=64, first_sample=10)
    want_lv, want_tt = R.bus_meter(rows, 64, 10)
    assert_same_words(lv, want_lv, "bus_meter: levels")
    assert_same_words(tt, want_tt, "bus_meter: totals")
    assert p.info().replace(" meter=5[w64]", "", 1) == before and " meter=5[w64]" in p.info()
    p.master(rows)
    info = p.info()
    assert info.count(" meter=5[w64]") == 1 and info.index(" master=") < info.index(" meter=")
    lv2, tt2 = p.bus_meter(rows, totals=tt)   # totals only, continued
    assert lv2 is None
    assert_same_words(tt2, R.bus_meter(rows, totals=want_tt)[1], "bus_meter: totals continued")
    assert " meter=5[w-]" in p.info()
    lv3, none = p.bus_meter(rows[:, :, 100:], window=64, first_sample=110, levels=p.bus_meter(rows[:, :, :100], window=64, first_sample=10, levels=np.zeros_like(lv), totals=False)[0], totals=False)
    assert none is None
    assert_same_words(lv3, want_lv, "bus_meter: levels in two calls")
    # the stage goes with the table, like every console stage
    p.set_buses(n_buses + 1, np.zeros(1, dtype=np.intc))
    assert "meter" not in p.info()
