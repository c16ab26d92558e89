"""The bus shapers on the device (srack_buses_shaper, csrc/busshape.hip.h): a wave per stretch of 1024 samples of one bus, both channels,
steps of 4 x 64 samples, the libm's tables in LDS.

Rows are seeded f32 values fed straight into srack_buses_shaper.  The reference is tests/busshaper_ref.py — two NumPy f32 products
around the host libm's powf —, which tests/test_bus_shaper_host.py holds to the oracle's modules bit for bit.  The criterion is BIT
EQUALITY (NaN matching NaN) — derived, not measured: the products are the same single-rounded f32 operations (the library is built with
-ffp-contract=off), and the device's power is the libm's algorithm operation for operation (modules.hip.h, powf_libm_plain; its cold
path answers the arguments C99 Annex F fixes).  No tolerance anywhere in this file.  The big case stands behind guards that the
reference is worth comparing with — among them that it is NOT the correctly rounded power."""
import ctypes as C
import functools

import numpy as np
import pytest

import srack_pkg
from tests import busshaper_ref as R
from tests import busvca_ref as RA
from tests import busvcf_ref as RF
from tests import master_ref as RM

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-54321.5)  # what d_out holds before a call, wherever the call must not write
GUARD = np.float32(12345.0)      # one float behind d_out
SEED = 7
NB, T = 130, 777


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
        raise AssertionError(f"{what}: {len(at)} of {ok.size} values differ, first at {first}: got {got[first]!r} "
                             f"({got.view(np.uint32)[first]:#010x}), reference {ref[first]!r} ({ref.view(np.uint32)[first]:#010x})")


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
def _case(n_buses, rc, n, seed):
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-2.0, 2.0, (n_buses, rc, n)).astype(np.float32)
    low = rng.random(n_buses) < 0.5
    expo = np.where(low, rng.uniform(0.5, 0.9, n_buses), rng.uniform(1.1, 2.0, n_buses))
    params = np.stack([rng.uniform(0.25, 4.0, n_buses), expo, rng.uniform(0.25, 2.0, n_buses)], axis=1).astype(np.float32)
    mode = rng.integers(0, 3, n_buses).astype(np.intc)
    mode[0] = R.CONST
    if n_buses > 2:
        mode[1], mode[2] = R.CV, R.OFF
    cv = rng.uniform(0.5, 2.0, (n_buses, n)).astype(np.float32)
    for a in (rows, cv, params, mode):
        a.setflags(write=False)
    return rows, cv, params, mode


def case(n_buses, rc, n, seed):
    """-> (rows [n_buses][rc][n] in (-2, 2), cv [n_buses][n] in [0.5, 2], params [n_buses][3], mode [n_buses]): read-only, shared"""
    return _case(n_buses, rc, n, seed)


@functools.lru_cache(maxsize=None)
def reference(n_buses, rc, n, seed, with_cv=True):
    rows, cv, params, mode = case(n_buses, rc, n, seed)
    out = R.bus_shaper(rows, cv if with_cv else None, params, mode)
    out.setflags(write=False)
    return out


def run_raw(S, p, rows, cv=None, in_place=False, off_rows=0, off_cv=0, off_out=0, stream=None):
    """srack_buses_shaper with its three pointers `off_*` floats into their allocations.  Out of place d_out holds SENTINEL beforehand;
    one GUARD float lies behind it.  -> (out of rows' shape, the guard as it came back)"""
    lib = S.lib
    x = np.ascontiguousarray(rows, dtype=np.float32)
    buf = np.full(x.size + 1, SENTINEL, dtype=np.float32)
    if in_place:
        buf[:-1] = x.ravel()
    buf[-1] = GUARD
    c = None
    if cv is not None:
        c = np.ascontiguousarray(cv, dtype=np.float32)
        assert c.shape == (x.shape[0], x.shape[2])
    with S.DeviceScope(stream) as dev:
        a_out = dev.upload(buf, off_out)
        a_in = a_out if in_place else dev.upload(x, off_rows)
        a_cv = None if c is None else dev.upload(c, off_cv)
        assert lib.srack_device_sync(None) == 0
        p.bus_shaper_raw(x.shape[2], a_in, x.shape[1], a_cv, a_out, stream)
        dev.download(buf, a_out)
    return buf[:-1].reshape(x.shape), buf[-1]


def check_both_ways(S, rows, cv, params, mode, ref, what, off=0):
    """out of place into SENTINEL and in place: the used channels against `ref`, everything else untouched"""
    n_buses, rc, _ = rows.shape
    used = min(rc, 2)
    off_buses = np.flatnonzero(np.asarray(mode) == R.OFF)
    p = host(S, n_buses)
    p.set_bus_shaper(params, mode)
    got, guard = run_raw(S, p, rows, cv, off_rows=off, off_cv=off, off_out=off)
    assert_same_bits(got[:, :used], ref[:, :used], f"{what}, out of place")
    assert (got[:, used:] == SENTINEL).all() and guard == GUARD, f"{what}: a channel beyond the second, or the float behind d_out, was written"
    assert (got[off_buses, :used].view(np.uint32) == rows[off_buses, :used].view(np.uint32)).all(), f"{what}: an OFF bus is a word copy"
    q = host(S, n_buses)
    q.set_bus_shaper(params, mode)
    inp, guard = run_raw(S, q, rows, cv, in_place=True, off_cv=off, off_out=off)
    assert_same_bits(inp[:, :used], ref[:, :used], f"{what}, in place")
    assert (inp[:, used:].view(np.uint32) == rows[:, used:].view(np.uint32)).all() and guard == GUARD, f"{what}: channels beyond the second, in place"
    assert (inp[off_buses].view(np.uint32) == rows[off_buses].view(np.uint32)).all(), f"{what}: an OFF bus is left alone in place"
    return p


# ---- 1. the big case, behind the guards on its reference ---------------------------------------------------------------------------------
def test_the_big_case(S):
    rows, cv, params, mode = case(NB, 2, T, SEED)
    ref, ref_const = reference(NB, 2, T, SEED), reference(NB, 2, T, SEED, with_cv=False)
    assert mode[:3].tolist() == [R.CONST, R.CV, R.OFF] and all(np.count_nonzero(mode == m) >= 20 for m in (R.OFF, R.CONST, R.CV))
    assert 0.25 <= params[:, 0].min() and params[:, 0].max() <= 4 and 0.25 <= params[:, 2].min() and params[:, 2].max() <= 2
    e = params[:, 1]
    assert ((e >= 0.5) & (e <= 0.9) | (e >= 1.1) & (e <= 2.0)).all() and (e <= 0.9).sum() >= 20 and (e >= 1.1).sum() >= 20
    on, by_cv = np.flatnonzero(mode != R.OFF), np.flatnonzero(mode == R.CV)
    y, x = ref[on], rows[on]
    # the guards, each before any comparison
    assert np.isfinite(y).all(), "the reference is not finite"
    nonzero, moved, cv_shows = np.count_nonzero(y), np.count_nonzero(y != x), np.count_nonzero(ref[by_cv] != ref_const[by_cv])
    driven = (x * params[on, 0][:, None, None]).astype(np.float32)
    expo = np.repeat(params[on, 1][:, None], T, axis=1)
    expo[mode[on] == R.CV] = cv[by_cv]
    power = R.nonlinear(driven, expo[:, None, :])
    once = (np.sign(driven.astype(np.float64)) * np.abs(driven.astype(np.float64)) ** expo[:, None, :].astype(np.float64)).astype(np.float32)
    misrounded = ~R.same_bits(power, once)
    print(f"big case: {y.size} processed samples, {nonzero} non-zero, {moved} differ from their input, CV differs from CONST on {cv_shows} of "
          f"{ref[by_cv].size}, the libm differs from the double-precision power rounded once on {np.count_nonzero(misrounded)} "
          f"over {np.count_nonzero(misrounded.any(axis=(1, 2)))} buses")
    assert nonzero >= y.size * 7 // 8, "the reference is (nearly) silent"
    assert moved >= y.size * 3 // 4, "the reference is its input"
    assert cv_shows >= ref[by_cv].size * 3 // 4, "the CV is meant to show"
    assert np.count_nonzero(misrounded) >= 32, "the reference is meant to be the libm's power, not the correctly rounded one"
    p = check_both_ways(S, rows, cv, params, mode, ref, "the big case")
    assert f" busshp={len(on)}[{len(by_cv)} cv]" in p.info()


# ---- 2. shapes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("n_buses", [1, 3, 65])
def test_shapes(S, n_buses, n):
    """1 / 3 / 65 buses, 1 / 63 / 64 / 65 / 257 samples — a partial load, a full one, a load with a tail, a step (256) with a tail —,
    row_channels going round 1, 2, 3 over the grid, every pointer one float into its allocation, out of place and in place"""
    rc = 1 + (n_buses + n) % 3
    rows, cv, params, mode = case(n_buses, rc, n, SEED)
    ref = reference(n_buses, rc, n, SEED)
    assert np.isfinite(ref).all()
    check_both_ways(S, rows, cv, params, mode, ref, f"{n_buses} x {rc} x {n}", off=1)


@pytest.mark.parametrize("rc,n", [(2, 1024), (1, 1025), (3, 2100)])
def test_more_than_one_stretch(S, rc, n):
    """a wave takes 1024 samples of a bus: exactly one stretch, one and a sample, two and a tail"""
    rows, cv, params, mode = case(3, rc, n, SEED + 1)
    ref = reference(3, rc, n, SEED + 1)
    assert np.isfinite(ref).all()
    check_both_ways(S, rows, cv, params, mode, ref, f"3 x {rc} x {n}", off=1)


def test_cv_buses_without_a_cv_row(S):
    """d_cv == NULL: In2 is unconnected, a CV bus's exponent is its EXPONENT"""
    rows, cv, params, mode = case(65, 2, 257, SEED)
    ref = reference(65, 2, 257, SEED, with_cv=False)
    with_cv = reference(65, 2, 257, SEED)
    by_cv = mode == R.CV
    assert by_cv.sum() >= 10 and np.count_nonzero(ref[by_cv] != with_cv[by_cv]) > ref[by_cv].size * 3 // 4
    as_const = R.bus_shaper(rows, None, params, np.where(by_cv, R.CONST, mode))
    assert_same_bits(ref, as_const, "the reference: a CV bus without a row is a CONST bus")
    check_both_ways(S, rows, None, params, mode, ref, "no CV row")


def test_all_buses_off(S):
    rows, cv, params, _ = case(65, 3, 257, SEED)
    rows = rows.copy()
    rows.view(np.uint32)[5, 0, :4] = (0x80000000, 0x7FC12345, 0xFFC00001, 0x00000001)   # -0.0, NaNs with payloads, a denormal
    mode = np.zeros(65, dtype=np.intc)
    ref = R.bus_shaper(rows, cv, params, mode)
    p = check_both_ways(S, rows, cv, params, mode, ref, "all OFF")
    assert " busshp=0[0 cv]" in p.info()


def test_cuts_give_the_same_bits(S):
    rows, cv, params, mode = case(NB, 2, T, SEED)
    ref = reference(NB, 2, T, SEED)
    p = host(S, NB)
    p.set_bus_shaper(params, mode)
    whole = p.bus_shaper(rows, cv)
    assert_same_bits(whole, ref, "one call")
    parts, at = [], 0
    for k in (1, 64, T - 65):
        parts.append(p.bus_shaper(rows[:, :, at:at + k], cv[:, at:at + k]))
        at += k
    assert at == T and (np.concatenate(parts, axis=2).view(np.uint32) == whole.view(np.uint32)).all(), "calls of 1, 64 and the rest"


# ---- 3. special values -------------------------------------------------------------------------------------------------------------------------
EXPONENTS = [2.0, 0.5, 0.0, -0.0, -1.0, 3.0, np.nan, np.inf, -np.inf]
SAMPLES = [0.0, -0.0, np.nan, np.inf, -np.inf, 1e-40, -1e-40, 1e-20, 1e30, -1e30, 1.0, -1.0, 1e-30]


@pytest.mark.parametrize("how", ["const", "cv"])
def test_special_values(S, how):
    """one bus per exponent, as its constant or as a CV row, its rows cycling through the samples: the cold path (zero, infinite and NaN
    arguments; exponents 0, -0, NaN, +-inf: a wholly cold bus next to ordinary ones), a subnormal argument (1e-40), a subnormal result
    (1e-20 squared), overflow (1e30 cubed) and underflow (1e-30 cubed)"""
    n_buses, n = len(EXPONENTS), 150
    rows = np.empty((n_buses, 2, n), dtype=np.float32)
    rows[:, 0] = np.resize(np.array(SAMPLES, dtype=np.float32), n)
    rows[:, 1] = np.roll(rows[:, 0], 5, axis=1)
    params = np.ones((n_buses, 3), dtype=np.float32)
    cv = None
    if how == "const":
        params[:, 1] = EXPONENTS
        mode = np.full(n_buses, R.CONST, dtype=np.intc)
    else:
        params[:, 1] = 1.5
        cv = np.repeat(np.array(EXPONENTS, dtype=np.float32)[:, None], n, axis=1)
        cv[0, ::2], cv[1, 1::3] = np.nan, 0.0   # ... and a row that is cold on some lanes only
        mode = np.full(n_buses, R.CV, dtype=np.intc)
    with np.errstate(all="ignore"):
        ref = R.bus_shaper(rows, cv, params, mode)
    sq, cube = ref[0, 0], ref[5, 0]
    k = {v: i for i, v in enumerate(SAMPLES) if v == v}
    if how == "const":
        assert 0 < sq[k[1e-20]] < 1.1754944e-38 and cube[k[1e30]] == np.inf and cube[k[-1e30]] == -np.inf and cube[k[1e-30]] == 0
        assert ref[4, 0, 0] == np.inf and ref[4, 0, 1] == -np.inf, "a zero to the power -1: -(-0.0).powf(-1) is +inf, -(0.0).powf(-1) is -inf"
        assert ref[2, 0, :13].tolist() == [-1.0, -1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 1.0], "powf(x, 0) is 1, NaN included"
    assert np.isnan(ref).any() and np.isinf(ref).any() and np.isfinite(ref).any()
    check_both_ways(S, rows, cv, params, mode, ref, f"special values, {how}")


# ---- 4. isolation ----------------------------------------------------------------------------------------------------------------------------------
def test_special_values_stay_in_their_bus(S):
    rows, cv, params, mode = case(NB, 2, T, SEED)
    base_ref = reference(NB, 2, T, SEED)
    p = host(S, NB)
    p.set_bus_shaper(params, mode)
    base = p.bus_shaper(rows, cv)
    assert_same_bits(base, base_ref, "without the specials")
    const, by_cv = np.flatnonzero(mode == R.CONST), np.flatnonzero(mode == R.CV)
    a, b, c, d = const[3], const[7], by_cv[2], by_cv[5]
    rows2, cv2, params2 = rows.copy(), cv.copy(), params.copy()
    params2[a, 1] = np.nan       # a NaN exponent: a wholly cold bus
    params2[b, 0] = np.inf       # an infinite drive
    rows2[c, 1, 70:300] = np.nan  # NaN samples on a CV bus
    cv2[d, 200] = np.inf         # an infinite CV value
    with np.errstate(all="ignore"):
        ref = R.bus_shaper(rows2, cv2, params2, mode)
    q = host(S, NB)
    q.set_bus_shaper(params2, mode)
    got = q.bus_shaper(rows2, cv2)
    assert_same_bits(got, ref, "with the specials")
    rest = np.setdiff1d(np.arange(NB), [a, b, c, d])
    assert (got[rest].view(np.uint32) == base[rest].view(np.uint32)).all(), "the buses the specials did not touch"
    assert np.isfinite(ref[rest]).all() and all(not np.isfinite(ref[x]).all() for x in (a, b, c, d))


# ---- 5. a caller's stream, settings replaced between calls in flight ---------------------------------------------------------------------------
def test_set_shaper_between_calls_on_a_stream(S):
    """eight calls on one non-blocking stream, nothing synchronised in between, set_shaper in front of every call: every call gives the
    reference for the settings it was issued under (the table is rewritten behind a wait for the call that reads it)"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    rows, cv, params, mode = case(NB, 2, T, SEED)
    rng = np.random.default_rng(SEED + 5)
    settings = []
    for k in range(8):
        par = params.copy()
        par[:, 1] = rng.permutation(params[:, 1])
        par[:, 0] = rng.uniform(0.25, 4.0, NB)
        settings.append((par, rng.permutation(mode).astype(np.intc)))
    refs = [R.bus_shaper(rows, cv, par, mo) for par, mo in settings]
    assert all(np.isfinite(r).all() for r in refs) and all(np.count_nonzero(refs[k] != refs[k + 1]) > refs[k].size // 2 for k in range(7))
    lib, st = S.lib, C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(st), 1) == 0   # hipStreamNonBlocking
    got = np.empty((8,) + rows.shape, dtype=np.float32)
    try:
        with S.DeviceScope(st) as dev:
            d_in, d_cv, d_out = dev.upload(rows), dev.upload(cv), dev.alloc(got.nbytes)
            assert lib.srack_device_sync(None) == 0
            p = host(S, NB)
            for k, (par, mo) in enumerate(settings):
                p.set_bus_shaper(par, mo)
                p.bus_shaper_raw(T, d_in, 2, d_cv, d_out + k * rows.nbytes, st)
            dev.download(got, d_out)
    finally:
        assert hip.hipStreamDestroy(st) == 0
    for k in range(8):
        assert_same_bits(got[k], refs[k], f"call {k}")


# ---- 6. the note, the lifecycle ------------------------------------------------------------------------------------------------------------------
def test_the_note_and_the_lifecycle(S):
    n_buses, n = 5, 100
    rows, cv, params, _ = case(n_buses, 2, n, SEED + 2)
    mode = np.array([R.CONST, R.CV, R.OFF, R.CV, R.CONST], dtype=np.intc)
    p = host(S, n_buses)
    p.set_bus_vca(mode=np.full(n_buses, RA.CV, dtype=np.intc))
    p.set_bus_reverbs()
    p.set_bus_shaper(params, mode)
    assert "busshp" not in p.info()   # no call has run
    assert_same_bits(p.bus_shaper(rows, cv), R.bus_shaper(rows, cv, params, mode), "first call")
    p.bus_vca(rows, cv)
    p.bus_reverb(rows)
    info = p.info()
    assert info.count(" busshp=4[2 cv]") == 1 and info.index(" busvca=") < info.index(" busshp=") < info.index(" busfx=")
    # set_shaper again is the slider; the same n_buses keeps the shapers, a field edit (a re-flatten) keeps them
    params2 = params[::-1].copy()
    p.set_bus_shaper(params2, mode[::-1].copy())
    p.set_buses(n_buses, np.zeros(1, dtype=np.intc))
    assert_same_bits(p.bus_shaper(rows, cv), R.bus_shaper(rows, cv, params2, mode[::-1]), "other settings")
    assert " busshp=4[2 cv]" in p.info()
    # another n_buses drops the stage and its note
    p.set_buses(n_buses + 2, np.zeros(1, dtype=np.intc))
    assert p.get_bus_shaper() == (0, None, None) and "busshp" not in p.info()
    assert S.lib.srack_buses_shaper(p.h, 16, 4096, 2, None, 1 << 20, None) == S.ERR_STATE
    rows7, cv7, params7, mode7 = case(n_buses + 2, 2, n, SEED + 3)
    p.set_bus_shaper(params7, mode7)
    assert_same_bits(p.bus_shaper(rows7, cv7), R.bus_shaper(rows7, cv7, params7, mode7), "seven buses")


# ---- 7. the chain: filter -> shaper -> VCA -> master on one stream ----------------------------------------------------------------------------------
def test_the_chain_on_one_stream(S):
    n_buses, n = 3, 130
    rows, cv, params, _ = case(n_buses, 2, n, SEED + 4)
    mode = np.array([R.CV, R.CONST, R.CV], dtype=np.intc)
    rng = np.random.default_rng(SEED + 4)
    fpar = np.stack([rng.uniform(0.05, 0.5, n_buses), rng.uniform(0.0, 0.9, n_buses), rng.uniform(-1.0, 1.0, n_buses)], axis=1).astype(np.float32)
    port, enabled = np.array([0, 1, 2], dtype=np.intc), np.array([1, 1, 0], dtype=np.intc)
    vmode, negative = np.array([RA.CV, RA.CV, RA.OFF], dtype=np.intc), np.array([0, 1, 0], dtype=np.intc)
    ctl = rng.uniform(-0.2, 1.0, (n_buses, n)).astype(np.float32)
    gain = rng.uniform(-1.0, 1.0, (n_buses, 2)).astype(np.float32)
    filtered, _ = RF.bus_filter(rows, ctl, fpar, port, enabled)
    shaped = R.bus_shaper(filtered, cv, params, mode)
    amped = RA.bus_vca(shaped, ctl, np.tile(np.array(RA.DEFAULTS, dtype=np.float32), (n_buses, 1)), vmode, negative, 48000)[0]
    want = RM.master_tree(amped, gain)
    assert np.isfinite(want).all() and np.count_nonzero(want) > want.size // 2
    assert np.count_nonzero(shaped != filtered) > shaped.size * 3 // 4 and np.count_nonzero(amped != shaped) > shaped.size // 4
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    st = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(st), 1) == 0
    p = host(S, n_buses)
    p.set_bus_filter(fpar, port, enabled)
    p.set_bus_shaper(params, mode)
    p.set_bus_vca(None, vmode, negative)
    p.set_master(gain)
    got, mid = np.empty_like(want), np.empty_like(rows)
    try:
        with S.DeviceScope(st) as dev:
            d = [dev.upload(a, stream=st) for a in (rows, ctl, cv)] + [dev.alloc(want.nbytes)]   # rows (processed in place), ctl, cv, master
            p.bus_filter_raw(n, d[0], 2, d[1], d[0], st)
            p.bus_shaper_raw(n, d[0], 2, d[2], d[0], st)
            p.bus_vca_raw(n, d[0], 2, d[1], d[0], None, st)
            p.master_raw(n, d[0], 2, d[3], None, st)
            dev.download(got, d[3])
            dev.download(mid, d[0])
    finally:
        assert hip.hipStreamDestroy(st) == 0
    assert_same_bits(mid, amped, "filter, shaper, VCA")
    assert_same_bits(got, want, "filter, shaper, VCA, master")
