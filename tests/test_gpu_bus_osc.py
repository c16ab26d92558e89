"""Bus oscillators on the device (srack_buses_osc, csrc/busosc.hip.h): a lane per enabled bus, tiles of 64 buses x 64 samples of the CV
and sync rows turned through LDS, osc_step with OSC_EXACT and two f32 Math operations per sample.

Everything is compared bit for bit with tests/busosc_ref.py — the oracle's own OscillatorModule and MathModules (tests/test_bus_osc_host.py
holds that file to the reference).  The guards — wraps, PolyBLEP windows, sync resets, held and moving CV — are asserted on the
reference's own output before the device is looked at."""
import ctypes as C
import functools

import numpy as np
import pytest

import srack_pkg
from tests import busosc_ref as R
from tests import busvca_ref as RA
from tests import busvcf_ref as RF

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-54321.5)  # what d_out holds before a call
GUARD = np.float32(12345.0)      # one float in front of d_out and one behind it
RUNS = (1, 2, 3, 5, 17, 40, 200)
NB, T = 130, 4100
CUTS = (1, 63, 64, 3972)
SEED = 11


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


def assert_same_state(got, ref, what=""):
    ok = R.same_state(got, ref)
    assert ok.all(), f"{what}: state differs at {tuple(np.argwhere(~ok)[0])}: {np.asarray(got)[~ok][:4]!r} against {np.asarray(ref)[~ok][:4]!r}"


def host(S, n_buses, rate=48000):
    """a handle to hang the table on: an oscillator into both channels, one voice in bus 0 of n_buses (never rendered here)"""
    p = S.Patch(rate, 64, 2)
    osc, out = p.add_module(S.MOD_OSCILLATOR), p.add_module(S.MOD_OUTPUT)
    for c in range(2):
        p.connect(osc, S.OSC_OUT_SINE, out, c)
    p.configure_voices(1)
    p.set_buses(n_buses)
    return p


def held_row(rng, n, lo, hi):
    """steps: values from [lo, hi] held for run lengths from RUNS"""
    row, at = np.empty(n, dtype=np.float32), 0
    while at < n:
        k = int(rng.choice(RUNS))
        row[at:at + k] = rng.uniform(lo, hi)
        at += k
    return row


def gate_row(rng, n, first_high):
    """runs of high values in (0, 2] and low values in [-1, 0] — both zeros among them —, run lengths from RUNS"""
    row, at, high = np.empty(n, dtype=np.float32), 0, bool(first_high)
    while at < n:
        k = int(rng.choice(RUNS[:6]))
        if high:
            v = 2.0 - rng.uniform(0.0, 2.0, k)
        else:
            v = -rng.uniform(0.0, 1.0, k)
            z = rng.random(k) < 0.3
            v[z] = np.where(rng.random(int(z.sum())) < 0.5, 0.0, -0.0)
        row[at:at + k] = v[:n - at]
        at, high = at + k, not high
    return row


@functools.lru_cache(maxsize=None)
def case(n_buses, n, seed):
    """-> (cv [n_buses][n], sync [n_buses][n], params [n_buses][3], port, aa, enabled): read-only, shared.  VAL 1 .. 2 at 48 kHz: 18 to 37
    samples per cycle, so wraps and PolyBLEP windows come within 100 samples.  Ports and flags cycle with different periods, so every
    wave holds all six classes; every seventh bus but the first is disabled.  CV rows by bus mod 4: held steps, audio rate, held steps
    up to delta >= 1, a held stretch followed by a moving one."""
    rng = np.random.default_rng(seed)
    b = np.arange(n_buses)
    params = np.stack([rng.uniform(1.0, 2.0, n_buses), rng.uniform(0.25, 2.0, n_buses) * np.where(rng.random(n_buses) < 0.3, -1, 1),
                       rng.uniform(-1.0, 1.0, n_buses)], axis=1).astype(np.float32)
    port, aa = (b % 3).astype(np.intc), ((b // 3) % 2).astype(np.intc)
    enabled = ((b % 7 != 6) | (b == 0)).astype(np.intc)
    cv, sync = np.empty((n_buses, n), dtype=np.float32), np.empty((n_buses, n), dtype=np.float32)
    for i in range(n_buses):
        kind = i % 4
        if kind == 0:
            cv[i] = held_row(rng, n, -1.0, 1.0)
        elif kind == 1:
            cv[i] = rng.uniform(-1.0, 1.0, n)
        elif kind == 2:
            cv[i] = held_row(rng, n, 3.0, 7.0)   # 440 * 2^(1.5 + 6) / 48000 = 1.66: increments beyond a whole cycle
        else:
            cv[i] = held_row(rng, n, -0.5, 0.5)
            cv[i, n // 2:] = rng.uniform(-0.5, 0.5, n - n // 2)
        sync[i] = gate_row(rng, n, first_high=i % 2 == 0)
    if n_buses > 20 and n > 300:
        cv[8, 100:140], cv[9, 150:160], cv[12, 200:210] = np.nan, np.inf, -np.inf   # (8, 9, 12: enabled)
        sync[5, 60:90] = np.nan
    for a in (cv, sync, params, port, aa, enabled):
        a.setflags(write=False)
    return cv, sync, params, port, aa, enabled


@functools.lru_cache(maxsize=None)
def reference(n_buses, n, seed, with_cv=True, with_sync=True, rate=48000):
    cv, sync, params, port, aa, enabled = case(n_buses, n, seed)
    out = R.bus_osc(cv if with_cv else None, sync if with_sync else None, params, port, aa, enabled, rate, n=n)
    for a in out:
        a.setflags(write=False)
    return out


def phases(cv, sync, params, rate, n=None, state=None):
    """the reference's own phase track: its raw saw without antialiasing is f32(pos) * 2 - 1 -> (saw [R][T], wraps per row)"""
    par = np.array(params, dtype=np.float32).reshape(-1, 3).copy()
    par[:, 1:] = (1.0, 0.0)
    saw, _ = R.bus_osc(cv, sync, par, np.full(len(par), R.SAW), np.zeros(len(par)), None, rate, state=state, n=n)
    return saw, np.count_nonzero(np.diff(saw, axis=1) < 0, axis=1)


def run_raw(S, p, n, cv=None, sync=None, off=(0, 0, 0)):
    """srack_buses_osc with d_cv, d_sync and d_out `off` floats further into their allocations; d_out holds SENTINEL beforehand, one GUARD
    float lies in front of it and one behind.  (The rows of d_out lie side by side: a write past a row's tail lands in the next row's head
    and shows in the comparison.)  -> (out [n_buses][n], the two guards as they came back)"""
    n_buses = p.n_buses()
    buf = np.full(n_buses * n + 2, SENTINEL, dtype=np.float32)
    buf[0] = buf[-1] = GUARD
    c = None if cv is None else np.ascontiguousarray(cv, dtype=np.float32)
    g = None if sync is None else np.ascontiguousarray(sync, dtype=np.float32)
    with S.DeviceScope() as dev:
        a_out = dev.upload(buf, off[2])
        a_cv = None if c is None else dev.upload(c, off[0])
        a_sync = None if g is None else dev.upload(g, off[1])
        p.bus_osc_raw(n, a_cv, a_sync, a_out + 4, None)
        dev.download(buf, a_out)
    return buf[1:-1].reshape(n_buses, n), (buf[0], buf[-1])


# ---- 1. shapes: tails of the last tile and of the last wave, one bus, one sample -----------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 4100])
@pytest.mark.parametrize("n_buses", [1, 63, 64, 65, 130])
def test_shapes(S, n_buses, n):
    cv, sync, params, port, aa, enabled = case(n_buses, n, SEED)
    ref, ref_state = reference(n_buses, n, SEED)
    on = np.flatnonzero(enabled)
    assert np.isfinite(ref[on[0]]).all() and (n < 64 or len(np.unique(ref[on[0]])) > 10)
    p = host(S, n_buses)
    p.set_bus_osc(params, port, aa, enabled)
    got, guards = run_raw(S, p, n, cv, sync)
    assert_same_bits(got, ref, f"{n_buses} buses x {n} samples")
    assert guards == (GUARD, GUARD)
    assert_same_state(p.bus_osc_state(), ref_state, "state")
    assert (got[enabled == 0].view(np.uint32) == 0).all()   # a disabled row is +0.0f
    assert f" busosc={len(on)}[cvsync]" in p.info()


# ---- 2. every port and flag wave-uniform, through each of the four kernels -------------------------------------------------------------------
@pytest.mark.parametrize("port", [R.SINE, R.SQUARE, R.SAW])
@pytest.mark.parametrize("aa", [1, 0])
def test_each_port_and_flag_with_and_without_rows(S, port, aa):
    n_buses, n = 70, 200
    cv, sync, params, _, _, _ = case(n_buses, n, SEED + 1)
    ports, flags = np.full(n_buses, port, dtype=np.intc), np.full(n_buses, aa, dtype=np.intc)
    p = host(S, n_buses)
    p.set_bus_osc(params, ports, flags)
    refs = []
    for c, g, note in ((None, None, "[--]"), (cv, None, "[cv-]"), (None, sync, "[-sync]"), (cv, sync, "[cvsync]")):
        p.reset_bus_osc()
        ref, ref_state = R.bus_osc(c, g, params, ports, flags, None, 48000, n=n)
        assert len(np.unique(ref[0])) > (1 if port == R.SQUARE else 20)   # (a square moves inside its PolyBLEP windows alone)
        got, guards = run_raw(S, p, n, c, g)
        assert_same_bits(got, ref, f"port {port}, antialiasing {aa}, {note}")
        assert_same_state(p.bus_osc_state(), ref_state, note)
        assert guards == (GUARD, GUARD) and f" busosc={n_buses}{note}" in p.info()
        refs.append(ref)
    assert all(not R.same_bits(refs[0], r).all() for r in refs[1:]), "the rows are meant to show"


# ---- 3. the big case: the guards on the reference, all six classes inside every wave ---------------------------------------------------------
def test_the_rows_visit_the_code_and_the_classes_mix_inside_a_wave(S):
    cv, sync, params, port, aa, enabled = case(NB, T, SEED)
    ref, ref_state = reference(NB, T, SEED)
    on = np.flatnonzero(enabled)
    # all three ports and both flags among the first 64 enabled buses, however the table is ordered
    assert len({(int(port[b]), int(aa[b])) for b in on[:64]}) == 6 and len(on) < NB
    # the guards, on the reference's own output: without rows every bus wraps and sits in PolyBLEP windows within 100 samples (a cycle is
    # 27 to 55 samples), at least twice within 200
    plain = list(on[:12])
    saw, wraps = phases(None, None, params[plain], 48000, n=200)
    assert wraps.min() >= 2 and np.count_nonzero(np.diff(saw[:, :100], axis=1) < 0, axis=1).min() >= 1, wraps
    sq, _ = R.bus_osc(None, None, np.array([[v, 1.0, 0.0] for v in params[plain, 0]], dtype=np.float32), np.full(len(plain), R.SQUARE), None, None, 48000, n=200)
    assert np.count_nonzero(np.abs(sq) != 1.0, axis=1).min() >= 8
    # sync: resets show as a phase of exactly 0 on a rising edge after the first sample; a gate whose first sample is high resets nothing
    track, _ = phases(cv[on], sync[on], params[on], 48000)
    rising = (sync[on][:, 1:] > 0) & ~(sync[on][:, :-1] > 0)
    resets = np.count_nonzero(rising & (track[:, 1:] == -1.0), axis=1)
    assert resets.min() >= 2, resets.min()
    first_high = sync[on][:, 0] > 0
    free, _ = phases(cv[on], None, params[on], 48000)
    assert first_high.any() and (~first_high).any() and R.same_bits(track[first_high, 0], free[first_high, 0]).all()
    # CV: held and moving stretches, increments of a whole cycle and more
    steady = cv[on][:, 1:] == cv[on][:, :-1]
    assert (steady.sum(axis=1) > 50).any() and ((~steady).sum(axis=1) > 1000).any() and ((steady.sum(axis=1) > 100) & ((~steady).sum(axis=1) > 100)).any()
    assert (440.0 * 2.0 ** (cv[on].astype(np.float64) + params[on, 0:1]) / 48000 >= 1.0).sum() > 1000
    assert np.isnan(ref[8]).any() and np.isnan(ref[9]).any() and np.isfinite(ref[10]).all()   # a NaN or infinite CV poisons its own row
    p = host(S, NB)
    p.set_bus_osc(params, port, aa, enabled)
    got, guards = run_raw(S, p, T, cv, sync)
    assert_same_bits(got, ref, "the big case")
    assert_same_state(p.bus_osc_state(), ref_state, "the big case's state")
    assert guards == (GUARD, GUARD)


# ---- 4. an LFO that wraps, another sample rate --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [48000, 44100])
def test_an_lfo_from_phases_near_one(S, rate):
    n_buses, n = 66, 300
    rng = np.random.default_rng(3)
    params = np.stack([np.full(n_buses, -8.0), rng.uniform(0.5, 1.5, n_buses), rng.uniform(-0.5, 0.5, n_buses)], axis=1).astype(np.float32)  # 1.72 Hz
    port, aa = (np.arange(n_buses) % 3).astype(np.intc), (np.arange(n_buses) % 2).astype(np.intc)
    delta = 440.0 * 2.0 ** -8.0 / rate
    pos = 1.0 - delta * rng.uniform(0.5, 250.0, n_buses)   # the wrap comes within the call
    state = np.stack([pos, np.ones(n_buses)], axis=1)
    ref, ref_state = R.bus_osc(None, None, params, port, aa, None, rate, state=state, n=n)
    saw, wraps = phases(None, None, params, rate, n=n, state=state)
    assert (wraps == 1).all() and (ref_state[:, 0] < pos).all()
    other, _ = R.bus_osc(None, None, params, port, aa, None, 92694 - rate, state=state, n=n)
    assert not R.same_bits(other, ref).all(), "the rate is meant to show"
    p = host(S, n_buses, rate=rate)
    p.set_bus_osc(params, port, aa)
    p.reset_bus_osc(pos)
    assert_same_state(p.bus_osc_state(), state, "reset_osc with phases")
    got, guards = run_raw(S, p, n)
    assert_same_bits(got, ref, f"LFOs at {rate} Hz")
    assert_same_state(p.bus_osc_state(), ref_state, "state behind the wrap")
    assert guards == (GUARD, GUARD) and f" busosc={n_buses}[--]" in p.info()


# ---- 5. CV rows: a call boundary inside a held stretch (the cache is not state) ---------------------------------------------------------------
def test_a_call_boundary_inside_a_held_cv_stretch(S):
    n_buses, n = 65, 260
    _, _, params, port, aa, _ = case(n_buses, n, SEED + 2)
    rng = np.random.default_rng(4)
    cv = np.repeat(rng.uniform(-1, 1, (n_buses, 4)).astype(np.float32), 65, axis=1)   # steps at 65, 130, 195
    cuts = (100, 1, 59, 100)                                                           # boundaries at 100, 101, 160: inside held stretches
    ref, ref_state = R.bus_osc(cv, None, params, port, aa, None, 48000)
    p = host(S, n_buses)
    p.set_bus_osc(params, port, aa)
    at, parts = 0, []
    for k in cuts:
        parts.append(run_raw(S, p, k, cv[:, at:at + k])[0])
        at += k
    assert_same_bits(np.concatenate(parts, axis=1), ref, "held CV across calls")
    assert_same_state(p.bus_osc_state(), ref_state, "state")
    # ... and the same value in the next call's first sample as in this call's last, after a call WITHOUT a CV row in between
    p.reset_bus_osc()
    a, _ = run_raw(S, p, 100, cv[:, :100])
    b, _ = run_raw(S, p, 30)
    c, _ = run_raw(S, p, 100, cv[:, 100:200])
    r1, s1 = R.bus_osc(cv[:, :100], None, params, port, aa, None, 48000)
    r2, s2 = R.bus_osc(None, None, params, port, aa, None, 48000, state=s1, n=30)
    r3, s3 = R.bus_osc(cv[:, 100:200], None, params, port, aa, None, 48000, state=s2)
    assert_same_bits(np.concatenate([a, b, c], axis=1), np.concatenate([r1, r2, r3], axis=1), "CV, none, CV")
    assert_same_state(p.bus_osc_state(), s3, "state")


# ---- 6. sync rows ---------------------------------------------------------------------------------------------------------------------------------
def test_sync_rows_and_a_call_without_one_in_between(S):
    n_buses, n = 64, 150
    cv, sync, params, port, aa, _ = case(n_buses, 3 * n, SEED + 3)
    sync = sync.copy()
    sync[:, 0] = 1.5            # every gate starts high: no reset, because `last` starts true
    sync[:, 2 * n] = 0.75       # ... and the third call starts high after a call without a row has cleared `last`: a reset
    sync[3, 20:50] = np.nan     # neither high nor low: `> 0.0` is false
    r1, s1 = R.bus_osc(cv[:, :n], sync[:, :n], params, port, aa, None, 48000)
    r2, s2 = R.bus_osc(cv[:, n:2 * n], None, params, port, aa, None, 48000, state=s1)
    r3, s3 = R.bus_osc(cv[:, 2 * n:], sync[:, 2 * n:], params, port, aa, None, 48000, state=s2)
    track, _ = phases(cv[:, :n], sync[:, :n], params, 48000)
    free, _ = phases(cv[:, :n], None, params, 48000)
    k = int(np.argmax(~(sync[0, :n] > 0)))   # bus 0's gate falls here: nothing was reset before
    assert 0 < k < n and R.same_bits(track[0, :k], free[0, :k]).all() and not R.same_bits(track, free).all()
    assert (s2[:, 1] == 0).all()             # d_sync == NULL: `last` becomes false
    t3, _ = phases(cv[:, 2 * n:], sync[:, 2 * n:], params, 48000, state=s2)
    assert (t3[:, 0] == -1.0).all() and (s2[:, 0] != 0).all()
    p = host(S, n_buses)
    p.set_bus_osc(params, port, aa)
    a, _ = run_raw(S, p, n, cv[:, :n], sync[:, :n])
    assert_same_state(p.bus_osc_state(), s1, "state behind the first call")
    b, _ = run_raw(S, p, n, cv[:, n:2 * n])
    assert_same_state(p.bus_osc_state(), s2, "state behind the call without a sync row")
    c, _ = run_raw(S, p, n, cv[:, 2 * n:], sync[:, 2 * n:])
    assert_same_bits(np.concatenate([a, b, c], axis=1), np.concatenate([r1, r2, r3], axis=1), "sync, none, sync")
    assert_same_state(p.bus_osc_state(), s3, "state")


# ---- 7. settings beyond the sliders -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_cv", [False, True])
def test_wide_val_and_non_finite_constants(S, with_cv):
    n_buses, n = 67, 130
    cv, _, params, port, aa, _ = case(n_buses, n, SEED + 4)
    params = params.copy()
    wild = {3: (20.0, None, None), 4: (200.0, None, None), 5: (2000.0, None, None), 6: (np.nan, None, None), 7: (-2000.0, None, None), 20: (-200.0, None, None),
            30: (None, np.inf, None), 31: (None, np.nan, None), 32: (None, None, -np.inf), 33: (None, None, np.nan), 34: (None, 0.0, np.inf), 64: (np.inf, None, None),
            65: (-np.inf, None, None)}
    for b, vals in wild.items():
        for f, v in enumerate(vals):
            if v is not None:
                params[b, f] = v
    c = cv if with_cv else None
    ref, ref_state = R.bus_osc(c, None, params, port, aa, None, 48000, n=n)
    tame = np.array([b for b in range(n_buses) if b not in wild])
    calm, _ = R.bus_osc(c, None, case(n_buses, n, SEED + 4)[2], port, aa, None, 48000, n=n)
    assert np.isnan(ref[6, 1:]).all() and np.isnan(ref[31]).all() and np.isnan(ref[33]).all() and np.isinf(ref[32]).all()
    assert R.same_bits(ref[tame], calm[tame]).all() and np.isfinite(ref[tame]).all()   # one bus's NaNs touch no other row
    p = host(S, n_buses)
    p.set_bus_osc(params, port, aa)
    got, guards = run_raw(S, p, n, c)
    assert_same_bits(got, ref, "wide settings")
    assert_same_state(p.bus_osc_state(), ref_state, "state")
    assert guards == (GUARD, GUARD)


# ---- 8. cuts ------------------------------------------------------------------------------------------------------------------------------------
def test_cuts_give_the_same_bits_and_the_oracles_state(S):
    cv, sync, params, port, aa, enabled = case(NB, T, SEED)
    ref, ref_state = reference(NB, T, SEED)
    assert sum(CUTS) == T
    p, q = host(S, NB), host(S, NB)
    for h in (p, q):
        h.set_bus_osc(params, port, aa, enabled)
    whole, _ = run_raw(S, p, T, cv, sync)
    at, parts = 0, []
    for k in CUTS:
        parts.append(run_raw(S, q, k, cv[:, at:at + k], sync[:, at:at + k])[0])
        at += k
    cut = np.concatenate(parts, axis=1)
    assert_same_bits(whole, ref, "uncut")
    assert_same_bits(cut, ref, "cut as 1, 63, 64, 3 972")
    sp, sq = p.bus_osc_state(), q.bus_osc_state()
    assert_same_state(sp, sq, "state, cut and uncut")
    assert_same_state(sp, ref_state, "state against the oracle's OSC_POS and OSC_SYNC_LAST")
    on = enabled != 0
    assert (sp[on, 0] != 0).any() and (sp[~on] == (0.0, 1.0)).all()


# ---- 9. lifecycle on the device -------------------------------------------------------------------------------------------------------------------
def test_slider_enable_reset_and_an_edit(S):
    n_buses, n = 70, 100
    cv, sync, params, port, aa, _ = case(n_buses, 3 * n, SEED + 5)
    enabled = np.ones(n_buses, dtype=np.intc)
    enabled[[2, 40, 69]] = 0
    p = S.Patch(48000, 64, 2)
    p.ids = S.build_p1(p)
    p.configure_voices(4)
    p.set_buses(n_buses, np.arange(4, dtype=np.intc))
    p.set_bus_osc(params, port, aa, enabled)
    r1, s1 = R.bus_osc(cv[:, :n], sync[:, :n], params, port, aa, enabled, 48000)
    a, guards = run_raw(S, p, n, cv[:, :n], sync[:, :n])
    assert_same_bits(a, r1, "first call")
    assert (a[[2, 40, 69]].view(np.uint32) == 0).all() and guards == (GUARD, GUARD)
    # set_osc again is the slider: other parameters, ports and flags, the state stays; bus 2 joins fresh, bus 5 leaves and drops its state;
    # an edit that re-flattens the patch changes nothing
    params2, port2, aa2 = params[::-1].copy(), ((port + 1) % 3).astype(np.intc), (1 - aa).astype(np.intc)
    enabled2 = enabled.copy()
    enabled2[2], enabled2[5] = 1, 0
    p.set_bus_osc(params2, port2, aa2, enabled2)
    p.set_field(p.ids["vcf"], S.VCF_RES, 0.3)
    s1b = s1.copy()
    s1b[5] = (0.0, 1.0)
    assert s1[5, 0] != 0 and (s1[2] == (0.0, 1.0)).all()
    assert_same_state(p.bus_osc_state(), s1b, "state behind the slider")
    r2, s2 = R.bus_osc(cv[:, n:2 * n], sync[:, n:2 * n], params2, port2, aa2, enabled2, 48000, state=s1b)
    b, _ = run_raw(S, p, n, cv[:, n:2 * n], sync[:, n:2 * n])
    assert_same_bits(b, r2, "behind the slider")
    assert_same_state(p.bus_osc_state(), s2, "state")
    fresh2, _ = R.bus_osc(cv[:, n:2 * n], sync[:, n:2 * n], params2, port2, aa2, enabled2, 48000)
    assert not R.same_bits(fresh2, r2).all(), "the state is meant to show"
    # bus 5 comes back: fresh
    p.set_bus_osc(params2, port2, aa2, enabled)
    s2b = s2.copy()
    s2b[2] = (0.0, 1.0)
    s2b[5] = (0.0, 1.0)
    assert_same_state(p.bus_osc_state(), s2b, "bus 2 left, bus 5 joined")
    # reset_osc with phases: quadrature
    pos = (np.arange(n_buses) % 4) / 4.0
    p.reset_bus_osc(pos)
    s3 = np.stack([np.where(enabled != 0, pos, 0.0), np.ones(n_buses)], axis=1)
    assert_same_state(p.bus_osc_state(), s3, "reset with phases")
    r3, s4 = R.bus_osc(cv[:, 2 * n:], sync[:, 2 * n:], params2, port2, aa2, enabled, 48000, state=s3)
    c, _ = run_raw(S, p, n, cv[:, 2 * n:], sync[:, 2 * n:])
    assert_same_bits(c, r3, "from the phases")
    assert_same_state(p.bus_osc_state(), s4, "state")
    p.reset_bus_osc()
    assert (p.bus_osc_state() == (0.0, 1.0)).all()
    d, _ = run_raw(S, p, n, cv[:, :n], sync[:, :n])
    assert_same_bits(d, R.bus_osc(cv[:, :n], sync[:, :n], params2, port2, aa2, enabled, 48000)[0], "after reset_osc(NULL)")
    # another n_buses drops the stage and its note
    assert " busosc=67[cvsync]" in p.info()
    p.set_buses(n_buses + 1, np.arange(4, dtype=np.intc))
    assert p.get_bus_osc()[0] == 0 and "busosc" not in p.info()


@pytest.mark.parametrize("off", [(1, 2, 3), (3, 1, 2), (2, 3, 1), (0, 0, 1)])
def test_bases_offset_by_floats(S, off):
    n_buses, n = 67, 131
    cv, sync, params, port, aa, enabled = case(n_buses, n, SEED + 6)
    ref, _ = reference(n_buses, n, SEED + 6)
    p = host(S, n_buses)
    p.set_bus_osc(params, port, aa, enabled)
    got, guards = run_raw(S, p, n, cv, sync, off=off)
    assert_same_bits(got, ref, f"offsets {off}")
    assert guards == (GUARD, GUARD)


# ---- 10. the whole chain on the device: the rows never leave it -----------------------------------------------------------------------------------
def test_lfos_gate_the_vcas_and_sweep_the_filters(S):
    V, n_buses, n = 64, 4, 600

    def make():
        p = S.Patch(48000, 64, 2)
        p.ids = S.build_p1(p, lfo_val=0.0)
        p.configure_voices(V)
        det, cut = S.p1_voice_params(V)
        p.set_voice_field(p.ids["osc_a"], S.OSC_VAL, det)
        p.set_voice_field(p.ids["vcf"], S.VCF_FREQ, cut)
        p.set_buses(n_buses, np.arange(V, dtype=np.intc) % n_buses)
        p.set_master()
        return p

    p, twin = make(), make()
    # a square LFO per bus as the VCAs' gate (-1.55 .. -1.1: about 160 Hz, a few periods in the call) ...
    gate_par = np.array([[-1.55, 1.0, 0.0], [-1.4, 1.0, 0.0], [-1.25, 2.0, 0.5], [-1.1, 1.0, -0.25]], dtype=np.float32)
    # ... then a sine per bus, scaled and shifted into the filters' CV
    sweep_par = np.array([[-3.0, 0.4, 0.1], [-2.5, 0.3, 0.0], [-2.0, 0.5, -0.2], [-1.5, 0.2, 0.3]], dtype=np.float32)
    vpar = np.array([[0.001, 0.002, 0.5, 0.003], [0.0, 0.001, 0.7, 0.001], RA.DEFAULTS, [0.002, 0.002, 0.5, 0.001]], dtype=np.float32)
    fpar = np.tile(np.array([0.1, 0.6, 0.7], dtype=np.float32), (n_buses, 1))
    gated, lowpass, all_on = np.full(n_buses, RA.GATE, dtype=np.intc), np.zeros(n_buses, dtype=np.intc), np.ones(n_buses, dtype=np.intc)
    square, sine = np.full(n_buses, R.SQUARE, dtype=np.intc), np.full(n_buses, R.SINE, dtype=np.intc)
    p.set_bus_vca(vpar, gated)
    p.set_bus_filter(fpar, lowpass, all_on)
    a = p.render_buses(n, frames=True, mix=True, stats=True)
    b = twin.render_buses(n, frames=True, mix=True, stats=True)
    bm = np.ascontiguousarray(a[3], dtype=np.float32)
    gates, s_gate = R.bus_osc(None, None, gate_par, square, None, None, 48000, n=n)
    sweeps, _ = R.bus_osc(None, None, sweep_par, sine, None, None, 48000, state=s_gate, n=n)   # (the slider: the phases carry on)
    assert ((gates > 0).sum(axis=1) > 100).all() and ((gates <= 0).sum(axis=1) > 100).all() and len(np.unique(sweeps[0])) > 100
    want_vca, _, _, _ = RA.bus_vca(bm, gates, vpar, gated, np.zeros(n_buses), 48000)
    want, _ = RF.bus_filter(want_vca, sweeps, fpar, lowpass, all_on)
    flat, _ = RF.bus_filter(want_vca, None, fpar, lowpass, all_on)
    assert np.isfinite(want).all() and np.count_nonzero(want != flat) > want.size // 4 and np.count_nonzero(want_vca != bm) > bm.size // 4
    got, got_master, twin_master = np.empty_like(want), np.empty((2, n), dtype=np.float32), np.empty((2, n), dtype=np.float32)
    with S.DeviceScope() as dev:
        d_rows, d_ctl, d_cv, d_out, d_m = dev.upload(bm), dev.alloc(4 * n_buses * n), dev.alloc(4 * n_buses * n), dev.alloc(bm.nbytes), dev.alloc(got_master.nbytes)
        p.set_bus_osc(gate_par, square)
        p.bus_osc_raw(n, None, None, d_ctl)
        p.set_bus_osc(sweep_par, sine)
        p.bus_osc_raw(n, None, None, d_cv)
        p.bus_vca_raw(n, d_rows, 2, d_ctl, d_rows)
        p.bus_filter_raw(n, d_rows, 2, d_cv, d_out)
        dev.download(got, d_out)
        d_twin = dev.upload(bm)
        p.master_raw(n, d_twin, 2, d_m)
        dev.download(got_master, d_m)
        twin.master_raw(n, d_twin, 2, d_m)
        dev.download(twin_master, d_m)
    assert_same_bits(got, want, "square LFOs gate the VCAs, sines sweep the filters")
    # a twin handle without the stage renders the same frames, mix, statistics and bus mixes, and the same master
    for x, y, what in zip(a, b, ("frames", "mix", "statistics", "bus mixes")):
        assert np.abs(np.nan_to_num(x)).max() > 0, what
        assert (np.ascontiguousarray(x).view(np.uint8) == np.ascontiguousarray(y).view(np.uint8)).all(), what
    a2, b2 = p.render_buses(n, frames=True, mix=True, stats=True), twin.render_buses(n, frames=True, mix=True, stats=True)
    for x, y, what in zip(a2, b2, ("frames", "mix", "statistics", "bus mixes")):
        assert (np.ascontiguousarray(x).view(np.uint8) == np.ascontiguousarray(y).view(np.uint8)).all(), f"{what}, behind the oscillators"
    assert_same_bits(got_master, twin_master, "master")
    ia, ib = p.info(), twin.info()
    token = " busosc=4[--]"
    assert ia.count(token) == 1 and "busosc" not in ib
    assert ia.index(token) < ia.index(" busvcf=") < ia.index(" busvca=")
    assert ia.split(" busosc=")[0] == ib.split(" master=")[0]   # whatever stands in front of the console's notes


# ---- 11. a caller's stream, settings replaced between calls in flight ---------------------------------------------------------------------------
def test_set_osc_between_calls_on_a_stream(S):
    """six calls on one non-blocking stream, nothing synchronised in between, set_osc in front of every call: every call gives the
    reference for the settings it was issued under and the state the calls before it left"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    n_buses, n = 130, 200
    cv, sync, params, port, aa, enabled = case(n_buses, n, SEED + 7)
    rng = np.random.default_rng(SEED + 8)
    settings, refs, state = [], [], None
    for k in range(6):
        par = params.copy()
        par[:, 0] = rng.permutation(params[:, 0])
        settings.append((par, rng.permutation(port).astype(np.intc), rng.permutation(aa).astype(np.intc)))
        ref, state = R.bus_osc(cv, sync, *settings[-1], enabled, 48000, state=state)
        refs.append(ref)
    assert all(np.count_nonzero(~R.same_bits(refs[k], refs[k + 1])) > refs[k].size // 2 for k in range(5))
    lib, st = S.lib, C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(st), 1) == 0   # hipStreamNonBlocking
    got = np.empty((6, n_buses, n), dtype=np.float32)
    try:
        with S.DeviceScope(st) as dev:
            d_cv, d_sync, d_out = dev.upload(cv), dev.upload(sync), dev.alloc(got.nbytes)
            assert lib.srack_device_sync(None) == 0
            p = host(S, n_buses)
            for k, (par, po, fl) in enumerate(settings):
                p.set_bus_osc(par, po, fl, enabled)
                p.bus_osc_raw(n, d_cv, d_sync, d_out + k * got[0].nbytes, st)
            dev.download(got, d_out)
        final = p.bus_osc_state()
    finally:
        assert hip.hipStreamDestroy(st) == 0
    for k in range(6):
        assert_same_bits(got[k], refs[k], f"call {k}")
    assert_same_state(final, state, "state behind the six calls")
