"""The bus filters on the device (srack_buses_filter, csrc/busvcf.hip.h): a Moog ladder per (enabled bus, channel) row, a lane per row,
tiles of 64 rows x 64 samples through LDS.

Rows are seeded f32 values fed straight into srack_buses_filter — mostly in [-2, 2], some buses scaled by 1e7 so that both arms of
vcf_run (the v_med3 clamps and the literal ones) run.  The reference is tests/busvcf_ref.py, the ladder stated in NumPy f32, which
tests/test_bus_filter_host.py holds to the oracle's MoogFilterModule bit for bit.  The criterion is BIT EQUALITY (NaN matching NaN) —
derived, not measured: both sides perform the same single-rounded IEEE f32 operations in the same order (the library is built with
-ffp-contract=off).  No tolerance anywhere in this file.  Every comparison is preceded by a guard that the reference is audible: finite,
not all zero, different from its input and different between ports."""
import ctypes as C

import numpy as np
import pytest

import srack_pkg
from oracle import oracle as O
from tests import busvcf_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-54321.5)  # what d_out holds before a call, wherever the call must not write
GUARD = np.float32(12345.0)      # one float behind d_out
EXACT = 1


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


def host(S, n_buses, channels=2):
    """a handle to hang the table on: an oscillator into every channel, one voice in bus 0 of n_buses (never rendered here)"""
    p = S.Patch(48000, 64, channels)
    osc, out = p.add_module(S.MOD_OSCILLATOR), p.add_module(S.MOD_OUTPUT)
    for c in range(channels):
        p.connect(osc, S.OSC_OUT_SINE, out, c)
    p.configure_voices(1)
    p.set_buses(n_buses)
    return p


def case(n_buses, rc, T, seed, with_cv=True, disabled=0.25):
    """-> (rows [n_buses][rc][T], cv [n_buses][T] or None, params [n_buses][3], port [n_buses], enabled [n_buses])"""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-2.0, 2.0, (n_buses, rc, T)).astype(np.float32)
    big = rng.random(n_buses) < 0.2
    big[min(2, n_buses - 1)] = True
    rows[big] *= np.float32(1e7)   # a mix of thousands of voices: past the bound below which the ladder may clamp with v_med3
    cv = None
    if with_cv:
        ph = rng.uniform(0, 6.28, (n_buses, 1)) + np.arange(T)[None, :] * rng.uniform(0.01, 0.2, (n_buses, 1))
        cv = np.sin(ph).astype(np.float32)
    params = np.stack([rng.uniform(0.02, 0.85, n_buses), rng.uniform(-0.1, 1.2, n_buses), rng.uniform(-1.0, 1.0, n_buses)], axis=1).astype(np.float32)
    port = rng.integers(0, 3, n_buses).astype(np.intc)
    enabled = (rng.random(n_buses) >= disabled).astype(np.intc)
    enabled[0] = 1
    return rows, cv, params, port, enabled


def assert_audible(rows, cv, params, port, enabled, ref, what=""):
    """the reference is worth comparing with: finite, not silent, not its input, and another port would have given other samples"""
    on = np.flatnonzero(enabled)
    used = min(rows.shape[1], 2)
    y, x = ref[on, :used], rows[on, :used]
    assert np.isfinite(y).all(), f"{what}: the reference is not finite"
    assert np.count_nonzero(y) >= max(1, y.size // 4), f"{what}: the reference is (nearly) silent"
    assert np.count_nonzero(y != x) >= max(1, y.size // 4), f"{what}: the reference is its input"
    other, _ = R.bus_filter(rows, cv, params, (np.asarray(port) + 1) % 3, enabled)
    assert np.count_nonzero(other[on, :used] != y) >= max(1, y.size // 4), f"{what}: the ports do not differ"


def run_raw(S, p, rows, cv=None, in_place=False, off_rows=0, off_cv=0, off_out=0):
    """srack_buses_filter with d_rows, d_cv and d_out `off_*` floats into their allocations.  Out of place d_out holds SENTINEL beforehand
    (it comes back wherever the call did not write); one GUARD float lies behind the output either way.
    -> (out of rows' shape, the guard as it came back)"""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    buf = np.full(x.size + 1, SENTINEL, dtype=np.float32)
    if in_place:
        buf[:-1] = x.ravel()
    buf[-1] = GUARD
    c = None
    if cv is not None:
        c = np.ascontiguousarray(cv, dtype=np.float32)
        assert c.shape == (x.shape[0], x.shape[2])
    with S.DeviceScope() as dev:
        a_out = dev.upload(buf, off_out)
        a_in = a_out if in_place else dev.upload(x, off_rows)
        a_cv = None if c is None else dev.upload(c, off_cv)
        p.bus_filter_raw(x.shape[2], a_in, x.shape[1], a_cv, a_out, None)
        dev.download(buf, a_out)
    return buf[:-1].reshape(x.shape), buf[-1]


# ---- 1. against the reference: partial and full waves and tiles ---------------------------------------------------------------------------
@pytest.mark.parametrize("with_cv", [True, False])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("n_buses", [1, 31, 32, 33, 130])
def test_against_the_reference(S, n_buses, T, with_cv):
    """31 / 32 / 33 stereo buses: a partial wave, a full one, two with the second partial (before disabling; 130: several); 63 / 64 / 65 /
    200 samples: a partial tile, a full one, two with a tail, four with a tail"""
    rows, cv, params, port, enabled = case(n_buses, 2, T, 1000 * n_buses + T, with_cv)
    ref, ref_state = R.bus_filter(rows, cv, params, port, enabled)
    assert_audible(rows, cv, params, port, enabled, ref, "reference")
    p = host(S, n_buses)
    p.set_bus_filter(params, port, enabled)
    got = p.bus_filter(rows, cv)
    assert_same_bits(got, ref, "output")
    assert_same_bits(p.bus_filter_state(), ref_state, "state")
    assert f" busvcf={int(enabled.sum())}[{(2 * int(enabled.sum()) + 63) // 64} waves]" in p.info()


# ---- 2. row_channels ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [1, 2, 3, 8])
def test_row_channels(S, rc):
    n_buses, T = 70, 97
    rows, cv, params, port, enabled = case(n_buses, rc, T, 20 + rc)
    ref, ref_state = R.bus_filter(rows, cv, params, port, enabled)
    assert_audible(rows, cv, params, port, enabled, ref, f"row_channels {rc}")
    p = host(S, n_buses)
    p.set_bus_filter(params, port, enabled)
    got, guard = run_raw(S, p, rows, cv)
    used = min(rc, 2)
    assert_same_bits(got[:, :used], ref[:, :used], f"row_channels {rc}")
    assert (got[:, used:] == SENTINEL).all() and guard == GUARD, "channels beyond the second, or the float behind the output, were written"
    assert_same_bits(p.bus_filter_state(), ref_state, "state")   # with one channel the second channel's state stays at zero
    if rc == 1:
        assert (ref_state[:, 1] == 0).all() and p.info().count(f" busvcf={int(enabled.sum())}[{(int(enabled.sum()) + 63) // 64} waves]") == 1


# ---- 3. cuts -----------------------------------------------------------------------------------------------------------------------------------
def test_cuts_give_the_same_bits(S):
    n_buses, T, cuts = 40, 200, (1, 63, 64, 65, 7)
    assert sum(cuts) == T
    rows, cv, params, port, enabled = case(n_buses, 2, T, 33)
    ref, ref_state = R.bus_filter(rows, cv, params, port, enabled)
    assert_audible(rows, cv, params, port, enabled, ref, "cuts")
    one = host(S, n_buses)
    one.set_bus_filter(params, port, enabled)
    whole = one.bus_filter(rows, cv)
    assert_same_bits(whole, ref, "one call")
    p = host(S, n_buses)
    p.set_bus_filter(params, port, enabled)
    parts, at = [], 0
    for n in cuts:
        parts.append(p.bus_filter(rows[:, :, at:at + n], cv[:, at:at + n]))
        at += n
    assert_same_bits(np.concatenate(parts, axis=2), whole, "calls of 1, 63, 64, 65, 7")
    assert_same_bits(p.bus_filter_state(), one.bus_filter_state(), "state, cut and uncut")
    assert_same_bits(p.bus_filter_state(), ref_state, "state")


# ---- 4. any 4-byte aligned address -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off_rows,off_cv,off_out", [(1, 2, 3), (2, 3, 1), (3, 1, 2), (1, 0, 0), (0, 0, 3)])
def test_bases_offset_by_floats(S, off_rows, off_cv, off_out):
    n_buses, T = 37, 131
    rows, cv, params, port, enabled = case(n_buses, 2, T, 44)
    ref, _ = R.bus_filter(rows, cv, params, port, enabled)
    assert_audible(rows, cv, params, port, enabled, ref, "offsets")
    p = host(S, n_buses)
    p.set_bus_filter(params, port, enabled)
    got, guard = run_raw(S, p, rows, cv, off_rows=off_rows, off_cv=off_cv, off_out=off_out)
    assert_same_bits(got, ref, f"offsets {off_rows}, {off_cv}, {off_out}")
    assert guard == GUARD


# ---- 5. in place -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc,T", [(2, 200), (3, 65), (1, 64)])
def test_in_place_gives_the_out_of_place_bits(S, rc, T):
    n_buses = 45
    rows, cv, params, port, enabled = case(n_buses, rc, T, 55 + rc)
    ref, ref_state = R.bus_filter(rows, cv, params, port, enabled)
    assert_audible(rows, cv, params, port, enabled, ref, "in place")
    used = min(rc, 2)
    p = host(S, n_buses)
    p.set_bus_filter(params, port, enabled)
    out, _ = run_raw(S, p, rows, cv)
    q = host(S, n_buses)
    q.set_bus_filter(params, port, enabled)
    inp, guard = run_raw(S, q, rows, cv, in_place=True, off_out=1)
    assert_same_bits(inp[:, :used], out[:, :used], "in place against out of place")
    assert_same_bits(inp[:, :used], ref[:, :used], "in place against the reference")
    assert_same_bits(inp[:, used:], rows[:, used:], "channels beyond the second, in place")   # left alone
    assert_same_bits(inp[enabled == 0], rows[enabled == 0], "disabled buses, in place")
    assert guard == GUARD
    assert_same_bits(q.bus_filter_state(), ref_state, "state")
    assert_same_bits(q.bus_filter(rows, cv, in_place=True)[:, :used], p.bus_filter(rows, cv)[:, :used], "the wrapper's in_place, second call")


def test_overlaps_are_refused(S):
    n_buses, T = 3, 16
    p = host(S, n_buses)
    p.set_bus_filter()
    nbytes, cvbytes = n_buses * 2 * T * 4, n_buses * T * 4
    with S.DeviceScope() as dev:
        d = dev.alloc(4 * nbytes)
        base = d + nbytes
        for d_out in (base + 4, base - 4, base + nbytes - 4, base - nbytes + 4):
            assert S.lib.srack_buses_filter(p.h, T, base, 2, None, d_out, None) == S.ERR_INVALID, d_out - base
        for d_cv in (base, base + nbytes - 4, base - cvbytes + 4):
            assert S.lib.srack_buses_filter(p.h, T, base, 2, d_cv, base, None) == S.ERR_INVALID, d_cv - base
            assert S.lib.srack_buses_filter(p.h, T, base + 2 * nbytes, 2, d_cv, base, None) == S.ERR_INVALID, d_cv - base
        assert "busvcf" not in p.info() and (p.bus_filter_state() == 0).all()   # nothing ran
        # neighbours are fine: d_out right behind d_rows, d_cv right behind d_out
        assert S.lib.srack_device_from_host(d, np.zeros(nbytes, dtype=np.float32).ctypes.data_as(C.c_void_p), 4 * nbytes, None) == 0
        assert S.lib.srack_buses_filter(p.h, T, d, 2, d + 2 * nbytes, d + nbytes, None) == S.OK


# ---- 6. special values are ordinary floats --------------------------------------------------------------------------------------------------
def test_special_values_stay_in_their_bus(S):
    n_buses, T = 40, 150
    rows, cv, params, port, enabled = case(n_buses, 2, T, 66, disabled=0.0)
    params[27, 1] = 0.6   # (a resonance that -inf, clamped to 0, differs from)
    base_ref, _ = R.bus_filter(rows, cv, params, port, enabled)
    assert_audible(rows, cv, params, port, enabled, base_ref, "without the specials")
    p = host(S, n_buses)
    p.set_bus_filter(params, port, enabled)
    base = p.bus_filter(rows, cv)
    assert_same_bits(base, base_ref, "without the specials")
    rows2, cv2, params2 = rows.copy(), cv.copy(), params.copy()
    rows2[3, 0, 10] = np.nan
    rows2[7, 1, 70] = np.inf
    rows2[11, 0, 64] = -np.inf
    cv2[15, 30] = np.nan
    params2[19, 0] = np.nan
    params2[23, 2] = np.inf
    params2[27, 1] = -np.inf
    touched = [3, 7, 11, 15, 19, 23, 27]
    ref, ref_state = R.bus_filter(rows2, cv2, params2, port, enabled)
    q = host(S, n_buses)
    q.set_bus_filter(params2, port, enabled)
    got = q.bus_filter(rows2, cv2)
    assert_same_bits(got, ref, "with the specials")
    assert_same_bits(q.bus_filter_state(), ref_state, "state with the specials")
    rest = np.setdiff1d(np.arange(n_buses), touched)
    assert_same_bits(got[rest], base[rest], "the buses the specials did not touch")
    for b in touched:
        assert not R.same_bits(ref[b], base_ref[b]).all(), f"bus {b}: the special value changed nothing in the reference"
    assert np.isnan(ref[3, 0, 10]) or np.isnan(ref[3, 0]).any() or not R.same_bits(ref[3, 0], base_ref[3, 0]).all()
    assert R.same_bits(ref[3, 1], base_ref[3, 1]).all() and R.same_bits(ref[7, 0], base_ref[7, 0]).all(), "a bus's other channel is another module"


# ---- 7. against the reference's module, end to end --------------------------------------------------------------------------------------------
def test_two_voices_one_bus_against_the_oracles_mixer_and_filter(S):
    T, B = 512, 64
    a, b, g0, g1 = -1.0, -0.4167, 0.75, 0.5
    freq, res, exp_amt = 0.25, 0.7, 0.4
    o = O.OraclePatch(48000, B, 2)
    osc_a, osc_b, lfo, mixer, vcf, out = (o.add_module(m) for m in (S.MOD_OSCILLATOR, S.MOD_OSCILLATOR, S.MOD_OSCILLATOR, S.MOD_MONO_MIXER, S.MOD_MOOG_FILTER, S.MOD_OUTPUT))
    o.set_field(osc_a, S.OSC_VAL, a)
    o.set_field(osc_b, S.OSC_VAL, b)
    o.set_field(lfo, S.OSC_VAL, -3.0)
    o.set_field(mixer, S.MIX_GAIN0, g0)
    o.set_field(mixer, S.MIX_GAIN1, g1)
    for f, v in ((S.VCF_FREQ, freq), (S.VCF_RES, res), (S.VCF_EXP_AMT, exp_amt)):
        o.set_field(vcf, f, v)
    o.connect(osc_a, S.OSC_OUT_SAW, mixer, 0)
    o.connect(osc_b, S.OSC_OUT_SAW, mixer, 1)
    o.connect(mixer, 0, vcf, 0)
    o.connect(lfo, S.OSC_OUT_SINE, vcf, 1)
    o.connect(vcf, S.VCF_OUT_BANDPASS, out, 0)
    o.connect(lfo, S.OSC_OUT_SINE, out, 1)
    want, tap = o.render(T, tap=(mixer, 0))
    assert np.isfinite(want).all() and np.abs(want[0]).max() > 1e-2 and np.abs(want[1]).max() > 0.5 and np.abs(tap).max() > 0.5
    assert np.count_nonzero(want[0] != tap) > T // 2

    p = S.Patch(48000, B, 2)
    osc, pout = p.add_module(S.MOD_OSCILLATOR), p.add_module(S.MOD_OUTPUT)
    p.connect(osc, S.OSC_OUT_SAW, pout, 0)
    p.connect(osc, S.OSC_OUT_SAW, pout, 1)
    p.configure_voices(2)
    p.set_voice_field(osc, S.OSC_VAL, np.array([a, b], dtype=np.float32))
    p.set_buses(1, np.zeros(2, dtype=np.intc), np.array([g0, g1], dtype=np.float32))
    _, _, _, bm = p.render_buses(T, flags=EXACT)
    assert_same_bits(bm[0, 0], tap, "the bus mix against the oracle's mixer")
    p.set_bus_filter(np.array([[freq, res, exp_amt]], dtype=np.float32), [S.VCF_OUT_BANDPASS])
    got = p.bus_filter(bm, want[1][None, :])
    assert_same_bits(got[0, 0], want[0], "the bus filter against the oracle's MoogFilterModule")
    assert_same_bits(got[0, 1], want[0], "the second channel: the same samples through a module of its own")
    state = np.array([o.get_field(vcf, S.VCF_ST_F + k) for k in range(R.NSTATE)], dtype=np.float32)
    assert_same_bits(p.bus_filter_state()[0, 0], state, "state against the oracle's")


# ---- 8. lifecycle --------------------------------------------------------------------------------------------------------------------------------
def test_slider_enable_disable_and_reset(S):
    n_buses, T = 36, 90
    rows, cv, params, port, enabled = case(n_buses, 2, 2 * T, 77, disabled=0.0)
    first, second = (rows[:, :, :T], cv[:, :T]), (rows[:, :, T:], cv[:, T:])
    en1 = enabled.copy()
    en1[[4, 20]] = 0            # 4 and 20 join later
    p = host(S, n_buses)
    p.set_bus_filter(params, port, en1)
    ref1, st1 = R.bus_filter(*first, params, port, en1)
    assert_audible(*first, params, port, en1, ref1, "first call")
    assert_same_bits(p.bus_filter(*first), ref1, "first call")
    assert_same_bits(p.bus_filter_state(), st1, "state after the first call")
    # set_filter again is the slider: parameters and ports change, state stays; 4 and 20 start from zeros, 9 is disabled and drops its state
    params2 = params.copy()
    params2[:, 0] = np.float32(0.9) - params[:, 0]
    port2 = (port + 1) % 3
    en2 = enabled.copy()
    en2[9] = 0
    p.set_bus_filter(params2, port2, en2)
    carried = st1.copy()
    carried[9] = 0
    assert_same_bits(p.bus_filter_state(), carried, "state behind set_filter: moved with its buses, nothing run")
    ref2, st2 = R.bus_filter(*second, params2, port2, en2, carried)
    assert_audible(*second, params2, port2, en2, ref2, "second call")
    fresh, _ = R.bus_filter(*second, params2, port2, en2)
    assert not R.same_bits(ref2, fresh).all(), "the carried state is meant to show"
    assert_same_bits(p.bus_filter(*second), ref2, "second call: sliders moved, neighbours carried on, late buses from zeros")
    assert_same_bits(p.bus_filter_state(), st2, "state after the second call")
    # enabling 9 again starts it from zeros
    p.set_bus_filter(params2, port2, enabled)
    back = st2.copy()
    back[9] = 0
    assert_same_bits(p.bus_filter_state(), back, "a bus enabled again starts from zeros")
    ref3, st3 = R.bus_filter(*first, params2, port2, enabled, back)
    assert_same_bits(p.bus_filter(*first), ref3, "third call")
    assert_same_bits(p.bus_filter_state(), st3, "state after the third call")
    # reset_filter zeroes every state and keeps the parameters
    p.reset_bus_filter()
    assert (p.bus_filter_state() == 0).all()
    n, a, o, e = p.get_bus_filter()
    assert n == n_buses and (a == params2).all() and (o == port2).all() and (e == enabled).all()
    ref4, st4 = R.bus_filter(*second, params2, port2, enabled)
    assert_same_bits(p.bus_filter(*second), ref4, "behind a reset")
    assert_same_bits(p.bus_filter_state(), st4, "state behind a reset")


def test_not_part_of_the_program(S):
    """the filters change nothing a render, the reverbs or the master write, survive an edit that re-flattens, and a twin handle that never
    heard of them says the same about itself once the ` busvcf=` token is taken out"""
    V, n_buses, T = 64, 4, 300

    def make():
        p = S.Patch(48000, 64, 2)
        p.ids = S.build_p1(p, lfo_val=0.0)
        p.configure_voices(V)
        det, cut = S.p1_voice_params(V)
        p.set_voice_field(p.ids["osc_a"], S.OSC_VAL, det)
        p.set_voice_field(p.ids["vcf"], S.VCF_FREQ, cut)
        p.set_buses(n_buses, np.arange(V, dtype=np.intc) % n_buses)
        p.set_bus_reverbs()
        p.set_master()
        p.set_sends([0], [1])
        return p

    p, twin = make(), make()
    params = np.array([[0.3, 0.6, 0.5], [0.1, 0.9, -0.5], [0.6, 0.2, 0.3], [0.2, 0.5, 0.5]], dtype=np.float32)
    port = np.array([0, 1, 2, 1], dtype=np.intc)
    p.set_bus_filter(params, port)
    ref_state = None
    cv = np.sin(np.arange(2 * T) * 0.05)[None, :].repeat(n_buses, 0).astype(np.float32)
    for k in range(2):
        a = p.render_buses(T, frames=True, mix=True, stats=True)
        b = twin.render_buses(T, frames=True, mix=True, stats=True)
        for x, y, what in zip(a, b, ("frames", "mix", "statistics", "bus mixes")):
            assert np.abs(np.nan_to_num(x)).max() > 0, what
            assert (np.ascontiguousarray(x).view(np.uint8) == np.ascontiguousarray(y).view(np.uint8)).all(), f"{what}, render {k}"
        bm = a[3]
        c = cv[:, k * T:(k + 1) * T]
        ref, ref_state = R.bus_filter(bm, c, params, port, np.ones(n_buses), ref_state)
        assert_audible(bm, c, params, port, np.ones(n_buses), ref, f"render {k}")
        assert_same_bits(p.bus_filter(bm, c), ref, f"the filters on render {k}'s bus mixes")   # (render 1: across the edit below)
        assert_same_bits(p.bus_filter_state(), ref_state, f"state behind render {k}")
        assert_same_bits(p.send(bm), twin.send(bm), "sends")
        assert_same_bits(p.bus_reverb(bm), twin.bus_reverb(bm), "reverbs")
        ma, mb = p.master(bm, stats=np.zeros((2, S.STAT_COUNT))), twin.master(bm, stats=np.zeros((2, S.STAT_COUNT)))
        assert_same_bits(ma[0], mb[0], "master")
        assert (ma[1] == mb[1]).all(), "master statistics"
        for field in (S.VCF_ST_B4, S.VCF_ST_B1):
            assert (p.get_voice_field(p.ids["vcf"], field) == twin.get_voice_field(twin.ids["vcf"], field)).all(), "voice state"
        ia, ib = p.info(), twin.info()
        token = f" busvcf={n_buses}[1 waves]"
        assert ia.count(token) == 1 and "busvcf" not in ib
        assert ia.replace(token, "") == ib, "info() apart from the token"
        assert ia.split("kernel=")[1] == ib.split("kernel=")[1]
        assert ia.index(" sends=") < ia.index(token) < ia.index(" busfx=")
        if k == 0:   # an edit that re-flattens the patch: the filters and their state stay
            for h in (p, twin):
                h.set_field(h.ids["vcf"], S.VCF_RES, 0.3)
    n, a, o, e = p.get_bus_filter()
    assert n == n_buses and (a == params).all() and (o == port).all() and (e == 1).all()
    # another n_buses drops them, state included; so does srack_voices_configure
    p.set_buses(n_buses + 1, np.arange(V, dtype=np.intc) % (n_buses + 1))
    assert p.get_bus_filter()[0] == 0 and "busvcf" not in p.info()
    p.set_bus_filter()
    assert (p.bus_filter_state() == 0).all()


# ---- 9. run to run -------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(S):
    n_buses, T = 130, 333
    rows, cv, params, port, enabled = case(n_buses, 2, T, 99)
    outs, states = [], []
    for _ in range(2):
        p = host(S, n_buses)
        p.set_bus_filter(params, port, enabled)
        outs.append(p.bus_filter(rows, cv))
        states.append(p.bus_filter_state())
    assert (outs[0].view(np.uint32) == outs[1].view(np.uint32)).all() and (states[0].view(np.uint32) == states[1].view(np.uint32)).all()
    ref, ref_state = R.bus_filter(rows, cv, params, port, enabled)
    assert_audible(rows, cv, params, port, enabled, ref, "two runs")
    assert_same_bits(outs[0], ref, "output")
    assert_same_bits(states[0], ref_state, "state")
