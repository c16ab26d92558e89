"""The bus VCAs on the device (srack_buses_vca, csrc/busvca.hip.h): an ADSR per gated bus on the first wave of a workgroup of eight, a tile of
64 buses x 64 control samples turned through LDS, the VCAs streamed by all eight waves.

Rows are seeded f32 values fed straight into srack_buses_vca.  The reference is tests/busvca_ref.py, ADSRModule and VCAModule stated in
NumPy f32, which tests/test_bus_vca_host.py holds to the oracle bit for bit.  The criterion is BIT EQUALITY (NaN matching NaN) —
derived, not measured: both sides perform the same single-rounded IEEE f32 operations in the same order (the library is built with
-ffp-contract=off).  No tolerance anywhere in this file.  Every comparison stands behind a guard that the reference is worth comparing
with: finite where it is meant to be, not silent, not its input, and different between `negative` on and off."""
import ctypes as C
import functools

import numpy as np
import pytest

import srack_pkg
from tests import busvca_ref as R
from tests import busvcf_ref as RF

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-54321.5)  # what d_out and d_env hold before a call, wherever the call must not write
GUARD = np.float32(12345.0)      # one float behind d_out and behind d_env
RUNS = (1, 2, 3, 5, 17, 40, 200)
SEED = 7                         # the seed of the big case: chosen so that the reference alone satisfies test_the_gates_visit_everything
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


def gate_row(rng, n):
    """runs of high values in (0, 2] and low values in [-1, 0] — both zeros among them —, run lengths from RUNS"""
    row, at, high = np.empty(n, dtype=np.float32), 0, bool(rng.integers(0, 2))
    while at < n:
        k = int(rng.choice(RUNS))
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
def _case(n_buses, rc, n, seed):
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-2.0, 2.0, (n_buses, rc, n)).astype(np.float32)
    mode = rng.integers(0, 3, n_buses).astype(np.intc)
    mode[0] = R.GATE
    if n_buses > 2:
        mode[1], mode[2] = R.CV, R.OFF
    negative = (rng.random(n_buses) < 0.5).astype(np.intc)
    # sliders in [0, 0.02] s, most of them short against the gates' runs; a_sec = 0, r_sec = 0 and a negative s_val among them
    params = np.stack([0.02 * rng.random(n_buses) ** 4, 0.02 * rng.random(n_buses) ** 4, rng.uniform(-0.5, 1.0, n_buses), 0.02 * rng.random(n_buses) ** 4],
                      axis=1).astype(np.float32)
    params[rng.random(n_buses) < 0.15, 0] = 0.0
    params[rng.random(n_buses) < 0.15, 3] = 0.0
    ctl = np.empty((n_buses, n), dtype=np.float32)
    for b in range(n_buses):
        ctl[b] = gate_row(rng, n) if mode[b] == R.GATE else rng.uniform(-1.0, 1.0, n)   # (an OFF bus's row is never read)
    gated = np.flatnonzero(mode == R.GATE)
    if len(gated) > 3 and n > 300:
        b = gated[1]                       # a stretch of NaN gate: neither high nor low
        ctl[b, 100:140] = np.nan
        b = gated[2]                       # the gate is low on the sample Decay ends and high on the next: a retrigger inside Sustain
        params[b], negative[b] = (0.0, 0.001, 0.5, 0.004), 0
        ctl[b] = 1.0
        _, _, track = R.envelope(ctl[b:b + 1], params[b:b + 1], 48000)
        ends = int(np.flatnonzero(track[0] == R.SUSTAIN)[0])
        ctl[b, ends], ctl[b, ends + 1:ends + 30], ctl[b, ends + 30:] = -0.0, 1.5, gate_row(rng, n - ends - 30)
    for a in (rows, ctl, params, mode, negative):
        a.setflags(write=False)
    return rows, ctl, params, mode, negative


def case(n_buses, rc, n, seed):
    """-> (rows [n_buses][rc][n], ctl [n_buses][n], params [n_buses][4], mode [n_buses], negative [n_buses]): read-only, shared"""
    return _case(n_buses, rc, n, seed)


@functools.lru_cache(maxsize=None)
def reference(n_buses, rc, n, seed, with_ctl=True, rate=48000):
    rows, ctl, params, mode, negative = case(n_buses, rc, n, seed)
    out = R.bus_vca(rows, ctl if with_ctl else None, params, mode, negative, rate)
    for a in out:
        a.setflags(write=False)
    return out


def assert_worth_comparing(rows, ctl, params, mode, negative, rate, ref_out, what="", state=None):
    """finite, not silent, not its input, and `negative` the other way round gives other samples"""
    on = np.flatnonzero(np.asarray(mode) != R.OFF)
    if len(on) == 0:
        return
    used = min(rows.shape[1], 2)
    y, x = ref_out[on, :used], rows[on, :used]
    assert np.isfinite(y).all(), f"{what}: the reference is not finite"
    if y.size < 64:
        return  # (a handful of samples may well all be closed)
    assert np.count_nonzero(y) >= y.size // 8, f"{what}: the reference is (nearly) silent"
    assert np.count_nonzero(y != x) >= y.size // 4, f"{what}: the reference is its input"
    if (np.asarray(mode) == R.CV).any() and ctl is not None:   # (an envelope that stays positive opens the VCA either way)
        other = R.bus_vca(rows, ctl, params, mode, 1 - np.asarray(negative), rate, state)[0]
        assert np.count_nonzero(other[on, :used] != y) >= y.size // 16, f"{what}: negative on and off do not differ"


def run_raw(S, p, rows, ctl=None, in_place=False, want_env=False, off_rows=0, off_ctl=0, off_out=0, off_env=0):
    """srack_buses_vca with its four pointers `off_*` floats into their allocations.  Out of place d_out holds SENTINEL beforehand, and so
    does d_env; one GUARD float lies behind each.  -> (out of rows' shape, env [n_buses][n] or None, the guards as they came back)"""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    buf = np.full(x.size + 1, SENTINEL, dtype=np.float32)
    if in_place:
        buf[:-1] = x.ravel()
    buf[-1] = GUARD
    ebuf = np.full(x.shape[0] * x.shape[2] + 1, SENTINEL, dtype=np.float32)
    ebuf[-1] = GUARD
    c = None
    if ctl is not None:
        c = np.ascontiguousarray(ctl, dtype=np.float32)
        assert c.shape == (x.shape[0], x.shape[2])
    with S.DeviceScope() as dev:
        a_out = dev.upload(buf, off_out)
        a_in = a_out if in_place else dev.upload(x, off_rows)
        a_ctl = None if c is None else dev.upload(c, off_ctl)
        a_env = dev.upload(ebuf, off_env) if want_env else None
        p.bus_vca_raw(x.shape[2], a_in, x.shape[1], a_ctl, a_out, a_env, None)
        dev.download(buf, a_out)
        if want_env:
            dev.download(ebuf, a_env)
    return buf[:-1].reshape(x.shape), (ebuf[:-1].reshape(x.shape[0], x.shape[2]) if want_env else None), (buf[-1], ebuf[-1])


# ---- 1. shapes: partial and full groups of buses, partial and full tiles, row_channels 1, 2, 3 ------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 777])
@pytest.mark.parametrize("n_buses", [1, 3, 64, 65, 130])
def test_shapes(S, n_buses, n):
    """1 / 3 / 64 / 65 / 130 buses: a partial workgroup, a full one, two with the second nearly empty, three; 1 / 63 / 64 / 65 / 777 samples:
    partial tiles, a full one, tiles with a tail.  row_channels goes round 1, 2, 3 over the grid; out of place and in place."""
    rc = 1 + (n_buses + n) % 3
    rows, ctl, params, mode, negative = case(n_buses, rc, n, SEED)
    ref, ref_env, ref_state, _ = reference(n_buses, rc, n, SEED)
    assert_worth_comparing(rows, ctl, params, mode, negative, 48000, ref, "reference")
    used = min(rc, 2)
    p = host(S, n_buses)
    p.set_bus_vca(params, mode, negative)
    got, env, guards = run_raw(S, p, rows, ctl, want_env=True)
    assert_same_bits(got[:, :used], ref[:, :used], "output")
    assert (got[:, used:] == SENTINEL).all() and guards == (GUARD, GUARD), "a channel beyond the second, or a float behind a buffer, was written"
    assert_same_bits(env, ref_env, "d_env")
    assert_same_bits(p.bus_vca_state(), ref_state, "state")
    assert f" busvca={int((mode != R.OFF).sum())}[{int((mode == R.GATE).sum())} gated]" in p.info()
    q = host(S, n_buses)
    q.set_bus_vca(params, mode, negative)
    inp, _, guards = run_raw(S, q, rows, ctl, in_place=True)
    assert_same_bits(inp[:, :used], ref[:, :used], "in place")
    assert_same_bits(inp[:, used:], rows[:, used:], "channels beyond the second, in place")
    assert guards[0] == GUARD


# ---- 2. a per-bus mix of modes and flags; special values stay in their bus ---------------------------------------------------------------
def test_per_bus_mix_and_special_values(S):
    rows, ctl, params, mode, negative = case(NB, 2, T, SEED)
    assert all(np.count_nonzero(mode == m) >= 20 for m in (R.OFF, R.CV, R.GATE)) and 30 < negative.sum() < 100
    gated = mode == R.GATE
    assert (params[gated, 0] == 0).any() and (params[gated, 3] == 0).any() and (params[gated, 2] < 0).any() and params[:, [0, 1, 3]].max() <= 0.02
    base_ref, _, _, _ = reference(NB, 2, T, SEED)
    assert_worth_comparing(rows, ctl, params, mode, negative, 48000, base_ref, "without the specials")
    p = host(S, NB)
    p.set_bus_vca(params, mode, negative)
    base = p.bus_vca(rows, ctl)
    assert_same_bits(base, base_ref, "without the specials")
    b, c = np.flatnonzero(gated)[5], np.flatnonzero(mode == R.CV)[3]
    rows2, ctl2, params2 = rows.copy(), ctl.copy(), params.copy()
    params2[b, 2] = np.nan       # a NaN s_val ...
    rows2[b, 1, 70] = np.inf     # ... and an infinite sample on one bus
    ctl2[c, 200] = np.inf        # an infinite CV on another
    ref, ref_env, ref_state, _ = R.bus_vca(rows2, ctl2, params2, mode, negative, 48000)
    q = host(S, NB)
    q.set_bus_vca(params2, mode, negative)
    got, env = q.bus_vca(rows2, ctl2, want_env=True)
    assert_same_bits(got, ref, "with the specials")
    assert_same_bits(env, ref_env, "d_env with the specials")
    assert_same_bits(q.bus_vca_state(), ref_state, "state with the specials")
    rest = np.setdiff1d(np.arange(NB), [b, c])
    assert_same_bits(got[rest], base[rest], "the buses the specials did not touch")
    assert np.isfinite(ref[rest]).all() and np.isnan(ref[b]).any() and not np.isfinite(ref[c]).all()


# ---- 3. the gate rows reach every mode and every way out of it ---------------------------------------------------------------------------
def test_the_gates_visit_everything(S):
    rows, ctl, params, mode, negative = case(NB, 2, T, SEED)
    ref, ref_env, ref_state, track = reference(NB, 2, T, SEED)
    gated = np.flatnonzero(mode == R.GATE)
    g, tr = ctl[gated], track[gated]
    assert np.isnan(g).any() and (g.view(np.uint32) == 0x80000000).any() and (g.view(np.uint32) == 0).any() and np.nanmax(g) <= 2 and np.nanmin(g) >= -1
    held = [np.count_nonzero(tr == m) / tr.size for m in range(5)]
    assert min(held) >= 0.01, held
    hits = R.retriggers(tr, g)
    assert all(hits[m] >= 1 for m in (R.ATTACK, R.DECAY, R.SUSTAIN, R.RELEASE)), hits
    assert len(np.unique(ref_state[gated, 1])) >= 3, "the envelopes are meant to end in several modes"
    p = host(S, NB)
    p.set_bus_vca(params, mode, negative)
    got, env = p.bus_vca(rows, ctl, want_env=True)
    assert_same_bits(env, ref_env, "envelopes")
    assert_same_bits(got, ref, "output")
    assert_same_bits(p.bus_vca_state(), ref_state, "state")


# ---- 4. d_ctl = NULL -------------------------------------------------------------------------------------------------------------------------
def test_without_a_control_row(S):
    n_buses, n = 70, 200
    rows, ctl, params, mode, negative = case(n_buses, 2, n, 41)
    params, mode = params.copy(), mode.copy()
    params[:4], mode[:4] = (0.0005, 0.0005, 0.5, 0.002), R.GATE
    p = host(S, n_buses)
    p.set_bus_vca(params, mode, negative)
    ref, ref_env, ref_state, _ = R.bus_vca(rows, None, params, mode, negative, 48000)
    got, env, _ = run_raw(S, p, rows, None, want_env=True)
    on = mode != R.OFF
    assert (got[on] == 0).all() and (env.view(np.uint32) == 0).all(), "fresh GATE buses give zeros (audio * 0.0 through an open VCA: of either sign)"
    assert (got[mode == R.CV].view(np.uint32) == 0).all() and negative[mode == R.CV].any(), "CV buses give +0.0 words, whatever `negative` says"
    assert (got[mode == R.GATE].view(np.uint32) == 0x80000000).any(), "... and the gated buses' zeros are the products' own"
    assert_same_bits(got, ref, "no control row, fresh")
    assert_same_bits(got[~on], rows[~on], "OFF buses pass")
    assert_same_bits(p.bus_vca_state(), ref_state, "state: the unconnected gate has cleared `last`")
    assert (ref_state[mode == R.GATE, 5] == 0).all()
    # buses 0..3 carried into Sustain by a call with the gate held high, then a call without a control row: they release
    p.reset_bus_vca()
    held = ctl.copy()
    held[:4] = 1.0
    ref1, _, st1, _ = R.bus_vca(rows, held, params, mode, negative, 48000)
    assert (st1[:4, 1] == R.SUSTAIN).all()
    assert_same_bits(p.bus_vca(rows, held), ref1, "the gate held high")
    ref2, env2, st2, tr2 = R.bus_vca(rows, None, params, mode, negative, 48000, st1)
    assert (tr2[:4, 0] == R.RELEASE).all() and (tr2[:4, -1] == R.NONE).all() and np.count_nonzero(ref2[:4]) > 100
    got2, genv2 = p.bus_vca(rows, want_env=True)
    assert_same_bits(got2, ref2, "the release without a gate")
    assert_same_bits(genv2, env2, "its envelope")
    assert_same_bits(p.bus_vca_state(), st2, "state behind the release")


# ---- 5. in place equals out of place; an OFF bus's words survive ---------------------------------------------------------------------------
@pytest.mark.parametrize("rc,n", [(2, 200), (3, 65), (1, 64)])
def test_in_place_gives_the_out_of_place_bits(S, rc, n):
    n_buses = 75
    rows, ctl, params, mode, negative = case(n_buses, rc, n, 50 + rc)
    rows = rows.copy()
    off = np.flatnonzero(mode == R.OFF)
    words = rows.view(np.uint32)
    words[off[0], 0, :4] = (0x80000000, 0x7FC12345, 0xFFC00001, 0x00000001)   # -0.0, NaNs with payloads, a denormal
    ref, _, ref_state, _ = R.bus_vca(rows, ctl, params, mode, negative, 48000)
    used = min(rc, 2)
    assert_worth_comparing(rows[1:], ctl[1:], params[1:], mode[1:], negative[1:], 48000, ref[1:], "in place")
    p, q = host(S, n_buses), host(S, n_buses)
    p.set_bus_vca(params, mode, negative)
    q.set_bus_vca(params, mode, negative)
    out, _, _ = run_raw(S, p, rows, ctl)
    inp, _, guards = run_raw(S, q, rows, ctl, in_place=True, off_out=1)
    assert (inp[:, :used].view(np.uint32) == out[:, :used].view(np.uint32)).all(), "in place against out of place, as words"
    assert_same_bits(inp[:, :used], ref[:, :used], "in place against the reference")
    assert (inp[off].view(np.uint32) == words[off]).all() and (out[off, :used].view(np.uint32) == words[off, :used]).all(), "an OFF bus's words"
    assert (inp[:, used:].view(np.uint32) == words[:, used:]).all() and (out[:, used:] == SENTINEL).all() and guards[0] == GUARD
    assert_same_bits(q.bus_vca_state(), ref_state, "state")


# ---- 6. d_env ------------------------------------------------------------------------------------------------------------------------------------
def test_the_envelope_rows(S):
    rows, ctl, params, mode, negative = case(NB, 2, 300, 61)
    ctl = ctl.copy()
    cvb = np.flatnonzero(mode == R.CV)
    ctl.view(np.uint32)[cvb[0], :3] = (0x7FC54321, 0x80000000, 0xFF800000)   # a CV bus's words come back word for word
    ref, ref_env, _, _ = R.bus_vca(rows, ctl, params, mode, negative, 48000)
    p, q = host(S, NB), host(S, NB)
    p.set_bus_vca(params, mode, negative)
    q.set_bus_vca(params, mode, negative)
    with_env, env, guards = run_raw(S, p, rows, ctl, want_env=True, off_env=1)
    without, none, _ = run_raw(S, q, rows, ctl)
    assert none is None and (with_env.view(np.uint32) == without.view(np.uint32)).all(), "d_out does not depend on d_env"
    rest = np.setdiff1d(np.arange(NB), [cvb[0]])
    assert_same_bits(with_env[rest], ref[rest], "output")
    assert_same_bits(env, ref_env, "d_env")
    assert (env[mode == R.CV].view(np.uint32) == ctl[mode == R.CV].view(np.uint32)).all(), "a CV bus's control row, word for word"
    assert (env[mode == R.OFF].view(np.uint32) == 0).all(), "an OFF bus's +0.0"
    gated = mode == R.GATE
    assert np.count_nonzero(env[gated] != ctl[gated]) > env[gated].size // 2 and len(np.unique(env[gated])) > 1000 and guards == (GUARD, GUARD)


# ---- 7. cuts ---------------------------------------------------------------------------------------------------------------------------------------
def test_cuts_give_the_same_bits(S):
    cuts = (1, 63, 64, 300, 349)
    assert sum(cuts) == T
    rows, ctl, params, mode, negative = case(NB, 2, T, SEED)
    ref, ref_env, ref_state, _ = reference(NB, 2, T, SEED)
    one = host(S, NB)
    one.set_bus_vca(params, mode, negative)
    whole, whole_env = one.bus_vca(rows, ctl, want_env=True)
    assert_same_bits(whole, ref, "one call")
    p = host(S, NB)
    p.set_bus_vca(params, mode, negative)
    parts, envs, at = [], [], 0
    for k in cuts:
        o, e = p.bus_vca(rows[:, :, at:at + k], ctl[:, at:at + k], want_env=True)
        parts.append(o)
        envs.append(e)
        at += k
    assert (np.concatenate(parts, axis=2).view(np.uint32) == whole.view(np.uint32)).all(), "calls of 1, 63, 64, 300, 349"
    assert (np.concatenate(envs, axis=1).view(np.uint32) == whole_env.view(np.uint32)).all()
    assert (p.bus_vca_state().view(np.uint32) == one.bus_vca_state().view(np.uint32)).all(), "state, cut and uncut"
    assert_same_bits(p.bus_vca_state(), ref_state, "state")
    assert not R.same_bits(ref_state[mode == R.GATE], R.fresh(1, 48000)).all(axis=1).all()


# ---- 8. lifecycle ------------------------------------------------------------------------------------------------------------------------------------
def test_slider_modes_and_reset(S):
    n_buses, n = 66, 150
    rows, ctl, params, mode, negative = case(n_buses, 2, 2 * n, 77)
    first, second = (rows[:, :, :n], ctl[:, :n]), (rows[:, :, n:], ctl[:, n:])
    p = host(S, n_buses)
    p.set_bus_vca(params, mode, negative)
    ref1, _, st1, _ = R.bus_vca(*first, params, mode, negative, 48000)
    assert_worth_comparing(*first, params, mode, negative, 48000, ref1, "first call")
    assert_same_bits(p.bus_vca(*first), ref1, "first call")
    assert_same_bits(p.bus_vca_state(), st1, "state after the first call")
    gated = np.flatnonzero(mode == R.GATE)
    moved = gated[~R.same_bits(st1[gated], R.fresh(1, 48000)).all(axis=1)]
    assert len(moved) > 5
    # set_vca again is the slider: sliders and flags change, state stays
    params2 = params.copy()
    params2[:, [0, 1, 3]] = np.float32(0.02) - params[:, [0, 1, 3]]
    negative2 = 1 - negative
    p.set_bus_vca(params2, mode, negative2)
    assert_same_bits(p.bus_vca_state(), st1, "state behind set_vca: nothing run, nothing lost")
    ref2, _, st2, _ = R.bus_vca(*second, params2, mode, negative2, 48000, st1)
    assert not R.same_bits(ref2, R.bus_vca(*second, params2, mode, negative2, 48000)[0]).all(), "the carried state is meant to show"
    assert_same_bits(p.bus_vca(*second), ref2, "second call: sliders moved, state carried")
    assert_same_bits(p.bus_vca_state(), st2, "state after the second call")
    # GATE -> CV -> GATE starts fresh; the neighbours keep their state
    b = next(x for x in gated if not R.same_bits(st2[x], R.fresh(1, 48000)[0]).all())
    mode_cv = mode.copy()
    mode_cv[b] = R.CV
    p.set_bus_vca(params2, mode_cv, negative2)
    dropped = st2.copy()
    dropped[b] = R.fresh(1, 48000)[0]
    assert_same_bits(p.bus_vca_state(), dropped, "a bus that leaves GATE drops its state")
    p.set_bus_vca(params2, mode, negative2)
    assert_same_bits(p.bus_vca_state(), dropped, "... and starts fresh when it comes back")
    ref3, _, st3, _ = R.bus_vca(*first, params2, mode, negative2, 48000, dropped)
    assert_same_bits(p.bus_vca(*first), ref3, "third call")
    assert_same_bits(p.bus_vca_state(), st3, "state after the third call")
    # reset_vca: every state fresh, the setting stays
    p.reset_bus_vca()
    assert p.bus_vca_state().tolist() == [[0.0, 4.0, 0.0, 0.0, 48000.0, 1.0]] * n_buses
    k, a, m, g = p.get_bus_vca()
    assert k == n_buses and (a == params2).all() and (m == mode).all() and (g == negative2).all()
    ref4, _, st4, _ = R.bus_vca(*second, params2, mode, negative2, 48000)
    assert_same_bits(p.bus_vca(*second), ref4, "behind a reset")
    assert_same_bits(p.bus_vca_state(), st4, "state behind a reset")
    # the same n_buses keeps the VCAs and their state, another drops them
    p.set_buses(n_buses, np.zeros(1, dtype=np.intc))
    assert_same_bits(p.bus_vca_state(), st4, "another table of the same n_buses")
    p.set_buses(n_buses + 1, np.zeros(1, dtype=np.intc))
    assert p.get_bus_vca()[0] == 0 and "busvca" not in p.info()
    p.set_bus_vca()
    assert p.bus_vca_state().tolist() == [[0.0, 4.0, 0.0, 0.0, 48000.0, 1.0]] * (n_buses + 1)


def test_not_part_of_the_program(S):
    """the VCAs change nothing a render, the filters, the reverbs or the master write, survive an edit that re-flattens, and a twin handle
    that never heard of them says the same about itself once the ` busvca=` token is taken out"""
    V, n_buses, n = 64, 4, 300

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
        p.set_bus_filter()
        return p

    p, twin = make(), make()
    params = np.array([[0.001, 0.002, 0.5, 0.003], [0.0, 0.001, 0.7, 0.001], R.DEFAULTS, [0.002, 0.002, -0.5, 0.0]], dtype=np.float32)
    mode, negative = np.array([2, 2, 1, 2], dtype=np.intc), np.array([0, 1, 1, 0], dtype=np.intc)
    p.set_bus_vca(params, mode, negative)
    rng = np.random.default_rng(8)
    ctl = np.stack([gate_row(rng, 2 * n), gate_row(rng, 2 * n), rng.uniform(-1, 1, 2 * n).astype(np.float32), gate_row(rng, 2 * n)])
    ref_state = None
    for k in range(2):
        a = p.render_buses(n, frames=True, mix=True, stats=True)
        b = twin.render_buses(n, frames=True, mix=True, stats=True)
        for x, y, what in zip(a, b, ("frames", "mix", "statistics", "bus mixes")):
            assert np.abs(np.nan_to_num(x)).max() > 0, what
            assert (np.ascontiguousarray(x).view(np.uint8) == np.ascontiguousarray(y).view(np.uint8)).all(), f"{what}, render {k}"
        bm = a[3]
        c = ctl[:, k * n:(k + 1) * n]
        ref, _, ref_state, _ = R.bus_vca(bm, c, params, mode, negative, 48000, ref_state)
        assert np.isfinite(ref).all() and np.count_nonzero(ref) > ref.size // 8 and np.count_nonzero(ref != bm) > ref.size // 4
        assert_same_bits(p.bus_vca(bm, c), ref, f"the VCAs on render {k}'s bus mixes")   # (render 1: across the edit below)
        assert_same_bits(p.bus_vca_state(), ref_state, f"state behind render {k}")
        assert_same_bits(p.bus_filter(bm), twin.bus_filter(bm), "filters")
        assert_same_bits(p.send(bm), twin.send(bm), "sends")
        assert_same_bits(p.bus_reverb(bm), twin.bus_reverb(bm), "reverbs")
        ma, mb = p.master(bm, stats=np.zeros((2, S.STAT_COUNT))), twin.master(bm, stats=np.zeros((2, S.STAT_COUNT)))
        assert_same_bits(ma[0], mb[0], "master")
        assert (ma[1] == mb[1]).all(), "master statistics"
        ia, ib = p.info(), twin.info()
        token = " busvca=4[3 gated]"
        assert ia.count(token) == 1 and "busvca" not in ib
        assert ia.replace(token, "") == ib, "info() apart from the token"
        assert ia.split("kernel=")[1] == ib.split("kernel=")[1]
        assert ia.index(" busvcf=") < ia.index(token) < ia.index(" busfx=")
        if k == 0:   # an edit that re-flattens the patch: the VCAs and their state stay
            for h in (p, twin):
                h.set_field(h.ids["vcf"], S.VCF_RES, 0.3)
    k, a, m, g = p.get_bus_vca()
    assert k == n_buses and (a == params).all() and (m == mode).all() and (g == negative).all()


# ---- 9. pointers -------------------------------------------------------------------------------------------------------------------------------------
def test_overlaps_are_refused(S):
    n_buses, n = 3, 16
    p = host(S, n_buses)
    p.set_bus_vca()
    nbytes, rowbytes = n_buses * 2 * n * 4, n_buses * n * 4
    with S.DeviceScope() as dev:
        d = dev.alloc(8 * nbytes)
        base, far, farther = d + nbytes, d + 4 * nbytes, d + 6 * nbytes
        run = S.lib.srack_buses_vca
        for d_out in (base + 4, base - 4, base + nbytes - 4, base - nbytes + 4):
            assert run(p.h, n, base, 2, None, d_out, None, None) == S.ERR_INVALID, d_out - base
        for d_x in (base, base + nbytes - 4, base - rowbytes + 4):
            assert run(p.h, n, base, 2, d_x, base, None, None) == S.ERR_INVALID, d_x - base        # d_ctl on d_out, in place
            assert run(p.h, n, far, 2, d_x, base, None, None) == S.ERR_INVALID, d_x - base         # ... out of place
            assert run(p.h, n, base, 2, None, base, d_x, None) == S.ERR_INVALID, d_x - base        # d_env on d_out, in place
            assert run(p.h, n, far, 2, None, base, d_x, None) == S.ERR_INVALID, d_x - base         # ... out of place
            assert run(p.h, n, base, 2, None, far, d_x, None) == S.ERR_INVALID, d_x - base         # d_env on d_rows
        for d_env in (farther, farther + rowbytes - 4, farther - rowbytes + 4):
            assert run(p.h, n, base, 2, farther, far, d_env, None) == S.ERR_INVALID                   # d_env on d_ctl
        assert "busvca" not in p.info() and p.bus_vca_state().tolist() == [[0.0, 4.0, 0.0, 0.0, 48000.0, 1.0]] * n_buses   # nothing ran
        # neighbours are fine: d_out right behind d_rows, d_ctl right behind d_out, d_env right behind d_ctl; d_ctl may lie on d_rows
        assert S.lib.srack_device_from_host(d, np.zeros(2 * nbytes, dtype=np.float32).ctypes.data_as(C.c_void_p), 8 * nbytes, None) == 0
        assert run(p.h, n, d, 2, d + 2 * nbytes, d + nbytes, d + 2 * nbytes + rowbytes, None) == S.OK
        assert run(p.h, n, d, 2, d, d + nbytes, None, None) == S.OK


@pytest.mark.parametrize("off_rows,off_ctl,off_out,off_env", [(1, 2, 3, 1), (2, 3, 1, 3), (3, 1, 2, 2), (1, 0, 0, 0), (0, 0, 0, 1)])
def test_bases_offset_by_floats(S, off_rows, off_ctl, off_out, off_env):
    n_buses, n = 67, 131
    rows, ctl, params, mode, negative = case(n_buses, 2, n, 44)
    ref, ref_env, _, _ = reference(n_buses, 2, n, 44)
    assert_worth_comparing(rows, ctl, params, mode, negative, 48000, ref, "offsets")
    p = host(S, n_buses)
    p.set_bus_vca(params, mode, negative)
    got, env, guards = run_raw(S, p, rows, ctl, want_env=True, off_rows=off_rows, off_ctl=off_ctl, off_out=off_out, off_env=off_env)
    assert_same_bits(got, ref, f"offsets {off_rows}, {off_ctl}, {off_out}, {off_env}")
    assert_same_bits(env, ref_env, "d_env")
    assert guards == (GUARD, GUARD)


# ---- 10. a 44 100 Hz patch -------------------------------------------------------------------------------------------------------------------------
def test_the_rate_is_the_patchs(S):
    n_buses, n = 40, 300
    rows, ctl, params, mode, negative = case(n_buses, 2, n, 91)
    ref, ref_env, ref_state, _ = R.bus_vca(rows, ctl, params, mode, negative, 44100)
    at48, env48, _, _ = reference(n_buses, 2, n, 91)
    assert_worth_comparing(rows, ctl, params, mode, negative, 44100, ref, "44.1 kHz")
    assert np.count_nonzero(~R.same_bits(ref_env, env48)) > n_buses * n // 20, "the rate is meant to show"
    p = host(S, n_buses, rate=44100)
    p.set_bus_vca(params, mode, negative)
    got, env = p.bus_vca(rows, ctl, want_env=True)
    assert_same_bits(env, ref_env, "envelopes at 44.1 kHz")
    assert_same_bits(got, ref, "output at 44.1 kHz")
    assert_same_bits(p.bus_vca_state(), ref_state, "state: the rate slot holds 44100")
    assert (p.bus_vca_state()[:, 4] == np.float32(44100)).all()


# ---- 11. the intended chain: the same gate opens the VCA and sweeps the bus filter ------------------------------------------------------------
def test_the_envelope_drives_the_bus_filter(S):
    n_buses, n = 20, 400
    rows, ctl, params, _, negative = case(n_buses, 2, n, 17)
    mode = np.full(n_buses, R.GATE, dtype=np.intc)
    ref, ref_env, _, _ = R.bus_vca(rows, ctl, params, mode, negative, 48000)
    assert_worth_comparing(rows, ctl, params, mode, negative, 48000, ref, "the VCAs")
    fpar = np.tile(np.array([0.1, 0.6, 0.7], dtype=np.float32), (n_buses, 1))
    port, enabled = np.zeros(n_buses, dtype=np.intc), np.ones(n_buses, dtype=np.intc)
    want, _ = RF.bus_filter(ref, ref_env, fpar, port, enabled)
    flat, _ = RF.bus_filter(ref, None, fpar, port, enabled)
    assert np.isfinite(want).all() and np.count_nonzero(want != flat) > want.size // 4, "the sweep is meant to show"
    p = host(S, n_buses)
    p.set_bus_vca(params, mode, negative)
    p.set_bus_filter(fpar, port, enabled)
    got = np.empty_like(want)
    with S.DeviceScope() as dev:
        d = [dev.upload(rows), dev.upload(ctl), dev.alloc(ctl.nbytes), dev.alloc(rows.nbytes)]   # rows (processed in place), ctl, env, filtered
        p.bus_vca_raw(n, d[0], 2, d[1], d[0], d[2])
        p.bus_filter_raw(n, d[0], 2, d[2], d[3])
        dev.download(got, d[3])
    assert_same_bits(got, want, "VCA, then the filter swept by the VCA's envelope")
