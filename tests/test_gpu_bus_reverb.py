"""Bus reverbs on the device (srack_buses_reverb, csrc/busfx.hip.h): a stereo Freeverb per mix bus, a workgroup per bus, time-parallel
over blocks of min(256, shortest line) samples.

Inputs are seeded f32 noise bursts with silence between them (the tails are what a reverb is about), fed straight into
srack_buses_reverb; the reference is oracle.srack_numpy._Freeverb ticked in Python on the same f32 values.  The criterion is BIT
EQUALITY (NaN matching NaN) — derived, not measured: both sides perform the same sequence of single-rounded IEEE f64 operations (the
library is built with -ffp-contract=off), and the f64 -> f32 conversion of the result rounds to nearest even on both.  No tolerance
anywhere in this file.  Every case asserts that what it compares is not silent."""
import numpy as np
import pytest

import srack_pkg
from oracle.srack_numpy import _Freeverb

pytestmark = pytest.mark.gpu

DEFAULTS = (0.5, 0.0, 1.0, 0.5, 0.5, 0.0)
SETTERS = ("set_dampening", "set_freeze", "set_wet", "set_width", "set_room_size", "set_dry")  # the module's field order (freeverb.rs:88-114)
# distinct rooms: long and wide with some dry, frozen, width 0 with dry 1, small and damped
ROOMS = [(1.7, 0.0, 0.6, 1.0, 0.9, 0.8), (0.5, 1.0, 1.0, 0.5, 0.3, 0.25), (0.3, 0.0, 0.7, 0.0, 0.6, 1.0), (2.0, 0.0, 0.45, 0.8, 0.1, 0.0)]


@pytest.fixture(scope="module")
def S():
    return srack_pkg.load()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_bits(got, ref, what=""):
    got, ref = np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    ok = (bits(got) == bits(ref)) | (np.isnan(got) & np.isnan(ref))
    if not ok.all():
        at = np.argwhere(~ok)
        first = tuple(at[0])
        raise AssertionError(f"{what}: {len(at)} of {ok.size} samples differ, first at {first}: got {got[first]!r} ({bits(got)[first]:#010x}), "
                             f"reference {ref[first]!r} ({bits(ref)[first]:#010x})")


def assert_audible(x, what=""):
    x = np.asarray(x)
    x = np.where(np.isfinite(x), x, 0)
    assert np.abs(x).max() > 1e-3 and np.count_nonzero(x) > x.size // 4, f"{what}: (nearly) silent — the comparison would show nothing"


def bursts(rng, rows, T):
    """f32 [rows][T]: bursts of uniform noise, silence between them (the last stretch is silence: a tail to the end)"""
    x = np.zeros((rows, T), dtype=np.float32)
    for r in range(rows):
        pos = int(rng.integers(0, max(1, T // 20)))
        while pos < T * 3 // 4:
            on, off = int(rng.integers(3, max(4, T // 12))), int(rng.integers(T // 30 + 1, T // 5 + 2))
            x[r, pos:pos + on] = rng.uniform(-1.0, 1.0, min(on, T - pos)).astype(np.float32)
            pos += on + off
    return x


def new_reverb(sr, params):
    """FreeverbModule's first calc(): Freeverb::new, then set_freeverb(true) — every setter once, in field order"""
    fv = _Freeverb(sr)
    for name, v in zip(SETTERS, params):
        getattr(fv, name)(bool(v != 0.0) if name == "set_freeze" else float(v))
    return fv


def change(fv, old, new):
    """the slider, set_freeverb(false): only the setters of the fields that changed run"""
    for name, a, b in zip(SETTERS, old, new):
        if a != b:
            getattr(fv, name)(bool(b != 0.0) if name == "set_freeze" else float(b))


def tick(fv, x):
    """x f32 [channels][T] (channels >= 1; the second is the Right input, one channel = Right unconnected) -> f32 [2][T]"""
    l = x[0].astype(np.float64).tolist()
    r = x[1].astype(np.float64).tolist() if x.shape[0] > 1 else [0.0] * len(l)
    out = np.array([fv.tick(a, b) for a, b in zip(l, r)], dtype=np.float64).reshape(-1, 2)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(out.T.astype(np.float32))


def copy_of(x):
    """what a bus without a reverb gives: channels 0 and 1 of the bus mix (zeros for a patch of one channel)"""
    return np.stack([x[0], x[1] if x.shape[0] > 1 else np.zeros_like(x[0])])


def host(S, sr, channels, n_buses):
    """a handle to hang the reverbs on: an oscillator into every channel, one voice in bus 0 of n_buses (never rendered here)"""
    p = S.Patch(sr, 64, channels)
    osc, out = p.add_module(S.MOD_OSCILLATOR), p.add_module(S.MOD_OUTPUT)
    for c in range(channels):
        p.connect(osc, S.OSC_OUT_SINE, out, c)
    p.configure_voices(1)
    p.set_buses(n_buses)
    return p


def run(p, x, cuts=None):
    """x f32 [n_buses][channels][T] through srack_buses_reverb, in calls of `cuts` samples (None: one call)"""
    T = x.shape[2]
    cuts = [T] if cuts is None else cuts
    assert sum(cuts) == T
    out, at = [], 0
    for n in cuts:
        out.append(p.bus_reverb(x[:, :, at:at + n]))
        at += n
    return np.concatenate(out, axis=2)


_PARITY = {}


def parity_case(S):
    """case 1, computed once: 2000 Hz (lines of 10 .. 74 slots: every line wraps eight times or more), five buses"""
    if not _PARITY:
        rng = np.random.default_rng(1401)
        sr, T = 2000, 600
        x = bursts(rng, 10, T).reshape(5, 2, T)
        x[4] = 0.0
        params = np.array([ROOMS[0], ROOMS[1], ROOMS[2], DEFAULTS, DEFAULTS])
        enabled = [1, 1, 1, 0, 1]
        ref = np.stack([tick(new_reverb(sr, params[b]), x[b]) if enabled[b] else copy_of(x[b]) for b in range(5)])
        _PARITY.update(sr=sr, T=T, x=x, params=params, enabled=enabled, ref=ref)
    return _PARITY


def test_parity_with_the_oracle(S):
    c = parity_case(S)
    p = host(S, c["sr"], 2, 5)
    p.set_bus_reverbs(c["params"], c["enabled"])
    ln, block = p.bus_reverb_plan()
    assert ln.min() == 10 and ln.max() == 74 and block == 10
    fx = run(p, c["x"])
    for b in range(5):
        assert_same_bits(fx[b], c["ref"][b], f"bus {b}")
    assert_same_bits(fx[3], c["x"][3], "the disabled bus is the copy")
    assert not fx[4].any()  # silence in, silence out (+0.0)
    assert_audible(fx[:3], "parity")
    assert_audible(fx[:3, :, 450:], "the tails")
    assert " busfx=4[block 10]" in p.info()


@pytest.mark.parametrize("sr,T,n_buses,block", [(784, 300, 1, 4), (48000, 3000, 2, 244), (65535, 2000, 1, 256)])
def test_block_length_extremes(S, sr, T, n_buses, block):
    """784 Hz: blocks of 4 and fewer; 48 kHz: the combs (1214 .. 1785 slots) wrap twice; 65 535 Hz: the cap of 256 lies below the shortest line (334)"""
    rng = np.random.default_rng(sr)
    x = bursts(rng, 2 * n_buses, T).reshape(n_buses, 2, T)
    params = np.array(([ROOMS[0], ROOMS[3]])[:n_buses])
    p = host(S, sr, 2, n_buses)
    p.set_bus_reverbs(params)
    ln, blk = p.bus_reverb_plan()
    assert blk == block == min(256, ln.min())
    fx = run(p, x)
    for b in range(n_buses):
        assert_same_bits(fx[b], tick(new_reverb(sr, params[b]), x[b]), f"{sr} Hz, bus {b}")
    assert_audible(fx, f"{sr} Hz")
    assert f"busfx={n_buses}[block {block}]" in p.info()


@pytest.mark.parametrize("sr,cuts", [(48000, [1, 7, 243, 244, 245, 1, 999]), (2000, [1, 9, 10, 11, 569])])
def test_however_the_samples_are_cut(S, sr, cuts):
    """calls around the block length (244 at 48 kHz, 10 at 2000 Hz) against one call of their sum (1740 and 600 samples)"""
    T = sum(cuts)
    rng = np.random.default_rng(7 + sr)
    x = bursts(rng, 6, T).reshape(3, 2, T)
    params, enabled = np.array([ROOMS[0], ROOMS[1], DEFAULTS]), [1, 1, 0]
    outs = []
    for c in (None, cuts):
        p = host(S, sr, 2, 3)
        p.set_bus_reverbs(params, enabled)
        outs.append(run(p, x, c))
    assert_same_bits(outs[1], outs[0], f"{sr} Hz in calls of {cuts}")
    assert_audible(outs[0][:2], "cutting")
    if sr == 2000:  # (at 48 kHz the one-call run is what test_block_length_extremes holds against the oracle)
        assert_same_bits(outs[0][0], tick(new_reverb(sr, params[0]), x[0]), "one call")


@pytest.mark.parametrize("channels", [1, 3])
def test_channels(S, channels):
    """one channel: the module with Right unconnected (in1 = 0.0); three: the third is ignored"""
    sr, T = 2000, 400
    rng = np.random.default_rng(40 + channels)
    x = bursts(rng, 3 * channels, T).reshape(3, channels, T)
    params, enabled = np.array([ROOMS[2], DEFAULTS, ROOMS[0]]), [1, 0, 1]
    p = host(S, sr, channels, 3)
    p.set_bus_reverbs(params, enabled)
    fx = run(p, x, [150, 250])
    for b in (0, 2):
        assert_same_bits(fx[b], tick(new_reverb(sr, params[b]), x[b, :2]), f"{channels} channels, bus {b}")
    assert_same_bits(fx[1], copy_of(x[1]), "the copy")
    assert_audible(fx, f"{channels} channels")
    if channels == 1:
        assert not fx[1, 1].any()
    else:
        y = x.copy()
        y[:, 2] = rng.uniform(-1, 1, (3, T)).astype(np.float32)
        q = host(S, sr, channels, 3)
        q.set_bus_reverbs(params, enabled)
        assert_same_bits(run(q, y), fx, "another third channel")


def test_edits_between_calls(S):
    """a parameter change is the slider (coefficients change, lines stay); a bus enabled later, or disabled and enabled again, starts
    fresh; reset zeroes; a new table of the same n_buses keeps the tails"""
    sr, n = 2000, 300
    rng = np.random.default_rng(55)
    seg = [bursts(rng, 8, n).reshape(4, 2, n) for _ in range(4)]  # (bursts in every step: each has something to reverberate)
    par = [np.array([ROOMS[0], ROOMS[1], ROOMS[2], ROOMS[3]])]
    par.append(par[0].copy())
    par[1][0] = (0.2, 1.0, 0.6, 0.3, 0.9, 0.1)  # bus 0: dampening, freeze, width and dry move; wet and room size stay
    p = host(S, sr, 2, 4)
    fv = [new_reverb(sr, par[0][b]) for b in range(4)]
    # 1: buses 0, 2, 3 on; 1 off
    p.set_bus_reverbs(par[0], [1, 0, 1, 1])
    fx = run(p, seg[0])
    for b in (0, 2, 3):
        assert_same_bits(fx[b], tick(fv[b], seg[0][b]), f"step 1, bus {b}")
    assert_same_bits(fx[1], seg[0][1], "step 1: bus 1 has no reverb")
    # 2: bus 0's sliders move; bus 1 comes on (a fresh reverb, 300 samples into the session); bus 2 goes off
    p.set_bus_reverbs(par[1], [1, 1, 0, 1])
    change(fv[0], par[0][0], par[1][0])
    fx = run(p, seg[1])
    for b in (0, 1, 3):
        assert_same_bits(fx[b], tick(fv[b], seg[1][b]), f"step 2, bus {b}")
    assert_same_bits(fx[2], seg[1][2], "step 2: bus 2 has no reverb")
    assert_audible(fx, "step 2")
    # 3: a new table of the same n_buses keeps parameters and tails; bus 2 comes back, fresh
    p.set_buses(4, np.array([3], dtype=np.intc), np.array([0.5], dtype=np.float32))
    p.set_bus_reverbs(par[1], [1, 1, 1, 1])
    fv[2] = new_reverb(sr, par[1][2])
    fx = run(p, seg[2], [7, 293])
    for b in range(4):
        assert_same_bits(fx[b], tick(fv[b], seg[2][b]), f"step 3, bus {b}")
    assert_audible(fx[:, :, 200:], "step 3")
    # 4: reset: lines and filter states to zero, the parameters stay
    p.reset_bus_reverbs()
    n_set, a, e = p.get_bus_reverbs()
    assert n_set == 4 and (a == par[1]).all() and e.tolist() == [1, 1, 1, 1]
    fx = run(p, seg[3])
    for b in range(4):
        assert_same_bits(fx[b], tick(new_reverb(sr, par[1][b]), seg[3][b]), f"step 4, bus {b}")
    assert_audible(fx, "step 4")


def test_nonfinite_input_stays_in_its_bus(S):
    sr, T = 2000, 400
    rng = np.random.default_rng(66)
    x = bursts(rng, 6, T).reshape(3, 2, T)
    bad = x.copy()
    bad[1, 0, 50] = np.nan
    bad[1, 1, 120] = np.inf
    params = np.array([ROOMS[0], ROOMS[3], ROOMS[2]])
    outs = []
    for inp in (x, bad):
        p = host(S, sr, 2, 3)
        p.set_bus_reverbs(params)
        outs.append(run(p, inp))
    for b in (0, 2):
        np.testing.assert_array_equal(bits(outs[1][b]), bits(outs[0][b]), err_msg=f"bus {b} moved")
    assert_same_bits(outs[1][1], tick(new_reverb(sr, params[1]), bad[1]), "the poisoned bus")
    assert np.isnan(outs[1][1][:, 130:]).all() and np.isfinite(outs[1][1][:, :50]).all()  # (the shortest comb is 50 slots: NaN all through from 101 on)
    assert_audible(outs[0], "non-finite")


def _two_oscillators(g, S, reverb=None):
    """the shape of tests/test_gpu_parity.py's _freeverb_patch: a saw and a square, into the two channels — through a FreeverbModule or straight"""
    osc, osc2 = g.add_module(S.MOD_OSCILLATOR), g.add_module(S.MOD_OSCILLATOR)
    fv = g.add_module(S.MOD_FREEVERB) if reverb is not None else None
    out = g.add_module(S.MOD_OUTPUT)
    g.set_field(osc, S.OSC_VAL, -1.0)
    g.set_field(osc2, S.OSC_VAL, 0.37)
    if fv is None:
        g.connect(osc, S.OSC_OUT_SAW, out, 0)
        g.connect(osc2, S.OSC_OUT_SQUARE, out, 1)
    else:
        g.connect(osc, S.OSC_OUT_SAW, fv, 0)
        g.connect(osc2, S.OSC_OUT_SQUARE, fv, 1)
        g.connect(fv, 0, out, 0)
        g.connect(fv, 1, out, 1)
        for f, v in enumerate(reverb):
            g.set_field(fv, f, v)


def test_against_the_module_in_the_graph(S):
    """the reverb behind the bus of a one-voice patch = the same oscillators through a FreeverbModule, bit for bit"""
    sr, T, room = 48000, 2500, ROOMS[0]
    a = S.Patch(sr, 64, 2)
    _two_oscillators(a, S)
    a.configure_voices(1)
    a.set_buses(1, gain=np.ones(1, dtype=np.float32))
    a.set_bus_reverbs(np.array([room]))
    _, _, _, bm = a.render_buses(T, flags=1)
    fx = a.bus_reverb(bm)
    b = S.Patch(sr, 64, 2)
    _two_oscillators(b, S, reverb=room)
    b.configure_voices(1)
    ref = b.render_channels(T, flags=1)[:, :, 0]
    assert_same_bits(fx[0], ref, "bus reverb against the module")
    assert_audible(fx, "against the module")
    assert_audible(fx[:, :, 2000:], "past the first comb")


def test_end_to_end_and_nothing_else_moves(S):
    """cfg3, 257 voices in 4 buses at 2000 Hz, 1500 samples in three calls with a field edit (a re-flatten) before the third: frames, mix,
    statistics, bus mixes and the kernel are what they are without reverbs; fx is the oracle's on the returned bus mix, the tail carrying
    on across the edit"""
    sr, V, n, NB = 2000, 257, 500, 4
    B2, build, overrides = S.bench_workload("cfg3", V)
    rng = np.random.default_rng(88)
    bus, gain = rng.integers(0, NB, V).astype(np.intc), rng.uniform(0.05, 0.3, V).astype(np.float32)
    params, enabled = np.array([ROOMS[0], ROOMS[1], DEFAULTS, ROOMS[3]]), [1, 1, 0, 1]

    def make():
        p = S.Patch(sr, B2, 2)
        ids = build(p, lfo_val=0.0)
        p.configure_voices(V)
        for m, f, v in overrides(ids):
            p.set_voice_field(m, f, v)
        p.set_buses(NB, bus, gain)
        return p, ids

    (p, ids), (q, _) = make(), make()
    p.set_bus_reverbs(params, enabled)
    fxs, bms = [], []
    for k in range(3):
        if k == 2:
            for g in (p, q):
                g.set_field(ids["vcf"], S.VCF_RES, 0.35)
        rp = p.render_buses(n, frames=True, mix=True, stats=True)
        rq = q.render_buses(n, frames=True, mix=True, stats=True)
        for what, x, y in zip(("frames", "mix", "statistics", "bus mixes"), rp, rq):
            np.testing.assert_array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8), err_msg=f"call {k}: {what} moved")
        fxs.append(p.bus_reverb(rp[3]))
        bms.append(rp[3])
        ip, iq = p.info(), q.info()
        assert ip.split("kernel=")[-1] == iq.split("kernel=")[-1] and "kernel=" in ip
        assert " busfx=3[block 10]" in ip and "busfx" not in iq and ip.replace(" busfx=3[block 10]", "") == iq
    assert p.get_bus_reverbs()[0] == NB  # (the edit re-flattened the patch: the reverbs are not part of it)
    fx, bm = np.concatenate(fxs, axis=2), np.concatenate(bms, axis=2)
    assert_audible(bm, "the bus mixes")
    for b in range(NB):
        assert_same_bits(fx[b], tick(new_reverb(sr, params[b]), bm[b]) if enabled[b] else bm[b], f"bus {b}")
    assert_audible(fx, "end to end")


def test_many_buses(S):
    sr, T, NB = 2000, 200, 300
    rng = np.random.default_rng(99)
    x = bursts(rng, 2 * NB, T).reshape(NB, 2, T)
    enabled = (np.arange(NB) % 2 == 0).astype(np.intc)
    params = np.column_stack([rng.uniform(0, 2, NB), (rng.random(NB) < 0.1).astype(float), rng.uniform(0.2, 1, NB), rng.uniform(0, 1, NB),
                              rng.uniform(0, 1, NB), rng.uniform(0, 1, NB)])
    p = host(S, sr, 2, NB)
    p.set_bus_reverbs(params, enabled)
    fx = run(p, x)
    assert "busfx=150[block 10]" in p.info()
    for b in range(NB):
        assert_same_bits(fx[b], tick(new_reverb(sr, params[b]), x[b]) if enabled[b] else x[b], f"bus {b}")
    assert_audible(fx[::2], "many buses")


def test_two_runs_give_the_same_bits(S):
    c = parity_case(S)
    outs = []
    for _ in range(2):
        p = host(S, c["sr"], 2, 5)
        p.set_bus_reverbs(c["params"], c["enabled"])
        outs.append(run(p, c["x"], [100, 500]))
    np.testing.assert_array_equal(bits(outs[0]), bits(outs[1]))
    assert_same_bits(outs[0], c["ref"], "and they are the oracle's")
    assert_audible(outs[0][:3], "determinism")
