"""The whole bus console on the device: srack_buses_send -> _reverb -> _vca (in place, d_env handed out) -> _filter (in place, swept by
that envelope) -> _master with statistics, against tests/console_ref.py — the composition of the references every stage is already held
to.  The criterion is BIT EQUALITY of every intermediate (NaN matching NaN), derived, not measured: each stage's own test establishes it
for that stage, and a stage's output is the next one's input word for word.  No tolerance anywhere in this file.  The guards that make
the reference worth comparing with are asserted in tests/test_console_host.py, with their figures.

Part one (tests 1-5) runs in process on the null stream, the way the stages' own files do.  Part two compares arrays which
tests/console_stream_driver.py wrote in a process of its own (torch must start HIP before the library loads: INTEGRATION.md section 3):
the same chain on the caller's streams, nothing synchronised, with settings edited, state read back, streams destroyed and tables
replaced while the previous calls are provably still waiting behind a stalled stream.  What is held there is the stream contract of
DESIGN.md section 3: the caller orders its own buffers; the library orders its state, tables and scratch across calls, streams and edits.

Measured on one MI355X: the driver's process takes 4.2 s, 1.8 s of them behind the imports (about 1 s of that is stalls); 20 ms of
torch.cuda._sleep came out as 46 074 031 cycles (the driver calibrates at start and prints the figure).  This file adds 6 s to `-m gpu`."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import srack_pkg
from tests import console_ref as CR
from tests.test_console_host import CUTS3
from tests.test_gpu_mix_buses import maker, mixed_gains

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def S():
    return srack_pkg.load()


def assert_same_bits(got, ref, what=""):
    got, ref = np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ok = CR.same_bits(got, ref)
    if not ok.all():
        at = np.argwhere(~ok)
        first = tuple(at[0])
        raise AssertionError(f"{what}: {len(at)} of {ok.size} values differ, first at {first}: got {got[first]!r} "
                             f"({got.view(np.uint32)[first]:#010x}), reference {ref[first]!r} ({ref.view(np.uint32)[first]:#010x})")


def assert_same_console(got, ref, what):
    for key in CR.KEYS:
        assert_same_bits(got[key], ref[key], f"{what}: {key}")
    assert got["stats"].shape == ref["stats"].shape and (got["stats"] == ref["stats"]).all(), f"{what}: master statistics\n{got['stats']}\n{ref['stats']}"


@functools.lru_cache(maxsize=None)
def reference(n_buses=70, channels=2, T=3000, seed=CR.SEED, n_aux=4, rate=48000, run=None):
    """the case and its reference cut as CR.CUTS (which test_console_host.py holds to the uncut one), computed once and shared"""
    rows, ctl, s = CR.case(n_buses, channels, T, seed, n_aux, rate)
    cuts = CR.CUTS if T == 3000 else [T]
    out, states, settings = CR.render(rows, ctl, s, cuts, CR.edits(s, run) if run else ())
    for a in out.values():
        a.setflags(write=False)
    return rows, ctl, s, out, states, settings


class Device:
    """buffers of a staging scope (S.DeviceScope, which frees them), copied synchronously on the null stream"""

    def __init__(self, S, scope):
        self.lib, self.alloc = S.lib, scope.alloc

    def up(self, d, a):
        a = np.ascontiguousarray(a)
        if a.nbytes:
            assert self.lib.srack_device_from_host(d, a.ctypes.data_as(C.c_void_p), a.nbytes, None) == 0

    def down(self, d, shape, dtype=np.float32):
        a = np.empty(shape, dtype=dtype)
        if a.nbytes:
            assert self.lib.srack_device_to_host(a.ctypes.data_as(C.c_void_p), d, a.nbytes, None) == 0
        assert self.lib.srack_device_sync(None) == 0
        return a


def run_chain(S, p, rows, ctl, cuts, render=None):
    """The chain on the null stream in calls of `cuts` samples, every intermediate read back between the stages.  render(n, d_rows):
    where the rows come from when not from `rows` (test 4)."""
    nb, ch, T = rows.shape
    parts, at = {k: [] for k in CR.KEYS}, 0
    with S.DeviceScope() as scope:
        dev = Device(S, scope)
        d_stats = dev.alloc(8 * 2 * S.STAT_COUNT)
        dev.up(d_stats, np.zeros((2, S.STAT_COUNT)))
        for n in cuts:
            d_rows, d_sent, d_buf, d_ctl, d_env, d_master = (dev.alloc(4 * k * n) for k in (nb * ch, nb * ch, nb * 2, nb, nb, 2))
            if render is None:
                dev.up(d_rows, rows[:, :, at:at + n])
            else:
                render(n, d_rows)
            dev.up(d_ctl, ctl[:, at:at + n])
            dev.up(d_sent, np.zeros((nb, ch, n), dtype=np.float32))   # (channels beyond the second are not written)
            p.send_raw(n, d_rows, ch, d_sent)
            parts["sent"].append(dev.down(d_sent, (nb, ch, n)))
            p.bus_reverb_raw(n, d_sent, d_buf)
            parts["fx"].append(dev.down(d_buf, (nb, 2, n)))
            p.bus_vca_raw(n, d_buf, 2, d_ctl, d_buf, d_env)
            parts["vca"].append(dev.down(d_buf, (nb, 2, n)))
            parts["env"].append(dev.down(d_env, (nb, n)))
            p.bus_filter_raw(n, d_buf, 2, d_env, d_buf)
            parts["vcf"].append(dev.down(d_buf, (nb, 2, n)))
            p.master_raw(n, d_buf, 2, d_master, d_stats)
            parts["master"].append(dev.down(d_master, (2, n)))
            at += n
        out = {k: np.concatenate(v, axis=-1) for k, v in parts.items()}
        out["stats"] = dev.down(d_stats, (2, S.STAT_COUNT), np.float64)
        return out


# ---- 1, 2. the chain in one call and in the cuts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cuts", [(3000,), CR.CUTS], ids=["one call", "cuts"])
def test_the_chain(S, cuts):
    rows, ctl, s, ref, states, _ = reference()
    p = CR.host(S, s)
    got = run_chain(S, p, rows, ctl, cuts)
    assert_same_console(got, ref, f"calls of {cuts}")
    assert_same_bits(p.bus_vca_state(), states[-1].vca, "the VCAs' state")
    assert_same_bits(p.bus_filter_state(), states[-1].vcf, "the filters' state")
    info = p.info()
    assert all(t in info for t in (" sends=", f" busvcf={int(s.vcf_enabled.sum())}[2 waves]", " busvca=", " busfx=2[block 244]", " master=70[2 runs]")), info


# ---- 3. three channels: row_channels = 3 into the reverb, 2 behind it ---------------------------------------------------------------------------
@pytest.mark.parametrize("cuts", [(400,), CUTS3], ids=["one call", "cuts"])
def test_three_channels(S, cuts):
    rows, ctl, s, ref, states, _ = reference(5, 3, 400, CR.SEED3, 2, 2000)
    p = CR.host(S, s)
    got = run_chain(S, p, rows, ctl, cuts)
    assert_same_console(got, ref, f"three channels, calls of {cuts}")
    assert not got["sent"][:, 2].any() and rows[:, 2].any(), "the third channel is not sent (and is not silent going in)"
    assert_same_bits(p.bus_vca_state(), states[-1].vca, "the VCAs' state")
    assert_same_bits(p.bus_filter_state(), states[-1].vcf, "the filters' state")


# ---- 4. from the voices: srack_render_buses with one voice per bus, then the console ------------------------------------------------------------
def voices_case(S, V=70, T=300):
    """tests/test_gpu_mix_buses.py::test_one_voice_per_bus_is_exact's patch and table (without its NaN voices: one NaN through an aux send
    is a master of NaN) -> (make(): a fresh patch with its table set, bus, gain)"""
    rng = np.random.default_rng(V + T)
    bus, gain = rng.permutation(V), mixed_gains(V, rng)
    make = maker(S, "cfg3", V)

    def made():
        p = make()
        p.set_buses(V, bus, gain)
        return p
    return made, bus, gain


def test_from_the_voices(S):
    V, T = 70, 300
    _, ctl, s, _, _, _ = reference()
    make, bus, gain = voices_case(S, V, T)
    alone = make()
    fr, _ = alone.render(T, mix=False)       # the same patch's frames, rendered alone: [planes][T][V]
    _, cp = alone.planes()
    rows = np.zeros((V, 2, T), dtype=np.float32)
    for c, plane in enumerate(cp):
        if plane >= 0:
            rows[bus, c] = (fr[plane] * gain[None, :]).T    # one voice per bus: the f32 product is the bus mix
    ref, states, _ = CR.render(rows, ctl[:, :T], s, [T])
    for key in CR.KEYS:
        assert np.isfinite(ref[key]).all(), key
    m = ref["master"]
    assert np.abs(m).max() > 1e-3 and np.count_nonzero(m) > m.size // 4 and np.count_nonzero(rows) > rows.size // 4, "the patch is (nearly) silent"
    p = make()
    CR.push_all(p, s)
    got = run_chain(S, p, rows, ctl[:, :T], [T], render=lambda n, d_rows: p.render_buses_raw(n, d_rows))
    assert_same_console(got, ref, "render_buses, then the console")
    assert "buses=70[fold]" in p.info() and " master=70[2 runs]" in p.info(), p.info()


# ---- 5. the five stages go with the mix table: another n_buses, srack_voices_configure -----------------------------------------------------------
NOTES = (" sends=", " busvcf=", " busvca=", " busfx=", " master=")


def notes_of(p, s):
    """what srack_render_info says of the console once every stage has run with the settings s, the filters and the master on two channels"""
    runs = int(((1 + np.bincount(s.send_dst, minlength=s.n_buses) + 63) // 64).sum())
    vcf = int(np.count_nonzero(s.vcf_enabled))
    return (f" sends={len(s.send_src)}[{runs} runs] busvcf={vcf}[{(2 * vcf + 63) // 64} waves] busvca={int(np.count_nonzero(s.vca_mode != 0))}"
            f"[{int(np.count_nonzero(s.vca_mode == 2))} gated] busfx={int(np.count_nonzero(s.rv_enabled))}[block {p.bus_reverb_plan()[1]}]"
            f" master={s.n_buses}[{(s.n_buses + 63) // 64} runs]")


def nothing_set(p):
    return (p.get_sends() is None and p.get_bus_reverbs()[0] == 0 and p.get_bus_vca()[0] == 0 and p.get_bus_filter()[0] == 0 and p.get_master() is None
            and not any(t in p.info() for t in NOTES))


# (130 samples: two tiles of 64 and a tail of 2.  2 kHz: the reverb's lines are 10 .. 74 slots, so its tail is in the state that must go)
@pytest.mark.parametrize("how,first,second", [("another n_buses", (3, 2, 130, CR.SEED3 + 23, 1, 2000), (5, 2, 130, CR.SEED3 + 3, 2, 2000)),
                                              ("configure_voices", (3, 2, 66, CR.SEED3 + 10, 1, 2000), None)], ids=["another n_buses", "configure_voices"])
def test_the_stages_go_with_the_table(S, how, first, second):
    """One handle: the chain, then the table goes (srack_voices_set_buses with another n_buses; srack_voices_configure) and every stage
    with it, then all five set again and the chain again — both runs held to the reference FROM FRESH STATE.
    The guard, on the reference alone: had the first run's state stayed, a second run of the same rows would differ from the fresh one on
    more than 1/16 of the reverbs', the envelopes' and the filters' samples (the seeds are chosen for it: 0.33, 0.22, 0.67 of them for
    the 130 samples, 0.33, 0.31, 0.67 for the 66; one bus in three has a reverb, one is gated)."""
    rows, ctl, s, ref, states, _ = reference(*first)
    T = rows.shape[2]
    carried, _, _ = CR.render(rows, ctl, s, [T], state=states[-1])
    assert np.abs(ref["master"]).max() > 1e-3 and np.count_nonzero(ref["master"]) > T // 2, "the master is (nearly) silent"
    assert all(CR.fraction_differing(carried[k], ref[k]) > 1 / 16 for k in ("fx", "env", "vcf")), "state that stayed is meant to show in the second run"
    p = CR.host(S, s)
    assert_same_console(run_chain(S, p, rows, ctl, [T]), ref, f"{how}: the first run")
    assert notes_of(p, s) in p.info(), p.info()
    if how == "another n_buses":
        p.set_buses(second[0])
        rows, ctl, s, ref, states, _ = reference(*second)
    else:
        p.configure_voices(1)
        assert not any(t in p.info() for t in NOTES), p.info()
        p.set_buses(s.n_buses)
    assert nothing_set(p), p.info()
    CR.push_all(p, s)
    assert_same_console(run_chain(S, p, rows, ctl, [T]), ref, f"{how}: the second run")
    assert_same_bits(p.bus_vca_state(), states[-1].vca, "the VCAs' state")
    assert_same_bits(p.bus_filter_state(), states[-1].vcf, "the filters' state")
    assert notes_of(p, s) in p.info(), p.info()


# ---- part two: the caller's streams (tests/console_stream_driver.py) ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driven(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("console") / "streams.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "console_stream_driver.py"), path], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, f"the driver failed (rc {r.returncode}):\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return dict(np.load(path))


def console_of(d, tag):
    return {k: d[f"{tag}_{k}"] for k in CR.KEYS + ("stats",)}


def assert_busy(d, tag):
    """A condition on the test's own worth, not a measurement: at every in-flight host action the stream had not run its calls yet."""
    busy = d[f"{tag}_busy"]
    assert busy.size >= 1 and busy.all(), f"{tag}: the stream was idle at in-flight point(s) {np.flatnonzero(~busy.ravel()).tolist()} of {busy.size}: lengthen the stall"


def test_the_stall_is_one(driven):
    ms = float(driven["stall_ms"])
    print(f"stall: {ms:.2f} ms by {str(driven['stall_how'])} ({int(driven['stall_cycles'])} cycles)")
    assert 2.0 <= ms <= 200.0


def test_one_stream_no_synchronisation(driven):
    _, _, _, ref, _, _ = reference()
    assert_same_console(console_of(driven, "s1"), ref, "one stream")


@pytest.mark.parametrize("run", ["grow", "primed"])
def test_edits_in_flight(driven, run):
    _, _, s, ref, states, _ = reference(run=run)
    tag = "s2" + run
    assert_busy(driven, tag)
    assert driven[f"{tag}_busy"].size == len(CR.CUTS) - 1, "a host action at every boundary"
    got = console_of(driven, tag)
    at = np.concatenate([[0], np.cumsum(CR.CUTS)])
    for k in range(len(CR.CUTS)):   # cut by cut: a missing wait shows on the cut BEFORE the edit
        for key in CR.KEYS:
            assert_same_bits(got[key][..., at[k]:at[k + 1]], ref[key][..., at[k]:at[k + 1]], f"{run}, cut {k}: {key}")
        assert (driven[f"{tag}_stats_per_cut"][k] == ref["stats_per_cut"][k]).all(), f"{run}, cut {k}: master statistics"
    k = CR.STATE_READS[run] - 1
    assert_same_bits(driven[f"{tag}_vca_state"], states[k].vca, f"{run}: bus_vca_state() in flight behind cut {k}")
    assert_same_bits(driven[f"{tag}_vcf_state"], states[k].vcf, f"{run}: bus_filter_state() in flight behind cut {k}")
    assert_same_bits(driven[f"{tag}_vca_state_end"], states[-1].vca, f"{run}: the VCAs' state at the end")
    assert_same_bits(driven[f"{tag}_vcf_state_end"], states[-1].vcf, f"{run}: the filters' state at the end")
    if run == "grow":
        assert sum(CR.CUTS[k] > max(CR.CUTS[:k]) for k in range(1, len(CR.CUTS))) >= 1, "the scratch grows while a call is pending"


def test_two_streams_take_turns(driven):
    _, _, _, ref, _, _ = reference()
    assert_busy(driven, "s3a")
    assert_same_console(console_of(driven, "s3a"), ref, "cuts alternating between two streams")


@pytest.mark.parametrize("stage", ["master", "sends"])
def test_two_streams_share_the_scratch(driven, stage):
    rows, _, s, ref, _, _ = reference()
    assert_busy(driven, "s3b_" + stage)
    x, y = (ref["vcf"], ref["fx"]) if stage == "master" else (np.ascontiguousarray(rows[:, :, :700]), np.ascontiguousarray(rows[::-1, :, :700]))
    f = (lambda a: CR.RM.master_tree(a, s.master_gain)) if stage == "master" else (lambda a: CR.RS.send_tree(a, s.send_src, s.send_dst, s.send_gain, s.through))
    want_x, want_y = f(x), f(y)
    assert CR.fraction_differing(want_x, want_y) > 0.5, "the two calls are meant to give different samples"
    got_x, got_y = driven[f"s3b_{stage}_x"], driven[f"s3b_{stage}_y"]
    for i in range(len(got_x)):
        assert_same_bits(got_x[i], want_x, f"{stage}, pair {i}, stream A")
        assert_same_bits(got_y[i], want_y, f"{stage}, pair {i}, stream B")


@pytest.mark.parametrize("stage,key", [("vca", "vca"), ("vca", "env"), ("filter", "vcf"), ("reverb", "fx")])
def test_two_streams_share_the_state(driven, stage, key):
    _, _, _, ref, _, _ = reference()
    assert_busy(driven, "s3c_" + stage)
    assert_same_bits(driven[f"s3c_{stage}_{key}"], ref[key], f"{stage} alone, cuts alternating between two streams")


def test_streams_and_state_that_go_away(driven):
    _, _, _, ref, _, _ = reference()
    assert_busy(driven, "s4")
    assert_same_console(console_of(driven, "s4"), ref, "five cuts on a stream destroyed behind them, two on another, then set_buses in flight")
    _, _, _, ref33, _, _ = reference(33, 2, 400, CR.SEED3 + 1, 3, 48000)
    assert_same_console(console_of(driven, "s4new"), ref33, "a fresh console of 33 buses")


def test_render_buses_on_a_stream(driven):
    assert_busy(driven, "s5")
    for key in ("bus_mix", "sent", "master"):
        got, want, unedited = driven[f"s5_{key}"], driven[f"s5null_{key}"], driven[f"s5plain_{key}"]
        assert np.isfinite(want).all() and np.abs(want).max() > 1e-3 and np.count_nonzero(want) > want.size // 4, f"{key} is (nearly) silent"
        assert_same_bits(got, want, f"on the stream against the null stream: {key}")
        half = want.shape[-1] // 2
        assert CR.same_bits(want[..., :half], unedited[..., :half]).all() and CR.fraction_differing(want[..., half:], unedited[..., half:]) > 1 / 16, \
            f"{key}: the new table is meant to show from the third call on"
