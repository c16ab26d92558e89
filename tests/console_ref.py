"""The whole bus console as one NumPy function: send -> reverb -> VCA -> ladder on the VCA's envelope -> master, and the case the
console tests share (tests/test_console_host.py, tests/test_gpu_console.py, tests/console_stream_driver.py).

Nothing is computed here that is not computed by a reference which already stands: tests/sends_ref.send_tree, oracle.srack_numpy._Freeverb
ticked by tests/test_gpu_bus_reverb's new_reverb / change / tick / copy_of, tests/busvca_ref.bus_vca, tests/busvcf_ref.bus_filter,
tests/master_ref.master_tree and stats_sequential.  Each of them is held to the oracle bit for bit by its own host test, and a stage's
output is the next stage's input as the f32 words it is, so the composition adds no rounding: the criterion stays BIT EQUALITY.

The chain, fixed (test_gpu_console.run_chain and console_stream_driver.Buffers.enqueue make exactly these calls):
    sent = send(rows)                 out of place        rows f32 [n_buses][channels][n]
    fx   = reverb(sent)               out of place        f32 [n_buses][2][n]: the row shape changes here
    vca, env = vca(fx, ctl)           in place on fx, d_env handed out
    vcf  = filter(vca, cv = env)      in place
    master, stats = master(vcf)       f32 [2][n], f64 [2][STAT_COUNT] carried from call to call

An EDIT is a change of the Settings between two calls of chain(); the state follows with the library's lifecycle rules: a bus that becomes
GATE starts fresh and one that leaves GATE drops its state (busvca_ref.bus_vca hands back a fresh state for every bus that is not GATE),
a newly enabled filter starts from zeros and a disabled one drops its state (busvcf_ref.bus_filter likewise), a newly enabled reverb is a
new _Freeverb, a disabled one is dropped, and a changed reverb slider runs only the changed setters."""
import copy

import numpy as np

from tests import busvca_ref as RA
from tests import busvcf_ref as RF
from tests import master_ref as RM
from tests import sends_ref as RS
from tests.test_gpu_bus_reverb import DEFAULTS as RV_DEFAULTS, ROOMS, bursts, change, copy_of, new_reverb, tick
from tests.test_gpu_bus_vca import gate_row

STAGES = ("sends", "reverb", "vca", "filter", "master")
KEYS = ("sent", "fx", "vca", "env", "vcf", "master")   # the f32 intermediates, in the chain's order ("stats" is f64)
CUTS = (1, 63, 64, 65, 700, 1107, 1000)
SEED, SEED3 = 2101, 2103                               # chosen so that the guards of tests/test_console_host.py hold; figures there


def same_bits(a, b):
    return RM.same_bits(a, b)


class Settings:
    """n_buses, channels, rate; send_src, send_dst int [n_sends], send_gain f32 [n_sends][2], through f32 [n_buses][2]; rv_params f64
    [n_buses][6], rv_enabled [n_buses]; vca_params f32 [n_buses][4], vca_mode, vca_negative [n_buses]; vcf_params f32 [n_buses][3],
    vcf_port, vcf_enabled [n_buses]; master_gain f32 [n_buses][2]"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def copy(self):
        return Settings(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.__dict__.items()})


class State:
    """what the console carries from call to call: reverbs {bus: [_Freeverb, the six parameters it was last given]}, vcf f32
    [n_buses][2][10], vca f32 [n_buses][6], stats f64 [2][STAT_COUNT]"""

    def __init__(self, n_buses, rate):
        self.reverbs = {}
        self.vcf = np.zeros((n_buses, 2, RF.NSTATE), dtype=np.float32)
        self.vca = RA.fresh(n_buses, rate)
        self.stats = np.zeros((2, RM.STAT_COUNT), dtype=np.float64)

    def copy(self):
        return copy.deepcopy(self)


def reset(state, stage):
    """srack_buses_reset_reverb / _filter / _vca on the reference's state -> a new State"""
    st = state.copy()
    if stage == "reverb":
        st.reverbs = {}      # (every enabled bus gets a new _Freeverb with its current parameters on the next call)
    elif stage == "filter":
        st.vcf[:] = 0
    elif stage == "vca":
        st.vca = RA.fresh(len(st.vca), st.vca[0, 4])
    else:
        raise ValueError(stage)
    return st


def chain(rows, ctl, s, state):
    """One call of every stage: rows f32 [n_buses][channels][n], ctl f32 [n_buses][n], s Settings, state State (left alone)
    -> ({"sent", "fx", "vca", "env", "vcf", "master", "stats"}, the new State)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    assert rows.shape[:2] == (s.n_buses, s.channels), rows.shape
    st = state.copy()
    for b in list(st.reverbs):
        if not s.rv_enabled[b]:
            del st.reverbs[b]
    for b in np.flatnonzero(s.rv_enabled).tolist():
        par = tuple(float(v) for v in s.rv_params[b])
        if b not in st.reverbs:
            st.reverbs[b] = [new_reverb(s.rate, par), par]
        elif st.reverbs[b][1] != par:
            change(st.reverbs[b][0], st.reverbs[b][1], par)
            st.reverbs[b][1] = par
    o = {}
    o["sent"] = RS.send_tree(rows, s.send_src, s.send_dst, s.send_gain, s.through)
    o["fx"] = np.stack([tick(st.reverbs[b][0], o["sent"][b]) if s.rv_enabled[b] else copy_of(o["sent"][b]) for b in range(s.n_buses)])
    o["vca"], o["env"], st.vca, _ = RA.bus_vca(o["fx"], ctl, s.vca_params, s.vca_mode, s.vca_negative, s.rate, st.vca)
    o["vcf"], st.vcf = RF.bus_filter(o["vca"], o["env"], s.vcf_params, s.vcf_port, s.vcf_enabled, st.vcf)
    o["master"] = RM.master_tree(o["vcf"], s.master_gain)
    o["stats"] = st.stats = RM.stats_sequential(o["master"], st.stats)
    return o, st


class Edit:
    """at the boundary in front of cut `cut`: `change(settings)` alters the Settings in place (None: a reset of `stage`'s state)"""

    def __init__(self, cut, name, stage, change=None):
        self.cut, self.name, self.stage, self.change = cut, name, stage, change

    def __repr__(self):
        return f"{self.name}@{self.cut}"


def apply(edits, cut, s, state, skip=None):
    """the edits in front of cut `cut`, but `skip` -> (Settings, State), the arguments left alone"""
    s = s.copy()
    for e in edits:
        if e.cut != cut or e is skip:
            continue
        if e.change is None:
            state = reset(state, e.stage)
        else:
            e.change(s)
    return s, state


def render(rows, ctl, s, cuts, edits=(), state=None):
    """the chain in calls of `cuts` samples, the edits made in front of their cuts
    -> (the intermediates joined along time, per cut the State BEHIND it and the Settings it ran with)"""
    state = State(s.n_buses, s.rate) if state is None else state
    parts, states, settings, at = [], [], [], 0
    for k, n in enumerate(cuts):
        s, state = apply(edits, k, s, state)
        o, state = chain(rows[:, :, at:at + n], ctl[:, at:at + n], s, state)
        parts.append(o)
        states.append(state)
        settings.append(s)
        at += n
    out = {key: np.concatenate([p[key] for p in parts], axis=-1) for key in KEYS}
    out["stats"] = parts[-1]["stats"]
    out["stats_per_cut"] = np.stack([p["stats"] for p in parts])
    return out, states, settings


# ---- the case --------------------------------------------------------------------------------------------------------------------------
def case(n_buses=70, channels=2, T=3000, seed=SEED, n_aux=4, rate=48000):
    """-> (rows f32 [n_buses][channels][T] noise bursts, ctl f32 [n_buses][T], Settings).  The last n_aux buses are aux buses fed by all
    the others; every other bus is fed by three of its kind besides (bursts are silent four samples in five: a VCA or a filter on one
    burst row alone would hand most of its input on as it is)."""
    rng = np.random.default_rng(seed)
    rows = bursts(rng, n_buses * channels, T).reshape(n_buses, channels, T)
    n_dry = n_buses - n_aux
    aux = np.arange(n_dry, n_buses)
    src = [b for a in aux for b in range(n_dry)] + [(b + k) % n_dry for b in range(n_dry) for k in (1, 7, 13) if n_dry > k]
    dst = [a for a in aux for b in range(n_dry)] + [b for b in range(n_dry) for k in (1, 7, 13) if n_dry > k]
    gain = rng.uniform(-0.5, 0.5, (len(src), 2)).astype(np.float32)
    gain[rng.random(len(src)) < 0.2] = 1.0
    through = np.ones((n_buses, 2), dtype=np.float32)
    some = rng.random(n_buses) < 0.5
    through[some] = rng.uniform(0.5, 1.5, (int(some.sum()), 2)).astype(np.float32)
    through[aux] = rng.uniform(0.0, 0.3, (n_aux, 2)).astype(np.float32)
    rv_params = np.tile(np.array(RV_DEFAULTS, dtype=np.float64), (n_buses, 1))
    rv_enabled = np.zeros(n_buses, dtype=np.intc)
    for k, a in enumerate(aux[:2]):
        rv_params[a], rv_enabled[a] = ROOMS[(0, 3)[k]], 1
    vca_mode = rng.integers(0, 3, n_buses).astype(np.intc)
    vca_mode[:3] = (RA.GATE, RA.CV, RA.OFF)
    vca_mode[aux[0]], vca_mode[aux[-1]] = RA.GATE, RA.CV
    vca_negative = (rng.random(n_buses) < 0.5).astype(np.intc)
    vca_params = np.stack([0.02 * rng.random(n_buses) ** 2, 0.02 * rng.random(n_buses) ** 2, rng.uniform(0.2, 1.0, n_buses), 0.02 * rng.random(n_buses) ** 2],
                          axis=1).astype(np.float32)
    ctl = np.stack([gate_row(rng, T) for _ in range(n_buses)])   # a gate row serves as a CV as well: a bus may change its mode in an edit
    cvb = np.flatnonzero(vca_mode == RA.CV)
    ctl[cvb[::2]] = rng.uniform(-1.0, 1.0, (len(cvb[::2]), T)).astype(np.float32)
    vcf_params = np.stack([rng.uniform(0.02, 0.6, n_buses), rng.uniform(0.0, 1.0, n_buses), rng.uniform(-1.0, 1.0, n_buses)], axis=1).astype(np.float32)
    vcf_port = (np.arange(n_buses) % 3).astype(np.intc)
    rng.shuffle(vcf_port)
    vcf_enabled = (np.arange(n_buses) % 2 == 0).astype(np.intc)
    vcf_enabled[aux[0]] = 1
    master_gain = rng.uniform(-1.0, 1.0, (n_buses, 2)).astype(np.float32)
    s = Settings(n_buses=n_buses, channels=channels, rate=rate, send_src=np.array(src, dtype=np.intc), send_dst=np.array(dst, dtype=np.intc),
                 send_gain=gain, through=through, rv_params=rv_params, rv_enabled=rv_enabled, vca_params=vca_params, vca_mode=vca_mode,
                 vca_negative=vca_negative, vcf_params=vcf_params, vcf_port=vcf_port, vcf_enabled=vcf_enabled, master_gain=master_gain)
    for a in (rows, ctl):
        a.setflags(write=False)
    return rows, ctl, s


def edits(s, run, seed=SEED):
    """The edits of the stream tests for the case of 70 buses cut as CUTS, in two runs of the chain, one host action per boundary (the
    first host-side wait behind a stalled cut is the one that is tested: a second edit at the same boundary would find the stream idle).
    "grow": a fresh handle, so the sends' and the master's scratch grows with the cuts; the edits that wait when they are MADE (they read
    state back, or free some).  "primed": a handle whose scratch has its final size; the edits that wait inside the stage's next CALL."""
    rng = np.random.default_rng(seed + 1)
    n = s.n_buses
    aux = np.arange(n - 4, n)
    new_master = rng.uniform(-1.0, 1.0, (n, 2)).astype(np.float32)
    more_src = [a for a in aux for _ in aux] + list(range(n - 4)) * 2
    more_dst = [b for _ in aux for b in aux] + [(b * 5 + 3) % (n - 4) for b in range(n - 4)] + [aux[b % 4] for b in range(n - 4)]
    more_gain = rng.uniform(-0.5, 0.5, (len(more_src), 2)).astype(np.float32)

    def vca_sliders(x):
        old = x.vca_params
        x.vca_params = np.stack([np.float32(0.02) - old[:, 0], np.float32(0.02) - old[:, 1], np.float32(1.2) - old[:, 2], np.float32(0.02) - old[:, 3]], axis=1).astype(np.float32)
        x.vca_negative = (1 - x.vca_negative).astype(np.intc)

    def master_gains(x):
        x.master_gain = new_master.copy()

    def vcf_sliders(x):
        x.vcf_params = np.stack([np.float32(0.62) - x.vcf_params[:, 0], np.float32(1.0) - x.vcf_params[:, 1], -x.vcf_params[:, 2]], axis=1).astype(np.float32)
        x.vcf_port = ((x.vcf_port + 1) % 3).astype(np.intc)

    def vca_modes(x):   # GATE -> CV, CV -> OFF, OFF -> GATE on every second bus
        x.vca_mode = np.where(np.arange(n) % 2 == 0, (x.vca_mode + 2) % 3, x.vca_mode).astype(np.intc)

    def reverb_slider(x):
        x.rv_params = x.rv_params.copy()
        x.rv_params[aux[0], 2], x.rv_params[aux[0], 5] = 0.3, 0.2     # wet, dry
        x.rv_params[aux[1], 4] = 0.8                                  # room size

    def vcf_more(x):
        x.vcf_enabled = np.ones(n, dtype=np.intc)
        x.vcf_enabled[[5, 11, 17, 23]] = 0

    def sends_longer(x):
        x.send_src = np.concatenate([x.send_src, np.array(more_src, dtype=np.intc)])
        x.send_dst = np.concatenate([x.send_dst, np.array(more_dst, dtype=np.intc)])
        x.send_gain = np.concatenate([x.send_gain, more_gain])

    def reverb_swap(x):
        x.rv_enabled = x.rv_enabled.copy()
        x.rv_enabled[aux[1]], x.rv_enabled[aux[2]] = 0, 1
        x.rv_params = x.rv_params.copy()
        x.rv_params[aux[2]] = ROOMS[2]

    def vcf_fewer(x):
        x.vcf_enabled = x.vcf_enabled.copy()
        x.vcf_enabled[np.arange(n) % 3 == 1] = 0

    if run == "grow":
        return [Edit(2, "vca modes", "vca", vca_modes), Edit(3, "filter enables more", "filter", vcf_more), Edit(4, "reverb swap", "reverb", reverb_swap),
                Edit(5, "sends longer", "sends", sends_longer), Edit(6, "filter disables some", "filter", vcf_fewer)]
    assert run == "primed", run
    return [Edit(1, "vca sliders", "vca", vca_sliders), Edit(2, "filter sliders", "filter", vcf_sliders), Edit(3, "reverb slider", "reverb", reverb_slider),
            Edit(4, "master gains", "master", master_gains), Edit(6, "vca reset", "vca", None)]


STATE_READS = {"grow": 1, "primed": 5}   # the cut in front of which a run reads bus_vca_state() and bus_filter_state() in flight, nothing else


# ---- a Settings object onto a handle -----------------------------------------------------------------------------------------------------
def push(p, s, stage):
    if stage == "sends":
        p.set_sends(s.send_src, s.send_dst, s.send_gain, s.through)
    elif stage == "reverb":
        p.set_bus_reverbs(s.rv_params, s.rv_enabled)
    elif stage == "vca":
        p.set_bus_vca(s.vca_params, s.vca_mode, s.vca_negative)
    elif stage == "filter":
        p.set_bus_filter(s.vcf_params, s.vcf_port, s.vcf_enabled)
    elif stage == "master":
        p.set_master(s.master_gain)
    else:
        raise ValueError(stage)


def push_all(p, s):
    for stage in STAGES:
        push(p, s, stage)


def reset_on_device(p, stage):
    {"reverb": p.reset_bus_reverbs, "filter": p.reset_bus_filter, "vca": p.reset_bus_vca}[stage]()


def host(S, s):
    """a handle to hang the console on: an oscillator into every channel, one voice in bus 0 of n_buses (never rendered)"""
    p = S.Patch(s.rate, 64, s.channels)
    osc, out = p.add_module(S.MOD_OSCILLATOR), p.add_module(S.MOD_OUTPUT)
    for c in range(s.channels):
        p.connect(osc, S.OSC_OUT_SINE, out, c)
    p.configure_voices(1)
    p.set_buses(s.n_buses)
    push_all(p, s)
    return p


# ---- the guards: is the reference worth comparing with? -----------------------------------------------------------------------------------
def fraction_differing(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.count_nonzero(~same_bits(a, b))) / max(1, a.size)


def stage_counts(rows, out, s):
    """per stage, (the samples on which its output differs from its input, the samples) over the buses it is enabled on (the sends: the
    buses that receive one)"""
    used = min(s.channels, 2)
    fed = np.unique(s.send_dst)
    rv, va, vf = np.flatnonzero(s.rv_enabled), np.flatnonzero(s.vca_mode != RA.OFF), np.flatnonzero(s.vcf_enabled)
    fx_in = np.stack([copy_of(x) for x in out["sent"]])
    pairs = {"sends": (out["sent"][fed, :used], rows[fed, :used]), "reverb": (out["fx"][rv], fx_in[rv]),
             "vca": (out["vca"][va], out["fx"][va]), "filter": (out["vcf"][vf], out["vca"][vf])}
    return {k: (int(np.count_nonzero(~same_bits(a, b))), a.size) for k, (a, b) in pairs.items()}


def stage_fractions(rows, out, settings, cuts=None):
    """-> {stage: the fraction of samples on which its output differs from its input}; `settings` one Settings, or one per cut of `cuts`
    (a render with edits: every cut is counted with the settings it ran with)"""
    if cuts is None:
        settings, cuts = [settings], [rows.shape[2]]
    total, at = {}, 0
    for s, n in zip(settings, cuts):
        part = stage_counts(rows[:, :, at:at + n], {k: out[k][..., at:at + n] for k in KEYS}, s)
        for k, (d, size) in part.items():
            total[k] = (total.get(k, (0, 0))[0] + d, total.get(k, (0, 0))[1] + size)
        at += n
    return {k: d / max(1, size) for k, (d, size) in total.items()}
