"""Warm starts (notes/r27.md): a render whose starting point is not zeros — every state field of every module (graph.cpp,
Graph::field_is_state) and the saved block of every port, as a rack file written by a running app carries them.  The cases, the oracle
references and the checker that tests/test_gpu_warm.py (on the device) and tests/test_warm_host.py (the guards, on the oracle and the
library's host side alone) share.

A starting point is made by the oracle alone: an OraclePatch is run for whole blocks (T0 = B * ceil(1500 / B) samples), every field is
read with get_field and every port with get_output (`harvest`), and the state fields and the blocks are written into a FRESH patch
(`apply`) — an OraclePatch for the reference, a Patch of the library for the device.  The reference is always such a fresh oracle, never
the warm one continued: the noise counter counts from srack_voices_configure and a reverb's lines are no fields, so both restart on both
sides.

Two state routes:
    "common"   the patch is warmed up as voice 0's instance WITHOUT the family's per-voice parameter overrides; the harvest is patch-level
               and the overrides are applied afterwards: the voices diverge from one running rack.  What is voice-invariant stays so: the
               control units' ring and state prologues start warm.
    "voices"   a clone per voice is warmed up WITH that voice's parameters.  Voice 0's harvest (fields and blocks) is written at patch level;
               every state field whose harvest differs between voices is passed as one more per-voice override on both sides
               (set_voice_field on the library's, f64 for OSC_POS; render_batch's override list on the oracle's).  The ABI has no per-voice
               block: every voice starts from voice 0's blocks, on both sides.
Two delivery routes, by the seed's parity: even — the graph API (set_field, set_output_buffer); odd — a file,
load_srk(load_srk(p.save_srk()).save_srk()) (a load reverses the module order; two loads restore it, and the plan with it).
"""
import contextlib
import functools
import os
from typing import NamedTuple

import numpy as np

from tests import handoff_ref as H

ROUTES = ("common", "voices")
FAMILIES = {"plain": range(60), "noise": range(20), "nonlin": range(2000, 2015)}
CASES = [(fam, s) for fam, seeds in FAMILIES.items() for s in seeds]
EXACT_FLAGS, EXACT_SPECIAL = (1, 3, 5, 7, 9, 11), (35, 39)     # as tests/test_gpu_fuzz.py: the special ones on every third seed
DEFAULT_FLAGS, DEFAULT_SPECIAL = (0, 2, 4), (34,)
FIRST_VOICES = (0, 63, 64)                                        # ... and V - 1: where the table is read back before the first render

N_FIELDS = {0: 0, 1: 4, 2: 13, 3: 10, 4: 1, 5: 4, 6: 2, 7: 7, 8: 4, 9: 1, 10: 6, 11: 0, 12: 6}   # fields per module type (include/srack_hip.h)
N_PORTS = {0: 0, 1: 3, 2: 3, 3: 1, 4: 1, 5: 1, 6: 1, 7: 3, 8: 9, 9: 1, 10: 1, 11: 1, 12: 2}      # output ports per module type


def workloads():
    import srack_pkg
    return srack_pkg.load_workloads()


def is_state(W, mtype, field):
    """graph.cpp, Graph::field_is_state, from the W constants"""
    return field in H.state_fields(W, mtype)


def is_loaded(W, mtype, field):
    """What `apply` writes: the state fields, and a sample player's wavebox.new — no state field (it is consumed by the first tick,
    sample.rs:199-203), but a player that has run starts its next render without it; written after build(), so after set_wave"""
    return is_state(W, mtype, field) or (mtype == W.MOD_SAMPLE and field == W.SAMPLE_WAVE_NEW)


# ---- harvest and apply -----------------------------------------------------------------------------------------------------------------
def harvest(o, types):
    """-> ({(m, f): value} of ALL fields, {(m, port): block} of ALL ports) of an oracle patch"""
    fields = {(m, f): o.get_field(m, f) for m, t in enumerate(types) for f in range(N_FIELDS[t])}
    blocks = {(m, port): o.get_output(m, port) for m, t in enumerate(types) for port in range(N_PORTS[t])}
    return fields, blocks


def apply(g, types, fields, blocks, zero_blocks=False):
    """The harvest into a freshly built OraclePatch or Patch `g`: state fields only (is_loaded), every port's block"""
    W = workloads()
    for (m, f), v in sorted(fields.items()):
        if is_loaded(W, types[m], f):
            g.set_field(m, f, v)
    for (m, port), blk in sorted(blocks.items()):
        g.set_output_buffer(m, port, np.zeros_like(blk) if zero_blocks else blk)


def module_types(build):
    """the module types in the order build() adds them (the OutputModule included)"""
    class Recorder:
        def __init__(self):
            self.types = []

        def add_module(self, t):
            self.types.append(t)
            return len(self.types) - 1

        def __getattr__(self, name):   # connect, set_field, set_step, set_wave, set_noise_seed, disconnect: nothing to record
            return lambda *a, **k: None
    rec = Recorder()
    build(rec)
    return tuple(rec.types)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
class Warm(NamedTuple):
    name: str
    B: int
    V: int
    T: int
    T0: int
    build: object      # build(g): for the product's Patch and the oracle's OraclePatch alike
    types: tuple
    params: tuple      # the family's per-voice parameter overrides ((module, field, values[V]), ...)
    fields: dict       # the patch-level harvest: {(m, f): value} (all fields; `apply` picks the loaded ones)
    blocks: dict       # {(m, port): block}
    voice_state: tuple  # route "voices": ((module, field, values[V]), ...) — the state fields whose harvest differs between voices
    noise_seed: object  # (seed, first voice) or None: no part of a rack file, set again behind a load

    @property
    def overrides(self):
        return list(self.params) + list(self.voice_state)


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def draw(family, seed):
    """-> (B, build, overrides) of tests/fuzz_patches.py, the NonLinear family through FUZZ_NONLIN"""
    from tests.fuzz_patches import random_patch
    with _env(FUZZ_NONLIN="1" if family == "nonlin" else None):
        return random_patch(seed, family == "noise")


def warm_up_samples(B):
    return B * -(-1500 // B)


def _oracle(B, build):
    """-> (a freshly built OraclePatch, what build() returned: the modules' indices)"""
    from oracle import oracle as O
    o = O.OraclePatch(48000, B, 2)
    return o, build(o)


def _warm(name, B, V, T, build, params, route, noise_seed=None):
    W = workloads()
    types = module_types(build)
    T0 = warm_up_samples(B)
    proto, _ = _oracle(B, build)
    if route == "common":
        proto.render(T0)
        fields, blocks = harvest(proto, types)
        return Warm(name, B, V, T, T0, build, types, tuple(params), fields, blocks, (), noise_seed)
    per_voice = []
    for v in range(V):
        o = proto.clone()
        for m, f, vals in params:
            o.set_field(m, f, float(vals[v]))
        o.render(T0)
        per_voice.append(harvest(o, types))
    fields, blocks = per_voice[0]
    voice_state = []
    for (m, f) in sorted(fields):
        if not is_state(W, types[m], f):
            continue
        vals = np.array([pv[0][(m, f)] for pv in per_voice], dtype=np.float64)
        if not H.same_bits(vals, np.full_like(vals, vals[0])).all():
            voice_state.append((m, f, vals if (types[m], f) == (W.MOD_OSCILLATOR, W.OSC_POS) else vals.astype(np.float32)))
    return Warm(name, B, V, T, T0, build, types, tuple(params), fields, blocks, tuple(voice_state), noise_seed)


@functools.lru_cache(maxsize=8)
def fuzz_case(family, seed, route):
    B, build, overrides = draw(family, seed)
    V, T = (67, 1300) if B < 1024 else (131, 2300)   # as tests/test_gpu_fuzz.py
    _, ids = _oracle(B, build)
    params = [(ids[m], f, fn(V)) for m, f, fn in overrides]   # drawn once: the generators are stateful
    return _warm(f"{family}-{seed}-{route}", B, V, T, build, params, route, (seed * 7919 + 1, 1000 * seed) if family == "noise" else None)


# the named patches of tests/handoff_ref.py at its 70 voices, on the "voices" route: (patch, buffer_size, samples, flags).  Every hand-matched
# kernel has a prologue of its own; the time-parallel FM pairs take calls of 4 096 samples and more.  Every call ends on a block boundary.
NAMED = [("p1", 1024, 2048, f) for f in (0, 1, 5, 3, 35)] + [("p1_poly", 1024, 2048, f) for f in (0, 1)] + \
        [("p3", 1024, 2048, f) for f in (0, 1, 33)] + [("p4", 1024, 2048, f) for f in (0, 1, 33)] + \
        [("p2", 1, 1300, f) for f in (1, 0, 64, 3)] + [("p2", 64, 1344, f) for f in (1, 64, 0)] + \
        [("p2", 1024, 2048, f) for f in (1, 64)] + [("p2", 1024, 5120, f) for f in (64, 0)]
NAMED_KERNELS = ("render_voice_chain_track", "render_voice_chain", "render_voice_chain_seq", "render_fm_pair", "render_fm_pair_x",
                 "render_fm_pair_ring", "render_fm_pair_block", "render_fm_pair_block_x", "render_interp", "render_specialized")


def named_kernel(patch, B, T, flags):
    return H.kernel_name(patch, B, H.V, flags, T)


@functools.lru_cache(maxsize=None)
def named_case(patch, B, T):
    import srack_pkg
    sp = H.spec(srack_pkg.load_workloads(), patch, B, H.V)
    _, ids = _oracle(sp.B, sp.build)
    return _warm(f"{patch}-B{sp.B}-T{T}", sp.B, H.V, T, sp.build, sp.overrides(ids), "voices"), ids


# ---- references ------------------------------------------------------------------------------------------------------------------------
def fresh_oracle(w, how="warm"):
    """A fresh OraclePatch with the harvest applied.  how: "warm" (the reference), "noblocks" (the state loaded, every block zeros —
    what a library that ignores the saved blocks renders), "cold" (nothing loaded: what the rest of the suite starts from)"""
    o, _ = _oracle(w.B, w.build)
    if how != "cold":
        apply(o, w.types, w.fields, w.blocks, zero_blocks=how == "noblocks")
    return o


def reference(w, how="warm", voices=None, T=None):
    """-> [C][T][V] f32 (read-only): fresh.render_batch(V, T, overrides).  `voices`: only these (the guards look at voice 0)"""
    ov = w.overrides if how != "cold" else list(w.params)
    n = w.V
    if voices is not None:
        assert list(voices) == list(range(len(voices))), "the noise streams are keyed by the voice's index: a prefix of the voices"
        n, ov = len(voices), [(m, f, np.asarray(vals)[:len(voices)]) for m, f, vals in ov]
    ref, _ = fresh_oracle(w, how).render_batch(n, T or w.T, ov, threads=8)
    ref.flags.writeable = False
    return ref


def final_state(w, voices):
    """{(m, f): {voice: value}} of the state fields after w.T samples (a multiple of buffer_size), one stateful fresh oracle per voice"""
    assert w.T % w.B == 0
    W = workloads()
    out = {}
    for v in voices:
        o = fresh_oracle(w)
        for m, f, vals in w.overrides:
            o.set_field(m, f, float(vals[v]))
        o.render(w.T)
        for m, t in enumerate(w.types):
            for f in H.state_fields(W, t):
                out.setdefault((m, f), {})[v] = o.get_field(m, f)
    return out


# ---- the library's side ----------------------------------------------------------------------------------------------------------------
def through_a_file(S, p, w):
    """load_srk(load_srk(p.save_srk()).save_srk()): a load reverses the module order, two loads restore it"""
    q = S.Patch.load_srk(S.Patch.load_srk(p.save_srk(), 48000, w.B, 2).save_srk(), 48000, w.B, 2)
    if w.noise_seed:
        q.set_noise_seed(*w.noise_seed)
    return q


def make_patch(S, w, via_file, voices=True):
    """The library's Patch with the harvest loaded — through the graph API, or through a rack file loaded twice — and the voices set up"""
    p = S.Patch(48000, w.B, 2)
    w.build(p)
    apply(p, w.types, w.fields, w.blocks)
    if via_file:
        p = through_a_file(S, p, w)
    if voices:
        p.configure_voices(w.V)
        for m, f, vals in w.overrides:
            p.set_voice_field(m, f, vals)
    return p


def loaded_state(w):
    """[(m, f, values[V])] of every loaded state field as the voices hold it before the first render"""
    W = workloads()
    per_voice = {(m, f): np.asarray(vals, dtype=np.float64) for m, f, vals in w.voice_state}
    return [(m, f, per_voice.get((m, f), np.full(w.V, w.fields[(m, f)]))) for (m, f) in sorted(w.fields) if is_state(W, w.types[m], f)]


# ---- the checker -----------------------------------------------------------------------------------------------------------------------
TOL = 1e-5


def contract_error(got, ref):
    """-> (largest |gpu - ref| / max(|ref|, 1) over the finite samples, non-finite positions and signs equal): the project's contract as
    tests/test_gpu_fuzz.py's default modes hold it"""
    got, ref = np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    masks = bool((np.isnan(got) == np.isnan(ref)).all() and (np.isinf(got) == np.isinf(ref)).all()
                 and (np.sign(got[np.isinf(got)]) == np.sign(ref[np.isinf(ref)])).all())
    ok = np.isfinite(ref) & np.isfinite(got)
    r64 = ref.astype(np.float64)[ok]
    err = np.abs(got.astype(np.float64)[ok] - r64) / np.maximum(np.abs(r64), 1.0)
    return (float(err.max()) if err.size else 0.0), masks


def check(got, ref, exact, what=""):
    """`got` [C][T][V] against `ref`: bit for bit (a NaN equal to a NaN) in the exact modes, the contract otherwise.  -> the largest
    relative error (0.0 in bit mode)"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if exact:
        same = H.same_bits(np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float32))
        assert same.all(), f"{what}: {int((~same).sum())} of {same.size} samples differ in their bits, the first at {np.unravel_index((~same).argmax(), same.shape)}"
        return 0.0
    err, masks = contract_error(got, ref)
    assert err <= TOL and masks, f"{what}: max rel err {err:.2e}, non-finite positions and signs equal: {masks}"
    return err


def max_diff(a, b):
    """largest |a - b|; equal bits (inf and inf, NaN and NaN) count as 0, a NaN or an infinity on one side only as infinite"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d = np.nan_to_num(np.abs(a - b), nan=np.inf)
    return float(np.where(H.same_bits(a, b), 0.0, d).max())
