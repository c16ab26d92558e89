"""Kernel hand-offs (notes/r26.md): one running patch, another kernel on the next call.  The case table, the patch makers, the oracle
references and the checker that tests/test_gpu_handoff.py (on the device) and tests/test_handoff_host.py (the guards, on the oracle
alone) share.

A case is a patch and a script of operations:
    ("r", n_samples, flags, mix)   one srack_render call (mix False: frames only — another instantiation / compilation of the kernel)
    ("e",)                         the patch's edit: a per-voice field on a module that was voice-invariant until then
Part A scripts change only the launch-policy bits (16, 32), the call's length or its output mode: the program is flattened once and a
different kernel loads the state the last one stored.  Part B scripts run under srack_patch_keep_state and change the bits that
re-flatten (1, 2, 4, 8, 64) or apply the edit: the state is read back, carried into another program, and rings / reverb lines are
transplanted device to device.

Routes (the issue's numbering, notes/r26.md):  1 launch-policy flags, 2 the call's length, 3 a flags change under keep_state,
4 transplant()'s "the module changed sides" branch.
"""
import functools
from typing import NamedTuple

import numpy as np

EXACT, NO_FUSION, NO_HOIST, ONE_UNIT, NO_SPEC, SPEC, KEEP = 1, 2, 4, 8, 16, 32, 64
REFLATTEN = EXACT | NO_FUSION | NO_HOIST | ONE_UNIT | KEEP   # the bits that are part of a program's identity (render.hip, program_current)
V = 70                             # a full wave and a ragged one; two full 32-voice FM workgroups and a ragged one
SAMPLED = (0, 31, 32, 63, 64, 69)  # the voices a stateful oracle is kept for
FM_BLOCK_MIN = 4096                # the shortest call the time-parallel FM pairs take (render.hip, Knobs::fm_block_min)
GUARD_DIFF, GUARD_PEAK = 1e-2, 0.25


# ---- patches ---------------------------------------------------------------------------------------------------------------------------
class Spec(NamedTuple):
    B: int
    build: object       # build(g) -> ids, for the product's Patch and the oracle's OraclePatch alike
    overrides: object   # overrides(ids) -> [(module, field, f32[V])]
    edit: object        # edit(ids) -> (module, field, f32[V]) or None


def _p2_reverb_build(S):
    def build(g):   # as tests/test_gpu_parity.py::test_keep_state_carries_feedback_rings_and_reverb_lines builds it
        ids = S.build_p2(g, beta=0.25, index=0.8)
        fv = g.add_module(S.MOD_FREEVERB)
        g.disconnect(ids["out"], 1)
        g.connect(ids["osc_c"], S.OSC_OUT_SINE, fv, 0)
        g.connect(fv, 1, ids["out"], 1)      # channel 1 through a reverb
        return dict(ids, fv=fv)
    return build


def _loop_build(S):
    def build(g):   # x[t] = 0.998 * x[t - B] + 0.02 (still rising after 192 blocks) through two stateless modules: all the patch holds is the ring of the delayed edge
        add, mul, out = g.add_module(S.MOD_MATH), g.add_module(S.MOD_MATH), g.add_module(S.MOD_OUTPUT)
        for m, op, c in ((add, S.MATH_ADD, 0.02), (mul, S.MATH_MULTIPLY, 0.998)):
            g.set_field(m, S.MATH_OPERATION, op)
            g.set_field(m, S.MATH_CONSTANT, c)
        g.connect(add, 0, mul, 0)
        g.connect(mul, 0, add, 0)
        g.connect(add, 0, out, 0)
        g.connect(mul, 0, out, 1)
        return dict(add=add, mul=mul, out=out)
    return build


def spec(S, name, B=None, n_voices=V):
    f = np.float32
    if name == "loop":
        return Spec(B, _loop_build(S), lambda ids: [], None)
    if name == "p1":
        det, cut = S.p1_voice_params(n_voices)
        return Spec(B or 1024, lambda g: S.build_p1(g, adsr="finite", lfo_val=-3.0),
                    lambda ids: [(ids["osc_a"], S.OSC_VAL, det), (ids["vcf"], S.VCF_FREQ, cut)],
                    lambda ids: (ids["osc_lfo"], S.OSC_VAL, np.linspace(-3.5, -2.0, n_voices).astype(f)))
    if name == "p1_poly":   # cfg3_poly's draw with the gate LFO five octaves up (55 - 440 Hz): nothing voice-invariant, every voice busy within a few hundred samples
        pv = dict(S.p1_poly_voice_params(n_voices))
        pv["lfo_val"] = (pv["lfo_val"] + f(5.0)).astype(f)
        return Spec(B or 1024, lambda g: S.build_p1(g, adsr="finite", lfo_val=-3.0), lambda ids: S.p1_poly_overrides(ids, pv), None)
    if name in ("p3", "p4"):
        B2, build, overrides = S.bench_workload(name, n_voices)
        return Spec(B2, build, overrides, None)
    if name in ("p2", "p2_flat"):
        beta, index = S.p2_voice_params(n_voices)
        if name == "p2":
            return Spec(B, S.build_p2, lambda ids: [(ids["mul_fb"], S.MATH_CONSTANT, beta), (ids["mul_idx"], S.MATH_CONSTANT, index)], None)
        return Spec(B, S.build_p2, lambda ids: [], lambda ids: (ids["mul_fb"], S.MATH_CONSTANT, beta))   # the whole patch voice-invariant until the edit
    if name in ("p2_reverb", "p2_reverb_flat"):
        fb, pitch = np.linspace(0.0, 0.5, n_voices).astype(f), np.linspace(-1.0, 1.0, n_voices).astype(f)
        if name == "p2_reverb":
            return Spec(B or 64, _p2_reverb_build(S), lambda ids: [(ids["mul_fb"], S.MATH_CONSTANT, fb), (ids["osc_c"], S.OSC_VAL, pitch)], None)
        return Spec(B or 64, _p2_reverb_build(S), lambda ids: [], lambda ids: (ids["mul_fb"], S.MATH_CONSTANT, np.linspace(0.05, 0.5, n_voices).astype(f)))
    raise ValueError(name)


def make_patch(S, name, B, n_voices=V, keep=False):
    sp = spec(S, name, B, n_voices)
    p = S.Patch(48000, sp.B, 2)
    ids = sp.build(p)
    p.configure_voices(n_voices)
    for m, f, vals in sp.overrides(ids):
        p.set_voice_field(m, f, vals)
    if keep:
        p.keep_state(True)
    return p, ids, sp


def state_fields(S, mtype):
    """The state fields of a module type (graph.cpp, Graph::field_is_state): what test_state_carried_across_an_edit_by_hand lists, plus the
    sequencers' and the sample player's."""
    return {S.MOD_OSCILLATOR: [S.OSC_POS, S.OSC_SYNC_LAST], S.MOD_MOOG_FILTER: list(range(S.VCF_ST_F, S.VCF_ST_RES + 1)),
            S.MOD_ADSR: [S.ADSR_PHASE, S.ADSR_MODE, S.ADSR_R_VAL, S.ADSR_FROM_A_VAL, S.ADSR_GATE_LAST],
            S.MOD_GRID_SEQUENCER: [S.GRIDSEQ_CURRENT_STEP, S.GRIDSEQ_STEP_LAST, S.GRIDSEQ_SYNC_LAST, S.GRIDSEQ_LAST],
            S.MOD_PATTERN_SEQUENCER: [S.PATSEQ_CURRENT_STEP, S.PATSEQ_STEP_LAST, S.PATSEQ_SYNC_LAST],
            S.MOD_SAMPLE: [S.SAMPLE_POS, S.SAMPLE_PLAYING, S.SAMPLE_GATE_LAST]}.get(mtype, [])


# ---- which kernel a call takes: DESIGN.md section 4 (render.hip, pick_kernel / resolve_specialized) for these patches -------------------
def kernel_name(patch, B, n_voices, flags, n_samples, edited=False):
    """The name srack_render_info gives the call.  Where tests/test_gpu_kernel_choice.py's table has the shape, its name; the others as
    observed on the device (notes/r26.md).  `edited`: the modules the control program evaluated are per voice by now — the patch's edit
    has been applied, or (keep_state) an earlier call ran them per voice (NO_UNIFORM_HOIST): their carried state stays a per-voice override,
    so p1 renders through render_voice_chain from then on, not through the flagship."""
    exact, general, nohoist, keep = flags & EXACT, flags & NO_FUSION, flags & NO_HOIST, flags & KEEP
    special = bool(flags & SPEC) or (n_voices >= 4096 and not flags & NO_SPEC)   # ... for a program that is a candidate
    if patch in ("p2_reverb", "p2_reverb_flat", "loop"):
        return "render_interp"   # the reverb is the interpreter's: no fused shape, no generated kernel; the loop has no voice kernel to fuse
    if patch in ("p1", "p1_poly", "p3"):
        if general:
            return "render_specialized" if special else "render_interp"
        if patch == "p1" and not nohoist and not edited:
            return "render_voice_chain_track"   # the flagship keeps its hand-written form
        if patch == "p3" and (exact or nohoist):
            return "render_specialized" if special else "render_interp"   # the sequencer chain is default mode's, with its clock hoisted
        return "render_specialized" if special else ("render_voice_chain_seq" if patch == "p3" else "render_voice_chain")
    if patch == "p4":
        return "render_specialized" if special else "render_interp"
    assert patch in ("p2", "p2_flat"), patch
    if patch == "p2_flat" and not edited and not nohoist:
        return "render_interp"   # everything in the control program: the voice program only copies its tracks
    blk = n_samples >= FM_BLOCK_MIN and not exact and not general and B <= 1024
    if general:
        return "render_specialized" if special else "render_interp"
    if not exact and not keep:   # default mode: the modulator exact as a whole, kernels of its own
        if flags & SPEC:
            return "render_specialized"
        if B == 1:
            return "render_fm_pair_x"
        if blk and B >= 256:
            return "render_fm_pair_block_x"
        return "render_specialized" if special else "render_interp"
    if B == 1:   # the z^-1 pair: a candidate in default arithmetic only (the exact two-wave split keeps its hand-written form)
        return "render_specialized" if special and not exact else "render_fm_pair"
    if B < 32:
        return "render_specialized" if special else "render_interp"
    return "render_fm_pair_block" if blk and B >= 256 else "render_fm_pair_ring"   # (launch_types.hpp, kBlkChunk: the time-parallel pair's chunk is 256 samples)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    id: str
    part: str        # "A": one program, another kernel per call.  "B": keep_state, a re-flatten with a carry.
    patch: str
    B: int
    V: int
    ops: tuple
    routes: tuple
    state_from: int = 0   # state is read back after call `state_from` and later (a read-back ends a tick session: the ticked case reads behind it)


def r(n, flags, mix=True):
    return ("r", n, flags, mix)


def _modes(name, patch, B, script, routes, exact=True, n_voices=V, **kw):
    """a script written with base flags f = 0 in default mode and, where it keeps its meaning, with every call | 1"""
    out = [Case(name, "A", patch, B, n_voices, tuple(script), routes, **kw)]
    if exact:
        out.append(Case(name + "-exact", "A", patch, B, n_voices, tuple(("r", n, f | EXACT, m) for _, n, f, m in script), routes, **kw))
    return out


def _part_a():
    c = []
    swap = lambda f, g: ([r(700, f), r(900, g), r(448, f)], [r(700, g), r(900, f), r(448, g)])
    for patch, f in (("p1_poly", 0), ("p3", 0), ("p1", NO_FUSION), ("p4", NO_FUSION), ("p4", 0)):
        a, b = swap(f, f | SPEC)
        c += _modes(f"{patch}-f{f}-special", patch, None, a, (1,)) + _modes(f"{patch}-f{f}-special-rev", patch, None, b, (1,))
    a, b = swap(KEEP, KEEP | SPEC)   # the z^-1 FM pair in default arithmetic: render_fm_pair <-> the generated kernel
    c += _modes("p2-B1-keep-special", "p2", 1, a, (1,), exact=False) + _modes("p2-B1-keep-special-rev", "p2", 1, b, (1,), exact=False)
    # the exact z^-1 pair (the two-wave split) is no candidate for a generated kernel: flags 1 | 32 renders through render_fm_pair again
    # (observed, notes/r26.md).  In its place: the exact pair through the general path, render_interp <-> render_specialized
    a, b = swap(EXACT | NO_FUSION, EXACT | NO_FUSION | SPEC)
    c += _modes("p2-B1-exact-general-special", "p2", 1, a, (1,), exact=False) + _modes("p2-B1-exact-general-special-rev", "p2", 1, b, (1,), exact=False)
    a, b = swap(0, SPEC)             # default mode: render_fm_pair_x <-> the generated kernel
    c += _modes("p2-B1-default-special", "p2", 1, a, (1,), exact=False) + _modes("p2-B1-default-special-rev", "p2", 1, b, (1,), exact=False)
    for B in (256, 1024):            # the call's length alone: ring <-> block (KEEP_DEFAULT), interpreter <-> block_x (default)
        for f, tag in ((KEEP, "keep"), (0, "default")):
            c += _modes(f"p2-B{B}-{tag}-short-long-short", "p2", B, [r(3072, f), r(5120, f), r(3072, f)], (2,), exact=False)
            c += _modes(f"p2-B{B}-{tag}-long-short-long", "p2", B, [r(5120, f), r(3072, f), r(4096, f)], (2,), exact=False)
            c += _modes(f"p2-B{B}-{tag}-ragged", "p2", B, [r(3000, f), r(4097, f), r(1001, f)], (2,), exact=False)   # the ring cursor mid-block at both hand-offs
        c += _modes(f"p2-B{B}-default-through-special", "p2", B, [r(3072, 0), r(3072, SPEC), r(5120, 0), r(2048, SPEC)], (1, 2), exact=False)
    # the middle call writes frames only: another instantiation (compilation) on the same table
    c += _modes("p1_poly-frames-only", "p1_poly", None, [r(700, 0), r(900, SPEC, False), r(448, 0)], (1,))
    c += _modes("p2-B1024-frames-only", "p2", 1024, [r(3072, KEEP), r(5120, KEEP, False), r(3072, KEEP)], (2,), exact=False)
    # the dispatcher's own choice from 4096 voices up, against render_voice_chain.  Calls of 1024 samples: with the 96 the issue proposed,
    # 4 144 of the 4 160 voices peak below 0.25 in the second call and 2 418 render what a restart renders (attack and filter lag), so the
    # guard every script has to meet (tests/test_handoff_host.py) does not hold; 1024 is the shortest power of two at which it does
    c += _modes("p1_poly-wide", "p1_poly", None, [r(1024, 0), r(1024, NO_SPEC), r(1024, 0)], (1,), n_voices=4160)
    # a tick session of three calls, one call through the interpreter, back
    g = NO_FUSION
    c += _modes("p1-ticked", "p1", None, [r(1024, g | SPEC)] * 3 + [r(1024, g | NO_SPEC), r(1024, g | SPEC)], (1,), state_from=2)
    return c


def _flag_script(seq, lens):
    return tuple(r(n, f) for n, f in zip(lens, seq))


def _both_ways(seq):
    seq = list(seq)
    back = seq[::-1] if seq[::-1] != seq else [seq[1], seq[0], seq[1]]   # a -> b -> a reversed is itself: b -> a -> b
    return seq, back


def _part_b():
    c = []
    def add(patch, B, seqs, lens):
        for seq in seqs:
            for s2 in _both_ways(seq):
                if any(k.patch == patch and k.B == B and [op[2] for op in k.ops] == s2 for k in c):
                    continue   # (1 -> 0 -> 1 is 0 -> 1 -> 0 reversed)
                c.append(Case(f"{patch}-B{B}-keep-" + "-".join(map(str, s2)), "B", patch, B, V, _flag_script(s2, lens), (3,)))
    add("p1", 64, [(1, 5, 1), (1, 3, 1), (1, 35, 1), (9, 1), (0, 4, 0), (0, 2, 0), (0, 34), (1, 0, 1), (0, 1, 0)], (1536, 1024, 1088))
    for patch in ("p3", "p4"):
        add(patch, 1024, [(1, 3, 35, 1), (0, 1, 0)], (1024, 2048, 1024, 1024))
    for B in (1, 8, 64, 1024):   # the ring: a state row up to buffer_size 16, in HBM above
        add("p2", B, [(1, 3, 1), (1, 35), (64, 0, 64), (0, 1, 0)], (2048, 1024, 2048) if B == 1024 else (1536, 1024, 1088))
    add("p2_reverb", 64, [(1, 3, 1), (0, 2, 0)], (1536, 1024, 1088))
    # Per voice -> voice-invariant: a stateful module never goes back (its carried state stays a per-voice override), but a loop of stateless
    # modules does — everything per voice under NO_UNIFORM_HOIST, in the control program without it — and its ring with it: transplant()'s
    # copy of voice 0 (4 -> 0, 5 -> 1) and its broadcast (0 -> 4, 1 -> 5); a state row of the table at buffer_size 8, a ring in HBM at 64
    for B in (8, 64):
        for seq in ((4, 0, 4), (0, 4, 0), (5, 1, 5), (1, 5, 1)):
            c.append(Case(f"loop-B{B}-keep-" + "-".join(map(str, seq)), "B", "loop", B, V, _flag_script(seq, (1536, 1024, 1088)), (3, 4)))
    # an edit that moves modules from the control program into the voice program, flags unchanged
    for f in (1, 3, 0):
        c.append(Case(f"p1-B64-edit-f{f}", "B", "p1", 64, V, (r(1536, f), ("e",), r(1088, f)), (3,)))
        for B in (8, 64):
            c.append(Case(f"p2_flat-B{B}-edit-f{f}", "B", "p2_flat", B, V, (r(1536, f), ("e",), r(1088, f)), (3, 4)))
        c.append(Case(f"p2_reverb_flat-B64-edit-f{f}", "B", "p2_reverb_flat", 64, V, (r(1536, f), ("e",), r(1088, f)), (3, 4)))
    return c


CASES = _part_a() + _part_b()
CASES_A = [k for k in CASES if k.part == "A"]
CASES_B = [k for k in CASES if k.part == "B"]


def renders(case):
    """-> [(op index, first sample, n_samples, flags, mix, edited)] of the case's render calls"""
    out, t, edited = [], 0, False
    for i, op in enumerate(case.ops):
        if op[0] == "e":
            edited = True
            continue
        out.append((i, t, op[1], op[2], op[3], edited))
        edited = edited or (case.part == "B" and bool(op[2] & NO_HOIST))
        t += op[1]
    return out


def total(case):
    return sum(op[1] for op in case.ops if op[0] == "r")


def has_edit(case):
    return any(op[0] == "e" for op in case.ops)


def kernels(case):
    return [kernel_name(case.patch, spec_B(case), case.V, f, n, ed) for _, _, n, f, _, ed in renders(case)]


def spec_B(case):
    return case.B or 1024


def all_exact(case, upto=None):
    """every render call up to and including op `upto` in exact mode: held to the oracle bit for bit"""
    return all(op[2] & EXACT for op in case.ops[:None if upto is None else upto + 1] if op[0] == "r")


def modulator_exact(case, upto):
    """p2's modulator is exact in default mode too (approx.cpp: a loop through a pitch), so its phase is the oracle's bit for bit after
    default-mode calls as well — as long as no call so far kept the default forms (64) or took the general path's flattening (2, 4, 8)"""
    return case.patch == "p2" and all(op[2] & EXACT or not op[2] & REFLATTEN for op in case.ops[:upto + 1] if op[0] == "r")


# ---- references: the project's own oracle ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _whole(patch, B, n_voices, T):
    import srack_pkg
    from oracle import oracle as O
    S = srack_pkg.load_workloads()
    sp = spec(S, patch, B, n_voices)
    o = O.OraclePatch(48000, sp.B, 2)
    ids = sp.build(o)
    ref, _ = o.render_batch(n_voices, T, sp.overrides(ids), threads=8)
    ref.flags.writeable = False
    return ref


def _voice_oracle(S, O, sp, v):
    o = O.OraclePatch(48000, sp.B, 2)
    ids = sp.build(o)
    for m, f, vals in sp.overrides(ids):
        o.set_field(m, f, float(vals[v]))
    return o, ids


@functools.lru_cache(maxsize=None)
def _edited(patch, B, ops):
    """An edit script on one stateful OraclePatch per sampled voice: render, set_field with that voice's value, render.
    -> ({voice: [C][T]}, {voice: [C][T2] restarted: a fresh patch with the edit applied})"""
    import srack_pkg
    from oracle import oracle as O
    S = srack_pkg.load_workloads()
    sp = spec(S, patch, B, V)
    cont, fresh = {}, {}
    for v in SAMPLED:
        o, ids = _voice_oracle(S, O, sp, v)
        m, f, vals = sp.edit(ids)
        parts = []
        for op in ops:
            if op[0] == "e":
                o.set_field(m, f, float(vals[v]))
                q, _ = _voice_oracle(S, O, sp, v)
                q.set_field(m, f, float(vals[v]))
                fresh[v] = q.render(sum(x[1] for x in ops[ops.index(op) + 1:] if x[0] == "r"))
            else:
                assert op[1] % sp.B == 0, "the oracle ticks in blocks: an edit script is cut at multiples of buffer_size"
                parts.append(o.render(op[1]))
        cont[v] = np.concatenate(parts, axis=1)
    return cont, fresh


def reference(case):
    """-> (ref [C][T][voices], voices): a flags-only script changes nothing audible — one uninterrupted render_batch of its whole length,
    every voice; an edit script — the stateful oracles of the sampled voices"""
    if not has_edit(case):
        return _whole(case.patch, case.B, case.V, total(case)), np.arange(case.V)
    cont, _ = _edited(case.patch, case.B, case.ops)
    return np.stack([cont[v] for v in SAMPLED], axis=2), np.array(SAMPLED)


def restarted(case, cut):
    """What the calls after sample `cut` would give had the voices restarted there from the state stored in the patch (what a re-flatten
    without a carry does, and what a kernel does that does not find the last one's state): the same voices as reference()."""
    ref, voices = reference(case)
    if not has_edit(case):
        return ref[:, :ref.shape[1] - cut]          # a fresh render IS the start of the whole one
    _, fresh = _edited(case.patch, case.B, case.ops)
    T_e = sum(op[1] for op in case.ops[:[op[0] for op in case.ops].index("e")])
    assert cut == T_e, "an edit script has one cut that is guarded: the edit"
    return np.stack([fresh[v] for v in SAMPLED], axis=2)


def oracle_state(case, upto):
    """{(module, field): {voice: value}} of the stateful oracle after op `upto` (a render that ends on a multiple of buffer_size), for the
    sampled voices; the ops replayed on a fresh OraclePatch per voice (neighbouring renders as one: the oracle ticks in blocks)"""
    import srack_pkg
    from oracle import oracle as O
    S = srack_pkg.load_workloads()
    sp = spec(S, case.patch, case.B, case.V)
    out = {}
    for v in SAMPLED:
        o, ids = _voice_oracle(S, O, sp, v)
        pending = 0
        for op in case.ops[:upto + 1]:
            if op[0] == "r":
                pending += op[1]
                continue
            assert pending % sp.B == 0
            if pending:
                o.render(pending)
            pending = 0
            m, f, vals = sp.edit(ids)
            o.set_field(m, f, float(vals[v]))
        assert pending % sp.B == 0
        if pending:
            o.render(pending)
        for m in range(o.num_modules()):
            for f in state_fields(S, _module_types(case.patch, case.B)[m]):
                out.setdefault((m, f), {})[v] = o.get_field(m, f)
    return out


@functools.lru_cache(maxsize=None)
def _module_types(patch, B):
    import srack_pkg
    S = srack_pkg.load_workloads()

    class Recorder:
        def __init__(self):
            self.types = []

        def add_module(self, t):
            self.types.append(t)
            return len(self.types) - 1

        def __getattr__(self, name):   # connect, set_field, set_step, set_wave, disconnect: nothing to record
            return lambda *a, **k: None
    rec = Recorder()
    spec(S, patch, B, V).build(rec)
    return tuple(rec.types)


# ---- the checker -----------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """bit for bit, a NaN equal to a NaN (x86's default NaN is 0xffc00000, the GPU's 0x7fc00000: tests/test_gpu_fuzz.py)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))


def rel_err(got, ref):
    """the contract's measure (tests/test_gpu_parity.py, assert_close): |gpu - ref| / max(|ref|, 1), its maximum"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)).max())


def check(got, ref, exact, what=""):
    """`got` [C][T][voices] against `ref`: bit for bit where every call so far was exact, through the suite's contract (1e-5 relative to
    max(|ref|, 1)) otherwise.  -> the largest relative error (0.0 in bit mode)."""
    from tests.test_gpu_parity import assert_close
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if exact:
        same = same_bits(np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float32))
        assert same.all(), f"{what}: {int((~same).sum())} of {same.size} samples differ in their bits, the first at {np.unravel_index((~same).argmax(), same.shape)}"
        return 0.0
    try:
        return assert_close(got, ref)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None


def guard_figures(case):
    """For every cut of the script: the smallest, over the voices, of the largest difference between the reference after the cut and the
    reference restarted there (over the samples of the next call), and the smallest per-voice peak of that call.  A hand-off that loses the
    state shows only where these are large.  -> [(cut, min diff, min peak)]"""
    ref, _ = reference(case)
    out = []
    for _, t0, n, _, _, _ in renders(case)[1:]:
        cont = ref[:, t0:t0 + n].astype(np.float64)
        again = restarted(case, t0)[:, :n].astype(np.float64)
        diff = np.nan_to_num(np.abs(cont - again), nan=np.inf).max(axis=(0, 1))
        peak = np.nan_to_num(np.abs(cont), nan=np.inf).max(axis=(0, 1))
        out.append((t0, float(diff.min()), float(peak.min())))
    return out
