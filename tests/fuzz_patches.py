"""Random patches for differential tests (tests/test_gpu_fuzz.py and tests/test_gpu_banked_fuzz.py: GPU vs oracle; tests/test_oracle.py and
tests/test_banked_fuzz_host.py: C oracle vs NumPy twin)."""
import numpy as np

import srack_pkg

W = srack_pkg.load_workloads()

OSC, VCF, ADSR, VCA, MIX, MATH, GRID, PAT, NONLIN, SMP, NOISE, VERB = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12
N_IN = {OSC: 2, VCF: 2, ADSR: 1, VCA: 2, MIX: 4, MATH: 2, GRID: 2, PAT: 2, NONLIN: 2, SMP: 2, NOISE: 0, VERB: 2}
import os
# (FUZZ_SINE=1: tools/fuzz_soak.py also draws the oscillators' sine port)
OUT_PORTS = {OSC: [0, 1, 2] if os.environ.get("FUZZ_SINE") else [1, 2], VCF: [0, 1, 2], ADSR: [0], VCA: [0], MIX: [0], MATH: [0], NONLIN: [0], GRID: [0, 1, 2], PAT: [0, 3, 7, 8], SMP: [0], NOISE: [0], VERB: [0, 1]}


def random_patch(seed, noise=False):
    """-> (B, build(g) -> None, overrides [(module, field, values per voice fn)]).  noise=True: a fifth of the modules are
    NoiseModules and a tenth FreeverbModules (a separate family of patches: the seeds of the first family keep their meaning)."""
    rng = np.random.default_rng(seed if not noise else (seed, 0x4e6f))
    B = int(rng.choice([1, 3, 16, 64, 1024]))
    n = int(rng.integers(4, 11))
    types = [OSC, OSC] + [int(rng.choice([OSC, VCF, ADSR, VCA, MIX, MATH, GRID, PAT, SMP], p=[.2, .15, .12, .13, .1, .15, .05, .05, .05])) for _ in range(n - 2)]
    rng.shuffle(types)
    if noise:
        types = [NOISE if u < 0.2 else VERB if u < 0.3 else t for t, u in zip(types, rng.random(n))]
        if NOISE not in types:
            types[int(rng.integers(0, n))] = NOISE
    fields, steps, conns, waves = [], [], [], []
    for m, t in enumerate(types):
        if t == OSC:
            fields.append((m, W.OSC_VAL, float(np.float32(rng.uniform(-6, 3)))))
            if rng.random() < 0.2:
                fields.append((m, W.OSC_ANTIALIASING, 0))
        elif t == VCF:
            fields += [(m, W.VCF_FREQ, float(np.float32(rng.uniform(0.02, 0.8)))), (m, W.VCF_RES, float(np.float32(rng.uniform(0, 1)))),
                       (m, W.VCF_EXP_AMT, float(np.float32(rng.uniform(0, 1))))]
        elif t == ADSR:
            fields += [(m, f, float(np.float32(v))) for f, v in zip((W.ADSR_A_SEC, W.ADSR_D_SEC, W.ADSR_S_VAL, W.ADSR_R_SEC),
                                                                    (rng.choice([0.0, 0.001, 0.004]), rng.uniform(0.001, 0.01), rng.uniform(0, 1), rng.uniform(0.001, 0.01)))]
        elif t == VCA:
            fields.append((m, W.VCA_NEGATIVE, int(rng.random() < 0.3)))
        elif t == MIX:
            fields += [(m, W.MIX_GAIN0 + k, float(np.float32(rng.uniform(0, 1.2)))) for k in range(4)]
        elif t == MATH:
            fields += [(m, W.MATH_CONSTANT, float(np.float32(rng.uniform(-1, 1)))), (m, W.MATH_OPERATION, int(rng.integers(0, 3)))]
        elif t == VERB:
            fields += [(m, f, float(rng.uniform(lo, hi))) for f, lo, hi in ((W.FREEVERB_DAMPENING, 0, 2), (W.FREEVERB_WET, 0, 1), (W.FREEVERB_WIDTH, 0, 1),
                                                                            (W.FREEVERB_ROOM_SIZE, 0, 1), (W.FREEVERB_DRY, 0, 1))]
            fields.append((m, W.FREEVERB_FREEZE, int(rng.random() < 0.2)))
        elif t == SMP:
            waves.append((m, rng.uniform(-1, 1, int(rng.integers(1, 400))).astype(np.float32), float(rng.choice([8000.0, 44100.0, 48000.0, 96000.0]))))
        elif t in (GRID, PAT):
            length = int(rng.integers(1, 9))
            fields.append((m, W.GRIDSEQ_LENGTH if t == GRID else W.PATSEQ_LENGTH, length))
            for i in range(length):
                for ch in ([0] if t == GRID else [0, 3, 7]):
                    steps.append((m, ch, i, int(rng.integers(0, 3)), int(rng.integers(0, 25))))
    for m, t in enumerate(types):  # wire most inputs to a random output of a random OTHER module (self-loops are rejected)
        for k in range(N_IN[t]):
            if rng.random() < 0.75:
                src = int(rng.integers(0, n - 1))
                src += src >= m
                conns.append((src, int(rng.choice(OUT_PORTS[types[src]])), m, k))
    out_src = [int(rng.integers(0, n)) for _ in range(2)]
    out_conns = [(s, int(rng.choice(OUT_PORTS[types[s]])), c) for c, s in enumerate(out_src) if rng.random() < 0.9]
    if not out_conns:
        out_conns = [(out_src[0], OUT_PORTS[types[out_src[0]]][0], 0)]
    out_pos = int(rng.integers(0, n + 1))  # where the OutputModule sits in all_modules: the planner cares
    if os.environ.get("FUZZ_NONLIN"):  # (tools/cpu_soak.py: half of the MathModules become NonLinearModules — same arity, so the rest of the patch keeps its draw)
        r3 = np.random.default_rng((seed, 0x9))
        for m, t in enumerate(types):
            if t == MATH and r3.random() < 0.5:
                types[m] = NONLIN
                fields = [x for x in fields if x[0] != m] + [(m, W.NONLIN_CONSTANT, float(np.float32(r3.choice([0.5, 2.0, 3.0, r3.uniform(0.3, 3.0)]))))]

    def build(g):
        ids = []
        for i, t in enumerate(types):
            if i == out_pos:
                build.out = g.add_module(0)
            ids.append(g.add_module(t))
        if out_pos == n:
            build.out = g.add_module(0)
        shift = lambda m: ids[m]
        for m, f, v in fields:
            g.set_field(shift(m), f, v)
        for m, ch, i, st, val in steps:
            g.set_step(shift(m), ch, i, st, val)
        for m, wave, rate in waves:
            g.set_wave(shift(m), wave, rate)
        for s, sp, k, kp in conns:
            g.connect(shift(s), sp, shift(k), kp)
        for s, sp, c in out_conns:
            g.connect(shift(s), sp, build.out, c)
        if noise:
            g.set_noise_seed(seed * 7919 + 1, 1000 * seed)
        return ids

    overrides = []
    for m, t in enumerate(types):
        if rng.random() < 0.45:
            if t == OSC:
                overrides.append((m, W.OSC_VAL, lambda V, r=np.random.default_rng(seed * 131 + m): r.uniform(-5, 2, V).astype(np.float32)))
            elif t == VCF:
                overrides.append((m, W.VCF_FREQ, lambda V, r=np.random.default_rng(seed * 131 + m): r.uniform(0.03, 0.7, V).astype(np.float32)))
            elif t == MATH:
                overrides.append((m, W.MATH_CONSTANT, lambda V, r=np.random.default_rng(seed * 131 + m): r.uniform(-1, 1, V).astype(np.float32)))
            elif t == NONLIN:
                overrides.append((m, W.NONLIN_CONSTANT, lambda V, r=np.random.default_rng(seed * 131 + m): r.uniform(0.3, 3.0, V).astype(np.float32)))
            elif t == MIX:
                overrides.append((m, W.MIX_GAIN0 + 1, lambda V, r=np.random.default_rng(seed * 131 + m): r.uniform(0, 1, V).astype(np.float32)))
            elif t == ADSR:
                overrides.append((m, W.ADSR_S_VAL, lambda V, r=np.random.default_rng(seed * 131 + m): r.uniform(0, 1, V).astype(np.float32)))
    if os.environ.get("FUZZ_MORE_OV"):  # (tools/fuzz_soak.py: per-voice overrides of further parameters and of initial STATE)
        r2 = np.random.default_rng((seed, 0x0F))
        more = {OSC: [(W.OSC_POS, 0.0, 1.0)], VCF: [(W.VCF_RES, 0.0, 1.0), (W.VCF_EXP_AMT, 0.0, 1.0), (W.VCF_ST_B2, -1.0, 1.0)],
                ADSR: [(W.ADSR_A_SEC, 0.0, 0.004), (W.ADSR_D_SEC, 0.0005, 0.01), (W.ADSR_R_SEC, 0.0005, 0.01), (W.ADSR_PHASE, 0.0, 1.0)],
                MIX: [(W.MIX_GAIN0, 0.0, 1.0), (W.MIX_GAIN3, -1.0, 1.0)]}
        for m, t in enumerate(types):
            for f, lo_, hi_ in more.get(t, []):
                if r2.random() < 0.35:
                    gen = np.random.default_rng((seed, m, f))
                    if f == W.OSC_POS:
                        overrides.append((m, f, lambda V, g=gen: g.uniform(0.0, 1.0, V)))  # f64 state
                    else:
                        overrides.append((m, f, lambda V, g=gen, a=lo_, b=hi_: g.uniform(a, b, V).astype(np.float32)))
    return B, build, overrides


# ---- the banked family: a wave / a sequence per voice (tests/test_gpu_banked_fuzz.py, tests/test_banked_fuzz_host.py) ----------------
BANK_WAVE_LENGTHS = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257]
BANK_RATES = [8000.0, 22050.0, 44100.0, 48000.0, 96000.0]
BANK_SEQ_LENGTHS = [1, 2, 7, 63, 64]
BANK_AMPLITUDES = [1.0, 1.0, 4.0]   # a bank's samples are uniform in +-a: a third of the banks are louder than any own wave
BANK_NOTE_MAX = 48                  # a bank's grid values are 0 ... 48, the own ones 0 ... 24: the bank's highest note is above the own one


def random_banked_patch(seed):
    """-> (B, build(g) -> ids, overrides, banks, assignments): random_patch's draw (types, fields, wiring rule, cycles, OutputModule anywhere)
    from a stream of its own, with at least one sample player and one sequencer, and a bank on every one of them.

    banks: [{"m", "type": SMP, "waves": [f32 arrays], "rates": [...]} | {"m", "type": GRID | PAT, "states": u8 [n][64] | [n][8][64],
    "values": u16 [n][64] | None, "lengths": int [n]}]; assignments: {m: fn(V, edit=0) -> int32 [V] in [-1, n)} — a bank whose module is
    not a key stays without an assignment; edit > 0 draws the fresh assignment of an edit.  build.types / .conns / .out_conns describe
    the graph to the guards; build.own ({m: (wave, rate) | None}) and build.cells are what build() leaves in the players and sequencers."""
    rng = np.random.default_rng((seed, 0xBA2C))
    B = int(rng.choice([1, 3, 16, 64, 1024]))
    n_smp = 1 if rng.random() < 0.65 else int(rng.integers(2, 4))
    seqs = [GRID, PAT] if rng.random() < 0.35 else [int(rng.choice([GRID, PAT]))]
    forced = [OSC, OSC] + [SMP] * n_smp + seqs
    n = int(rng.integers(max(4, len(forced)), 11))
    types = forced + [int(rng.choice([OSC, VCF, ADSR, VCA, MIX, MATH, GRID, PAT, SMP], p=[.2, .15, .12, .13, .1, .15, .05, .05, .05])) for _ in range(n - len(forced))]
    rng.shuffle(types)
    fields, steps, conns, waves, own = [], [], [], [], {}
    for m, t in enumerate(types):
        if t == OSC:
            fields.append((m, W.OSC_VAL, float(np.float32(rng.uniform(-6, 3)))))
            if rng.random() < 0.2:
                fields.append((m, W.OSC_ANTIALIASING, 0))
        elif t == VCF:
            fields += [(m, W.VCF_FREQ, float(np.float32(rng.uniform(0.02, 0.8)))), (m, W.VCF_RES, float(np.float32(rng.uniform(0, 1)))),
                       (m, W.VCF_EXP_AMT, float(np.float32(rng.uniform(0, 1))))]
        elif t == ADSR:
            fields += [(m, f, float(np.float32(v))) for f, v in zip((W.ADSR_A_SEC, W.ADSR_D_SEC, W.ADSR_S_VAL, W.ADSR_R_SEC),
                                                                    (rng.choice([0.0, 0.001, 0.004]), rng.uniform(0.001, 0.01), rng.uniform(0, 1), rng.uniform(0.001, 0.01)))]
        elif t == VCA:
            fields.append((m, W.VCA_NEGATIVE, int(rng.random() < 0.3)))
        elif t == MIX:
            fields += [(m, W.MIX_GAIN0 + k, float(np.float32(rng.uniform(0, 1.2)))) for k in range(4)]
        elif t == MATH:
            fields += [(m, W.MATH_CONSTANT, float(np.float32(rng.uniform(-1, 1)))), (m, W.MATH_OPERATION, int(rng.integers(0, 3)))]
        elif t == SMP:
            wave, rate = rng.uniform(-1, 1, int(rng.integers(1, 401))).astype(np.float32), float(rng.choice([8000.0, 44100.0, 48000.0, 96000.0]))
            own[m] = None if rng.random() < 0.125 else (wave, rate)   # one in eight: a player nobody loaded a wave into
            if own[m]:
                waves.append((m, wave, rate))
        elif t in (GRID, PAT):
            length = int(rng.integers(1, 9))
            fields.append((m, W.GRIDSEQ_LENGTH if t == GRID else W.PATSEQ_LENGTH, length))
            for i in range(length):
                for ch in ([0] if t == GRID else [0, 3, 7]):
                    steps.append((m, ch, i, int(rng.integers(0, 3)), int(rng.integers(0, 25))))
    for m, t in enumerate(types):
        for k in range(N_IN[t]):
            if rng.random() < 0.75:
                src = int(rng.integers(0, n - 1))
                src += src >= m
                conns.append((src, int(rng.choice(OUT_PORTS[types[src]])), m, k))
    out_src = [int(rng.integers(0, n)) for _ in range(2)]
    if rng.random() < 0.4:   # (the one weight that differs from random_patch's: else half of the family's assigned modules are dead code)
        out_src[0] = int(rng.choice([m for m, t in enumerate(types) if t in (SMP, GRID, PAT)]))
    out_conns = [(s, int(rng.choice(OUT_PORTS[types[s]])), c) for c, s in enumerate(out_src) if rng.random() < 0.9]
    if not out_conns:
        out_conns = [(out_src[0], OUT_PORTS[types[out_src[0]]][0], 0)]
    out_pos = int(rng.integers(0, n + 1))

    def build(g):
        ids = []
        for i, t in enumerate(types):
            if i == out_pos:
                build.out = g.add_module(0)
            ids.append(g.add_module(t))
        if out_pos == n:
            build.out = g.add_module(0)
        for m, f, v in fields:
            g.set_field(ids[m], f, v)
        for m, ch, i, st, val in steps:
            g.set_step(ids[m], ch, i, st, val)
        for m, wave, rate in waves:
            g.set_wave(ids[m], wave, rate)
        for s, sp, k, kp in conns:
            g.connect(ids[s], sp, ids[k], kp)
        for s, sp, c in out_conns:
            g.connect(ids[s], sp, build.out, c)
        return ids

    build.types, build.conns, build.out_conns, build.own = list(types), list(conns), list(out_conns), own
    build.cells = {}   # what build() leaves in a sequencer: {m: (states u8 [channels][64], values u16 [64], length)}
    for m, t in enumerate(types):
        if t in (GRID, PAT):
            build.cells[m] = (np.zeros((1 if t == GRID else 8, 64), dtype=np.uint8), np.zeros(64, dtype=np.uint16), next(v for mm, f, v in fields if mm == m))
    for m, ch, i, st, val in steps:
        build.cells[m][0][ch, i] = st
        if types[m] == GRID:
            build.cells[m][1][i] = val

    overrides = []
    for m, t in enumerate(types):
        if rng.random() < 0.45:
            gen = np.random.default_rng((seed, 0xBA2C, m))
            if t == OSC:
                overrides.append((m, W.OSC_VAL, lambda V, r=gen: r.uniform(-5, 2, V).astype(np.float32)))
            elif t == VCF:
                overrides.append((m, W.VCF_FREQ, lambda V, r=gen: r.uniform(0.03, 0.7, V).astype(np.float32)))
            elif t == MATH:
                overrides.append((m, W.MATH_CONSTANT, lambda V, r=gen: r.uniform(-1, 1, V).astype(np.float32)))
            elif t == MIX:
                overrides.append((m, W.MIX_GAIN0 + 1, lambda V, r=gen: r.uniform(0, 1, V).astype(np.float32)))
            elif t == ADSR:
                overrides.append((m, W.ADSR_S_VAL, lambda V, r=gen: r.uniform(0, 1, V).astype(np.float32)))

    # ---- banks, assignments, and the overrides that meet them ----
    banks, assignments = [], {}
    long_wave_at = int(rng.integers(0, n_smp)) if rng.random() < 0.25 else -1   # a quarter of the patches: one wave past the 2 048 an LDS copy holds
    k_smp = 0
    for m, t in enumerate(types):
        if t == SMP:
            n_waves = int(rng.integers(1, 10))
            lengths = [int(rng.choice(BANK_WAVE_LENGTHS)) if rng.random() < 0.7 else int(rng.integers(0, 1201)) for _ in range(n_waves)]
            if rng.random() < 0.5:   # a small bank: with the own wave it fits one LDS copy
                lengths = [min(x, 257) for x in lengths]
            if k_smp == long_wave_at:
                lengths[int(rng.integers(0, n_waves))] = int(rng.integers(2049, 5001))
            k_smp += 1
            a = float(rng.choice(BANK_AMPLITUDES))
            banks.append({"m": m, "type": SMP, "waves": [rng.uniform(-a, a, x).astype(np.float32) for x in lengths],
                          "rates": [float(rng.choice(BANK_RATES)) for _ in range(n_waves)]})
            n_items = n_waves
        elif t in (GRID, PAT):
            n_items = int(rng.integers(1, 9))
            lengths = np.array([int(rng.choice(BANK_SEQ_LENGTHS)) if rng.random() < 0.6 else int(rng.integers(1, 65)) for _ in range(n_items)], dtype=np.intc)
            if t == GRID:   # cells past a sequence's length are drawn like the others: only `lengths` may delimit
                st, vals = rng.integers(0, 3, (n_items, 64)).astype(np.uint8), rng.integers(0, BANK_NOTE_MAX + 1, (n_items, 64)).astype(np.uint16)
            else:
                st, vals = rng.integers(0, 3, (n_items, 8, 64)).astype(np.uint8), None
            banks.append({"m": m, "type": t, "states": st, "values": vals, "lengths": lengths})
            if rng.random() < 0.5:   # at or past most lengths: the wrap happens at sample 0
                overrides.append((m, W.GRIDSEQ_CURRENT_STEP if t == GRID else W.PATSEQ_CURRENT_STEP,
                                  lambda V, r=np.random.default_rng((seed, 0xBA2C, m, 1)): r.integers(0, 64, V).astype(np.float32)))
        else:
            continue
        if rng.random() < 0.8:
            const = int(rng.integers(-1, n_items)) if rng.random() < 0.2 else None   # one assignment in five: the same item for every voice

            def assign(V, edit=0, m=m, n_items=n_items, const=const):
                if const is not None and edit == 0:
                    return np.full(V, const, dtype=np.intc)
                return np.random.default_rng((seed, 0xBA2C, m, 2, edit)).integers(-1, n_items, V).astype(np.intc)

            assignments[m] = assign
            if t == SMP and rng.random() < 0.35:   # honoured by the voices on the own wave, ignored by the banked ones
                overrides.append((m, W.SAMPLE_WAVE_SAMPLE_RATE, lambda V, r=np.random.default_rng((seed, 0xBA2C, m, 3)): r.choice(BANK_RATES + [12345.0, 32000.0], V).astype(np.float32)))
    return B, build, overrides, banks, assignments


# ---- the wide family: settings beyond the sliders (tests/test_gpu_wide_fuzz.py, tests/test_wide_fuzz_host.py, tools/cpu_soak.py --family wide) ----
# Nothing in the library clamps a field: every value below is valid for the ABI.  Each module is *wide* with probability one half and draws
# from the table; the others draw as random_patch does, so wide values meet ordinary neighbours.
WIDE_OSC_ODD = [-1100.0, -150.0, -130.0, -113.0, 130.0, 1100.0]   # (below about -119.2 the increment 440 x 2^val / 48 000 is no normal f32)
WIDE_OSC_UNDERFLOW = -119.0
WIDE_ADSR_TIMES = [0.0, -0.01, 1e-6, 1e-4, 0.02, 30.0]
WIDE_SPO = [0, 1, 5, 19, 65535]
WIDE_SPO_P = [0.4, 0.15, 0.15, 0.15, 0.15]   # (0 is the value that has no bound: drawn more often than the others)
WIDE_WAVE_RATES = [1.0, 100.0, 384000.0, 3e6]
WIDE_SPECIALS = [np.inf, -np.inf, np.nan, 1e-40, -0.0, 3e38, -3e38]
WIDE_CLASSES = ("osc", "vcf", "adsr", "gain", "nonlin", "spo", "smp", "verb")          # the table's rows ...
WIDE_SUBCLASSES = ("adsr_neg", "osc_underflow", "spo0")                                    # ... and three kinds of value inside them
# the RNG streams, one per sub-family: chosen so that the pinned seeds meet the guards' bars (tests/test_wide_fuzz_host.py; notes/r28.md R28.3 has the search)
WIDE_STREAMS = {"plain": 123, "noise": 89, "nonlin": 4982, "special": 25}


def _wide_tags(cls, f, v):
    tags = {cls}
    if cls == "adsr" and f != W.ADSR_S_VAL and v < 0:
        tags.add("adsr_neg")
    if cls == "osc" and v < WIDE_OSC_UNDERFLOW:
        tags.add("osc_underflow")
    if cls == "spo" and v == 0:
        tags.add("spo0")
    return tags


def random_wide_patch(seed, noise=False, special=False, clamp=()):
    """-> (B, build(g) -> ids, overrides): random_patch's graph draw (types, wiring rule, cycles, the OutputModule anywhere; FUZZ_NONLIN as
    there) from streams of its own, with half of the modules *wide* (the table in notes/r28.md).  Per-voice overrides by random_patch's 0.45
    rule over more fields; for a wide module voice 0 and every fourth voice draw from today's range and the rest from the wide one.
    special: each float setting (patch level, or one voice of an override) is replaced with probability 0.06 by one of WIDE_SPECIALS.
    clamp: names out of WIDE_CLASSES / WIDE_SUBCLASSES — the wide values of that kind are clamped back into today's range (the guards'
    "is this class heard" question); the rest of the patch keeps its draw.  build.types / .wide ({m: class}) / .kinds (the kinds of wide value at patch level) describe the patch."""
    stream = WIDE_STREAMS["noise" if noise else "special" if special else "nonlin" if os.environ.get("FUZZ_NONLIN") else "plain"]
    tag = (seed, 0x51DE, stream, int(noise), int(special))
    rng, wr, sr_ = np.random.default_rng(tag), np.random.default_rng(tag + (1,)), np.random.default_rng(tag + (2,))
    clamp = set(clamp)
    f32 = lambda v: float(np.float32(v))
    B = int(rng.choice([1, 3, 16, 64, 1024]))
    n = int(rng.integers(4, 11))
    types = [OSC, OSC] + [int(rng.choice([OSC, VCF, ADSR, VCA, MIX, MATH, GRID, PAT, SMP], p=[.2, .15, .12, .13, .1, .15, .05, .05, .05])) for _ in range(n - 2)]
    rng.shuffle(types)
    if noise:
        types = [NOISE if u < 0.2 else VERB if u < 0.3 else t for t, u in zip(types, rng.random(n))]
        if NOISE not in types:
            types[int(rng.integers(0, n))] = NOISE
    if os.environ.get("FUZZ_NONLIN"):
        r3 = np.random.default_rng(tag + (9,))
        types = [NONLIN if t == MATH and r3.random() < 0.5 else t for t in types]
    is_wide = [bool(u < 0.5) for u in wr.random(n)]
    fields, steps, conns, waves, wide, kinds = [], [], [], [], {}, set()

    def put(m, f, today, wide_value, cls, lo, hi):
        """one float setting: today's draw, or (wide module) the wide one — clamped into today's [lo, hi] where `clamp` names its kind"""
        v = today
        if is_wide[m]:
            v, wide[m] = f32(wide_value), cls
            kinds.update(_wide_tags(cls, f, v))
            if _wide_tags(cls, f, v) & clamp:
                v = min(max(v, lo), hi)
        fields.append((m, f, f32(v)))

    for m, t in enumerate(types):
        if t == OSC:
            odd = wr.random() < 0.1
            put(m, W.OSC_VAL, rng.uniform(-6, 3), wr.choice(WIDE_OSC_ODD) if odd else wr.uniform(-14, 9), "osc", -6.0, 3.0)
            if rng.random() < 0.2:
                fields.append((m, W.OSC_ANTIALIASING, 0))
        elif t == VCF:
            put(m, W.VCF_FREQ, rng.uniform(0.02, 0.8), wr.uniform(-0.3, 1.4), "vcf", 0.02, 0.8)
            put(m, W.VCF_RES, rng.uniform(0, 1), wr.uniform(-0.5, 1.6), "vcf", 0.0, 1.0)
            put(m, W.VCF_EXP_AMT, rng.uniform(0, 1), wr.uniform(-3, 3), "vcf", 0.0, 1.0)
        elif t == ADSR:
            put(m, W.ADSR_A_SEC, rng.choice([0.0, 0.001, 0.004]), wr.choice(WIDE_ADSR_TIMES), "adsr", 0.0, 0.004)
            put(m, W.ADSR_D_SEC, rng.uniform(0.001, 0.01), wr.choice(WIDE_ADSR_TIMES), "adsr", 0.001, 0.01)
            put(m, W.ADSR_S_VAL, rng.uniform(0, 1), wr.uniform(-1.5, 2.5), "adsr", 0.0, 1.0)
            put(m, W.ADSR_R_SEC, rng.uniform(0.001, 0.01), wr.choice(WIDE_ADSR_TIMES), "adsr", 0.001, 0.01)
        elif t == VCA:
            fields.append((m, W.VCA_NEGATIVE, int(rng.random() < 0.3)))
        elif t == MIX:
            for k in range(4):
                put(m, W.MIX_GAIN0 + k, rng.uniform(0, 1.2), wr.uniform(-12, 12), "gain", 0.0, 1.2)
        elif t == MATH:
            put(m, W.MATH_CONSTANT, rng.uniform(-1, 1), wr.uniform(-12, 12), "gain", -1.0, 1.0)
            fields.append((m, W.MATH_OPERATION, int(rng.integers(0, 3))))
        elif t == NONLIN:
            put(m, W.NONLIN_CONSTANT, rng.choice([0.5, 2.0, 3.0, rng.uniform(0.3, 3.0)]), wr.choice([0.0, 1.0, wr.uniform(-1, 6), wr.uniform(-1, 6)]), "nonlin", 0.3, 3.0)
        elif t == VERB:
            for f, lo, hi in ((W.FREEVERB_DAMPENING, 0, 2), (W.FREEVERB_WET, 0, 1), (W.FREEVERB_WIDTH, 0, 1), (W.FREEVERB_ROOM_SIZE, 0, 1), (W.FREEVERB_DRY, 0, 1)):
                put(m, f, rng.uniform(lo, hi), wr.uniform(-0.5, 2.5), "verb", float(lo), float(hi))
            fields.append((m, W.FREEVERB_FREEZE, int(rng.random() < 0.2)))
        elif t == SMP:
            wave, rate = rng.uniform(-1, 1, int(rng.integers(1, 400))).astype(np.float32), float(rng.choice([8000.0, 44100.0, 48000.0, 96000.0]))
            if is_wide[m]:
                wide[m] = "smp"
                kinds.add("smp")
                loud, fast = (wave * np.float32(8.0)).astype(np.float32), float(wr.choice(WIDE_WAVE_RATES))
                if "smp" not in clamp:
                    wave, rate = loud, fast
            waves.append((m, wave, rate))
        elif t in (GRID, PAT):
            length = int(rng.integers(1, 9))
            fields.append((m, W.GRIDSEQ_LENGTH if t == GRID else W.PATSEQ_LENGTH, length))
            for i in range(length):
                for ch in ([0] if t == GRID else [0, 3, 7]):
                    steps.append((m, ch, i, int(rng.integers(0, 3)), int(rng.integers(0, 25))))
            if t == GRID and is_wide[m]:
                spo, wide[m] = int(wr.choice(WIDE_SPO, p=WIDE_SPO_P)), "spo"
                kinds.update(_wide_tags("spo", 0, spo))
                fields.append((m, W.GRIDSEQ_STEPS_PER_OCTAVE, 12 if _wide_tags("spo", 0, spo) & clamp else spo))
    for m, t in enumerate(types):
        for k in range(N_IN[t]):
            if rng.random() < 0.75:
                src = int(rng.integers(0, n - 1))
                src += src >= m
                conns.append((src, int(rng.choice(OUT_PORTS[types[src]])), m, k))
    # (a NonLinear's exponent is its setting only while nothing is wired to its exponent input: a wide one keeps that input free — the wire
    # is drawn and dropped, so the rest of the patch keeps its draw.  Without this three in four wide exponents are dead settings.)
    conns = [c for c in conns if not (types[c[2]] == NONLIN and c[3] == 1 and is_wide[c[2]])]
    out_src = [int(rng.integers(0, n)) for _ in range(2)]
    out_conns = [(s, int(rng.choice(OUT_PORTS[types[s]])), c) for c, s in enumerate(out_src) if rng.random() < 0.9]
    if not out_conns:
        out_conns = [(out_src[0], OUT_PORTS[types[out_src[0]]][0], 0)]
    out_pos = int(rng.integers(0, n + 1))

    # ---- per-voice overrides: (field, today's lo, hi, wide draw(r, V) -> values) per type; a module passes the 0.45 rule, then a non-empty subset of its fields ----
    times = lambda r, V: r.choice(WIDE_ADSR_TIMES, V)
    table = {OSC: [(W.OSC_VAL, -5.0, 2.0, lambda r, V: np.where(r.random(V) < 0.1, r.choice(WIDE_OSC_ODD, V), r.uniform(-14, 9, V)))],
             VCF: [(W.VCF_FREQ, 0.03, 0.7, lambda r, V: r.uniform(-0.3, 1.4, V)), (W.VCF_RES, 0.0, 1.0, lambda r, V: r.uniform(-0.5, 1.6, V)),
                   (W.VCF_EXP_AMT, 0.0, 1.0, lambda r, V: r.uniform(-3, 3, V))],
             ADSR: [(W.ADSR_A_SEC, 0.0, 0.004, times), (W.ADSR_D_SEC, 0.001, 0.01, times), (W.ADSR_S_VAL, 0.0, 1.0, lambda r, V: r.uniform(-1.5, 2.5, V)),
                    (W.ADSR_R_SEC, 0.001, 0.01, times)],
             MIX: [(W.MIX_GAIN0 + 1, 0.0, 1.0, lambda r, V: r.uniform(-12, 12, V))],
             MATH: [(W.MATH_CONSTANT, -1.0, 1.0, lambda r, V: r.uniform(-12, 12, V))],
             NONLIN: [(W.NONLIN_CONSTANT, 0.3, 3.0, lambda r, V: np.where(r.random(V) < 0.2, r.choice([0.0, 1.0], V), r.uniform(-1, 6, V)))],
             GRID: [(W.GRIDSEQ_STEPS_PER_OCTAVE, 12, 12, lambda r, V: r.choice(WIDE_SPO, V, p=WIDE_SPO_P))]}
    cls_of = {OSC: "osc", VCF: "vcf", ADSR: "adsr", MIX: "gain", MATH: "gain", NONLIN: "nonlin", GRID: "spo"}
    overrides = []
    for m, t in enumerate(types):
        if rng.random() < 0.45 and t in table and not (t == GRID and not is_wide[m]):   # (an ordinary sequencer keeps its 12 steps per octave)
            rows = table[t]
            picked = [rows[k] for k in range(len(rows)) if len(rows) == 1 or rng.random() < 0.5] or [rows[int(rng.integers(0, len(rows)))]]
            for f, lo, hi, draw in picked:
                def values(V, m=m, f=f, lo=lo, hi=hi, draw=draw, cls=cls_of[t]):
                    r = np.random.default_rng(tag + (3, m, f))
                    integer = f == W.GRIDSEQ_STEPS_PER_OCTAVE and t == GRID
                    today = np.full(V, 12.0) if integer else r.uniform(lo, hi, V)
                    vals = today.astype(np.float32)
                    if is_wide[m]:
                        wv = np.asarray(draw(r, V), dtype=np.float64).astype(np.float32)
                        keep = np.array([bool(_wide_tags(cls, f, float(x)) & clamp) for x in wv])   # clamped: back into today's range
                        wv = np.where(keep, np.clip(wv, np.float32(lo), np.float32(hi)), wv).astype(np.float32)
                        ordinary = np.arange(V) % 4 == 0     # voice 0 and every fourth voice: today's range
                        vals = np.where(ordinary, vals, wv).astype(np.float32)
                        if special and not integer:
                            rs = np.random.default_rng(tag + (4, m, f))
                            hit = rs.random(V) < 0.06
                            vals = np.where(hit, rs.choice(WIDE_SPECIALS, V).astype(np.float32), vals).astype(np.float32)
                    elif special and not integer:
                        rs = np.random.default_rng(tag + (4, m, f))
                        hit = rs.random(V) < 0.06
                        vals = np.where(hit, rs.choice(WIDE_SPECIALS, V).astype(np.float32), vals).astype(np.float32)
                    return vals
                overrides.append((m, f, values))
                if is_wide[m]:
                    wide[m] = cls_of[t]
    if special:   # patch level: every float setting (the integer-typed fields keep integers of their type)
        ints = {(OSC, W.OSC_ANTIALIASING), (VCA, W.VCA_NEGATIVE), (MATH, W.MATH_OPERATION), (VERB, W.FREEVERB_FREEZE), (GRID, W.GRIDSEQ_LENGTH),
                (GRID, W.GRIDSEQ_STEPS_PER_OCTAVE), (PAT, W.PATSEQ_LENGTH)}
        fields = [(m, f, v) if (types[m], f) in ints or sr_.random() >= 0.06 else (m, f, float(np.float32(sr_.choice(WIDE_SPECIALS)))) for m, f, v in fields]

    def build(g):
        ids = []
        for i, t in enumerate(types):
            if i == out_pos:
                build.out = g.add_module(0)
            ids.append(g.add_module(t))
        if out_pos == n:
            build.out = g.add_module(0)
        for m, f, v in fields:
            g.set_field(ids[m], f, v)
        for m, ch, i, st, val in steps:
            g.set_step(ids[m], ch, i, st, val)
        for m, wave, rate in waves:
            g.set_wave(ids[m], wave, rate)
        for s, sp, k, kp in conns:
            g.connect(ids[s], sp, ids[k], kp)
        for s, sp, c in out_conns:
            g.connect(ids[s], sp, build.out, c)
        if noise:
            g.set_noise_seed(seed * 7919 + 1, 1000 * seed)
        return ids

    build.types, build.wide, build.kinds, build.fields, build.conns, build.out_conns = list(types), dict(wide), set(kinds), list(fields), list(conns), list(out_conns)
    return B, build, overrides
