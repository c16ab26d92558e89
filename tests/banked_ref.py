"""The reference of the banked fuzz family (tests/fuzz_patches.py, random_banked_patch): the oracle knows no bank.

The contract stated at the top of tests/test_gpu_wave_bank.py and tests/test_gpu_sequence_bank.py: voice v renders what a ONE-voice patch
renders after set_wave of its bank wave, or after set_step + *_LENGTH of its bank sequence.  So the reference clones the built patch per
voice (or per group of voices that play the same tuple of items), writes the items the way those two files' oracle_voice / oracle_write
do, applies the voice's overrides and renders.  No arithmetic is restated here."""
import numpy as np

from tests.fuzz_patches import GRID, PAT, SMP, W, random_banked_patch

SEEDS = list(range(48))            # the GPU file's seed list; tests/test_banked_fuzz_host.py asserts the guards on it
WIDE_SEEDS = [3, 11]               # players and sequencers that render, at B = 3 and B = 1024
MIXED_STAGING = [20, 30, 43, 46]   # seeds whose generated kernel holds one bank staged in LDS and one read through the window: specialised on the GPU too
SMP_STATE = ["SAMPLE_POS", "SAMPLE_PLAYING"]
GRID_STATE = ["GRIDSEQ_CURRENT_STEP", "GRIDSEQ_STEP_LAST", "GRIDSEQ_SYNC_LAST", "GRIDSEQ_LAST"]
PAT_STATE = ["PATSEQ_CURRENT_STEP", "PATSEQ_STEP_LAST", "PATSEQ_SYNC_LAST"]
STATE = {SMP: SMP_STATE, GRID: GRID_STATE, PAT: PAT_STATE}


def sizes(B):
    """voices, samples: the existing fuzz's — past the first control chunk and, at B = 1024, past two ring periods"""
    return (67, 1300) if B < 1024 else (131, 2300)


def draw(seed, V=None):
    """One draw of the seed's patch for V voices (None: sizes(B)'s; the generators are stateful: drawn once, here) ->
    (B, build, ov [(m, field, values [V])], banks, idx {m: int32 [V]})"""
    B, build, overrides, banks, assignments = random_banked_patch(seed)
    V = V or sizes(B)[0]
    return B, build, [(m, f, fn(V)) for m, f, fn in overrides], banks, {m: fn(V) for m, fn in assignments.items()}


def install(p, ids, build, banks, idx):
    """banks and assignments onto a library patch whose voices are configured"""
    for b in banks:
        if b["type"] == SMP:
            p.set_wave_bank(ids[b["m"]], b["waves"], b["rates"])
        else:
            p.set_sequence_bank(ids[b["m"]], b["states"], b["values"], b["lengths"])
    for m, a in idx.items():
        (p.set_voice_waves if build.types[m] == SMP else p.set_voice_sequences)(ids[m], a)


def state_fields(bank):
    return [getattr(W, name) for name in STATE[bank["type"]]]


def write_item(g, ids, build, bank, item, own_rate=None, load_own=False):
    """Voice's item of one bank into the one-voice patch g, the way a host without a bank would set it.  item < 0 is the module's own
    wave / cells: nothing to do on a fresh patch, a wave load / a rewrite of the cells in an edit (load_own)."""
    m, mid = bank["m"], ids[bank["m"]]
    if bank["type"] == SMP:
        if item >= 0:
            g.set_wave(mid, bank["waves"][item], bank["rates"][item])
        elif load_own:
            own = build.own[m]
            g.set_wave(mid, own[0] if own else np.zeros(0, dtype=np.float32), own_rate)
        return
    grid = bank["type"] == GRID
    if item < 0 and not load_own:
        return
    states, values, length = build.cells[m] if item < 0 else (bank["states"][item].reshape(-1, 64), bank["values"][item] if grid else None, int(bank["lengths"][item]))
    f_len = W.GRIDSEQ_LENGTH if grid else W.PATSEQ_LENGTH
    g.set_field(mid, f_len, 64)
    for i in range(64):
        inside = item < 0 or i < length
        for c in range(states.shape[0]):
            st = int(states[c, i]) if inside else 0
            g.set_step(mid, c, i, st, int(values[i]) if grid and st else 0)
    g.set_field(mid, f_len, length)


def ignored_override(bank_of, items, m, f):
    """a per-voice wave_sample_rate is ignored by a voice that plays a bank wave"""
    return m in bank_of and bank_of[m]["type"] == SMP and f == W.SAMPLE_WAVE_SAMPLE_RATE and items.get(m, -1) >= 0


def reference(oracle, B, build, ov, banks, idx, V, T, channels=2, threads=8):
    """One render, every voice from a fresh patch -> frames f32 [C][T][V].  Voices that play the same tuple of items share one clone
    and one render_batch."""
    proto = oracle.OraclePatch(48000, B, channels)
    ids = build(proto)
    mods = sorted(idx)
    bank_of = {b["m"]: b for b in banks}
    keys = np.stack([idx[m] for m in mods], axis=1) if mods else np.zeros((V, 0), dtype=np.intc)
    out = np.empty((channels, T, V), dtype=np.float32)
    for key in sorted(set(map(tuple, keys.tolist()))):
        who = np.flatnonzero((keys == np.array(key, dtype=keys.dtype)).all(axis=1))
        items = dict(zip(mods, key))
        g = proto.clone()
        for m in mods:
            write_item(g, ids, build, bank_of[m], items[m])
        part = [(ids[m], f, vals[who]) for m, f, vals in ov if not ignored_override(bank_of, items, m, f)]
        out[:, :, who] = g.render_batch(len(who), T, part, threads=threads)[0]
    return out


def reference_edits(oracle, B, build, ov, banks, segments, V, channels=2):
    """render / write / render per voice.  segments: [({m: idx [V]}, samples), ...] — the first dict is the patch's assignment, each later
    one names the modules that are given a new assignment there (a wave load / an edit of cells for EVERY voice of that module, the ones
    that stay on their item included).  Samples are whole multiples of B.  -> frames f32 [C][sum][V], state {m: f64 [fields][V]}."""
    proto = oracle.OraclePatch(48000, B, channels)
    ids = build(proto)
    bank_of = {b["m"]: b for b in banks}
    n = sum(s[1] for s in segments)
    assert all(s[1] % B == 0 for s in segments)
    out = np.empty((channels, n, V), dtype=np.float32)
    state = {b["m"]: np.empty((len(STATE[b["type"]]), V)) for b in banks}
    for v in range(V):
        g = proto.clone()
        items, parts = {}, []
        for k, (assign, samples) in enumerate(segments):
            for m in sorted(assign):
                items[m] = int(assign[m][v])
                bank = bank_of[m]
                own_rate = None
                if bank["type"] == SMP and items[m] < 0 and k > 0:   # the own wave's rate: this voice's override, or the module's
                    per_voice = [vals[v] for mm, f, vals in ov if mm == m and f == W.SAMPLE_WAVE_SAMPLE_RATE]
                    own_rate = float(per_voice[0]) if per_voice else (build.own[m][1] if build.own[m] else proto.get_field(ids[m], W.SAMPLE_WAVE_SAMPLE_RATE))
                write_item(g, ids, build, bank, items[m], own_rate=own_rate, load_own=k > 0)
            if k == 0:
                for m, f, vals in ov:
                    if not ignored_override(bank_of, items, m, f):
                        g.set_field(ids[m], f, float(vals[v]))
            parts.append(g.render(samples))
        out[:, :, v] = np.concatenate(parts, axis=1)
        for b in banks:
            state[b["m"]][:, v] = [g.get_field(ids[b["m"]], f) for f in state_fields(b)]
    return out, state


# ---- what a seed's graph looks like: the shapes the coverage guards count ------------------------------------------------------------
def graph_facts(build, ov, banks, idx):
    """-> dict of the structural facts of one drawn patch (module indices are the generator's)"""
    n = len(build.types)
    preds = {m: set() for m in range(n)}
    for s, sp, k, kp in build.conns:
        preds[k].add(s)

    def ancestors(roots):
        seen, todo = set(), list(roots)
        while todo:
            for s in preds[todo.pop()]:
                if s not in seen:
                    seen.add(s)
                    todo.append(s)
        return seen

    out_src = {s for s, sp, c in build.out_conns}
    live = out_src | ancestors(out_src)
    per_voice = {m for m, f, vals in ov} | set(idx)
    bank_of = {b["m"]: b for b in banks}
    players = [m for m in idx if bank_of[m]["type"] == SMP]
    region = {m: (len(build.own[m][0]) if build.own[m] else 0) + sum(len(w) for w in bank_of[m]["waves"]) for m in players}

    def louder(m):
        own = np.abs(build.own[m][0]).max() if build.own[m] else 0.0
        return max([np.abs(w).max() for w in bank_of[m]["waves"] if len(w)], default=0.0) > own

    seqs = [b["m"] for b in banks if b["type"] in (GRID, PAT)]
    return {
        "live": live,
        "live_waves": sum(len(bank_of[m]["waves"]) for m in players if m in live),
        "live_sequences": sum(len(bank_of[m]["lengths"]) for m in idx if m in live and bank_of[m]["type"] != SMP),
        "two_players": len(players) >= 2,
        "staged_and_not": len(players) >= 2 and min(region.values()) <= 2048 < max(region.values()),
        "on_cycle": any(m in ancestors([m]) and m in live for m in idx),
        "nothing_per_voice_upstream": any(m in live and not (ancestors([m]) & per_voice) and not any(mm == m for mm, f, vals in ov) for m in idx),
        "dead": any(m not in live for m in idx),
        "constant": any(len(set(a.tolist())) == 1 for a in idx.values()),
        "unassigned_bank": any(b["m"] not in idx for b in banks),
        "louder_live_player": any(m in live and louder(m) and (idx[m] >= 0).any() for m in players),
        "seq_beside_unassigned": any(m in idx for m in seqs) and any(m not in idx for m in seqs),
    }


def edit_module(seed):
    """the module an edit scenario gives a fresh assignment: the seed's first assigned module that renders (None: it has none)"""
    B, build, ov, banks, idx = draw(seed, 2)
    live = graph_facts(build, ov, banks, idx)["live"]
    return next((m for m in sorted(idx) if m in live), None)


EDIT_SEEDS = [s for s in SEEDS if edit_module(s) is not None][:16]
