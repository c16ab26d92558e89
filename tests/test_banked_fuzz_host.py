"""The banked fuzz family (tests/fuzz_patches.py, random_banked_patch) without a GPU: the C oracle against its NumPy twin on it, the
reference (tests/banked_ref.py) against the plain oracle where no voice plays a bank item, and the guards — conditions on the reference
alone, over the seed list tests/test_gpu_banked_fuzz.py runs: the assignments bite, the renders are not trivial, and every shape the
family is meant to reach (notes/r22.md) occurs."""
import numpy as np
import pytest

import srack_pkg
from tests import banked_ref as R
from tests.npgraph import NumpyGraph


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("seed", R.SEEDS[:24])
def test_c_oracle_equals_numpy_twin(oracle, seed):
    """two voices of the seed's patch, each as a one-voice patch with its items written and its overrides set, in both restatements"""
    V = 8
    B, build, ov, banks, idx = R.draw(seed, V)
    T = 500 if B < 1024 else 1300
    bank_of = {b["m"]: b for b in banks}
    for v in (3, 6):
        g, ng = oracle.OraclePatch(48000, B, 2), NumpyGraph(48000, B, 2)
        ids = build(g)
        build(ng)
        items = {m: int(a[v]) for m, a in idx.items()}
        for m in sorted(items):
            for graph in (g, ng):
                R.write_item(graph, ids, build, bank_of[m], items[m])
        for m, f, vals in ov:
            if not R.ignored_override(bank_of, items, m, f):
                g.set_field(ids[m], f, float(vals[v]))
                ng.set_field(ids[m], f, float(vals[v]))
        assert g.plan() == ng.plan()[0]
        a, b = g.render(T), ng.render(T)
        assert same(a, b).all(), f"seed {seed} voice {v}: {1 - same(a, b).mean():.5f} of the samples differ"


_CACHE = {}


def renders(oracle, seed):
    """-> (facts, frames with the assignment, frames with every voice on the own item, the plain patch's render_batch, banked voices)"""
    if seed not in _CACHE:
        B, build, ov, banks, idx = R.draw(seed)
        V, T = R.sizes(B)
        ref = R.reference(oracle, B, build, ov, banks, idx, V, T)
        own = R.reference(oracle, B, build, ov, banks, {m: np.full(V, -1, dtype=np.intc) for m in idx}, V, T)
        o = oracle.OraclePatch(48000, B, 2)
        ids = build(o)
        plain, _ = o.render_batch(V, T, [(ids[m], f, vals) for m, f, vals in ov], threads=8)
        banked = np.zeros(V, dtype=bool)
        for a in idx.values():
            banked |= a >= 0
        _CACHE[seed] = (R.graph_facts(build, ov, banks, idx), ref, own, plain, banked, (B, build, ov, banks, idx))
    return _CACHE[seed]


@pytest.mark.parametrize("seed", R.SEEDS)
def test_all_voices_on_the_own_item_is_the_plain_patch(oracle, seed):
    _, _, own, plain, _, _ = renders(oracle, seed)
    assert same(own, plain).all()


def test_guard_the_assignment_bites(oracle):
    """in at least three quarters of the seeds, at least a quarter of the voices that play a bank item differ from themselves on the own
    item (the others: dead code, a bank without an assignment, an effect that a closed VCA or an unconnected port hides)"""
    bites = []
    for seed in R.SEEDS:
        _, ref, own, _, banked, _ = renders(oracle, seed)
        differs = (~same(ref, own)).any(axis=(0, 1))
        bites.append(bool(banked.any()) and differs[banked].mean() >= 0.25)
    print("the assignment bites in %d of %d seeds" % (sum(bites), len(bites)))
    assert sum(bites) * 4 >= 3 * len(bites), bites


def test_guard_the_reference_is_not_trivial(oracle):
    loud, nonfinite = 0, 0
    for seed in R.SEEDS:
        ref = renders(oracle, seed)[1]
        fin = np.isfinite(ref)
        loud += bool(fin.any()) and float(np.abs(ref[fin]).max()) > 0.01
        nonfinite += not fin.all()
    print("max |ref| > 0.01 in %d of %d seeds, a non-finite sample in %d" % (loud, len(R.SEEDS), nonfinite))
    assert loud * 4 >= 3 * len(R.SEEDS) and nonfinite * 8 <= len(R.SEEDS)


def test_guard_coverage(oracle):
    """every shape at least three times.  Whether the default mode approximates a patch is the library's word (srack_render_info, which
    flattens without a GPU); everything else is read off the drawn graph."""
    S = srack_pkg.load()
    count = {}
    for seed in R.SEEDS:
        facts, _, _, _, _, (B, build, ov, banks, idx) = renders(oracle, seed)
        V = R.sizes(B)[0]
        p = S.Patch(48000, B, 2)
        ids = build(p)
        p.configure_voices(V)
        for m, f, vals in ov:
            p.set_voice_field(ids[m], f, vals)
        R.install(p, ids, build, banks, idx)
        info = p.info()
        facts = dict(facts, louder_in_an_approximated_patch=facts["louder_live_player"] and "approx[bound" in info)
        # the library's dead-code elimination and this file's reading of the graph agree on which assigned modules render
        assert ("waves=%d[" % facts["live_waves"] in info) == (facts["live_waves"] > 0) and ("waves=" in info) == (facts["live_waves"] > 0), (seed, info)
        assert ("sequences=%d[" % facts["live_sequences"] in info) == (facts["live_sequences"] > 0) and ("sequences=" in info) == (facts["live_sequences"] > 0), (seed, info)
        for k in SHAPES:
            count[k] = count.get(k, 0) + bool(facts[k])
    print("coverage over %d seeds: %s" % (len(R.SEEDS), count))
    assert all(count[k] >= 3 for k in SHAPES), count


SHAPES = ["two_players", "staged_and_not", "on_cycle", "nothing_per_voice_upstream", "dead", "constant", "unassigned_bank",
          "louder_in_an_approximated_patch", "seq_beside_unassigned"]


@pytest.mark.parametrize("seed", R.MIXED_STAGING)
def test_one_generated_kernel_stages_one_bank_and_windows_another(seed):
    """two banked players in one generated kernel, own + bank below 2 048 frames for one and above for the other: both forms in the source"""
    S = srack_pkg.load()
    B, build, ov, banks, idx = R.draw(seed)
    p = S.Patch(48000, B, 2)
    ids = build(p)
    p.configure_voices(R.sizes(B)[0])
    for m, f, vals in ov:
        p.set_voice_field(ids[m], f, vals)
    R.install(p, ids, build, banks, idx)
    for flags in (S.RENDER_SPECIALIZE | 1, S.RENDER_SPECIALIZE | 2):
        src = p.kernel_source(flags)
        assert "_bank_lds[" in src and "smp_window_read(" in src, (seed, flags)


def test_the_edit_reference_continues_the_plain_one(oracle):
    """reference_edits with one segment is reference(); with two it starts the same way (state and all: the edit is the only difference)"""
    seed = R.EDIT_SEEDS[0]
    B, build, ov, banks, idx = R.draw(seed, 5)
    a = R.reference(oracle, B, build, ov, banks, idx, 5, 2 * B)
    b, state = R.reference_edits(oracle, B, build, ov, banks, [(idx, 2 * B)], 5)
    assert same(a, b).all() and set(state) == {bk["m"] for bk in banks}
    m = sorted(idx)[0]
    c, _ = R.reference_edits(oracle, B, build, ov, banks, [(idx, B), ({m: R.random_banked_patch(seed)[4][m](5, 1)}, B)], 5)
    assert same(a[:, :B], c[:, :B]).all()
