"""The guards of tests/test_gpu_warm.py, on the oracle and the library's host side alone (notes/r27.md): a warm-start test is only worth
something if the harvest is complete (a fresh patch with it applied continues like the warm one, bit for bit), if ignoring the state or
the saved blocks would show, if both delivery routes hand the library the same patch, if "start from a saved block" does not rest on one
implementation (the C oracle against its NumPy twin), and if the checker fails on a cold start and on a start without the blocks."""
import numpy as np
import pytest

import srack_pkg
from tests import handoff_ref as H
from tests import warm_ref as WR
from tests.npgraph import NumpyGraph

GUARD = 1e-2
PLAIN = list(WR.FAMILIES["plain"])


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


@pytest.fixture(scope="module")
def S():
    return srack_pkg.load()


def _ids(cases):
    return [f"{fam}-{seed}" for fam, seed in cases]


def _voice0(w, how):
    return WR.reference(w, how, voices=[0])


# ---- completeness ----------------------------------------------------------------------------------------------------------------------
COMPLETE = [c for c in WR.CASES if c[0] != "noise"]


@pytest.mark.parametrize("family,seed", COMPLETE, ids=_ids(COMPLETE))
def test_a_fresh_patch_with_the_harvest_continues_like_the_warm_one(family, seed):
    """voice 0 of either route: the warm oracle rendered on against a FRESH oracle with the harvest applied — the reference of the GPU tests"""
    for route in WR.ROUTES:
        w = WR.fuzz_case(family, seed, route)
        warm, _ = WR._oracle(w.B, w.build)
        if route == "voices":
            for m, f, vals in w.params:
                warm.set_field(m, f, float(vals[0]))
        warm.render(w.T0)
        cont = warm.render(w.T)
        if route == "common":   # the harvest is the unmodified patch's: compared before the voices' parameters are applied
            fresh = WR.fresh_oracle(w).render(w.T)
        else:
            fresh = _voice0(w, "warm")[:, :, 0]
        assert H.same_bits(fresh, cont).all(), (w.name, WR.max_diff(fresh, cont))


NOISE = [c for c in WR.CASES if c[0] == "noise"]
SILENT = {("noise", 17), ("noise", 19)}   # patches that render zeros from any start: nothing to tell there (the plain family has three: 33, 39, 41)


@pytest.mark.parametrize("family,seed", NOISE, ids=_ids(NOISE))
def test_the_noise_familys_reference_is_reproducible_and_no_cold_start(family, seed):
    """The noise counter and a reverb's lines are no fields: the reference restarts them (as the library does), so it is no continuation
    of the warm oracle.  It is the same render twice, and another one than the cold start's."""
    for route in WR.ROUTES:
        w = WR.fuzz_case(family, seed, route)
        a, b = WR.reference(w), WR.reference(w)
        assert H.same_bits(a, b).all(), w.name
        if (family, seed) in SILENT:
            assert not a.any() and not WR.reference(w, "cold").any(), w.name
        else:
            assert WR.max_diff(a, WR.reference(w, "cold")) > GUARD, w.name


# ---- sensitivity: conditions on the inputs, met by the reference alone (no tolerance of anything) ----------------------------------------
@pytest.fixture(scope="module")
def figures():
    """{(route, seed): (B, broken edges, warm against cold, warm against state-loaded-blocks-zero)}: voice 0, the first T samples"""
    out = {}
    for route in WR.ROUTES:
        for seed in PLAIN:
            w = WR.fuzz_case("plain", seed, route)
            warm = _voice0(w, "warm")
            o, _ = WR._oracle(w.B, w.build)
            o.plan()
            out[route, seed] = (w.B, len(o.removed_edges()), WR.max_diff(warm, _voice0(w, "cold")), WR.max_diff(warm, _voice0(w, "noblocks")))
    return out


@pytest.mark.parametrize("route", WR.ROUTES)
def test_a_cold_start_would_show(figures, route):
    n = sum(figures[route, s][2] > GUARD for s in PLAIN)
    print(f"warm against cold, route {route}: {n} of {len(PLAIN)} seeds differ by more than {GUARD}; the others: {[s for s in PLAIN if not figures[route, s][2] > GUARD]}")
    assert n >= 50


@pytest.mark.parametrize("route", WR.ROUTES)
def test_ignored_blocks_would_show(figures, route):
    audible = [s for s in PLAIN if figures[route, s][3] > GUARD]
    print(f"warm against blocks zero, route {route}: {len(audible)} of {len(PLAIN)} seeds differ by more than {GUARD}: {audible}")
    assert len(audible) >= 25


@pytest.mark.parametrize("route", WR.ROUTES)
@pytest.mark.parametrize("B", [1, 3, 16, 64, 1024])
def test_every_buffer_size_has_a_seed_with_two_broken_edges_and_audible_blocks(figures, route, B):
    seeds = [s for s in PLAIN if figures[route, s][0] == B and figures[route, s][1] >= 2 and figures[route, s][3] > GUARD]
    print(f"B = {B}, route {route}: two or more broken edges and audible blocks at seeds {seeds}")
    assert seeds


@pytest.mark.parametrize("patch,B,T", sorted({(p, B, T) for p, B, T, _ in WR.NAMED}))
def test_the_named_patches_start_warm(patch, B, T):
    """Every named case differs from its cold start; p2 — the one with a ring — as the issue sets it, by more than 1e-2 (here: in every voice)"""
    w, _ = WR.named_case(patch, B, T)
    warm, cold = WR.reference(w), WR.reference(w, "cold")
    per_voice = np.abs(warm.astype(np.float64) - cold).max(axis=(0, 1))
    print(f"{w.name}: warm against cold, smallest per-voice difference {per_voice.min():.3g}; {len(w.voice_state)} state fields per voice")
    assert per_voice.min() > GUARD
    assert w.voice_state, "the voices' state differs: the route is the per-voice one"


def test_the_named_table_reaches_every_hand_matched_kernel():
    seen = {WR.named_kernel(p, B, T, f) for p, B, T, f in WR.NAMED}
    assert seen == set(WR.NAMED_KERNELS), seen ^ set(WR.NAMED_KERNELS)
    assert all(T % B == 0 for _, B, T, _ in WR.NAMED), "state is compared behind the render: it ends on a block boundary"
    assert all(T >= H.FM_BLOCK_MIN for p, B, T, f in WR.NAMED if "block" in WR.named_kernel(p, B, T, f))


# ---- both delivery routes hand the library the same patch ------------------------------------------------------------------------------
def _describe(S, p):
    out = []
    for m in range(p.num_modules()):
        t = p.module_type(m)
        ins = [p.get_input(m, k) for k in range(p.get_num_inputs(m))]
        fields = np.array([p.get_field(m, f) for f in range(WR.N_FIELDS[t])], dtype=np.float64).tobytes()
        steps = [p.get_step(m, ch, i) for ch in ([0] if t == S.MOD_GRID_SEQUENCER else range(8) if t == S.MOD_PATTERN_SEQUENCER else []) for i in range(64)]
        wave = None
        if t == S.MOD_SAMPLE:
            a, rate = p.get_wave(m)
            wave = (a.tobytes(), rate)
        # (a port without a block reads as fresh zeros, and a file holds no block of zeros: an empty answer and a block of zeros are one)
        blocks = [(lambda a: a if a.size else np.zeros(p.buffer_size, dtype=np.float32))(p.get_output_buffer(m, port)).tobytes() for port in range(p.get_num_outputs(m))]
        out.append((p.module_id(m), t, fields, ins, steps, wave, blocks))
    return out


@pytest.mark.parametrize("family,seed", WR.CASES, ids=_ids(WR.CASES))
def test_the_graph_api_and_the_file_deliver_the_same_patch(S, family, seed):
    for route in WR.ROUTES:
        w = WR.fuzz_case(family, seed, route)
        a = WR.make_patch(S, w, False, voices=False)
        b = WR.through_a_file(S, a, w)
        da, db = _describe(S, a), _describe(S, b)
        assert [x[1] for x in da] == list(w.types)
        assert da == db, w.name
        assert a.save_srk() == b.save_srk(), w.name
        assert a.plan() == b.plan() == WR.fresh_oracle(w).plan()
        # ... and it is the harvest that arrived: every loaded field, every block
        W = WR.workloads()
        for (m, f), v in w.fields.items():
            if WR.is_loaded(W, w.types[m], f):
                assert np.float64(b.get_field(m, f)).tobytes() == np.float64(v).tobytes(), (w.name, m, f)
        for (m, port), blk in w.blocks.items():
            got = b.get_output_buffer(m, port)
            assert got.tobytes() == blk.tobytes() or (got.size == 0 and not blk.any() and not np.signbit(blk).any()), (w.name, m, port)


@pytest.mark.parametrize("family,seed", WR.CASES, ids=_ids(WR.CASES))
def test_the_voices_hold_what_was_loaded_before_the_first_render(S, family, seed):
    """srack_voices_get_field's "nothing rendered yet" branch on the host: the initial table is the loaded state (the device test reads it
    again where a device holds it)"""
    for route in WR.ROUTES:
        w = WR.fuzz_case(family, seed, route)
        p = WR.make_patch(S, w, seed % 2 == 1)
        for m, f, vals in WR.loaded_state(w):
            got = p.get_voice_field(m, f)
            for v in WR.FIRST_VOICES + (w.V - 1,):
                assert H.same_bits(np.float64(got[v]), np.float64(vals[v])).all(), (w.name, m, f, v, got[v], vals[v])


# ---- the C oracle against its NumPy twin, from a warm start ----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(20))
def test_c_equals_numpy_from_a_warm_start(seed):
    """as tests/test_oracle.py::test_random_patches_c_equals_numpy, but both start from the harvest: state fields and saved blocks"""
    w = WR.fuzz_case("plain", seed, "common")
    T = 500 if w.B < 1024 else 1300
    g, ng = WR.fresh_oracle(w), NumpyGraph(48000, w.B, 2)
    w.build(ng)
    WR.apply(ng, w.types, w.fields, w.blocks)
    for m, f, vals in w.params:   # one voice: voice 3's draw
        g.set_field(m, f, float(vals[3]))
        ng.set_field(m, f, float(vals[3]))
    assert g.plan() == ng.plan()[0]
    a, b = g.render(T), ng.render(T)
    assert H.same_bits(a, b).all(), (seed, WR.max_diff(a, b))
    cold, _ = WR._oracle(w.B, w.build)
    for m, f, vals in w.params:
        cold.set_field(m, f, float(vals[3]))
    print(f"seed {seed}: warm against cold {WR.max_diff(a, cold.render(T)):.3g}")


# ---- the checker -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", WR.ROUTES)
@pytest.mark.parametrize("seed", [0, 5, 22, 23])   # buffer_size 1024, 64, 64, 1
def test_the_checker_fails_on_a_cold_start_and_on_a_start_without_the_blocks(figures, seed, route):
    w = WR.fuzz_case("plain", seed, route)
    assert figures[route, seed][3] > GUARD, "a seed whose blocks are audible"
    ref = WR.reference(w)
    for exact in (True, False):
        WR.check(ref.copy(), ref, exact)
        for how in ("cold", "noblocks"):
            with pytest.raises(AssertionError):
                WR.check(WR.reference(w, how), ref, exact)


def test_the_checker_tells_an_ulp_and_holds_non_finite_samples_to_their_place_and_sign():
    ref = np.linspace(-1, 1, 24, dtype=np.float32).reshape(2, 4, 3)
    off = ref.copy()
    off[1, 2, 1] = np.nextafter(off[1, 2, 1], np.float32(2))
    with pytest.raises(AssertionError):
        WR.check(off, ref, True)
    assert WR.check(off, ref, False) < 1e-6
    a, b = ref.copy(), ref.copy()
    a[0, 0, 0], b[0, 0, 0] = np.float32(np.nan), -np.float32(np.nan)
    WR.check(a, b, True)
    WR.check(a, b, False)
    a[0, 1, 0], b[0, 1, 0] = np.float32(np.inf), -np.float32(np.inf)
    for exact in (True, False):
        with pytest.raises(AssertionError):
            WR.check(a, b, exact)
        with pytest.raises(AssertionError):
            WR.check(a, ref, exact)
