"""The guards of tests/test_gpu_handoff.py, on the oracle alone (notes/r26.md): a hand-off test is only worth something if losing the
state at the cut would show.  For every script and every cut the reference after the cut differs from the reference restarted there
by more than 1e-2 somewhere in EVERY voice, and every voice peaks above 0.25; the checker fails on two restarted renders glued
together, in its bit mode and in its contract mode; the table covers what the issue lists and no script's neighbouring calls share a kernel."""
import numpy as np
import pytest

from tests import handoff_ref as H


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


def _ids(cases):
    return [k.id for k in cases]


def test_case_ids_are_unique_and_the_table_is_whole():
    assert len(set(_ids(H.CASES))) == len(H.CASES)
    flagseq = lambda patch, B: {tuple(op[2] for op in k.ops if op[0] == "r") for k in H.CASES_B if k.patch == patch and k.B == B and not H.has_edit(k)}
    want_p1 = [(1, 5, 1), (1, 3, 1), (1, 35, 1), (9, 1), (0, 4, 0), (0, 2, 0), (0, 34), (1, 0, 1), (0, 1, 0)]
    for seq in want_p1 + [(5, 1, 5), (3, 1, 3), (35, 1, 35), (1, 9), (4, 0, 4), (2, 0, 2), (34, 0)]:
        assert seq in flagseq("p1", 64), seq
    for patch in ("p3", "p4"):
        assert flagseq(patch, 1024) == {(1, 3, 35, 1), (1, 35, 3, 1), (0, 1, 0), (1, 0, 1)}
    for B in (1, 8, 64, 1024):
        assert flagseq("p2", B) == {(1, 3, 1), (3, 1, 3), (1, 35), (35, 1), (64, 0, 64), (0, 64, 0), (0, 1, 0), (1, 0, 1)}
    assert flagseq("p2_reverb", 64) == {(1, 3, 1), (3, 1, 3), (0, 2, 0), (2, 0, 2)}
    for B in (8, 64):   # per voice -> voice-invariant and back: only a loop of stateless modules gets there (notes/r26.md)
        assert flagseq("loop", B) == {(4, 0, 4), (0, 4, 0), (5, 1, 5), (1, 5, 1)}
    edits = {(k.patch, k.B, k.ops[0][2]) for k in H.CASES_B if H.has_edit(k)}
    assert edits == {(p, B, f) for f in (1, 3, 0) for p, B in (("p1", 64), ("p2_flat", 8), ("p2_flat", 64), ("p2_reverb_flat", 64))}


@pytest.mark.parametrize("case", H.CASES_A, ids=_ids(H.CASES_A))
def test_part_a_scripts_share_the_program_and_change_the_kernel(case):
    calls = H.renders(case)
    assert len({f & H.REFLATTEN for _, _, _, f, _, _ in calls}) == 1, "a part A script never re-flattens"
    names = H.kernels(case)
    for (a, na), (b, nb) in zip(zip(calls, names), zip(calls[1:], names[1:])):
        # (the calls of a tick session repeat one kind of call on purpose: the hand-offs are in front of it and behind it)
        assert na != nb or a[2:5] == b[2:5], (case.id, na, nb)
    assert len(set(names)) > 1


@pytest.mark.parametrize("case", H.CASES_B, ids=_ids(H.CASES_B))
def test_part_b_scripts_re_flatten_or_change_the_kernel_at_every_cut(case):
    calls, names = H.renders(case), H.kernels(case)
    for (a, na), (b, nb) in zip(zip(calls, names), zip(calls[1:], names[1:])):
        assert (a[3] & H.REFLATTEN) != (b[3] & H.REFLATTEN) or a[5] != b[5] or na != nb, case.id   # (3 -> 35: the same program, the generated kernel)
    assert any((a[3] & H.REFLATTEN) != (b[3] & H.REFLATTEN) or a[5] != b[5] for a, b in zip(calls, calls[1:]))
    sp_B = H.spec_B(case)
    assert all(n % sp_B == 0 for _, _, n, _, _, _ in calls), "state is compared after every call: cuts on multiples of buffer_size"


@pytest.mark.parametrize("case", H.CASES, ids=_ids(H.CASES))
def test_losing_the_state_at_a_cut_would_show_in_every_voice(case):
    figures = H.guard_figures(case)
    assert len(figures) == len(H.renders(case)) - 1
    print(case.id, " ".join(f"cut {t}: diff {d:.3g} peak {p:.3g}" for t, d, p in figures))
    for t, diff, peak in figures:
        assert diff > H.GUARD_DIFF, (case.id, t, diff)
        assert peak > H.GUARD_PEAK, (case.id, t, peak)


def _glued(case):
    """two restarted renders in place of a continued one, cut at the script's first hand-off"""
    ref, _ = H.reference(case)
    cut = H.renders(case)[1][1]
    return np.concatenate([ref[:, :cut], H.restarted(case, cut)[:, :ref.shape[1] - cut]], axis=1), ref


@pytest.mark.parametrize("case", [k for k in H.CASES if k.id in ("p1_poly-f0-special", "p2-B256-keep-ragged", "p3-B1024-keep-0-1-0", "p2_flat-B8-edit-f1")],
                         ids=lambda k: k.id)
def test_the_checker_fails_on_two_restarted_renders_glued_together(case):
    glued, ref = _glued(case)
    for exact in (True, False):
        H.check(ref.copy(), ref, exact)             # ... and passes on the continued one
        with pytest.raises(AssertionError):
            H.check(glued, ref, exact)


def test_the_checker_tells_an_ulp_and_takes_a_nan_for_a_nan():
    ref = np.linspace(-1, 1, 24, dtype=np.float32).reshape(2, 4, 3)
    off = ref.copy()
    off[1, 2, 1] = np.nextafter(off[1, 2, 1], np.float32(2))
    with pytest.raises(AssertionError):
        H.check(off, ref, True)
    assert H.check(off, ref, False) < 1e-6
    a, b = ref.copy(), ref.copy()
    a[0, 0, 0], b[0, 0, 0] = np.float32(np.nan), -np.float32(np.nan)
    H.check(a, b, True)
    with pytest.raises(AssertionError):
        H.check(a, ref, True)
    with pytest.raises(AssertionError):   # the contract mode wants finite renders
        H.check(a, b, False)
