"""Kernel hand-offs (notes/r26.md): a patch's running state lives on the device between calls, every kernel family has a prologue of its
own that loads it and an epilogue of its own that stores it — and every other test has the same kernel on both sides of a cut.  Here the
next call is another kernel's:

  part A   the same flattened program: the launch-policy bits (16, 32), the call's length (the FM pair's ring / time-parallel kernels) or
           the output mode pick another kernel, which continues on the table the last one wrote;
  part B   srack_patch_keep_state and a change of the bits that re-flatten (exact <-> default, fused <-> general, hoisted <-> per voice,
           pipelined <-> one unit), or an edit that moves modules out of the control program: the state is read back, carried into another
           program's rows (another encoding, another side) and the rings and reverb lines are transplanted.

Per call: the kernel srack_render_info names (tests/handoff_ref.py, kernel_name), the frames against the oracle — one uninterrupted
render_batch of the script's whole length for a flags-only script, a stateful OraclePatch per sampled voice for an edit script — bit for
bit while every call so far was exact, through the suite's contract (1e-5 relative to max(|ref|, 1)) otherwise; after a call that ends on a
multiple of buffer_size, every state field of every module against the stateful oracle, bit for bit (after default-mode calls: the phase
of the FM pair's exact-by-default modulator).  tests/test_handoff_host.py holds the guards: at every cut, losing the state would show in
every voice."""
import numpy as np
import pytest

import srack_pkg
from tests import handoff_ref as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    S = srack_pkg.load()
    assert S.device_count() > 0, "no GPU visible: the render path has no CPU fallback"
    return S


def render_call(p, n, flags, mix):
    """one srack_render -> (frames expanded to [channels][n][V], mix or None)"""
    fr, mx = p.render(n, frames=True, mix=mix, flags=flags)
    _, planes = p.planes()
    out = np.zeros((p.channels, n, p.n_voices), dtype=np.float32)
    for c, pl in enumerate(planes):
        if pl >= 0:
            out[c] = fr[pl]
    return out, mx


def check_state(S, p, ids, case, i, exact):
    want = H.oracle_state(case, i)
    for (m, f), per_voice in sorted(want.items()):
        if not exact and (m, f) != (ids.get("osc_m"), S.OSC_POS):
            continue   # default arithmetic: held to the oracle through the next call's samples
        got = p.get_voice_field(m, f)
        for v, w in per_voice.items():
            same = np.float64(got[v]).view(np.uint64) == np.float64(w).view(np.uint64) or (np.isnan(got[v]) and np.isnan(w))
            assert same, f"{case.id}: after op {i}, module {m} field {f} voice {v}: {got[v]!r}, the oracle holds {w!r}"


def run(S, case):
    p, ids, sp = H.make_patch(S, case.patch, case.B, case.V, keep=case.part == "B")
    ref, voices = H.reference(case)
    names = H.kernels(case)
    t = k = 0
    worst, seen = 0.0, []
    for i, op in enumerate(case.ops):
        if op[0] == "e":
            p.set_voice_field(*sp.edit(ids))
            continue
        _, n, flags, mix = op
        got, mx = render_call(p, n, flags, mix)
        seen.append(p.info().split("kernel=")[-1])
        what = f"{case.id}: call {k} ({n} samples, flags {flags}, {seen[-1]})"
        assert seen[-1] == names[k], f"{what}: the table says {names[k]}; {p.info()}"
        if case.patch == "loop":   # the route itself: the loop (and its ring) per voice under NO_UNIFORM_HOIST, in a control unit without it
            assert (" + ctl[" in p.info()) == (not flags & H.NO_HOIST), p.info()
        exact = H.all_exact(case, i)
        err = H.check(got[:, :, voices], ref[:, t:t + n], exact, what)
        worst = max(worst, err)
        if mx is not None:   # the mix is the call's own frames summed (as __graft_entry__.smoke holds it)
            own = got.astype(np.float64)
            assert (np.abs(mx - own.sum(axis=2)) <= 2e-5 * np.maximum(np.abs(own).sum(axis=2), 1.0)).all(), what
        t += n
        if t % sp.B == 0 and k >= case.state_from and (exact or H.modulator_exact(case, i)):
            check_state(S, p, ids, case, i, exact)
        k += 1
    print(f"handoff {case.id} | {' -> '.join(seen)} | max rel err {worst:.2e}")


@pytest.mark.parametrize("case", H.CASES_A, ids=[k.id for k in H.CASES_A])
def test_another_kernel_continues_the_same_program(S, oracle, case):
    run(S, case)


@pytest.mark.parametrize("case", H.CASES_B, ids=[k.id for k in H.CASES_B])
def test_a_re_flatten_under_keep_state_hands_the_state_to_another_kernel(S, oracle, case):
    run(S, case)
