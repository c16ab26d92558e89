"""The console's chained reference (tests/console_ref.py), on the CPU: is it worth comparing a device with?

The GPU tests (tests/test_gpu_console.py) hold the device to this reference bit for bit, so a reference that is silent, that hands its
input on, or that an edit does not change would let a wrong device pass.  The guards, on the reference alone:
  * every intermediate is finite;
  * the master is audible: max |x| > 1e-3 and more than a quarter of its samples non-zero;
  * each stage's output differs from its input on at least a quarter of the samples of the buses it is enabled on;
  * every edit of the stream tests shows: the first cut behind it, rendered with and without it, differs on at least 1/16 of the master's
    samples;
  * cut and uncut renders are the same bits (the reference's own state passing).

The figures (printed by each test; seeds console_ref.SEED = 2101 and SEED3 = 2103):
  70 buses x 2 channels x 3000 at 48 kHz: non-zero master 0.9997, max |master| 8.5; output differs from input on 0.52 (sends), 0.9997
  (reverb), 0.63 (VCA), 0.96 (filter) of the samples.
  5 buses x 3 channels x 400 at 2 kHz (the reverb's lines are 10 .. 74 slots there and wrap many times within 400 samples; at 48 kHz
  not one echo would have arrived): non-zero master 0.9925, max |master| 0.65; 0.45 (sends), 0.97 (reverb), 0.66 (VCA), 0.96 (filter).
  The edits: see test_every_edit_shows."""
import functools

import numpy as np
import pytest

from tests import console_ref as CR

CUTS3 = (1, 63, 64, 65, 207)


@functools.lru_cache(maxsize=None)
def big():
    rows, ctl, s = CR.case()
    whole, _, _ = CR.render(rows, ctl, s, [rows.shape[2]])
    return rows, ctl, s, whole


def assert_worth_comparing(rows, s, out, what, cuts=None):
    for key in CR.KEYS:
        assert np.isfinite(out[key]).all(), f"{what}: {key} is not finite"
    assert np.isfinite(out["stats"]).all()
    m = out["master"]
    nz = np.count_nonzero(m) / m.size
    fr = CR.stage_fractions(rows, out, s, cuts)
    print(f"{what}: master max {np.abs(m).max():.3f}, non-zero {nz:.4f}; output differs from input: {fr}")
    assert np.abs(m).max() > 1e-3 and nz > 0.25, f"{what}: the master is (nearly) silent"
    for stage, f in fr.items():
        assert f >= 0.25, f"{what}: the {stage} hand their input on ({f:.3f} of the samples differ)"


def test_the_case_spans_every_grouping():
    rows, ctl, s, _ = big()
    assert s.n_buses == 70 and rows.shape == (70, 2, 3000) and sum(CR.CUTS) == 3000
    assert set(s.send_dst[:4 * 66]) == {66, 67, 68, 69} and np.bincount(s.send_dst, minlength=70)[66:].min() >= 66, "the aux buses are fed by all others"
    assert len(np.unique(s.send_gain)) > 100 and (s.send_gain == 1).any()
    assert np.flatnonzero(s.rv_enabled).tolist() == [66, 67]
    assert 30 <= s.vcf_enabled.sum() <= 40 and set(s.vcf_port[s.vcf_enabled != 0]) == {0, 1, 2}
    assert all(np.count_nonzero(s.vca_mode == m) >= 10 for m in (0, 1, 2))
    # the scratch of the sends and of the master is re-allocated while the previous call is pending: a cut longer than all before it
    assert sum(CR.CUTS[k] > max(CR.CUTS[:k]) for k in range(1, len(CR.CUTS))) >= 1


def test_the_reference_is_worth_comparing_with():
    rows, ctl, s, whole = big()
    assert_worth_comparing(rows, s, whole, "70 buses")


def test_cut_equals_uncut():
    rows, ctl, s, whole = big()
    cut, states, _ = CR.render(rows, ctl, s, CR.CUTS)
    for key in CR.KEYS:
        assert CR.same_bits(cut[key], whole[key]).all(), key
    assert (cut["stats"] == whole["stats"]).all()
    _, one, _ = CR.render(rows, ctl, s, [3000])
    assert CR.same_bits(states[-1].vca, one[-1].vca).all() and CR.same_bits(states[-1].vcf, one[-1].vcf).all()
    assert not CR.same_bits(states[-1].vca, CR.State(70, 48000).vca).all() and np.count_nonzero(states[-1].vcf) > 300, "the state is meant to have moved"


@pytest.mark.parametrize("run", ["grow", "primed"])
def test_every_edit_shows(run):
    """The fraction of the master's samples of the first cut behind the edit that differ with and without it (the bound is 1/16):
    grow:   vca modes 1.0, filter enables more 1.0, reverb swap 0.9886, sends longer 1.0, filter disables some 1.0
    primed: vca sliders 0.9921, filter sliders 1.0, reverb slider 1.0, master gains 1.0, vca reset 1.0"""
    rows, ctl, s, _ = big()
    edits = CR.edits(s, run)
    assert {e.stage for e in CR.edits(s, "grow") + CR.edits(s, "primed")} == set(CR.STAGES), "every stage gets an edit"
    assert len({e.cut for e in edits}) == len(edits) and CR.STATE_READS[run] not in {e.cut for e in edits}, "one host action per boundary"
    out, states, settings = CR.render(rows, ctl, s, CR.CUTS, edits)
    assert_worth_comparing(rows, settings, out, run, CR.CUTS)   # (every cut counted with the settings it ran with)
    at = np.concatenate([[0], np.cumsum(CR.CUTS)])
    for e in edits:
        k = e.cut
        s0, st0 = CR.apply(edits, k, settings[k - 1], states[k - 1], skip=e)
        without, _ = CR.chain(rows[:, :, at[k]:at[k + 1]], ctl[:, at[k]:at[k + 1]], s0, st0)
        f = CR.fraction_differing(without["master"], out["master"][:, at[k]:at[k + 1]])
        print(f"{run}: {e.name} in front of cut {k} ({CR.CUTS[k]} samples): {f:.4f} of the master's samples differ")
        assert f >= 1 / 16, f"{e.name}: the edit does not show ({f:.4f})"
    # the state the stream tests read back in flight is not the fresh one
    k = CR.STATE_READS[run] - 1
    assert not CR.same_bits(states[k].vca, CR.State(70, 48000).vca).all() and np.count_nonzero(states[k].vcf) > 100


def test_three_channels():
    rows, ctl, s = CR.case(n_buses=5, channels=3, T=400, seed=CR.SEED3, n_aux=2, rate=2000)
    whole, _, _ = CR.render(rows, ctl, s, [400])
    assert_worth_comparing(rows, s, whole, "5 buses, 3 channels")
    assert whole["sent"].shape == (5, 3, 400) and whole["fx"].shape == (5, 2, 400) and not whole["sent"][:, 2].any() and rows[:, 2].any()
    cut, _, _ = CR.render(rows, ctl, s, CUTS3)
    for key in CR.KEYS:
        assert CR.same_bits(cut[key], whole[key]).all(), key
