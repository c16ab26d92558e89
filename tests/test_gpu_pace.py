"""Pacing of the flagship kernel's voice waves (csrc/wave.hip.h pace_*, render_voice_chain_track; notes/r10.md): a wave's issue priority
follows its lead over the other voice waves of its SIMD.  Priority decides WHEN an instruction issues, never what it computes, so the
contract is: no bit changes — of frames, mix, statistics, or the voice state read back afterwards.  Needs a real MI355X (-m gpu).

Each case of tests/pace_driver.py runs in two processes, one after the other, SRACK_PACE=1 (the default) and SRACK_PACE=0 (the open-loop
priority ramp: the library as it was), and the two .npz files must agree bit for bit.  The frames are also held to the CPU oracle —
exact mode bit for bit, default mode at the suite's 1e-5 — so that "both wrong alike" does not pass.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import srack_pkg
from tests.test_gpu_flagship_shapes import check_frames, check_mix

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pace_driver  # noqa: E402


@pytest.fixture(scope="module")
def S():
    S = srack_pkg.load()
    assert S.device_count() > 0, "no GPU visible: the render path has no CPU fallback"
    return S


def run(case, flags, pace, tmp_path):
    out = os.path.join(tmp_path, f"{case}_{flags}_{pace}.npz")
    env = dict(os.environ, SRACK_PACE=str(pace))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pace_driver.py"), case, str(flags), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(out)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def both(case, flags, tmp_path):
    on, off = run(case, flags, 1, tmp_path), run(case, flags, 0, tmp_path)
    assert sorted(on.files) == sorted(off.files)
    for k in on.files:
        if k != "infos":
            np.testing.assert_array_equal(bits(on[k]), bits(off[k]), err_msg=k)
    for d in (on, off):
        assert all("kernel=render_voice_chain_track" in str(i) for i in d["infos"]), d["infos"]
    # (srack_render_info names the tuning variables a process carries: each child did read the knob it was given)
    assert all("SRACK_PACE=1" in str(i) for i in on["infos"]) and all("SRACK_PACE=0" in str(i) for i in off["infos"])
    state = [k for k in on.files if "_osc_pos" in k or "_vcf_" in k]
    assert len(state) == 9 * len(pace_driver.CASES[case][0])
    return on


def oracle_frames(S, oracle, V, T, pick=None, audible=True):
    o = oracle.OraclePatch(48000, 1024, 2)
    ids, over = pace_driver.p1(o, S, V)
    if pick is not None:
        over = [(m, f, v[pick]) for m, f, v in over]
    ref, _ = o.render_batch(V if pick is None else len(pick), T, over, threads=8)
    assert not audible or np.abs(ref[0]).max() > 0.05, "oracle render is silent"
    return ref[0]


CASES = [("small", 0), ("chunks", 0), ("chunks", 1), ("two", 0)]


@pytest.mark.parametrize("case,flags", CASES, ids=[f"{c}-{'exact' if f else 'default'}" for c, f in CASES])
def test_pacing_changes_no_bit(S, oracle, tmp_path, case, flags):
    on = both(case, flags, tmp_path)
    voices, T, calls = pace_driver.CASES[case]
    for k, V in enumerate(voices):
        # (the 100 samples of "small" end before the gate first opens: the VCA's output is 0.0 throughout, and what the case holds is
        # the state the oscillators and filters ran to behind it)
        ref = oracle_frames(S, oracle, V, calls * T, audible=case != "small")
        assert np.unique(on[f"p{k}_osc_pos"]).size > V // 2 and np.abs(on[f"p{k}_vcf_B0"]).max() > 0, "the voices did not run"
        for c in range(calls):   # a later call continues the first
            fr = on[f"p{k}_fr{c}"]
            assert fr.shape == (T, V)
            check_frames(fr, ref[c * T:(c + 1) * T], flags & 1)
            scale = np.abs(fr.astype(np.float64)).sum(axis=1)
            check_mix(on[f"p{k}_mx{c}"][0], fr.astype(np.float64).sum(axis=1), scale)


def test_pacing_with_late_joiners_changes_no_bit(S, oracle, tmp_path):
    """4 097 x 64 + 5 voices: four waves per SIMD and two more, which join their groups when a first wave has ended."""
    on = both("grid", 0, tmp_path)
    (V,), T, _ = pace_driver.CASES["grid"]
    pick = pace_driver.grid_pick(V)
    check_frames(on["p0_fr0"], oracle_frames(S, oracle, V, T, pick), False)
    check_mix(on["p0_mx0"][0], on["p0_own0"], on["p0_scale0"])


def test_pacing_in_the_statistics_variant_changes_no_bit(S, oracle, tmp_path):
    on = both("stats", 0, tmp_path)
    (V,), T, _ = pace_driver.CASES["stats"]
    st = on["p0_st0"]
    assert st.shape == (1, S.STAT_COUNT, V)   # all six fields went through the bit-for-bit comparison above
    fr = on["p0_fr0"]
    check_frames(fr, oracle_frames(S, oracle, V, T), False)
    np.testing.assert_array_equal(st[0, S.STAT_PEAK_POS], np.maximum(fr.max(axis=0), 0.0).astype(np.float64))
    assert (st[0, S.STAT_SUM_SQ] > 0).all()
