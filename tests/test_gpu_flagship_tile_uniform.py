"""The flagship kernel's wave-uniform work done once per tile (render_voice_chain_track, csrc/fused.hip.h; notes/r15.md): the envelope
arrives eight samples per scalar load, and a full 32-sample tile whose envelope values are all > 0 runs a copy of the samples without
the VCA's gate, (negative || cv > 0) ? y * cv : 0.  Both are meant to change no bit.  Needs a real MI355X (-m gpu).

Voices: 1, 2, 63, 64, 65 and 200 (one voice alone renders through render_voice_chain — nothing of it is voice-invariant, so it has no
envelope track —; it is rendered and compared all the same, and two voices are the fewest the flagship takes).  Calls: 1, 31, 32, 33,
95 and 4 103 samples, then a session of 7, 243, 1 024 and 33, every call continuing the one before, the output modes taking turns;
the statistics variant with calls of its own.

Each envelope kind of tests/tile_uniform_driver.py runs in two processes, one after the other, SRACK_TILE_PLAIN=1 (the default) and
SRACK_TILE_PLAIN=0 (every tile keeps the gate), and the two .npz files must agree bit for bit: frames and mix as uint32, so that the sign
of a zero counts, the statistics, and the voice state read back.  The renders are also held to the CPU oracle — exact mode bit for bit,
default mode at the suite's 1e-5 — so that "both wrong alike" does not pass.  The kinds are envelopes that change class INSIDE a tile
(to 0.0 in mid-gate, below 0.0, `negative` set for every third voice only): from the oracle's own envelope track each kind is shown to
hold, among the full tiles of its calls, at least one with both classes and at least one all > 0.

Against a library from before the change SRACK_TILE_PLAIN is an unknown variable that nothing reads: the two processes then run the
same code, and the comparison passes trivially.
"""
import functools
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
import tile_uniform_driver as D  # noqa: E402

TILE = 32
KINDS = sorted(D.KINDS)


@pytest.fixture(scope="module")
def S():
    S = srack_pkg.load()
    assert S.device_count() > 0, "no GPU visible: the render path has no CPU fallback"
    return S


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


@functools.lru_cache(maxsize=None)
def rendered(kind, plain, tmp):
    """The kind's .npz from a child process with SRACK_TILE_PLAIN=plain (once per module: both modes' cases read it)."""
    out = os.path.join(tmp, f"{kind}_{plain}.npz")
    env = dict(os.environ, SRACK_TILE_PLAIN=str(plain))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tile_uniform_driver.py"), kind, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(out)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("tile_uniform"))


@functools.lru_cache(maxsize=None)
def reference(kind, V, total):
    """The oracle's frames [T][V] of the kind's patch (computed once, never written to)."""
    from oracle import oracle as O
    S = srack_pkg.load()
    o = O.OraclePatch(48000, 1024, 2)
    _, over = D.build(o, S, kind, V)
    ref, _ = o.render_batch(V, total, over, threads=8)
    ref[0].setflags(write=False)
    return ref[0]


@functools.lru_cache(maxsize=None)
def envelope(kind, total):
    """The oracle's envelope track (the ADSR's output wire; the same for every voice)."""
    from oracle import oracle as O
    S = srack_pkg.load()
    o = O.OraclePatch(48000, 1024, 2)
    ids, _ = D.build(o, S, kind, 1)
    _, env = o.render(total, tap=(ids["adsr"], 0))
    return env


def full_tiles(calls):
    """(first sample, absolute) of every full tile of a sequence of calls: tiles count from a call's first sample (the library's
    launches within a call are whole numbers of tiles long, but for the last)."""
    at, out = 0, []
    for n in calls:
        out += [at + t for t in range(0, n - TILE + 1, TILE)]
        at += n
    return out


def tile_census(env, calls):
    """-> (tiles with both classes, tiles all > 0, tiles with none > 0) among the full tiles; class = the kernel's own predicate on the bits"""
    pos = (env.view(np.uint32) - np.uint32(1)) < np.uint32(0x7f800000)
    k = [int(pos[t:t + TILE].sum()) for t in full_tiles(calls)]
    return sum(0 < x < TILE for x in k), sum(x == TILE for x in k), sum(x == 0 for x in k)


@pytest.mark.parametrize("kind", KINDS)
def test_envelope_changes_class_inside_a_tile(oracle, kind):
    """What the cases below rest on, from the oracle's track alone (no GPU work, but of no use without the cases)."""
    for calls in (D.CALLS, D.STATS_CALLS):
        env = envelope(kind, sum(D.CALLS))[:sum(calls)]
        both, plain, none = tile_census(env, calls)
        assert both >= 1 and plain >= 1, (kind, both, plain, none)
        if kind == "sustain0":   # reaches exactly 0.0 behind a run of values > 0, inside a tile
            z = np.flatnonzero((env[1:] == 0.0) & (env[:-1] > 0.0)) + 1
            assert any(t < i < t + TILE and (env[t:i] > 0).any() for t in full_tiles(calls) for i in z)
        if kind.startswith("negative"):
            assert any((env[t:t + TILE] < 0).any() and (env[t:t + TILE] > 0).any() for t in full_tiles(calls))


def check_against_oracle(got_fr, got_mx, ref, flags):
    scale = np.abs(ref.astype(np.float64)).sum(axis=1)
    if got_fr is not None:
        assert got_fr.shape == ref.shape
        check_frames(got_fr, ref, flags & 1)
    if got_mx is not None:
        for ch in range(got_mx.shape[0]):
            check_mix(got_mx[ch], ref.astype(np.float64).sum(axis=1), scale)
            if got_fr is not None:
                check_mix(got_mx[ch], got_fr.astype(np.float64).sum(axis=1), scale)


@pytest.mark.parametrize("flags", [0, 1], ids=["default", "exact"])
@pytest.mark.parametrize("kind", KINDS)
def test_plain_tiles_change_no_bit(S, oracle, tmp, kind, flags):
    on, off = rendered(kind, 1, tmp), rendered(kind, 0, tmp)
    assert sorted(on.files) == sorted(off.files)
    mine = [k for k in on.files if k.startswith(f"x{flags}_")]
    n_state = 9 * (len(D.VOICES) + len(D.STATS_VOICES))
    assert len([k for k in mine if "_osc_pos" in k or "_vcf_" in k]) == n_state
    for k in mine:
        if not k.endswith("_infos"):
            np.testing.assert_array_equal(bits(on[k]), bits(off[k]), err_msg=k)
    for d, v in ((on, 1), (off, 0)):
        for k in mine:
            if k.endswith("_infos"):
                # (one voice alone has no voice-invariant part to hoist: no envelope track, and render_voice_chain renders it)
                want = "kernel=render_voice_chain" if k == f"x{flags}_v1_infos" else "kernel=render_voice_chain_track"
                assert len(d[k]) in (len(D.CALLS), len(D.STATS_CALLS)) and all(str(i).endswith(want) for i in d[k]), (k, d[k])
                assert all(f"SRACK_TILE_PLAIN={v}" in str(i) for i in d[k])   # each child did carry the knob it was given
    for j, V in enumerate(D.VOICES):
        ref, at = reference(kind, V, sum(D.CALLS)), 0
        if kind == "finite":
            assert np.abs(ref).max() > 0.05, "oracle render is silent"
        for c, n in enumerate(D.CALLS):
            what = D.mode_of(j, c)
            fr = on[f"x{flags}_v{V}_c{c}_fr"] if "f" in what else None
            mx = on[f"x{flags}_v{V}_c{c}_mx"] if "m" in what else None
            assert (f"x{flags}_v{V}_c{c}_fr" in on.files) == ("f" in what) and (f"x{flags}_v{V}_c{c}_mx" in on.files) == ("m" in what)
            check_against_oracle(fr, mx, ref[at:at + n], flags)
            at += n
        assert np.unique(on[f"x{flags}_v{V}_osc_pos"]).size > V // 2 and np.abs(on[f"x{flags}_v{V}_vcf_B0"]).max() > 0, "the voices did not run"
    for V in D.STATS_VOICES:
        ref, at = reference(kind, V, sum(D.CALLS)), 0
        for c, n in enumerate(D.STATS_CALLS):
            fr, st = on[f"x{flags}_s{V}_c{c}_fr"], on[f"x{flags}_s{V}_c{c}_st"]
            check_against_oracle(fr, on[f"x{flags}_s{V}_c{c}_mx"], ref[at:at + n], flags)
            assert st.shape == (1, S.STAT_COUNT, V)
            np.testing.assert_array_equal(st[0, S.STAT_PEAK_POS], np.maximum(fr.max(axis=0), 0.0).astype(np.float64))
            at += n
