"""The NumPy statement of srack_buses_master (include/srack_hip.h): the three-level sum over the buses and the sequential statistics.

The arrays are f32 and vectorised over TIME only; buses, runs and blocks are explicit Python loops starting from zeros, so every
addition and every product is one IEEE f32 operation with one rounding, in exactly the order the header fixes:
    run r   = ((+0.0 + p[64r]) + p[64r+1]) + ...     its up to 64 buses, ascending        p[b] = fl32(gain[b][c] * rows[b][c])
    block k = +0.0 + its up to 64 run sums, ascending
    master  = +0.0 + the up to 16 block sums, ascending
The statistics are the sequential loop of srack_render_stats in Python floats (f64)."""
import math

import numpy as np

RUN, BLOCK = 64, 64
STAT_SUM, STAT_SUM_SQ, STAT_PEAK_POS, STAT_PEAK_NEG, STAT_NONFINITE, STAT_CLIPPED, STAT_COUNT = range(7)


def _products(rows, gain, b, used):
    with np.errstate(over="ignore", invalid="ignore"):
        return gain[b, :used, None] * rows[b, :used]  # f32 * f32 -> f32: one rounding


def master_tree(rows, gain=None):
    """rows f32 [n_buses][row_channels][T], gain f32 [n_buses][2] (None: 1.0) -> f32 [2][T]; channel 1 is +0.0 for one row channel"""
    rows = np.asarray(rows)
    assert rows.dtype == np.float32 and rows.ndim == 3
    n_buses, rc, T = rows.shape
    gain = np.ones((n_buses, 2), dtype=np.float32) if gain is None else np.asarray(gain)
    assert gain.dtype == np.float32 and gain.shape == (n_buses, 2)
    used = min(rc, 2)
    out = np.zeros((2, T), dtype=np.float32)
    master = np.zeros((used, T), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k0 in range(0, n_buses, RUN * BLOCK):
            block = np.zeros((used, T), dtype=np.float32)
            for r0 in range(k0, min(n_buses, k0 + RUN * BLOCK), RUN):
                run = np.zeros((used, T), dtype=np.float32)
                for b in range(r0, min(n_buses, r0 + RUN)):
                    run = run + _products(rows, gain, b, used)
                block = block + run
            master = master + block
    assert master.dtype == np.float32
    out[:used] = master
    return out


def master_sequential(rows, gain=None):
    """the plain sequential sum over the buses: what the tree coincides with up to 65 buses, and what it must differ from beyond"""
    rows = np.asarray(rows)
    n_buses, rc, T = rows.shape
    gain = np.ones((n_buses, 2), dtype=np.float32) if gain is None else np.asarray(gain)
    used = min(rc, 2)
    out = np.zeros((2, T), dtype=np.float32)
    acc = np.zeros((used, T), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(n_buses):
            acc = acc + _products(rows, gain, b, used)
    out[:used] = acc
    return out


def stats_sequential(master, stats=None, channels=2):
    """master f32 [2][T] -> f64 [2][STAT_COUNT], continued from `stats` (None: zeros); rows of channels >= `channels` are left alone"""
    st = np.zeros((2, STAT_COUNT), dtype=np.float64) if stats is None else np.array(stats, dtype=np.float64)
    for c in range(channels):
        s, sq = float(st[c, STAT_SUM]), float(st[c, STAT_SUM_SQ])
        pp, pn = float(np.float32(st[c, STAT_PEAK_POS])), float(np.float32(st[c, STAT_PEAK_NEG]))
        nonfinite = clipped = 0
        for x in np.asarray(master[c], dtype=np.float32).astype(np.float64).tolist():
            if not math.isfinite(x):
                nonfinite += 1
                continue
            s += x
            sq += x * x
            if x > pp:
                pp = x
            if -x > pn:
                pn = -x
            if abs(x) > 1.0:
                clipped += 1
        st[c] = (s, sq, pp, pn, st[c, STAT_NONFINITE] + nonfinite, st[c, STAT_CLIPPED] + clipped)
    return st


def case_inputs(n_buses, T, seed=1701, row_channels=2):
    """rows: uniform(-1, 1) * 2^k, k uniform in -12 .. 0; gains: uniform(-2, 2)"""
    rng = np.random.default_rng(seed)
    rows = (rng.uniform(-1.0, 1.0, (n_buses, row_channels, T)) * np.exp2(rng.integers(-12, 1, (n_buses, row_channels, 1)))).astype(np.float32)
    gain = rng.uniform(-2.0, 2.0, (n_buses, 2)).astype(np.float32)
    return rows, gain


def same_bits(a, b):
    """boolean array: equal bit for bit, or both NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
