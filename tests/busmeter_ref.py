"""The NumPy statement of srack_buses_meter (include/srack_hip.h): windowed records and totals per (bus, channel) row, continued from
given buffers.

Every row is master_ref.stats_sequential's literal loop — the sequential f64 loop of srack_render_stats in Python floats — applied to
the stretch of the row that falls into one window, continued from what the record holds; the totals are the same loop over the whole
row.  Two deliberately DIFFERENT associations of the same sums stand next to it (reversed order; partial sums per stream tile of 64,
added in order): the tests' guards use them to show that the case inputs tell the orders apart."""
import math

import numpy as np

from tests import master_ref as M

STAT_SUM, STAT_SUM_SQ, STAT_PEAK_POS, STAT_PEAK_NEG, STAT_NONFINITE, STAT_CLIPPED, STAT_COUNT = M.STAT_SUM, M.STAT_SUM_SQ, M.STAT_PEAK_POS, M.STAT_PEAK_NEG, M.STAT_NONFINITE, M.STAT_CLIPPED, M.STAT_COUNT
MIN_WINDOW = 64
TILE = 64


def _row(x, rec, pos=0):
    """one row's samples (from stream position `pos` on) into one record f64 [STAT_COUNT] -> the continued record;
    master_ref.stats_sequential on channel 0 of a pair"""
    st = np.zeros((2, STAT_COUNT), dtype=np.float64)
    st[0] = rec
    return M.stats_sequential(np.stack([x, x]), st, channels=1)[0]


def n_windows_for(first, T, window):
    return max(1, -(-(first + T) // window))


def windows_touched(first, T, window):
    """the records a call of T >= 1 samples at `first` reads and writes: floor(first / window) .. floor((first + T - 1) / window)"""
    return range(first // window, (first + T - 1) // window + 1)


def bus_meter(rows, window=None, first=0, levels=None, totals=None, row_fn=_row):
    """rows f32 [n_buses][row_channels][T] -> (levels f64 [n_windows][STAT_COUNT][n_buses][2] or None, totals f64 [STAT_COUNT][n_buses][2]
    or None), continued from `levels` / `totals`.  window None: no levels.  levels None with a window: zeros over the windows the call
    needs.  totals None: zeros; False: no totals.  Entries of channel 1 are left alone for one row channel; so is every record outside
    windows_touched()."""
    rows = np.asarray(rows)
    assert rows.dtype == np.float32 and rows.ndim == 3
    n_buses, rc, T = rows.shape
    used = min(rc, 2)
    lv = tt = None
    if window is not None:
        assert window >= MIN_WINDOW
        lv = np.zeros((n_windows_for(first, T, window), STAT_COUNT, n_buses, 2)) if levels is None else np.array(levels, dtype=np.float64, copy=True)
        assert lv.shape[1:] == (STAT_COUNT, n_buses, 2) and first + T <= lv.shape[0] * window
    if totals is not False:
        tt = np.zeros((STAT_COUNT, n_buses, 2)) if totals is None else np.array(totals, dtype=np.float64, copy=True)
        assert tt.shape == (STAT_COUNT, n_buses, 2)
    if T == 0:
        return lv, tt
    for b in range(n_buses):
        for c in range(used):
            x = rows[b, c]
            if tt is not None:
                tt[:, b, c] = row_fn(x, tt[:, b, c], first)
            if lv is not None:
                for k in windows_touched(first, T, window):
                    lo, hi = max(k * window - first, 0), min((k + 1) * window - first, T)
                    lv[k, :, b, c] = row_fn(x[lo:hi], lv[k, :, b, c], first + lo)
    return lv, tt


# ---- two other associations of SUM and SUM_SQ (the guards') ----------------------------------------------------------------------------
def _finite(x):
    return [v for v in np.asarray(x, dtype=np.float32).astype(np.float64).tolist() if math.isfinite(v)]


def row_reversed(x, rec, pos=0):
    """the same record with SUM and SUM_SQ added in reversed sample order"""
    out = _row(x, rec)
    s, sq = float(rec[STAT_SUM]), float(rec[STAT_SUM_SQ])
    for v in reversed(_finite(x)):
        s += v
        sq += v * v
    out[STAT_SUM], out[STAT_SUM_SQ] = s, sq
    return out


def row_tiled(x, rec, pos=0):
    """the same record with SUM and SUM_SQ as partial sums per tile of 64 stream positions, each from zero, added in order"""
    out = _row(x, rec)
    s, sq = float(rec[STAT_SUM]), float(rec[STAT_SUM_SQ])
    x = np.asarray(x, dtype=np.float32)
    cuts = [0] + [t for t in range(TILE - pos % TILE, len(x), TILE)] + [len(x)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        ps = psq = 0.0
        for v in _finite(x[lo:hi]):
            ps += v
            psq += v * v
        s += ps
        sq += psq
    out[STAT_SUM], out[STAT_SUM_SQ] = s, sq
    return out


def case_rows(n_buses, T, seed, row_channels=2):
    """uniform(-2, 2) * 2^k with k drawn PER SAMPLE from -30 .. 0: sums that round in f64, so their order shows (plain uniform(-2, 2)
    rows leave SUM exact in f64 and would prove nothing about order)"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-2.0, 2.0, (n_buses, row_channels, T)) * np.exp2(rng.integers(-30, 1, (n_buses, row_channels, T)))).astype(np.float32)


def same_bits64(a, b):
    """boolean array: f64 words equal bit for bit"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.view(np.uint64) == b.view(np.uint64)
