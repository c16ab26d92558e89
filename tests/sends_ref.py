"""The NumPy statement of srack_buses_send (include/srack_hip.h): per destination bus the master section's three-level sum over its terms.

The terms of destination d: term 0 is (d, through[d]), then the sends i with dst[i] == d in ascending i (a stable grouping of the list).
The arrays are f32 and vectorised over TIME only; destinations, terms, runs and blocks are explicit Python loops starting from zeros, so
every addition and every product is one IEEE f32 operation with one rounding, in exactly the order the header fixes:
    p_k     = fl32(g_k[c] * rows[src_k][c])
    run r   = ((+0.0 + p[64r]) + p[64r+1]) + ...     its up to 64 terms, ascending
    block k = +0.0 + its up to 64 run sums, ascending
    out[d]  = +0.0 + the up to 16 block sums, ascending
The input rows are read, never the output: one call is one level of routing."""
import numpy as np

from tests.master_ref import RUN, BLOCK, case_inputs, same_bits  # noqa: F401  (the tests take them from here)


def grouping(n_buses, dst):
    """-> (n_terms int [n_buses], through term included; order: the send indices grouped by destination ascending, stable)"""
    dst = np.asarray(dst, dtype=np.int64)
    n_terms = np.ones(n_buses, dtype=np.int64)
    feeders = [[] for _ in range(n_buses)]
    for i, d in enumerate(dst.tolist()):
        feeders[d].append(i)
        n_terms[d] += 1
    order = [i for f in feeders for i in f]
    return n_terms, np.array(order, dtype=np.int64)


def n_runs(n_terms):
    return int(sum((int(n) + RUN - 1) // RUN for n in n_terms))


def terms(n_buses, src, dst, gain=None, through=None):
    """-> per destination the list of (source bus, gain f32 [2])"""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    gain = np.ones((len(src), 2), dtype=np.float32) if gain is None else np.asarray(gain)
    through = np.ones((n_buses, 2), dtype=np.float32) if through is None else np.asarray(through)
    assert gain.dtype == np.float32 and gain.shape == (len(src), 2) and through.dtype == np.float32 and through.shape == (n_buses, 2)
    out = [[(d, through[d])] for d in range(n_buses)]
    for i in range(len(src)):
        out[int(dst[i])].append((int(src[i]), gain[i]))
    return out


def _product(rows, s, g, used):
    with np.errstate(over="ignore", invalid="ignore"):
        return g[:used, None] * rows[s, :used]  # f32 * f32 -> f32: one rounding


def send_tree(rows, src, dst, gain=None, through=None, only=None):
    """rows f32 [n_buses][row_channels][T] -> f32 of the same shape; channels beyond the second stay zeros (they are not written).
    only: the destinations to compute (the others stay zeros), None for all"""
    rows = np.asarray(rows)
    assert rows.dtype == np.float32 and rows.ndim == 3
    n_buses, rc, T = rows.shape
    used = min(rc, 2)
    out = np.zeros_like(rows)
    tt = terms(n_buses, src, dst, gain, through)
    with np.errstate(over="ignore", invalid="ignore"):
        want = list(range(n_buses) if only is None else only)
        # the buses without sends, all at once: +0.0 + p_0 (one run of one term, one block, one sum: each further level adds to +0.0 a sum
        # that is not -0.0 and changes no bit)
        alone = np.array([d for d in want if len(tt[d]) == 1], dtype=np.int64)
        if len(alone):
            g0 = np.stack([tt[d][0][1] for d in alone])[:, :used, None]
            out[alone, :used] = np.zeros((used, T), dtype=np.float32) + g0 * rows[alone, :used]
        for d in want:
            t = tt[d]
            if len(t) == 1:
                continue
            total = np.zeros((used, T), dtype=np.float32)
            for k0 in range(0, len(t), RUN * BLOCK):
                block = np.zeros((used, T), dtype=np.float32)
                for r0 in range(k0, min(len(t), k0 + RUN * BLOCK), RUN):
                    run = np.zeros((used, T), dtype=np.float32)
                    for s, g in t[r0:r0 + RUN]:
                        run = run + _product(rows, s, g, used)
                    block = block + run
                total = total + block
            assert total.dtype == np.float32
            out[d, :used] = total
    return out


def send_sequential(rows, src, dst, gain=None, through=None, only=None):
    """the plain sequential sum per destination: what the tree coincides with up to 65 terms, and what it must differ from beyond"""
    rows = np.asarray(rows)
    n_buses, rc, T = rows.shape
    used = min(rc, 2)
    out = np.zeros_like(rows)
    tt = terms(n_buses, src, dst, gain, through)
    with np.errstate(over="ignore", invalid="ignore"):
        for d in (range(n_buses) if only is None else only):
            acc = np.zeros((used, T), dtype=np.float32)
            for s, g in tt[d]:
                acc = acc + _product(rows, s, g, used)
            out[d, :used] = acc
    return out


def all_to_one(n_buses):
    """bus 0 fed by every other bus: (src, dst) of n_buses - 1 sends; bus 0 then has n_buses terms"""
    return np.arange(1, n_buses, dtype=np.intc), np.zeros(n_buses - 1, dtype=np.intc)
