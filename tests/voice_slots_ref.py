"""The bit-exact NumPy reference of the voice bus slots (srack_voices_set_bus_slots; the definition is in include/srack_hip.h), from
the frames a call returned:

    bus_mix[b][c][t]: the terms are all (v, k) with bus[v][k] == b, each fl32(gain[v][k][c] * x[plane(c)][t][v]).  A group is the terms
    of one (tile = v / 64, slot k), voices ascending: its first product, then one f32 addition per further term.  The bus's sample is
    the first group's sum, then one f32 addition per further group, in ascending (tile, slot).  A bus without terms and an unconnected
    channel are +0.

np.float32 products and sequential np.float32 additions in exactly that order, vectorised over time only: no tolerance is involved.
`slot_sums_f64` is the same sum in f64 with the derived bound of tests/test_gpu_mix_buses.py (bus_reference), to pin this reference
itself on the CPU."""
import numpy as np

TILE = 64
NONE = -1
U = 2.0 ** -24


def as_table(V, C, bus, gain=None):
    """-> (bus int [V][K], gain f32 [V][K][C]) with the defaults of the C ABI filled in"""
    bus = np.asarray(bus, dtype=np.int64)
    assert bus.ndim == 2 and bus.shape[0] == V, bus.shape
    g = np.ones((V, bus.shape[1], C), dtype=np.float32) if gain is None else np.asarray(gain, dtype=np.float32)
    assert g.shape == (V, bus.shape[1], C), g.shape
    return bus, g


def groups(V, bus):
    """the groups in ascending (tile, slot) order -> [(tile, slot, {bus: voices ascending})]"""
    K = bus.shape[1]
    out = []
    for tile in range((V + TILE - 1) // TILE):
        v0, v1 = tile * TILE, min(V, (tile + 1) * TILE)
        for k in range(K):
            members = {}
            for v in range(v0, v1):
                if bus[v, k] != NONE:
                    members.setdefault(int(bus[v, k]), []).append(v)
            out.append((tile, k, members))
    return out


def slot_reference(fr, cp, n_buses, bus, gain=None):
    """frames f32 [planes][T][V], the channels' planes cp -> bus_mix f32 [n_buses][C][T], bit for bit"""
    fr = np.asarray(fr)
    assert fr.dtype == np.float32
    _, T, V = fr.shape
    C = len(cp)
    bus, gain = as_table(V, C, bus, gain)
    out = np.zeros((n_buses, C, T), dtype=np.float32)
    started = np.zeros((n_buses, C), dtype=bool)
    with np.errstate(all="ignore"):
        for _, k, members in groups(V, bus):
            for b in sorted(members):
                for c, plane in enumerate(cp):
                    if plane < 0:
                        continue
                    acc = None
                    for v in members[b]:
                        p = gain[v, k, c] * fr[plane][:, v]   # f32 * f32 [T]: one rounding
                        assert p.dtype == np.float32
                        acc = p if acc is None else acc + p   # f32 + f32: one rounding
                    out[b, c] = acc if not started[b, c] else out[b, c] + acc
                    started[b, c] = True
    return out


def slot_sums_f64(fr, cp, n_buses, bus, gain=None):
    """-> (sum f64 [n_buses][C][T] of the exact products, bound f64 of an f32 sum of n rounded products in any order —
    1.02 n 2^-24 sum |g x| + n 2^-149 —, terms [n_buses])"""
    fr = np.asarray(fr)
    _, T, V = fr.shape
    C = len(cp)
    bus, gain = as_table(V, C, bus, gain)
    ref, mag, n = np.zeros((n_buses, C, T)), np.zeros((n_buses, C, T)), np.zeros(n_buses)
    with np.errstate(all="ignore"):
        for v in range(V):
            for k in range(bus.shape[1]):
                b = bus[v, k]
                if b == NONE:
                    continue
                n[b] += 1
                for c, plane in enumerate(cp):
                    if plane >= 0:
                        p = np.float64(gain[v, k, c]) * fr[plane][:, v].astype(np.float64)
                        ref[b, c] += p
                        mag[b, c] += np.abs(p)
    nn = n[:, None, None]
    return ref, 1.02 * nn * U * mag + nn * 2.0 ** -149, n


def slot_gains(shape, rng, odd=0.0):
    """gains among 0, -0.0, negative, powers of two and ordinary values; a share `odd` of them inf, -inf or NaN"""
    g = rng.uniform(-2.0, 2.0, shape).astype(np.float32)
    r = rng.random(shape)
    g[r < 0.10] = 0.0
    g[(r >= 0.10) & (r < 0.15)] = -0.0
    pw = (r >= 0.15) & (r < 0.35)
    g[pw] = ((2.0 ** rng.integers(-6, 4, shape)) * np.where(rng.random(shape) < 0.5, -1, 1)).astype(np.float32)[pw]
    if odd > 0:
        o = rng.random(shape) < odd
        g[o] = rng.choice(np.array([np.inf, -np.inf, np.nan], dtype=np.float32), shape)[o]
    return g


# the case of tests/voice_slots_stream_driver.py, shared with the test that reads what it wrote: voices, slots, buses, calls, samples per call
STREAM_CASE = (130, 2, 9, 4, 75)


def stream_tables():
    """-> two (bus, gain) tables for that case; the second replaces the first before the third call"""
    V, K, NB, _, _ = STREAM_CASE
    rng = np.random.default_rng(V + K)
    out = []
    for _ in range(2):
        bus = rng.integers(-1, NB - 1, (V, K))
        out.append((bus, slot_gains((V, K, 2), rng)))
    return out
