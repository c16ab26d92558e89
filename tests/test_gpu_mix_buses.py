"""Mix buses (srack_voices_set_buses, srack_render_buses): bus_mix[b][c][t] = f32 sum over the voices of bus b of the f32 product
gain[v] * x[plane(c)][t][v], by a two-pass fold over each launch's frames (folds.hip.h: bus_fold_tiles, bus_fold_sum).

References are NumPy f64 sums over FRAMES — the frames the same call returned, and once the oracle's.  The bound is the standard one
for an f32 sum of n rounded products in any order, |got - ref| <= 1.02 n 2^-24 sum |gain x| + n 2^-149 (gamma_{n-1} (1 + u) + u with
u = 2^-24, under 1.02 n u for n <= 262 144; the last term covers products that underflow): derived, not tuned.

Measured on one MI355X: this file adds 7 s to the `-m gpu` suite."""
import numpy as np
import pytest

import srack_pkg

pytestmark = pytest.mark.gpu

KEEP, EXACT, NO_FUSION, NO_HOIST, NO_SPEC, SPEC = 64, 1, 2, 4, 16, 32
U = 2.0 ** -24


@pytest.fixture(scope="module")
def S():
    return srack_pkg.load()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def maker(S, w, V, B=None, lfo_val=0.0, nan_voices=()):
    """-> make() giving a fresh patch of workload `w` with V voices, and its ids.  (P1's gate LFO runs at 440 Hz here: at its default
    1.7 Hz the first 14 000 samples of every voice are silence, and a sum of zeros checks nothing.)"""
    B2, build, overrides = S.bench_workload(w, V)
    def make():
        p = S.Patch(48000, B2 if B is None else B, 2)
        ids = build(p, lfo_val=lfo_val) if build is S.build_p1 else build(p)
        p.configure_voices(V)
        for m, f, v in overrides(ids):
            v = np.array(v, dtype=np.float32)
            if w == "cfg3" and m == ids["vcf"] and f == S.VCF_FREQ:
                for k, c in zip(nan_voices, (np.nan, 40.0, np.inf, -40.0)):
                    if k < V:
                        v[k] = np.float32(c)
            p.set_voice_field(m, f, v)
        p.ids = ids
        return p
    return make


def mixed_gains(V, rng):
    g = rng.uniform(-2.0, 2.0, V).astype(np.float32)
    g[rng.random(V) < 0.15] = 0.0
    pw = rng.random(V) < 0.2
    g[pw] = (2.0 ** rng.integers(-6, 4, V)).astype(np.float32)[pw] * np.where(rng.random(V) < 0.5, -1, 1).astype(np.float32)[pw]
    return g


def bus_reference(fr, cp, n_buses, bus, gain):
    """-> (ref f64 [n_buses][C][T], bound f64 [n_buses][C][T], members [n_buses]) from frames [planes][T][V] f32"""
    P, T, V = fr.shape
    C = len(cp)
    ref, mag = np.zeros((n_buses, C, T)), np.zeros((n_buses, C, T))
    voices = np.flatnonzero(bus >= 0)
    order = voices[np.argsort(bus[voices], kind="stable")]
    members = np.bincount(bus[voices], minlength=n_buses)
    present = np.flatnonzero(members)
    starts = np.concatenate(([0], np.cumsum(members[present])[:-1])).astype(np.intp)
    g = gain.astype(np.float64)[order]
    with np.errstate(all="ignore"):
        for c, plane in enumerate(cp):
            if plane < 0 or len(order) == 0:
                continue
            prod = fr[plane][:, order].astype(np.float64) * g  # [T][voices in bus order]
            ref[present, c] = np.add.reduceat(prod, starts, axis=1).T
            mag[present, c] = np.add.reduceat(np.abs(prod), starts, axis=1).T
    n = members.astype(np.float64)[:, None, None]
    return ref, 1.02 * n * U * mag + n * 2.0 ** -149, members


def assert_audible(fr):
    x = np.where(np.isfinite(fr), fr, 0)
    # (cfg3_poly's voices have gates of their own, most of them slow: thousands of non-zero samples, not most of them)
    assert np.abs(x).max() > 0.01 and np.count_nonzero(x) >= min(2000, x.size // 4), "the patch is (nearly) silent: the check would hold for any sum"


def assert_within_bound(got, ref, bound, factor=1.0, what=""):
    with np.errstate(all="ignore"):
        fin = np.isfinite(ref)
        np.testing.assert_array_equal(np.isfinite(got), fin, err_msg=f"{what}: non-finite where the reference is finite, or the reverse")
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=f"{what}: NaN against inf")
        err = np.where(fin, np.abs(np.where(fin, got, 0).astype(np.float64) - np.where(fin, ref, 0)), 0.0)
        lim = np.where(fin, factor * bound, 0.0)
    worst = float((err - lim).max())
    print(f"{what}: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(lim, 1e-300)):.3f}")
    assert worst <= 0.0, f"{what}: |got - ref| exceeds the bound by {worst:.3e}"


# (workload, buffer_size, V, T, flags, kernel): every kind of voice kernel; shadow lanes and short waves (1, 20, 257, 4097 voices);
# renders that cross launches
KERNELS = [
    ("cfg3", None, 1, 3000, 0, "render_voice_chain"),
    ("cfg3", None, 20, 5000, 0, "render_voice_chain_track"),
    ("cfg3", None, 257, 4500, NO_HOIST, "render_voice_chain"),
    ("cfg3", None, 100, 2500, EXACT, "render_voice_chain_track"),
    ("p3", None, 257, 5000, 0, "render_voice_chain_seq"),
    ("cfg4", 1, 257, 5000, 0, "render_fm_pair_x"),
    ("cfg4", 1024, 100, 9000, 0, "render_fm_pair_block_x"),
    ("cfg2", None, 4096, 3000, 0, None),
    ("cfg3_poly", None, 4097, 2500, 0, "render_specialized"),
    ("p4", None, 4097, 2500, 0, "render_specialized"),
    ("cfg3", None, 257, 5000, NO_FUSION | NO_SPEC, "render_interp"),
]


@pytest.mark.parametrize("w,B,V,T,flags,kernel", KERNELS)
def test_one_voice_per_bus_is_exact(S, w, B, V, T, flags, kernel):
    rng = np.random.default_rng(V + T)
    p = maker(S, w, V, B, nan_voices=(3, 17, 5, 9))()
    bus, gain = rng.permutation(V), mixed_gains(V, rng)
    p.set_buses(V, bus, gain)
    fr, _, _, bm = p.render_buses(T, frames=True, flags=flags)
    info = p.info()
    assert f"buses={V}[fold]" in info, info
    assert info.split("kernel=")[-1] == kernel if kernel else "kernel=" in info, info
    assert_audible(fr)
    n_planes, cp = p.planes()
    if w in ("p3", "p4"):
        assert n_planes == 2
    assert bm.shape == (V, 2, T)
    with np.errstate(all="ignore"):
        for c, plane in enumerate(cp):
            want = (fr[plane] * gain[None, :]).T if plane >= 0 else np.zeros((V, T), np.float32)  # f32 products, [V][T]
            assert want.dtype == np.float32
            got = bm[bus, c]
            same = (got == want) | (np.isnan(got) & np.isnan(want))
            assert same.all(), f"channel {c}: {np.count_nonzero(~same)} samples differ from gain * frame"
    # a plain render of the same patch: the kernel and every bit of the frames are those of a render that never heard of buses
    q = maker(S, w, V, B, nan_voices=(3, 17, 5, 9))()
    fr0, _ = q.render(T, mix=False, flags=flags)
    assert q.info().split("kernel=")[-1] == info.split("kernel=")[-1] and "buses=" not in q.info()
    np.testing.assert_array_equal(bits(fr), bits(fr0))


def tables(V, rng, none=0.15):
    """(name, n_buses, bus): random with voices in no bus and empty buses for n in {1, 7, 64, V}; contiguous blocks; v mod n"""
    out = []
    for n in (1, 7, 64, V):
        b = rng.integers(0, max(1, n - n // 4), V)  # (the last quarter of the buses stays empty)
        b[rng.random(V) < none] = -1
        out.append((f"random{n}", n, b))
    out.append(("blocks", (V + 99) // 100, np.arange(V) // 100))
    out.append(("mod7", 7, np.arange(V) % 7))
    out.append(("mod64", 64, np.arange(V) % 64))
    return out


@pytest.mark.parametrize("w,V,T,flags", [("cfg3", 4097, 2100, 0), ("p4", 257, 3000, 0), ("cfg4", 300, 2500, 0)])
def test_general_tables_within_the_derived_bound(S, w, V, T, flags):
    rng = np.random.default_rng(17)
    nan_voice = 5
    for name, n, bus in tables(V, rng):
        bus = bus.copy()
        bus[nan_voice] = -1  # its cutoff is NaN (cfg3) and so is its gain: a voice in no bus contributes to nothing
        gain = mixed_gains(V, rng)
        gain[nan_voice] = np.nan
        p = maker(S, w, V, nan_voices=(nan_voice,))()
        p.set_buses(n, bus, gain)
        fr, _, _, bm = p.render_buses(T, frames=True, flags=flags)
        assert np.isfinite(bm).all(), f"{name}: a voice in no bus reached a bus"
        assert_audible(fr)
        ref, bound, members = bus_reference(fr, p.planes()[1], n, bus, gain)
        assert_within_bound(bm, ref, bound, what=f"{w} {name}")
        assert (members == 0).any() or name in ("blocks", "mod7", "mod64") or n == 1
        assert not bm[members == 0].any(), f"{name}: an empty bus is not 0"


@pytest.mark.parametrize("w", ["cfg3", "p4"])
def test_end_to_end_against_the_oracle_in_exact_mode(S, oracle, w):
    V, T = 300, 3000
    rng = np.random.default_rng(3)
    B, build, overrides = S.bench_workload(w, V)
    kw = dict(adsr="finite", lfo_val=0.0) if w == "cfg3" else {}
    p = S.Patch(48000, B, 2)
    ids = build(p, **kw)
    p.configure_voices(V)
    for m, f, v in overrides(ids):
        p.set_voice_field(m, f, v)
    bus = rng.integers(0, 12, V)
    bus[rng.random(V) < 0.1] = -1
    gain = mixed_gains(V, rng)
    p.set_buses(16, bus, gain)
    _, _, _, bm = p.render_buses(T, flags=EXACT)
    o = oracle.OraclePatch(48000, B, 2)
    build(o, **kw)
    ref_fr, _ = o.render_batch(V, T, overrides(ids), mix=True, threads=4)
    ref_fr = np.asarray(ref_fr, dtype=np.float32)  # per channel: [channels][T][V]
    assert np.abs(ref_fr).max() > 0.05
    ref, bound, _ = bus_reference(ref_fr, [0, 1], 16, bus, gain)
    assert_within_bound(bm, ref, bound, what=f"{w} against the oracle")


def all_fields(S, p):
    """every field of every module, per voice, as the device holds it after the render"""
    out = {}
    for m in range(p.num_modules()):
        for f in range(32):
            try:
                p.get_field(m, f)  # (host side: does the module have this field?)
            except S.SrackError:
                break
            out[(m, f)] = p.get_voice_field(m, f)
    return out


@pytest.mark.parametrize("w,V,T,flags", [("cfg3", 300, 6000, 0), ("cfg3", 300, 6000, NO_HOIST), ("cfg3_poly", 4097, 5000, 0), ("cfg4", 257, 5000, 0), ("p3", 100, 5000, 0)])
def test_nothing_else_moves(S, w, V, T, flags):
    rng = np.random.default_rng(8)
    make = maker(S, w, V)
    p = make()
    fr0, mx0, st0 = p.render_stats(T, frames=True, mix=True, flags=flags)
    q = make()
    q.set_buses(7, rng.integers(-1, 7, V), mixed_gains(V, rng))
    fr, mx, st, bm = q.render_buses(T, frames=True, mix=True, stats=True, flags=flags)
    assert q.info().split("kernel=")[-1] == p.info().split("kernel=")[-1]
    np.testing.assert_array_equal(bits(fr), bits(fr0))
    np.testing.assert_array_equal(bits(mx), bits(mx0))
    np.testing.assert_array_equal(st.view(np.uint64), st0.view(np.uint64))
    # buses alone (frames go to the library's scratch), buses + mix, buses + statistics: mix, statistics and bus mixes keep their bits
    r = make()
    r.set_buses(*q.get_buses())
    _, _, _, bm1 = r.render_buses(T, flags=flags)
    np.testing.assert_array_equal(bits(bm1), bits(bm))
    r2 = make()
    r2.set_buses(*q.get_buses())
    _, mx2, st2, bm2 = r2.render_buses(T, mix=True, stats=True, flags=flags)
    np.testing.assert_array_equal(bits(bm2), bits(bm))
    np.testing.assert_array_equal(bits(mx2), bits(mx0))
    np.testing.assert_array_equal(st2.view(np.uint64), st0.view(np.uint64))
    want = all_fields(S, p)
    assert len(want) >= 8
    for x in (q, r):
        got = all_fields(S, x)
        assert got.keys() == want.keys()
        for k in want:
            np.testing.assert_array_equal(got[k].view(np.uint64), want[k].view(np.uint64), err_msg=f"module {k[0]} field {k[1]}")


def test_setting_the_table_between_renders_restarts_nothing(S):
    V, T = 300, 10000
    rng = np.random.default_rng(9)
    make = maker(S, "cfg3", V)
    whole, _ = make().render(T, mix=False)
    p = make()
    p.set_buses(3, rng.integers(0, 3, V))
    a, _, _, _ = p.render_buses(T // 2, frames=True)
    desc = p.info().split(" buses=")[0]
    p.set_buses(5, rng.integers(-1, 5, V), mixed_gains(V, rng))
    p.set_buses(2, rng.integers(0, 2, V))
    assert p.info().split(" buses=")[0] == desc
    b, _, _, bm = p.render_buses(T - T // 2, frames=True)
    np.testing.assert_array_equal(bits(np.concatenate([a, b], axis=1)), bits(whole))
    assert bm.shape == (2, 2, T - T // 2)
    # ... nor does a plain render in between, which leaves the table in place
    c, _ = p.render(100, mix=False)
    assert "buses=" not in p.info()
    assert p.get_buses()[0] == 2


def test_however_the_render_is_cut(S):
    V = 300
    rng = np.random.default_rng(10)
    bus, gain = rng.integers(-1, 9, V), mixed_gains(V, rng)
    def make(w="cfg3", Vn=V):
        p = maker(S, w, Vn)()
        p.set_buses(9, bus[:Vn], gain[:Vn])
        return p
    T = 47 * 1024
    _, _, _, whole = make().render_buses(T)
    _, _, _, again = make().render_buses(T)  # the same call on a fresh handle
    np.testing.assert_array_equal(bits(again), bits(whole))
    _, _, _, full = make().render_buses(T, frames=True, mix=True, stats=True)
    np.testing.assert_array_equal(bits(full), bits(whole))
    q = make()  # a tick session: 47 calls of one block
    parts = [q.render_buses(1024)[3] for _ in range(47)]
    np.testing.assert_array_equal(bits(np.concatenate(parts, axis=2)), bits(whole))
    q = make()  # calls of unequal length, some with frames
    cuts = (1, 31, 1000, 4096, 777, 16384)
    parts = [q.render_buses(n, frames=(k % 2 == 0))[3] for k, n in enumerate(cuts + (T - sum(cuts),))]
    np.testing.assert_array_equal(bits(np.concatenate(parts, axis=2)), bits(whole))
    # across the 65 536-sample segment boundary, and through a folded kernel whose launches are 2048 samples
    for w, Vn, Tn in (("cfg3", 64, 70000), ("cfg4", 100, 70000)):
        _, _, _, one = make(w, Vn).render_buses(Tn)
        q = make(w, Vn)
        parts = [q.render_buses(n)[3] for n in (30000, 40000)]
        np.testing.assert_array_equal(bits(np.concatenate(parts, axis=2)), bits(one))
        fr, _, _, with_frames = make(w, Vn).render_buses(Tn, frames=True)
        np.testing.assert_array_equal(bits(with_frames), bits(one))
        assert_audible(fr)
        ref, bound, _ = bus_reference(fr, [0, 0], 9, bus[:Vn], gain[:Vn])
        assert_within_bound(one, ref, bound, what=f"{w} across the segment boundary")


def test_nonfinite_samples(S):
    # the +inf-sustain patch of the statistics suite: +-inf samples, NaN where the filter's output is 0
    V, T = 100, 48000
    rng = np.random.default_rng(11)
    p = maker(S, "cfg3", V, lfo_val=-8.0)()  # (that suite's patch: silence, then the envelope opens)
    p.set_field(p.ids["adsr"], S.ADSR_S_VAL, float("inf"))
    bus = rng.integers(0, 6, V)
    bus[rng.random(V) < 0.1] = -1
    bus[:8] = 6  # bus 6: eight voices, every gain 0 — 0 * inf = NaN
    gain = mixed_gains(V, rng)
    gain[:8] = 0.0
    p.set_buses(8, bus, gain)
    fr, _, _, bm = p.render_buses(T, frames=True)
    assert "kernel=render_voice_chain_track" in p.info(), p.info()
    fin = np.isfinite(fr[0])
    assert (~fin).any() and fin.any(), "the patch no longer produces the samples this test is about"
    ref, bound, members = bus_reference(fr, p.planes()[1], 8, bus, gain)
    assert_within_bound(bm, ref, bound, what="inf sustain")
    inf_rows = np.isinf(fr[0][:, :8]).any(axis=1)
    assert inf_rows.any() and np.isnan(bm[6, 0][inf_rows]).all()         # gain 0 on an infinite sample
    assert not bm[6, 0][fin[:, :8].all(axis=1)].any()                    # ... and 0 on finite ones
    assert not bm[7].any() and members[7] == 0


def test_one_bus_of_unit_gains_agrees_with_the_mix(S):
    for w, V, T in (("cfg3", 4097, 3000), ("p4", 300, 3000)):
        p = maker(S, w, V)()
        p.set_buses(1)
        fr, mx, _, bm = p.render_buses(T, frames=True, mix=True)
        assert_audible(fr)
        ref, bound, _ = bus_reference(fr, p.planes()[1], 1, np.zeros(V, dtype=int), np.ones(V, np.float32))
        assert_within_bound(bm, ref, bound, what=f"{w} one bus")
        err = np.abs(bm[0].astype(np.float64) - mx.astype(np.float64))
        assert (err <= 2.0 * bound[0]).all(), f"{w}: bus mix and mix differ by {err.max():.3e}"  # two orders of the same sum


def test_full_size(S):
    V, T, NB = 262144, 1024, 4096
    rng = np.random.default_rng(12)
    gain = mixed_gains(V, rng)
    pick = np.sort(rng.choice(NB, 64, replace=False))
    for name, bus in (("contiguous", np.arange(V) // 64), ("mod", np.arange(V) % NB)):
        p = maker(S, "cfg3", V)()
        p.set_buses(NB, bus, gain)
        fr, _, _, bm = p.render_buses(T, frames=True)
        assert f"buses={NB}[fold]" in p.info() and "kernel=render_voice_chain_track" in p.info(), p.info()
        assert bm.shape == (NB, 2, T)
        cols = np.flatnonzero(np.isin(bus, pick))
        sub = np.ascontiguousarray(fr[:, :, cols])
        assert_audible(sub)
        ref, bound, members = bus_reference(sub, p.planes()[1], NB, bus[cols], gain[cols])
        assert (members[pick] == 64).all()
        assert_within_bound(bm[pick], ref[pick], bound[pick], what=f"full size, {name}")
        del fr, sub
