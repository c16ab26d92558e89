"""Per-voice output statistics (srack_render_stats): in registers of the fused voice chains (wave.hip.h, EmitStats), folded from each
launch's frames for every other kernel (folds.hip.h, stats_fold).

The statistics must be what a sequential f64 loop over the frames gives, bit for bit, however the render is cut (launches, segments,
calls, tick sessions) and whichever kernel renders, and asking for them must change no bit of frames, mix or voice state."""
import numpy as np
import pytest

import srack_pkg
from tests.patch_makers import bits, p2_overrides, patch_maker, workload_maker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    return srack_pkg.load()


def ref_stats(fr, init=None):
    """The sequential f64 loop of include/srack_hip.h over frames [planes][T][V] (f32), continuing from `init`."""
    P, T, V = fr.shape
    st = np.zeros((P, 6, V)) if init is None else init.copy()
    for p in range(P):
        s, q = st[p, 0].copy(), st[p, 1].copy()
        pk, pn = st[p, 2].copy(), st[p, 3].copy()
        nf, cl = np.zeros(V, np.int64), np.zeros(V, np.int64)
        for t in range(T):
            x = fr[p, t].astype(np.float64)
            fin = np.isfinite(x)
            xs = np.where(fin, x, -0.0)  # (s + -0.0 == s: the same as skipping the sample)
            s = s + xs
            q = q + xs * xs
            pk = np.where(xs > pk, xs, pk)  # (a peak moves only to a value strictly above it: a zero peak is +0.0)
            pn = np.where(-xs > pn, -xs, pn)
            nf += ~fin
            cl += fin & (np.abs(xs) > 1.0)
        st[p, 0], st[p, 1], st[p, 2], st[p, 3] = s, q, pk, pn
        st[p, 4] += nf
        st[p, 5] += cl
    return st


def assert_stats_equal(got, want):
    assert got.shape == want.shape
    for k in range(6):  # every field bit for bit (peaks included: a peak of nothing is +0.0)
        np.testing.assert_array_equal(np.ascontiguousarray(got[:, k]).view(np.uint64), np.ascontiguousarray(want[:, k]).view(np.uint64), err_msg=f"field {k}")


def make_p1(S, V, B=1024, adsr="default", nan_voices=()):
    p = S.Patch(48000, B, 2)
    ids = S.build_p1(p, adsr=adsr)
    p.configure_voices(V)
    det, cut = S.p1_voice_params(V)
    det = det.astype(np.float32)
    cut = cut.astype(np.float32)
    for v, c in zip(nan_voices, (np.nan, 40.0, np.inf, -40.0)):  # out-of-range cutoffs: the kernels' clamps must keep the stats exact
        if v < V:
            cut[v] = np.float32(c)
    p.set_voice_field(ids["osc_a"], S.OSC_VAL, det)
    p.set_voice_field(ids["vcf"], S.VCF_FREQ, cut)
    return p, ids


# (V, T, flags, kernel): shadow lanes and short waves (1, 20, 100, 257, 4097 voices), renders that cross launches and once the 65 536-sample
# segment; flags 4 (RENDER_NO_UNIFORM_HOIST) keeps the envelope per voice: render_voice_chain; 1 = exact oscillators
KERNELS = [
    (1, 3000, 0, "render_voice_chain"),
    (20, 5000, 0, "render_voice_chain_track"),
    (100, 2500, 1, "render_voice_chain_track"),
    (257, 4500, 4, "render_voice_chain"),
    (257, 3000, 5, "render_voice_chain"),
    (4097, 9000, 0, "render_voice_chain_track"),
    (64, 70000, 0, "render_voice_chain_track"),
]


@pytest.mark.parametrize("V,T,flags,kernel", KERNELS)
def test_every_kernel_matches_the_sequential_loop(S, V, T, flags, kernel):
    p, _ = make_p1(S, V, nan_voices=(3, 17, 5, 9))
    fr, mx, st = p.render_stats(T, frames=True, mix=True, flags=flags)
    assert f"kernel={kernel}" in p.info(), p.info()
    assert_stats_equal(st, ref_stats(fr))
    # asking for statistics changes no bit of what the render writes
    q, _ = make_p1(S, V, nan_voices=(3, 17, 5, 9))
    fr0, mx0 = q.render(T, flags=flags)
    np.testing.assert_array_equal(bits(fr), bits(fr0))
    np.testing.assert_array_equal(bits(mx), bits(mx0))
    # statistics alone (no frames, no mix): the same bits
    r, _ = make_p1(S, V, nan_voices=(3, 17, 5, 9))
    fr1, mx1, st1 = r.render_stats(T, flags=flags)
    assert fr1 is None and mx1 is None
    assert_stats_equal(st1, st)
    # ... and mix + statistics
    u, _ = make_p1(S, V, nan_voices=(3, 17, 5, 9))
    _, mx2, st2 = u.render_stats(T, mix=True, flags=flags)
    assert_stats_equal(st2, st)
    np.testing.assert_array_equal(bits(mx2), bits(mx0))


def test_nonfinite_samples_are_counted_and_left_out(S):
    # an envelope that sustains at +inf makes the output +-inf, or NaN where the filter's output is 0 (NONFINITE) — and those samples enter
    # neither the sums nor the peaks.  (CLIPPED: every test compares it with the reference loop; an envelope above 1, the obvious way to
    # drive this patch past full scale, takes it off the fused kernels)
    sustain = float("inf")
    V, T = 100, 48000
    p, ids = make_p1(S, V)
    p.set_field(ids["adsr"], S.ADSR_S_VAL, sustain)
    fr, _, st = p.render_stats(T, frames=True)
    assert "kernel=render_voice_chain_track" in p.info(), p.info()
    fin = np.isfinite(fr)
    clip = fin & (np.abs(np.where(fin, fr, 0)) > 1)
    assert (~fin).any() and fin.any(), "the patch no longer produces the samples this test is about"
    np.testing.assert_array_equal(st[:, 4], (~fin).sum(axis=1))
    np.testing.assert_array_equal(st[:, 5], clip.sum(axis=1))
    assert np.isfinite(st[:, :4]).all()
    assert_stats_equal(st, ref_stats(fr))


def test_against_the_oracle_in_exact_mode(S, oracle):
    V, T = 64, 3000
    det, cut = S.p1_voice_params(V)
    p = S.Patch(48000, 1024, 2)
    ids = S.build_p1(p, adsr="finite", lfo_val=0.0)
    p.configure_voices(V)
    p.set_voice_field(ids["osc_a"], S.OSC_VAL, det)
    p.set_voice_field(ids["vcf"], S.VCF_FREQ, cut)
    _, _, st = p.render_stats(T, flags=S.RENDER_EXACT_OSC)
    o = oracle.OraclePatch(48000, 1024, 2)
    S.build_p1(o, adsr="finite", lfo_val=0.0)
    ref, _ = o.render_batch(V, T, [(ids["osc_a"], S.OSC_VAL, det), (ids["vcf"], S.VCF_FREQ, cut)], mix=True, threads=4)
    assert_stats_equal(st, ref_stats(np.asarray(ref, dtype=np.float32)[:1]))  # (the oracle's frames are per channel; P1's two are one plane)


def test_accumulation_across_calls_and_tick_sessions(S):
    V = 300
    p, _ = make_p1(S, V)
    fr_all, _, st_all = p.render_stats(47 * 1024, frames=True)
    # 47 calls of one block each: a tick session (the control program runs ahead across calls)
    q, _ = make_p1(S, V)
    st = None
    for _ in range(47):
        _, _, st = q.render_stats(1024, stats=st)
    assert_stats_equal(st, st_all)
    # calls of unequal length
    q, _ = make_p1(S, V)
    st = None
    for n in (1, 31, 1000, 4096, 777, 16384, 47 * 1024 - (1 + 31 + 1000 + 4096 + 777 + 16384)):
        _, _, st = q.render_stats(n, stats=st)
    assert_stats_equal(st, st_all)
    # block calls that alternate statistics on and off: the stats cover the calls that asked; the frames of the others are those of a
    # render that never asked
    q, _ = make_p1(S, V)
    st = None
    fr_on = []
    for k in range(12):
        if k % 2 == 0:
            f, _, st = q.render_stats(1024, frames=True, stats=st)
            fr_on.append(f)
        else:
            f, _ = q.render(1024)
            np.testing.assert_array_equal(bits(f), bits(fr_all[:, k * 1024:(k + 1) * 1024]))
    assert_stats_equal(st, ref_stats(np.concatenate(fr_on, axis=1)))


def test_accumulation_across_edits_with_keep_state(S):
    V = 128
    runs = []
    for with_stats in (True, False):
        p, ids = make_p1(S, V)
        p.keep_state(True)
        st, frs = None, []
        for k in range(3):
            if with_stats:
                f, _, st = p.render_stats(2000, frames=True, stats=st)
            else:
                f, _ = p.render(2000)
            frs.append(f)
            p.set_field(ids["vcf"], S.VCF_EXP_AMT, 0.3 + 0.1 * k)
        runs.append((np.concatenate(frs, axis=1), st))
    np.testing.assert_array_equal(bits(runs[0][0]), bits(runs[1][0]))
    assert_stats_equal(runs[0][1], ref_stats(runs[1][0]))


def test_a_patch_without_planes_leaves_the_buffer_alone(S):
    p = S.Patch(48000, 1024, 2)
    p.add_module(S.MOD_OUTPUT)
    osc = p.add_module(S.MOD_OSCILLATOR)
    p.set_field(osc, S.OSC_VAL, 0.0)
    p.configure_voices(10)
    assert p.planes()[0] == 0
    fr, mx, st = p.render_stats(500, mix=True)
    assert st.shape == (0, 6, 10)
    assert not mx.any()


def test_full_width(S):
    V, T = 262144, 8192
    p, _ = make_p1(S, V)
    fr, _, st = p.render_stats(T, frames=True)
    q, _ = make_p1(S, V)
    _, _, st_only = q.render_stats(T)
    assert "kernel=render_voice_chain_track" in q.info()
    assert_stats_equal(st_only, st)
    want = ref_stats(fr[:, :, ::97])  # the loop over a sample of the voices (the whole of it is 2 G f64 operations)
    assert_stats_equal(st[:, :, ::97], want)


# ---- every other kernel: the statistics folded from each launch's frames (stats_fold) -------------------------------------------------
def check_all_routes(S, make, T, flags, kernels=None):
    """frames + mix + stats against the loop over those frames; frames and mix against a plain render; statistics alone and mix +
    statistics (the kernel writes frames nobody asked for into the library's scratch) give the same bits"""
    p = make()
    fr, mx, st = p.render_stats(T, frames=True, mix=True, flags=flags)
    if kernels is not None:
        assert any(f"kernel={k}" in p.info() for k in kernels), p.info()
    assert_stats_equal(st, ref_stats(fr))
    fr0, mx0 = make().render(T, flags=flags)
    np.testing.assert_array_equal(bits(fr), bits(fr0))
    np.testing.assert_array_equal(bits(mx), bits(mx0))
    _, _, st1 = make().render_stats(T, flags=flags)
    assert_stats_equal(st1, st)
    _, mx2, st2 = make().render_stats(T, mix=True, flags=flags)
    assert_stats_equal(st2, st)
    np.testing.assert_array_equal(bits(mx2), bits(mx0))
    return fr, st


KEEP, EXACT, NO_FUSION, NO_SPEC, SPEC = 64, 1, 2, 16, 32
# (workload, buffer_size, V, T, flags, kernels)
OTHER_KERNELS = [
    ("p2", 1, 257, 5000, 0, ["render_fm_pair_x"]),
    ("p2", 1, 100, 5000, KEEP, ["render_fm_pair"]),
    ("p2", 1, 20, 3000, EXACT, ["render_fm_pair"]),
    ("p2", 1024, 100, 3000, KEEP, ["render_fm_pair_ring"]),
    ("p2", 1024, 257, 9000, KEEP, ["render_fm_pair_block"]),
    ("p2", 1024, 100, 9000, 0, ["render_fm_pair_block_x"]),
    ("p2", 1024, 64, 70000, 0, ["render_fm_pair_block_x"]),
    ("p3", 1024, 100, 5000, 0, ["render_voice_chain_seq"]),
    ("p3", 1024, 257, 5000, SPEC, ["render_specialized"]),
    ("p4", 1024, 20, 5000, 0, None),
    ("cfg3", 1024, 257, 5000, NO_FUSION, ["render_interp"]),
    ("cfg3", 1024, 257, 5000, NO_FUSION | SPEC, ["render_specialized"]),
    ("cfg3_poly", 1024, 4097, 5000, 0, ["render_specialized"]),
    ("cfg2", 1024, 4096, 5000, 0, None),
]


@pytest.mark.parametrize("w,B,V,T,flags,kernels", OTHER_KERNELS)
def test_other_kernels_fold_the_same_statistics(S, w, B, V, T, flags, kernels):
    make = workload_maker(S, w, B, V)
    fr, st = check_all_routes(S, make, T, flags, kernels)
    assert st.shape[0] == make().planes()[0]
    # run to run: the same bits again
    _, _, st_again = make().render_stats(T, flags=flags)
    assert_stats_equal(st_again, st)


def test_fm_voices_whose_phase_goes_nan(S):
    W = 64
    rng = np.random.default_rng(11)
    beta = rng.uniform(0.1, 0.4, 2 * W).astype(np.float32)
    index = rng.uniform(0.5, 1.5, 2 * W).astype(np.float32)
    beta[W + 17] = 3.0e4  # 2^(30000 sin) overflows: the voice's phase, and its output, go NaN
    V = 2 * W
    for B, T in ((1, 2500), (1024, 9000)):
        for flags in (0, KEEP):
            make = patch_maker(S, B, S.build_p2, lambda ids: [(ids["mul_fb"], S.MATH_CONSTANT, beta), (ids["mul_idx"], S.MATH_CONSTANT, index)], V)
            fr, st = check_all_routes(S, make, T, flags)
            assert st[0, 4, W + 17] > 0 and st[0, 4, :W + 17].sum() == 0
            assert np.isfinite(st[:, :4]).all()


def test_math_overflow_to_inf_then_nan_and_clipping(S):
    # osc -> x c1 -> x c2 overflows to +-inf (plane 0); (x c2) - (x c2) is inf - inf = NaN there (plane 1); osc x 4 clips (plane 2 via a mixer)
    V, T = 130, 3000
    c1 = np.linspace(1e20, 1e25, V).astype(np.float32)
    c1[::2] = 2.0  # half the voices stay finite
    def build(g):
        osc = g.add_module(S.MOD_OSCILLATOR)
        m1, m2, diff, gain = (g.add_module(S.MOD_MATH) for _ in range(4))
        out = g.add_module(S.MOD_OUTPUT)
        g.set_field(osc, S.OSC_VAL, 0.0)
        for m in (m1, m2, gain):
            g.set_field(m, S.MATH_OPERATION, S.MATH_MULTIPLY)
        g.set_field(m2, S.MATH_CONSTANT, 1e25)
        g.set_field(gain, S.MATH_CONSTANT, 4.0)
        g.set_field(diff, S.MATH_OPERATION, S.MATH_SUBTRACT)
        g.connect(osc, S.OSC_OUT_SINE, m1, 0)
        g.connect(m1, 0, m2, 0)
        g.connect(m2, 0, diff, 0)
        g.connect(m2, 0, diff, 1)
        g.connect(osc, S.OSC_OUT_SINE, gain, 0)
        g.connect(diff, 0, out, 0)
        g.connect(gain, 0, out, 1)
        return dict(osc=osc, m1=m1, m2=m2, diff=diff, gain=gain, out=out)
    make = patch_maker(S, 1024, build, lambda ids: [(ids["m1"], S.MATH_CONSTANT, c1), (ids["gain"], S.MATH_CONSTANT, np.linspace(0.5, 4.0, V).astype(np.float32))], V)
    for flags in (0, NO_SPEC, SPEC):
        fr, st = check_all_routes(S, make, T, flags)
        assert st.shape[0] == 2
        assert st[0, 4, 1::2].min() > 0 and st[0, 4, ::2].max() == 0  # NaN where the product overflowed, nowhere else
        assert st[1, 5].max() > 0 and st[1, 5][:V // 8].max() == 0      # gains above 1 clip, small ones do not
        assert np.isfinite(st[:, :4]).all()


def test_planes_unconnected_channel_and_oracle_p2(S, oracle):
    # an unconnected channel: one plane, the other channel silent
    V, T = 100, 3000
    def build(g):
        ids = S.build_p1(g)
        g.disconnect(ids["out"], 1)
        return ids
    det, cut = S.p1_voice_params(V)
    make = patch_maker(S, 1024, build, lambda ids: [(ids["osc_a"], S.OSC_VAL, det), (ids["vcf"], S.VCF_FREQ, cut)], V)
    fr, st = check_all_routes(S, make, T, 0)
    assert st.shape[0] == 1
    # P2 in exact mode against the oracle's frames
    V, T = 64, 3000
    o = oracle.OraclePatch(48000, 1, 2)
    ids = S.build_p2(o)
    over = p2_overrides(S, V)(ids)
    ref, _ = o.render_batch(V, T, over, threads=4)
    p = patch_maker(S, 1, S.build_p2, p2_overrides(S, V), V)()
    _, _, st = p.render_stats(T, flags=EXACT)
    assert_stats_equal(st, ref_stats(np.asarray(ref, dtype=np.float32)[:1]))


@pytest.mark.parametrize("seed,noise", [(s, False) for s in range(10)] + [(s, True) for s in range(3)])
def test_random_patches(S, seed, noise):
    from tests.fuzz_patches import random_patch
    B, build, overrides = random_patch(seed, noise)
    V, T = 67, 2300
    vals = [fn(V) for m, f, fn in overrides]  # (a draw per call: drawn once, every patch gets the same voices)
    done = 0
    for flags in (0, NO_SPEC, SPEC):
        make = patch_maker(S, B, build, lambda ids: [(ids[m], f, vals[k]) for k, (m, f, fn) in enumerate(overrides)], V)
        try:
            make().render(16, flags=flags)
        except S.SrackError as e:  # SPECIALIZE on a program the generator cannot express: fails loudly, nothing to compare
            assert flags == SPEC and e.code == S.ERR_UNSUPPORTED
            continue
        if make().planes()[0] == 0:
            continue
        check_all_routes(S, make, T, flags)
        done += 1
    assert done >= 1
