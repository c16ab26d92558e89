// seq.hip.h — render_voice_chain_seq: patch P3's shape, the sequencer-driven subtractive voice, with every wire and all state in VGPRs.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "kernel_args.hip.h"
#include "modules.hip.h"
#include "wave.hip.h"

namespace srack {

// ---- fused sequencer-driven voice chain (patch P3's shape after hoisting) ------------------------------------------
//   [MATH(note track, k)] -> OSC.cv ; OSC -> VCF (cutoff CV = envelope track) -> VCA (CV = envelope track) -> OUT,
//   plus output channels that carry a track unchanged (a raw gate).  The three tracks are wave-uniform: each is
//   prefetched one 32-sample tile ahead (lane l holds sample l) and read per sample with v_readlane, so "did the note /
//   the cutoff CV change" is a scalar compare.  Between note changes the oscillator is the carried-phase one; at a
//   change every lane recomputes its increment 440 / sr * 2^(cv + val) and rebuilds the carried terms from the exact f64
//   phase (as tile_osc's stepwise path).  The filter coefficients are recomputed only when the cutoff CV's bits changed
//   (vcf_coeffs re-checks per lane, as filter.rs:61 does).
template <uint32_t kOscPort, int kOut>
__global__ __launch_bounds__(64) void render_voice_chain_seq(KernelArgs a, SeqRoles r)
{
    using namespace dev;
    __shared__ __attribute__((aligned(16))) float mix_tile[kMixTile];
    const int lane = threadIdx.x;
    const WaveMap wm = wave_map(a, lane);
    const uint32_t voice = wm.voice, vc = wm.vc, V = a.V;
    const bool active = wm.active;
    auto row = [&](int rr) { return a.table[(size_t)rr * V + vc]; };
    auto parv = [&](const DevOp& op, int k) { return op.par_row[k] >= 0 ? __uint_as_float(row(op.par_row[k])) : op.par_val[k]; };

    const DevOp& oo = a.ops[r.osc];
    const DevOp& ov = a.ops[r.vcf];
    const DevOp& oc = a.ops[r.vca];
    const int plane = a.ops[r.out].aux;
    const bool has_math = r.math >= 0, has_cut = r.trk_cutoff >= 0;
    const uint32_t mflags = has_math ? a.ops[r.math].flags : 0u;
    const float mconst = has_math ? parv(a.ops[r.math], MATH_P_CONST) : 0.0f;
    const float* __restrict__ pitch_track = a.tracks + (size_t)r.trk_pitch * a.t_stride;
    const float* __restrict__ cut_track = a.tracks + (size_t)(has_cut ? r.trk_cutoff : r.trk_env) * a.t_stride;
    const float* __restrict__ env_track = a.tracks + (size_t)r.trk_env * a.t_stride;

    constexpr uint32_t fo = OSC_HAS_CV | OSC_AA | kOscPort;
    OscConst ko;
    ko.sr = oo.sample_rate;
    ko.val = (double)parv(oo, OSC_P_VAL);
    ko.delta = 0.0;
    ko.inv_dt = 0.0f;
    COsc co;
    co.pos = make_f64(row(oo.state_row + OSC_S_POS_LO), row(oo.state_row + OSC_S_POS_HI));
    co.delta = 0.0;
    bool carried = false, have_pitch = false, have_cut = false;
    uint32_t seen_pitch = 0u, seen_cut = 0u;
    float cv_lane = 0.0f;

    VcfRegs sv;
    const int s0 = ov.state_row;
    sv.f = __uint_as_float(row(s0 + VCF_S_F));
    sv.p = __uint_as_float(row(s0 + VCF_S_P));
    sv.q = __uint_as_float(row(s0 + VCF_S_Q));
    sv.b0 = __uint_as_float(row(s0 + VCF_S_B0 + 0));
    sv.b1 = __uint_as_float(row(s0 + VCF_S_B0 + 1));
    sv.b2 = __uint_as_float(row(s0 + VCF_S_B0 + 2));
    sv.b3 = __uint_as_float(row(s0 + VCF_S_B0 + 3));
    sv.b4 = __uint_as_float(row(s0 + VCF_S_B0 + 4));
    sv.freq = __uint_as_float(row(s0 + VCF_S_FREQ));
    sv.res = __uint_as_float(row(s0 + VCF_S_RES));
    const float vfreq = parv(ov, VCF_P_FREQ), vexp = parv(ov, VCF_P_EXP), vres = vcf_resonance(parv(ov, VCF_P_RES));
    const uint32_t vport = ov.flags & (VCF_OUT_LP | VCF_OUT_BP | VCF_OUT_HP);
    if (!has_cut && a.T > 0) vcf_coeffs<true>(sv, vcf_frequency(vfreq, 0.0f, vexp), vres);
    const bool negative = parv(oc, VCA_P_NEG) != 0.0f;

    Emit em = make_emit(a, plane, lane);
    float* extra_row[4] = {nullptr, nullptr, nullptr, nullptr};   // frame rows of the track-fed planes (wave-uniform)
    float* extra_mp[4] = {nullptr, nullptr, nullptr, nullptr};    // ... and their mix partials
    __amdgpu_buffer_rsrc_t extra_rsrc[4];
    const float* extra_track[4] = {env_track, env_track, env_track, env_track};
#pragma unroll
    for (int e = 0; e < 4; e++) {
        if (e >= r.n_extra) continue;
        extra_track[e] = a.tracks + (size_t)r.extra_trk[e] * a.t_stride;
        if (a.frames) extra_row[e] = a.frames + (size_t)r.extra_plane[e] * a.plane_stride + wm.wave0;
        extra_rsrc[e] = __builtin_amdgcn_make_buffer_rsrc(extra_row[e], 0, 0x7fffffff, 0x00020000);
        if (a.mixpart) extra_mp[e] = a.mixpart + ((size_t)r.extra_plane[e] * a.n_waves + (blockIdx.x - a.block0)) * a.t_stride;
    }

    // Per-sample track values come through the scalar unit (constant address space => s_load into SGPRs); the VGPR tiles
    // below (lane l = sample l of the tile) only serve the once-per-tile "did anything change" ballots and the mix partials.
    typedef const __attribute__((address_space(4))) float CFloat;
    CFloat* pitch_s = (CFloat*)(uintptr_t)pitch_track;
    CFloat* cut_s = (CFloat*)(uintptr_t)cut_track;
    CFloat* env_s = (CFloat*)(uintptr_t)env_track;
    CFloat* extra_s[4];
#pragma unroll
    for (int e = 0; e < 4; e++) extra_s[e] = (CFloat*)(uintptr_t)extra_track[e];
    const uint32_t l32 = (uint32_t)(lane & (kMixRows - 1));
    auto fetch = [&](const float* trk, uint32_t t0) { return trk[min(t0 + l32, a.T - 1)]; };
    float pitch_tile = fetch(pitch_track, 0), cut_tile = fetch(cut_track, 0);
    float extra_tile[4];
#pragma unroll
    for (int e = 0; e < 4; e++) extra_tile[e] = fetch(extra_track[e], 0);
    for (uint32_t t0 = 0; t0 < a.T; t0 += kMixRows) {
        const float pitch_next = fetch(pitch_track, t0 + kMixRows), cut_next = fetch(cut_track, t0 + kMixRows);
        float extra_next[4];
#pragma unroll
        for (int e = 0; e < 4; e++) extra_next[e] = fetch(extra_track[e], t0 + kMixRows);
        const int n = (int)min((uint32_t)kMixRows, a.T - t0);
        // A note lasts thousands of samples and an envelope rests in sustain or at zero for long stretches: when a whole
        // tile holds the pitch (the cutoff CV) the oscillator (the coefficients) were last set up for, its samples run
        // without the per-sample "did it change" branches, which lets the compiler interleave oscillator and filter of
        // neighbouring samples.  `steady_pitch` / `steady_cut` are compile-time constants inside each unrolled loop.
        auto sample = [&](int i, bool steady_pitch, bool steady_cut) {
            if (!steady_pitch) {
                const uint32_t pb = __float_as_uint(pitch_s[t0 + (uint32_t)i]);
                if (!have_pitch || pb != seen_pitch) {  // a new note (scalar test): new increment, carried terms rebuilt
                    have_pitch = true;
                    seen_pitch = pb;
                    const float note = __uint_as_float(pb);
                    cv_lane = has_math ? math_step(mflags, note, 0.0f, mconst) : note;
                    const double delta = osc_delta_cold((double)cv_lane + ko.val, ko.sr);  // once per note: the reference's own increment (modules.hip.h)
                    carried = __builtin_amdgcn_ballot_w64(!(delta < 0.25)) == 0;
                    cosc_init(co, co.pos, delta);
                }
            }
            float x;
            if (steady_pitch || carried) {  // (a steady tile is only declared when the carried form holds)
                x = cosc_step<kOscPort>(co);
            } else {  // an increment of a quarter cycle or more somewhere in the wave: the literal per-sample form
                OscRegs g;
                g.pos = co.pos;
                g.sync_last = false;
                g.seen_cv = cv_lane;
                g.seen_delta = co.delta;
                float sine = 0.0f, square = 0.0f, saw = 0.0f;
                osc_step(fo, g, ko, cv_lane, 0.0f, sine, square, saw);
                x = kOscPort == OSC_OUT_SINE ? sine : (kOscPort == OSC_OUT_SQUARE ? square : saw);
                co.pos = g.pos;
            }
            if (has_cut && !steady_cut) {  // vcf_coeffs itself recomputes only for lanes whose (frequency, res) changed
                const float cutv = cut_s[t0 + (uint32_t)i];
                vcf_coeffs<true>(sv, vcf_frequency(vfreq, cutv, vexp), vres);
            }
            float lp, bp, hp;
            vcf_step<true>(sv, x, lp, bp, hp);
            const float y = vport == VCF_OUT_LP ? lp : (vport == VCF_OUT_BP ? bp : hp);
            const float env = env_s[t0 + (uint32_t)i];
            const bool cv_pos = (uint32_t)(__float_as_int(env) - 1) < 0x7f800000u;  // env > 0.0 on the scalar unit
            const float o = (negative || cv_pos) ? y * env : 0.0f;
            emit_put<kOut>(em, mix_tile, o, i, V);
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (e < r.n_extra && extra_row[e]) {  // same tile-relative row offset as the main plane (em.soff was just advanced)
                    const float v = extra_s[e][t0 + (uint32_t)i];
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), extra_rsrc[e], em.lane_c * 4, (int)(em.soff - V * 4u), 2);
                }
        };
        const bool in_tile = (int)l32 < n;
        const bool steady_pitch = have_pitch && carried && __builtin_amdgcn_ballot_w64(in_tile && __float_as_uint(pitch_tile) != seen_pitch) == 0;
        const bool steady_cut = !has_cut || (have_cut && __builtin_amdgcn_ballot_w64(in_tile && __float_as_uint(cut_tile) != seen_cut) == 0);
        if (n == kMixRows) {
            if (steady_pitch && steady_cut) {
#pragma unroll 8
                for (int i = 0; i < kMixRows; i++) sample(i, true, true);
            } else if (steady_pitch) {
#pragma unroll 8
                for (int i = 0; i < kMixRows; i++) sample(i, true, false);
            } else {
#pragma unroll 4
                for (int i = 0; i < kMixRows; i++) sample(i, false, false);
            }
        } else {
            for (int i = 0; i < n; i++) sample(i, false, false);
        }
        if (has_cut && !steady_cut) {  // the coefficients now belong to the tile's last cutoff CV
            have_cut = true;
            seen_cut = __float_as_uint(cut_s[t0 + (uint32_t)(n - 1)]);
        }
        emit_flush<kOut>(em, mix_tile, t0, n, V);
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (e < r.n_extra && extra_row[e]) {
                extra_row[e] += (size_t)n * V;
                extra_rsrc[e] = __builtin_amdgcn_make_buffer_rsrc(extra_row[e], 0, 0x7fffffff, 0x00020000);
            }
#pragma unroll
        for (int e = 0; e < 4; e++)  // every voice carries the same sample: the wave's partial is count x sample
            if (e < r.n_extra && extra_mp[e] && lane < n) extra_mp[e][t0 + lane] = (float)em.n_active * extra_tile[e];
        pitch_tile = pitch_next;
        cut_tile = cut_next;
#pragma unroll
        for (int e = 0; e < 4; e++) extra_tile[e] = extra_next[e];
    }
    if (active) {
        auto put = [&](int rr, uint32_t v) { a.table[(size_t)rr * V + voice] = v; };
        put(oo.state_row + OSC_S_POS_LO, f64_lo(co.pos));
        put(oo.state_row + OSC_S_POS_HI, f64_hi(co.pos));
        put(oo.state_row + OSC_S_SYNC_LAST, 0u);  // sync unconnected: `last` follows the constant 0.0 input
        put(s0 + VCF_S_F, __float_as_uint(sv.f));
        put(s0 + VCF_S_P, __float_as_uint(sv.p));
        put(s0 + VCF_S_Q, __float_as_uint(sv.q));
        put(s0 + VCF_S_B0 + 0, __float_as_uint(sv.b0));
        put(s0 + VCF_S_B0 + 1, __float_as_uint(sv.b1));
        put(s0 + VCF_S_B0 + 2, __float_as_uint(sv.b2));
        put(s0 + VCF_S_B0 + 3, __float_as_uint(sv.b3));
        put(s0 + VCF_S_B0 + 4, __float_as_uint(sv.b4));
        put(s0 + VCF_S_FREQ, __float_as_uint(sv.freq));
        put(s0 + VCF_S_RES, __float_as_uint(sv.res));
    }
}

}  // namespace srack
