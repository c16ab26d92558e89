// fm_pair.hip.h — patch P2's shape one sample at a time: two-operator FM with a broken feedback edge.
//   render_fm_pair        buffer_size 1: the z^-1 edge in a register
//   render_fm_pair_split  ... on two waves per 64 voices (exact mode)
//   render_fm_pair_ring   buffer_size >= 32: the ring in HBM
//   render_fm_pair_x      buffer_size 1 with the modulator exact as a whole (default mode's config 4)
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "fm_common.hip.h"

#ifndef SRK_FM_UNROLL
#define SRK_FM_UNROLL 8
#endif

namespace srack {

// ---- fused 2-operator FM with a z^-1 feedback edge (patch P2's shape, buffer_size == 1) --------------------
//   MATH_FB(in1 = OSC_M.sine delayed by one sample) -> OSC_M.cv ; OSC_M.sine -> MATH_IDX -> OSC_C.cv ; OSC_C.sine -> out
// The broken edge is a one-sample delay, so the fed-back sine lives in a VGPR ("in-register recurrence").
// Both oscillators have CV: 2^x and sin per sample per operator (oscillator.rs:45,132-133).  The modulator of
// sample t+1 depends only on its own sine of sample t, so it runs one sample ahead of the carrier.
template <bool kExact, int kOut>
__global__ __launch_bounds__(64) void render_fm_pair(KernelArgs a, ChainRoles r)
{
    using namespace dev;
    __shared__ __attribute__((aligned(16))) float mix_tile[kMixTile];
    const int lane = threadIdx.x;
    const WaveMap wm = wave_map(a, lane);
    const uint32_t voice = wm.voice, vc = wm.vc, V = a.V;
    const bool active = wm.active;
    auto row = [&](int rr) { return a.table[(size_t)rr * V + vc]; };
    auto parv = [&](const DevOp& op, int k) { return op.par_row[k] >= 0 ? __uint_as_float(row(op.par_row[k])) : op.par_val[k]; };

    const DevOp& ofb = a.ops[r.adsr];    // MATH on the feedback path   (roles reuse the ChainRoles slots)
    const DevOp& om = a.ops[r.osc_l];    // modulator
    const DevOp& oix = a.ops[r.vca];     // MATH scaling the modulation index
    const DevOp& ocr = a.ops[r.osc_a];   // carrier
    const int plane = a.ops[r.out].aux;
    const int ring_row = r.track;        // the z^-1 ring: one state row

    constexpr uint32_t fo = OSC_HAS_CV | OSC_CV_AUDIO_RATE | OSC_AA | OSC_OUT_SINE | (kExact ? OSC_EXACT : 0u);
    constexpr uint32_t fo_carrier = fo | OSC_SINE_LOOSE;  // the carrier's sine only feeds the OutputModule (the matched shape): nothing integrates it
    OscRegs sm, sc;
    OscConst km, kc;
    sm.pos = make_f64(row(om.state_row + OSC_S_POS_LO), row(om.state_row + OSC_S_POS_HI));
    sm.sync_last = row(om.state_row + OSC_S_SYNC_LAST) != 0;
    sc.pos = make_f64(row(ocr.state_row + OSC_S_POS_LO), row(ocr.state_row + OSC_S_POS_HI));
    sc.sync_last = row(ocr.state_row + OSC_S_SYNC_LAST) != 0;
    km.sr = om.sample_rate;
    km.val = (double)parv(om, OSC_P_VAL);
    km.delta = 0.0;
    km.inv_dt = 0.0f;
    kc = km;
    kc.sr = ocr.sample_rate;
    kc.val = (double)parv(ocr, OSC_P_VAL);
    if (!kExact) {  // (the proved loops: OSC_VAL_FOLDED)
        km.scale = (440.0 / km.sr) * exp2(km.val);
        kc.scale = (440.0 / kc.sr) * exp2(kc.val);
    }
    // both MATH modules are Multiply by a constant (host-checked): in1 * constant (math.rs:152)
    const float c_fb = parv(ofb, MATH_P_CONST), c_ix = parv(oix, MATH_P_CONST);
    float fed = __uint_as_float(row(ring_row));  // OSC_M.sine of the previous tick (0.0 before the first)

    Emit em = make_emit(a, plane, lane);
    float sq = 0.0f, sw = 0.0f;
    float sine_m = 0.0f;
    double pos_m = sm.pos;  // modulator phase after exactly t samples (the loop runs it one sample ahead)
    // What a wave can prove about its own voices once per launch (default mode).  A sine is at most 1 in magnitude, so each oscillator's
    // CV is bounded by its gain: below 1000 (and |val| too) the increment is finite and positive and the wrap is one v_fract
    // (OSC_PHASE_TAME); at most 2 and 2^cv is (2^(cv/4))^4, at most 1/2 and it needs no range reduction at all (fm_facts).  The folded
    // val and the squarings round differently from the literal form (1e-16), so a launch is proved as a whole or not at all — the first
    // modulator step and a ragged last tile included: a render must not depend on where it was split.  The one value that is not a
    // sine is the ring's initial one (the host's): checked here.
    const FmFacts facts = kExact ? FmFacts{} : fm_facts(c_fb, km, sm.pos, c_ix, kc, sc.pos);
    const bool proved = !kExact && facts.tame && __builtin_amdgcn_ballot_w64(!(__builtin_fabsf(fed) <= 1.0f)) == 0;
    if (a.T > 0) {  // modulator of sample 0
        if (proved)
            fm_proved_tile<fo, fo_carrier>(facts, [&](auto m, auto) { osc_step(decltype(m)::value, sm, km, fed * c_fb, 0.0f, sine_m, sq, sw); });
        else
            osc_step(fo, sm, km, fed * c_fb, 0.0f, sine_m, sq, sw);
    }
    for (uint32_t t0 = 0; t0 < a.T; t0 += kMixRows) {
        const int n = (int)min((uint32_t)kMixRows, a.T - t0);
        auto tile = [&](auto fm_c, auto fc_c, auto whole) {
            constexpr uint32_t FM = decltype(fm_c)::value, FC = decltype(fc_c)::value;
            auto sample = [&](int i) {
                const float cur = sine_m;  // OSC_M.sine[t]: feeds the carrier now and, through the z^-1 ring, the modulator of t+1
                float out = 0.0f;
                osc_step(FC, sc, kc, cur * c_ix, 0.0f, out, sq, sw);      // carrier of sample t
                pos_m = sm.pos;
                osc_step(FM, sm, km, cur * c_fb, 0.0f, sine_m, sq, sw);   // modulator of sample t+1 (independent of the carrier)
                fed = cur;
                emit_put<kOut>(em, mix_tile, out, i, V);
            };
            if (decltype(whole)::value) {  // straight-line code over several samples: the tail of one sample's chains overlaps the head of the next's
#pragma unroll SRK_FM_UNROLL
                for (int i = 0; i < kMixRows; i++) sample(i);
            } else {
                for (int i = 0; i < n; i++) sample(i);
            }
        };
        using std::integral_constant;
        using std::true_type;
        using std::false_type;
        if (proved && n == kMixRows)
            fm_proved_tile<fo, fo_carrier>(facts, [&](auto m, auto c) { tile(m, c, true_type{}); });
        else if (proved)
            fm_proved_tile<fo, fo_carrier>(facts, [&](auto m, auto c) { tile(m, c, false_type{}); });
        else if (n == kMixRows)
            tile(integral_constant<uint32_t, fo>{}, integral_constant<uint32_t, fo_carrier>{}, true_type{});
        else
            tile(integral_constant<uint32_t, fo>{}, integral_constant<uint32_t, fo_carrier>{}, false_type{});
        emit_flush<kOut>(em, mix_tile, t0, n, V);
    }
    sm.pos = pos_m;  // drop the look-ahead step
    if (active) {
        auto put = [&](int rr, uint32_t v) { a.table[(size_t)rr * V + voice] = v; };
        put(om.state_row + OSC_S_POS_LO, f64_lo(sm.pos));
        put(om.state_row + OSC_S_POS_HI, f64_hi(sm.pos));
        put(om.state_row + OSC_S_SYNC_LAST, 0u);
        put(ocr.state_row + OSC_S_POS_LO, f64_lo(sc.pos));
        put(ocr.state_row + OSC_S_POS_HI, f64_hi(sc.pos));
        put(ocr.state_row + OSC_S_SYNC_LAST, 0u);
        put(ring_row, __float_as_uint(fed));
    }
}

// ---- the z^-1 FM pair on TWO waves per 64 voices ------------------------------------------------------------------------------
// The carrier is not part of the feedback loop: it only consumes the modulator's sine.  Wave 0 of the workgroup runs the modulators of
// its 64 voices (the recurrence), wave 1 their carriers, frames and mix; the sines cross through a double-buffered LDS tile, one
// barrier per 32 samples: while the carrier wave works on tile k - 1 the modulator wave produces tile k.  65 536 voices are then 2048
// waves — two per SIMD instead of one, each with half the f64 work — and the other wave's instructions fill the gaps a lone wave's
// dependent chains leave.  Same arithmetic, same proofs per wave (each about its own oscillator) as render_fm_pair; results are
// bit-identical to it.  MEASURED (config 4, one box, tools/ab_env.sh SRACK_FM_SPLIT "0 1"): exact mode 55.4 -> 44.0 ms per step — its
// correctly rounded 2^cv, library sine and division are long serial chains behind wave-uniform branches —, default mode 7.29 -> 7.57:
// render_fm_pair already interleaves its four chains by hand, and the LDS hand-over and the barrier only add to it (swapping the two
// jobs in every other workgroup, by any bit of its index, to balance the SIMDs: 7.6 - 7.8).  So the launch code takes this kernel in
// exact mode only.
template <bool kExact, int kOut>
__global__ __launch_bounds__(128) void render_fm_pair_split(KernelArgs a, ChainRoles r)
{
    using namespace dev;
    using std::integral_constant;
    __shared__ __attribute__((aligned(16))) float mix_tile[kMixTile];
    __shared__ float sines[2][kMixRows * 64];
    const int lane = (int)(threadIdx.x & 63u);
    const bool carrier = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) != 0;
    const WaveMap wm = wave_map(a, lane);
    const uint32_t voice = wm.voice, vc = wm.vc, V = a.V;
    const bool active = wm.active;
    auto row = [&](int rr) { return a.table[(size_t)rr * V + vc]; };
    auto parv = [&](const DevOp& op, int k) { return op.par_row[k] >= 0 ? __uint_as_float(row(op.par_row[k])) : op.par_val[k]; };
    auto put = [&](int rr, uint32_t v) { a.table[(size_t)rr * V + voice] = v; };
    const DevOp& oscop = a.ops[carrier ? r.osc_a : r.osc_l];   // this wave's oscillator (roles as in render_fm_pair)
    const DevOp& mulop = a.ops[carrier ? r.vca : r.adsr];      // the Multiply in front of its CV: x index / x feedback gain
    const int plane = a.ops[r.out].aux;
    const int ring_row = r.track;

    constexpr uint32_t fo = OSC_HAS_CV | OSC_CV_AUDIO_RATE | OSC_AA | OSC_OUT_SINE | (kExact ? OSC_EXACT : 0u);
    constexpr uint32_t fo_carrier = fo | OSC_SINE_LOOSE;
    OscRegs s;
    OscConst k;
    s.pos = make_f64(row(oscop.state_row + OSC_S_POS_LO), row(oscop.state_row + OSC_S_POS_HI));
    s.sync_last = false;
    k.sr = oscop.sample_rate;
    k.val = (double)parv(oscop, OSC_P_VAL);
    k.delta = 0.0;
    k.inv_dt = 0.0f;
    const float gain = parv(mulop, MATH_P_CONST);
    float fed = __uint_as_float(row(ring_row));  // (modulator wave) OSC_M.sine of the previous tick
    Emit em = make_emit(a, plane, lane);         // (carrier wave)
    float sq = 0.0f, sw = 0.0f;
    OscFacts facts = kExact ? OscFacts{} : fm_osc_facts(gain, k, s.pos);

    const uint32_t n_tiles = (a.T + (uint32_t)kMixRows - 1u) / (uint32_t)kMixRows;
    for (uint32_t kt = 0; kt <= n_tiles; kt++) {
        if (!carrier) {
            if (kt < n_tiles) {
                const uint32_t t0 = kt * (uint32_t)kMixRows;
                const int n = (int)min((uint32_t)kMixRows, a.T - t0);
                float* const dst = sines[kt & 1u] + lane;
                // the tile's first fed-back value is the host's at the start of a launch, a sine afterwards: the bound is checked where it enters
                const bool proved = !kExact && facts.tame && n == kMixRows && __builtin_amdgcn_ballot_w64(!(__builtin_fabsf(fed) <= 1.0f)) == 0;
                auto tile = [&](auto flags_c) {
                    constexpr uint32_t F = decltype(flags_c)::value;
#pragma unroll SRK_FM_UNROLL
                    for (int i = 0; i < kMixRows; i++) {
                        float sine = 0.0f;
                        osc_step(F, s, k, fed * gain, 0.0f, sine, sq, sw);
                        fed = sine;
                        dst[i * 64] = sine;
                    }
                };
                if (proved && facts.small)
                    tile(integral_constant<uint32_t, fo | OSC_PHASE_TAME | OSC_CV_SMALL>{});
                else if (proved)
                    tile(integral_constant<uint32_t, fo | OSC_PHASE_TAME>{});
                else if (n == kMixRows)
                    tile(integral_constant<uint32_t, fo>{});
                else
                    for (int i = 0; i < n; i++) {
                        float sine = 0.0f;
                        osc_step(fo, s, k, fed * gain, 0.0f, sine, sq, sw);
                        fed = sine;
                        dst[i * 64] = sine;
                    }
                if (!kExact && !proved) facts = fm_osc_facts(gain, k, s.pos);  // the literal forms may have left [0, 1)
            }
        } else if (kt > 0) {
            const uint32_t t0 = (kt - 1u) * (uint32_t)kMixRows;
            const int n = (int)min((uint32_t)kMixRows, a.T - t0);
            const float* const src = sines[(kt - 1u) & 1u] + lane;
            float in[kMixRows];
#pragma unroll
            for (int i = 0; i < kMixRows; i++) in[i] = src[i * 64];  // (rows past a short last tile: stale, unused)
            bool proved = false;
            if (!kExact && facts.tame && n == kMixRows) {  // a sine from a phase outside [0, 1) is not bounded by 1: look
                float m = 0.0f;
#pragma unroll
                for (int i = 0; i < kMixRows; i++) m = __builtin_fmaxf(m, __builtin_fabsf(in[i]));
                proved = __builtin_amdgcn_ballot_w64(!(m <= 1.0f)) == 0;
            }
            auto tile = [&](auto flags_c) {
                constexpr uint32_t F = decltype(flags_c)::value;
#pragma unroll SRK_FM_UNROLL
                for (int i = 0; i < kMixRows; i++) {
                    float out = 0.0f;
                    osc_step(F, s, k, in[i] * gain, 0.0f, out, sq, sw);
                    emit_put<kOut>(em, mix_tile, out, i, V);
                }
            };
            if (proved && facts.small)
                tile(integral_constant<uint32_t, fo_carrier | OSC_PHASE_TAME | OSC_CV_SMALL>{});
            else if (proved)
                tile(integral_constant<uint32_t, fo_carrier | OSC_PHASE_TAME>{});
            else if (n == kMixRows)
                tile(integral_constant<uint32_t, fo_carrier>{});
            else {
#pragma unroll
                for (int i = 0; i < kMixRows; i++)
                    if (i < n) {
                        float out = 0.0f;
                        osc_step(fo_carrier, s, k, in[i] * gain, 0.0f, out, sq, sw);
                        emit_put<kOut>(em, mix_tile, out, i, V);
                    }
            }
            if (!kExact && !proved) facts = fm_osc_facts(gain, k, s.pos);
            emit_flush<kOut, false>(em, mix_tile, t0, n, V);
        }
        __syncthreads();  // tile kt is complete and visible; the carrier is done with the buffer tile kt + 1 will overwrite
    }
    if (active) {
        put(oscop.state_row + OSC_S_POS_LO, f64_lo(s.pos));
        put(oscop.state_row + OSC_S_POS_HI, f64_hi(s.pos));
        put(oscop.state_row + OSC_S_SYNC_LAST, 0u);
        if (!carrier) put(ring_row, __float_as_uint(fed));
    }
}

// ---- the same FM pair with the app's default delay: buffer_size >= 32, the ring in HBM ---------------------------------
// The modulator of sample t reads what it produced buffer_size samples ago (ring[(n0 + t) mod B], [B][V] f32, voice-
// minor) and overwrites it.  A 32-sample tile's reads were all written before the tile began (B >= 32), so they are
// issued together at the tile's start; the modulator no longer depends on its own previous sample, which leaves the
// compiler free to overlap modulator and carrier of neighbouring samples.
template <bool kExact, int kOut>
__global__ __launch_bounds__(64) void render_fm_pair_ring(KernelArgs a, ChainRoles r)
{
    using namespace dev;
    __shared__ __attribute__((aligned(16))) float mix_tile[kMixTile];
    const int lane = threadIdx.x;
    const WaveMap wm = wave_map(a, lane);
    const uint32_t voice = wm.voice, vc = wm.vc, V = a.V;
    const bool active = wm.active;
    auto row = [&](int rr) { return a.table[(size_t)rr * V + vc]; };
    auto parv = [&](const DevOp& op, int k) { return op.par_row[k] >= 0 ? __uint_as_float(row(op.par_row[k])) : op.par_val[k]; };

    const DevOp& ofb = a.ops[r.adsr];    // MATH on the feedback path   (roles reuse the ChainRoles slots)
    const DevOp& om = a.ops[r.osc_l];    // modulator
    const DevOp& oix = a.ops[r.vca];     // MATH scaling the modulation index
    const DevOp& ocr = a.ops[r.osc_a];   // carrier
    const int plane = a.ops[r.out].aux;
    const uint32_t B = (uint32_t)a.prog.buffer_size;
    float* ring = a.rings + (size_t)r.track * B * V;  // r.track: the ring's id

    constexpr uint32_t fo = OSC_HAS_CV | OSC_CV_AUDIO_RATE | OSC_AA | OSC_OUT_SINE | (kExact ? OSC_EXACT : 0u);
    constexpr uint32_t fo_carrier = fo | OSC_SINE_LOOSE;  // the carrier's sine only feeds the OutputModule (the matched shape): nothing integrates it
    OscRegs sm, sc;
    OscConst km, kc;
    sm.pos = make_f64(row(om.state_row + OSC_S_POS_LO), row(om.state_row + OSC_S_POS_HI));
    sm.sync_last = false;
    sc.pos = make_f64(row(ocr.state_row + OSC_S_POS_LO), row(ocr.state_row + OSC_S_POS_HI));
    sc.sync_last = false;
    km.sr = om.sample_rate;
    km.val = (double)parv(om, OSC_P_VAL);
    km.delta = 0.0;
    km.inv_dt = 0.0f;
    kc = km;
    kc.sr = ocr.sample_rate;
    kc.val = (double)parv(ocr, OSC_P_VAL);
    if (!kExact) {
        km.scale = (440.0 / km.sr) * exp2(km.val);
        kc.scale = (440.0 / kc.sr) * exp2(kc.val);
    }
    const float c_fb = parv(ofb, MATH_P_CONST), c_ix = parv(oix, MATH_P_CONST);

    Emit em = make_emit(a, plane, lane);
    float sq = 0.0f, sw = 0.0f;
    uint32_t p0 = (uint32_t)(a.n0 % B);  // ring position of the tile's first sample
    auto ring_at = [&](uint32_t p) { return p < B ? p : p - B; };
    auto load_tile = [&](float (&dst)[kMixRows], uint32_t first) {  // (past the end of a short last tile: harmless re-reads of valid ring rows)
#pragma unroll
        for (int i = 0; i < kMixRows; i++) dst[i] = ring[(size_t)ring_at(first + (uint32_t)i) * V + vc];
    };
    // With buffer_size >= 64 the NEXT tile's 32 values are older than this tile too: they are fetched while this tile computes
    // (one wave per SIMD at 65 536 voices: nobody else hides the 32 loads' latency; the app's 1024: 12.7 -> see NOTES.md section 4).
    const bool ahead = B >= 2u * (uint32_t)kMixRows;
    float fed[kMixRows];
    load_tile(fed, p0);
    FmFacts facts = kExact ? FmFacts{} : fm_facts(c_fb, km, sm.pos, c_ix, kc, sc.pos);  // as in render_fm_pair; re-proved below once a tile left them
    for (uint32_t t0 = 0; t0 < a.T; t0 += kMixRows) {
        const int n = (int)min((uint32_t)kMixRows, a.T - t0);
        const bool more = t0 + kMixRows < a.T;
        float nxt[kMixRows];
        if (ahead && more) load_tile(nxt, ring_at(p0 + (uint32_t)kMixRows));
        auto tile = [&](auto fm_c, auto fc_c, auto whole) {
            constexpr uint32_t FM = decltype(fm_c)::value, FC = decltype(fc_c)::value;
            auto sample = [&](int i) {
                float sine_m = 0.0f, out = 0.0f;
                osc_step(FM, sm, km, fed[i] * c_fb, 0.0f, sine_m, sq, sw);   // modulator of sample t
                const uint32_t p = p0 + (uint32_t)i < B ? p0 + (uint32_t)i : p0 + (uint32_t)i - B;
                if (active) ring[(size_t)p * V + voice] = sine_m;
                osc_step(FC, sc, kc, sine_m * c_ix, 0.0f, out, sq, sw);      // carrier of sample t
                emit_put<kOut>(em, mix_tile, out, i, V);
            };
            if (decltype(whole)::value) {
#pragma unroll SRK_FM_UNROLL
                for (int i = 0; i < kMixRows; i++) sample(i);
            } else {
#pragma unroll
                for (int i = 0; i < kMixRows; i++)
                    if (i < n) sample(i);
            }
        };
        using std::integral_constant;
        using std::true_type;
        using std::false_type;
        // the ring's first lap holds whatever the host put there (a rack file's saved buffers), not sines: the bound on the CVs (fm_facts)
        // holds for a tile whose fed-back values are at most 1 in magnitude — one v_max per sample, wave-uniform per tile.  (A ragged
        // last tile takes the same arithmetic as a whole one: a render must not depend on where it was split.)
        bool fed_unit = false;
        if (!kExact && facts.tame) {
            float m = 0.0f;
#pragma unroll
            for (int i = 0; i < kMixRows; i++) m = __builtin_fmaxf(m, i < n ? __builtin_fabsf(fed[i]) : 0.0f);
            // (max skips a NaN, and may: a NaN CV makes the increment and then the phase NaN through either form of 2^x and of the wrap)
            fed_unit = __builtin_amdgcn_ballot_w64(!(m <= 1.0f)) == 0;
        }
        if (fed_unit && n == kMixRows)
            fm_proved_tile<fo, fo_carrier>(facts, [&](auto m, auto c) { tile(m, c, true_type{}); });
        else if (fed_unit)
            fm_proved_tile<fo, fo_carrier>(facts, [&](auto m, auto c) { tile(m, c, false_type{}); });
        else if (n == kMixRows)
            tile(integral_constant<uint32_t, fo>{}, integral_constant<uint32_t, fo_carrier>{}, true_type{});
        else
            tile(integral_constant<uint32_t, fo>{}, integral_constant<uint32_t, fo_carrier>{}, false_type{});
        if (!kExact && !fed_unit) facts = fm_facts(c_fb, km, sm.pos, c_ix, kc, sc.pos);  // the literal forms may have left [0, 1)
        emit_flush<kOut>(em, mix_tile, t0, n, V);
        p0 = ring_at(p0 + (uint32_t)n);
        if (more) {
            if (ahead) {
#pragma unroll
                for (int i = 0; i < kMixRows; i++) fed[i] = nxt[i];
            } else {
                load_tile(fed, p0);
            }
        }
    }
    if (active) {
        auto put = [&](int rr, uint32_t v) { a.table[(size_t)rr * V + voice] = v; };
        put(om.state_row + OSC_S_POS_LO, f64_lo(sm.pos));
        put(om.state_row + OSC_S_POS_HI, f64_hi(sm.pos));
        put(om.state_row + OSC_S_SYNC_LAST, 0u);
        put(ocr.state_row + OSC_S_POS_LO, f64_lo(sc.pos));
        put(ocr.state_row + OSC_S_POS_HI, f64_hi(sc.pos));
        put(ocr.state_row + OSC_S_SYNC_LAST, 0u);
    }
}

// ---- the z^-1 FM pair with the MODULATOR EXACT (config 4 as default mode renders it; round 6) -----------------------------------------------------
// buffer_size 1: the fed-back sine is last sample's, in a register, and nothing can be evaluated across time — the modulator of sample t + 1 needs
// the sine of sample t.  Until round 6 this program was the general path's (a kernel specialised at run time: 18.5 ms per step, 16.4 with the
// cheaper sine decision).  Written by hand, on TWO waves per 64 voices like render_fm_pair_split: wave 0 of the workgroup runs the modulators (the
// recurrence), wave 1 their carriers, frames and mix; the sines cross through a double-buffered LDS tile, one barrier per 32 samples.  65 536
// voices are then 2048 waves — two per SIMD, each with half the work — and one wave's instructions fill the gaps the other's dependent chains
// leave (a lone wave per SIMD issued 54 % of the time: 14.1 ms per step on one wave against this kernel's two).  Per modulator sample two chains
// that do not wait for each other — the increment from the fed-back sine (the libm's 2^e, the correctly rounded quotient), the sine from the
// phase —, the exact forms' constants in registers, the libm's table in LDS, ONE test per sample for "some lane could not decide", and what a wave
// can prove once per launch (|gain| + |val| <= 800, a fed-back value of at most 1: no test of the quotient's range, a phase that stays in [0, 1)).
// The modulator's arithmetic is osc_step's exact flavour operation for operation (x_exp2_libm_plain, div_rn_proved / div_rn_plain,
// x_sine_exact_plain, v_fract / fmod1): bit-identical to it and to the CPU tick; the carrier's is render_fm_pair's default loop.
// Reference: oscillator.rs:43-48,124-153, math.rs:152.
// (a tile with an undecided sample, again through osc_step itself — out of line: inlined, its cold arms' calls sat in the kernel's hot
// function, and their register conventions with them)
__device__ __attribute__((noinline)) void fm_x_tile_again(double pos0, float fed0, double sr, double val, float gain, float* dst, double& pos_out, float& fed_out)
{
    using namespace dev;
    OscRegs s;
    s.pos = pos0;
    s.sync_last = false;
    OscConst k;
    k.sr = sr;
    k.val = val;
    k.delta = 0.0;
    k.inv_dt = 0.0f;
    float fed = fed0, sq = 0.0f, sw = 0.0f;
    for (int i = 0; i < kMixRows; i++) {
        float sine = 0.0f;
        osc_step(OSC_HAS_CV | OSC_CV_AUDIO_RATE | OSC_AA | OSC_OUT_SINE | OSC_EXACT, s, k, fed * gain, 0.0f, sine, sq, sw);
        fed = sine;
        dst[i * 64] = sine;
    }
    pos_out = s.pos;
    fed_out = fed;
}

template <int kOut>
__global__ __launch_bounds__(128) void render_fm_pair_x(KernelArgs a, ChainRoles r)
{
    using namespace dev;
    using std::integral_constant;
    __shared__ __attribute__((aligned(16))) float mix_tile[kMixTile];
    __shared__ float sines[2][kMixRows * 64];
    __shared__ uint64_t tab[256];
    const int lane = (int)(threadIdx.x & 63u);
    const bool carrier = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) != 0;
    const WaveMap wm = wave_map(a, lane);
    const uint32_t voice = wm.voice, vc = wm.vc, V = a.V;
    const bool active = wm.active;
    auto row = [&](int rr) { return a.table[(size_t)rr * V + vc]; };
    auto parv = [&](const DevOp& op, int k) { return op.par_row[k] >= 0 ? __uint_as_float(row(op.par_row[k])) : op.par_val[k]; };
    auto put = [&](int rr, uint32_t v) { a.table[(size_t)rr * V + voice] = v; };
    const DevOp& oscop = a.ops[carrier ? r.osc_a : r.osc_l];   // this wave's oscillator (roles as in render_fm_pair)
    const DevOp& mulop = a.ops[carrier ? r.vca : r.adsr];      // the Multiply in front of its CV: x index / x feedback gain
    const int plane = a.ops[r.out].aux;
    const int ring_row = r.track;

    for (int k = (int)threadIdx.x; k < 256; k += 128) tab[k] = kLibmExpTab[k];
    constexpr uint32_t fo = OSC_HAS_CV | OSC_CV_AUDIO_RATE | OSC_AA | OSC_OUT_SINE;
    constexpr uint32_t fo_mod = fo | OSC_EXACT, fo_carrier = fo | OSC_SINE_LOOSE;
    OscRegs s;
    OscConst k;
    s.pos = make_f64(row(oscop.state_row + OSC_S_POS_LO), row(oscop.state_row + OSC_S_POS_HI));
    s.sync_last = false;
    k.sr = oscop.sample_rate;
    k.val = (double)parv(oscop, OSC_P_VAL);
    k.delta = 0.0;
    k.inv_dt = 0.0f;
    k.scale = (440.0 / k.sr) * exp2(k.val);  // (the carrier's proved loops)
    const float gain = parv(mulop, MATH_P_CONST);
    float fed = __uint_as_float(row(ring_row));  // (modulator wave) OSC_M.sine of the previous tick
    Emit em = make_emit(a, plane, lane);         // (carrier wave)
    float sq = 0.0f, sw = 0.0f;
    XConsts X;
    x_consts_load(X);
    const LibmTabLds libm{tab};
    const double inv_sr = 1.0 / k.sr;
    OscFacts facts = fm_osc_facts(gain, k, s.pos);  // (carrier wave: its class; re-proved once a tile has left it)
    int car_class = fm_gain_class(gain);
    // (modulator wave) what the exact forms may skip once it is proved for the launch — see render_fm_pair_block_x
    const bool mod_ok = (double)__builtin_fabsf(gain) + __builtin_fabs(k.val) <= 800.0 && k.sr >= 1.0 && k.sr <= 65535.0 && s.pos >= 0.0 && s.pos < 1.0 && __builtin_fabsf(fed) <= 1.0f;
    const bool mod_proved = __builtin_amdgcn_ballot_w64(!mod_ok) == 0;
    __syncthreads();  // the table

    const uint32_t n_tiles = (a.T + (uint32_t)kMixRows - 1u) / (uint32_t)kMixRows;
    for (uint32_t kt = 0; kt <= n_tiles; kt++) {
        if (!carrier) {
            if (kt < n_tiles) {
                const uint32_t t0 = kt * (uint32_t)kMixRows;
                const int n = (int)min((uint32_t)kMixRows, a.T - t0);
                float* const dst = sines[kt & 1u] + lane;
                if (mod_proved && n == kMixRows) {
                    // A tile of 32 samples SPECULATIVELY: osc_step's exact flavour (merged form) with its tests proved away and its one remaining
                    // question — "could some lane not decide?" (a sine within 1e-13 of an f32 rounding boundary, an exponent below pow's plain range:
                    // 3.4e-6 of the samples) — asked ONCE, after the tile.  Asked per sample it is a wave-uniform branch between every two samples of a
                    // recurrence that runs at one or two waves per SIMD: 14.5 ms per step against 9.2 without the question (tools/gpu_r6.sh ab).  A tile
                    // with an undecided sample (0.7 % of them) is rendered again from its first sample through osc_step itself — every value the
                    // reference's, the decided ones the same bits as before.
                    const double pos0 = s.pos;
                    const float fed0 = fed;
                    bool cold = false;
#pragma unroll SRK_FM_UNROLL
                    for (int i = 0; i < kMixRows; i++) {
                        const double e = (double)(fed * gain) + k.val;
                        const double delta = div_rn_proved(X.k440 * x_exp2_libm_plain(X, e, cold, libm), k.sr, inv_sr);
                        const float sn = x_sine_exact_plain<false>(X, s.pos, cold);
                        s.pos = __builtin_amdgcn_fract(s.pos + delta);
                        fed = sn;
                        dst[i * 64] = sn;
                    }
                    if (__builtin_expect(__builtin_amdgcn_ballot_w64(cold) != 0, 0)) fm_x_tile_again(pos0, fed0, k.sr, k.val, gain, dst, s.pos, fed);
                } else {  // a ragged last tile, a modulator that is not proved: osc_step itself (the same values)
                    for (int i = 0; i < n; i++) {
                        float sine = 0.0f;
                        osc_step(fo_mod, s, k, fed * gain, 0.0f, sine, sq, sw);
                        fed = sine;
                        dst[i * 64] = sine;
                    }
                }
            }
        } else if (kt > 0) {
            const uint32_t t0 = (kt - 1u) * (uint32_t)kMixRows;
            const int n = (int)min((uint32_t)kMixRows, a.T - t0);
            const float* const src = sines[(kt - 1u) & 1u] + lane;
            float in[kMixRows];
#pragma unroll
            for (int i = 0; i < kMixRows; i++) in[i] = src[i * 64];  // (rows past a short last tile: stale, unused)
            bool proved = false;
            if (facts.tame) {  // a sine from a phase outside [0, 1), or a NaN, is not bounded by 1: look (a ragged last tile takes the same arithmetic as a whole one)
                float m = 0.0f;
#pragma unroll
                for (int i = 0; i < kMixRows; i++) m = __builtin_fmaxf(m, i < n ? __builtin_fabsf(in[i]) : 0.0f);
                proved = __builtin_amdgcn_ballot_w64(!(m <= 1.0f)) == 0;
            }
            auto tile = [&](auto flags_c) {
                constexpr uint32_t F = decltype(flags_c)::value;
                if (n == kMixRows) {
#pragma unroll SRK_FM_UNROLL
                    for (int i = 0; i < kMixRows; i++) {
                        float out = 0.0f;
                        osc_step(F, s, k, in[i] * gain, 0.0f, out, sq, sw);
                        emit_put<kOut>(em, mix_tile, out, i, V);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < kMixRows; i++)
                        if (i < n) {
                            float out = 0.0f;
                            osc_step(F, s, k, in[i] * gain, 0.0f, out, sq, sw);
                            emit_put<kOut>(em, mix_tile, out, i, V);
                        }
                }
            };
            constexpr uint32_t P = OSC_PHASE_TAME | OSC_VAL_FOLDED | OSC_CV_SERIES9;
            if (proved && car_class == 2)
                tile(integral_constant<uint32_t, fo_carrier | P | OSC_CV_SMALL>{});
            else if (proved && car_class == 1)
                tile(integral_constant<uint32_t, fo_carrier | P | OSC_CV_QUAD>{});
            else if (proved)
                tile(integral_constant<uint32_t, fo_carrier | P>{});
            else
                tile(integral_constant<uint32_t, fo_carrier>{});
            if (!proved) {  // the literal forms may have left [0, 1)
                facts = fm_osc_facts(gain, k, s.pos);
                car_class = fm_gain_class(gain);
            }
            emit_flush<kOut, false>(em, mix_tile, t0, n, V);
        }
        __syncthreads();  // tile kt is complete and visible; the carrier is done with the buffer tile kt + 1 will overwrite
    }
    if (active) {
        put(oscop.state_row + OSC_S_POS_LO, f64_lo(s.pos));
        put(oscop.state_row + OSC_S_POS_HI, f64_hi(s.pos));
        put(oscop.state_row + OSC_S_SYNC_LAST, 0u);
        if (!carrier) put(ring_row, __float_as_uint(fed));
    }
}

}  // namespace srack
