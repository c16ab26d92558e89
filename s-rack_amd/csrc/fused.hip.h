// fused.hip.h — the fused voice chain (patch P1's shape): every wire and all state in VGPRs (no LDS except the mix-down transpose
// tile).  Templates only: chain_unit.hip.h instantiates them, a translation unit per audio oscillator port.  The other fused shapes have
// headers of their own: seq.hip.h, fm_pair.hip.h, fm_block.hip.h.
//   render_voice_chain        patch P1 with every module per voice
//   render_voice_chain_track  P1 after uniform hoisting (the flagship kernel), with the co-scheduled control block
//   ctl_gate_env              P1's control program, OSC -> ADSR -> track: that block, and render_ctl_gate_env (chain.hip) on its own
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "kernel_args.hip.h"
#include "launch_types.hpp"
#include "modules.hip.h"
#include "wave.hip.h"

// render_voice_chain_track's priority ramp: a voice wave drops to priority 1 at SRK_PRIO_AT1 / 64 of its launch, to 0 at SRK_PRIO_AT0 / 64
#ifndef SRK_PRIO_AT1
#define SRK_PRIO_AT1 32
#endif
#ifndef SRK_PRIO_AT0
#define SRK_PRIO_AT0 56
#endif


namespace srack {

// ---- fused control chain: OSC (constant pitch) -> ADSR -> track ---------------------------------------------
// The voice-invariant half of patch P1's shape: one voice, one wave, every lane computes the same numbers.
// It is a pure latency chain (phase accumulate -> gate -> envelope state machine), so it is kept short: state
// in VGPRs, the carried-phase oscillator and the segmented ADSR, 64 samples gathered across lanes per store.

// kExact: the oscillator's outputs are the reference's f64 formulas (osc_step with OSC_EXACT) instead of the default mode's f32
// PolyBLEP.  The phase recurrence is the same f64 add and exact wrap either way, and the segmented envelope performs adsr.rs's own
// operations in both modes.
template <uint32_t kOscPort, bool kExact>
SRK_DEV void ctl_gate_env_body(const CtlWork& a)
{
    using namespace dev;
    const ChainRoles r{0, 0, 0, 1, 0, 2, 0};  // op order of the matched control program: OSC, ADSR, OUT
    const int lane = threadIdx.x;
    auto row = [&](int rr) { return a.table[rr]; };  // V == 1
    const DevOp& ol = a.ops[r.osc_l];
    const DevOp& od = a.ops[r.adsr];
    float* __restrict__ track = a.track;

    COsc cl;
    cosc_init(cl, make_f64(row(ol.state_row + OSC_S_POS_LO), row(ol.state_row + OSC_S_POS_HI)), ol.delta);
    AdsrRegs sd;
    sd.phase = __uint_as_float(row(od.state_row + ADSR_S_PHASE));
    sd.mode = (int)row(od.state_row + ADSR_S_MODE);
    sd.r_val = __uint_as_float(row(od.state_row + ADSR_S_R_VAL));
    sd.from_a_val = __uint_as_float(row(od.state_row + ADSR_S_FROM_A));
    sd.gate_last = row(od.state_row + ADSR_S_GATE_LAST) != 0;
    const AdsrConst kd = adsr_consts(od.par_val[ADSR_P_A], od.par_val[ADSR_P_D], od.par_val[ADSR_P_S], od.par_val[ADSR_P_R], od.par_val[ADSR_P_SR]);
    AdsrSeg seg;
    adsr_seg_enter(sd, kd, seg);

    // One voice on one wave is a latency chain, so the block works a tile at a time across lanes (modules.hip.h): the oscillator runs only
    // its two-instruction phase recurrence per sample and lane j evaluates sample j's output; the envelope takes whole runs of samples
    // between the events that can end its segment.  55 ns per sample where the sample-by-sample form (four-sample speculative groups)
    // took 102 — it is the first chunk's track that nothing hides.
    constexpr uint32_t osc_flags = OSC_AA | kOscPort | (kExact ? OSC_EXACT : 0u);
    for (uint32_t t0 = 0; t0 < a.T; t0 += kMixRows) {
        const int n = (int)min((uint32_t)kMixRows, a.T - t0);
        const float gate = cosc_tile<kExact>(osc_flags, cl, n);
        const float env = adsr_seg_tile(sd, kd, seg, gate, n);
        if (lane < n) track[t0 + lane] = env;
    }
    adsr_seg_flush(sd, seg);
    uint32_t* const tout = a.table_out ? a.table_out : a.table;
    if (a.table_out) {  // the rows this block does not rewrite travel with the state (lane r's store, then lane 0's below: fenced)
        for (uint32_t rr = (uint32_t)lane; rr < a.n_rows; rr += 64u) a.table_out[rr] = a.table[rr];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    }
    if (lane == 0) {
        tout[ol.state_row + OSC_S_POS_LO] = f64_lo(cl.pos);
        tout[ol.state_row + OSC_S_POS_HI] = f64_hi(cl.pos);
        tout[ol.state_row + OSC_S_SYNC_LAST] = 0u;
        tout[od.state_row + ADSR_S_PHASE] = __float_as_uint(sd.phase);
        tout[od.state_row + ADSR_S_MODE] = (uint32_t)sd.mode;
        tout[od.state_row + ADSR_S_R_VAL] = __float_as_uint(sd.r_val);
        tout[od.state_row + ADSR_S_FROM_A] = __float_as_uint(sd.from_a_val);
        tout[od.state_row + ADSR_S_GATE_LAST] = sd.gate_last ? 1u : 0u;
    }
}


template <bool kExact>
SRK_DEV void ctl_gate_env(const CtlWork& w)
{
    const uint32_t port = w.port & (OSC_OUT_SINE | OSC_OUT_SQUARE | OSC_OUT_SAW);
    if (port == OSC_OUT_SQUARE)
        ctl_gate_env_body<OSC_OUT_SQUARE, kExact>(w);
    else if (port == OSC_OUT_SAW)
        ctl_gate_env_body<OSC_OUT_SAW, kExact>(w);
    else
        ctl_gate_env_body<OSC_OUT_SINE, kExact>(w);
}

// ---- fused voice chain (patch P1's shape) -------------------------------------------------------------
// OSC_A.<port> -> VCF.<port> -> VCA <- ADSR <- OSC_L.<port>; all wires and all state in VGPRs.

template <uint32_t kOscAPort, uint32_t kOscLPort, uint32_t kVcfPort, bool kExact, int kOut>
__global__ __launch_bounds__(64) void render_voice_chain(KernelArgs a, ChainRoles r)
{
    using namespace dev;
    __shared__ __attribute__((aligned(16))) float mix_tile[kMixTile];
    const int lane = threadIdx.x;
    const WaveMap wm = wave_map(a, lane);
    const uint32_t voice = wm.voice, vc = wm.vc, V = a.V;
    const bool active = wm.active;
    auto row = [&](int rr) { return a.table[(size_t)rr * V + vc]; };
    auto parv = [&](const DevOp& op, int k) { return op.par_row[k] >= 0 ? __uint_as_float(row(op.par_row[k])) : op.par_val[k]; };

    const DevOp& oa = a.ops[r.osc_a];
    const DevOp& ol = a.ops[r.osc_l];
    const DevOp& ov = a.ops[r.vcf];
    const DevOp& od = a.ops[r.adsr];
    const DevOp& oc = a.ops[r.vca];
    const int plane = a.ops[r.out].aux;

    constexpr uint32_t kEx = kExact ? OSC_EXACT : 0u;
    constexpr uint32_t fa = OSC_AA | kOscAPort | kEx;
    constexpr uint32_t fl = OSC_AA | kOscLPort | kEx;

    OscRegs sa, sl;
    OscConst ka, kl;
    sa.pos = make_f64(row(oa.state_row + OSC_S_POS_LO), row(oa.state_row + OSC_S_POS_HI));
    sa.sync_last = row(oa.state_row + OSC_S_SYNC_LAST) != 0;
    sl.pos = make_f64(row(ol.state_row + OSC_S_POS_LO), row(ol.state_row + OSC_S_POS_HI));
    sl.sync_last = row(ol.state_row + OSC_S_SYNC_LAST) != 0;
    ka.sr = oa.sample_rate;
    ka.val = 0.0;
    ka.delta = oa.delta_row >= 0 ? make_f64(row(oa.delta_row), row(oa.delta_row + 1)) : oa.delta;
    ka.inv_dt = inv_dt_f32(ka.delta);
    kl.sr = ol.sample_rate;
    kl.val = 0.0;
    kl.delta = ol.delta_row >= 0 ? make_f64(row(ol.delta_row), row(ol.delta_row + 1)) : ol.delta;
    kl.inv_dt = inv_dt_f32(kl.delta);

    VcfRegs sv;
    {
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
    }
    if (a.T > 0) vcf_coeffs<!kExact>(sv, vcf_frequency(parv(ov, VCF_P_FREQ), 0.0f, parv(ov, VCF_P_EXP)), vcf_resonance(parv(ov, VCF_P_RES)));
    bool sv_fin = !kExact || vcf_nan_free(sv);  // (exact mode: v_med3 clamps while nothing can turn into a NaN, modules.hip.h vcf_run)

    AdsrRegs sd;
    sd.phase = __uint_as_float(row(od.state_row + ADSR_S_PHASE));
    sd.mode = (int)row(od.state_row + ADSR_S_MODE);
    sd.r_val = __uint_as_float(row(od.state_row + ADSR_S_R_VAL));
    sd.from_a_val = __uint_as_float(row(od.state_row + ADSR_S_FROM_A));
    sd.gate_last = row(od.state_row + ADSR_S_GATE_LAST) != 0;
    const AdsrConst kd = adsr_consts(parv(od, ADSR_P_A), parv(od, ADSR_P_D), parv(od, ADSR_P_S), parv(od, ADSR_P_R), parv(od, ADSR_P_SR));
    const bool negative = parv(oc, VCA_P_NEG) != 0.0f;

    EmitOf<kOut> em = make_emit_of<kOut>(a, plane, lane);

    COsc ca, cl;
    FOsc fa_osc;
    // default mode, a saw nothing integrates or thresholds: the host stored its phase and increment as value * 2^64 (OSC_FIXED_PHASE; wave-uniform)
    const bool fixed_a = !kExact && kOscAPort == OSC_OUT_SAW && (oa.flags & OSC_FIXED_PHASE) != 0;
    uint32_t fix_lo = 0u, fix_hi = 0u;  // ... its phase after exactly t samples
    AdsrSeg seg;
    float x = 0.0f, gate = 0.0f;
    double pos_a = sa.pos, pos_l = sl.pos;  // oscillator phases after exactly t samples (the loop runs one sample ahead)
    if (!kExact) {
        if (fixed_a) {
            const uint64_t dbits = (uint64_t)__double_as_longlong(oa.delta);
            fosc_init(fa_osc, row(oa.state_row + OSC_S_POS_LO), row(oa.state_row + OSC_S_POS_HI), oa.delta_row >= 0 ? row(oa.delta_row) : (uint32_t)dbits,
                      oa.delta_row >= 0 ? row(oa.delta_row + 1) : (uint32_t)(dbits >> 32));
            fix_lo = fa_osc.lo;
            fix_hi = fa_osc.hi;
        } else {
            cosc_init(ca, sa.pos, ka.delta);
        }
        cosc_init(cl, sl.pos, kl.delta);
        adsr_seg_enter(sd, kd, seg);
        if (a.T > 0) {  // software pipeline: the oscillators of sample t+1 are evaluated beside the filter of sample t
            x = fixed_a ? fosc_saw(fa_osc) : cosc_step<kOscAPort>(ca);
            gate = cosc_step<kOscLPort>(cl);
        }
    }

    for (uint32_t t0 = 0; t0 < a.T; t0 += kMixRows) {
        const int n = (int)min((uint32_t)kMixRows, a.T - t0);
        for (int i = 0; i < n; i++) {
            float env, x_next = 0.0f, gate_next = 0.0f;
            if (kExact) {
                float sine = 0.0f, square = 0.0f, saw = 0.0f;
                osc_step(fa, sa, ka, 0.0f, 0.0f, sine, square, saw);
                x = kOscAPort == OSC_OUT_SINE ? sine : (kOscAPort == OSC_OUT_SQUARE ? square : saw);
                float gs = 0.0f, gq = 0.0f, gw = 0.0f;
                osc_step(fl, sl, kl, 0.0f, 0.0f, gs, gq, gw);
                gate = kOscLPort == OSC_OUT_SINE ? gs : (kOscLPort == OSC_OUT_SQUARE ? gq : gw);
            }
            float lp, bp, hp;
            vcf_run<!kExact>(sv, sv_fin, x, lp, bp, hp);
            const float y = kVcfPort == VCF_OUT_LP ? lp : (kVcfPort == VCF_OUT_BP ? bp : hp);
            if (!kExact) {  // next sample's oscillators: same basic block as the filter chain above => they interleave
                pos_l = cl.pos;
                if (fixed_a) {
                    fix_lo = fa_osc.lo;
                    fix_hi = fa_osc.hi;
                    x_next = fosc_saw(fa_osc);
                } else {
                    pos_a = ca.pos;
                    x_next = cosc_step<kOscAPort>(ca);
                }
                gate_next = cosc_step<kOscLPort>(cl);
            }
            if (kExact)
                env = adsr_step(ADSR_HAS_GATE, sd, kd, gate);
            else
                env = adsr_seg_step(sd, kd, seg, gate);
            const float o = vca_step(VCA_HAS_AUDIO | VCA_HAS_CV, negative, y, env);
            emit_put<kOut>(em, mix_tile, o, i, V);
            if (!kExact) {
                x = x_next;
                gate = gate_next;
            }
        }
        emit_flush<kOut>(em, mix_tile, t0, n, V);
    }
    if (!kExact) {
        sa.pos = pos_a;
        sl.pos = pos_l;
        sa.sync_last = sl.sync_last = false;  // sync unconnected: `last` follows the constant 0.0 input
        adsr_seg_flush(sd, seg);
    }
    emit_stats_end(em);

    if (active) {
        auto put = [&](int rr, uint32_t v) { a.table[(size_t)rr * V + voice] = v; };
        put(oa.state_row + OSC_S_POS_LO, fixed_a ? fix_lo : f64_lo(sa.pos));
        put(oa.state_row + OSC_S_POS_HI, fixed_a ? fix_hi : f64_hi(sa.pos));
        put(oa.state_row + OSC_S_SYNC_LAST, sa.sync_last ? 1u : 0u);
        put(ol.state_row + OSC_S_POS_LO, f64_lo(sl.pos));
        put(ol.state_row + OSC_S_POS_HI, f64_hi(sl.pos));
        put(ol.state_row + OSC_S_SYNC_LAST, sl.sync_last ? 1u : 0u);
        const int s0 = ov.state_row;
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
        put(od.state_row + ADSR_S_PHASE, __float_as_uint(sd.phase));
        put(od.state_row + ADSR_S_MODE, (uint32_t)sd.mode);
        put(od.state_row + ADSR_S_R_VAL, __float_as_uint(sd.r_val));
        put(od.state_row + ADSR_S_FROM_A, __float_as_uint(sd.from_a_val));
        put(od.state_row + ADSR_S_GATE_LAST, sd.gate_last ? 1u : 0u);
    }
}

#ifdef SRK_WAVE_CENSUS
// Tools-only build (tools/wave_census.py): lane 0 of every wave of render_voice_chain_track records when it started and ended on the
// 100 MHz constant clock (comparable across XCDs) and where it ran.  Eight words per wave slot: [0..1] start, [2..3] end, [4] HW_ID,
// [5] XCC_ID, [6] 1 = recorded | 2 = the control block, [7] the wave's index.  Plain global stores; null: this launch is not recorded.
static __device__ uint32_t* srk_census_rec;  // (one per translation unit: launch.hpp, census_rec)
SRK_DEV uint32_t* census_begin(uint32_t slot, uint32_t wave, bool ctl, int lane)
{
    uint32_t* rec = srk_census_rec;
    if (!rec || lane != 0) return nullptr;
    rec += (size_t)slot * 8;
    const uint64_t t = __builtin_amdgcn_s_memrealtime();
    rec[0] = (uint32_t)t;
    rec[1] = (uint32_t)(t >> 32);
    rec[4] = (uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_REG_HW_ID: wave / SIMD / CU / SH / SE
    rec[5] = (uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 20);  // HW_REG_XCC_ID
    rec[6] = ctl ? 3u : 1u;
    rec[7] = wave;
    return rec;
}
SRK_DEV void census_end(uint32_t* rec)
{
    if (!rec) return;
    const uint64_t t = __builtin_amdgcn_s_memrealtime();
    rec[2] = (uint32_t)t;
    rec[3] = (uint32_t)(t >> 32);
}
// ... and a paced voice wave (wave.hip.h) adds to word [6]: 4 = paced, bits 3 .. 15 its pace key, bits 16 .. 23 the largest lead (either
// way, in steps summed over the group's other waves, at most 255) it saw, bits 24 .. 31 the steps it took (at most 255)
SRK_DEV void census_end(uint32_t* rec, const dev::Pace& p)
{
    if (rec && p.word) rec[6] = 1u | 4u | (p.key << 3) | ((p.max_lead < 255u ? p.max_lead : 255u) << 16) | ((p.mine < 255u ? p.mine : 255u) << 24);
    census_end(rec);
}
#endif

// ---- fused voice chain, envelope from a control track (P1 after uniform hoisting) ---------------------
// OSC_A.<port> -> VCF.<port> -> VCA <- track[t]; the track sample is wave-uniform (scalar load, SGPR operand).
// The loop body is one basic block: the filter chain of sample t interleaves with the oscillator of t+1.
template <uint32_t kOscAPort, uint32_t kVcfPort, bool kExact, int kOut>
__global__ __launch_bounds__(64) void render_voice_chain_track(KernelArgs a, ChainRoles r, CtlWork co)
{
    using namespace dev;
    __shared__ __attribute__((aligned(16))) float mix_tile[kMixTile];
    // Block 0 of a co-scheduled launch is not a voice wave: it computes the NEXT chunk's envelope track while the
    // voice blocks consume this chunk's (written by the previous launch).  Same stream, no events, no second queue.
    if (blockIdx.x < a.block0) {
        // a latency chain sharing its SIMD with four throughput-bound voice waves: without priority it gets a
        // fifth of the issue slots and can outlast the voice blocks (measured: 1.9 -> 2.6 ms per launch)
        __builtin_amdgcn_s_setprio(3);
#ifdef SRK_WAVE_CENSUS
        uint32_t* crec = census_begin(a.n_waves, 0xffffffffu, true, threadIdx.x);
#endif
        ctl_gate_env<kExact>(co);
#ifdef SRK_WAVE_CENSUS
        census_end(crec);
#endif
        return;
    }
    const int lane = threadIdx.x;
#ifdef SRK_WAVE_CENSUS
    uint32_t* crec = census_begin(blockIdx.x - a.block0, blockIdx.x - a.block0, false, lane);
#endif
    const WaveMap wm = wave_map(a, lane);
    const uint32_t voice = wm.voice, vc = wm.vc, V = a.V;
    const bool active = wm.active;
    auto row = [&](int rr) { return a.table[(size_t)rr * V + vc]; };
    auto parv = [&](const DevOp& op, int k) { return op.par_row[k] >= 0 ? __uint_as_float(row(op.par_row[k])) : op.par_val[k]; };

    const DevOp& oa = a.ops[r.osc_a];
    const DevOp& ov = a.ops[r.vcf];
    const DevOp& oc = a.ops[r.vca];
    const int plane = a.ops[r.out].aux;
    const float* __restrict__ env_track = a.tracks + (size_t)r.track * a.t_stride;

    constexpr uint32_t fa = OSC_AA | kOscAPort | (kExact ? OSC_EXACT : 0u);
    OscRegs sa;
    OscConst ka;
    sa.pos = make_f64(row(oa.state_row + OSC_S_POS_LO), row(oa.state_row + OSC_S_POS_HI));
    sa.sync_last = row(oa.state_row + OSC_S_SYNC_LAST) != 0;
    ka.sr = oa.sample_rate;
    ka.val = 0.0;
    ka.delta = oa.delta_row >= 0 ? make_f64(row(oa.delta_row), row(oa.delta_row + 1)) : oa.delta;
    ka.inv_dt = inv_dt_f32(ka.delta);

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
    if (a.T > 0) vcf_coeffs<!kExact>(sv, vcf_frequency(parv(ov, VCF_P_FREQ), 0.0f, parv(ov, VCF_P_EXP)), vcf_resonance(parv(ov, VCF_P_RES)));
    bool sv_fin = !kExact || vcf_nan_free(sv);  // (exact mode: v_med3 clamps while nothing can turn into a NaN, modules.hip.h vcf_run)
    const bool negative = parv(oc, VCA_P_NEG) != 0.0f;

    EmitOf<kOut> em = make_emit_of<kOut>(a, plane, lane);

    // default mode, saw: the phase lives in 64-bit fixed point (modules.hip.h, FOsc); the host stores state and increment so
    constexpr bool kFixed = !kExact && kOscAPort == OSC_OUT_SAW;
    COsc ca;
    FOsc fa_osc;
    float x = 0.0f;
    double pos_a = sa.pos;
    uint32_t fpos_lo = 0u, fpos_hi = 0u;
    if (kFixed) {
        const uint64_t dbits = oa.delta_row >= 0 ? ((uint64_t)row(oa.delta_row + 1) << 32) | row(oa.delta_row) : (uint64_t)__double_as_longlong(oa.delta);
        fosc_init(fa_osc, row(oa.state_row + OSC_S_POS_LO), row(oa.state_row + OSC_S_POS_HI), (uint32_t)dbits, (uint32_t)(dbits >> 32));
        fpos_lo = fa_osc.lo;
        fpos_hi = fa_osc.hi;
        if (a.T > 0) x = fosc_saw(fa_osc);
    } else if (!kExact) {
        cosc_init(ca, sa.pos, ka.delta);
        if (a.T > 0) x = cosc_step<kOscAPort>(ca);
    }
    // Default mode: the ladder's clamp behind the cubic is proved idle for the whole launch (modules.hip.h, vcf_b4_bounded: this filter
    // has no CV, so its coefficients stay; the state's and the coefficients' bound is the helper's), given an input within [-1, 1] —
    // which every port of the oscillator delivers while its two PolyBLEP windows do not overlap (increment below 1/4; the phase
    // inside [0, 1), which the fixed-point phase is by construction).  A wave for which every lane passes runs the tile copies without
    // that clamp; any other wave, or all of them without kTileVcfB4 in a.tile_flags (SRACK_VCF_B4=0), the copies with all five.
    bool b4_free = false;
    if (!kExact && (a.tile_flags & kTileVcfB4) != 0u && a.T > 0) {
        const bool osc_ok = kFixed ? fa_osc.dhi < 0x40000000u : (ka.delta >= 0.0 && ka.delta < 0.25 && sa.pos >= 0.0 && sa.pos < 1.0);
        b4_free = __builtin_amdgcn_ballot_w64(!osc_ok) == 0 && vcf_b4_bounded(sv);
    }
    // The envelope track is wave-uniform data written by an earlier launch: it is read through the scalar unit (constant address
    // space), costing no vector instruction.  A full tile takes it eight samples at a time (uniform_load8, wave.hip.h: one
    // s_load_dwordx8, the next eight requested while these are consumed — four loads and four waits per tile); a short last tile one
    // dword per sample.  Left to itself the compiler loads one dword per sample, unrolled or not: the predicated PolyBLEP regions
    // split the tile into a block per sample, and nothing is merged across blocks.
    typedef const __attribute__((address_space(4))) float CFloat;
    CFloat* env_s = (CFloat*)(uintptr_t)env_track;
    // The VCA's gate, (negative || cv > 0) ? y * cv : 0, asks the same question of a wave-uniform cv on every sample.  It is answered
    // once per tile instead: lane l looks at sample l & 31 of the NEXT tile (a vector load at the top of this full tile, its ballot taken
    // after this tile's samples — in flight behind the frame stores, never waited for at once; clamped to the launch's last sample),
    // and a full tile whose 32 values are all > 0 runs a copy of the samples with o = y * cv alone: the select would have taken the
    // product on every one of them, whatever `negative` is.  Any other tile runs the copy that asks per sample.  Without kTilePlain in a.tile_flags
    // (SRACK_TILE_PLAIN=0, tools/ and tests/): always that one — every value then looks negative to the ballot.
    const uint32_t* env_bits = (const uint32_t*)env_track;
    const uint32_t l32 = (uint32_t)lane & (uint32_t)(kMixRows - 1);
    const uint32_t gate_force = (a.tile_flags & kTilePlain) != 0u ? 0u : 0x80000000u;
    auto all_pos = [&](uint32_t bits) { return __builtin_amdgcn_ballot_w64(!(((bits | gate_force) - 1u) < 0x7f800000u)) == 0; };
    bool plain = a.T >= (uint32_t)kMixRows && all_pos(env_bits[l32]);
    // Exact mode, saw: the oscillator writes a whole tile first (modules.hip.h, XSaw: windowless values, then each lane repairs
    // its own PolyBLEP rows with the reference's f64 division), into the rows of the mix tile that the samples' outputs overwrite
    // one by one afterwards.  Its preconditions also make every filter input finite, which licenses the v_med3 clamps.
    XSaw xo;
    const bool xs = kExact && kOscAPort == OSC_OUT_SAW && xsaw_usable(sa.pos, ka.delta) && vcf_nan_free(sv);
    if (xs) xsaw_init(xo, sa.pos, ka.delta);
    // Waves in step (notes/r07.md, notes/r10.md): the four voice waves of a SIMD run the same code for the same samples, yet under age-ordered
    // arbitration the oldest runs ahead and the youngest finishes up to ~30 % of the launch later, alone on its SIMD for the tail.  Paced
    // (a.pace, wave.hip.h): a wave's priority follows its lead over its SIMD's other waves, measured every SRK_PACE_TILES tiles.  Not paced:
    // the open-loop ramp, priority 2 -> 1 -> 0 as the wave passes fixed points of the launch.  (The control block keeps 3.)  Scalar work
    // once per 32-sample tile either way; priority changes no bit of the output.
    const uint32_t prio1_at = (uint32_t)(((uint64_t)a.T * SRK_PRIO_AT1) >> 6), prio0_at = (uint32_t)(((uint64_t)a.T * SRK_PRIO_AT0) >> 6);
    Pace pace = pace_join(a.pace, lane);
    __builtin_amdgcn_s_setprio(2);
    auto sample_x = [&](int i, float xin, float env, bool gated, bool pinned) __attribute__((always_inline)) {
        float lp, bp, hp;
        vcf_step<false, true>(sv, xin, lp, bp, hp);
        const float y = kVcfPort == VCF_OUT_LP ? lp : (kVcfPort == VCF_OUT_BP ? bp : hp);
        const bool cv_pos = (uint32_t)(__float_as_int(env) - 1) < 0x7f800000u;
        const float o = (!gated || negative || cv_pos) ? y * env : 0.0f;
        emit_put<kOut>(em, mix_tile, o, i, V);
        if (pinned) emit_row_pin<kOut>(em);
    };
    // kB4: std::true_type = with the ladder's clamp behind the cubic; std::false_type (default mode, b4_free) = without
    auto sample = [&](int i, float env, bool gated, bool pinned, auto kB4) __attribute__((always_inline)) {
        if (kExact) {
            float sine = 0.0f, square = 0.0f, saw = 0.0f;
            osc_step(fa, sa, ka, 0.0f, 0.0f, sine, square, saw);
            x = kOscAPort == OSC_OUT_SINE ? sine : (kOscAPort == OSC_OUT_SQUARE ? square : saw);
        }
        float lp, bp, hp;
        if (!kExact && !decltype(kB4)::value)
            vcf_step<true, true, false>(sv, x, lp, bp, hp);
        else
            vcf_run<!kExact>(sv, sv_fin, x, lp, bp, hp);
        const float y = kVcfPort == VCF_OUT_LP ? lp : (kVcfPort == VCF_OUT_BP ? bp : hp);
        if (kFixed) {
            fpos_lo = fa_osc.lo;
            fpos_hi = fa_osc.hi;
            x = fosc_saw(fa_osc);  // sample t+1
        } else if (!kExact) {
            pos_a = ca.pos;
            x = cosc_step<kOscAPort>(ca);  // sample t+1
        }
        // vca.rs:132: (negative || cv > 0.0) ? audio * cv : 0.0 — cv is wave-uniform here, so `cv > 0.0` is decided
        // on the scalar unit from the bit pattern: positive, non-zero, not NaN  <=>  0 < bits <= 0x7f800000
        const bool cv_pos = (uint32_t)(__float_as_int(env) - 1) < 0x7f800000u;
        const float o = (!gated || negative || cv_pos) ? y * env : 0.0f;  // (gated = false: the tile's 32 values are known to be > 0)
        emit_put<kOut>(em, mix_tile, o, i, V);
        if (pinned) emit_row_pin<kOut>(em);
    };
    // One full tile at t0 (constant trip count: unrollable — readlane is convergent, so a runtime count is not).  kX: the tile-wise
    // exact saw; gated: the copy that keeps the VCA's gate; kB4: the copy that keeps the ladder's fifth clamp.
    auto full_tile = [&](uint32_t t0, auto kX, bool gated, auto kB4) __attribute__((always_inline)) {
        if (!pace.word) {
            if (t0 >= prio1_at && t0 < prio1_at + kMixRows) __builtin_amdgcn_s_setprio(1);
            if (t0 >= prio0_at && t0 < prio0_at + kMixRows) __builtin_amdgcn_s_setprio(0);
        }
        if (decltype(kX)::value) xsaw_tile(xo, mix_tile + lane, kMixPitch, kMixRows);
        // pacing: the step's atomic before the tile's samples, its value looked at after them — in this block alone, so that the value
        // is neither waited for behind the frame stores in flight nor alive anywhere else in the loop.  Likewise the next tile's gate.
        const uint32_t gate_next = env_bits[min(t0 + (uint32_t)kMixRows + l32, a.T - 1u)];
        uint32_t pace_seen;
        const bool pace_now = pace_step(pace, t0 / kMixRows, lane, pace_seen);
        // the envelope by eights, the second eight requested two samples into the first (behind the wait for the first: scalar loads
        // return in any order, so a wait is for all of them) and so on
        float8u e[kMixRows / 8];
        float xin[8];
        e[0] = uniform_load8(env_s + t0);
#pragma unroll 32
        for (int i = 0; i < kMixRows; i++) {
            if ((i & 7) == 2 && i + 8 < kMixRows) e[(i >> 3) + 1] = uniform_load8(env_s + t0 + (uint32_t)((i & ~7) + 8));
            if (decltype(kX)::value) {  // eight rows of the tile in flight per LDS round trip; a row is read before its output overwrites it
                if ((i & 7) == 0) {
#pragma unroll
                    for (int u = 0; u < 8; u++) xin[u] = mix_tile[(i + u) * kMixPitch + lane];
                }
                sample_x(i, xin[i & 7], e[i >> 3][i & 7], gated, true);
            } else {
                sample(i, e[i >> 3][i & 7], gated, true, kB4);
            }
        }
        // (the atomic's value is looked at whether a step was taken or not: a register that a vector-memory result may still be on its
        // way to makes the compiler drain every frame store in flight where it next writes that register — in emit_flush, every tile)
        const uint32_t seen = (uint32_t)__builtin_amdgcn_readfirstlane((int)pace_seen);
        if (pace_now) pace_apply(pace, seen);
        plain = all_pos(gate_next);
        emit_flush<kOut>(em, mix_tile, t0, kMixRows, V);
    };
    // The launch's tiles: runs of plain tiles and runs of gated ones, each run a loop of its own around ONE copy of the samples, then the
    // short last tile.  (One loop around both copies: behind the join of the two the compiler's wait counts no longer tell the pace
    // atomic and the next tile's gate from the 32 frame stores issued after them, and every tile waits for all of its stores.  A run
    // ends where the envelope changes class — twice per gate period — and there the counts are settled once, by hand.)
    auto tiles = [&](auto kX) __attribute__((always_inline)) {
        const uint32_t t_full = a.T & ~(uint32_t)(kMixRows - 1);
        uint32_t t0 = 0;
        // (exact mode's stepwise oscillator, hundreds of f64 instructions per sample, keeps the one gated copy: a second copy of it costs
        // the statistics variant its fourth wave per SIMD, 100 -> 131 VGPRs, for one instruction per sample)
        // Default mode has four copies: plain and gated without the ladder's fifth clamp for a wave whose vote passed (b4_free), and
        // plain and gated with all five for any other wave, which so runs exactly the two loops it ran before the vote existed.
        constexpr bool kTwo = !kExact || decltype(kX)::value;
        while (t0 < t_full) {
            if (!kExact && b4_free) {
                if (plain) {
                    do {
                        full_tile(t0, kX, false, std::false_type{});
                        t0 += kMixRows;
                    } while (t0 < t_full && plain);
                } else {
                    do {
                        full_tile(t0, kX, true, std::false_type{});
                        t0 += kMixRows;
                    } while (t0 < t_full && !plain);
                }
            } else if (kTwo && plain) {
                do {
                    full_tile(t0, kX, false, std::true_type{});
                    t0 += kMixRows;
                } while (t0 < t_full && plain);
            } else {
                do {
                    full_tile(t0, kX, true, std::true_type{});
                    t0 += kMixRows;
                } while (t0 < t_full && !(kTwo && plain));
            }
            __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0)
        }
        if (t0 < a.T) {
            const int n = (int)(a.T - t0);
            if (!pace.word) {
                if (t0 >= prio1_at && t0 < prio1_at + kMixRows) __builtin_amdgcn_s_setprio(1);
                if (t0 >= prio0_at && t0 < prio0_at + kMixRows) __builtin_amdgcn_s_setprio(0);
            }
            if (decltype(kX)::value) {
                xsaw_tile(xo, mix_tile + lane, kMixPitch, n);
                for (int i = 0; i < n; i++) sample_x(i, mix_tile[i * kMixPitch + lane], env_s[t0 + (uint32_t)i], true, false);
            } else {
                for (int i = 0; i < n; i++) sample(i, env_s[t0 + (uint32_t)i], true, false, std::true_type{});  // (all five clamps: a rolled loop, no further copy)
            }
            emit_flush<kOut>(em, mix_tile, t0, n, V);
        }
    };
    if (xs)
        tiles(std::true_type{});
    else
        tiles(std::false_type{});
    if (!kExact) {
        sa.pos = pos_a;
        sa.sync_last = false;
    }
    if (xs) {
        sa.pos = xo.pos;
        sa.sync_last = false;  // sync unconnected: `last` follows the constant 0.0 input
    }
    emit_stats_end(em);
    if (active) {
        auto put = [&](int rr, uint32_t v) { a.table[(size_t)rr * V + voice] = v; };
        put(oa.state_row + OSC_S_POS_LO, kFixed ? fpos_lo : f64_lo(sa.pos));
        put(oa.state_row + OSC_S_POS_HI, kFixed ? fpos_hi : f64_hi(sa.pos));
        put(oa.state_row + OSC_S_SYNC_LAST, sa.sync_last ? 1u : 0u);
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
#ifdef SRK_WAVE_CENSUS
    census_end(crec, pace);
#endif
}

}  // namespace srack
