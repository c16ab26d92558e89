// fm_block.hip.h — patch P2's shape TIME-PARALLEL (default mode, buffer_size 256 ... 1024): 32 voices per 512-thread workgroup, the ring in LDS.
//   render_fm_pair_block    both oscillators in their default forms
//   render_fm_pair_block_x  the modulator exact as a whole
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "fm_common.hip.h"
#include "launch_types.hpp"

namespace srack {

// ---- the same FM pair, TIME-PARALLEL: buffer_size 256 ... 1024, the ring in LDS (round 3) ----------------------------------------------
// With a delay of B samples the modulator's pitch CV for the next B samples is already in the ring: beta * sine[t - B].  So for a
// chunk of L <= B samples every modulator increment is known up front, and the modulator's phase at sample i is a PREFIX SUM of
// increments (mod 1) instead of a recurrence: pos[i] = frac(pos[0] + sum_{j<i} delta[j]).  Its sines then follow independently,
// the carrier's increments from them, the carrier's phases by a second prefix sum.  Nothing in a chunk waits for its own past.
//   * One workgroup of 512 threads owns 32 voices for the whole launch: lane (g, s) = voice g of the 32, time slice s of 16.  A chunk
//     is 256 samples; slice s holds samples [16 s, 16 s + 16) of it: 16 increments in registers, a local prefix, the 16 slice totals
//     exchanged through LDS (two barriers per chunk), every lane adds the totals below its own.
//   * 2048 workgroups x 8 waves instead of 1024 lone waves: two waves per SIMD, each with 16 independent evaluations of 2^x and of
//     the sine in flight — the z^-1 kernel's one wave per SIMD is bound by the latency of its own dependency chains (NOTES.md section 4).
//   * The ring ([B][32] f32 = 128 KB at the app's buffer_size 1024) lives in LDS for the whole launch: loaded from HBM once, stored back
//     once.  render_fm_pair_ring reads and writes it in HBM every sample (8 B per voice-sample: 3.0 x the algorithmic bytes); here the
//     launch is the whole render segment and the ring costs 8 B per voice and B samples of it.
//   * Frames leave as 128-byte rows per (sample, workgroup): a wave stores two of them per instruction (its two slices).
//   * Arithmetic: the proved per-oscillator loops of render_fm_pair (modules.hip.h, fm_class_flags: scale * 2^cv with val folded, no
//     range reduction for |cv| <= 1/2, (2^(cv/4))^4 for |cv| <= 2, one-instruction wrap), voted per workgroup and launch; the literal
//     forms otherwise.  Default mode only: a prefix sum associates differently from the reference's recurrence — 1e-16 in a phase, nine
//     orders below the contract, but not bit-identical, and a render split between calls sums in other groups than an unsplit one.
// Reference: oscillator.rs:43-48,132-153 (the two oscillators), math.rs:152 (the two gains), synth.rs:164-192 (which edge is delayed).
SRK_DEV size_t fm_block_lds_bytes(uint32_t B) { return sizeof(float) * B * kBlkVoices + sizeof(double) * 2 * kBlkSlices * kBlkVoices + 16; }

// The polynomials' coefficients as REGISTERS.  A VOP3 f64 fma cannot take a 64-bit literal, and with sixteen evaluations in flight the
// compiler rematerialised every coefficient at every use (s_mov + v_mov: a fifth of the chunk's instructions).  Loaded once per launch and
// made opaque, they stay where they are; the operations are exp2_fast's and sine_fast's own (modules.hip.h), bit for bit.
struct BlkConsts {
    double e[10];  // 2^f: degree 8 (e[9] unused) or, loaded with kSeries9, degree 9 (exp2_fast9's coefficients)
    double q[7];   // sin(2 pi x) / x in x^2, degree 6
};
template <bool kSeries9 = false>
SRK_DEV void blk_consts_load(BlkConsts& K)
{
    const double e8[10] = {1.0000000000000004, 0.6931471805459332, 0.24022650695814518, 0.055504109412108156, 0.009618129159053034,
                           0.0013333450563173552, 0.00015403456082633648, 1.5310080611926545e-05, 1.3255179556479267e-06, 0.0};
    const double e9[10] = {0x1.000000000003dp+0, 0x1.62e42fefa39f7p-1, 0x1.ebfbdff8149f2p-3, 0x1.c6b08d7044119p-5, 0x1.3b2ab72b175eep-7,
                           0x1.5d87fe908f88ap-10, 0x1.43088e257f341p-13, 0x1.ffcb76789860fp-17, 0x1.63ef969a64d3cp-20, 0x1.b6571de2f2351p-24};
    const double q[7] = {6.283185307179272, -41.34170223990684, 81.60524914955879, -76.70584757807868, 42.05813586028645, -15.081496425342264, 3.6659216216293173};
    K.e[9] = 0.0;
#pragma unroll
    for (int i = 0; i < (kSeries9 ? 10 : 9); i++) {
        K.e[i] = kSeries9 ? e9[i] : e8[i];
        asm volatile("" : "+v"(K.e[i]));
    }
#pragma unroll
    for (int i = 0; i < 7; i++) {
        K.q[i] = q[i];
        asm volatile("" : "+v"(K.q[i]));
    }
}
template <bool kReduce>
SRK_DEV double blk_exp2(const BlkConsts& K, double x)  // == dev::exp2_fast<kReduce>(x)
{
    const double n = kReduce ? __builtin_rint(x) : 0.0;
    const double f = kReduce ? x - n : x;
    const double f2 = f * f;
    const double a01 = __builtin_fma(K.e[1], f, K.e[0]);
    const double a23 = __builtin_fma(K.e[3], f, K.e[2]);
    const double a45 = __builtin_fma(K.e[5], f, K.e[4]);
    const double a67 = __builtin_fma(K.e[7], f, K.e[6]);
    const double f4 = f2 * f2;
    const double b0 = __builtin_fma(a23, f2, a01);
    const double b1 = __builtin_fma(a67, f2, a45);
    const double b2 = __builtin_fma(K.e[8], f4, b1);
    const double p = __builtin_fma(b2, f4, b0);
    return kReduce ? __builtin_ldexp(p, (int)n) : p;
}
template <bool kReduce>
SRK_DEV double blk_exp2_9(const BlkConsts& K, double x)  // == dev::exp2_fast9<kReduce>(x); K loaded with kSeries9
{
    const double n = kReduce ? __builtin_rint(x) : 0.0;
    const double f = kReduce ? x - n : x;
    const double f2 = f * f;
    const double a01 = __builtin_fma(K.e[1], f, K.e[0]);
    const double a23 = __builtin_fma(K.e[3], f, K.e[2]);
    const double a45 = __builtin_fma(K.e[5], f, K.e[4]);
    const double a67 = __builtin_fma(K.e[7], f, K.e[6]);
    const double a89 = __builtin_fma(K.e[9], f, K.e[8]);
    const double f4 = f2 * f2;
    const double b0 = __builtin_fma(a23, f2, a01);
    const double b1 = __builtin_fma(a67, f2, a45);
    const double b2 = __builtin_fma(a89, f4, b1);
    const double p = __builtin_fma(b2, f4, b0);
    return kReduce ? __builtin_ldexp(p, (int)n) : p;
}
SRK_DEV float blk_sine(const BlkConsts& K, double pos)  // == dev::sine_fast(pos)
{
    uint32_t sign;
    const double x = dev::sine_fold(pos, sign);
    const double z = x * x;
    const double a01 = __builtin_fma(K.q[1], z, K.q[0]);
    const double a23 = __builtin_fma(K.q[3], z, K.q[2]);
    const double a45 = __builtin_fma(K.q[5], z, K.q[4]);
    const double z2 = z * z;
    const double b0 = __builtin_fma(a23, z2, a01);
    const double b1 = __builtin_fma(K.q[6], z2, a45);
    const double z4 = z2 * z2;
    const double p = __builtin_fma(b1, z4, b0);
    return __uint_as_float(__float_as_uint((float)(p * x)) ^ sign);
}
// The carrier's sine — it only feeds the OutputModule (the matched shape), nothing integrates it — folded in f32: the phase's 6e-8 of
// f32 rounding is 4e-7 of sine, beside the polynomial's 2e-7 (sine_loose folds in f64: three f64-rate instructions more per sample).
SRK_DEV float blk_sine_loose(double pos)
{
    const float qn = 0.5f - (float)pos;
    const uint32_t sign = __float_as_uint(qn) & 0x80000000u;
    const float x = 0.25f - __builtin_fabsf(__builtin_fabsf(qn) - 0.25f);
    const float z = x * x;
    const float a01 = __builtin_fmaf(-41.34168243408203f, z, 6.2831854820251465f);
    const float a23 = __builtin_fmaf(-76.58116912841797f, z, 81.60247802734375f);
    const float z2 = z * z;
    const float p = __builtin_fmaf(__builtin_fmaf(39.75982666015625f, z2, a23), z2, a01);
    return __uint_as_float(__float_as_uint(p * x) ^ sign);
}
// the phase increment of one sample, as osc_step spells it for the proved flags (default mode)
template <uint32_t kFlags>
SRK_DEV double fm_increment(const BlkConsts& K, const dev::OscConst& c, float cv)
{
    static_assert((kFlags & OSC_VAL_FOLDED) != 0, "the time-parallel pair runs proved loops only");
    double p;
    constexpr bool d9 = (kFlags & OSC_CV_SERIES9) != 0;  // (the degree-9 series: K loaded with kSeries9)
    if (kFlags & OSC_CV_QUAD) {
        p = d9 ? blk_exp2_9<false>(K, (double)(cv * 0.25f)) : blk_exp2<false>(K, (double)(cv * 0.25f));
        p = p * p;
        p = p * p;
    } else if (kFlags & OSC_CV_SMALL) {
        p = d9 ? blk_exp2_9<false>(K, (double)cv) : blk_exp2<false>(K, (double)cv);
    } else {
        p = d9 ? blk_exp2_9<true>(K, (double)cv) : blk_exp2<true>(K, (double)cv);
    }
    return c.scale * p;
}
// lane i's value from lane i ^ kMask of its row of 16, through the DPP network (no LDS crossbar): the masks a halving butterfly over 16
// lanes can use are 1 and 2 (quad permutes), 7 (row_half_mirror: i <-> 7 - i) and 15 (row_mirror: i <-> 15 - i) — together they span the row
template <int kMask>
SRK_DEV float row_xchg(float v)
{
    constexpr int ctrl = kMask == 1 ? 0xB1 : kMask == 2 ? 0x4E : kMask == 7 ? 0x141 : 0x140;
    static_assert(kMask == 1 || kMask == 2 || kMask == 7 || kMask == 15, "not a single DPP control");
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xf, 0xf, false));
}

// (two waves per SIMD is all the LDS allows — one workgroup per CU —, so the kernel may as well use their 256 registers each: the
// sixteen evaluations per lane and the polynomials' constants stay in registers instead of being rematerialised)
template <int kOut>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void render_fm_pair_block(KernelArgs a, ChainRoles r)
{
    using namespace dev;
    extern __shared__ __attribute__((aligned(16))) float blk_lds[];
    const uint32_t B = (uint32_t)a.prog.buffer_size, V = a.V;
    float* const ring_l = blk_lds;                                                   // [B][32]
    double* const sums = (double*)(blk_lds + (size_t)B * kBlkVoices);                 // [2][16][32]: per oscillator, per slice, per voice
    uint32_t* const flag = (uint32_t*)(sums + 2 * kBlkSlices * kBlkVoices);
    const int tid = (int)threadIdx.x, g = tid & 31, s = tid >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // this wave holds slices 2 w and 2 w + 1 of all 32 voices
    const bool odd = (s & 1) != 0;
    const uint32_t voice0 = (blockIdx.x - a.block0) * (uint32_t)kBlkVoices;
    const uint32_t n_act = min((uint32_t)kBlkVoices, V - voice0);
    const bool active = (uint32_t)g < n_act;
    const uint32_t voice = voice0 + (uint32_t)g, vc = active ? voice : voice0 + n_act - 1u;
    auto row = [&](int rr) { return a.table[(size_t)rr * V + vc]; };
    auto parv = [&](const DevOp& op, int k) { return op.par_row[k] >= 0 ? __uint_as_float(row(op.par_row[k])) : op.par_val[k]; };

    const DevOp& ofb = a.ops[r.adsr];    // roles as in render_fm_pair_ring
    const DevOp& om = a.ops[r.osc_l];
    const DevOp& oix = a.ops[r.vca];
    const DevOp& ocr = a.ops[r.osc_a];
    const int plane = a.ops[r.out].aux;
    float* const ring = a.rings + (size_t)r.track * B * V;

    constexpr uint32_t fo = OSC_HAS_CV | OSC_CV_AUDIO_RATE | OSC_AA | OSC_OUT_SINE;
    constexpr uint32_t fo_carrier = fo | OSC_SINE_LOOSE;
    OscConst km, kc;
    double pos_m = make_f64(row(om.state_row + OSC_S_POS_LO), row(om.state_row + OSC_S_POS_HI));
    double pos_c = make_f64(row(ocr.state_row + OSC_S_POS_LO), row(ocr.state_row + OSC_S_POS_HI));
    km.sr = om.sample_rate;
    km.val = (double)parv(om, OSC_P_VAL);
    km.delta = 0.0;
    km.inv_dt = 0.0f;
    kc = km;
    kc.sr = ocr.sample_rate;
    kc.val = (double)parv(ocr, OSC_P_VAL);
    km.scale = (440.0 / km.sr) * exp2(km.val);
    kc.scale = (440.0 / kc.sr) * exp2(kc.val);
    const float c_fb = parv(ofb, MATH_P_CONST), c_ix = parv(oix, MATH_P_CONST);
    BlkConsts K;
    blk_consts_load(K);

    // the ring: HBM -> LDS, looking at every value on the way (the host's may be anything; a sine is at most 1)
    if (tid == 0) *flag = 0u;
    __syncthreads();
    bool unit = true;
    for (uint32_t p = (uint32_t)s; p < B; p += (uint32_t)kBlkSlices) {
        const float x = ring[(size_t)p * V + vc];
        ring_l[p * kBlkVoices + (uint32_t)g] = x;
        unit = unit && __builtin_fabsf(x) <= 1.0f;
    }
    if (!unit) atomicOr(flag, 1u);
    __syncthreads();
    // every wave holds all 32 voices (two slices of each): its ballots speak for the workgroup
    const FmFacts facts = fm_facts(c_fb, km, pos_m, c_ix, kc, pos_c);
    // A prefix sum adds a chunk's increments BEFORE it wraps: fine while they are of ordinary size (256 x 2^20 cycles still leaves 2^-24 of
    // a cycle), wrong for the huge ones a gain of hundreds of octaves produces — the recurrence wraps after every step and carries on from
    // the fraction, a sum would swallow every later increment.  A workgroup with such a voice (or with host values above 1 in its ring, or
    // a phase outside [0, 1)) renders through the recurrence itself, below: one lane per voice, the literal forms, as render_fm_pair_ring.
    const double biggest = __builtin_fmax(km.scale * exp2((double)__builtin_fabsf(c_fb)), kc.scale * exp2((double)__builtin_fabsf(c_ix)));
    const bool sane = facts.tame && *flag == 0u && __builtin_amdgcn_ballot_w64(!(biggest <= 1048576.0)) == 0;
    uint32_t p0 = (uint32_t)(a.n0 % B);
    const uint32_t i0 = (uint32_t)s * (uint32_t)kBlkPer;  // this lane's first sample of a chunk
    float* const frame_base = a.frames ? a.frames + (size_t)plane * a.plane_stride + voice0 : nullptr;
    float* const mp = a.mixpart ? a.mixpart + ((size_t)plane * a.n_waves + (blockIdx.x - a.block0)) * a.t_stride : nullptr;
    const bool frames = kOut == 0 ? frame_base != nullptr : (kOut & 1) != 0;
    const bool mix = kOut == 0 ? mp != nullptr : (kOut & 2) != 0;

    // Where a lane's slice starts: the phase at the chunk's first sample + the totals of the slices below it.  The 16 slice totals of a
    // voice sit in 8 waves, two per wave: each wave leaves one total per voice (its two slices') in LDS, a lane adds the waves below
    // its own — a wave-uniform count: scalar branches, no selects — and the odd slice its even neighbour's, 32 lanes away.
    auto slice_base = [&](int osc, double mine, double start, double& base, double& total) {
        const double pair = mine + __shfl_xor(mine, 32);
        if (!odd) sums[(osc * 8 + w) * kBlkVoices + g] = pair;
        __syncthreads();
        base = start;
        total = 0.0;
#pragma unroll
        for (int w2 = 0; w2 < 8; w2++) {
            const double v = sums[(osc * 8 + w2) * kBlkVoices + g];
            total += v;
            if (w2 < w) base += v;
        }
        if (odd) base += pair - mine;  // (the even neighbour's total; exact enough: the same additions in another order are not bit-identical anyway)
    };

    auto run = [&](auto fm_c, auto fc_c) {
        constexpr uint32_t FM = decltype(fm_c)::value, FC = decltype(fc_c)::value;
        auto chunk = [&](uint32_t t0, uint32_t n, auto fast_c) {
            // kFast: all 256 samples are the render's, every slice's 16 ring rows are contiguous (no wrap inside a slice: the ring's position
            // and length are multiples of 16) and all 32 voices are real — no masks, no selects, ring addresses as instruction offsets
            constexpr bool kFast = decltype(fast_c)::value;
            uint32_t idx[kBlkPer];
            double pre[kBlkPer];
            // ---- modulator: increments from what the ring holds, local prefix ----
            double acc = 0.0;
            if (kFast) {
                uint32_t p = p0 + i0;
                p = p >= B ? p - B : p;
                const uint32_t first = p * (uint32_t)kBlkVoices + (uint32_t)g;
#pragma unroll
                for (int k = 0; k < kBlkPer; k++) idx[k] = first + (uint32_t)(k * kBlkVoices);
            } else {
#pragma unroll
                for (int k = 0; k < kBlkPer; k++) {
                    uint32_t p = p0 + i0 + (uint32_t)k;
                    p = p >= B ? p - B : p;
                    idx[k] = p * (uint32_t)kBlkVoices + (uint32_t)g;
                }
            }
            float fed[kBlkPer];
#pragma unroll
            for (int k = 0; k < kBlkPer; k++) fed[k] = ring_l[idx[k]];
#pragma unroll
            for (int k = 0; k < kBlkPer; k++) {
                double d = fm_increment<FM>(K, km, fed[k] * c_fb);
                if (!kFast) {
                    asm("" : "+v"(d));  // (computed in every lane: a select, not sixteen branches that would fence the evaluations off from each other)
                    d = i0 + (uint32_t)k < n ? d : 0.0;
                }
                pre[k] = acc;
                acc += d;
            }
            double base, total;
            slice_base(0, acc, pos_m, base, total);
            pos_m = __builtin_amdgcn_fract(pos_m + total);
            // ---- modulator sines -> ring; carrier increments, local prefix ----
            acc = 0.0;
#pragma unroll
            for (int k = 0; k < kBlkPer; k++) {
                const double pm = __builtin_amdgcn_fract(base + pre[k]);
                const float sine = blk_sine(K, pm);
                double d = fm_increment<FC>(K, kc, sine * c_ix);
                if (kFast) {
                    ring_l[idx[k]] = sine;
                } else {
                    asm("" : "+v"(d));
                    const bool live = i0 + (uint32_t)k < n;
                    if (live) ring_l[idx[k]] = sine;
                    d = live ? d : 0.0;
                }
                pre[k] = acc;
                acc += d;
            }
            slice_base(1, acc, pos_c, base, total);
            pos_c = __builtin_amdgcn_fract(pos_c + total);
            // ---- carrier sines: frames and the workgroup's mix partial ----
            float out[kBlkPer];
#pragma unroll
            for (int k = 0; k < kBlkPer; k++) out[k] = blk_sine_loose(__builtin_amdgcn_fract(base + pre[k]));
            if (frames && (kFast || active)) {
                // one descriptor per wave and chunk: its two slices' first rows; lane offset = voice (+ 16 rows for the odd slice), scalar offset = row k
                const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(frame_base + (size_t)(t0 + (uint32_t)w * 2u * (uint32_t)kBlkPer) * V, 0, 0x7fffffff, 0x00020000);
                const uint32_t voff = ((uint32_t)g + (odd ? (uint32_t)kBlkPer * V : 0u)) * 4u;
#pragma unroll
                for (int k = 0; k < kBlkPer; k++)
                    if (kFast || i0 + (uint32_t)k < n) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(out[k]), rsrc, (int)voff, (int)((uint32_t)k * V * 4u), SRK_FRAME_AUX);
            }
            if (mix) {
                // sum over the 32 voices of each of this slice's 16 samples: a halving butterfly — 16 -> 8 -> 4 -> 2 -> 1 values per lane
                // while the lanes pair up (i ^ 15, i ^ 7, i ^ 2, i ^ 1: single DPP controls) — then the two rows of 16 lanes: lane g ends with sample (g & 15)
                float v[kBlkPer];
#pragma unroll
                for (int k = 0; k < kBlkPer; k++) v[k] = (kFast || active) ? out[k] : 0.0f;
                auto halve = [&](auto mask_c, int bit, int h) {  // lanes i and i ^ mask share the work: the one with `bit` set keeps the upper half
                    const bool up = (g & bit) != 0;
#pragma unroll
                    for (int j = 0; j < 8; j++)
                        if (j < h) {
                            const float send = up ? v[j] : v[j + h], keep = up ? v[j + h] : v[j];
                            v[j] = keep + row_xchg<decltype(mask_c)::value>(send);
                        }
                };
                halve(std::integral_constant<int, 15>{}, 8, 8);
                halve(std::integral_constant<int, 7>{}, 4, 4);
                halve(std::integral_constant<int, 2>{}, 2, 2);
                halve(std::integral_constant<int, 1>{}, 1, 1);
                const float sum = v[0] + __shfl_xor(v[0], 16);
                if (g < kBlkPer && (kFast || i0 + (uint32_t)g < n)) mp[t0 + i0 + (uint32_t)g] = sum;
            }
            p0 += n;
            p0 = p0 >= B ? p0 - B : p0;
        };
        const bool fast = (B % (uint32_t)kBlkPer) == 0u && (p0 % (uint32_t)kBlkPer) == 0u && n_act == (uint32_t)kBlkVoices;  // (uniform; p0 stays a multiple of 16 over full chunks)
        uint32_t t0 = 0;
        if (fast)
            for (; t0 + (uint32_t)kBlkChunk <= a.T; t0 += (uint32_t)kBlkChunk) chunk(t0, (uint32_t)kBlkChunk, std::true_type{});
        for (; t0 < a.T; t0 += (uint32_t)kBlkChunk) chunk(t0, min((uint32_t)kBlkChunk, a.T - t0), std::false_type{});
    };
    if (sane) {
        fm_proved_tile<fo, fo_carrier>(facts, [&](auto m, auto c) { run(m, c); });
    } else if (s == 0) {  // the recurrence, sample by sample, one lane per voice (the other fifteen slices have nothing to do in this launch)
        OscRegs sm, sc;
        sm.pos = pos_m;
        sc.pos = pos_c;
        sm.sync_last = sc.sync_last = false;
        float sq = 0.0f, sw = 0.0f;
        for (uint32_t t = 0; t < a.T; t++) {
            const uint32_t at = p0 * (uint32_t)kBlkVoices + (uint32_t)g;
            float sine_m = 0.0f, out = 0.0f;
            osc_step(fo, sm, km, ring_l[at] * c_fb, 0.0f, sine_m, sq, sw);
            ring_l[at] = sine_m;
            osc_step(fo_carrier, sc, kc, sine_m * c_ix, 0.0f, out, sq, sw);
            if (frames && active) frame_base[(size_t)t * V + (uint32_t)g] = out;
            if (mix) {
                float v = active ? out : 0.0f;
#pragma unroll
                for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m);
                if (g == 0) mp[t] = v;
            }
            p0 = p0 + 1u == B ? 0u : p0 + 1u;
        }
        pos_m = sm.pos;
        pos_c = sc.pos;
    }
    __syncthreads();  // the last chunk's ring writes
    if (active) {
        for (uint32_t p = (uint32_t)s; p < B; p += (uint32_t)kBlkSlices) ring[(size_t)p * V + voice] = ring_l[p * kBlkVoices + (uint32_t)g];
        if (s == 0) {
            auto put = [&](int rr, uint32_t v) { a.table[(size_t)rr * V + voice] = v; };
            put(om.state_row + OSC_S_POS_LO, f64_lo(pos_m));
            put(om.state_row + OSC_S_POS_HI, f64_hi(pos_m));
            put(om.state_row + OSC_S_SYNC_LAST, 0u);
            put(ocr.state_row + OSC_S_POS_LO, f64_lo(pos_c));
            put(ocr.state_row + OSC_S_POS_HI, f64_hi(pos_c));
            put(ocr.state_row + OSC_S_SYNC_LAST, 0u);
        }
    }
}

// ---- the same, with the MODULATOR EXACT: time lanes for everything but two instructions (round 6) -----------------------------------------
// Default mode renders config 4 with the modulator exact as a whole (csrc/approx.cpp: its feedback loop runs through a pitch, where only the
// reference's own bits follow the reference for longer than seconds) — 2^cv by the host libm's pow operation for operation, the reference's
// sine —, and until round 6 that program was the general path's: one lane per voice, 48 000 samples in a row, one wave per SIMD, the ring
// through HBM both ways (22.2 ms per step, 3.0 x the algorithmic bytes).  But with a delay of B >= 256 samples the modulator's pitch CV of a
// whole chunk is in the ring when the chunk starts, exactly as for the kernel above; what an EXACT oscillator may not do is add its
// increments in another order.  So only that stays serial:
//     pos[t + 1] = (pos[t] + delta[t]) % 1.0            oscillator.rs:152-153 — one v_add_f64 and one v_fract_f64 per voice-sample,
// the reference's operations in the reference's order, and everything around it is evaluated across TIME lanes, each value by the
// reference's own expression: delta[t] = 440 * 2^(f64(cv[t]) + f64(val)) / sr (oscillator.rs:43-48,132: exp2_libm, div_rn) before the scan,
// sine[t] = (pos[t] * PI * 2).sin() as f32 (oscillator.rs:133: sine_exact) after it.  Bit-identical to osc_step's exact flavour, hence to
// the CPU tick.
//   * A workgroup of 512 threads owns 32 voices for the launch, lane (g, s) = voice g, time slice s of 16; a chunk is 64 samples, slice s
//     holds samples [4 s, 4 s + 4).  The ring ([B][32] f32, 128 KB at the app's 1024) lives in LDS for the whole launch: HBM sees the frames.
//   * The scan runs in the first 32 lanes of wave 0, through one [64][32] f64 buffer in LDS (increments in, phases out, in place), while
//     all eight waves do the rest — a three-stage pipeline over chunks, two barriers per chunk:
//         iteration k:   phases of chunk k -> registers, increments of chunk k + 1 -> buffer (a lane overwrites what it has just read) | barrier |
//                        scan(k + 1)  ||  carrier frames of chunk k - 1, sines of chunk k (-> ring, carrier increments), increments of chunk k + 2 -> registers | barrier
//   * The carrier behind the loop keeps the default forms of the kernel above (bounded-CV classes, prefix sum of its increments, f32
//     sine): nothing feeds it back.  Its slice totals cross between the waves one iteration late, on the pipeline's own barriers.
//   * A workgroup whose carrier cannot be proved tame (gains of hundreds of octaves, a phase outside [0, 1)) renders sample by sample
//     through osc_step, one lane per voice, like the kernel above; increments that are not finite send the scan through fmod1.
constexpr int kXPer = 4, kXChunk = kBlkSlices * kXPer;  // 64 samples per chunk
__host__ __device__ inline size_t fm_block_x_lds_bytes(uint32_t B) { return sizeof(float) * B * kBlkVoices + sizeof(double) * kXChunk * kBlkVoices + sizeof(double) * 2 * 8 * kBlkVoices + sizeof(uint64_t) * 256 + 16; }

template <int kOut>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void render_fm_pair_block_x(KernelArgs a, ChainRoles r)
{
    using namespace dev;
    extern __shared__ __attribute__((aligned(16))) float blk_lds[];
    const uint32_t B = (uint32_t)a.prog.buffer_size, V = a.V;
    float* const ring_l = blk_lds;                                                   // [B][32]
    double* const buf = (double*)(blk_lds + (size_t)B * kBlkVoices);                 // [64][32]: a chunk's modulator increments, then its phases
    double* const sums = buf + kXChunk * kBlkVoices;                                  // [2][8][32]: the carrier's slice totals, per chunk parity, per wave, per voice
    uint64_t* const tab = (uint64_t*)(sums + 2 * 8 * kBlkVoices);                     // the libm's 2^(k/128) table
    uint32_t* const flag = (uint32_t*)(tab + 256);                                    // [0]: some modulator increment is not an ordinary number; [1]: the ring came with a value above 1
    const int tid = (int)threadIdx.x, g = tid & 31, s = tid >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // this wave holds slices 2 w and 2 w + 1 of all 32 voices
    const bool odd = (s & 1) != 0;
    const uint32_t voice0 = (blockIdx.x - a.block0) * (uint32_t)kBlkVoices;
    const uint32_t n_act = min((uint32_t)kBlkVoices, V - voice0);
    const bool active = (uint32_t)g < n_act;
    const uint32_t voice = voice0 + (uint32_t)g, vc = active ? voice : voice0 + n_act - 1u;
    auto row = [&](int rr) { return a.table[(size_t)rr * V + vc]; };
    auto parv = [&](const DevOp& op, int k) { return op.par_row[k] >= 0 ? __uint_as_float(row(op.par_row[k])) : op.par_val[k]; };

    const DevOp& ofb = a.ops[r.adsr];    // roles as in render_fm_pair_ring
    const DevOp& om = a.ops[r.osc_l];
    const DevOp& oix = a.ops[r.vca];
    const DevOp& ocr = a.ops[r.osc_a];
    const int plane = a.ops[r.out].aux;
    float* const ring = a.rings + (size_t)r.track * B * V;

    constexpr uint32_t fo = OSC_HAS_CV | OSC_CV_AUDIO_RATE | OSC_AA | OSC_OUT_SINE;
    constexpr uint32_t fo_mod = fo | OSC_EXACT, fo_carrier = fo | OSC_SINE_LOOSE;
    OscConst km, kc;
    double pos_m = make_f64(row(om.state_row + OSC_S_POS_LO), row(om.state_row + OSC_S_POS_HI));  // (scan lanes: the phase at the start of the next chunk to scan)
    double pos_c = make_f64(row(ocr.state_row + OSC_S_POS_LO), row(ocr.state_row + OSC_S_POS_HI));
    km.sr = om.sample_rate;
    km.val = (double)parv(om, OSC_P_VAL);
    km.delta = 0.0;
    km.inv_dt = 0.0f;
    kc = km;
    kc.sr = ocr.sample_rate;
    kc.val = (double)parv(ocr, OSC_P_VAL);
    kc.scale = (440.0 / kc.sr) * exp2(kc.val);
    const float c_fb = parv(ofb, MATH_P_CONST), c_ix = parv(oix, MATH_P_CONST);
    BlkConsts K;
    blk_consts_load<true>(K);  // (the carrier's 2^cv at degree 9: OSC_CV_SERIES9)
    XConsts X;
    x_consts_load(X);
    const LibmTabLds libm{tab};

    if (tid == 0) flag[0] = flag[1] = 0u;
    for (int k = tid; k < 256; k += kBlkVoices * kBlkSlices) tab[k] = kLibmExpTab[k];
    __syncthreads();
    bool unit = true;  // the ring: HBM -> LDS, looking at every value on the way (the host's may be anything; a sine is at most 1)
    for (uint32_t p = (uint32_t)s; p < B; p += (uint32_t)kBlkSlices) {
        const float x = ring[(size_t)p * V + vc];
        ring_l[p * kBlkVoices + (uint32_t)g] = x;
        unit = unit && __builtin_fabsf(x) <= 1.0f;
    }
    if (!unit) atomicOr(flag + 1, 1u);
    __syncthreads();
    // every wave holds all 32 voices (two slices of each): its ballots speak for the workgroup
    const OscFacts cf = fm_osc_facts(c_ix, kc, pos_c);
    const int car_class = fm_gain_class(c_ix);
    const double biggest = kc.scale * exp2((double)__builtin_fabsf(c_ix));  // (a prefix sum adds a chunk's increments before it wraps: see the kernel above)
    const bool sane = cf.tame && __builtin_amdgcn_ballot_w64(!(biggest <= 1048576.0)) == 0;
    // What the modulator's arithmetic may skip once it is PROVED for the launch: |cv| <= |gain| (the ring holds sines: looked at above) and
    // |gain| + |val| <= 800 put every exponent within pow's plain range on the large side and every increment, 440 * 2^e / sr, within the
    // normal range and below 2^52 — no test of the quotient, no look at the increments, a phase that stays in [0, 1): the wrap is the one
    // instruction, the sine needs no range check.  (The SMALL side of pow's plain range — |e ln 2| < 2^-54, e = 0 among them: a silent ring —
    // is an argument's own business and stays tested per sample.)
    const bool mod_ok = (double)__builtin_fabsf(c_fb) + __builtin_fabs(km.val) <= 800.0 && km.sr >= 1.0 && km.sr <= 65535.0 && pos_m >= 0.0 && pos_m < 1.0;
    const bool proved = flag[1] == 0u && __builtin_amdgcn_ballot_w64(!mod_ok) == 0;
    if (!(pos_m >= 0.0 && pos_m < 1.0)) atomicOr(flag, 1u);  // (only a host can store such a phase: the scan then wraps with fmod1)
    uint32_t p0 = (uint32_t)(a.n0 % B);
    const uint32_t i0 = (uint32_t)s * (uint32_t)kXPer;  // this lane's first sample of a chunk
    float* const frame_base = a.frames ? a.frames + (size_t)plane * a.plane_stride + voice0 : nullptr;
    float* const mp = a.mixpart ? a.mixpart + ((size_t)plane * a.n_waves + (blockIdx.x - a.block0)) * a.t_stride : nullptr;
    const bool frames = kOut == 0 ? frame_base != nullptr : (kOut & 1) != 0;
    const bool mix = kOut == 0 ? mp != nullptr : (kOut & 2) != 0;
    const double inv_sr = 1.0 / km.sr;

    // kFast: the modulator proved (above), every chunk whole (the launch's length a multiple of 64), no slice wraps inside the ring (its length
    // and position multiples of 4) and all 32 voices real — no masks, no selects, ring addresses as instruction offsets
    auto run = [&](auto fc_c, auto fast_c) {
        constexpr uint32_t FC = decltype(fc_c)::value;
        constexpr bool kFast = decltype(fast_c)::value;
        const uint32_t n_chunks = (a.T + (uint32_t)kXChunk - 1u) / (uint32_t)kXChunk;
        // the ring's word for this lane's sample j of a chunk whose first sample of this slice sits at ring position `at` (below B; B >= 4)
        auto ring_at = [&](uint32_t at, int j) {
            if (kFast) return (at + (uint32_t)j) * (uint32_t)kBlkVoices + (uint32_t)g;
            const uint32_t p = at + (uint32_t)j;
            return (p >= B ? p - B : p) * (uint32_t)kBlkVoices + (uint32_t)g;
        };
        auto ring_step = [&](uint32_t at) {  // ... one chunk on (B >= 256 > 64)
            const uint32_t p = at + (uint32_t)kXChunk;
            return p >= B ? p - B : p;
        };
        auto live = [&](uint32_t chunk, int j) { return kFast || chunk * (uint32_t)kXChunk + i0 + (uint32_t)j < a.T; };
        // the modulator's increments of a chunk, from what the ring holds: 440 * 2^(f64(cv) + f64(val)) / sr (oscillator.rs:43-48,132)
        // (`redo`: the lanes whose plain forms could not decide — the reference's expression itself, the same value wherever they had.  The
        // question "could some lane not decide" is asked ONCE per iteration, after its arithmetic, for increments and sines together: a branch
        // in the middle fences the iteration's two halves off from each other — 13.7 against 12.7 ms per step without any question)
        auto increments = [&](uint32_t chunk, uint32_t at, double (&d)[kXPer], bool& cold, bool redo) {
            float fed[kXPer];
#pragma unroll
            for (int j = 0; j < kXPer; j++) fed[j] = ring_l[ring_at(at, j)];
            double e[kXPer];
#pragma unroll
            for (int j = 0; j < kXPer; j++) {
                e[j] = (double)(fed[j] * c_fb) + km.val;
                if (redo) {
                    d[j] = osc_delta_exact_cold(e[j], km.sr);
                } else {
                    const double pw = X.k440 * x_exp2_libm_plain(X, e[j], cold, libm);
                    d[j] = kFast ? div_rn_proved(pw, km.sr, inv_sr) : div_rn_plain(pw, km.sr, cold);
                }
            }
            if (!kFast) {
                bool ordinary = true;
#pragma unroll
                for (int j = 0; j < kXPer; j++) {
                    ordinary = ordinary && d[j] >= 0.0 && d[j] < 4503599627370496.0;
                    d[j] = live(chunk, j) ? d[j] : 0.0;  // (past the launch's last sample: the phase stands still)
                }
                if (!ordinary) atomicOr(flag, 1u);
            }
        };
        // the scan: chunk's increments in `buf` -> its phases, in place; lanes 0 .. 31 of wave 0, one voice each
        auto scan = [&]() {
#ifdef SRK_X_NOSCAN
            return;  // (timing experiment only)
#endif
            if (tid >= kBlkVoices) return;
            double p = pos_m;
            double* const col = buf + g;
            if (kFast || flag[0] == 0u) {
#pragma unroll 1
                for (int t0 = 0; t0 < kXChunk; t0 += 16) {
                    double d[16];
#pragma unroll
                    for (int t = 0; t < 16; t++) d[t] = col[(t0 + t) * kBlkVoices];
#pragma unroll
                    for (int t = 0; t < 16; t++) {
                        col[(t0 + t) * kBlkVoices] = p;
                        p = __builtin_amdgcn_fract(p + d[t]);   // pos += delta; pos %= 1.0 — exact for ordinary increments and a phase in [0, 1)
                    }
                }
            } else {
                for (int t = 0; t < kXChunk; t++) {
                    const double d = col[t * kBlkVoices];
                    col[t * kBlkVoices] = p;
                    p = fmod1(p + d);
                }
            }
            pos_m = p;
        };
        // where a lane's slice starts (carrier): the phase at the chunk's first sample + the totals of the slices below it
        // (returns the OTHER slice of this wave's pair: the odd slice starts behind the even one's total — taken as it is, not as pair - mine: a
        // voice whose modulator has just overflowed has a NaN in ITS slice's total, and the samples before it must not inherit it)
        auto slice_totals = [&](int parity, double mine) {
            const double other = __shfl_xor(mine, 32);
            if (!odd) sums[(parity * 8 + w) * kBlkVoices + g] = mine + other;
            return other;
        };
        auto slice_base = [&](int parity, double mine, double other, double start, double& base, double& total) {
            // (the waves below this one: a wave-uniform count.  A product with a scalar 0 / 1 — one fma per wave where an addition behind a
            // select costs three instructions, two scalar-count loops more still (measured: 13.7 / 14.5 / 14.6 ms per step) — unless a total is
            // a NaN: a voice whose modulator has overflowed hands them on, and they must not reach the slices BEFORE them: then the selects)
            base = start;
            total = 0.0;
#pragma unroll
            for (int w2 = 0; w2 < 8; w2++) {
                const double v = sums[(parity * 8 + w2) * kBlkVoices + g];
                total += v;
                base = __builtin_fma(v, w2 < w ? 1.0 : 0.0, base);
            }
            if (__builtin_amdgcn_ballot_w64(total != total) != 0) {
                base = start;
#pragma unroll
                for (int w2 = 0; w2 < 8; w2++) {
                    const double v = sums[(parity * 8 + w2) * kBlkVoices + g];
                    base = w2 < w ? base + v : base;
                }
            }
            (void)mine;
            if (odd) base += other;
        };
        // frames and mix partial of a chunk whose carrier phases are known
        auto emit = [&](uint32_t chunk, const double (&pre)[kXPer], double base) {
            const uint32_t t0 = chunk * (uint32_t)kXChunk;
            float out[kXPer];
#pragma unroll
            for (int j = 0; j < kXPer; j++) out[j] = blk_sine_loose(__builtin_amdgcn_fract(base + pre[j]));
            if (frames && (kFast || active)) {
                const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(frame_base + (size_t)(t0 + (uint32_t)w * 2u * (uint32_t)kXPer) * V, 0, 0x7fffffff, 0x00020000);
                const uint32_t voff = ((uint32_t)g + (odd ? (uint32_t)kXPer * V : 0u)) * 4u;
#pragma unroll
                for (int j = 0; j < kXPer; j++)
                    if (live(chunk, j)) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(out[j]), rsrc, (int)voff, (int)((uint32_t)j * V * 4u), SRK_FRAME_AUX);
            }
            if (mix) {
                // sum over the 32 voices of each of this slice's 4 samples: 4 -> 2 -> 1 values per lane while lanes pair up (g ^ 1, g ^ 2), then
                // plain butterflies over the remaining voice bits: lane g ends with sample (g & 3) of its slice
                float v[kXPer];
#pragma unroll
                for (int j = 0; j < kXPer; j++) v[j] = (kFast || active) ? out[j] : 0.0f;
                {
                    const bool up = (g & 1) != 0;
                    const float s0 = up ? v[0] : v[2], s1 = up ? v[1] : v[3], k0 = up ? v[2] : v[0], k1 = up ? v[3] : v[1];
                    v[0] = k0 + row_xchg<1>(s0);
                    v[1] = k1 + row_xchg<1>(s1);
                }
                {
                    const bool up = (g & 2) != 0;
                    const float send = up ? v[0] : v[1], keep_ = up ? v[1] : v[0];
                    v[0] = keep_ + row_xchg<2>(send);
                }
                float sum = v[0];
                sum += __shfl_xor(sum, 4);
                sum += __shfl_xor(sum, 8);
                sum += __shfl_xor(sum, 16);
                const int mine_j = ((g & 1) ? 2 : 0) + ((g & 2) ? 1 : 0);  // which of the slice's samples this lane ended up with
                if (g < 4 && (kFast || t0 + i0 + (uint32_t)mine_j < a.T)) mp[t0 + i0 + (uint32_t)mine_j] = sum;
            }
        };

        // ---- prologue: increments of chunks 0 and 1, phases of chunk 0 ----
        double dM[kXPer];
        uint32_t at_k = (p0 + i0) % B;                     // ring position of this slice's first sample of chunk k ...
        uint32_t at_inc = at_k;                            // ... and of the chunk whose increments are computed next
        {
            bool cold = false;
            increments(0u, at_inc, dM, cold, false);
            if (__builtin_amdgcn_ballot_w64(cold) != 0) increments(0u, at_inc, dM, cold, true);
        }
        at_inc = ring_step(at_inc);
#pragma unroll
        for (int j = 0; j < kXPer; j++) buf[(i0 + (uint32_t)j) * kBlkVoices + (uint32_t)g] = dM[j];
        __syncthreads();
        scan();
        if (n_chunks > 1u) {
            bool cold = false;
            increments(1u, at_inc, dM, cold, false);
            if (__builtin_amdgcn_ballot_w64(cold) != 0) increments(1u, at_inc, dM, cold, true);
        }
        at_inc = ring_step(at_inc);
        __syncthreads();
        double preC[kXPer] = {0.0, 0.0, 0.0, 0.0}, pairC = 0.0, mineC = 0.0;  // the carrier's local prefix / totals of the chunk whose frames are still to come
        for (uint32_t k = 0; k < n_chunks; k++) {
            double pM[kXPer];
#pragma unroll
            for (int j = 0; j < kXPer; j++) pM[j] = buf[(i0 + (uint32_t)j) * kBlkVoices + (uint32_t)g];
            // (no barrier here: a lane overwrites exactly the entries it has just read; the scan, which reads everybody's, is behind the next one)
            if (k + 1u < n_chunks) {
#pragma unroll
                for (int j = 0; j < kXPer; j++) buf[(i0 + (uint32_t)j) * kBlkVoices + (uint32_t)g] = dM[j];
            }
            __syncthreads();
            if (k + 1u < n_chunks) scan();
            if (k > 0u) {  // the carrier's frames of chunk k - 1 (its slice totals crossed on the barriers above)
                double base, total;
                slice_base((int)((k - 1u) & 1u), mineC, pairC, pos_c, base, total);
                emit(k - 1u, preC, base);
                pos_c = __builtin_amdgcn_fract(pos_c + total);
            }
            // sines of chunk k -> ring; the carrier's increments, their local prefix and slice totals; the modulator's increments of chunk k + 2
            auto second_half = [&](bool& cold, bool redo) {
                float sine[kXPer];
#pragma unroll
                for (int j = 0; j < kXPer; j++) {
                    if (redo) {
                        double unused = 0.0;
                        osc_exact_cold(0.0, 1.0, pM[j], false, unused, sine[j]);
                    } else {
                        sine[j] = x_sine_exact_plain<!kFast>(X, pM[j], cold);  // (pos * PI * 2).sin() as f32, oscillator.rs:133
                    }
                }
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j < kXPer; j++) {
                    double d = fm_increment<FC>(K, kc, sine[j] * c_ix);
                    const bool lv = live(k, j);
                    if (lv) ring_l[ring_at(at_k, j)] = sine[j];
                    if (!kFast) d = lv ? d : 0.0;
                    preC[j] = acc;
                    acc += d;
                }
                mineC = acc;
                pairC = slice_totals((int)(k & 1u), acc);
                if (k + 2u < n_chunks) increments(k + 2u, at_inc, dM, cold, redo);
            };
            bool cold = false;
            second_half(cold, false);
#ifndef SRK_X_NOCOLD
            if (__builtin_amdgcn_ballot_w64(cold) != 0) second_half(cold, true);  // (3.4e-6 of the samples: this wave's part of the iteration again, every value the reference's own)
#endif
            at_k = ring_step(at_k);
            at_inc = ring_step(at_inc);
            __syncthreads();
        }
        {   // the last chunk's frames
            double base, total;
            slice_base((int)((n_chunks - 1u) & 1u), mineC, pairC, pos_c, base, total);
            emit(n_chunks - 1u, preC, base);
            pos_c = __builtin_amdgcn_fract(pos_c + total);
        }
    };
    const bool fast = proved && (a.T % (uint32_t)kXChunk) == 0u && (B % (uint32_t)kXPer) == 0u && (p0 % (uint32_t)kXPer) == 0u && n_act == (uint32_t)kBlkVoices;
    if (a.T == 0u) {
        // nothing to render: the ring goes back as it came
    } else if (sane) {
        using std::integral_constant;
        using std::true_type;
        using std::false_type;
        constexpr uint32_t P = OSC_PHASE_TAME | OSC_VAL_FOLDED | OSC_CV_SERIES9;
        // (the fast copy for the class config 4's draw takes — index 0.5 ... 1.5: (2^(cv/4))^4 —; the general one for every class)
        if (car_class == 2)
            run(integral_constant<uint32_t, fo_carrier | P | OSC_CV_SMALL>{}, false_type{});
        else if (car_class == 1 && fast)
            run(integral_constant<uint32_t, fo_carrier | P | OSC_CV_QUAD>{}, true_type{});
        else if (car_class == 1)
            run(integral_constant<uint32_t, fo_carrier | P | OSC_CV_QUAD>{}, false_type{});
        else
            run(integral_constant<uint32_t, fo_carrier | P>{}, false_type{});
    } else if (s == 0) {  // the recurrence, sample by sample, one lane per voice
        OscRegs sm, sc;
        sm.pos = pos_m;
        sc.pos = pos_c;
        sm.sync_last = sc.sync_last = false;
        float sq = 0.0f, sw = 0.0f;
        for (uint32_t t = 0; t < a.T; t++) {
            const uint32_t at = p0 * (uint32_t)kBlkVoices + (uint32_t)g;
            float sine_m = 0.0f, out = 0.0f;
            osc_step(fo_mod, sm, km, ring_l[at] * c_fb, 0.0f, sine_m, sq, sw);
            ring_l[at] = sine_m;
            osc_step(fo_carrier, sc, kc, sine_m * c_ix, 0.0f, out, sq, sw);
            if (frames && active) frame_base[(size_t)t * V + (uint32_t)g] = out;
            if (mix) {
                float v = active ? out : 0.0f;
#pragma unroll
                for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m);
                if (g == 0) mp[t] = v;
            }
            p0 = p0 + 1u == B ? 0u : p0 + 1u;
        }
        pos_m = sm.pos;
        pos_c = sc.pos;
    }
    __syncthreads();  // the last chunk's ring writes
    if (active) {
        for (uint32_t p = (uint32_t)s; p < B; p += (uint32_t)kBlkSlices) ring[(size_t)p * V + voice] = ring_l[p * kBlkVoices + (uint32_t)g];
        if (s == 0) {
            auto put = [&](int rr, uint32_t v) { a.table[(size_t)rr * V + voice] = v; };
            put(om.state_row + OSC_S_POS_LO, f64_lo(pos_m));   // (slice 0 = the scan lanes)
            put(om.state_row + OSC_S_POS_HI, f64_hi(pos_m));
            put(om.state_row + OSC_S_SYNC_LAST, 0u);
            put(ocr.state_row + OSC_S_POS_LO, f64_lo(pos_c));
            put(ocr.state_row + OSC_S_POS_HI, f64_hi(pos_c));
            put(ocr.state_row + OSC_S_SYNC_LAST, 0u);
        }
    }
}

}  // namespace srack
