// busshape.hip.h — the bus shapers (srack_buses_shaper): a drive, a waveshaper and a make-up gain per channel on every mix bus, behind the mixer.
//
// Channel c (0 or 1) of a bus that is not OFF is three reference modules in series, ticked once per sample: MathModule(Multiply) by PRE,
// NonLinearModule (math.rs:203-205: sign(a) |a|^b, a sample that is not > 0 — both zeros and NaN — through -(-a).powf(b)), its exponent
// the bus's EXPONENT or, in mode CV, the bus's row cv[b][t], and MathModule(Multiply) by POST.  The unit is built with -ffp-contract=off:
// the two products are the reference's f32 products, one rounding each (modules.hip.h: math_step), and the power is nonlin_step with
// NONLIN_EXACT — the host libm's powf operation for operation, its misroundings included (modules.hip.h: powf_libm_plain).  Nothing of
// that arithmetic is restated here.
//
// The stage is stateless and elementwise, so the lanes stay on time and every access is a whole line.  A wave takes a stretch of one
// bus — kBusShpStretch samples — and walks it in steps of kBusShpLoads x 64 samples: the step's loads (the exponent words first when the
// bus is CV, then both used channels) are issued together and are in flight at once; then every word goes through the three modules and
// is stored by the lane that read it.  The bus's table entry is read once per wave and the exponent words once per step: both channels
// use them.  A workgroup is kBusShpWaves such waves on neighbouring stretches; what they share is the libm's two tables (16 x 2 + 32
// u64, 512 bytes), copied into LDS by the first wave before anything else and handed to nonlin_step as LdsTables: a lane's own index is
// a ds_read there, and a gather for the vector-memory pipe through the global pointer (modules.hip.h: P4 was bound by exactly that).
//
// The cold path — a zero, infinite or NaN argument, an exponent that is 0 or not finite — is powf_pos's own: one wave-uniform ballot
// around the out-of-line powf_cold.  A CONST bus's exponent is wave-uniform, so a bus whose exponent is 0 or not finite is cold as a
// whole: correct, not fast.  A lane past the end of the row computes on 1.0 (and a CV of 1.0) and stores nothing: tails are masked, never
// padded, and they do not send a wave of ordinary samples down the cold path.
//
// The buses a call works on come from a list (a.list: the buses that are not OFF, made on the host) when out is rows itself — nothing is
// launched for an OFF bus — and are all buses otherwise: an OFF bus's words are then copied, 32 bits at a time.  In place is safe: a
// word is read and written by the same lane, read first.  Nothing needs more than 4-byte alignment.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "launch_types.hpp"
#include "modules.hip.h"

namespace srack {

constexpr int kBusShpWaves = 4;                       // waves per workgroup, each on a stretch of its own
constexpr int kBusShpLoads = 4;                       // loads per row a wave has in flight: a step is kBusShpLoads x 64 samples
constexpr int kBusShpStep = kBusShpLoads * 64;
constexpr int kBusShpStretch = kBusShaperStretch;     // samples of one bus a wave takes (launch_types.hpp: the host counts the stretches)
static_assert(kBusShpStretch % kBusShpStep == 0, "whole steps");

// grid (ceil(n_work * ceil(n / kBusShpStretch) / kBusShpWaves)), block kBusShpWaves * 64.  kUsed: a.used, 1 or 2 — the channels of a bus that are processed.
template <int kUsed>
__global__ __launch_bounds__(kBusShpWaves * 64) void bus_shaper(const BusShaperArgs a)
{
    using namespace dev;
    __shared__ uint64_t s_tab[64];  // kPowfLog2Tab [16][2], then kExp2fTab [32]
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave == 0) s_tab[lane] = lane < 32 ? ((const uint64_t*)kPowfLog2Tab)[lane] : kExp2fTab[lane - 32];
    __syncthreads();
    LdsTables tabs;  // (assigned, not brace-initialised: a constant initialiser may not cast into the LDS address space)
    tabs.log2_tab = (LdsTab*)s_tab;
    tabs.exp2f_tab = tabs.log2_tab + 32;

    const uint32_t unit = blockIdx.x * (uint32_t)kBusShpWaves + wave;  // (wave-uniform from here on)
    if (unit >= a.n_units) return;
    const uint32_t k = unit / a.n_stretches;
    const uint32_t b = a.list ? a.list[k] : k;
    const uint32_t t_begin = (unit - k * a.n_stretches) * (uint32_t)kBusShpStretch;
    const uint32_t t_end = min(a.n, t_begin + (uint32_t)kBusShpStretch);
    const BusShaperBus me = a.tab[b];
    const bool off = me.mode == (uint32_t)SRACK_BUS_SHAPER_OFF;
    const bool has_cv = me.mode == (uint32_t)SRACK_BUS_SHAPER_CV && a.cv;  // (a CV bus without a row: In2 unconnected, the exponent is EXPONENT)
    const uint32_t mul = MATH_HAS_IN1 | ((uint32_t)SRACK_MATH_MULTIPLY << MATH_OP_SHIFT);
    const uint32_t pw = MATH_HAS_IN1 | NONLIN_EXACT | (has_cv ? MATH_HAS_IN2 : 0u);

    const uint32_t* rows = reinterpret_cast<const uint32_t*>(a.rows) + (size_t)b * a.row_channels * a.n;
    const uint32_t* cv = reinterpret_cast<const uint32_t*>(a.cv) + (size_t)b * a.n;
    uint32_t* out = reinterpret_cast<uint32_t*>(a.out) + (size_t)b * a.row_channels * a.n;

    for (uint32_t t0 = t_begin; t0 < t_end; t0 += (uint32_t)kBusShpStep) {
        uint32_t e[kBusShpLoads], x[kUsed][kBusShpLoads];
#pragma unroll
        for (int u = 0; u < kBusShpLoads; u++) {
            const uint32_t t = t0 + (uint32_t)u * 64u + lane;
            e[u] = 0x3f800000u;
            if (has_cv && t < t_end) e[u] = cv[t];
        }
#pragma unroll
        for (int c = 0; c < kUsed; c++) {
#pragma unroll
            for (int u = 0; u < kBusShpLoads; u++) {
                const uint32_t t = t0 + (uint32_t)u * 64u + lane;
                x[c][u] = 0x3f800000u;
                if (t < t_end) x[c][u] = rows[(size_t)c * a.n + t];
            }
        }
        if (off) {  // (out of place only: in place an OFF bus is not in the list)
#pragma unroll
            for (int c = 0; c < kUsed; c++) {
#pragma unroll
                for (int u = 0; u < kBusShpLoads; u++) {
                    const uint32_t t = t0 + (uint32_t)u * 64u + lane;
                    if (t < t_end) out[(size_t)c * a.n + t] = x[c][u];
                }
            }
            continue;
        }
#pragma unroll
        for (int c = 0; c < kUsed; c++) {
#pragma unroll
            for (int u = 0; u < kBusShpLoads; u++) {
                const uint32_t t = t0 + (uint32_t)u * 64u + lane;
                const float driven = math_step(mul, __uint_as_float(x[c][u]), 0.0f, me.pre);
                const float shaped = nonlin_step(pw, driven, __uint_as_float(e[u]), me.exponent, tabs);
                const float y = math_step(mul, shaped, 0.0f, me.post);
                if (t < t_end) out[(size_t)c * a.n + t] = __float_as_uint(y);
            }
        }
    }
}

}  // namespace srack
