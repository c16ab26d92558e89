// fm_common.hip.h — what the FM-pair kernels of fm_pair.hip.h and fm_block.hip.h share: the wave-uniform facts their sample loops are
// picked by, and the exact modulator's forms with their constants in registers.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "kernel_args.hip.h"
#include "modules.hip.h"
#include "wave.hip.h"

namespace srack {

// Wave-uniform facts about an FM pair's voices (default mode), from which the kernels below pick their sample loop.  Inactive lanes
// mirror a real voice (WaveMap::vc), so every lane votes.  In the proved loops the increment is scale * 2^cv with scale = 440 / sr * 2^val
// per voice (OSC_VAL_FOLDED), so what matters is |cv| <= |gain| (the fed-back value is a sine: at most 1, checked where it enters).
struct FmFacts {
    bool tame = false;  // |gain| + |val| below 1000 per oscillator, both phases in [0, 1), sample rates >= 1: increments finite and >= 0
    int mod = 0, car = 0;  // per oscillator: 2 = |gain| <= 1/2 (no range reduction), 1 = |gain| <= 2 ((2^(cv/4))^4), 0 = range reduction
};
using dev::fm_gain_class;  // modules.hip.h: shared with the kernels specialised at run time
SRK_DEV FmFacts fm_facts(float c_fb, const dev::OscConst& km, double pos_m, float c_ix, const dev::OscConst& kc, double pos_c)
{
    // the exponent of an increment is val + cv with |cv| <= |gain|: the SUM has to stay clear of 2^x's overflow (val = 600 with gain = 600 would
    // not), and then scale = 440 / sr * 2^val and scale * 2^cv are finite too
    const bool sizes = (double)__builtin_fabsf(c_fb) + __builtin_fabs(km.val) < 1000.0 && (double)__builtin_fabsf(c_ix) + __builtin_fabs(kc.val) < 1000.0;
    const bool phases = pos_m >= 0.0 && pos_m < 1.0 && pos_c >= 0.0 && pos_c < 1.0;
    const bool rates = km.sr >= 1.0 && kc.sr >= 1.0 && sizes && dev::osc_below_rate(c_fb, km.val, km.sr) && dev::osc_below_rate(c_ix, kc.val, kc.sr);  // 440 / sr finite, increments below a cycle per sample (modules.hip.h)
    FmFacts f;
    f.tame = __builtin_amdgcn_ballot_w64(!(sizes && phases && rates)) == 0;  // NaNs vote no
    f.mod = fm_gain_class(c_fb);
    f.car = fm_gain_class(c_ix);
    return f;
}
// the proved sample loops: tile(modulator flags, carrier flags) for the facts' classes
template <uint32_t kMod, uint32_t kCar, class Tile>
SRK_DEV void fm_proved_tile(const FmFacts& f, Tile&& tile)
{
    using std::integral_constant;
    constexpr uint32_t P = OSC_PHASE_TAME | OSC_VAL_FOLDED;
    auto with_car = [&](auto m) {
        constexpr uint32_t M = kMod | P | decltype(m)::value;
        if (f.car == 2)
            tile(integral_constant<uint32_t, M>{}, integral_constant<uint32_t, kCar | P | OSC_CV_SMALL>{});
        else if (f.car == 1)
            tile(integral_constant<uint32_t, M>{}, integral_constant<uint32_t, kCar | P | OSC_CV_QUAD>{});
        else
            tile(integral_constant<uint32_t, M>{}, integral_constant<uint32_t, kCar | P>{});
    };
    if (f.mod == 2)  // (a feedback gain between 1/2 and 2 takes the range reduction: three more copies of every loop for one more instruction pair)
        with_car(integral_constant<uint32_t, OSC_CV_SMALL>{});
    else
        with_car(integral_constant<uint32_t, 0u>{});
}

struct OscFacts {
    bool tame = false, small = false;  // as FmFacts, for one oscillator
};
SRK_DEV OscFacts fm_osc_facts(float gain, const dev::OscConst& k, double pos)
{
    const float e = __builtin_fabsf(gain) + __builtin_fabsf((float)k.val);
    OscFacts f;
    f.tame = __builtin_amdgcn_ballot_w64(!(e < 1000.0f && pos >= 0.0 && pos < 1.0 && k.sr >= 1.0 && dev::osc_below_rate(gain, k.val, k.sr))) == 0;
    f.small = __builtin_amdgcn_ballot_w64(!(e <= 0.4999f)) == 0;
    return f;
}

struct LibmTabLds {
    const uint64_t* t;
    SRK_DEV uint64_t operator()(uint32_t i) const { return t[i]; }
};
// The exact forms' constants as REGISTERS (as BlkConsts above: an f64 VOP3 cannot take a 64-bit literal, and with four evaluations in flight the
// compiler rematerialised every one at every use — 95 of the chunk loop's 544 vector instructions were moves).  The operations below are
// dev::exp2_libm_plain_t's and dev::sine_exact_plain's own (modules.hip.h), operation for operation: same values, same roundings.
struct XConsts {
    double lhi, llo, inv_ln2n, shift, nln2hi, nln2lo, c2, c3, c4, c5, k440;  // 2^e as the host libm's pow
    double q[7], quarter, rel, abs_;                                          // the sine's polynomial, its fold, the decision's interval
};
SRK_DEV void x_consts_load(XConsts& X)
{
    X.lhi = 0x1.62e42fefa39efp-1, X.llo = 0x1.abc9e3b398000p-56, X.inv_ln2n = 0x1.71547652b82fep+7, X.shift = 0x1.8p52;
    X.nln2hi = -0x1.62e42fefa0000p-8, X.nln2lo = -0x1.cf79abc9e3b3ap-47;
    X.c2 = 0x1.ffffffffffdbdp-2, X.c3 = 0x1.555555555543cp-3, X.c4 = 0x1.55555cf172b91p-5, X.c5 = 0x1.1111167a4d017p-7, X.k440 = 440.0;
    const double q[7] = {6.283185307179272, -41.34170223990684, 81.60524914955879, -76.70584757807868, 42.05813586028645, -15.081496425342264, 3.6659216216293173};
#pragma unroll
    for (int i = 0; i < 7; i++) X.q[i] = q[i];
    X.quarter = 0.25, X.rel = 1.0e-13, X.abs_ = 2.0e-15;
    double* const all = &X.lhi;
    static_assert(sizeof(XConsts) == 21 * sizeof(double), "XConsts is 21 doubles in a row");
#pragma unroll
    for (int i = 0; i < 21; i++) asm volatile("" : "+v"(all[i]));
}
template <class Tab>
SRK_DEV double x_exp2_libm_plain(const XConsts& X, double e, bool& cold, const Tab& tab)  // == dev::exp2_libm_plain_t(e, cold, tab)
{
    const double ehi = e * X.lhi;
    const double elo = __builtin_fma(e, X.llo, __builtin_fma(X.lhi, e, -ehi));
    const uint32_t abstop = ((uint32_t)__double2hiint(ehi) >> 20) & 0x7ffu;
    cold = cold || !(abstop - 0x3c9u <= 0x3eu);
    const double kds = __builtin_fma(ehi, X.inv_ln2n, X.shift);
    const uint64_t ki = (uint64_t)__double_as_longlong(kds);
    const double kd = kds - X.shift;
    double r = __builtin_fma(kd, X.nln2lo, __builtin_fma(kd, X.nln2hi, ehi));
    r = elo + r;
    const uint32_t idx = 2u * ((uint32_t)ki & 127u);
    const double tail = __longlong_as_double((long long)tab(idx));
    const uint64_t sbits = tab(idx + 1u) + (ki << 45);
    const double r2 = r * r;
    const double a = __builtin_fma(r, X.c3, X.c2);
    const double b = r + tail;
    const double c = __builtin_fma(r, X.c5, X.c4);
    double tmp = __builtin_fma(a, r2, b);
    tmp = __builtin_fma(c, r2 * r2, tmp);
    const double scale = __longlong_as_double((long long)sbits);
    return __builtin_fma(tmp, scale, scale);
}
template <bool kRange>
SRK_DEV float x_sine_exact_plain(const XConsts& X, double pos, bool& cold)  // == dev::sine_exact_plain<kRange>(pos, cold)
{
    const double qn = 0.5 - pos;
    const uint32_t sign = (uint32_t)__double2hiint(qn) & 0x80000000u;
    const double t = __builtin_fabs(qn) - X.quarter;
    const double x = X.quarter - __builtin_fabs(t);
    const double z = x * x;
    const double a01 = __builtin_fma(X.q[1], z, X.q[0]);
    const double a23 = __builtin_fma(X.q[3], z, X.q[2]);
    const double a45 = __builtin_fma(X.q[5], z, X.q[4]);
    const double z2 = z * z;
    const double b0 = __builtin_fma(a23, z2, a01);
    const double b1 = __builtin_fma(X.q[6], z2, a45);
    const double z4 = z2 * z2;
    const double y = __builtin_fma(b1, z4, b0) * x;
    const double d = __builtin_fma(X.rel, y, X.abs_);
    const float r = (float)(y - d), r2 = (float)(y + d);
    bool sure = __float_as_uint(r) == __float_as_uint(r2);
    if (kRange) sure = sure && pos >= 0.0 && pos < 1.0;
    cold = cold || !sure;
    return __uint_as_float(__float_as_uint(r) ^ sign);
}

}  // namespace srack
