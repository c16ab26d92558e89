// The ladder's vote on its clamp behind the cubic (csrc/modules.hip.h, vcf_b4_bounded_lane) against the ladder itself, on the host with the
// real fmaf.  tests/test_vcf_bound_host.py cuts VcfRegs, clamp1, vcf_polys, vcf_step and the vote out of modules.hip.h into
// vcf_bound_excerpt.tmp (the device header itself needs the HIP runtime) and compiles this file with -ffp-contract=off, so that the
// literal form rounds every operation and the contracted form contracts exactly where it says fmaf.  Stand-alone: no input, one JSON
// line, exit status 0 unless it could not run; the assertions are the test's.
//
//   g++ -std=c++17 -O2 -ffp-contract=off -o vcf_bound_probe vcf_bound_probe.cpp && ./vcf_bound_probe
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#define SRK_DEV static inline
static inline float host_med3(float x, float lo, float hi)  // v_med3_f32 on non-NaN operands (a NaN: the smaller of the other two)
{
    if (x != x) return lo;
    return fmaxf(fminf(x, hi), lo);
}
#define __builtin_amdgcn_fmed3f host_med3
namespace srack {
namespace dev {
#include "vcf_bound_excerpt.tmp"
}
}
using namespace srack::dev;

static float next_down(float x) { return std::nextafterf(x, -INFINITY); }
static uint32_t ord(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }   // positive floats: ordered as their bits
static float unord(uint32_t u) { float x; std::memcpy(&x, &u, 4); return x; }

struct Tally {
    double pass_max_g[2] = {0, 0}, fail_max_g[2] = {0, 0};   // [form]: 0 = contracted (default mode), 1 = literal
    double pass_max_pre = 0;
    long n = 0, n_pass = 0, pass_over = 0, fail_over_one = 0;
};

template <bool kFast>
static VcfRegs coeffs(float cutoff, float res)
{
    VcfRegs s{};
    vcf_polys<kFast>(cutoff, res, s.p, s.f, s.q);
    s.freq = cutoff;
    s.res = res;
    return s;
}

// the fourth stage and the cubic alone, on an operand sum = b3' + b3 given from outside (the issue's model of the stage)
template <bool kFast>
static float stage4(const VcfRegs& s, float sum, float b4, float& pre)
{
    if (kFast) {
        pre = __builtin_fmaf(sum, s.p, -(b4 * s.f));
        return __builtin_fmaf(-(pre * pre * pre), 0.166667f, pre);
    }
    pre = sum * s.p - b4 * s.f;
    return pre - (pre * pre * pre) * 0.166667f;
}

template <bool kFast>
static void stage_point(Tally& t, float cutoff, float res, float sum, float b4)
{
    VcfRegs s = coeffs<kFast>(cutoff, res);
    s.b0 = s.b1 = s.b2 = s.b3 = 1.0f;
    s.b4 = b4;
    const bool vote = vcf_b4_bounded_lane(s);
    float pre;
    const double g = std::fabs((double)stage4<kFast>(s, sum, b4, pre));
    const int form = kFast ? 0 : 1;
    t.n++;
    if (vote) {
        t.n_pass++;
        if (g > t.pass_max_g[form]) t.pass_max_g[form] = g;
        if (std::fabs((double)pre) > t.pass_max_pre) t.pass_max_pre = std::fabs((double)pre);
        if (!(g <= (double)kVcfB4Bound)) t.pass_over++;
    } else {
        if (g > t.fail_max_g[form]) t.fail_max_g[form] = g;
        if (g > 1.0) t.fail_over_one++;
    }
}

// a whole step of the ladder WITHOUT the fifth clamp from a given state: the stages see the step's own b1 ... b3 unclamped
struct StepTally {
    double pass_max_b4[2] = {0, 0}, fail_max_b4[2] = {0, 0};
    long n = 0, n_pass = 0, pass_over = 0, fail_over_one = 0;
    long stage_only_pass = 0, stage_only_over_one = 0;   // points the bound 2p + |f| max(|b4|, B) <= 2.83 alone would pass, and those of them that leave [-1, 1]
    double stage_only_max_b4 = 0;
};

template <bool kFast>
static void step_point(StepTally& t, float cutoff, float res, const float b[5], float x)
{
    VcfRegs s = coeffs<kFast>(cutoff, res);
    s.b0 = b[0]; s.b1 = b[1]; s.b2 = b[2]; s.b3 = b[3]; s.b4 = b[4];
    const bool vote = vcf_b4_bounded_lane(s);
    const bool stage_only = 2.0f * s.p + std::fabs(s.f) * fmaxf(std::fabs(s.b4), kVcfB4Bound) <= kVcfB4PreMax;
    float lp, bp, hp;
    vcf_step<kFast, kFast, false>(s, x, lp, bp, hp);
    const double g = std::fabs((double)s.b4);
    const int form = kFast ? 0 : 1;
    t.n++;
    if (vote) {
        t.n_pass++;
        if (g > t.pass_max_b4[form]) t.pass_max_b4[form] = g;
        if (!(g <= (double)kVcfB4Bound)) t.pass_over++;
    } else {
        if (g > t.fail_max_b4[form]) t.fail_max_b4[form] = g;
        if (g > 1.0) t.fail_over_one++;
    }
    if (stage_only) {
        t.stage_only_pass++;
        if (g > 1.0) t.stage_only_over_one++;
        if (g > t.stage_only_max_b4) t.stage_only_max_b4 = g;
    }
}

// many steps without the fifth clamp behind a vote that passed: every b4 on the way must stay inside the bound
template <bool kFast>
static long run_points(std::mt19937& rng, float cutoff, float res, int steps, double& max_b4)
{
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    VcfRegs s = coeffs<kFast>(cutoff, res);
    s.b0 = u(rng); s.b1 = u(rng); s.b2 = u(rng); s.b3 = u(rng); s.b4 = u(rng);
    if (!vcf_b4_bounded_lane(s)) return 0;
    long over = 0;
    float sign = 1.0f;
    for (int i = 0; i < steps; i++) {
        if ((rng() & 15u) == 0) sign = -sign;   // a square-like input at the rim keeps the state near its corners
        const float x = (rng() & 3u) ? sign : u(rng);
        float lp, bp, hp;
        vcf_step<kFast, kFast, false>(s, x, lp, bp, hp);
        const double g = std::fabs((double)s.b4);
        if (g > max_b4) max_b4 = g;
        if (!(g <= (double)kVcfB4Bound)) over++;
    }
    return over;
}

// the largest cutoff in [0.3, 0.9] whose vote passes at this resonance with |b4| <= the bound (the vote's expression grows with the cutoff there)
static float threshold(float res)
{
    auto pass = [&](float c) {
        VcfRegs s = coeffs<true>(c, res);
        s.b0 = s.b1 = s.b2 = s.b3 = 1.0f;
        s.b4 = kVcfB4Bound;
        return vcf_b4_bounded_lane(s);
    };
    uint32_t lo = ord(0.3f), hi = ord(0.9f);
    if (!pass(unord(lo))) return 0.0f;
    if (pass(unord(hi))) return 0.9f;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        (pass(unord(mid)) ? lo : hi) = mid;
    }
    return unord(lo);
}

int main()
{
    std::mt19937 rng(20240530u);
    std::uniform_real_distribution<float> u01(0.0f, 1.0f), u11(-1.0f, 1.0f);
    const float Bt = next_down(kVcfB4Bound);
    const float res_list[] = {0.0f, 0.25f, 0.5f, 1.0f};
    float thr[4];
    std::vector<float> cutoffs = {0.0f, 0.05f, 0.6f, 0.89f, 0.9f};
    for (int r = 0; r < 4; r++) {
        thr[r] = threshold(res_list[r]);
        if (thr[r] > 0.0f && thr[r] < 0.9f)
            for (int k = -64; k <= 64; k++) cutoffs.push_back(unord(ord(thr[r]) + (uint32_t)k));
    }
    const size_t n_fixed = cutoffs.size();
    for (int i = 0; i < 1000000; i++) cutoffs.push_back(0.9f * u01(rng));

    Tally st;
    StepTally sp;
    long run_over = 0, runs = 0;
    double run_max = 0;
    for (size_t ci = 0; ci < cutoffs.size(); ci++) {
        const float c = cutoffs[ci];
        const bool fixed = ci < n_fixed;
        // near the threshold and at the named cutoffs: every resonance of the list; a random cutoff: one of them and a random one
        const int n_res = fixed ? 4 : 2;
        for (int r = 0; r < n_res; r++) {
            const float res = fixed ? res_list[r] : (r == 0 ? res_list[rng() & 3u] : u01(rng));
            const float b4s[] = {1.0f, -1.0f, kVcfB4Bound, -kVcfB4Bound, Bt, -Bt, u11(rng)};
            const float sums[] = {2.0f, -2.0f, 2.0f * u11(rng)};
            for (float b4 : b4s)
                for (float sum : sums) {
                    stage_point<true>(st, c, res, sum, b4);
                    stage_point<false>(st, c, res, sum, b4);
                }
            // whole steps: the corners of the state's box (all sixteen for a fixed cutoff, two random ones otherwise) and a point inside
            const int n_corner = fixed ? 16 : 2;
            for (int k = 0; k < n_corner; k++) {
                const uint32_t m = fixed ? (uint32_t)k : (rng() & 15u);
                for (float b4 : {kVcfB4Bound, -kVcfB4Bound, 1.0f, -1.0f}) {
                    const float b[5] = {m & 1u ? 1.0f : -1.0f, m & 2u ? 1.0f : -1.0f, m & 4u ? 1.0f : -1.0f, m & 8u ? 1.0f : -1.0f, b4};
                    for (float x : {1.0f, -1.0f}) {
                        step_point<true>(sp, c, res, b, x);
                        step_point<false>(sp, c, res, b, x);
                    }
                }
            }
            const float b[5] = {u11(rng), u11(rng), u11(rng), u11(rng), u11(rng)};
            step_point<true>(sp, c, res, b, u11(rng));
            step_point<false>(sp, c, res, b, u11(rng));
            if (fixed || (ci & 63u) == 0) {
                run_over += run_points<true>(rng, c, res, 256, run_max) + run_points<false>(rng, c, res, 256, run_max);
                runs += 2;
            }
        }
    }
    std::printf("{\"cutoffs\": %zu, \"thresholds\": [%.9g, %.9g, %.9g, %.9g], "
                "\"stage\": {\"n\": %ld, \"pass\": %ld, \"pass_over\": %ld, \"pass_max_g\": [%.9g, %.9g], \"pass_max_pre\": %.9g, \"fail_over_one\": %ld, \"fail_max_g\": [%.9g, %.9g]}, "
                "\"step\": {\"n\": %ld, \"pass\": %ld, \"pass_over\": %ld, \"pass_max_b4\": [%.9g, %.9g], \"fail_over_one\": %ld, \"fail_max_b4\": [%.9g, %.9g], "
                "\"stage_only_pass\": %ld, \"stage_only_over_one\": %ld, \"stage_only_max_b4\": %.9g}, "
                "\"runs\": {\"n\": %ld, \"over\": %ld, \"max_b4\": %.9g}, \"bound\": %.9g, \"pre_max\": %.9g}\n",
                cutoffs.size(), thr[0], thr[1], thr[2], thr[3], st.n, st.n_pass, st.pass_over, st.pass_max_g[0], st.pass_max_g[1], st.pass_max_pre, st.fail_over_one,
                st.fail_max_g[0], st.fail_max_g[1], sp.n, sp.n_pass, sp.pass_over, sp.pass_max_b4[0], sp.pass_max_b4[1], sp.fail_over_one, sp.fail_max_b4[0],
                sp.fail_max_b4[1], sp.stage_only_pass, sp.stage_only_over_one, sp.stage_only_max_b4, runs, run_over, run_max, (double)kVcfB4Bound, (double)kVcfB4PreMax);
    return 0;
}
