// busvcf.hip.h — the bus filters (srack_buses_filter): a Moog ladder per (enabled bus, channel) row, behind the mixer.
//
// A row is one MoogFilterModule (filter.rs:182-221): audio in rows[bus][c][t], CV in cv[bus][t] (or 0.0f), the chosen port out.  The
// ladder is a non-linear recurrence, strictly serial in time: a lane is a row, and the kernel is the lane-per-row tile loop of
// bustile.hip.h, eight samples read ahead.  The arithmetic is modules.hip.h's literal ladder (vcf_frequency, vcf_resonance,
// vcf_coeffs<false>, vcf_run<false>; the unit is built with -ffp-contract=off): the reference's f32 operations one by one.
//
// Optional: the CV, a second tile of 64 / kUsed rows — the rows of the wave's buses, fetched and turned like the audio.  The results go
// into the audio tile, over the samples they were made from, and out the way the audio came in; in place (out == rows) is safe.  The
// state stays in registers across the tiles of a call and is loaded and stored once per call, from a layout in which a wave's 64 slots
// lie side by side per field.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "bustile.hip.h"
#include "launch_types.hpp"
#include "modules.hip.h"

namespace srack {

constexpr int kBusVcfAhead = 8;     // samples a lane reads from LDS at a time
constexpr int kBusVcfCopyThreads = 256;
static_assert(kBusVcfFields == SRACK_BUS_FILTER_NSTATE && sizeof(dev::VcfRegs) == sizeof(float) * kBusVcfFields, "the state is VcfRegs field by field, as the C ABI hands it out");

// grid (ceil(n_rows / 64)), block 64.  kCv: a.cv is given.  kUsed: a.used, 1 or 2 — the table entries that share a bus and a row of cv.
template <bool kCv, int kUsed>
__global__ __launch_bounds__(64) void bus_filter(const BusVcfArgs a)
{
    using namespace dev;
    constexpr int kCvRows = kRowTile / kUsed;
    __shared__ float s_x[kRowTileWords];
    __shared__ float s_cv[kCv ? kCvRows * kRowTileStride : 1];
    const uint32_t lane = threadIdx.x;
    const uint32_t r0 = blockIdx.x * 64u;
    const uint32_t live = min(64u, a.n_rows - r0);         // rows of this wave (wave-uniform)
    const bool on = lane < live;
    // A lane past the last row takes row 0's entry: it runs that filter on zeros and stores nothing, and — every lane holding a row that
    // exists — row j's place comes out of lane j's registers, past the last row another read of row 0.
    const BusVcfRow me = a.tab[r0 + (on ? lane : 0u)];
    const uint64_t my_x = (uint64_t)me.row * a.n, my_cv = (uint64_t)me.bus * a.n;   // in floats
    const uint32_t cv_at = (lane / kUsed) * kRowTileStride;
    const uint32_t x_at = lane * kRowTileStride;
    auto x_row = [&](int j) { return bustile_from_lane(my_x, j); };
    auto cv_row = [&](int j) { return bustile_from_lane(my_cv, j * kUsed); };

    float* st = a.state + (size_t)(me.slot >> 6) * (kBusVcfFields * 64) + (me.slot & 63u);
    VcfRegs s;
    s.f = st[0 * 64], s.p = st[1 * 64], s.q = st[2 * 64];
    s.b0 = st[3 * 64], s.b1 = st[4 * 64], s.b2 = st[5 * 64], s.b3 = st[6 * 64], s.b4 = st[7 * 64];
    s.freq = st[8 * 64], s.res = st[9 * 64];
    bool fin = vcf_nan_free(s);
    const float res = vcf_resonance(me.res);

    float pre[kRowTile];                     // the tile fetched ahead
    float cpre[kCv ? kCvRows : 1];
    auto fetch = [&](uint32_t t0) {
        const uint32_t tl = bustile_sample(lane, a.n, t0);
        bustile_fetch(pre, a.rows, t0, tl, x_row);
        if constexpr (kCv) bustile_fetch(cpre, a.cv, t0, tl, cv_row);
    };
    // eight samples of this lane's row (and of its bus's CV) out of the tile
    auto read8 = [&](uint32_t k0, float (&x)[kBusVcfAhead], float (&c)[kBusVcfAhead]) {
#pragma unroll
        for (int q = 0; q < kBusVcfAhead; q++) {
            x[q] = on ? s_x[x_at + k0 + q] : 0.0f;
            c[q] = 0.0f;
            if constexpr (kCv) c[q] = s_cv[cv_at + k0 + q];
        }
    };

    const uint32_t n_tiles = (a.n + kRowTile - 1) / kRowTile;
    fetch(0);
    for (uint32_t i = 0; i < n_tiles; i++) {
        const uint32_t t0 = i * kRowTile;
        const uint32_t len = min((uint32_t)kRowTile, a.n - t0);
        bustile_turn(s_x, pre, lane);
        if constexpr (kCv) {  // (its own loop: bustile_turn of 32 rows is unrolled before it is inlined, and bus_filter<true, 2> was other code)
#pragma unroll
            for (int j = 0; j < kCvRows; j++) s_cv[j * kRowTileStride + lane] = cpre[j];
        }
        __syncthreads();
        if (i + 1 < n_tiles) fetch(t0 + kRowTile);

        // the serial part
        auto run = [&](auto full) {
            constexpr bool kFull = decltype(full)::value;
            float x[kBusVcfAhead], c[kBusVcfAhead];
            read8(0, x, c);
            for (uint32_t k0 = 0; k0 < (kFull ? (uint32_t)kRowTile : len); k0 += kBusVcfAhead) {
                float xn[kBusVcfAhead], cn[kBusVcfAhead];
                read8(min(k0 + kBusVcfAhead, (uint32_t)(kRowTile - kBusVcfAhead)), xn, cn);
                float y[kBusVcfAhead];
#pragma unroll
                for (int q = 0; q < kBusVcfAhead; q++) {
                    y[q] = 0.0f;
                    if (kFull || k0 + q < len) {
                        float lp, bp, hp;
                        vcf_coeffs<false>(s, vcf_frequency(me.freq, c[q], me.exp_amt), res);
                        vcf_run<false>(s, fin, x[q], lp, bp, hp);
                        y[q] = me.port == SRACK_VCF_OUT_LOWPASS ? lp : me.port == SRACK_VCF_OUT_BANDPASS ? bp : hp;
                    }
                }
#pragma unroll
                for (int q = 0; q < kBusVcfAhead; q++) s_x[x_at + k0 + q] = y[q];
#pragma unroll
                for (int q = 0; q < kBusVcfAhead; q++) x[q] = xn[q], c[q] = cn[q];
            }
        };
        if (len == (uint32_t)kRowTile)
            run(std::true_type{});
        else
            run(std::false_type{});
        __syncthreads();
        bustile_store(a.out, s_x, t0, lane, len, live, x_row);
        __syncthreads();
    }

    if (on) {
        st[0 * 64] = s.f, st[1 * 64] = s.p, st[2 * 64] = s.q;
        st[3 * 64] = s.b0, st[4 * 64] = s.b1, st[5 * 64] = s.b2, st[6 * 64] = s.b3, st[7 * 64] = s.b4;
        st[8 * 64] = s.freq, st[9 * 64] = s.res;
    }
}

// The disabled buses' used channels, out of place: bit for bit (as words: -0.0 stays -0.0, a NaN keeps its payload).
// grid (ceil(n / 256), ceil(n_copy / gridDim.y rows each)): a block walks the rows y, y + gridDim.y, ...
__global__ __launch_bounds__(kBusVcfCopyThreads) void bus_filter_copy(const BusVcfArgs a)
{
    const size_t t = (size_t)blockIdx.x * kBusVcfCopyThreads + threadIdx.x;
    if (t >= a.n) return;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.rows);
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.out);
    for (uint32_t r = blockIdx.y; r < a.n_copy; r += gridDim.y) {
        const size_t at = (size_t)a.copy_rows[r] * a.n + t;
        dst[at] = src[at];
    }
}

}  // namespace srack
