// busosc.hip.h — the bus oscillators (srack_buses_osc): an LFO per enabled mix bus writes a control row of the console.
//
// A row is three reference modules in series, ticked once per sample: OscillatorModule (oscillator.rs:108-157; CV in cv[bus][t], Sync in
// sync[bus][t], either may be absent), MathModule(Multiply) by DEPTH and MathModule(Add) of OFFSET (math.rs:150-155) -> out[bus][t].
// The oscillator is modules.hip.h's osc_step with OSC_EXACT, as it stands: the f64 phase, the f64 PolyBLEP, the host libm's pow and sin with
// their cold arms.  The two Math operations are f32, one rounding each (the unit is built with -ffp-contract=off).
//
// The phase is a serial recurrence: a lane is a bus, and the kernel is the lane-per-row tile loop of bustile.hip.h with the buses' rows of
// cv, sync and out as the rows.  Four samples are read ahead of the four being computed — the outputs of different samples depend on each
// other through the phase alone, so four steps side by side are four sines in flight.  Optional: the CV tile and the sync tile; the results
// go into the first tile, over the values they were made from, and that tile is stored.  A call with neither CV nor sync has one tile,
// for the results, and reads nothing from memory but its table and state.  The state (pos as f64, last as 0.0 / 1.0 in f64) stays in
// registers for the call and is indexed by bus.
//
// osc_step guards its cold arms with wave ballots and takes wave-uniform flags; port and antialiasing belong to a bus.  The host orders the
// table by (port, antialiasing), so all but a few waves have one class; every wave ORs its lanes' ports into the flags, every lane picks
// its own port, and a wave that holds both antialiasing settings steps a copy of the state a second time with the other one.  All of
// osc_step's outputs are functions of (pos, delta) alone, so no bit depends on which wave a bus landed in.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "bustile.hip.h"
#include "launch_types.hpp"
#include "modules.hip.h"

namespace srack {

constexpr int kBusOscAhead = 4;     // samples a lane reads from LDS at a time, and steps side by side
constexpr int kBusOscZeroThreads = 256;
constexpr uint32_t kBusOscPorts = OSC_OUT_SINE | OSC_OUT_SQUARE | OSC_OUT_SAW;
static_assert(kBusOscFields == SRACK_BUS_OSC_NSTATE, "the state is (pos, last) per bus, as the C ABI hands it out");
static_assert(kRowTile % kBusOscAhead == 0, "a tile is a whole number of chunks");

// The same sample with the other antialiasing setting, for a wave that holds both: square and saw from a copy of the state.  Out of line —
// the table's order keeps such waves to the class boundaries, and inlined it doubled every step of every wave's loop.
__device__ __attribute__((noinline)) void busosc_other_aa(uint32_t flags, dev::OscRegs s, dev::OscConst k, float cv, float sync, float& square, float& saw)
{
    float none = 0.0f;
    dev::osc_step(flags | OSC_EXACT, s, k, cv, sync, none, square, saw);
}

// grid (ceil(n_on / 64)), block 64.  kCv: a.cv is given.  kSync: a.sync is given.
template <bool kCv, bool kSync>
__global__ __launch_bounds__(64) void bus_osc(const BusOscArgs a)
{
    using namespace dev;
    constexpr int kTiles = (kCv ? 1 : 0) + (kSync ? 1 : 0) > 0 ? (kCv ? 1 : 0) + (kSync ? 1 : 0) : 1;
    __shared__ float s_t[kTiles * kRowTileWords];
    float* const s_cv = s_t;                                  // (kCv)
    float* const s_sync = s_t + (kCv ? kRowTileWords : 0);    // (kSync)
    float* const s_y = s_t;                                   // the results: over the first tile
    const uint32_t lane = threadIdx.x;
    const uint32_t r0 = blockIdx.x * 64u;
    const uint32_t live = min(64u, a.n_on - r0);              // buses of this wave (wave-uniform)
    const bool on = lane < live;
    // A lane past the last bus takes the wave's first entry: it runs that oscillator and stores nothing, and — every lane holding a bus
    // that exists — row j's place comes out of lane j's registers.
    const BusOscBus me = a.tab[r0 + (on ? lane : 0u)];
    const uint64_t my_row = (uint64_t)me.bus * a.n;           // in floats: the bus's row of cv, sync and out
    const uint32_t at = lane * kRowTileStride;
    auto row = [&](int j) { return bustile_from_lane(my_row, j); };

    OscRegs s;
    s.pos = a.state[me.bus];
    s.sync_last = a.state[(size_t)a.n_buses + me.bus] != 0.0;
    OscConst k;
    k.delta = me.delta;
    k.val = me.val;
    k.sr = a.sr;
    k.inv_dt = 0.0f;

    // The wave's flags: every port some lane wants, the first lane's antialiasing; a second pass with the other setting where both occur.
    const bool my_aa = (me.flags & OSC_AA) != 0;
    uint32_t wf = OSC_EXACT | (kCv ? OSC_HAS_CV : 0u) | (kSync ? OSC_HAS_SYNC : 0u);
    if (__builtin_amdgcn_ballot_w64((me.flags & OSC_OUT_SINE) != 0) != 0) wf |= OSC_OUT_SINE;
    if (__builtin_amdgcn_ballot_w64((me.flags & OSC_OUT_SQUARE) != 0) != 0) wf |= OSC_OUT_SQUARE;
    if (__builtin_amdgcn_ballot_w64((me.flags & OSC_OUT_SAW) != 0) != 0) wf |= OSC_OUT_SAW;
    const uint64_t aa_lanes = __builtin_amdgcn_ballot_w64(my_aa);
    const bool first_aa = (aa_lanes & 1u) != 0;
    if (first_aa) wf |= OSC_AA;
    const uint32_t n_pass = (aa_lanes != 0 && ~aa_lanes != 0) ? 2u : 1u;
    const bool mine_first = my_aa == first_aa;

    // One sample of this lane's bus: the oscillator's port, times DEPTH, plus OFFSET.  (Inlined by force: bustile.hip.h.)
    auto step = [&](float cv, float sync) __attribute__((always_inline)) -> float {
        float sine = 0.0f, square = 0.0f, saw = 0.0f;
        const OscRegs before = s;
        osc_step(wf, s, k, cv, sync, sine, square, saw);
        if (n_pass == 2u) {  // (wave-uniform.  The sine knows no antialiasing; phase and held-CV cache come out the same: discarded)
            float square2 = 0.0f, saw2 = 0.0f;
            busosc_other_aa((wf ^ OSC_AA) & ~(uint32_t)OSC_OUT_SINE, before, k, cv, sync, square2, saw2);
            if (!mine_first) square = square2, saw = saw2;
        }
        const float y = (me.flags & OSC_OUT_SINE) ? sine : (me.flags & OSC_OUT_SQUARE) ? square : saw;
        const float scaled = y * me.depth;   // MathModule(Multiply): a * constant
        return scaled + me.offset;           // MathModule(Add): a + constant
    };

    float pre[kCv ? kRowTile : 1];           // the tiles fetched ahead
    float spre[kSync ? kRowTile : 1];
    auto fetch = [&](uint32_t t0) {
        const uint32_t tl = bustile_sample(lane, a.n, t0);
        if constexpr (kCv) bustile_fetch(pre, a.cv, t0, tl, row);
        if constexpr (kSync) bustile_fetch(spre, a.sync, t0, tl, row);
    };
    auto read_ahead = [&](uint32_t k0, float (&c)[kBusOscAhead], float (&g)[kBusOscAhead]) {
#pragma unroll
        for (int q = 0; q < kBusOscAhead; q++) {
            c[q] = 0.0f, g[q] = 0.0f;
            if constexpr (kCv) c[q] = s_cv[at + k0 + q];
            if constexpr (kSync) g[q] = s_sync[at + k0 + q];
        }
    };

    const uint32_t n_tiles = (a.n + kRowTile - 1) / kRowTile;
    if constexpr (kCv || kSync) fetch(0);
    for (uint32_t i = 0; i < n_tiles; i++) {
        const uint32_t t0 = i * kRowTile;
        const uint32_t len = min((uint32_t)kRowTile, a.n - t0);
        if constexpr (kCv) bustile_turn(s_cv, pre, lane);
        if constexpr (kSync) bustile_turn(s_sync, spre, lane);
        if constexpr (kCv || kSync) {
            __syncthreads();
            if (i + 1 < n_tiles) fetch(t0 + kRowTile);
        }

        // the serial part.  A sample past the end is not stepped: the state after the call is the state after its last sample.
        auto run = [&](auto full) {
            constexpr bool kFull = decltype(full)::value;
            float c[kBusOscAhead], g[kBusOscAhead];
            read_ahead(0, c, g);
            for (uint32_t k0 = 0; k0 < (kFull ? (uint32_t)kRowTile : len); k0 += kBusOscAhead) {
                float cn[kBusOscAhead], gn[kBusOscAhead];
                read_ahead(min(k0 + kBusOscAhead, (uint32_t)(kRowTile - kBusOscAhead)), cn, gn);
                float y[kBusOscAhead];
#pragma unroll
                for (int q = 0; q < kBusOscAhead; q++) {
                    y[q] = 0.0f;
                    if (kFull || k0 + q < len) y[q] = step(c[q], g[q]);   // (wave-uniform: every lane is in every step)
                }
#pragma unroll
                for (int q = 0; q < kBusOscAhead; q++) s_y[at + k0 + q] = y[q];
#pragma unroll
                for (int q = 0; q < kBusOscAhead; q++) c[q] = cn[q], g[q] = gn[q];
            }
        };
        if (len == (uint32_t)kRowTile)
            run(std::true_type{});
        else
            run(std::false_type{});
        __syncthreads();
        bustile_store(a.out, s_y, t0, lane, len, live, row);
        __syncthreads();
    }

    if (on) {
        a.state[me.bus] = s.pos;
        a.state[(size_t)a.n_buses + me.bus] = s.sync_last ? 1.0 : 0.0;
    }
}

// The disabled buses' rows: +0.0f, the convention of srack_buses_vca's d_env.
// grid (ceil(n / 256), up to 65535 rows side by side): a block walks the rows y, y + gridDim.y, ...
__global__ __launch_bounds__(kBusOscZeroThreads) void bus_osc_zero(const BusOscArgs a)
{
    const size_t t = (size_t)blockIdx.x * kBusOscZeroThreads + threadIdx.x;
    if (t >= a.n) return;
    for (uint32_t r = blockIdx.y; r < a.n_off; r += gridDim.y) a.out[(size_t)a.off[r] * a.n + t] = 0.0f;
}

}  // namespace srack
