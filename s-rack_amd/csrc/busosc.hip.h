// busosc.hip.h — the bus oscillators (srack_buses_osc): an LFO per enabled mix bus writes a control row of the console.
//
// A row is three reference modules in series, ticked once per sample: OscillatorModule (oscillator.rs:108-157; CV in cv[bus][t], Sync in
// sync[bus][t], either may be absent), MathModule(Multiply) by DEPTH and MathModule(Add) of OFFSET (math.rs:150-155) -> out[bus][t].
// The oscillator is modules.hip.h's osc_step with OSC_EXACT, as it stands: the f64 phase, the f64 PolyBLEP, the host libm's pow and sin with
// their cold arms.  The two Math operations are f32, one rounding each (the unit is built with -ffp-contract=off).
//
// The phase is a serial recurrence, so the parallelism is across buses, in bus_filter's shape (busvcf.hip.h): a lane is a bus, a wave 64
// buses, a workgroup one wave — the few waves of a small console land on different CUs.  The CV and sync rows are time-minor in memory, the
// lanes want them bus-minor: tiles of 64 buses x 64 samples pass through LDS with a stride of 65 words.
//   load    row j of the tile as one 256-byte piece, lane l on sample t0 + l.  Tile i + 1's loads are issued before tile i's serial loop
//           and wait in registers.
//   run     lane l reads row l, sample k: LDS word l * 65 + k.  Four samples are read ahead of the four being computed — the outputs of
//           different samples depend on each other through the phase alone, so four steps side by side are four sines in flight.  The
//           results go into the first tile, over the values they were made from.
//   store   that tile, row by row.
// A call with neither CV nor sync has one tile, for the results, and reads nothing from memory but its table and state.
// Tails — a last tile of fewer than 64 samples, a last wave of fewer than 64 buses — are masked, never padded in memory; rows need no
// alignment beyond 4 bytes.  The state (pos as f64, last as 0.0 / 1.0 in f64) stays in registers for the call and is indexed by bus.
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

#include "launch_types.hpp"
#include "modules.hip.h"

namespace srack {

constexpr int kBusOscTile = 64;     // samples per tile (and buses per wave)
constexpr int kBusOscStride = 65;   // LDS words per tile row: odd, so that a column of 32 rows is 32 banks
constexpr int kBusOscAhead = 4;     // samples a lane reads from LDS at a time, and steps side by side
constexpr int kBusOscZeroThreads = 256;
constexpr uint32_t kBusOscPorts = OSC_OUT_SINE | OSC_OUT_SQUARE | OSC_OUT_SAW;
static_assert(kBusOscFields == SRACK_BUS_OSC_NSTATE, "the state is (pos, last) per bus, as the C ABI hands it out");
static_assert(kBusOscTile % kBusOscAhead == 0, "a tile is a whole number of chunks");

// A 64-bit value of lane `l` (wave-uniform), as a scalar: two v_readlane_b32, no memory access.
__device__ __forceinline__ uint64_t busosc_from_lane(uint64_t v, uint32_t l)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
    return ((uint64_t)hi << 32) | lo;
}

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
    constexpr int kTileWords = kBusOscTile * kBusOscStride;
    __shared__ float s_t[kTiles * kTileWords];
    float* const s_cv = s_t;                                  // (kCv)
    float* const s_sync = s_t + (kCv ? kTileWords : 0);       // (kSync)
    float* const s_y = s_t;                                   // the results: over the first tile
    const uint32_t lane = threadIdx.x;
    const uint32_t r0 = blockIdx.x * 64u;
    const uint32_t live = min(64u, a.n_on - r0);              // buses of this wave (wave-uniform)
    const bool on = lane < live;
    // A lane past the last bus takes the wave's first entry: it runs that oscillator and stores nothing, and — every lane holding a bus
    // that exists — the tile's loads need no test of the row.
    const BusOscBus me = a.tab[r0 + (on ? lane : 0u)];
    const uint64_t my_row = (uint64_t)me.bus * a.n;           // in floats: the bus's row of cv, sync and out
    const uint32_t at = lane * kBusOscStride;

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

    // One sample of this lane's bus: the oscillator's port, times DEPTH, plus OFFSET.  (Inlined by force: out of line the state went
    // through scratch memory on every sample, and the four steps of a chunk one behind the other.)
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

    float pre[kCv ? kBusOscTile : 1];        // the tile loaded ahead: row j, sample t0 + lane
    float spre[kSync ? kBusOscTile : 1];
    // (a lane past the end of the rows reads the last sample again: the loads back to back, none of them under a mask)
    auto fetch = [&](uint32_t t0) {
        const uint32_t tl = min(lane, a.n - 1u - t0);
        if constexpr (kCv) {
#pragma unroll
            for (int j = 0; j < kBusOscTile; j++) pre[j] = (a.cv + busosc_from_lane(my_row, j) + t0)[tl];
        }
        if constexpr (kSync) {
#pragma unroll
            for (int j = 0; j < kBusOscTile; j++) spre[j] = (a.sync + busosc_from_lane(my_row, j) + t0)[tl];
        }
    };
    auto read_ahead = [&](uint32_t k0, float (&c)[kBusOscAhead], float (&g)[kBusOscAhead]) {
#pragma unroll
        for (int q = 0; q < kBusOscAhead; q++) {
            c[q] = 0.0f, g[q] = 0.0f;
            if constexpr (kCv) c[q] = s_cv[at + k0 + q];
            if constexpr (kSync) g[q] = s_sync[at + k0 + q];
        }
    };

    const uint32_t n_tiles = (a.n + kBusOscTile - 1) / kBusOscTile;
    if constexpr (kCv || kSync) fetch(0);
    for (uint32_t i = 0; i < n_tiles; i++) {
        const uint32_t t0 = i * kBusOscTile;
        const uint32_t len = min((uint32_t)kBusOscTile, a.n - t0);
        if constexpr (kCv) {
#pragma unroll
            for (int j = 0; j < kBusOscTile; j++) s_cv[j * kBusOscStride + lane] = pre[j];
        }
        if constexpr (kSync) {
#pragma unroll
            for (int j = 0; j < kBusOscTile; j++) s_sync[j * kBusOscStride + lane] = spre[j];
        }
        if constexpr (kCv || kSync) {
            __syncthreads();
            if (i + 1 < n_tiles) fetch(t0 + kBusOscTile);
        }

        // the serial part (kFull: a whole tile, no sample asks whether it exists).  A sample past the end is not stepped: the state
        // after the call is the state after its last sample.
        auto run = [&](auto full) {
            constexpr bool kFull = decltype(full)::value;
            float c[kBusOscAhead], g[kBusOscAhead];
            read_ahead(0, c, g);
            for (uint32_t k0 = 0; k0 < (kFull ? (uint32_t)kBusOscTile : len); k0 += kBusOscAhead) {
                float cn[kBusOscAhead], gn[kBusOscAhead];
                read_ahead(min(k0 + kBusOscAhead, (uint32_t)(kBusOscTile - kBusOscAhead)), cn, gn);  // (the last chunk reads itself again: no branch)
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
        if (len == (uint32_t)kBusOscTile)
            run(std::true_type{});
        else
            run(std::false_type{});
        __syncthreads();
        if (lane < len) {
#pragma unroll
            for (int j = 0; j < kBusOscTile; j++)
                if ((uint32_t)j < live) (a.out + busosc_from_lane(my_row, j) + t0)[lane] = s_y[j * kBusOscStride + lane];
        }
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
