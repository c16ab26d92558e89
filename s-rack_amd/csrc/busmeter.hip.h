// busmeter.hip.h — the bus meters (srack_buses_meter): windowed level tracks and totals per (bus, channel) row, a read-only tap on the bus rows.
//
// A row's six numbers are the per-voice statistics' (wave.hip.h: VoiceStats, stats_add, stats_load, stats_store — used as they stand,
// nothing of the definitions is restated here): SUM and SUM_SQ continue the sequential f64 loop from what the buffer holds, the peaks
// are read back as f32 and move only upwards, the counts are added.  The sums are serial in time per row, so the only parallelism is
// across rows: a lane is a row, and the kernel is the lane-per-row tile loop of bustile.hip.h, eight samples read ahead of the eight
// being added — a read-only tap: nothing goes back into the tile and nothing is stored to the rows.
//
// A lane keeps two sets of VoiceStats in registers: the open window's record and the totals.  Every row shares the stream position, so a
// window boundary is wave-uniform: a tile is walked in segments that end where the open window ends (or the tile does); at a boundary
// the wave stores the open record and — when the call has samples left — loads the next one to continue it.  The buffers are
// entity-minor, f64 [SRACK_STAT_COUNT][n_buses][2] per record: with two used channels a wave's 64 entities lie side by side, 512 bytes
// per field.  With one used channel the lanes are 16 bytes apart and the channel-1 entries are never touched.
//
// Indices: a sample index is t0 + min(lane, n - 1 - t0) < n; row j of a tile is r0 + min(j, live - 1) < n_rows = n_buses * used, so the bus is
// below n_buses and the channel below used; a lane at or past `live` loads and stores no record; the window index w starts at
// first / window and is raised only when a sample of the call lies in the next window, so w <= (first + n - 1) / window < n_windows
// (the host has checked first + n <= n_windows * window).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "bustile.hip.h"
#include "launch_types.hpp"
#include "wave.hip.h"

namespace srack {

constexpr int kBusMeterAhead = 8;    // samples a lane reads from LDS at a time
static_assert(SRACK_BUS_METER_MIN_WINDOW >= kRowTile, "a tile holds one window boundary at the most");
static_assert(kStatCount == SRACK_STAT_COUNT, "a record is VoiceStats field by field");

// grid (ceil(n_buses * kUsed / 64)), block 64.  kUsed: a.used, 1 or 2.  kLevels / kTotals: a.levels / a.totals is given.
template <int kUsed, bool kLevels, bool kTotals>
__global__ __launch_bounds__(64) void bus_meter(const BusMeterArgs a)
{
    __shared__ float s_x[kRowTileWords];
    const uint32_t lane = threadIdx.x;
    const uint32_t n_rows = a.n_buses * (uint32_t)kUsed;
    const uint32_t r0 = blockIdx.x * 64u;
    const uint32_t live = min(64u, n_rows - r0);  // rows of this wave (wave-uniform)
    const bool on = lane < live;
    const uint32_t x_at = lane * kRowTileStride;
    // this lane's entity: (bus, channel) of its row, in a frame of [n_buses][2]
    const uint32_t my_row = r0 + (on ? lane : 0u);
    const size_t ents = (size_t)a.n_buses * 2;
    const size_t ent = (size_t)(my_row / kUsed) * 2 + my_row % kUsed;
    constexpr size_t kRecord = (size_t)kStatCount;  // fields per record, `ents` doubles each

    VoiceStats win = {}, tot = {};
    uint64_t w = 0;          // the open window
    uint32_t left = ~0u;     // samples until it ends (no levels: never)
    bool open = false;       // its record is in registers
    if constexpr (kLevels) {
        w = a.first / a.window;
        left = a.window - (uint32_t)(a.first - w * a.window);
        if (on) stats_load(win, a.levels + (size_t)w * kRecord * ents + ent, ents);
        open = true;
    }
    if constexpr (kTotals) {
        if (on) stats_load(tot, a.totals + ent, ents);
    }

    float pre[kRowTile];  // the tile fetched ahead
    auto row = [&](int j) {  // (wave-uniform: the address is a scalar base and the lane's sample; past the last row the last row again)
        const uint32_t r = r0 + min((uint32_t)j, live - 1u);
        return ((size_t)(r / kUsed) * a.row_channels + r % kUsed) * a.n;
    };
    auto fetch = [&](uint32_t t0) { bustile_fetch(pre, a.rows, t0, bustile_sample(lane, a.n, t0), row); };
    // (a segment begins anywhere: every word is held to the tile, the last chunk reads its last word again)
    auto read8 = [&](uint32_t k0, float (&x)[kBusMeterAhead]) {
#pragma unroll
        for (int q = 0; q < kBusMeterAhead; q++) x[q] = s_x[x_at + min(k0 + q, (uint32_t)(kRowTile - 1))];
    };
    auto add = [&](float x) {
        if constexpr (kLevels) stats_add(win, x);
        if constexpr (kTotals) stats_add(tot, x);
    };
    // samples kb .. ke - 1 of the tile in LDS (kFull: the whole tile, no sample asks whether it belongs)
    auto run = [&](auto full, uint32_t kb, uint32_t ke) {
        constexpr bool kFull = decltype(full)::value;
        float x[kBusMeterAhead];
        read8(kFull ? 0u : kb, x);
        for (uint32_t k0 = kFull ? 0u : kb; k0 < (kFull ? (uint32_t)kRowTile : ke); k0 += kBusMeterAhead) {
            float xn[kBusMeterAhead];
            read8(k0 + kBusMeterAhead, xn);
#pragma unroll
            for (int q = 0; q < kBusMeterAhead; q++)
                if (kFull || k0 + q < ke) add(x[q]);
#pragma unroll
            for (int q = 0; q < kBusMeterAhead; q++) x[q] = xn[q];
        }
    };

    const uint32_t n_tiles = (a.n + kRowTile - 1) / kRowTile;
    fetch(0);
    for (uint32_t i = 0; i < n_tiles; i++) {
        const uint32_t t0 = i * kRowTile;
        const uint32_t len = min((uint32_t)kRowTile, a.n - t0);
        bustile_turn(s_x, pre, lane);
        __syncthreads();
        if (i + 1 < n_tiles) fetch(t0 + kRowTile);

        uint32_t k = 0;
        while (k < len) {  // (wave-uniform: segments that end with the open window or with the tile)
            const uint32_t m = min(len - k, left);
            if (m == (uint32_t)kRowTile)
                run(std::true_type{}, 0u, (uint32_t)kRowTile);
            else
                run(std::false_type{}, k, k + m);
            k += m;
            if constexpr (kLevels) {
                left -= m;
                if (left == 0) {
                    if (on) stats_store(win, a.levels + (size_t)w * kRecord * ents + ent, ents);
                    open = false;
                    left = a.window;
                    if (t0 + k < a.n) {  // a sample of this call lies in the next window: w + 1 <= (first + n - 1) / window
                        w++;
                        if (on) stats_load(win, a.levels + (size_t)w * kRecord * ents + ent, ents);
                        open = true;
                    }
                }
            }
        }
        __syncthreads();
    }

    if constexpr (kLevels) {
        if (open && on) stats_store(win, a.levels + (size_t)w * kRecord * ents + ent, ents);
    }
    if constexpr (kTotals) {
        if (on) stats_store(tot, a.totals + ent, ents);
    }
}

}  // namespace srack
