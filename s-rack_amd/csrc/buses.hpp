// buses.hpp — the mix table of a handle's voices (srack_voices_set_buses) and what the bus fold reads of it on the device.
//
// bus_mix[b][c][t] = sum over the voices of bus b of fl32(gain[v] * x[plane(c)][t][v]).  The fold (folds.hip.h: bus_fold_tiles,
// bus_fold_sum) streams a launch's frames once, 64 voices — one 256-byte piece of a frame row — per wave: a TILE.  Everything the
// kernels need to know about the table is prepared here, on the host, once per srack_voices_set_buses, by a pure function:
//   order    per tile, the lanes of its voices that are in a bus, sorted by bus (ties: ascending voice): the order they are added in
//   segments per tile, one per bus present in it: the run of `order` that belongs to the bus
//   partials a bus present in several tiles gets one row of scratch per segment, the rows of a bus consecutive and in ascending
//            tile order — the order bus_fold_sum adds them in; a bus present in ONE tile has no partial: its segment's sum is the
//            bus's sample and goes straight to the bus mix
// So the order of the f32 additions depends on the table and the voice count alone — not on how a render is cut.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace srack {

constexpr uint32_t kBusTile = 64;  // voices per tile

struct BusPlan {
    uint32_t n_voices = 0, n_buses = 0, n_tiles = 0, n_partials = 0;
    std::vector<uint32_t> order;      // [n_tiles * 64] lane of the tile's j-th voice in bus order (slots past the tile's last segment: unused, 0)
    std::vector<uint32_t> tile_seg;   // [n_tiles + 1] the tile's segments are [tile_seg[i], tile_seg[i + 1]), at most 64
    std::vector<uint32_t> seg_end;    // [segments] end of the segment in the tile's order (it starts where the one before it ends; the first at 0)
    std::vector<int32_t> seg_dst;     // [segments] >= 0: its row of the partials; < 0: ~bus — the bus's only segment, written to the bus mix
    std::vector<int32_t> seg_bus;     // [segments] (host side: diagnostics and tests)
    std::vector<uint32_t> bus_first;  // [n_buses] first partial row of the bus
    std::vector<int32_t> bus_count;   // [n_buses] its partial rows (0: an empty bus); -1: one segment, no partial
};

// bus: n_voices entries in [0, n_buses) or -1 (validated by the caller)
inline BusPlan bus_plan_make(uint32_t n_voices, uint32_t n_buses, const int32_t* bus)
{
    BusPlan P;
    P.n_voices = n_voices;
    P.n_buses = n_buses;
    P.n_tiles = (n_voices + kBusTile - 1) / kBusTile;
    P.order.assign((size_t)P.n_tiles * kBusTile, 0u);
    P.tile_seg.assign((size_t)P.n_tiles + 1, 0u);
    std::vector<uint32_t> segs_of_bus(n_buses, 0u);
    for (uint32_t i = 0; i < P.n_tiles; i++) {
        const uint32_t v0 = i * kBusTile, n = std::min(kBusTile, n_voices - v0);
        uint32_t lanes[kBusTile], m = 0;
        for (uint32_t l = 0; l < n; l++)
            if (bus[v0 + l] >= 0) lanes[m++] = l;
        std::stable_sort(lanes, lanes + m, [&](uint32_t a, uint32_t b) { return bus[v0 + a] < bus[v0 + b]; });
        for (uint32_t j = 0; j < m; j++) {
            P.order[(size_t)v0 + j] = lanes[j];
            if (j + 1 == m || bus[v0 + lanes[j + 1]] != bus[v0 + lanes[j]]) {
                P.seg_end.push_back(j + 1);
                P.seg_bus.push_back(bus[v0 + lanes[j]]);
                segs_of_bus[(size_t)bus[v0 + lanes[j]]]++;
            }
        }
        P.tile_seg[(size_t)i + 1] = (uint32_t)P.seg_end.size();
    }
    P.bus_first.assign(n_buses, 0u);
    P.bus_count.assign(n_buses, 0);
    uint32_t rows = 0;
    for (uint32_t b = 0; b < n_buses; b++) {
        P.bus_first[b] = rows;
        P.bus_count[b] = segs_of_bus[b] == 1 ? -1 : (int32_t)segs_of_bus[b];
        if (segs_of_bus[b] > 1) rows += segs_of_bus[b];
    }
    P.n_partials = rows;
    // segments are visited in ascending tile order, so a bus's rows come out in ascending tile order
    std::vector<uint32_t> next(P.bus_first);
    P.seg_dst.resize(P.seg_end.size());
    for (size_t s = 0; s < P.seg_end.size(); s++) {
        const int32_t b = P.seg_bus[s];
        P.seg_dst[s] = P.bus_count[(size_t)b] < 0 ? ~b : (int32_t)next[(size_t)b]++;
    }
    return P;
}

// A slot table (srack_voices_set_bus_slots): a voice feeds up to n_slots buses.  The plan is the one above over GROUPS instead of
// tiles: group tile * n_slots + k is slot k of the tile's 64 voices, laid out as 64 entries of a virtual voice array (the ragged
// tail in no bus), so `order` still holds lanes of the tile, a bus's rows ascend in (tile, slot) order, and n_slots == 1 gives the
// plan of the same table through srack_voices_set_buses (n_tiles counts groups; n_voices is the virtual array's length).
// bus: [n_voices][n_slots], entries in [0, n_buses) or -1 (validated by the caller)
inline BusPlan bus_slot_plan_make(uint32_t n_voices, uint32_t n_buses, uint32_t n_slots, const int32_t* bus)
{
    const uint32_t n_tiles = (n_voices + kBusTile - 1) / kBusTile;
    std::vector<int32_t> virt((size_t)n_tiles * n_slots * kBusTile, -1);
    for (uint32_t v = 0; v < n_voices; v++)
        for (uint32_t k = 0; k < n_slots; k++) virt[((size_t)(v / kBusTile) * n_slots + k) * kBusTile + v % kBusTile] = bus[(size_t)v * n_slots + k];
    return bus_plan_make((uint32_t)virt.size(), n_buses, virt.data());
}

}  // namespace srack
