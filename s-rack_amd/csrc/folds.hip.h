// folds.hip.h — the passes over what the voice kernels wrote:
//   mix_reduce_groups/final   deterministic sum of the per-wave mix partials (no atomics)
//   stats_fold                per-voice statistics of a launch's frames
//   bus_fold_tiles/sum        weighted, grouped mix-down of a launch's frames (mix buses)
//   bus_slot_fold_tiles/sum   the same with up to four buses per voice and a gain per channel (voice bus slots)
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "kernel_args.hip.h"
#include "modules.hip.h"
#include "wave.hip.h"

namespace srack {

// ---- mix-down, passes 2 and 3: mix[c][i] = sum over waves of mixpart[plane(c)][w][i] ---------------------------
// Deterministic (fixed order, no atomics).  Pass 2 splits the waves into kMixSplit groups so that enough loads
// are in flight to stream the partials at HBM rate: block (x, y) sums group y for 256 consecutive samples into
// mixgroup[plane][y][i].  Pass 3 adds the kMixSplit group sums and fans planes out to channels.
constexpr uint32_t kMixSplit = 16;

struct MixArgs {
    const float* mixpart;   // [planes][n_waves][T]
    float* mixgroup;        // [planes][kMixSplit][T]
    float* mix;             // [channels][mix_stride], T samples of it
    uint32_t T, n_waves, n_channels, n_planes;
    uint32_t mix_stride;    // samples between channels of `mix` (the whole render's length; T is one segment of it)
    uint32_t t_begin, t_end;  // mix_reduce_groups: the samples of the segment this launch sums (a chunk)
    int32_t channel_plane[8];
};

__global__ __launch_bounds__(256) void mix_reduce_groups(MixArgs m)
{
    const uint32_t i = m.t_begin + blockIdx.x * 256u + threadIdx.x;  // samples [t_begin, t_end) of the segment: one chunk's, or all
    if (i >= m.t_end) return;
    const uint32_t per = (m.n_waves + kMixSplit - 1) / kMixSplit;
    const uint32_t w0 = blockIdx.y * per, w1 = min(m.n_waves, w0 + per);
    for (uint32_t plane = 0; plane < m.n_planes; plane++) {
        const float* p = m.mixpart + (size_t)plane * m.n_waves * m.T + i;
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // fixed 8-way split: deterministic, 8 loads in flight per thread
        uint32_t w = w0;
        for (; w + 8 <= w1; w += 8) {
#pragma unroll
            for (int k = 0; k < 8; k++) s[k] += p[(size_t)(w + k) * m.T];
        }
        for (; w < w1; w++) s[0] += p[(size_t)w * m.T];
        m.mixgroup[((size_t)plane * kMixSplit + blockIdx.y) * m.T + i] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    }
}

__global__ __launch_bounds__(256) void mix_reduce_final(MixArgs m)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m.t_end) return;  // (m.T is the row pitch of the partials, not the segment's length)
    for (uint32_t c = 0; c < m.n_channels; c++) {
        const int plane = m.channel_plane[c];
        float s = 0.0f;
        if (plane >= 0)
            for (uint32_t y = 0; y < kMixSplit; y++) s += m.mixgroup[((size_t)plane * kMixSplit + y) * m.T + i];
        m.mix[(size_t)c * m.mix_stride + i] = s;
    }
}

// Per-voice statistics of a launch's frames, for the kernels that do not carry the accumulators themselves (everything but
// render_voice_chain / render_voice_chain_track): one thread per (voice, plane) walks the launch's T rows in sample order — the
// sequential loop, so its sums are bit for bit what the in-kernel accumulators give, time-parallel kernels included.  A wave reads 256
// contiguous bytes of a row per sample.  frames: the launch's first row; plane_stride as in KernelArgs.
__global__ __launch_bounds__(256) void stats_fold(const float* __restrict__ frames, uint64_t plane_stride, uint32_t V, uint32_t T, double* stats)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x, plane = blockIdx.y;
    if (v >= V) return;
    double* s = stats + (size_t)plane * kStatCount * V + v;
    const float* f = frames + (size_t)plane * plane_stride + v;
    VoiceStats st;
    stats_load(st, s, V);
    for (uint32_t t = 0; t < T; t++) stats_add(st, f[(size_t)t * V]);
    stats_store(st, s, V);
}

// ---- mix buses: bus_mix[b][c][t] = sum over the voices v of bus b of fl32(gain[v] * x[plane(c)][t][v]) -------------------------
// A fold over a launch's frames like stats_fold, but nothing here is ordered in time, so it is a streaming reduction in two
// deterministic passes (no atomics).  The table side — who is in which bus, in which order things are added — is prepared on the
// host (buses.hpp) and only read here.
//
// Pass 1, bus_fold_tiles: one wave per (tile of 64 voices, slab of 64 rows, plane).  Lane l reads voice l of the tile row after row —
// 256 contiguous bytes per wave and row, each frame read exactly once, whatever the table looks like —, multiplies by the voice's
// gain and puts the product into row r, column l of an LDS tile.  Then lane r sums ROW r, one bus segment after the other, in the
// tile's bus order (`order`, held one entry per lane and handed round with v_readlane: wave-uniform, no memory access in the loop).
// LDS banks (ds_write_b32 / ds_read_b32: bank = dword address mod 32, conflicts within a 32-lane half): the write of row r puts lanes
// 0 .. 31 on 32 consecutive dwords; the read of column c by lanes r = 0 .. 31 hits dwords 65 r + c, banks (r + c) mod 32 — all
// different for ANY c, so no table can produce a conflict.  A segment's sums (64 consecutive samples, one per lane) leave as one
// 256-byte store: to the segment's row of the partials, or — the bus has no other segment — straight to the bus mix.
// Pass 2, bus_fold_sum: one thread per (bus, sample) adds the bus's partial rows in ascending row (= tile) order and fans planes out
// to channels; an empty bus and an unconnected channel are 0.
constexpr int kBusRows = 64;    // rows of a slab (one per lane in the summing phase)
constexpr int kBusPitch = 65;   // dwords per LDS row

struct BusFoldArgs {
    const float* frames;     // the slab's first row of plane 0: [planes][rows][V], planes plane_stride apart
    uint64_t plane_stride;
    uint32_t V, T;           // voices; rows of this slab
    const float* gain;       // [V]
    const uint32_t* order;   // [tiles * 64]
    const uint32_t* tile_seg;  // [tiles + 1]
    const uint32_t* seg_end;
    const int32_t* seg_dst;
    const uint32_t* bus_first;
    const int32_t* bus_count;
    float* part;             // [planes][n_partials][part_pitch]
    uint32_t n_partials, part_pitch;
    uint32_t n_buses, n_planes, n_channels;
    float* out;              // the bus mix at the slab's first sample: [n_buses][channels][out_stride]
    uint32_t out_stride;
    int32_t channel_plane[8];
};

__global__ __launch_bounds__(64) void bus_fold_tiles(BusFoldArgs a)
{
    __shared__ float tile[kBusRows * kBusPitch];
    const int lane = (int)threadIdx.x;
    const uint32_t ti = blockIdx.x, t0 = blockIdx.y * (uint32_t)kBusRows, plane = blockIdx.z;
    const uint32_t n = min((uint32_t)kBusRows, a.T - t0);
    const uint32_t v = min(ti * 64u + (uint32_t)lane, a.V - 1u);  // (lanes past the last voice read it again; `order` never names them)
    const uint32_t s0 = a.tile_seg[ti], n_seg = a.tile_seg[ti + 1] - s0;
    if (n_seg == 0) return;  // no voice of this tile is in a bus
    const float g = a.gain[v];
    const int ord = (int)a.order[(size_t)ti * 64u + (uint32_t)lane];
    const int my_end = (uint32_t)lane < n_seg ? (int)a.seg_end[s0 + (uint32_t)lane] : 0;
    const int my_dst = (uint32_t)lane < n_seg ? a.seg_dst[s0 + (uint32_t)lane] : 0;
    const float* f = a.frames + (size_t)plane * a.plane_stride + (size_t)t0 * a.V + v;
    if (n == (uint32_t)kBusRows) {
#pragma unroll 16
        for (int r = 0; r < kBusRows; r++) tile[r * kBusPitch + lane] = __fmul_rn(g, f[(size_t)r * a.V]);
    } else {
        for (uint32_t r = 0; r < n; r++) tile[r * kBusPitch + lane] = __fmul_rn(g, f[(size_t)r * a.V]);
    }
    __syncthreads();  // (one wave: orders the LDS writes before the reads)
    if ((uint32_t)lane >= n) return;
    const float* row = tile + lane * kBusPitch;
    int j = 0;
    for (uint32_t s = 0; s < n_seg; s++) {
        const int end = __builtin_amdgcn_readlane(my_end, (int)s), dst = __builtin_amdgcn_readlane(my_dst, (int)s);
        float sum = row[__builtin_amdgcn_readlane(ord, j)];
        j++;
        for (; j + 4 <= end; j += 4) {  // four reads in flight; the additions stay in order
            const float x0 = row[__builtin_amdgcn_readlane(ord, j)], x1 = row[__builtin_amdgcn_readlane(ord, j + 1)];
            const float x2 = row[__builtin_amdgcn_readlane(ord, j + 2)], x3 = row[__builtin_amdgcn_readlane(ord, j + 3)];
            sum = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(sum, x0), x1), x2), x3);
        }
        for (; j < end; j++) sum = __fadd_rn(sum, row[__builtin_amdgcn_readlane(ord, j)]);
        if (dst >= 0) {
            a.part[((size_t)plane * a.n_partials + (uint32_t)dst) * a.part_pitch + t0 + (uint32_t)lane] = sum;
        } else {
            float* o = a.out + (size_t)(uint32_t)~dst * a.n_channels * a.out_stride + t0 + (uint32_t)lane;
            for (uint32_t c = 0; c < a.n_channels; c++)
                if (a.channel_plane[c] == (int)plane) o[(size_t)c * a.out_stride] = sum;
        }
    }
}

__global__ __launch_bounds__(256) void bus_fold_sum(BusFoldArgs a)
{
    const uint32_t n_tb = (a.T + 255u) / 256u;
    const uint32_t b = blockIdx.x / n_tb, t = (blockIdx.x % n_tb) * 256u + threadIdx.x;
    if (t >= a.T) return;
    const int cnt = a.bus_count[b];
    const uint32_t first = a.bus_first[b];
    float* o = a.out + (size_t)b * a.n_channels * a.out_stride + t;
    for (uint32_t plane = 0; plane < a.n_planes; plane++) {
        if (cnt < 0) break;  // its one segment went straight to the bus mix
        float s = 0.0f;
        if (cnt > 0) {
            const float* p = a.part + ((size_t)plane * a.n_partials + first) * a.part_pitch + t;
            s = p[0];
#pragma unroll 8
            for (int k = 1; k < cnt; k++) s = __fadd_rn(s, p[(size_t)k * a.part_pitch]);
        }
        for (uint32_t c = 0; c < a.n_channels; c++)
            if (a.channel_plane[c] == (int)plane) o[(size_t)c * a.out_stride] = s;
    }
    for (uint32_t c = 0; c < a.n_channels; c++)
        if (a.channel_plane[c] < 0) o[(size_t)c * a.out_stride] = 0.0f;
}

// ---- voice bus slots: bus_mix[b][c][t] = sum over the (v, k) with bus[v][k] == b of fl32(gain[v][k][c] * x[plane(c)][t][v]) ------------
// The same two passes over a plan of GROUPS (tile, slot) instead of tiles (buses.hpp: bus_slot_plan_make), with a gain per slot and
// channel.
//
// Pass 1, bus_slot_fold_tiles: one wave per (tile of 64 voices, slab of 64 rows, plane), as bus_fold_tiles.  The wave loads its 64
// rows ONCE, into 64 registers per lane (64 loads of 256 bytes in flight) — each frame is read from global memory once per wave,
// whatever the number of slots and channels: that is what a slot costs less than a plane.  Then, for every slot of the tile that has
// a segment and every channel mapped to this plane, it (1) writes fl32(gain * row) into the one LDS tile, (2) sums row-wise, segment
// by segment, in the group's order handed round by v_readlane, (3) stores each segment's 64 sums as one 256-byte store, to the
// segment's partial row OF THAT CHANNEL or straight to out[bus][channel].  A barrier separates the uses of the tile.  The LDS tile
// has the pitch of bus_fold_tiles (65 dwords) and is written and read in the same pattern, so the bank argument in that kernel's
// header carries over unchanged: no table can produce a conflict.
// Pass 2, bus_slot_fold_sum: one thread per (bus, channel, sample) adds the bus's partial rows of the channel in ascending row
// (= (tile, slot)) order; an empty bus and an unconnected channel are +0.
struct BusSlotFoldArgs : BusFoldArgs {  // gain: [n_slots][n_channels][V]; part: [n_channels][n_partials][part_pitch]; tile_seg per GROUP
    uint32_t n_slots;
};

__global__ __launch_bounds__(64) void bus_slot_fold_tiles(BusSlotFoldArgs a)
{
    __shared__ float tile[kBusRows * kBusPitch];
    const int lane = (int)threadIdx.x;
    const uint32_t ti = blockIdx.x, t0 = blockIdx.y * (uint32_t)kBusRows, plane = blockIdx.z;
    const uint32_t K = a.n_slots, g0 = ti * K;
    if (a.tile_seg[g0] == a.tile_seg[g0 + K]) return;  // no voice of this tile is in a bus, in any slot
    const uint32_t n = min((uint32_t)kBusRows, a.T - t0);
    const uint32_t v = min(ti * 64u + (uint32_t)lane, a.V - 1u);  // (lanes past the last voice read it again; `order` never names them)
    const float* f = a.frames + (size_t)plane * a.plane_stride + (size_t)t0 * a.V + v;
    float x[kBusRows];  // the wave's frames: loaded here, once, and only multiplied below
    if (n == (uint32_t)kBusRows) {
#pragma unroll
        for (int r = 0; r < kBusRows; r++) x[r] = f[(size_t)r * a.V];
    } else {  // a ragged last slab: only the rows that exist
#pragma unroll
        for (int r = 0; r < kBusRows; r++) x[r] = (uint32_t)r < n ? f[(size_t)r * a.V] : 0.0f;
    }
    const float* row = tile + lane * kBusPitch;
    for (uint32_t k = 0; k < K; k++) {
        const uint32_t s0 = a.tile_seg[g0 + k], n_seg = a.tile_seg[g0 + k + 1] - s0;
        if (n_seg == 0) continue;  // (wave-uniform)
        const int ord = (int)a.order[(size_t)(g0 + k) * 64u + (uint32_t)lane];
        const int my_end = (uint32_t)lane < n_seg ? (int)a.seg_end[s0 + (uint32_t)lane] : 0;
        const int my_dst = (uint32_t)lane < n_seg ? a.seg_dst[s0 + (uint32_t)lane] : 0;
        for (uint32_t c = 0; c < a.n_channels; c++) {
            if (a.channel_plane[c] != (int)plane) continue;  // (wave-uniform)
            const float g = a.gain[((size_t)k * a.n_channels + c) * a.V + v];
            __syncthreads();  // (one wave: the reads of the tile's last use before these writes)
#pragma unroll
            for (int r = 0; r < kBusRows; r++) tile[r * kBusPitch + lane] = __fmul_rn(g, x[r]);
            __syncthreads();  // (the writes before the reads)
            if ((uint32_t)lane < n) {
                int j = 0;
                for (uint32_t s = 0; s < n_seg; s++) {
                    const int end = __builtin_amdgcn_readlane(my_end, (int)s), dst = __builtin_amdgcn_readlane(my_dst, (int)s);
                    float sum = row[__builtin_amdgcn_readlane(ord, j)];
                    j++;
                    for (; j + 4 <= end; j += 4) {  // four reads in flight; the additions stay in order
                        const float x0 = row[__builtin_amdgcn_readlane(ord, j)], x1 = row[__builtin_amdgcn_readlane(ord, j + 1)];
                        const float x2 = row[__builtin_amdgcn_readlane(ord, j + 2)], x3 = row[__builtin_amdgcn_readlane(ord, j + 3)];
                        sum = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(sum, x0), x1), x2), x3);
                    }
                    for (; j < end; j++) sum = __fadd_rn(sum, row[__builtin_amdgcn_readlane(ord, j)]);
                    if (dst >= 0) a.part[((size_t)c * a.n_partials + (uint32_t)dst) * a.part_pitch + t0 + (uint32_t)lane] = sum;
                    else a.out[((size_t)(uint32_t)~dst * a.n_channels + c) * a.out_stride + t0 + (uint32_t)lane] = sum;
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void bus_slot_fold_sum(BusSlotFoldArgs a)
{
    const uint32_t n_tb = (a.T + 255u) / 256u;
    const uint32_t bc = blockIdx.x / n_tb, t = (blockIdx.x % n_tb) * 256u + threadIdx.x;  // bc = bus * channels + channel
    if (t >= a.T) return;
    const uint32_t b = bc / a.n_channels, c = bc % a.n_channels;
    const int cnt = a.channel_plane[c] < 0 ? 0 : a.bus_count[b];
    if (cnt < 0) return;  // its one segment went straight to the bus mix
    float s = 0.0f;
    if (cnt > 0) {
        const float* p = a.part + ((size_t)c * a.n_partials + a.bus_first[b]) * a.part_pitch + t;
        s = p[0];
        // A bus that many voices send to through a slot (an aux bus) has a row per tile: thousands, for a handful of (bus, channel)
        // pairs — few threads, each latency-bound.  32 loads in flight per thread; the additions stay in row order.
        int k = 1;
        for (; k + 32 <= cnt; k += 32) {
            float x[32];
#pragma unroll
            for (int i = 0; i < 32; i++) x[i] = p[(size_t)(k + i) * a.part_pitch];
#pragma unroll
            for (int i = 0; i < 32; i++) s = __fadd_rn(s, x[i]);
        }
        for (; k < cnt; k++) s = __fadd_rn(s, p[(size_t)k * a.part_pitch]);
    }
    a.out[(size_t)bc * a.out_stride + t] = s;
}

__global__ void fill_zero(float* p, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0.0f;
}

}  // namespace srack
