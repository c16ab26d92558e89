// busvcf.hip.h — the bus filters (srack_buses_filter): a Moog ladder per (enabled bus, channel) row, behind the mixer.
//
// A row is one MoogFilterModule (filter.rs:182-221): audio in rows[bus][c][t], CV in cv[bus][t] (or 0.0f), the chosen port out.  The
// ladder is a non-linear recurrence, strictly serial in time, so the only parallelism is across rows: a lane is a row, a wave 64 rows,
// a workgroup one wave — the few waves of a small console land on different CUs.  The arithmetic is modules.hip.h's literal ladder
// (vcf_frequency, vcf_resonance, vcf_coeffs<false>, vcf_run<false>; the unit is built with -ffp-contract=off): the reference's f32
// operations one by one.
//
// The rows are time-minor in memory, the lanes want them row-minor: a tile of 64 rows x 64 samples passes through LDS.
//   load    row j of the tile as one 256-byte piece, lane l on sample t0 + l (64 loads per lane and tile, whole lines each); the CV rows of
//           the wave's buses the same way.  Tile i + 1's loads are issued before tile i's serial loop and wait in registers: a wave that
//           is alone on its SIMD has nobody to hide them behind.
//   run     lane l reads row l, sample k: LDS word l * 65 + k.  The stride of 65 words puts the 32 lanes of a half-wave on 32 banks
//           (ds_read_b32 banks by word mod 32, 65 mod 32 = 1).  Eight samples are read ahead of the eight being computed; the results go
//           back into the tile.
//   store   the tile the way it was loaded.
// In place (out == rows) is safe: a tile is read completely before any of it is written, and the tile loaded ahead is disjoint from it.
// Tails — a last tile of fewer than 64 samples, a last wave of fewer than 64 rows — are masked, never padded in memory; rows need no
// alignment beyond 4 bytes.  The state stays in registers across the tiles of a call and is loaded and stored once per call, from a
// layout in which a wave's 64 slots lie side by side per field.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "launch_types.hpp"
#include "modules.hip.h"

namespace srack {

constexpr int kBusVcfTile = 64;     // samples per tile (and rows per wave)
constexpr int kBusVcfStride = 65;   // LDS words per tile row: odd, so that a column of 32 rows is 32 banks
constexpr int kBusVcfAhead = 8;     // samples a lane reads from LDS at a time
constexpr int kBusVcfCopyThreads = 256;
static_assert(kBusVcfFields == SRACK_BUS_FILTER_NSTATE && sizeof(dev::VcfRegs) == sizeof(float) * kBusVcfFields, "the state is VcfRegs field by field, as the C ABI hands it out");

// A 64-bit value of lane `l` (wave-uniform), as a scalar: two v_readlane_b32, no memory access.
__device__ __forceinline__ uint64_t busvcf_from_lane(uint64_t v, uint32_t l)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
    return ((uint64_t)hi << 32) | lo;
}

// grid (ceil(n_rows / 64)), block 64.  kCv: a.cv is given.  kUsed: a.used, 1 or 2 — the table entries that share a bus and a row of cv.
template <bool kCv, int kUsed>
__global__ __launch_bounds__(64) void bus_filter(const BusVcfArgs a)
{
    using namespace dev;
    constexpr int kCvRows = kBusVcfTile / kUsed;
    __shared__ float s_x[kBusVcfTile * kBusVcfStride];
    __shared__ float s_cv[kCv ? kCvRows * kBusVcfStride : 1];
    const uint32_t lane = threadIdx.x;
    const uint32_t r0 = blockIdx.x * 64u;
    const uint32_t live = min(64u, a.n_rows - r0);         // rows of this wave (wave-uniform)
    const bool on = lane < live;
    // A lane past the last row takes row 0's entry: it runs that filter on zeros and stores nothing, and — every lane holding a row that
    // exists — the tile's loads need no test of the row: row j's place comes out of lane j's registers, past the last row another read of
    // row 0.
    const BusVcfRow me = a.tab[r0 + (on ? lane : 0u)];
    const uint64_t my_x = (uint64_t)me.row * a.n, my_cv = (uint64_t)me.bus * a.n;   // in floats
    const uint32_t cv_at = (lane / kUsed) * kBusVcfStride;
    const uint32_t x_at = lane * kBusVcfStride;

    float* st = a.state + (size_t)(me.slot >> 6) * (kBusVcfFields * 64) + (me.slot & 63u);
    VcfRegs s;
    s.f = st[0 * 64], s.p = st[1 * 64], s.q = st[2 * 64];
    s.b0 = st[3 * 64], s.b1 = st[4 * 64], s.b2 = st[5 * 64], s.b3 = st[6 * 64], s.b4 = st[7 * 64];
    s.freq = st[8 * 64], s.res = st[9 * 64];
    bool fin = vcf_nan_free(s);
    const float res = vcf_resonance(me.res);

    float pre[kBusVcfTile];                  // the tile loaded ahead: row j, sample t0 + lane
    float cpre[kCv ? kCvRows : 1];
    // (a lane past the end of the rows reads the last sample again: 64 loads back to back, none of them under a mask)
    auto fetch = [&](uint32_t t0) {
        const uint32_t tl = min(lane, a.n - 1u - t0);
#pragma unroll
        for (int j = 0; j < kBusVcfTile; j++) pre[j] = (a.rows + busvcf_from_lane(my_x, j) + t0)[tl];
        if constexpr (kCv) {
#pragma unroll
            for (int j = 0; j < kCvRows; j++) cpre[j] = (a.cv + busvcf_from_lane(my_cv, j * kUsed) + t0)[tl];
        }
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

    const uint32_t n_tiles = (a.n + kBusVcfTile - 1) / kBusVcfTile;
    fetch(0);
    for (uint32_t i = 0; i < n_tiles; i++) {
        const uint32_t t0 = i * kBusVcfTile;
        const uint32_t len = min((uint32_t)kBusVcfTile, a.n - t0);
#pragma unroll
        for (int j = 0; j < kBusVcfTile; j++) s_x[j * kBusVcfStride + lane] = pre[j];
        if constexpr (kCv) {
#pragma unroll
            for (int j = 0; j < kCvRows; j++) s_cv[j * kBusVcfStride + lane] = cpre[j];
        }
        __syncthreads();
        if (i + 1 < n_tiles) fetch(t0 + kBusVcfTile);

        // the serial part: eight samples are read out of the tile ahead of the eight being computed (kFull: a whole tile, no sample asks
        // whether it exists)
        auto run = [&](auto full) {
            constexpr bool kFull = decltype(full)::value;
            float x[kBusVcfAhead], c[kBusVcfAhead];
            read8(0, x, c);
            for (uint32_t k0 = 0; k0 < (kFull ? (uint32_t)kBusVcfTile : len); k0 += kBusVcfAhead) {
                float xn[kBusVcfAhead], cn[kBusVcfAhead];
                read8(min(k0 + kBusVcfAhead, (uint32_t)(kBusVcfTile - kBusVcfAhead)), xn, cn);  // (the last chunk reads itself again: no branch)
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
        if (len == (uint32_t)kBusVcfTile)
            run(std::true_type{});
        else
            run(std::false_type{});
        __syncthreads();
        if (lane < len) {
#pragma unroll
            for (int j = 0; j < kBusVcfTile; j++)
                if ((uint32_t)j < live) (a.out + busvcf_from_lane(my_x, j) + t0)[lane] = s_x[j * kBusVcfStride + lane];
        }
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
