// bustile.hip.h — the lane-per-row tile of the bus console's stages whose recurrence is serial in time: bus_filter (busvcf.hip.h),
// bus_meter (busmeter.hip.h) and bus_osc (busosc.hip.h).  The skeleton the three kernels have in common is described here, once.
//
// Such a stage's only parallelism is across rows: a lane is a row, a wave 64 rows, a workgroup one wave — the few waves of a small
// console land on different CUs.  The rows are time-minor in memory, the lanes want them row-minor: a tile of 64 rows x 64 samples
// passes through LDS.  A kernel's tile loop is  fetch(0); per tile: turn, barrier, fetch the next tile, serial part, barrier, store,
// barrier.
//   fetch   row j of the tile as one 256-byte piece, lane l on sample t0 + l (whole lines each).  A lane past the end of the rows reads
//           the last sample again, and the kernel names for every j a row that exists: the loads are back to back, none under a mask,
//           none testing its row (notes/r19.md).  Tile i + 1's loads are issued before tile i's serial part and wait in registers: a
//           wave that is alone on its SIMD has nobody to hide them behind.
//   turn    pre[j] into LDS row j: word j * 65 + l.
//   serial  lane l reads row l, sample k: LDS word l * 65 + k.  The stride of 65 words puts the 32 lanes of a half-wave on 32 banks
//           (ds_read_b32 banks by word mod 32, 65 mod 32 = 1).  A chunk of kAhead samples is read ahead of the chunk being computed —
//           the last chunk reads itself again, so there is no branch — and what the stage writes goes back into the tile.  A whole
//           tile and a tail tile are two instances of the loop (run(std::true_type{}) / run(std::false_type{})): in a whole one no
//           sample asks whether it exists.
//   store   the tile the way it was fetched, row by row under lane < len and j < live.
// In place is safe: a tile is read completely before any of it is written, and the tile fetched ahead is disjoint from it.  Tails — a
// last tile of fewer than 64 samples, a last wave of fewer than 64 rows — are masked, never padded in memory; rows need no alignment
// beyond 4 bytes.  pre[] and the chunks live in registers, so a per-sample step must be inlined: one that went out of line, its state
// through scratch memory on every sample, was three to five times slower (notes/r32.md).
//
// What is code here is what the kernels can call and still compile to the instructions they had: the geometry, the 64-bit readlane,
// the fetch, the turn and the store.  The chunked read-ahead and the serial loop are a few lines in each kernel: as functions of this
// header they moved every kernel's instructions (notes/r33.md).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace srack {

constexpr int kRowTile = 64;                              // samples per tile, and rows per wave
constexpr int kRowTileStride = 65;                        // LDS words per tile row: odd, so that a column of 32 rows is 32 banks
constexpr int kRowTileWords = kRowTile * kRowTileStride;  // LDS words per tile

// A 64-bit value of lane `l` (wave-uniform), as a scalar: two v_readlane_b32, no memory access.
__device__ __forceinline__ uint64_t bustile_from_lane(uint64_t v, uint32_t l)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
    return ((uint64_t)hi << 32) | lo;
}

// The sample of the tile at t0 that `lane` fetches, of rows n long: its own, or the last one again.
__device__ __forceinline__ uint32_t bustile_sample(uint32_t lane, uint32_t n, uint32_t t0) { return min(lane, n - 1u - t0); }

// N rows of the tile at t0 into registers, tl being bustile_sample.  base(j): where row j begins, in floats, wave-uniform — out of
// lane j's registers (bustile_from_lane) or computed as a scalar.
template <int N, class Base>
__device__ __forceinline__ void bustile_fetch(float (&pre)[N], const float* rows, uint32_t t0, uint32_t tl, Base base)
{
#pragma unroll
    for (int j = 0; j < N; j++) pre[j] = (rows + base(j) + t0)[tl];
}

// pre[j] into row j of the tile at `s`.  No unroll pragma, here and in bustile_store, on purpose: a function's loop that is unrolled
// before the function is inlined reaches the kernel as 64 statements and moves the kernel's instructions (notes/r33.md); this one
// arrives as a loop and is unrolled in the kernel, with the kernel's own.  It has to be — pre[] is registers only when j is a
// constant —, and a kernel's scratch size in tools/kernel_meta.sh says whether it was.
template <int N>
__device__ __forceinline__ void bustile_turn(float* s, const float (&pre)[N], uint32_t lane)
{
    for (int j = 0; j < N; j++) s[j * kRowTileStride + lane] = pre[j];
}

// The first `live` rows' first `len` samples out of the tile at `s`, row j to out + base(j).
template <class Base>
__device__ __forceinline__ void bustile_store(float* out, const float* s, uint32_t t0, uint32_t lane, uint32_t len, uint32_t live, Base base)
{
    if (lane < len) {
        for (int j = 0; j < kRowTile; j++)
            if ((uint32_t)j < live) (out + base(j) + t0)[lane] = s[j * kRowTileStride + lane];
    }
}

}  // namespace srack
