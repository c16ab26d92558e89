// master.hip.h — the master section (srack_buses_master): a gain per bus and channel, one stereo sum over the buses, its statistics.
//
//   master[c][t] = sum over the buses b of fl32(gain[b][c] * rows[b][c][t]),  c in {0, 1}
//
// IEEE f32, one rounding per operation (the unit is built with -ffp-contract=off), in an order that is part of the ABI and depends on
// n_buses alone (include/srack_hip.h): a RUN is ((+0.0f + p[64r]) + p[64r+1]) + ... over its up to 64 buses, a BLOCK +0.0f plus its up to
// 64 run sums, the master +0.0f plus the up to 16 block sums, each ascending.  Up to 64 buses that is MonoMixerModule's loop
// (mixer.rs:106-119: output.fill(0.0); *dst += src * gain).
//
//   master_runs   level 1.  Rows are time-minor, so a lane is a sample (or four neighbours: float4, when every row is 16-byte aligned)
//                 and a wave reads 256 contiguous bytes (1 KiB) of one row per instruction, then walks the run's rows channels *
//                 n_samples floats apart.  The add chain is serial per lane, so the row loads are issued in batches ahead of it.  One
//                 workgroup takes 256 lanes of one run and one channel: runs, channels and time all spread over the grid, so a call
//                 of 1 024 samples over 4 096 buses is still 512 waves of four samples a lane (2 048 of one).  The run sums go to the
//                 handle's scratch, f32 [n_runs][2][n_samples]: 1/64 of the input or less.
//   master_tree   levels 2 and 3.  A workgroup takes 64 samples of one channel, wave k block k: it adds the block's run sums in order
//                 (lane = sample, loads batched as above) and leaves the block sum in LDS; wave 0 adds the block sums in order and
//                 writes the master.
//   master_stats  the statistics of what the call wrote, f64 [2][SRACK_STAT_COUNT]: a second pass over [2][n_samples] by one workgroup.
//                 SUM and SUM_SQ are serial f64 chains in sample order (bit for bit the sequential loop, continued from the buffer):
//                 one wave per chain, 2 channels * 2 sums, each loading 64 samples at a time (a group ahead of the chain) and handing
//                 them along lane by lane (v_readlane: every lane carries the same sum).  Peaks and counts are order-free: per lane,
//                 then a wave reduction.  A non-finite sample enters the chains as -0.0, exactly as in stats_add (wave.hip.h).
// No floating-point atomics anywhere; every input byte is read once.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/srack_hip.h"
#include "launch_types.hpp"

namespace srack {

constexpr int kMasterRun = SRACK_MASTER_RUN;      // buses per run
constexpr int kMasterBlock = SRACK_MASTER_BLOCK;  // runs per block
constexpr int kMasterMaxBlocks = SRACK_MAX_BUSES / (SRACK_MASTER_RUN * SRACK_MASTER_BLOCK);
static_assert(kMasterMaxBlocks == 16, "master_tree takes a wave per block: at most 16 waves");
constexpr int kMasterThreads = 256;  // master_runs: lanes per workgroup

// kVec floats of one lane (1 or 4)
template <int kVec>
struct MasterLane {
    float v[kVec];
};
template <int kVec>
__device__ __forceinline__ MasterLane<kVec> master_load(const float* p)
{
    MasterLane<kVec> x;
    if constexpr (kVec == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        x.v[0] = q.x, x.v[1] = q.y, x.v[2] = q.z, x.v[3] = q.w;
    } else {
        x.v[0] = *p;
    }
    return x;
}
template <int kVec>
__device__ __forceinline__ void master_store(float* p, const MasterLane<kVec>& x)
{
    if constexpr (kVec == 4)
        *reinterpret_cast<float4*>(p) = make_float4(x.v[0], x.v[1], x.v[2], x.v[3]);
    else
        *p = x.v[0];
}

// grid (ceil(n / (256 * kVec)), n_runs, used).  kVec == 4 needs n % 4 == 0 and 16-byte aligned rows and runs (the launch decides).
template <int kVec, int kBatch>
__global__ __launch_bounds__(kMasterThreads) void master_runs(const MasterArgs a)
{
    const size_t t = ((size_t)blockIdx.x * kMasterThreads + threadIdx.x) * kVec;
    if (t >= a.n) return;
    const uint32_t r = blockIdx.y, c = blockIdx.z;
    const uint32_t b0 = r * kMasterRun;
    const uint32_t nb = min((uint32_t)kMasterRun, a.n_buses - b0);
    const size_t stride = (size_t)a.row_channels * a.n;
    const float* src = a.rows + ((size_t)b0 * a.row_channels + c) * a.n + t;
    const float* g = a.gain + (size_t)b0 * 2 + c;  // (wave-uniform: scalar loads)
    MasterLane<kVec> acc;
#pragma unroll
    for (int k = 0; k < kVec; k++) acc.v[k] = 0.0f;
    for (uint32_t i = 0; i < nb; i += kBatch) {
        MasterLane<kVec> x[kBatch];
        float gj[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; j++) {  // (a ragged last batch loads its last row again and leaves it out below)
            const uint32_t b = min(i + j, nb - 1);
            x[j] = master_load<kVec>(src + (size_t)b * stride);
            gj[j] = g[(size_t)b * 2];
        }
#pragma unroll
        for (int j = 0; j < kBatch; j++)
            if (i + j < nb) {
#pragma unroll
                for (int k = 0; k < kVec; k++) acc.v[k] = acc.v[k] + gj[j] * x[j].v[k];
            }
    }
    master_store<kVec>(a.runs + ((size_t)r * 2 + c) * a.n + t, acc);
}

// grid (ceil(n / 64), 2), block 64 * n_blocks.  A channel that is not summed (row_channels == 1: channel 1) is written +0.0f.
__global__ __launch_bounds__(64 * kMasterMaxBlocks) void master_tree(const MasterArgs a)
{
    __shared__ float s_block[kMasterMaxBlocks][64];
    constexpr int kBatch = 8;
    const uint32_t lane = threadIdx.x & 63u, k = threadIdx.x >> 6, c = blockIdx.y;
    const size_t t = (size_t)blockIdx.x * 64 + lane;
    const bool live = t < a.n;
    if (c >= a.used) {
        if (k == 0 && live) a.master[(size_t)c * a.n + t] = 0.0f;
        return;
    }
    const uint32_t n_runs = (a.n_buses + kMasterRun - 1) / kMasterRun;
    const uint32_t n_blocks = (n_runs + kMasterBlock - 1) / kMasterBlock;
    const uint32_t r0 = k * kMasterBlock;
    const uint32_t nr = min((uint32_t)kMasterBlock, n_runs - r0);
    float acc = 0.0f;
    if (live) {
        const float* src = a.runs + ((size_t)r0 * 2 + c) * a.n + t;
        const size_t stride = (size_t)2 * a.n;
        for (uint32_t i = 0; i < nr; i += kBatch) {
            float x[kBatch];
#pragma unroll
            for (int j = 0; j < kBatch; j++) x[j] = src[(size_t)min(i + j, nr - 1) * stride];
#pragma unroll
            for (int j = 0; j < kBatch; j++)
                if (i + j < nr) acc = acc + x[j];
        }
    }
    s_block[k][lane] = acc;
    __syncthreads();
    if (k == 0 && live) {
        float m = 0.0f;
        for (uint32_t j = 0; j < n_blocks; j++) m = m + s_block[j][lane];
        a.master[(size_t)c * a.n + t] = m;
    }
}

// one workgroup of 128 * used threads: wave w is channel w >> 1, chain w & 1 (0: SUM, and it carries the peaks and counts; 1: SUM_SQ)
__global__ __launch_bounds__(256) void master_stats(const MasterArgs a)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t c = w >> 1, kind = w & 1u;
    const float* x = a.master + (size_t)c * a.n;
    double* s = a.stats + (size_t)c * SRACK_STAT_COUNT;
    double chain = s[kind == 0 ? SRACK_STAT_SUM : SRACK_STAT_SUM_SQ];  // (every lane the same value)
    float peak_pos = (float)s[SRACK_STAT_PEAK_POS], peak_neg = (float)s[SRACK_STAT_PEAK_NEG];
    uint32_t nonfinite = 0, clipped = 0;
    const uint32_t n = a.n;
    // what a lane holds of the group at t0: its sample (past the end: 0, taking no part)
    auto load = [&](uint32_t t0) -> float { return lane < n - t0 ? x[t0 + lane] : 0.0f; };
    float cur = load(0);
    for (uint32_t t0 = 0; t0 < n; t0 += 64) {
        const uint32_t m = min(64u, n - t0);
        const float v = cur;
        if (t0 + 64 < n) cur = load(t0 + 64);  // the next group's load is in flight behind this group's chain
        const bool fin = __builtin_isfinite(v);
        if (lane < m) {
            if (fin) {
                peak_pos = v > peak_pos ? v : peak_pos;
                peak_neg = -v > peak_neg ? -v : peak_neg;
                clipped += fabsf(v) > 1.0f ? 1u : 0u;
            } else {
                nonfinite++;
            }
        }
        const int xi = __float_as_int(fin ? v : -0.0f);  // s + -0.0 == s for every s, and fma(-0.0, -0.0, q) == q for every q but -0.0
        if (m == 64) {
            if (kind == 0) {
#pragma unroll
                for (int i = 0; i < 64; i++) chain += (double)__int_as_float(__builtin_amdgcn_readlane(xi, i));
            } else {
#pragma unroll
                for (int i = 0; i < 64; i++) {
                    const double xd = (double)__int_as_float(__builtin_amdgcn_readlane(xi, i));
                    chain = __builtin_fma(xd, xd, chain);  // (the product is exact: fma and multiply-add agree)
                }
            }
        } else {
            for (uint32_t i = 0; i < m; i++) {
                const double xd = (double)__int_as_float(__builtin_amdgcn_readlane(xi, (int)i));
                chain = kind == 0 ? chain + xd : __builtin_fma(xd, xd, chain);
            }
        }
    }
    if (kind == 0) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            peak_pos = fmaxf(peak_pos, __shfl_xor(peak_pos, d));
            peak_neg = fmaxf(peak_neg, __shfl_xor(peak_neg, d));
            nonfinite += __shfl_xor(nonfinite, d);
            clipped += __shfl_xor(clipped, d);
        }
    }
    if (lane == 0) {
        if (kind == 0) {
            s[SRACK_STAT_SUM] = chain;
            s[SRACK_STAT_PEAK_POS] = (double)peak_pos;
            s[SRACK_STAT_PEAK_NEG] = (double)peak_neg;
            s[SRACK_STAT_NONFINITE] += (double)nonfinite;
            s[SRACK_STAT_CLIPPED] += (double)clipped;
        } else {
            s[SRACK_STAT_SUM_SQ] = chain;
        }
    }
}

}  // namespace srack
