// sends.hip.h — the bus sends (srack_buses_send): aux sends from bus to bus, one gather-sum per destination bus.
//
//   out[d][c][t] = the master's tree over the terms of d:  p_k = fl32(g_k[c] * rows[src_k][c][t]),  c in {0, 1}
//
// Term 0 of a destination is its own row times its through gain, the others are the sends that name it, in the order of the host's
// list (include/srack_hip.h).  IEEE f32, one rounding per operation (the unit is built with -ffp-contract=off), in the master section's
// order: a RUN is ((+0.0f + p[64r]) + p[64r+1]) + ... over its up to 64 terms, a BLOCK +0.0f plus its up to 64 run sums, the result
// +0.0f plus the up to 16 block sums, each ascending.  The order depends on the send list alone.  Up to 64 terms that is
// MonoMixerModule's loop (mixer.rs:106-119: output.fill(0.0); *dst += src * gain).
//
// The host lays the list out when it is set (capi.cpp, sends_plan_make): the terms in CSR order (source bus and gain pair per term, a
// destination's through term first), and a run table — destination, first term, term count, target.
//
//   send_runs   level 1: master_runs with an indirection.  A lane is a sample (or four neighbours: float4, when rows and out are
//               16-byte aligned and n % 4 == 0), a workgroup 256 lanes of one run and one channel.  The run's source indices and gains
//               are wave-uniform (scalar loads, issued with each batch); the row loads are issued a batch ahead of the add chain,
//               which is serial per lane.  A ragged last batch loads what it has and no more: most destinations of a real table are
//               through-only, one term, and must cost one row load.  A destination of one run is written straight to its row of
//               out — a run sum is never -0.0, so levels 2 and 3 would change no bit —, the runs of any other go to the handle's
//               scratch, f32 [scratch rows][2][n].
//   send_tree   levels 2 and 3 for the destinations of more than one run: master_tree over (time, destination, channel).  Wave k adds
//               block k's run sums in order, the block sums meet in LDS, wave 0 adds them in order and writes the row of out.
// No floating-point atomics; every output float is written once, by a plain vector store; rows is only read, out only written.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/srack_hip.h"
#include "launch_types.hpp"

namespace srack {

// (master.hip.h defines kernels that are not templates: a second unit cannot include it, so the lane helpers have twins here)
constexpr int kSendBlock = SRACK_MASTER_BLOCK;  // runs per block
constexpr int kSendMaxBlocks = 65536 / (SRACK_MASTER_RUN * SRACK_MASTER_BLOCK);  // a destination's 65 536 terms
static_assert(kSendMaxBlocks == 16, "send_tree takes a wave per block: at most 16 waves");

// kVec floats of one lane (1 or 4)
template <int kVec>
struct SendLane {
    float v[kVec];
};
template <int kVec>
__device__ __forceinline__ SendLane<kVec> send_load(const float* p)
{
    SendLane<kVec> x;
    if constexpr (kVec == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        x.v[0] = q.x, x.v[1] = q.y, x.v[2] = q.z, x.v[3] = q.w;
    } else {
        x.v[0] = *p;
    }
    return x;
}
template <int kVec>
__device__ __forceinline__ void send_store(float* p, const SendLane<kVec>& x)
{
    if constexpr (kVec == 4)
        *reinterpret_cast<float4*>(p) = make_float4(x.v[0], x.v[1], x.v[2], x.v[3]);
    else
        *p = x.v[0];
}

constexpr int kSendThreads = 256;  // send_runs: lanes per workgroup
// Runs outnumber the buses (65 536 of them, and 1 048 576 sends): more than a grid's y holds.  The runs go over y and z.
constexpr uint32_t kSendGridY = 32768;

// grid (ceil(n / (256 * kVec)), min(n_runs, kSendGridY), used * ceil(n_runs / kSendGridY)).  kVec == 4 needs n % 4 == 0 and 16-byte
// aligned rows, out and scratch (the launch decides).
template <int kVec, int kBatch>
__global__ __launch_bounds__(kSendThreads) void send_runs(const SendArgs a)
{
    const size_t t = ((size_t)blockIdx.x * kSendThreads + threadIdx.x) * kVec;
    const uint32_t c = blockIdx.z % a.used;
    const uint32_t r = (blockIdx.z / a.used) * kSendGridY + blockIdx.y;
    if (r >= a.n_runs || t >= a.n) return;
    const SendRun run = a.runs[r];  // (wave-uniform, like everything read through ts and tg: scalar loads)
    const uint32_t* ts = a.term_src + run.first;
    const float* tg = a.term_gain + (size_t)run.first * 2 + c;
    const size_t stride = (size_t)a.row_channels * a.n;
    const float* src = a.rows + (size_t)c * a.n + t;
    SendLane<kVec> acc;
#pragma unroll
    for (int k = 0; k < kVec; k++) acc.v[k] = 0.0f;
    uint32_t i = 0;
    for (; i + kBatch <= run.count; i += kBatch) {
        SendLane<kVec> x[kBatch];
        float gj[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; j++) {
            x[j] = send_load<kVec>(src + (size_t)ts[i + j] * stride);
            gj[j] = tg[(size_t)(i + j) * 2];
        }
#pragma unroll
        for (int j = 0; j < kBatch; j++) {
#pragma unroll
            for (int k = 0; k < kVec; k++) acc.v[k] = acc.v[k] + gj[j] * x[j].v[k];
        }
    }
    if (i < run.count) {  // the ragged batch: its m < kBatch loads (the conditions are wave-uniform), then its m links of the chain
        const uint32_t m = run.count - i;
        SendLane<kVec> x[kBatch];
        float gj[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; j++) {
#pragma unroll
            for (int k = 0; k < kVec; k++) x[j].v[k] = 0.0f;
            gj[j] = 0.0f;
            if ((uint32_t)j < m) {
                x[j] = send_load<kVec>(src + (size_t)ts[i + j] * stride);
                gj[j] = tg[(size_t)(i + j) * 2];
            }
        }
#pragma unroll
        for (int j = 0; j < kBatch; j++)
            if ((uint32_t)j < m) {
#pragma unroll
                for (int k = 0; k < kVec; k++) acc.v[k] = acc.v[k] + gj[j] * x[j].v[k];
            }
    }
    float* to = run.srow < 0 ? a.out + ((size_t)run.dst * a.row_channels + c) * a.n + t : a.scratch + ((size_t)run.srow * 2 + c) * a.n + t;
    send_store<kVec>(to, acc);
}

// grid (ceil(n / 64), n_multi, used), block 64 * max_blocks (the most blocks any destination has; a wave past its destination's
// blocks brings +0.0f to LDS, which nobody reads)
__global__ __launch_bounds__(64 * kSendMaxBlocks) void send_tree(const SendArgs a)
{
    __shared__ float s_block[kSendMaxBlocks][64];
    constexpr int kBatch = 8;
    const uint32_t lane = threadIdx.x & 63u, k = threadIdx.x >> 6, c = blockIdx.z;
    const SendMulti d = a.multi[blockIdx.y];
    const size_t t = (size_t)blockIdx.x * 64 + lane;
    const bool live = t < a.n;
    const uint32_t n_blocks = (d.n_runs + kSendBlock - 1) / kSendBlock;
    float acc = 0.0f;
    if (live && k < n_blocks) {
        const uint32_t r0 = k * kSendBlock;
        const uint32_t nr = min((uint32_t)kSendBlock, d.n_runs - r0);
        const float* src = a.scratch + ((size_t)(d.first_row + r0) * 2 + c) * a.n + t;
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
        a.out[((size_t)d.dst * a.row_channels + c) * a.n + t] = m;
    }
}

}  // namespace srack
