// busfx.hip.h — the bus reverbs (srack_buses_reverb): one stereo Freeverb per mix bus, behind the mixer, time-parallel on the device.
//
// What is computed is the freeverb crate's Freeverb::tick as restated for OP_FREEVERB (interp.hip.h, tile_freeverb), f64, one rounding
// per operation, in the same order:
//   x = (in0 + in1) * 0.015 * input_gain
//   comb:    out = line.read(); state = out * (1 - damp) + state * damp; line.write(x + state * feedback)     o += out, from 0.0, comb order
//   allpass: d = line.read(); out = -in + d; line.write(in + d * 0.5)                                        four in series
//   fx0 = o0 * wet0 + o1 * wet1 + in0 * dry        fx1 = o1 * wet0 + o0 * wet1 + in1 * dry
//
// tile_freeverb has one LANE per reverb and is a chain of memory round trips: right for 262 144 voices, hopeless for a handful of
// buses.  Here a reverb has a WORKGROUP, and the parallelism is in time: a line is read `length` samples after it was written, so
// within a block of T <= shortest line samples every read of every line is of data written before the block.  Everything is then
// parallel over the block's samples except the combs' one-pole, `state = out * (1 - damp) + state * damp`: 16 independent scans of two
// dependent f64 operations per step.  Per block:
//   A  thread t: x[t]; the 16 comb lines' slots of sample t, coalesced, into registers (for the comb sums) and into LDS (for the scans)
//   B  lanes 0..15 of wave 0: the 16 scans out of LDS; they leave what goes back into the lines there
//   C  thread t: the combs' write-backs to the lines, the two comb sums, the four allpass stages straight from and to the lines,
//      the wet / dry gains, fx
// A slot index wraps inside a block (pos + t >= length, per element).  Block k's stores (C) are read by OTHER threads in block k + 1 (A
// and C): a workgroup-scope fence and a barrier stand between the blocks; nothing of a block is fetched ahead of it.
// State per bus: 16 filter states, then the 24 lines back to back, f64, in HBM (L2-resident while a call runs), allocated for enabled
// buses only.  A bus without a reverb is a copy of the bus mix's channels 0 and 1.
#pragma once
#include <hip/hip_runtime.h>

#include "busfx_args.hpp"
#include "program.hpp"

namespace srack {

constexpr int kBusFxThreads = 256;  // = the longest block: one sample per thread
// doubles between two comb rows in LDS: lane j of the scans reads row j, 8 bytes wide (bank = dword address mod 64): a pitch of
// 2 (mod 32) doubles puts the 16 rows 4 banks apart — conflict-free; the threads' column accesses are consecutive doubles
constexpr int kBusFxPitch = 258;
constexpr int kBusFxScan = 8;       // scan steps whose LDS reads are issued together

__global__ __launch_bounds__(kBusFxThreads) void bus_reverb(const BusFxArgs a)
{
    __shared__ double s_line[kFvStates * kBusFxPitch];
    __shared__ double s_x[kBusFxThreads];
    const uint32_t b = blockIdx.x, t = threadIdx.x, n = a.n;
    const BusFxDev* e = a.tab + b;
    double* const state = e->state;
    const float* const in0 = a.in + (size_t)b * a.channels * n;
    const float* const in1 = a.channels > 1 ? in0 + n : nullptr;  // one channel: the module with Right unconnected
    float* const out0 = a.out + (size_t)b * 2 * n;
    float* const out1 = out0 + n;
    if (!state) {
        for (uint32_t i = t; i < n; i += kBusFxThreads) {
            out0[i] = in0[i];
            out1[i] = in1 ? in1[i] : 0.0f;
        }
        return;
    }
    const double feedback = e->par[0], damp = e->par[1], damp_inv = e->par[2], wet0 = e->par[3], wet1 = e->par[4], dry = e->par[5], gain = e->par[6];
    double* const lines = state + kFvStates;
    uint32_t base[kFvLines];  // slot of the block's first sample, per line (the same in every thread)
#pragma unroll
    for (int j = 0; j < kFvLines; j++) base[j] = a.pos[j];
    // where line j keeps sample t of the block: base < length and t < T <= length, so one subtraction wraps
    auto slot = [&](int j) {
        uint32_t s = base[j] + t;
        if (s >= a.len[j]) s -= a.len[j];
        return a.first[j] + s;
    };
    double fs = t < (uint32_t)kFvStates ? state[t] : 0.0;  // lane j < 16 of wave 0 carries comb line j's filter state through the call
    for (uint32_t t0 = 0; t0 < n; t0 += a.block) {
        const uint32_t m = min(a.block, n - t0);
        const bool on = t < m;
        float l = 0.0f, r = 0.0f;
        double out[kFvStates];
#pragma unroll
        for (int j = 0; j < kFvStates; j++) out[j] = 0.0;
        if (on) {  // A
            l = in0[t0 + t];
            r = in1 ? in1[t0 + t] : 0.0f;
            s_x[t] = ((double)l + (double)r) * 0.015 * gain;
#pragma unroll
            for (int j = 0; j < kFvStates; j++) {
                out[j] = lines[slot(j)];
                s_line[j * kBusFxPitch + t] = out[j];
            }
        }
        __syncthreads();
        if (t < (uint32_t)kFvStates) {  // B (a short last group reads past m, inside the row: unused)
            double* const row = s_line + t * kBusFxPitch;
            for (uint32_t i0 = 0; i0 < m; i0 += kBusFxScan) {
                double o[kBusFxScan], x[kBusFxScan];
#pragma unroll
                for (int k = 0; k < kBusFxScan; k++) {
                    o[k] = row[i0 + k];
                    x[k] = s_x[i0 + k];
                }
#pragma unroll
                for (int k = 0; k < kBusFxScan; k++)
                    if (i0 + k < m) {
                        fs = o[k] * damp_inv + fs * damp;
                        row[i0 + k] = x[k] + fs * feedback;
                    }
            }
        }
        __syncthreads();
        if (on) {  // C
            uint32_t at[8];
            double d[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {  // (the allpass reads do not wait for the chain below)
                at[k] = slot(kFvStates + k);
                d[k] = lines[at[k]];
            }
#pragma unroll
            for (int j = 0; j < kFvStates; j++) lines[slot(j)] = s_line[j * kBusFxPitch + t];
            double o0 = 0.0, o1 = 0.0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                o0 += out[2 * k];
                o1 += out[2 * k + 1];
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const double i0 = o0, i1 = o1;
                o0 = -i0 + d[2 * k];
                o1 = -i1 + d[2 * k + 1];
                lines[at[2 * k]] = i0 + d[2 * k] * 0.5;
                lines[at[2 * k + 1]] = i1 + d[2 * k + 1] * 0.5;
            }
            out0[t0 + t] = (float)(o0 * wet0 + o1 * wet1 + (double)l * dry);
            out1[t0 + t] = (float)(o1 * wet0 + o0 * wet1 + (double)r * dry);
        }
#pragma unroll
        for (int j = 0; j < kFvLines; j++) {  // m <= T <= length: one subtraction wraps
            base[j] += m;
            if (base[j] >= a.len[j]) base[j] -= a.len[j];
        }
        __threadfence_block();  // this block's stores to the lines, before any thread's loads of the next
        __syncthreads();
    }
    if (t < (uint32_t)kFvStates) state[t] = fs;
}

}  // namespace srack
