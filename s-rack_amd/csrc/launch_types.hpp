// launch_types.hpp — the few types and constants the kernels and the launch code (launch.hpp, render.hip) both see.  Kept apart from
// launch.hpp so that a changed launch signature recompiles no kernel.
#pragma once
#include <cstdint>

#include "kernel_args.hip.h"

namespace srack {

// What the fused gate -> envelope control block (fused.hip.h) needs: a slice of KernelArgs small enough to ride along with a voice kernel's arguments.
struct CtlWork {
    const DevOp* ops;
    uint32_t* table;   // the control program's one-voice table
    float* track;      // this chunk's first sample of the envelope track
    uint32_t T;        // samples to produce (0: nothing to do)
    uint32_t port;     // OSC_OUT_* of the gate oscillator, | OSC_EXACT in the exact render mode
    uint32_t* table_out;  // where the state goes (a tick session, render.hip: another copy of the table; null: in place) ...
    uint32_t n_rows;      // ... and how many rows the table has
};

// The time-parallel FM pairs' launch shape (fm_block.hip.h): pick_kernel needs it for the voices per workgroup and the shortest ring.
constexpr int kBlkVoices = 32, kBlkSlices = 16, kBlkPer = 16, kBlkChunk = kBlkSlices * kBlkPer;  // 256 samples per chunk

// One srack_buses_master call (master.hip.h).
struct MasterArgs {
    const float* rows;   // [n_buses][row_channels][n]
    const float* gain;   // [n_buses][2]
    float* runs;         // [n_runs][2][n]: the run sums (the handle's scratch)
    float* master;       // [2][n]
    double* stats;       // [2][SRACK_STAT_COUNT] or null
    uint32_t n;          // samples
    uint32_t n_buses;
    uint32_t row_channels;
    uint32_t used;       // min(row_channels, 2): the channels that are summed
};

}  // namespace srack
