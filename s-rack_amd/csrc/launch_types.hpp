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

// One srack_buses_send call (sends.hip.h).  The tables are made on the host when the sends are set (capi.cpp, sends_plan_make).
struct SendRun {
    uint32_t dst;        // the destination bus
    uint32_t first;      // its first term in the term table ...
    uint32_t count;      // ... and how many it has: 1 .. SRACK_MASTER_RUN
    int32_t srow;        // the scratch row the run sum goes to; < 0: the destination has this run only, the sum is its row of out
};
struct SendMulti {       // a destination of more than one run
    uint32_t dst;
    uint32_t first_row;  // its first scratch row
    uint32_t n_runs;
    uint32_t pad;
};
static_assert(sizeof(SendRun) == 16 && sizeof(SendMulti) == 16, "the host keeps both tables as four 32-bit words per entry (runtime.hpp)");
struct SendArgs {
    const float* rows;          // [n_buses][row_channels][n]
    float* out;                 // [n_buses][row_channels][n]
    float* scratch;             // [scratch rows][2][n]: the run sums of the destinations of several runs (the handle's)
    const uint32_t* term_src;   // [n_buses + n_sends] the terms in CSR order, a destination's through term first: source bus ...
    const float* term_gain;     // ... and gain pair [n_buses + n_sends][2]
    const SendRun* runs;        // [n_runs]
    const SendMulti* multi;     // [n_multi]
    uint32_t n;                 // samples
    uint32_t row_channels;
    uint32_t used;              // min(row_channels, 2): the channels that are mixed
    uint32_t n_runs;
    uint32_t n_multi;
    uint32_t max_blocks;        // the most blocks (of SRACK_MASTER_BLOCK runs) any destination has: send_tree's waves
};

// One srack_buses_filter call (busvcf.hip.h).  The row table is made on the host (render.hip, device_buses_filter): the (enabled bus,
// used channel) pairs compacted, 64 to a wave.
struct BusVcfRow {
    uint32_t row;        // the row of rows / out: bus * row_channels + channel
    uint32_t bus;        // its row of cv
    uint32_t slot;       // where its state lives: 2 * (the bus's place among the enabled ones) + channel
    uint32_t port;       // SRACK_VCF_OUT_*
    float freq, res, exp_amt;  // the bus's sliders, as given
    uint32_t pad;
};
static_assert(sizeof(BusVcfRow) == 32, "the host uploads the table as it stands");
constexpr int kBusVcfFields = 10;  // SRACK_BUS_FILTER_NSTATE: f, p, q, b0 .. b4, freq, res
struct BusVcfArgs {
    const float* rows;          // [n_buses][row_channels][n]
    const float* cv;            // [n_buses][n] or null
    float* out;                 // [n_buses][row_channels][n]; may be rows itself
    float* state;               // [slots / 64][kBusVcfFields][64]: a wave's 64 slots side by side per field
    const BusVcfRow* tab;       // [n_rows]
    const uint32_t* copy_rows;  // [n_copy] rows of the disabled buses' used channels, copied when out is not rows
    uint32_t n;                 // samples
    uint32_t n_rows;
    uint32_t n_copy;
    uint32_t used;              // min(row_channels, 2): table entries that share a bus, and a row of cv
};

// One srack_buses_vca call (busvca.hip.h).  The table has an entry per bus, in bus order: nothing is compacted, a workgroup takes 64
// buses as they lie.
struct BusVcaBus {
    float a_sec, d_sec, s_val, r_sec;  // the bus's ADSR sliders, as given
    uint32_t mode;                     // SRACK_BUS_VCA_OFF / _CV / _GATE
    uint32_t negative;                 // the VCAs' flag
    uint32_t pad[2];
};
static_assert(sizeof(BusVcaBus) == 32, "the host uploads the table as it stands");
constexpr int kBusVcaFields = 6;  // SRACK_BUS_VCA_NSTATE: phase, mode, r_val, from_a_val, sample rate, gate_last
struct BusVcaArgs {
    const float* rows;          // [n_buses][row_channels][n]
    const float* ctl;           // [n_buses][n] or null
    float* out;                 // [n_buses][row_channels][n]; may be rows itself
    float* env;                 // [n_buses][n] or null
    float* state;               // [kBusVcaFields][n_buses], every value an f32 as the C ABI hands it out
    const BusVcaBus* tab;       // [n_buses]
    float rate;                 // the f32 sample rate a fresh ADSRModule of the patch carries
    uint32_t n;                 // samples
    uint32_t n_buses;
    uint32_t row_channels;
    uint32_t used;              // min(row_channels, 2): the channels that are processed
};

// One srack_buses_osc call (busosc.hip.h).  The table has an entry per enabled bus, ordered by (port, antialiasing) and then by bus, so
// that a wave's 64 lanes share a class wherever they can; behind it lies the list of the disabled buses, whose rows are zeroed.
struct BusOscBus {
    double delta;        // the increment without a CV row: 440 * 2^f64(val) / f64(sample rate), the host libm's pow
    double val;          // f64(val), for the increment with a CV row
    float depth, offset; // the two Math constants, as given
    uint32_t bus;        // its row of cv, sync and out, and its place in the state
    uint32_t flags;      // one of OSC_OUT_SINE / _SQUARE / _SAW, and OSC_AA (program.hpp)
};
static_assert(sizeof(BusOscBus) == 32, "the host uploads the table as it stands");
constexpr int kBusOscFields = 2;  // SRACK_BUS_OSC_NSTATE: pos, sync_last
struct BusOscArgs {
    const float* cv;            // [n_buses][n] or null: the CV port is unconnected
    const float* sync;          // [n_buses][n] or null: the Sync port is unconnected
    float* out;                 // [n_buses][n]
    double* state;              // [kBusOscFields][n_buses]: pos, then last as 0.0 / 1.0
    const BusOscBus* tab;       // [n_on]
    const uint32_t* off;        // [n_off] the disabled buses
    double sr;                  // f64(sample rate)
    uint32_t n;                 // samples
    uint32_t n_buses;
    uint32_t n_on;
    uint32_t n_off;
};

// One srack_buses_shaper call (busshape.hip.h).  The table has an entry per bus, in bus order; behind it lies the list of the buses
// that are not OFF, which an in-place call works through (an out-of-place one takes every bus: an OFF bus is a copy).
struct BusShaperBus {
    float pre, exponent, post;  // the bus's three constants, as given
    uint32_t mode;              // SRACK_BUS_SHAPER_OFF / _CONST / _CV
};
static_assert(sizeof(BusShaperBus) == 16, "the host uploads the table as it stands");
constexpr uint32_t kBusShaperStretch = 1024;  // samples of one bus a wave takes
struct BusShaperArgs {
    const float* rows;          // [n_buses][row_channels][n]
    const float* cv;            // [n_buses][n] or null
    float* out;                 // [n_buses][row_channels][n]; may be rows itself
    const BusShaperBus* tab;    // [n_buses]
    const uint32_t* list;       // [n_work] the buses to work on; null: buses 0 .. n_work - 1
    uint32_t n;                 // samples
    uint32_t n_work;            // buses this call works on
    uint32_t n_stretches;       // ceil(n / kBusShaperStretch): the stretches of a bus
    uint32_t n_units;           // n_work * n_stretches: a wave each
    uint32_t row_channels;
    uint32_t used;              // min(row_channels, 2): the channels that are processed
};

// One srack_buses_meter call (busmeter.hip.h).  A read-only tap: rows in, records and totals continued where they stand.
struct BusMeterArgs {
    const float* rows;          // [n_buses][row_channels][n]
    double* levels;             // [n_windows][SRACK_STAT_COUNT][n_buses][2] or null
    double* totals;             // [SRACK_STAT_COUNT][n_buses][2] or null
    uint64_t first;             // the stream position of sample 0 (levels only)
    uint32_t window;            // samples per record (levels only)
    uint32_t n;                 // samples
    uint32_t n_buses;
    uint32_t row_channels;
    uint32_t used;              // min(row_channels, 2): the channels that are metered
};

}  // namespace srack
