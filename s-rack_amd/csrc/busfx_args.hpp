// busfx_args.hpp — what the bus reverbs' kernel (busfx.hip.h) and the host side that fills it in (console.cpp) both see: the table entry
// of a bus and the argument block of one srack_buses_reverb call.  No kernel is visible here.
#pragma once
#include <cstdint>

#include "program.hpp"

namespace srack {

struct BusFxDev {    // one bus, on the device
    double* state;   // [kFvStates + sum of line lengths]; null: the bus has no reverb
    double par[7];   // comb feedback, comb dampening, 1 - dampening, wet_gains.0, wet_gains.1, dry, input_gain (freeverb_params.hpp)
};

struct BusFxArgs {
    const float* in;       // [n_buses][channels][n]
    float* out;            // [n_buses][2][n]
    const BusFxDev* tab;   // [n_buses]
    uint32_t n, channels;
    uint32_t block;        // T: 1 <= T <= min(kBusFxThreads, shortest line)
    uint32_t len[kFvLines], first[kFvLines];
    uint32_t pos[kFvLines];  // slot of the call's first sample in each line: samples since the last reset mod length
};

}  // namespace srack
