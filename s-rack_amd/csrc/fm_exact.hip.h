// fm_exact.hip.h — the FM-pair instantiations that reach dev::osc_exact_cold (modules.hip.h), declared here and instantiated in
// interp.hip.  The optimiser shapes an out-of-line device function for the callers it sees in its translation unit: the time-parallel
// pair is the only one that asks osc_exact_cold for the sine alone, and a unit without that call drops the argument — and allocates
// the function's callers differently.  Its callers share one unit, the interpreter's, so that each is compiled as beside all the others.
#pragma once
#include "fm_block.hip.h"
#include "fm_pair.hip.h"

#ifndef SRK_FM_EXACT_HERE
#define SRK_FM_EXACT_HERE extern
#endif

namespace srack {

SRK_FM_EXACT_HERE template __global__ void render_fm_pair<true, 0>(KernelArgs, ChainRoles);
SRK_FM_EXACT_HERE template __global__ void render_fm_pair_ring<true, 0>(KernelArgs, ChainRoles);
SRK_FM_EXACT_HERE template __global__ void render_fm_pair_split<true, 0>(KernelArgs, ChainRoles);
SRK_FM_EXACT_HERE template __global__ void render_fm_pair_x<0>(KernelArgs, ChainRoles);
SRK_FM_EXACT_HERE template __global__ void render_fm_pair_x<1>(KernelArgs, ChainRoles);
SRK_FM_EXACT_HERE template __global__ void render_fm_pair_x<2>(KernelArgs, ChainRoles);
SRK_FM_EXACT_HERE template __global__ void render_fm_pair_x<3>(KernelArgs, ChainRoles);
SRK_FM_EXACT_HERE template __global__ void render_fm_pair_block_x<0>(KernelArgs, ChainRoles);
SRK_FM_EXACT_HERE template __global__ void render_fm_pair_block_x<1>(KernelArgs, ChainRoles);
SRK_FM_EXACT_HERE template __global__ void render_fm_pair_block_x<2>(KernelArgs, ChainRoles);
SRK_FM_EXACT_HERE template __global__ void render_fm_pair_block_x<3>(KernelArgs, ChainRoles);

}  // namespace srack
