// chain_unit.hip.h — the chain family's launch ladder for ONE audio oscillator port: launch_chain<port> (declared in launch.hpp).
// chain_saw.hip, chain_square.hip and chain_sine.hip include this and instantiate it explicitly, which is what puts that port's 21
// render_voice_chain and 24 render_voice_chain_track kernels into their translation unit.
#pragma once
#include "fused.hip.h"
#include "launch.hpp"

namespace srack {

template <uint32_t A, uint32_t F, bool E, int O>
static void launch_fused4(bool track, const KernelArgs& ka, const ChainRoles& roles, const CtlWork& co, dim3 grid, hipStream_t st)
{
    if (track)
        hipLaunchKernelGGL((render_voice_chain_track<A, F, E, O>), grid, dim3(64), 0, st, ka, roles, co);
    else
        hipLaunchKernelGGL((render_voice_chain<A, OSC_OUT_SQUARE, F, E, O>), grid, dim3(64), 0, st, ka, roles);
}

template <uint32_t A, uint32_t F>
static void launch_fused3(bool exact, int out_mode, bool track, const KernelArgs& ka, const ChainRoles& roles, const CtlWork& co, dim3 grid, hipStream_t st)
{
    if ((out_mode & kOutStats) && exact)  // per-voice statistics (wave.hip.h): one instantiation per flavour, frames and mix decided at run time
        launch_fused4<A, F, true, kOutStats>(track, ka, roles, co, grid, st);
    else if (out_mode & kOutStats)
        launch_fused4<A, F, false, kOutStats>(track, ka, roles, co, grid, st);
    else if (exact && out_mode == 3 && track)  // frames + mix, the usual request, also gets the compile-time output mode in exact mode
        hipLaunchKernelGGL((render_voice_chain_track<A, F, true, 3>), grid, dim3(64), 0, st, ka, roles, co);
    else if (exact)  // otherwise one instantiation, output mode decided at run time
        launch_fused4<A, F, true, 0>(track, ka, roles, co, grid, st);
    else
        with_out_mode(out_mode, [&](auto O) { launch_fused4<A, F, false, O>(track, ka, roles, co, grid, st); });
}

template <uint32_t kOscAPort>
void launch_chain(uint32_t vcf_port, bool exact, int out_mode, bool track, const KernelArgs& ka, const ChainRoles& roles, const CtlWork& co, dim3 grid, hipStream_t st)
{
#ifdef SRK_WAVE_CENSUS
    // (a failure is the launch's: the caller asks hipGetLastError behind it)
    if (track) (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(srk_census_rec), census_rec, sizeof(*census_rec), 0, hipMemcpyHostToDevice, st);
#endif
    with_port<VCF_OUT_LP, VCF_OUT_BP, VCF_OUT_HP>(vcf_port, [&](auto F) { launch_fused3<kOscAPort, F>(exact, out_mode, track, ka, roles, co, grid, st); });
}

}  // namespace srack
