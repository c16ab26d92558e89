// chain.hip — the chain family's own unit: render_ctl_gate_env, P1's control program as a kernel of its own (a kernel that is not a
// template cannot sit in a header three units include), and launch_fused, which picks the unit of the audio oscillator's port.
#include "fused.hip.h"
#include "launch.hpp"

namespace srack {

__global__ __launch_bounds__(64) void render_ctl_gate_env(CtlWork w)
{
    if (w.port & OSC_EXACT)
        ctl_gate_env<true>(w);
    else
        ctl_gate_env<false>(w);
}

void launch_ctl_gate_env(const CtlWork& w, hipStream_t st)
{
    hipLaunchKernelGGL(render_ctl_gate_env, dim3(1), dim3(64), 0, st, w);
}

void launch_fused(uint32_t osc_port, uint32_t vcf_port, bool exact, int out_mode, bool track, const KernelArgs& ka, const ChainRoles& roles, const CtlWork& co,
                  dim3 grid, hipStream_t st)
{
    with_osc_port(osc_port, [&](auto A) { launch_chain<decltype(A)::value>(vcf_port, exact, out_mode, track, ka, roles, co, grid, st); });
}

}  // namespace srack
